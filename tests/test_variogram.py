"""The variogram score's fused route without a device: the float64 restatement (tests/variogram_cases.py) against the host route
and the oracle's full tables, the rule that any non-finite input makes a point NaN, the case generator's promises, the C ABI's
declaration against the bindings, the gating of metrics.multivariate (every condition keeps the host route, and without a device
nothing is asked of one), and the README row."""
import os
import re

import numpy as np
import pytest

import fake_device
import variogram_cases as VC
from oracle import wbx_oracle as O
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import multivariate
from weatherbenchx_amd.metrics import probabilistic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = ('time', 'level', 'latitude', 'longitude')
SHAPE = (2, 3, 6, 9)
M = 5
POWERS = (0.5, 1.0, 2.0)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('power', POWERS)
def test_restatement_equals_the_oracle_and_the_host_route(power):
  rng = np.random.default_rng(7)
  for _ in range(12):
    m, nl = int(rng.integers(1, 9)), int(rng.integers(1, 12))
    p = rng.normal(size=(m, 2, 3, 4, nl)) * 3
    t = rng.normal(size=(2, 3, 4, nl)) * 3
    stat, bound = VC.variogram_points(p, t, power)
    want = O.variogram_score(p, t[None], pair_axis=-1, ensemble_axis=0, power=power)
    np.testing.assert_allclose(stat, want, rtol=1e-12, atol=1e-13 * float(np.abs(want).max() + 1))
    assert (bound >= 0).all() and np.isfinite(bound).all()
    dims = ('a', 'b', 'c', 'run')
    host = multivariate.VariogramScore(dim='run', ensemble_dim='number', p=power).host_per_variable(
        xr.DataArray(p, dims=('number',) + dims), xr.DataArray(t, dims=dims))
    np.testing.assert_allclose(np.asarray(host.transpose('a', 'b', 'c').values), stat, rtol=1e-12, atol=1e-13 * float(np.abs(want).max() + 1))


@pytest.mark.parametrize('power', [0.5, 1.0])
def test_restatement_reproduces_the_pinned_known_answers(power):
  """The fields and the table tests/test_probabilistic_more.py pins VariogramScore with; members equal to the target score 0."""
  rng = np.random.default_rng(9)
  p, t = rng.normal(size=(2, 5, 6, 3)), rng.normal(size=(2, 5, 6))  # [time, latitude, longitude, realization]
  stat, _ = VC.variogram_points(np.moveaxis(p, -1, 0), t, power)
  np.testing.assert_allclose(stat, O.variogram_score(p, t[..., None], pair_axis=2, ensemble_axis=3, power=power), rtol=1e-12)
  pred = {'v': xr.DataArray(p, dims=('time', 'latitude', 'longitude', 'realization'))}
  targ = {'v': xr.DataArray(t, dims=('time', 'latitude', 'longitude'))}
  got = probabilistic.VariogramScore(dim='longitude', ensemble_dim='realization', p=power).compute(pred, targ)['v']
  np.testing.assert_allclose(np.asarray(got.values), stat, rtol=1e-12)
  same, _ = VC.variogram_points(np.repeat(t[None], 3, axis=0), t, power)
  assert (same <= 1e-28).all()  # (the mean of three equal float64 terms need not be that term to the last bit)


@pytest.mark.parametrize('power', POWERS)
@pytest.mark.parametrize('kind', VC.NONFINITE + ('inf_target', 'two_inf_opposite'))
def test_any_non_finite_input_gives_nan(kind, power):
  """The restatement, the oracle's full tables and the host route agree: NaN, never +inf, and only at that point."""
  rng = np.random.default_rng(3)
  p = rng.integers(-64, 65, size=(4, 1, 1, 3, 5)) / 8.0
  t = rng.integers(-64, 65, size=(1, 1, 3, 5)) / 8.0
  if kind == 'inf_member':
    p[2, 0, 0, 1, 3] = -np.inf
  elif kind == 'two_inf':
    p[0, 0, 0, 1, 3] = p[3, 0, 0, 1, 3] = np.inf
  elif kind == 'two_inf_opposite':
    p[0, 0, 0, 1, 3], p[3, 0, 0, 1, 0] = np.inf, -np.inf
  elif kind == 'nan_member':
    p[1, 0, 0, 1, 0] = np.nan
  elif kind == 'nan_target':
    t[0, 0, 1, 4] = np.nan
  else:
    t[0, 0, 1, 2] = np.inf
  stat, _ = VC.variogram_points(p, t, power)
  assert np.isnan(stat[0, 0, 1]) and np.isfinite(stat[0, 0, [0, 2]]).all()
  with np.errstate(all='ignore'):
    table = O.variogram_score(p, t[None], pair_axis=-1, ensemble_axis=0, power=power)
    host = multivariate.VariogramScore(dim='run', ensemble_dim='number', p=power).host_per_variable(
        xr.DataArray(p, dims=('number', 'a', 'b', 'c', 'run')), xr.DataArray(t, dims=('a', 'b', 'c', 'run')))
  for other in (table, np.asarray(host.transpose('a', 'b', 'c').values)):
    np.testing.assert_array_equal(np.isnan(other), np.isnan(stat))
    assert not np.isinf(other).any()
  one = np.full((1, 1, 1, 1, 1), np.inf)  # L = 1: no pairs, the diagonal alone decides
  assert np.isnan(VC.variogram_points(one, np.zeros((1, 1, 1, 1)), power)[0]).all()
  assert (VC.variogram_points(np.ones((2, 1, 1, 1, 1)), np.zeros((1, 1, 1, 1)), power)[0] == 0.0).all()


@pytest.mark.parametrize('flags', [0, VC.FLAG_MASKED, VC.FLAG_SKIPNA, VC.FLAG_MASKED | VC.FLAG_SKIPNA])
def test_cases_keep_their_promises(flags):
  for seed, (m, nl, nx, dc, x_kept) in enumerate([(5, 3, 9, 2, False), (51, 9, 57, 5, True), (1, 1, 7, 2, True), (4, 17, 16, 5, False)]):
    for dtype, power in ((np.float32, 0.5), (np.float64, 2.0)):
      p, t, mask, want, bound, stat = VC.variogram_case(seed, m, nl, 2, 5, nx, dtype, flags, dc, x_kept, power)
      assert p.shape == (m, 2, 5, nx, nl) and t.shape == (2, 5, nx, nl) and p.dtype == t.dtype == dtype and p.flags.c_contiguous
      assert want.shape == bound.shape == (2, -(-5 // dc), 2 if flags else 1, nx if x_kept else 1)
      assert (bound >= 0).all() and np.isfinite(bound).all() and not np.isinf(stat).any()
      if flags & VC.FLAG_SKIPNA:
        assert np.isnan(stat).any() and not np.isnan(want).any()
      else:
        assert np.isfinite(want[:, :, 0]).mean() >= 0.8
      fin = np.isfinite(want[:, :, 0]) & (want[:, :, 0] > 0)
      if np.dtype(dtype) == np.float32 and nl > 1:  # about 1e-6 of the score: a lost member or a float32 member sum would exceed it
        assert (bound[:, :, 0][fin] <= 1e-5 * want[:, :, 0][fin]).all()
      zero = (p == t[None]).all(axis=(0, -1))
      assert zero.any() or nx < 9
      assert (stat[zero & np.isfinite(stat)] <= 1e-24).all()  # (0 up to the float64 rounding of a mean of equal terms)


def test_tile_points_and_member_chunks_mirror_the_kernels_formulas():
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_ens_variogram.hip')) as f:
    source = f.read()
  consts = {k: int(v) for k, v in re.findall(r'constexpr int VGRM_(PMAX|ITEMS_TOTAL|STAGE|TGT) = (\d+);', source)}
  assert consts == {'PMAX': VC.PMAX, 'ITEMS_TOTAL': VC.ITEMS_TOTAL, 'STAGE': VC.STAGE_ELEMS, 'TGT': VC.TGT_ELEMS}
  for l in range(1, VC.MAX_RUN + 1):
    tile = VC.tile_points(l)
    assert tile == _hip.vgram_tile_points(l) and 1 <= tile <= VC.PMAX
    assert tile * (l * (l - 1) // 2) <= VC.ITEMS_TOTAL and tile * l <= VC.TGT_ELEMS
    for m in range(1, VC.MAX_MEMBERS + 1):
      mc = VC.member_chunk(m, l)
      assert mc == _hip.vgram_member_chunk(m, l) and 1 <= mc <= m and tile * mc * l <= VC.STAGE_ELEMS


# ---- the C ABI, no device ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_binding_agrees():
  with open(os.path.join(ROOT, 'include', 'wbx.h')) as f:
    header = f.read()
  assert re.search(r'int wbx_ens_variogram_partial\(wbx_ctx\* ctx, const wbx_s1_plan\* plan, int dtype[^;]*int M, int64_t member_stride,\s*'
                   r'int64_t L, int64_t p_run_stride, int64_t t_run_stride, int power[^;]*const void\* p,\s*const void\* t,\s*'
                   r'const uint8_t\* mask, double\* partial_out\);', header)
  assert int(re.search(r'WBX_FN_ENS_VARIOGRAM_PARTIAL\s*=\s*(\d+)', header).group(1)) == _hip.FN_IDS['wbx_ens_variogram_partial'] == 23
  define = lambda name: int(re.search(rf'#define {name} (\d+)', header).group(1))
  assert define('WBX_VGRAM_LANES') == _hip.VGRAM_LANES == VC.NLANE == 1
  assert define('WBX_VGRAM_MAX_MEMBERS') == _hip.VGRAM_MAX_MEMBERS == VC.MAX_MEMBERS == 64
  assert define('WBX_VGRAM_MAX_RUN') == _hip.VGRAM_MAX_RUN == VC.MAX_RUN == 64
  assert (define('WBX_VGRAM_POW_HALF'), define('WBX_VGRAM_POW_ONE'), define('WBX_VGRAM_POW_TWO')) == (0, 1, 2)
  assert (_hip.VGRAM_POW_HALF, _hip.VGRAM_POW_ONE, _hip.VGRAM_POW_TWO) == (0, 1, 2)
  assert _hip.VGRAM_POWERS == VC.POWERS == {0.5: 0, 1.0: 1, 2.0: 2}
  assert define('WBX_ABI_VERSION') == 13
  assert len(set(_hip.FN_IDS.values())) == len(_hip.FN_IDS)
  assert 'wbx_ens_variogram_partial' in _hip.EXPORTED_SYMBOLS
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_replay.hip')) as f:
    assert 'WBX_REPLAY_CASE(WBX_FN_ENS_VARIOGRAM_PARTIAL, wbx_ens_variogram_partial)' in f.read()
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'Makefile')) as f:
    assert 'wbx_ens_variogram.hip' in f.read()


def test_library_exports_the_entry_point_and_refuses_a_null_context():
  lib = _hip.load_library()
  # ctx, plan, dtype, M, member_stride, L, p_run_stride, t_run_stride, power, p, t, mask, partial_out
  assert len(_hip.PROTOS['wbx_ens_variogram_partial']) == 13
  assert lib.wbx_abi_version() == 13
  rc = lib.wbx_ens_variogram_partial(None, None, _hip.F32, 2, 1, 2, 1, 1, 0, None, None, None, None)
  assert rc == -1  # WBX_ERR_INVALID
  assert 'wbx_ens_variogram_partial: ctx is NULL' in lib.wbx_last_error().decode()


# ---- the gating -------------------------------------------------------------------------------------------------------------------
def _inputs(dtype=np.float32, seed=3, m=M, shape=SHAPE):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(shape[0]), 'level': np.arange(shape[1]) * 100.0, 'latitude': np.linspace(-75, 75, shape[2]),
        'longitude': np.arange(shape[3]) * 40.0}
  p = (rng.integers(-64, 65, size=(m,) + shape) / 8.0).astype(dtype)
  t = (rng.integers(-64, 65, size=shape) / 8.0).astype(dtype)
  return (xr.DataArray(p, dims=('number',) + DIMS, coords=dict(cs, number=np.arange(m)), name='v'),
          xr.DataArray(t, dims=DIMS, coords=cs, name='v'))


class _Ctx(_hip.Context):  # a context the gate may ask: nothing is launched on it
  def __init__(self):  # pylint: disable=super-init-not-called
    self.lib = type('Lib', (), {'wbx_ens_variogram_partial': staticmethod(lambda *a: 0)})()

  def __del__(self):
    pass


def test_the_gate_declines_every_fallback_condition_without_a_device(monkeypatch):
  monkeypatch.setattr(_hip, 'default_context', _Ctx)
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  gate = multivariate._fused_variogram  # pylint: disable=protected-access
  p, t = _inputs()
  taken = gate(p, t, 'level', 'number', 0.5)
  assert isinstance(taken, lazy.LazyStatistic) and taken._group.kind == 'vgrm' and taken.dims == ('time', 'latitude', 'longitude')  # pylint: disable=protected-access
  assert taken._group.ens['power'] == 0.5 and taken._group.ens['norm_dims'] == ('level',)  # pylint: disable=protected-access
  for power in (1, 2, 1.0, 2.0, np.float32(0.5)):
    assert gate(p, t, 'level', 'number', power) is not None, power
  # two powers on one pair: two groups, although the statistics' unique names are the same
  g1, g2 = gate(p, t, 'level', 'number', 0.5)._group, gate(p, t, 'level', 'number', 2.0)._group  # pylint: disable=protected-access
  assert g1 is taken._group and g2 is not g1 and g2.ens['power'] == 2.0  # pylint: disable=protected-access
  a, b = multivariate.VariogramScore('level', 'number', 0.5), multivariate.VariogramScore('level', 'number', 2.0)
  assert a.unique_name == b.unique_name == 'VariogramScore_dim=level_ensemble_dim=number'
  for why, args in {
      'p = 0.3': (p, t, 'level', 'number', 0.3),
      'p is no number': (p, t, 'level', 'number', None),
      'a list of dims': (p, t, ['level'], 'number', 0.5),
      'no member dim': (p, t, 'level', 'realization', 0.5),
      'members in the targets': (p, p, 'level', 'number', 0.5),
      'the member dim as dim': (p, t, 'number', 'number', 0.5),
      'a dim the targets lack': (p, t.isel(level=0, drop=True), 'level', 'number', 0.5),
      'two sizes along dim': (p, t.isel(level=slice(0, 2)), 'level', 'number', 0.5),
      'integer inputs': (p.astype(np.int64), t, 'level', 'number', 0.5),
      'targets with a dim of their own': (p, t.expand_dims(realization=[0, 1]), 'level', 'number', 0.5),
      'nothing left of the frame': (p.isel(time=0, latitude=0, longitude=0, drop=True), t.isel(time=0, latitude=0, longitude=0, drop=True),
                                    'level', 'number', 0.5),
      'a mask along dim': (p, t.assign_coords(mask=(('level', 'latitude'), np.ones((3, 6), bool))), 'level', 'number', 0.5),
      'a mask along the member dim': (p.assign_coords(mask=(('number',), np.ones(M, bool))), t, 'level', 'number', 0.5),
      'labels that differ': (p, t.assign_coords(latitude=np.linspace(-75, 75, 6) + 1.0), 'level', 'number', 0.5),
  }.items():
    assert gate(*args) is None, why
  big_l = _inputs(shape=(1, 65, 2, 2))
  assert gate(*big_l, 'level', 'number', 0.5) is None
  assert gate(*_inputs(shape=(1, 64, 2, 2)), 'level', 'number', 0.5) is not None
  assert gate(*_inputs(m=65), 'level', 'number', 0.5) is None
  assert gate(*_inputs(m=64), 'level', 'number', 0.5) is not None and gate(*_inputs(m=1), 'level', 'number', 0.5) is not None
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', False)
  assert gate(p, t, 'level', 'number', 0.5) is None


def test_a_run_of_stride_zero_is_no_strided_run():
  lay = lazy.planner.InputLayout(strides={'a': 4, 'run': 0}, itemsize=4)
  assert engine.norm_run(lay, ('run',), {'a': 3, 'run': 4}) is None
  assert engine.norm_run(lay, ('run',), {'a': 3, 'run': 1}) == (1, 0)


def test_without_a_device_the_gate_declines_instead_of_raising(monkeypatch):
  def no_device(*a, **k):
    raise _hip.WbxUnavailableError('no device')
  monkeypatch.setattr(_hip, 'default_context', no_device)
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  p, t = _inputs(np.float64)
  got = multivariate.VariogramScore(dim='level', ensemble_dim='number').compute({'v': p}, {'v': t})['v']
  assert not isinstance(got, lazy.LazyStatistic)
  want, _ = VC.variogram_points(np.moveaxis(p.values, 2, -1), np.moveaxis(t.values, 1, -1), 0.5)
  np.testing.assert_allclose(np.asarray(got.values), want, rtol=1e-12)


def test_a_context_without_the_library_keeps_the_host_route(monkeypatch):
  """The plan interpreter's context is no _hip.Context, so nothing asks it for the new launch; TiledVariogramScore through the
  Aggregator is the host route's and the restatement's number."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  assert not engine.ens_variogram_available(_hip.default_context()) and not engine.ens_variogram_available(object())
  p, t = _inputs(np.float64)
  log = []
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', log)
  metrics = {'vs': probabilistic.TiledVariogramScore(window_size=3, ensemble_dim='number', p=1.0)}
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, {'v': p}, {'v': t})
  assert not any(isinstance(s, lazy.LazyStatistic) for per_var in stats.values() for s in per_var.values())
  values = aggregation.Aggregator(reduce_dims=['time', 'level', 'latitude', 'longitude']).aggregate_statistics(stats).metric_values(metrics)
  assert not [e for e in log if e['kind'] == 'vgrm']
  tile = lambda a, ilat: np.stack([np.roll(np.roll(a, 1 - i, ilat), 1 - j, ilat + 1) for i in range(3) for j in range(3)], axis=-1)
  pw, tw = tile(p.values, 3)[:, :, :, 1:-1], tile(t.values, 2)[:, :, 1:-1]
  want, _ = VC.variogram_points(pw, tw, 1.0)
  np.testing.assert_allclose(float(np.asarray(values['vs.v'].values)), want.mean(), rtol=1e-12)
  engine.clear_caches()


def test_the_switch_reads_the_environment_and_the_readme_documents_it():
  assert lazy.FUSED_VARIOGRAM == (os.environ.get('WBX_FUSED_VARIOGRAM', '1') != '0')
  with open(os.path.join(ROOT, 'README.md')) as f:
    readme = f.read()
  row = [line for line in readme.splitlines() if line.startswith('| `WBX_FUSED_VARIOGRAM` |')]
  assert len(row) == 1 and 'wbx_ens_variogram_partial' in row[0] and 'tools/bench_variogram.py' in row[0]
  assert 'variogram score' in [line for line in readme.splitlines() if line.startswith('| hot kernels |')][0]
