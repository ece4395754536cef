"""The Wasserstein distance's fused route without a device: the float64 restatement (tests/wasserstein_cases.py) against scipy, the
oracle and the host route, the non-finite rule, the walk's piece count, the case generator's promises, the C ABI's declaration
against the bindings, the gating of metrics.multivariate (every condition keeps the host route, and without a device nothing is
asked of one), and the README row."""
import math
import os
import re

import numpy as np
import pytest
import scipy.stats

import fake_device
import wasserstein_cases as WC
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
SHAPE = (2, 3, 4, 5)
M, N = 5, 3


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_restatement_equals_scipy_and_the_oracle():
  """Random (M, N) in 1..64, ties, rounded values and mixed scales; the tolerance is the derived bound's, a side."""
  rng = np.random.default_rng(11)
  for k in range(120):
    m, n = int(rng.integers(1, 65)), int(rng.integers(1, 65))
    scale = 10.0 ** rng.integers(-3, 4)
    p, t = rng.normal(size=(m, 3)) * scale, rng.normal(size=(n, 3)) * scale + rng.normal()
    if k % 3 == 0:
      p, t = np.round(p, 1), np.round(t, 1)  # ties within and between the ensembles
    if k % 4 == 0:
      t[: min(m, n)] = p[: min(m, n)]
    stat, bound = WC.wasserstein_points(p, t)
    rtol = 2.0 * (m + n + 4) * 2.0 ** -53
    for q in range(3):
      assert abs(stat[q] - scipy.stats.wasserstein_distance(p[:, q], t[:, q])) <= rtol * stat[q] + 1e-300, (m, n)
      assert abs(stat[q] - O.wasserstein_1d(p[:, q], t[:, q])) <= rtol * stat[q] + 1e-300, (m, n)
    assert (bound >= 0).all() and np.isfinite(bound).all()


def test_restatement_equals_the_host_route():
  rng = np.random.default_rng(2)
  for m, n in ((1, 1), (5, 3), (7, 7), (51, 10)):
    p, t = rng.normal(size=(m, 2, 3)).astype(np.float32), rng.normal(size=(n, 2, 3)).astype(np.float32)
    host = multivariate.WassersteinDistance('number').host_per_variable(xr.DataArray(p, dims=('number', 'a', 'b')),
                                                                       xr.DataArray(t, dims=('number', 'a', 'b')))
    np.testing.assert_allclose(np.asarray(host.transpose('a', 'b').values), WC.wasserstein_points(p, t)[0], rtol=1e-13)


def test_exact_evaluation_equals_the_restatement_on_dyadic_inputs():
  for seed, (m, n) in enumerate(((1, 1), (2, 3), (6, 4), (51, 10), (64, 63))):
    for dtype in (np.float32, np.float64):
      p, t = WC.values(seed, m, n, (2, 3, 7), dtype)
      np.testing.assert_array_equal(WC.exact_points(p, t), WC.wasserstein_points(p, t)[0])


HAND_MADE = [  # (p, t, what the reference gives)
    ([np.nan, 1.0], [0.0], 'nan'), ([1.0, 2.0], [np.nan, 0.0, 3.0], 'nan'), ([np.inf, np.inf], [0.0], 'nan'),
    ([np.inf, 1.0], [np.inf, 0.0], 'nan'), ([0.0], [-np.inf, -np.inf, 2.0], 'nan'), ([-np.inf, 1.0], [-np.inf], 'nan'),
    ([np.inf, 1.0], [2.0, 3.0], 'inf'), ([1.0], [-np.inf, 3.0, 4.0], 'inf'), ([-np.inf, 2.0], [np.inf, 0.0], 'inf'),
    ([-np.inf, np.inf, 0.5], [0.0, 1.0], 'inf'), ([np.inf], [5.0], 'inf'), ([-np.inf], [np.inf], 'inf'),
]


@pytest.mark.parametrize('p, t, kind', HAND_MADE)
def test_the_non_finite_rule_is_what_scipy_the_oracle_and_the_host_route_give(p, t, kind):
  p, t = np.array(p), np.array(t)
  stat = float(WC.wasserstein_points(p[:, None], t[:, None])[0][0])
  with np.errstate(all='ignore'):
    others = [scipy.stats.wasserstein_distance(p, t), O.wasserstein_1d(p, t),
              float(multivariate.WassersteinDistance('number').host_per_variable(
                  xr.DataArray(p[:, None], dims=('number', 'a')), xr.DataArray(t[:, None], dims=('number', 'a'))).values[0])]
  for got in [stat] + others:
    assert (np.isnan(got) if kind == 'nan' else got == np.inf), (kind, got, others)


def test_the_walk_has_m_plus_n_minus_gcd_pieces_that_cover_the_unit_interval():
  for m in range(1, 65):
    for n in range(1, 65):
      walk = WC.pieces(m, n)
      assert len(walk) == m + n - math.gcd(m, n) == WC.piece_count(m, n)
      assert sum(c for _, _, c in walk) == m * n and all(c >= 1 for _, _, c in walk)
      assert walk[0][:2] == (0, 0) and walk[-1][:2] == (m - 1, n - 1)
      assert all(0 <= b[0] - a[0] <= 1 and 0 <= b[1] - a[1] <= 1 for a, b in zip(walk, walk[1:]))
  assert [WC.padded(m) for m in (1, 4, 5, 8, 9, 16, 17, 32, 33, 50, 51, 52, 64)] == [4, 4, 8, 8, 16, 16, 32, 32, 50, 50, 51, 64, 64]


@pytest.mark.parametrize('flags', [0, WC.FLAG_MASKED, WC.FLAG_SKIPNA, WC.FLAG_MASKED | WC.FLAG_SKIPNA])
def test_cases_keep_their_promises(flags):
  for seed, (m, n, nx, dc, x_kept) in enumerate([(5, 3, 9, 2, False), (51, 10, 70, 5, True), (1, 1, 7, 2, True), (4, 64, 16, 5, False)]):
    for dtype in (np.float32, np.float64):
      p, t, mask, want, bound, stat = WC.wasserstein_case(seed, m, n, 2, 5, nx, dtype, flags, dc, x_kept)
      assert p.shape == (m, 2, 5, nx) and t.shape == (n, 2, 5, nx) and p.dtype == t.dtype == dtype and p.flags.c_contiguous
      assert want.shape == bound.shape == (2, -(-5 // dc), 2 if flags else 1, nx if x_kept else 1)
      assert (bound >= 0).all() and np.isfinite(bound).all() and not np.isinf(stat).any()
      if flags & WC.FLAG_SKIPNA:
        assert np.isnan(stat).any() and not np.isnan(want).any()
      else:
        assert np.isfinite(want[:, :, 0]).mean() >= 0.8
      fin = np.isfinite(want[:, :, 0]) & (want[:, :, 0] > 0)
      assert (bound[:, :, 0][fin] <= 1e-13 * want[:, :, 0][fin]).all()  # float32 differences would miss it by seven digits
      np.testing.assert_array_equal(np.isnan(stat), WC.nan_rule(p, t))
      zero = (p == p[:1]).all(axis=0) & (t == p[:1]).all(axis=0) & ~WC.nan_rule(p, t)  # (one member a side: inf against inf is equal too)
      assert (stat[zero] == 0.0).all()


# ---- the C ABI, no device ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_binding_agrees():
  with open(os.path.join(ROOT, 'include', 'wbx.h')) as f:
    header = f.read()
  assert re.search(r'int wbx_ens_wasserstein_partial\(wbx_ctx\* ctx, const wbx_s1_plan\* plan, int dtype[^;]*int M, int64_t member_stride,\s*'
                   r'int N, int64_t target_member_stride, const void\* p, const void\* t, const uint8_t\* mask,\s*double\* partial_out\);',
                   header)
  assert int(re.search(r'WBX_FN_ENS_WASSERSTEIN_PARTIAL\s*=\s*(\d+)', header).group(1)) == _hip.FN_IDS['wbx_ens_wasserstein_partial'] == 24
  define = lambda name: int(re.search(rf'#define {name} (\d+)', header).group(1))
  assert define('WBX_WASS_LANES') == _hip.WASS_LANES == WC.NLANE == 1
  assert define('WBX_WASS_MAX_MEMBERS') == _hip.WASS_MAX_MEMBERS == WC.MAX_MEMBERS == 64
  assert define('WBX_ABI_VERSION') == 13
  assert len(set(_hip.FN_IDS.values())) == len(_hip.FN_IDS)
  assert 'wbx_ens_wasserstein_partial' in _hip.EXPORTED_SYMBOLS
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_replay.hip')) as f:
    assert 'WBX_REPLAY_CASE(WBX_FN_ENS_WASSERSTEIN_PARTIAL, wbx_ens_wasserstein_partial)' in f.read()
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'Makefile')) as f:
    assert 'wbx_ens_wasserstein.hip' in f.read()
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_ens_wasserstein.hip')) as f:
    source = f.read()
  assert tuple(int(s) for s in re.search(r'const int sizes\[\] = \{([^}]*)\}', source).group(1).split(',')) == WC.NETWORK_SIZES


def test_library_exports_the_entry_point_and_refuses_a_null_context():
  lib = _hip.load_library()
  # ctx, plan, dtype, M, member_stride, N, target_member_stride, p, t, mask, partial_out
  assert len(_hip.PROTOS['wbx_ens_wasserstein_partial']) == 11 == len(_hip.PROTOS['wbx_ens2_partial'])
  assert lib.wbx_abi_version() == 13
  rc = lib.wbx_ens_wasserstein_partial(None, None, _hip.F32, 2, 1, 2, 1, None, None, None, None)
  assert rc == -1  # WBX_ERR_INVALID
  assert 'wbx_ens_wasserstein_partial: ctx is NULL' in lib.wbx_last_error().decode()


# ---- the gating -------------------------------------------------------------------------------------------------------------------
def _inputs(dtype=np.float32, seed=3, m=M, n=N, shape=SHAPE):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(shape[0]), 'level': np.arange(shape[1]) * 100.0, 'latitude': np.linspace(-75, 75, shape[2]),
        'longitude': np.arange(shape[3]) * 40.0}
  p = (rng.integers(-64, 65, size=(m,) + shape) / 8.0).astype(dtype)
  t = (rng.integers(-64, 65, size=shape + (n,)) / 8.0).astype(dtype)
  return (xr.DataArray(p, dims=('number',) + DIMS, coords=dict(cs, number=np.arange(m)), name='v'),
          xr.DataArray(t, dims=DIMS + ('number',), coords=dict(cs, number=np.arange(n) + 100), name='w'))


def _same(a, b):
  """Values, dims, coordinates and name of two results."""
  assert a.dims == b.dims and a.name == b.name
  np.testing.assert_array_equal(np.asarray(a.values), np.asarray(b.values))
  assert set(a.coords) == set(b.coords)
  for k in a.coords:
    assert a.coords[k].dims == b.coords[k].dims
    np.testing.assert_array_equal(np.asarray(a.coords[k].values), np.asarray(b.coords[k].values))


class _Ctx(_hip.Context):  # a context the gate may ask: nothing is launched on it
  def __init__(self):  # pylint: disable=super-init-not-called
    self.lib = type('Lib', (), {'wbx_ens_wasserstein_partial': staticmethod(lambda *a: 0)})()

  def __del__(self):
    pass


def test_the_gate_declines_every_fallback_condition_without_a_device(monkeypatch):
  monkeypatch.setattr(_hip, 'default_context', _Ctx)
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', True)
  gate = multivariate._fused_wasserstein  # pylint: disable=protected-access
  stat = multivariate.WassersteinDistance('number')
  p, t = _inputs()
  host = stat.host_per_variable(p, t)
  taken = gate(p, t, 'number')
  assert isinstance(taken, lazy.LazyStatistic) and taken._group.kind == 'wass' and taken._lane == 0  # pylint: disable=protected-access
  assert taken._group.ens == {'member_dim': 'number', 'M': M, 'N': N, 'fair': False}  # pylint: disable=protected-access
  assert stat.compute({'v': p}, {'v': t})['v']._group is taken._group  # pylint: disable=protected-access
  # the lazy result is labelled as the host route's
  assert taken.dims == host.dims == DIMS and taken.name == host.name == 'v' and set(taken.coords) == set(host.coords) == set(DIMS)
  for k in DIMS:
    np.testing.assert_array_equal(np.asarray(taken.coords[k].values), np.asarray(host.coords[k].values))
  for why, (a, b) in {
      'integer inputs': (p.astype(np.int64), t.astype(np.int64)),
      'float16 inputs': (p.astype(np.float16), t.astype(np.float16)),
      'two dtypes': (p, t.astype(np.float64)),
      '65 predictions': _inputs(m=65),
      '65 targets': _inputs(n=65),
      'a mask along the member dim (p)': (p.assign_coords(mask=(('number',), np.ones(M, bool))), t),
      'a mask along the member dim (t)': (p, t.assign_coords(mask=(('latitude', 'number'), np.ones((4, N), bool)))),
      'nothing left of the frame': (p.isel(time=0, level=0, latitude=0, longitude=0, drop=True),
                                    t.isel(time=0, level=0, latitude=0, longitude=0, drop=True)),
      'a dim the targets lack': (p, t.isel(level=0, drop=True)),
      'a dim the predictions lack': (p.isel(time=0, drop=True), t),
      'a coordinate the two disagree about': (p.assign_coords(height=(('level',), np.arange(3.0))),
                                              t.assign_coords(height=(('level',), np.arange(3.0) + 1))),
  }.items():
    assert gate(a, b, 'number') is None, why
    got = stat.compute({'v': a}, {'v': b})['v']
    assert not isinstance(got, lazy.LazyStatistic), why
    _same(got, stat.host_per_variable(a, b))
  shifted = t.assign_coords(latitude=np.linspace(-75, 75, 4) + 1.0)
  assert gate(p, shifted, 'number') is None  # labels that differ: the host route joins nothing and takes the predictions'
  _same(stat.compute({'v': p}, {'v': shifted})['v'], stat.host_per_variable(p, shifted))
  assert gate(*_inputs(m=64, n=64), 'number') is not None and gate(*_inputs(m=1, n=1), 'number') is not None
  assert gate(*_inputs(np.float64, m=64, n=1), 'number') is not None
  masked = gate(p.assign_coords(mask=(('latitude', 'longitude'), np.ones((4, 5), bool))), t, 'number')
  assert masked is not None and 'mask' in masked.coords  # a mask over the frame is the Aggregator's business
  # the two checks come first, with their messages
  with pytest.raises(ValueError, match="Ensemble dimension 'realization' not found in predictions"):
    multivariate.WassersteinDistance('realization').compute({'v': p}, {'v': t})
  with pytest.raises(ValueError, match="Ensemble dimension 'number' not found in targets"):
    stat.compute({'v': p}, {'v': t.isel(number=0, drop=True)})
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', False)
  assert gate(p, t, 'number') is None
  _same(stat.compute({'v': p}, {'v': t})['v'], host)


def test_a_library_without_the_symbol_keeps_the_host_route(monkeypatch):
  class Old(_Ctx):
    def __init__(self):  # pylint: disable=super-init-not-called
      self.lib = type('Lib', (), {})()
  monkeypatch.setattr(_hip, 'default_context', Old)
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', True)
  assert multivariate._fused_wasserstein(*_inputs(), 'number') is None  # pylint: disable=protected-access


def test_without_a_device_the_gate_declines_instead_of_raising(monkeypatch):
  def no_device(*a, **k):
    raise _hip.WbxUnavailableError('no device')
  monkeypatch.setattr(_hip, 'default_context', no_device)
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', True)
  p, t = _inputs(np.float64)
  got = multivariate.WassersteinDistance('number').compute({'v': p}, {'v': t})['v']
  assert not isinstance(got, lazy.LazyStatistic)
  want, _ = WC.wasserstein_points(p.values, np.moveaxis(t.values, -1, 0))
  np.testing.assert_allclose(np.asarray(got.values), want, rtol=1e-13)


def test_a_context_without_the_library_keeps_the_host_route(monkeypatch):
  """The plan interpreter's context is no _hip.Context, so nothing asks it for the new launch; WassersteinDistance through the
  Aggregator is the host route's and the restatement's number."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', True)
  assert not engine.ens_wasserstein_available(_hip.default_context()) and not engine.ens_wasserstein_available(object())
  p, t = _inputs(np.float64)
  log = []
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', log)
  stat = probabilistic.WassersteinDistance('number')
  stats = {'w': {'v': stat.compute({'v': p}, {'v': t})['v']}}
  assert not isinstance(stats['w']['v'], lazy.LazyStatistic)
  agg = aggregation.Aggregator(reduce_dims=['time', 'level', 'latitude', 'longitude']).aggregate_statistics(stats)
  assert not [e for e in log if e['kind'] == 'wass']
  want, _ = WC.wasserstein_points(p.values, np.moveaxis(t.values, -1, 0))
  np.testing.assert_allclose(float(np.asarray(agg.mean_statistics()['w']['v'].values)), want.mean(), rtol=1e-12)
  engine.clear_caches()


def test_the_switch_reads_the_environment_and_the_readme_documents_it():
  assert lazy.FUSED_WASSERSTEIN == (os.environ.get('WBX_FUSED_WASSERSTEIN', '1') != '0')
  with open(os.path.join(ROOT, 'README.md')) as f:
    readme = f.read()
  row = [line for line in readme.splitlines() if line.startswith('| `WBX_FUSED_WASSERSTEIN` |')]
  assert len(row) == 1 and 'wbx_ens_wasserstein_partial' in row[0] and 'tools/bench_wasserstein.py' in row[0]
  assert 'Wasserstein' in [line for line in readme.splitlines() if line.startswith('| hot kernels |')][0]
