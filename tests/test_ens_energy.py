"""The energy score's fused route without a device: the C ABI's declaration, the float64 restatement (tests/energy_cases.py)
against the oracle, the case generator's promises, the gating of metrics.multivariate (every condition keeps the host route, and
without a device nothing is asked of one), and engine.norm_run."""
import os
import re

import numpy as np
import pytest

import energy_cases as GC
import fake_device
from oracle import wbx_oracle as O
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import planner
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import multivariate
from weatherbenchx_amd.metrics import probabilistic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = ('time', 'level', 'latitude', 'longitude')
SHAPE = (2, 3, 6, 9)
M = 5


# ---- the C ABI, no device ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_binding_agrees():
  with open(os.path.join(ROOT, 'include', 'wbx.h')) as f:
    header = f.read()
  assert re.search(r'int wbx_ens_energy_partial\(wbx_ctx\* ctx, const wbx_s1_plan\* plan, int dtype[^;]*int M, int64_t member_stride,\s*'
                   r'int64_t L, int64_t p_norm_stride, int64_t t_norm_stride, const void\* p, const void\* t,\s*const uint8_t\* mask, '
                   r'double\* partial_out\);', header)
  assert int(re.search(r'WBX_FN_ENS_ENERGY_PARTIAL\s*=\s*(\d+)', header).group(1)) == _hip.FN_IDS['wbx_ens_energy_partial'] == 22
  assert int(re.search(r'#define WBX_ENRG_LANES (\d+)', header).group(1)) == _hip.ENRG_LANES == 2
  assert int(re.search(r'#define WBX_ENRG_MAX_MEMBERS (\d+)', header).group(1)) == _hip.ENRG_MAX_MEMBERS >= 64
  assert int(re.search(r'#define WBX_ABI_VERSION (\d+)', header).group(1)) == 13
  assert len(set(_hip.FN_IDS.values())) == len(_hip.FN_IDS)
  assert 'wbx_ens_energy_partial' in _hip.EXPORTED_SYMBOLS
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_replay.hip')) as f:
    assert 'WBX_REPLAY_CASE(WBX_FN_ENS_ENERGY_PARTIAL, wbx_ens_energy_partial)' in f.read()
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_ens_energy.hip')) as f:
    source = f.read()
  assert int(re.search(r'constexpr int ENRG_LC = (\d+);', source).group(1)) == _hip.ENRG_LDS_CHUNK == GC.LDS_CHUNK


def test_library_exports_the_entry_point_and_refuses_a_null_context():
  lib = _hip.load_library()
  # ctx, plan, dtype, M, member_stride, L, p_norm_stride, t_norm_stride, p, t, mask, partial_out
  assert len(_hip.PROTOS['wbx_ens_energy_partial']) == 12
  assert lib.wbx_abi_version() == 13
  rc = lib.wbx_ens_energy_partial(None, None, _hip.F32, 2, 1, 1, 1, 1, None, None, None, None)
  assert rc == -1  # WBX_ERR_INVALID
  assert 'wbx_ens_energy_partial: ctx is NULL' in lib.wbx_last_error().decode()


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_oracle_point_by_point():
  rng = np.random.default_rng(7)
  for i in range(40):
    m, nl = int(rng.integers(2, 20)), int(rng.integers(1, 12))
    p = rng.normal(size=(m, 2, 3, 4, nl)) * 3
    t = rng.normal(size=(2, 3, 4, nl)) * 3
    fair = bool(i % 2)
    stat = GC.energy_points(p, t, fair)
    np.testing.assert_allclose(stat[..., 0], O.energy_score_skill(p, t[None], -1, 0), rtol=1e-13, atol=0)
    np.testing.assert_allclose(stat[..., 1], O.energy_score_spread(p, -1, 0, fair=fair), rtol=1e-13, atol=0)


def test_restatement_has_the_ieee_classes():
  t = np.zeros((1, 1, 1, 2))
  p = np.arange(6, dtype=np.float64).reshape(3, 1, 1, 1, 2)
  q = p.copy(); q[1, ..., 0] = np.inf
  assert np.isposinf(GC.energy_points(q, t, True)).all()  # an infinite member against finite ones
  q[2, ..., 0] = np.inf
  s = GC.energy_points(q, t, True)[0, 0, 0]
  assert np.isposinf(s[0]) and np.isnan(s[1])  # two of one sign: inf - inf in the spread only
  q = p.copy(); q[0, ..., 1] = np.nan
  assert np.isnan(GC.energy_points(q, t, True)).all()
  u = t.copy(); u[..., 0] = np.nan
  s = GC.energy_points(p, u, True)[0, 0, 0]
  assert np.isnan(s[0]) and np.isfinite(s[1])  # the spread never looks at the target
  one = np.full((4, 1, 1, 1, 3), np.inf)  # (a member is never paired with itself: NaN here comes from the pairs, not the diagonal)
  assert np.isnan(GC.energy_points(one, np.zeros((1, 1, 1, 3)), False)[..., 1]).all()
  p[:] = 280.25
  assert (GC.energy_points(p, np.full_like(t, 280.25), True) == 0.0).all()


@pytest.mark.parametrize('flags', [0, GC.FLAG_MASKED, GC.FLAG_SKIPNA, GC.FLAG_MASKED | GC.FLAG_SKIPNA])
def test_cases_keep_their_promises(flags):
  for seed, (m, nl, nx, dc, x_kept) in enumerate([(5, 3, 9, 2, False), (51, 13, 65, 5, True), (3, 17, 1, 2, True), (4, 1, 64, 5, False)]):
    for dtype in (np.float32, np.float64):
      p, t, mask = GC.energy_case(seed, m, nl, 2, 5, nx, dtype, flags, dc, x_kept)
      assert p.shape == (m, 2, 5, nx, nl) and t.shape == (2, 5, nx, nl) and p.dtype == t.dtype == dtype
      fin = p[np.isfinite(p)]
      grid = np.abs(fin) <= 8
      assert (fin[grid] * 8 == np.round(fin[grid] * 8)).all()                                        # the dyadic grid
      assert ((fin[~grid] >= 280) & (fin[~grid] < 281) & (fin[~grid] * 1024 == np.round(fin[~grid] * 1024))).all()  # the clusters
      want, bound, stat = GC.expected(p, t, True, mask, flags, dc, x_kept)
      assert (bound >= 0).all() and np.isfinite(bound).all()
      if flags & GC.FLAG_SKIPNA:
        assert np.isnan(stat).any() and not np.isnan(want).any()
      else:
        assert np.isfinite(want[:, :, :2]).all(axis=2).mean() >= 0.8
      zero = (p == t[None]).all(axis=(0, -1))
      if nx > 1:
        assert zero.any()
      assert (stat[zero & np.isfinite(stat).all(axis=-1)] == 0.0).all()
      for member in GC.MEMBER_AXES:
        for norm in GC.NORM_AXES:
          pv, tv = GC.arrange(p, t, member, norm)
          assert np.array_equal(pv, p, equal_nan=True) and np.array_equal(tv, t, equal_nan=True)


def test_tile_points_mirror_the_kernels_formula():
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_ens_energy.hip')) as f:
    source = f.read()
  consts = {k: int(v) for k, v in re.findall(r'constexpr int ENRG_(PMAX|VECS|ITEMS) = (\d+);', source)}
  assert consts == {'PMAX': 64, 'VECS': 416, 'ITEMS': 3}
  for m in range(2, _hip.ENRG_MAX_MEMBERS + 1):
    for threads in (64, 128, 256):
      tile = _hip.enrg_tile_points(m, threads)
      mp = (m + 4) // 4 * 4
      nblk = (mp // 4) * (mp // 4 + 1) // 2
      assert 1 <= tile <= 64 and tile * mp <= 416 and tile * nblk <= 3 * threads


def test_norm_run_collapses_adjacent_dims_only():
  lay = planner.layout_of(np.zeros((4, 3, 5, 6), np.float32), ('a', 'b', 'c', 'd'))
  sizes = {'a': 4, 'b': 3, 'c': 5, 'd': 6}
  assert engine.norm_run(lay, ('d',), sizes) == (6, 1)
  assert engine.norm_run(lay, ('b',), sizes) == (3, 30)
  assert engine.norm_run(lay, ('c', 'd'), sizes) == (30, 1) == engine.norm_run(lay, ('d', 'c'), sizes)
  assert engine.norm_run(lay, ('b', 'd'), sizes) is None
  assert engine.norm_run(lay, ('a', 'b', 'c', 'd'), sizes) == (360, 1)
  one = planner.layout_of(np.zeros((4, 1, 5), np.float32), ('a', 'b', 'c'))
  assert engine.norm_run(one, ('b',), {'a': 4, 'b': 1, 'c': 5}) == (1, 0)
  assert engine.norm_run(one, ('a', 'c'), {'a': 4, 'b': 1, 'c': 5}) == (20, 1)  # a dim of size 1 in between does not matter


# ---- the gating -------------------------------------------------------------------------------------------------------------------
def _inputs(dtype=np.float32, seed=3):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(SHAPE[0]), 'level': np.array([500.0, 700.0, 850.0]), 'latitude': np.linspace(-75, 75, SHAPE[2]),
        'longitude': np.arange(SHAPE[3]) * 40.0}
  p = (rng.integers(-64, 65, size=(M,) + SHAPE) / 8.0).astype(dtype)
  t = (rng.integers(-64, 65, size=SHAPE) / 8.0).astype(dtype)
  return ({'v': xr.DataArray(p, dims=('number',) + DIMS, coords=dict(cs, number=np.arange(M)), name='v')},
          {'v': xr.DataArray(t, dims=DIMS, coords=cs, name='v')})


def _oracle_score(pred, targ, norm_axes, fair=True):
  p, t = np.asarray(pred['v'].values, np.float64), np.asarray(targ['v'].values, np.float64)
  return (O.energy_score_skill(p, t[None], norm_axes, 0) - 0.5 * O.energy_score_spread(p, norm_axes, 0, fair=fair)).mean()


def test_without_a_device_the_gate_declines_instead_of_raising(monkeypatch):
  def no_device(*a, **k):
    raise _hip.WbxUnavailableError('no device')
  monkeypatch.setattr(_hip, 'default_context', no_device)
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', True)
  pred, targ = _inputs()
  skill = multivariate.EnergyScoreSkill(dim='level', ensemble_dim='number').compute(pred, targ)['v']
  spread = multivariate.EnergyScoreSpread(dim='level', ensemble_dim='number').compute(pred, targ)['v']
  assert not isinstance(skill, lazy.LazyStatistic) and not isinstance(spread, lazy.LazyStatistic)
  want = GC.energy_points(np.moveaxis(pred['v'].values, 2, -1), np.moveaxis(targ['v'].values, 1, -1), True)
  np.testing.assert_allclose(np.asarray(skill.values), want[..., 0], rtol=1e-5)
  np.testing.assert_allclose(np.asarray(spread.values), want[..., 1], rtol=1e-5)


def test_a_context_without_the_library_keeps_the_host_route(monkeypatch):
  """The gate as shipped: the plan interpreter's context is no _hip.Context, so nothing asks it for the new launch; the host route
  and the restatement both agree with the oracle."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', True)
  assert not engine.ens_energy_available(_hip.default_context()) and not engine.ens_energy_available(object())
  pred, targ = _inputs(np.float64)
  log = []
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', log)
  metrics = {'es': probabilistic.EnergyScore(dim='level', ensemble_dim='number')}
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  assert not any(isinstance(s, lazy.LazyStatistic) for per_var in stats.values() for s in per_var.values())
  values = aggregation.Aggregator(reduce_dims=['time', 'latitude', 'longitude']).aggregate_statistics(stats).metric_values(metrics)
  assert not [e for e in log if e['kind'] == 'enrg']
  want = _oracle_score(pred, targ, 2)
  np.testing.assert_allclose(float(np.asarray(values['es.v'].values)), want, rtol=1e-12)
  stat = GC.energy_points(np.moveaxis(pred['v'].values, 2, -1), np.moveaxis(targ['v'].values, 1, -1), True)
  np.testing.assert_allclose((stat[..., 0] - 0.5 * stat[..., 1]).mean(), want, rtol=1e-13)
  engine.clear_caches()


def test_probabilistic_hands_the_names_on_and_unique_names_do_not_change():
  assert probabilistic.EnergyScoreSkill is multivariate.EnergyScoreSkill
  assert multivariate.EnergyScoreSkill(dim='level', ensemble_dim='number').unique_name == 'EnergyScore_Skill_dim=level_ensemble_dim=number'
  assert (multivariate.EnergyScoreSpread(dim='level', ensemble_dim='number', fair=False).unique_name
          == 'EnergyScore_Spread_dim=level_ensemble_dim=number_fair=False')


def test_the_switch_reads_the_environment():
  assert lazy.FUSED_ENERGY == (os.environ.get('WBX_FUSED_ENERGY', '1') != '0')
  assert lazy.ENERGY_LANE == {'EnergyScoreSkill': 0, 'EnergyScoreSpread': 1}
