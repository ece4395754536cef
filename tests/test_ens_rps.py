"""The fused ranked probability score of ensembles (wbx_ens_rps_partial) without a device: the entry point's export and argument
checks, the integer restatement of tests/ens_rps_cases.py against the oracle, the float32 threshold roundings, the eligibility
rules of `EnsembleRankedProbabilityScore._compute_per_variable`, the lazy statistic as a labelled array, and the host logic of
the fused route (one launch per (p, t) pair and threshold tables, the gate) through the Aggregator with the launch itself stood in
for by the restatement.

Bounds.  Per point the restatement and the float64 arithmetic of the oracle / the host route (about ten float64 operations on
magnitudes <= 1 per threshold) agree within 16 * K * eps absolute; a sum over N points within N times that."""
import os
import pickle
import re

import numpy as np
import pytest

import ens_rps_cases as EC
import fake_device
from oracle import wbx_oracle as O
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import binning
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import weighting
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import probabilistic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
DIMS = ('time', 'latitude', 'longitude')
SHAPE = (3, 8, 10)
M = 7
THR = [0.5, 1.0, 2.5]


# ---- the C ABI, no device ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_refuses_a_null_context():
  lib = _hip.load_library()
  assert 'wbx_ens_rps_partial' in _hip.EXPORTED_SYMBOLS and 'wbx_ens_rps_partial' in _hip.PROTOS
  assert lib.wbx_abi_version() == 13
  rc = lib.wbx_ens_rps_partial(None, None, _hip.F32, 2, 1, 1, None, None, 1, None, None, None, None)
  assert rc == -1  # WBX_ERR_INVALID
  assert 'wbx_ens_rps_partial: ctx is NULL' in lib.wbx_last_error().decode()
  with pytest.raises(_hip.WbxError, match='ctx is NULL'):
    _hip.check(rc, 'wbx_ens_rps_partial')


def test_header_enum_matches_the_binding():
  with open(os.path.join(ROOT, 'include', 'wbx.h')) as f:
    header = f.read()
  assert int(re.search(r'WBX_FN_ENS_RPS_PARTIAL\s*=\s*(\d+)', header).group(1)) == _hip.FN_IDS['wbx_ens_rps_partial'] == 21
  assert int(re.search(r'#define WBX_ERPS_MAX_THRESHOLDS (\d+)', header).group(1)) == _hip.ERPS_MAX_THRESHOLDS == 16
  assert int(re.search(r'#define WBX_ERPS_MAX_MEMBERS (\d+)', header).group(1)) == _hip.ERPS_MAX_MEMBERS == 256
  assert int(re.search(r'#define WBX_ABI_VERSION (\d+)', header).group(1)) == 13
  assert len(set(_hip.FN_IDS.values())) == len(_hip.FN_IDS)
  # prototype: ctx, plan, dtype, M, member_stride, nthr, p_thresholds, t_thresholds, right_inclusive, p, t, mask, partial_out
  assert len(_hip.load_library() and _hip.PROTOS['wbx_ens_rps_partial']) == 13
  # a point's numerator fits the kernel's int32
  assert _hip.ERPS_MAX_THRESHOLDS * (_hip.ERPS_MAX_MEMBERS - 1) * _hip.ERPS_MAX_MEMBERS ** 2 < 2 ** 31


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_oracle_point_by_point():
  """400 random cases (M 2..69, K 1..16, the four fair / inclusive settings), values on a grid shared with the thresholds so that
  ties occur: |restatement - oracle| <= 16 K eps."""
  rng = np.random.default_rng(2024)
  worst = 0.0
  for case in range(400):
    m, k = int(rng.integers(2, 70)), int(rng.integers(1, 17))
    fair, right = bool(case & 1), bool(case & 2)
    thr = rng.integers(-12, 13, size=k) / 8.0
    p = (rng.integers(-16, 17, size=(m, 6)) / 8.0).astype(np.float32 if case & 4 else np.float64)
    t = (rng.integers(-16, 17, size=6) / 8.0).astype(p.dtype)
    if case % 5 == 0:
      p[:, 0], p[:, 1] = -np.inf, np.inf  # c = M and c = 0
    got = EC.rps_points(p, t, thr, thr, fair, right)
    want = np.array([O.ensemble_rps(p[:, j], t[j], thr, fair=fair, right_inclusive=right) for j in range(6)])
    err = float(np.abs(got - want).max())
    worst = max(worst, err)
    assert err <= 16 * k * EPS, (case, m, k, fair, right, err)
  print(f'worst |restatement - oracle| over 400 cases: {worst / EPS:.2f} eps')
  # NaN: a member or the target
  p = np.zeros((4, 3), np.float32)
  t = np.zeros(3, np.float32)
  p[2, 0], t[1] = np.nan, np.nan
  np.testing.assert_array_equal(np.isnan(EC.rps_points(p, t, [0.0], [0.0], True, True)), [True, True, False])
  # two lists: every point's target against b, its members against a
  a, b = EC.thresholds(5)
  p = (rng.integers(-16, 17, size=(9, 50)) / 8.0)
  t = (rng.integers(-16, 17, size=50) / 8.0)
  for fair in (True, False):
    want = np.zeros(50)
    for ak, bk in zip(a, b):
      cp, ct = (p <= ak).astype(np.float64), (t <= bk).astype(np.float64)
      want += (cp.mean(axis=0) - ct) ** 2 - (cp.var(axis=0, ddof=1) / 9 if fair else 0.0)
    np.testing.assert_allclose(EC.rps_points(p, t, a, b, fair, True), want, rtol=0, atol=16 * 5 * EPS)


def _round_down(thr):
  """float64 thresholds -> float32 rounded toward -inf."""
  with np.errstate(over='ignore'):
    f = np.asarray(thr, np.float64).astype(np.float32)
  up = f.astype(np.float64) > thr
  return np.where(up, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def _round_up(thr):
  with np.errstate(over='ignore'):
    f = np.asarray(thr, np.float64).astype(np.float32)
  down = f.astype(np.float64) < thr
  return np.where(down, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def test_float32_comparisons_against_directed_roundings_decide_like_float64():
  """`<=` against the threshold rounded toward -inf and `<` against the threshold rounded toward +inf agree with the float64
  comparison for every float32 value; rounding to nearest does not."""
  rng = np.random.default_rng(7)
  thr = np.concatenate([rng.normal(size=190), rng.normal(size=100) * 1e-3, rng.normal(size=98) * 1e30,
                        [0.1, -0.1, 0.0, -0.0, 1e40, -1e40, np.inf, -np.inf, 1e-50, -1e-50, 3.4028235677973366e38, 0.125]])
  assert thr.size == 400
  x = np.concatenate([rng.normal(size=9000).astype(np.float32), (rng.normal(size=5000) * 1e-3).astype(np.float32),
                      (rng.normal(size=1000) * 1e30).astype(np.float32)])
  near = thr[np.isfinite(thr) & (np.abs(thr) < 3e38)].astype(np.float32)  # the float32 neighbours of the thresholds
  x = np.concatenate([x, near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf)),
                      np.array([np.inf, -np.inf, 0.0, -0.0, np.float32(0.1), np.finfo(np.float32).max, -np.finfo(np.float32).max,
                                np.finfo(np.float32).tiny, 1e-45, -1e-45], np.float32)]).astype(np.float32)
  x = np.concatenate([x, rng.normal(size=20000 - x.size).astype(np.float32)]) if x.size < 20000 else x[:20000]
  assert x.size == 20000 and x.dtype == np.float32
  rd, ru = _round_down(thr), _round_up(thr)
  x64 = x.astype(np.float64)[:, None]
  np.testing.assert_array_equal(x[:, None] <= rd[None, :], x64 <= thr[None, :])
  np.testing.assert_array_equal(x[:, None] < ru[None, :], x64 < thr[None, :])
  with np.errstate(over='ignore'):
    nearest = thr.astype(np.float32)
  assert ((x[:, None] <= nearest[None, :]) != (x64 <= thr[None, :])).any()
  assert np.float32(0.1) <= np.float64(0.1).astype(np.float32) and not np.float64(np.float32(0.1)) <= 0.1
  # beyond the float32 range
  assert rd[thr == 1e40][0] == np.finfo(np.float32).max and ru[thr == 1e40][0] == np.inf
  assert rd[thr == -1e40][0] == -np.inf and ru[thr == -1e40][0] == -np.finfo(np.float32).max


def test_cases_hold_the_edges_and_the_nan_caps():
  for nthr in (1, 3, 5, 16):
    a, b = EC.thresholds(nthr)
    assert a.size == b.size == nthr and not np.isnan(a).any() and not np.isnan(b).any()
  a, b = EC.thresholds(3)
  assert len(set(a)) < 3 and (np.diff(a) < 0).any()  # a duplicate, unsorted
  a, b = EC.thresholds(5)
  assert (a != b).any()
  a, b = EC.thresholds(16)
  for v in (np.inf, -np.inf, 1e40, -1e40, 0.1, 0.125):
    assert v in a and v in b
  assert any(v == 0 and not np.signbit(v) for v in a) and any(v == 0 and np.signbit(v) for v in a)
  for flags in (0, EC.FLAG_MASKED, EC.FLAG_SKIPNA, EC.FLAG_MASKED | EC.FLAG_SKIPNA):
    for x_kept in (False, True):
      for dc in (5, 2):
        p, t, mask = EC.ens_rps_case(3, 9, 2, 5, 65, np.float32, flags, dc, x_kept, a)
        want, stat = EC.expected(p, t, a, b, True, True, mask, flags, dc, x_kept)
        c = EC.counts(p, a, True)
        assert (c == 9).all(axis=-1).any() and (c[..., np.isfinite(a)] == 0).all(axis=-1).any()  # c = M everywhere; no member below
        nan_p, nan_t = np.isnan(p).any(axis=0), np.isnan(t)
        if flags & EC.FLAG_SKIPNA:  # NaN in a member only, in the target only and in both; every output finite
          assert np.isnan(stat).any() and np.isfinite(want).all()
          assert (nan_p & ~nan_t).any() and (nan_t & ~nan_p).any() and (nan_p & nan_t).any()
        else:  # (two partials hold no NaN at all: a fifth of them is less than one)
          assert np.isfinite(want[:, :, 0]).mean() >= 0.8
          assert np.isnan(want).any() == (x_kept or dc == 2) and np.isnan(stat).any() == (x_kept or dc == 2 or bool(flags))
        assert want.shape == (2, -(-5 // dc), 1 if not flags else 2, 65 if x_kept else 1)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _inputs(dtype=np.float32, nans=False, mask=False, seed=41, variables=('v',), m=M, shape=SHAPE):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(shape[0]), 'latitude': np.linspace(-70, 70, shape[1]), 'longitude': np.arange(shape[2]) * (360.0 / shape[2])}
  pred, targ = {}, {}
  for v in variables:
    p = (np.round(rng.gamma(2.0, size=(m,) + shape) * 4) / 4).astype(dtype)  # ties with the thresholds
    t = (np.round(rng.gamma(2.0, size=shape) * 4) / 4).astype(dtype)
    if nans:
      p[rng.random(p.shape) < 0.01] = np.nan
      t[rng.random(shape) < 0.05] = np.nan
    tc = dict(cs)
    if mask:
      tc['mask'] = (DIMS[1:], rng.random(shape[1:]) > 0.3)
    pred[v] = xr.DataArray(p, dims=('number',) + DIMS, coords=dict(cs, number=np.arange(m)), name=v)
    targ[v] = xr.DataArray(t, dims=DIMS, coords=tc, name=v)
  return pred, targ


def _rps(thresholds=THR, target_thresholds=None, **kw):
  return probabilistic.EnsembleRankedProbabilityScore(thresholds, thresholds if target_thresholds is None else target_thresholds,
                                                      'bin', 's', **kw)


# ---- host logic of the fused route, the launch stood in for -----------------------------------------------------------------------
def _run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=0, ens=None, cat=None, inputs=None, fold=None):
  """fake_device._run_s1 + kind 'erps': the partials of wbx_ens_rps_partial from the integer restatement."""
  if kind != 'erps':
    return fake_device._run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=func, ens=ens, cat=cat, inputs=inputs, fold=fold)  # pylint: disable=protected-access
  m, mstride = ens
  nthr, a, b, right = cat
  a, b = np.asarray(a.ptr, np.float64), np.asarray(b.ptr, np.float64)
  assert a.shape == b.shape == (nthr,) and nthr <= _hip.ERPS_MAX_THRESHOLDS and 1 <= m <= _hip.ERPS_MAX_MEMBERS
  assert plan.plane_rows == 0 and plan.x_weights is None and not plan.flags & ~(_hip.FLAG_MASKED | _hip.FLAG_SKIPNA | _hip.FLAG_FAIR)
  fair = bool(plan.flags & _hip.FLAG_FAIR)
  if engine.S1_EVENT_LOG is not None:
    engine.S1_EVENT_LOG.append({'kind': kind, 'flags': int(plan.flags), 'ms': 0.0, 'x_kept': plan.x_kept, 'nthr': nthr, 'vec': plan.vec,
                                'right': bool(right), 'thresholds': (a.tobytes(), b.tobytes())})
  off = fake_device._offsets(plan, 0)  # pylint: disable=protected-access
  p = np.stack([devs[0].ptr[off + k * mstride] for k in range(m)], axis=0)
  t = devs[1].ptr[fake_device._offsets(plan, 1)]  # pylint: disable=protected-access
  stat = EC.numerators(p, t, a, b, fair, bool(right)).astype(np.float64)  # integers; [key, depth, x]
  stat[EC.nan_points(p, t)] = np.nan
  valid = np.ones(stat.shape, bool)
  if plan.flags & _hip.FLAG_MASKED:
    valid = devs[3].ptr[fake_device._offsets(plan, 3)] != 0  # pylint: disable=protected-access
  chunked = fake_device._chunked  # pylint: disable=protected-access
  denom = EC.denominator(m, fair)
  with np.errstate(all='ignore'):
    if plan.flags & _hip.FLAG_SKIPNA:
      ok = valid & ~np.isnan(stat)
      cols = [chunked(plan, np.where(ok, stat, 0.0)) / denom, chunked(plan, ok.astype(np.float64))]
    elif plan.flags & _hip.FLAG_MASKED:
      cols = [chunked(plan, np.where(valid, stat, 0.0)) / denom, chunked(plan, valid.astype(np.float64))]
    else:
      cols = [chunked(plan, stat) / denom]
  partial = np.stack(cols, axis=2)
  assert partial.shape[2] == nlanes_total
  return fake_device._Buf(partial.reshape(plan.partial_shape(nlanes_total)))  # pylint: disable=protected-access


@pytest.fixture
def fused(monkeypatch):
  """The emulated backend with the launch available: what a device context whose library exports the symbol gives."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(engine, '_run_s1', _run_s1)
  monkeypatch.setattr(engine, 'ens_rps_available', lambda ctx: True)
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  yield monkeypatch
  engine.clear_caches()


def _launches(kind='erps'):
  return [e for e in engine.S1_EVENT_LOG if e['kind'] == kind]


def _is_fused(stat):
  return isinstance(stat, lazy.LazyStatistic) and stat._group.kind == 'erps'  # pylint: disable=protected-access


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_plain_thresholds_give_a_lazy_statistic_with_the_host_routes_values(fused, dtype):
  pred, targ = _inputs(dtype, nans=True, mask=True)
  for fair in (True, False):
    for right in (True, False):
      for values in (THR, tuple(THR), np.array(THR), [1, 2.5, np.float32(3.5)], [0.25]):
        stat = _rps(values, fair=fair, right_inclusive=right).compute(pred, targ)['v']
        assert _is_fused(stat) and stat.is_lazy and stat._lane == 0 and stat.name == 'v'  # pylint: disable=protected-access
        assert stat.dims == DIMS and stat.shape == SHAPE and stat.dtype == np.float64
        assert tuple(stat.coords['mask'].dims) == DIMS[1:] and 'number' not in stat.coords
        fused.setattr(lazy, 'FUSED_ENS_RPS', False)
        want = _rps(values, fair=fair, right_inclusive=right).compute(pred, targ)['v']
        fused.setattr(lazy, 'FUSED_ENS_RPS', True)
        assert not _is_fused(want) and tuple(want.dims) == DIMS and str(want.dtype) == 'float64'
        assert set(stat.coords) == set(want.coords)
        got = np.asarray(stat.values)
        assert not stat.is_lazy and got.dtype == np.float64
        np.testing.assert_array_equal(got, np.asarray(want.values))  # bit for bit, NaN positions included
        assert np.isnan(got).any() and np.isfinite(got).any()
        # ... which is the restatement's number
        np.testing.assert_allclose(got, EC.rps_points(pred['v'].values, targ['v'].values, list(values), list(values), fair, right),
                                   rtol=0, atol=16 * len(values) * EPS)
  assert not _launches()  # reading values launches nothing of the new kind
  # statistics with the same tables share a group; other tables, fair or inclusive settings have their own
  s1, s2 = _rps().compute(pred, targ)['v'], _rps().compute(pred, targ)['v']
  assert s1._group is s2._group  # pylint: disable=protected-access
  for other in (_rps([0.5, 1.0]), _rps(fair=False), _rps(right_inclusive=False)):
    assert other.compute(pred, targ)['v']._group is not s1._group  # pylint: disable=protected-access
  # targets on fewer dims than the predictions
  t0 = {'v': targ['v'].isel(time=0, drop=True)}
  assert _is_fused(_rps().compute(pred, t0)['v'])


def test_everything_else_keeps_the_host_route(fused):
  pred, targ = _inputs()
  labelled = xr.DataArray(np.array(THR), dims=['bin'], coords={'bin': np.arange(3)})
  m1 = {'v': pred['v'].isel(number=slice(0, 1))}
  ens_t = {'v': xr.DataArray(np.asarray(pred['v'].values)[:3], dims=('number',) + DIMS, coords=dict(targ['v'].coords, number=np.arange(3)), name='v')}
  nan_thr = [0.5, np.nan, 2.5]
  k17 = list(np.arange(17) * 0.25)
  not_eligible = [
      ('labelled thresholds', probabilistic.EnsembleRankedProbabilityScore(labelled, labelled, 'bin', 's'), pred, targ),
      ('labelled per variable', probabilistic.EnsembleRankedProbabilityScore(xr.Dataset({'v': labelled}), xr.Dataset({'v': labelled}), 'bin', 's'), pred, targ),
      ('a NaN threshold', _rps(nan_thr, enforce_monotonicity=False), pred, targ),
      ('skipna_ensemble', _rps(skipna_ensemble=True), pred, targ),
      ('ensemble-valued targets', _rps(), pred, ens_t),
      ('17 thresholds', _rps(k17), pred, targ),
      ('one member, fair', _rps(), m1, targ),
      ('thresholds that are no numbers', _rps([True, 2.0], enforce_monotonicity=False), pred, targ),
      ('two different lists', _rps(THR, [0.5, 1.0, 2.0]), pred, targ),
      ('a generator', probabilistic.EnsembleRankedProbabilityScore((x for x in THR), (x for x in THR), 'bin', 's'), pred, targ),
  ]
  for what, stat, p, t in not_eligible:
    with np.errstate(all='ignore'):
      out = stat.compute(p, t)['v']
      np.asarray(out.values)
    assert not _is_fused(out), what
    assert not _launches(), what
  assert _is_fused(_rps(fair=False).compute(m1, targ)['v'])  # one member, unfair: fine
  # integer payloads; the bin dim on an input
  ints = {'v': xr.DataArray(np.asarray(pred['v'].values).astype(np.int32), dims=pred['v'].dims, coords=dict(pred['v'].coords), name='v')}
  assert not _is_fused(_rps().compute(ints, targ)['v'])
  assert not _is_fused(probabilistic.EnsembleRankedProbabilityScore(THR, THR, 'time', 's')._fused_per_variable(pred['v'], targ['v']) or 0)  # pylint: disable=protected-access
  # a sequence that is not increasing raises as before
  with pytest.raises(ValueError, match='monotonically increasing'):
    np.asarray(_rps([1.0, 0.5]).compute(pred, targ)['v'].values)
  assert _is_fused(_rps([1.0, 0.5, 1.0], enforce_monotonicity=False).compute(pred, targ)['v'])
  # the switch
  fused.setattr(lazy, 'FUSED_ENS_RPS', False)
  assert not _is_fused(_rps().compute(pred, targ)['v'])
  fused.setattr(lazy, 'FUSED_ENS_RPS', True)
  # a context without the symbol
  fused.setattr(engine, 'ens_rps_available', lambda ctx: False)
  assert not _is_fused(_rps().compute(pred, targ)['v'])
  metrics = {'rps': _StatisticAsMetric(_rps())}
  _evaluate(metrics, pred, targ, aggregation.Aggregator(reduce_dims=list(DIMS)))
  assert not _launches() and engine.S1_EVENT_LOG


def test_a_context_without_the_library_keeps_the_host_route(monkeypatch):
  """The gate as shipped: the plan interpreter's context is no _hip.Context, so nothing asks it for the new launch."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  assert not engine.ens_rps_available(_hip.default_context())
  assert not engine.ens_rps_available(object())
  pred, targ = _inputs()
  log = []
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', log)
  stats, _, values = _evaluate({'rps': _StatisticAsMetric(_rps())}, pred, targ, aggregation.Aggregator(reduce_dims=list(DIMS)))
  assert not any(_is_fused(s) for per_var in stats.values() for s in per_var.values())
  assert log and not [e for e in log if e['kind'] == 'erps']
  want = EC.rps_points(pred['v'].values, targ['v'].values, THR, THR, True, True).mean()
  np.testing.assert_allclose(float(np.asarray(values['rps.v'].values)), want, rtol=0, atol=16 * 3 * EPS)
  engine.clear_caches()


def test_unique_name_does_not_change():
  assert _rps().unique_name == 'RankedProbabilityScore_number_skipna_ensemble_False_fair_True_s'
  assert _rps(fair=False, right_inclusive=False).unique_name == 'RankedProbabilityScore_number_skipna_ensemble_False_fair_False_s'


def test_pickling_of_the_statistic_and_of_the_lazy_result(fused):
  pred, targ = _inputs(nans=True, mask=True)
  stat_obj = _rps()
  again = pickle.loads(pickle.dumps(stat_obj))
  assert again.unique_name == stat_obj.unique_name
  stat = again.compute(pred, targ)['v']
  assert _is_fused(stat) and stat.is_lazy
  back = pickle.loads(pickle.dumps(stat))  # materialises on the host route
  fused.setattr(lazy, 'FUSED_ENS_RPS', False)
  want = stat_obj.compute(pred, targ)['v']
  assert tuple(back.dims) == DIMS and str(back.dtype) == 'float64' and not isinstance(back, lazy.LazyStatistic)
  np.testing.assert_array_equal(np.asarray(back.values), np.asarray(want.values))
  np.testing.assert_array_equal(np.asarray(back.coords['mask'].values), np.asarray(targ['v'].coords['mask'].values))
  assert not _launches()


# ---- through the Aggregator -------------------------------------------------------------------------------------------------------
class _StatisticAsMetric(metrics_base.PerVariableMetric):

  def __init__(self, statistic):
    self._statistic = statistic

  @property
  def statistics(self):
    return {'s': self._statistic}

  def _values_from_mean_statistics_per_variable(self, statistic_values):
    return statistic_values['s']


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


REGIONS = {'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180)), 'nowhere-much': ((60, 90), (300, 360))}
# name -> (reduce_dims, the other arguments of the Aggregator)
AGGREGATORS = {
    'plain': (DIMS, lambda: {}),
    'keep-latitude': (('time', 'longitude'), lambda: {}),
    'keep-longitude': (('time', 'latitude'), lambda: {}),
    'area': (DIMS, lambda: dict(weigh_by=[weighting.GridAreaWeighting()])),
    'regions+area': (DIMS, lambda: dict(weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)])),
    'latitude-bins+masked': (DIMS, lambda: dict(bin_by=[binning.LatitudeBins(30)], masked=True)),
    'masked': (DIMS, lambda: dict(masked=True)),
    'masked-keeping-the-mask': (('time',), lambda: dict(masked=True)),
    'skipna': (('time', 'longitude'), lambda: dict(skipna=True)),
    'masked+skipna+area': (DIMS, lambda: dict(masked=True, skipna=True, weigh_by=[weighting.GridAreaWeighting()])),
}


def _aggregator(which):
  reduce_dims, kw = AGGREGATORS[which]
  return aggregation.Aggregator(reduce_dims=list(reduce_dims), **kw())


def _points_per_output(which):
  """The product of the sizes of the dims the aggregator reduces: no output sums more points (bins and masks leave fewer)."""
  return int(np.prod([SHAPE[DIMS.index(d)] for d in AGGREGATORS[which][0]]))


def _assert_like_the_host_route(which, nthr, name, variables, state, state0, values, values0):
  """Sums within 16 K eps x (points per output) x (the largest weight, where the aggregator weighs), weights the same numbers in
  another order, coordinates equal.  The metric values are weighted means with non-negative weights of per-point values that differ
  by at most 16 K eps each: they differ by at most 16 K eps whatever the number of points."""
  bound = 16 * nthr * EPS * _points_per_output(which) * _max_weight(which)
  for var in variables:
    for tree, tree0, tol in ((state.sum_weighted_statistics, state0.sum_weighted_statistics, bound), (state.sum_weights, state0.sum_weights, 0.0)):
      x, y = tree[name][var], tree0[name][var]
      assert tuple(x.dims) == tuple(y.dims), (var, x.dims, y.dims)
      _assert_same_coords(x, y, f'{which} {var}')
      if tol:
        np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=0, atol=tol, equal_nan=True, err_msg=f'{which} {var}')
      else:
        np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=1e-12, atol=0, err_msg=f'{which} {var} weights')
    # (NaNs are in the skipna cases only, where they are counted out: every sum is finite)
    assert np.isfinite(np.asarray(state.sum_weighted_statistics[name][var].values)).all(), (which, var)
  assert set(values) == set(values0)
  for key in values:
    assert tuple(values[key].dims) == tuple(values0[key].dims)
    _assert_same_coords(values[key], values0[key], key)
    np.testing.assert_allclose(np.asarray(values[key].values), np.asarray(values0[key].values), rtol=0, atol=16 * nthr * EPS, equal_nan=True, err_msg=key)


def _assert_same_coords(x, y, what):
  assert set(x.coords) == set(y.coords), (what, sorted(map(str, x.coords)), sorted(map(str, y.coords)))
  for name in x.coords:
    assert tuple(x.coords[name].dims) == tuple(y.coords[name].dims), (what, name)
    np.testing.assert_array_equal(np.asarray(x.coords[name].values), np.asarray(y.coords[name].values), err_msg=f'{what}: coordinate {name}')


def _max_weight(which):
  if 'area' not in which:
    return 1.0
  probe = xr.DataArray(np.zeros(SHAPE[1:]), dims=DIMS[1:], coords={d: _inputs()[0]['v'].coords[d].values for d in DIMS[1:]})
  return float(np.asarray(weighting.GridAreaWeighting().weights(probe).values).max())


@pytest.mark.parametrize('fair', [True, False], ids=['fair', 'unfair'])
@pytest.mark.parametrize('which', list(AGGREGATORS))
def test_one_launch_per_variable_and_the_host_routes_numbers(fused, which, fair):
  nans = 'skipna' in which
  pred, targ = _inputs(nans=nans, mask='masked' in which, variables=('u', 'v'))
  metrics = {'rps': _StatisticAsMetric(_rps(fair=fair))}
  stats, state, values = _evaluate(metrics, pred, targ, _aggregator(which))
  assert all(_is_fused(s) and s.is_lazy for per_var in stats.values() for s in per_var.values())
  assert len(_launches()) == 2 and len(engine.S1_EVENT_LOG) == 2, engine.S1_EVENT_LOG  # one per variable, nothing else
  assert all(bool(e['flags'] & _hip.FLAG_FAIR) == fair for e in _launches())
  # the same evaluation on the host route
  fused.setattr(lazy, 'FUSED_ENS_RPS', False)
  fused.setattr(engine, 'S1_EVENT_LOG', [])
  stats0, state0, values0 = _evaluate(metrics, pred, targ, _aggregator(which))
  assert not any(_is_fused(s) for per_var in stats0.values() for s in per_var.values()) and not _launches()
  _assert_like_the_host_route(which, len(THR), _rps(fair=fair).unique_name, ('u', 'v'), state, state0, values, values0)
  name = _rps(fair=fair).unique_name
  if which == 'masked-keeping-the-mask':
    assert 'mask' in state.sum_weighted_statistics[name]['v'].coords


@pytest.mark.parametrize('which', ['plain', 'keep-latitude', 'regions+area', 'masked+skipna+area'])
def test_a_list_with_a_duplicate_counts_it_twice_like_the_host_route(fused, which):
  """[1.0, 0.5, 1.0] on both sides, enforce_monotonicity=False: the host route's two transforms carry the duplicate label on both
  sides and sum three terms, as the kernel does."""
  thr = [1.0, 0.5, 1.0]
  pred, targ = _inputs(nans='skipna' in which, mask='masked' in which)
  for fair in (True, False):
    stat = lambda: _rps(thr, fair=fair, enforce_monotonicity=False)
    metrics = {'rps': _StatisticAsMetric(stat())}
    fused.setattr(lazy, 'FUSED_ENS_RPS', True)
    fused.setattr(engine, 'S1_EVENT_LOG', [])
    stats, state, values = _evaluate(metrics, pred, targ, _aggregator(which))
    assert all(_is_fused(s) for per_var in stats.values() for s in per_var.values()) and [e['nthr'] for e in _launches()] == [3]
    fused.setattr(lazy, 'FUSED_ENS_RPS', False)
    fused.setattr(engine, 'S1_EVENT_LOG', [])
    stats0, state0, values0 = _evaluate(metrics, pred, targ, _aggregator(which))
    assert not any(_is_fused(s) for per_var in stats0.values() for s in per_var.values()) and not _launches()
    _assert_like_the_host_route(which, 3, stat().unique_name, ('v',), state, state0, values, values0)
    if which == 'plain':  # ... which is twice the 1.0 term plus the 0.5 term
      want = (2 * EC.rps_points(pred['v'].values, targ['v'].values, [1.0], [1.0], fair, True) + EC.rps_points(pred['v'].values, targ['v'].values, [0.5], [0.5], fair, True)).mean()
      np.testing.assert_allclose(float(np.asarray(values['rps.v'].values)), want, rtol=0, atol=16 * 3 * EPS)


def test_without_a_device_the_gate_declines_instead_of_raising(monkeypatch):
  """No device or no library: _hip.default_context raises.  The gate then answers "host route" (where the same error comes from
  the first kernel the host route itself needs, as it did before the fused route existed) and never raises on its own."""
  def no_device(device_id=None):
    raise _hip.WbxUnavailableError('no HIP device visible')
  monkeypatch.setattr(_hip, 'default_context', no_device)
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', True)
  pred, targ = _inputs()
  for fair in (True, False):
    assert _rps(fair=fair)._fused_per_variable(pred['v'], targ['v']) is None  # pylint: disable=protected-access
  # the gate declined: with a backend for the host route's own kernels the statistic is the host route's, values and all
  engine.clear_caches()
  calls = []
  ctx = fake_device.FakeCtx()

  def only_for_the_host_route(device_id=None):
    import traceback  # pylint: disable=g-import-not-at-top
    if any(f.name == '_fused_per_variable' for f in traceback.extract_stack()[-3:]):
      calls.append('gate')
      raise _hip.WbxUnavailableError('no HIP device visible')
    return ctx
  fake_device.install(monkeypatch)
  monkeypatch.setattr(_hip, 'default_context', only_for_the_host_route)
  out = _rps().compute(pred, targ)['v']
  assert calls == ['gate'] and not _is_fused(out)
  np.testing.assert_allclose(np.asarray(out.values), EC.rps_points(pred['v'].values, targ['v'].values, THR, THR, True, True), rtol=0, atol=16 * 3 * EPS)
  engine.clear_caches()


def test_plain_sum_is_the_restatements_integer_sum(fused):
  """Without weights the launch's sums are float64(S) / float64(D), whatever the chunking of stage 1."""
  del fused
  pred, targ = _inputs()
  for fair in (True, False):
    _, state, _ = _evaluate({'rps': _StatisticAsMetric(_rps(fair=fair))}, pred, targ, aggregation.Aggregator(reduce_dims=list(DIMS)))
    got = float(np.asarray(state.sum_weighted_statistics[_rps(fair=fair).unique_name]['v'].values))
    s = int(EC.numerators(pred['v'].values, targ['v'].values, THR, THR, fair, True).sum())
    np.testing.assert_allclose(got, s / EC.denominator(M, fair), rtol=4 * EPS, atol=0)  # (stage 2 adds a few partials)
    assert float(np.asarray(state.sum_weights[_rps(fair=fair).unique_name]['v'].values)) == float(np.prod(SHAPE))


def test_different_thresholds_launch_twice_identical_ones_once(fused):
  del fused
  pred, targ = _inputs()
  agg = aggregation.Aggregator(reduce_dims=list(DIMS))
  metrics = {'a': _StatisticAsMetric(_rps(THR)), 'b': _StatisticAsMetric(probabilistic.EnsembleRankedProbabilityScore([0.5, 2.0], [0.5, 2.0], 'bin', 'other'))}
  stats, _, values = _evaluate(metrics, pred, targ, agg)
  assert len(stats) == 2 and len(_launches()) == 2
  assert sorted(e['nthr'] for e in _launches()) == [2, 3]
  assert float(np.asarray(values['a.v'].values)) != float(np.asarray(values['b.v'].values))
  # two statistics (different suffixes: two entries) of one pair with identical thresholds meet in one group: one launch
  engine.S1_EVENT_LOG.clear()
  pred, targ = _inputs()
  metrics = {'a': _StatisticAsMetric(_rps(THR)), 'b': _StatisticAsMetric(probabilistic.EnsembleRankedProbabilityScore(list(THR), tuple(THR), 'bin', 'other'))}
  stats, _, values = _evaluate(metrics, pred, targ, agg)
  assert len(stats) == 2 and len(_launches()) == 1, engine.S1_EVENT_LOG
  assert float(np.asarray(values['a.v'].values)) == float(np.asarray(values['b.v'].values))
  # ... and fair against unfair, or right- against left-inclusive, are launches of their own
  engine.S1_EVENT_LOG.clear()
  pred, targ = _inputs()
  metrics = {'a': _StatisticAsMetric(_rps(THR)), 'b': _StatisticAsMetric(_rps(THR, fair=False)),
             'c': _StatisticAsMetric(probabilistic.EnsembleRankedProbabilityScore(THR, THR, 'bin', 'left', right_inclusive=False))}
  _evaluate(metrics, pred, targ, agg)
  assert len(_launches()) == 3
  assert sorted((bool(e['flags'] & _hip.FLAG_FAIR), e['right']) for e in _launches()) == [(False, True), (True, False), (True, True)]
