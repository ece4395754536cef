"""MSE, RMSE, MAE and Bias of event probabilities (the Brier score and its kin) through the public API on the device:
compute_unique_statistics_for_all_metrics + the Aggregator behind ContinuousToBinary('both') -> EnsembleMean, -> WeibullEnsembleTo-
Probabilistic and behind ContinuousToBinary('both') alone, on small fields (7 members, 4 x 13 x 24) under a plain reduction,
GridAreaWeighting with Regions x land / sea bins, a target mask, and skipna with NaNs; torch-resident payloads; a recorded and
replayed chunk loop; accumulation over chunks.

Bounds.  Tight check, against the exact restatement (tests/brier_cases.py: one correctly rounded float64 quotient per point) pushed
through the oracle's float64 weighted sum.  A per-point value is at most 1 in magnitude and a weighted term at most wmax, the largest
weight (1 where the aggregator does not weigh).  The fused route adds integers exactly and rounds once per partial, the restatement
once per point: either is within 2^-53 of the exact rational per point it holds.  Each side then rounds once per product with a
weight and once per float64 addition, a 2^-53 of a term each to first order.  An output that sums N points -- N = the product of
the sizes of the dims the aggregator reduces -- is therefore within 16 * eps * N * wmax (eps = 2^-52: eight such roundings per
point and side); sums of weights are the same numbers in another order (rtol 1e-12).
Route check, against the host route (lazy.FUSED_BRIER = False: the parent commit's arithmetic).  Its probability is a float32 mean
of float32 indicators, so the values agree within rtol = 1e-6, the tolerance the project grants that route
(tests/test_wrappers_more.py); dims, coordinates and NaN placement are identical.  A relative tolerance holds for a mean whose terms
do not cancel: every rounding of the host route is relative to a term (2^-24 of the probability c / 7, which float32 does not hold),
so MSE, RMSE and MAE -- means of non-negative terms -- agree within a few 2^-24 whatever the data.  Bias is a mean of signed terms:
behind the plotting position (c / 8) and behind the one transform (0 / 1) the host route's float32 terms are exact and so is the
comparison; behind the member mean it is compared on fields whose members are all at or above the target, where o = 1 implies c = M
and every error c - 7 o is >= 0, so that Bias does not cancel either (on the general fields Bias behind the member mean is held by
the tight check alone, which is absolute)."""
import numpy as np
import pytest

import brier_cases as BC
from oracle import wbx_oracle as O
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import binning
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import pipeline
from weatherbenchx_amd import replay
from weatherbenchx_amd import time_chunks
from weatherbenchx_amd import weighting
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import deterministic
from weatherbenchx_amd.metrics import wrappers

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
DIMS = ('time', 'latitude', 'longitude')
SHAPE = (4, 13, 24)
M = 7
THR = [0.1, 0.5, 1.0, 2.5, 4.0]
LAT = np.linspace(-90, 90, SHAPE[1])
LON = np.arange(SHAPE[2]) * (360.0 / SHAPE[2])
REGIONS = {'global': ((-90, 90), (0, 360)), 'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180))}
STAT_NAMES = ('Error', 'AbsoluteError', 'SquaredError')


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.brier_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


def _outer(thr=None):
  return wrappers.ContinuousToBinary('both', THR if thr is None else thr, 'threshold')


# form -> (the transforms, the denominator, whether the predictions are an ensemble)
FORMS = {
    'mean': (lambda: [_outer(), wrappers.EnsembleMean('predictions', 'number')], M, True),
    'weibull': (lambda: [_outer(), wrappers.WeibullEnsembleToProbabilistic('predictions', 'number')], M + 1, True),
    'single': (lambda: [_outer()], 1, False),
}


def _metrics(chain):
  return {'mse': wrappers.WrappedMetric(deterministic.MSE(), chain()), 'rmse': wrappers.WrappedMetric(deterministic.RMSE(), chain()),
          'mae': wrappers.WrappedMetric(deterministic.MAE(), chain()), 'bias': wrappers.WrappedMetric(deterministic.Bias(), chain())}


def _unique_names(metrics):
  """base statistic name -> the unique name of the wrapped statistic."""
  out = {}
  for metric in metrics.values():
    for stat in metric.statistics.values():
      out[stat.unique_name.split('_')[0]] = stat.unique_name
  assert set(out) == set(STAT_NAMES), out
  return out


def _inputs(dtype=np.float32, nans=False, mask=False, seed=11, variables=('u', 'v'), ensemble=True, ordered=False):
  """`ordered`: every member at or above the target (the target plus a non-negative step that is 0 for many members)."""
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(SHAPE[0]), 'latitude': LAT, 'longitude': LON}
  pred, targ = {}, {}
  for v in variables:
    p = (np.round(rng.gamma(2.0, size=(M,) + SHAPE) * 4) / 4).astype(dtype)  # ties with the thresholds
    t = (np.round(rng.gamma(2.0, size=SHAPE) * 4) / 4).astype(dtype)
    if ordered:
      p = (t[None] + np.round(np.maximum(rng.normal(0.0, 1.5, size=(M,) + SHAPE), 0.0) * 4) / 4).astype(dtype)
      assert (p >= t[None]).all() and (p == t[None]).mean() > 0.3
    p[:4, 0, 0, 0] = [0.5, np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(0)), np.nextafter(np.float32(0.1), np.float32(1))]
    if nans:
      p[rng.random(p.shape) < 0.01] = np.nan
      t[rng.random(SHAPE) < 0.05] = np.nan
    tc = dict(cs)
    if mask:
      tc['mask'] = (DIMS[1:], rng.random(SHAPE[1:]) > 0.3)
    if ensemble:
      pred[v] = xr.DataArray(p, dims=('number',) + DIMS, coords=dict(cs, number=np.arange(M)), name=v)
    else:
      pred[v] = xr.DataArray(p[0], dims=DIMS, coords=cs, name=v)
    targ[v] = xr.DataArray(t, dims=DIMS, coords=tc, name=v)
  return pred, targ


def _members(da):
  """The values of the predictions with the member axis first (one member for a deterministic field)."""
  v = np.asarray(da.values)
  return v if 'number' in da.dims else v[None]


def _lsm():
  land = (np.sin(np.deg2rad(LON) * 3)[None, :] * np.cos(np.deg2rad(LAT) * 2.5)[:, None]) > 0.1
  return xr.DataArray(land, dims=DIMS[1:], coords={'latitude': LAT, 'longitude': LON})


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyBrier)


CASES = {
    'plain': dict(reduce=DIMS, kw=lambda: {}, nans=False, mask=False, area=False),
    'keep-longitude': dict(reduce=('time', 'latitude'), kw=lambda: {}, nans=False, mask=False, area=False),
    'area-weights': dict(reduce=('latitude', 'longitude'), kw=lambda: dict(weigh_by=[weighting.GridAreaWeighting()]), nans=False, mask=False, area=True),
    'regions-x-landsea': dict(reduce=DIMS, kw=lambda: dict(weigh_by=[weighting.GridAreaWeighting()],
                                                           bin_by=[binning.Regions(REGIONS), binning.LandSea(_lsm().astype(np.float64))]),
                              nans=False, mask=False, area=True, oracle=False),
    'masked': dict(reduce=DIMS, kw=lambda: dict(masked=True, weigh_by=[weighting.GridAreaWeighting()]), nans=False, mask=True, area=True),
    'skipna': dict(reduce=('time', 'longitude'), kw=lambda: dict(skipna=True), nans=True, mask=False, area=False),
}


def _aggregator(case):
  return aggregation.Aggregator(reduce_dims=list(case['reduce']), **case['kw']())


def _points_per_output(case):
  """The product of the sizes of the reduced dims: no output sums more points (bins and masks leave fewer)."""
  return int(np.prod([SHAPE[DIMS.index(d)] for d in case['reduce']]))


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('which', list(CASES))
def test_scores_against_the_restatement_and_the_host_route(monkeypatch, which, dtype, form):
  case = CASES[which]
  chain, denom, ensemble = FORMS[form]
  pred, targ = _inputs(dtype, nans=case['nans'], mask=case['mask'], ensemble=ensemble)
  metrics = _metrics(chain)
  names = _unique_names(metrics)
  monkeypatch.setattr(lazy, 'FUSED_BRIER', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(metrics, pred, targ, _aggregator(case))
  assert all(_is_fused(s) and s.is_lazy for per_var in stats.values() for s in per_var.values())
  launches = [e for e in engine.S1_EVENT_LOG if e['kind'] == 'brier']
  # three statistics of a variable: ONE launch; one launch per variable, nothing else
  assert len(launches) == 2 and len(engine.S1_EVENT_LOG) == 2, engine.S1_EVENT_LOG
  # ---- tight: the exact restatement through the oracle's float64 weighted sum
  if case.get('oracle', True):
    w = [(O.grid_area_weights(LAT), ('latitude',))] if case['area'] else []
    wmax = float(O.grid_area_weights(LAT).max()) if case['area'] else 1.0
    bound = 16 * EPS * _points_per_output(case) * wmax
    sdims = DIMS + ('threshold',)
    for var in ('u', 'v'):
      pts = BC.points(_members(pred[var]), targ[var].values, THR, denom).reshape(SHAPE + (3, len(THR)))
      mask = np.asarray(targ[var].coords['mask'].values, bool) if case['mask'] else None
      for lane, sname in enumerate(STAT_NAMES):
        sws, sw, od = O.aggregate(pts[..., lane, :], sdims, case['reduce'], weights=w, mask=mask, mask_dims=DIMS[1:], skipna=case['nans'])
        x = state.sum_weighted_statistics[names[sname]][var]
        assert set(x.dims) == set(od), (x.dims, od)
        got = np.asarray(x.transpose(*od).values)
        print(which, form, var, sname, 'max |fused - restatement| of the sums:', float(np.nanmax(np.abs(got - sws))), 'bound', bound)
        np.testing.assert_allclose(got, sws, rtol=0, atol=bound, err_msg=f'{which} {form} {var} {sname} sums')
        np.testing.assert_allclose(np.asarray(state.sum_weights[names[sname]][var].transpose(*od).values), sw, rtol=1e-12, atol=0)
  # ---- the same evaluation on the host route
  monkeypatch.setattr(lazy, 'FUSED_BRIER', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats0, state0, values0 = _evaluate(metrics, pred, targ, _aggregator(case))
  assert not any(_is_fused(s) for per_var in stats0.values() for s in per_var.values())
  assert not [e for e in engine.S1_EVENT_LOG if e['kind'] == 'brier']
  for sname in STAT_NAMES:
    for var in ('u', 'v'):
      for tree, tree0 in ((state.sum_weighted_statistics, state0.sum_weighted_statistics), (state.sum_weights, state0.sum_weights)):
        x, y = tree[names[sname]][var], tree0[names[sname]][var]
        assert tuple(x.dims) == tuple(y.dims) and set(x.coords) == set(y.coords), (sname, var, x.dims, y.dims)
        for k in y.coords:
          np.testing.assert_array_equal(np.asarray(x.coords[k].values), np.asarray(y.coords[k].values), err_msg=f'{sname} {var}: {k}')
  assert set(values) == set(values0) == {f'{m}.{v}' for m in metrics for v in ('u', 'v')}
  for key in values:
    a, b = values[key], values0[key]
    assert tuple(a.dims) == tuple(b.dims) and set(a.coords) == set(b.coords), key
    for k in b.coords:
      np.testing.assert_array_equal(np.asarray(a.coords[k].values), np.asarray(b.coords[k].values), err_msg=f'{key}: {k}')
    av, bv = np.asarray(a.values, np.float64), np.asarray(b.values, np.float64)
    np.testing.assert_array_equal(np.isnan(av), np.isnan(bv), err_msg=key)
    if form == 'mean' and key.startswith('bias'):
      continue  # (signed terms with float32 roundings: compared below, where they do not cancel)
    with np.errstate(all='ignore'):
      print(which, form, key, 'max relative |fused - host| of the values:', float(np.nanmax(np.abs(av - bv) / np.abs(bv))) if np.isfinite(bv).any() else None)
    np.testing.assert_allclose(av, bv, rtol=1e-6, atol=0, equal_nan=True, err_msg=key)


@pytest.mark.parametrize('which', list(CASES))
def test_bias_behind_the_member_mean_against_the_host_route(monkeypatch, which):
  """Fields whose members are all at or above the target: every error is >= 0, Bias is a mean of non-negative terms (and equals MAE),
  and the host route's float32 roundings are relative to it."""
  case = CASES[which]
  pred, targ = _inputs(nans=case['nans'], mask=case['mask'], ordered=True)
  for var in pred:
    p, t = np.asarray(pred[var].values), np.asarray(targ[var].values)
    p[:, 0, 0, 0] = t[0, 0, 0] + 0.25  # (the float32(0.1) probes of _inputs back in order)
    with np.errstate(invalid='ignore'):
      assert not (p < t[None]).any()
  metrics = _metrics(FORMS['mean'][0])
  monkeypatch.setattr(lazy, 'FUSED_BRIER', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, _, values = _evaluate(metrics, pred, targ, _aggregator(case))
  assert all(_is_fused(s) for per_var in stats.values() for s in per_var.values()) and len(engine.S1_EVENT_LOG) == 2
  monkeypatch.setattr(lazy, 'FUSED_BRIER', False)
  _, _, values0 = _evaluate(metrics, pred, targ, _aggregator(case))
  assert set(values) == set(values0)
  for key in values:
    av, bv = np.asarray(values[key].values, np.float64), np.asarray(values0[key].values, np.float64)
    assert tuple(values[key].dims) == tuple(values0[key].dims)
    np.testing.assert_array_equal(np.isnan(av), np.isnan(bv), err_msg=key)
    assert np.nanmin(bv) >= 0 and np.nanmax(bv) > 0, key
    np.testing.assert_allclose(av, bv, rtol=1e-6, atol=0, equal_nan=True, err_msg=key)
  for var in pred:
    np.testing.assert_allclose(np.asarray(values[f'bias.{var}'].values), np.asarray(values[f'mae.{var}'].values), rtol=1e-14, atol=0, equal_nan=True)


def test_more_than_sixteen_thresholds_are_cut_into_blocks(monkeypatch):
  thr = list(np.round(np.linspace(0.25, 6.0, 37), 3))
  pred, targ = _inputs(variables=('v',))
  chain = lambda: [_outer(thr), wrappers.EnsembleMean('predictions', 'number')]
  metrics = _metrics(chain)
  names = _unique_names(metrics)
  make = lambda: aggregation.Aggregator(reduce_dims=['latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])
  monkeypatch.setattr(lazy, 'FUSED_BRIER', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  _, state, _ = _evaluate(metrics, pred, targ, make())
  assert [e['kind'] for e in engine.S1_EVENT_LOG] == ['brier'] * 3
  pts = BC.points(_members(pred['v']), targ['v'].values, thr, M).reshape(SHAPE + (3, len(thr)))
  w = O.grid_area_weights(LAT)
  for lane, sname in enumerate(STAT_NAMES):
    sws, _, od = O.aggregate(pts[..., lane, :], DIMS + ('threshold',), ('latitude', 'longitude'), weights=[(w, ('latitude',))])
    x = state.sum_weighted_statistics[names[sname]]['v']
    np.testing.assert_array_equal(np.asarray(x.coords['threshold'].values), thr)
    np.testing.assert_allclose(np.asarray(x.transpose(*od).values), sws, rtol=0, atol=16 * EPS * SHAPE[1] * SHAPE[2] * float(w.max()))


def test_a_nan_under_a_valid_point_poisons_and_under_the_mask_does_not(monkeypatch):
  monkeypatch.setattr(lazy, 'FUSED_BRIER', True)
  metrics = _metrics(FORMS['mean'][0])
  name = _unique_names(metrics)['SquaredError']
  make = lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude'], masked=True)
  pred, targ = _inputs(mask=True, variables=('v',))
  valid = np.asarray(targ['v'].coords['mask'].values, bool)
  hidden, shown = np.argwhere(~valid)[0], np.argwhere(valid)[0]
  pred['v'].data[3, 2, hidden[0], hidden[1]] = np.nan  # one member, hidden
  _, state, _ = _evaluate(metrics, pred, targ, make())
  assert np.isfinite(np.asarray(state.sum_weighted_statistics[name]['v'].values)).all()
  pred, targ = _inputs(mask=True, variables=('v',))
  pred['v'].data[5, 1, shown[0], shown[1]] = np.nan  # one member, under a valid point
  _, state, _ = _evaluate(metrics, pred, targ, make())
  x = state.sum_weighted_statistics[name]['v']
  bad = np.isnan(np.asarray(x.transpose('latitude', 'threshold').values))
  assert bad[shown[0]].all() and not np.delete(bad, shown[0], axis=0).any()  # that latitude at every threshold, nothing else


def test_torch_resident_payloads_give_the_same_bits(monkeypatch):
  import torch  # pylint: disable=g-import-not-at-top
  monkeypatch.setattr(lazy, 'FUSED_BRIER', True)
  make = lambda: aggregation.Aggregator(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)])
  on_dev = lambda da: xr.DataArray(torch.as_tensor(np.asarray(da.values)).cuda(), dims=da.dims, coords={d: da.coords[d].values for d in da.dims}, name=da.name)
  for form, (chain, _, ensemble) in FORMS.items():
    metrics = _metrics(chain)
    names = _unique_names(metrics)
    pred, targ = _inputs(variables=('v',), ensemble=ensemble)
    _, state, _ = _evaluate(metrics, pred, targ, make())
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    stats, state_t, _ = _evaluate(metrics, {'v': on_dev(pred['v'])}, {'v': on_dev(targ['v'])}, make())
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', None)
    for name in names.values():
      assert _is_fused(stats[name]['v']), form
      np.testing.assert_array_equal(np.asarray(state_t.sum_weighted_statistics[name]['v'].values), np.asarray(state.sum_weighted_statistics[name]['v'].values))
      np.testing.assert_array_equal(np.asarray(state_t.sum_weights[name]['v'].values), np.asarray(state.sum_weights[name]['v'].values))


def test_values_read_from_the_lazy_statistic_are_the_host_routes(monkeypatch):
  """`.values` of a fused statistic is labelled-array arithmetic on the host: the numbers the host route's statistic evaluates to."""
  for form, (chain, _, ensemble) in FORMS.items():
    pred, targ = _inputs(nans=True, mask=True, variables=('v',), ensemble=ensemble)
    for cls in (deterministic.Error, deterministic.AbsoluteError, deterministic.SquaredError):
      stat = cls()
      for tr in reversed(chain()):
        stat = wrappers.WrappedStatistic(stat, tr)
      monkeypatch.setattr(lazy, 'FUSED_BRIER', True)
      got = stat.compute(pred, targ)['v']
      monkeypatch.setattr(lazy, 'FUSED_BRIER', False)
      want = stat.compute(pred, targ)['v']
      assert _is_fused(got) and not _is_fused(want)
      assert tuple(got.dims) == tuple(want.dims) and set(got.coords) == set(want.coords) and got.shape == want.shape
      a, b = np.asarray(got.values, np.float64), np.asarray(want.values, np.float64)
      np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
      # (float32 arithmetic on values of at most 1 on both sides: a few roundings of 2^-24)
      np.testing.assert_allclose(a, b, rtol=0, atol=2.0 ** -22, equal_nan=True, err_msg=f'{form} {cls.__name__}')


def _chunk_job(n, nlead=2, keep_init=False):
  import torch  # pylint: disable=g-import-not-at-top
  rng = np.random.default_rng(23)
  shape = (n, nlead) + SHAPE[1:]
  p_all = (np.round(rng.gamma(2.0, size=(n, nlead, M) + SHAPE[1:]) * 4) / 4).astype(np.float32)
  t_all = (np.round(rng.gamma(2.0, size=shape) * 4) / 4).astype(np.float32)
  lead = (np.arange(nlead) * 12).astype('timedelta64[h]').astype('timedelta64[ns]')
  inits = np.datetime64('2020-01-01T00', 'ns') + np.arange(n) * np.timedelta64(24, 'h')
  index = {int(t.astype('int64')): i for i, t in enumerate(inits)}
  pd, td = ('init_time', 'lead_time', 'number', 'latitude', 'longitude'), ('init_time', 'lead_time', 'latitude', 'longitude')
  dev = [(torch.as_tensor(p_all[i:i + 1]).cuda(), torch.as_tensor(t_all[i:i + 1]).cuda()) for i in range(n)]

  def load(init_chunk, lead_chunk):
    del lead_chunk
    i = index[int(init_chunk[0].astype('int64'))]
    cs = {'init_time': init_chunk, 'lead_time': lead, 'latitude': LAT, 'longitude': LON}
    return {'v': xr.DataArray(dev[i][0], dims=pd, coords=cs)}, {'v': xr.DataArray(dev[i][1], dims=td, coords=cs)}

  reduce_dims = ['latitude', 'longitude'] if keep_init else ['init_time', 'latitude', 'longitude']
  agg = aggregation.Aggregator(reduce_dims=reduce_dims, weigh_by=[weighting.GridAreaWeighting()])
  whole = ({'v': xr.DataArray(p_all, dims=pd, coords={'init_time': inits, 'lead_time': lead, 'latitude': LAT, 'longitude': LON})},
           {'v': xr.DataArray(t_all, dims=td, coords={'init_time': inits, 'lead_time': lead, 'latitude': LAT, 'longitude': LON})})
  return time_chunks.TimeChunks(inits, lead, init_time_chunk_size=1), load, agg, whole


def test_chunk_loop_records_and_replays_with_identical_bytes(monkeypatch):
  """pipeline.evaluate_chunks over 8 one-init chunks of device-resident fields: the launch is part of the chunk record (chunks
  alternate between two launch streams: of each kind one builds, one is recorded, the rest are replayed), nothing is refused, and
  the same loop without records gives the same accumulators bit for bit."""
  times, load, agg, whole = _chunk_job(8)
  metrics = dict(_metrics(FORMS['mean'][0]), weibull=wrappers.WrappedMetric(deterministic.MSE(), FORMS['weibull'][0](), unique_name_suffix='w'))
  names = _unique_names({k: v for k, v in metrics.items() if k != 'weibull'})
  monkeypatch.setattr(lazy, 'FUSED_BRIER', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['recorded'] >= 1 and stats['replayed'] >= 1 and stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  assert set(state.sum_weighted_statistics) == set(off.sum_weighted_statistics) and len(state.sum_weighted_statistics) == 4
  for name in state.sum_weighted_statistics:
    np.testing.assert_array_equal(np.asarray(state.sum_weighted_statistics[name]['v'].values), np.asarray(off.sum_weighted_statistics[name]['v'].values))
    np.testing.assert_array_equal(np.asarray(state.sum_weights[name]['v'].values), np.asarray(off.sum_weights[name]['v'].values))
  # ... and they are the restatement's numbers: per lead time and threshold, 8 x 13 x 24 area-weighted points
  p_all, t_all = np.asarray(whole[0]['v'].values), np.asarray(whole[1]['v'].values)
  pts = BC.points(np.moveaxis(p_all, 2, 0), t_all, THR, M).reshape(t_all.shape + (3, len(THR)))  # [init, lead, lat, lon, stat, k]
  w = O.grid_area_weights(LAT)
  for lane, sname in enumerate(STAT_NAMES):
    want = (pts[..., lane, :] * w[None, None, :, None, None]).sum(axis=(0, 2, 3))
    got = state.sum_weighted_statistics[names[sname]]['v']
    np.testing.assert_allclose(np.asarray(got.transpose('lead_time', 'threshold').values), want, rtol=0,
                               atol=16 * EPS * 8 * SHAPE[1] * SHAPE[2] * float(w.max()))


def test_accumulation_over_two_chunks_equals_the_one_shot_result(monkeypatch):
  """init_time survives, so every output belongs to one chunk: the accumulators of the deferred chunk loop hold exactly what one
  aggregation of the whole arrays gives."""
  times, load, agg, whole = _chunk_job(2, keep_init=True)
  metrics = _metrics(FORMS['mean'][0])
  monkeypatch.setattr(lazy, 'FUSED_BRIER', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', None)
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  engine.clear_caches()
  stats, one, _ = _evaluate(metrics, whole[0], whole[1], agg)
  for name in _unique_names(metrics).values():
    assert _is_fused(stats[name]['v'])
    for tree, tree1 in ((state.sum_weighted_statistics, one.sum_weighted_statistics), (state.sum_weights, one.sum_weights)):
      x, y = tree[name]['v'], tree1[name]['v']
      assert set(x.dims) == set(y.dims) == {'init_time', 'lead_time', 'threshold'}
      np.testing.assert_array_equal(np.asarray(x.transpose(*y.dims).values), np.asarray(y.values))
