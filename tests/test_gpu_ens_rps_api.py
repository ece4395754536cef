"""EnsembleRankedProbabilityScore through the public API on the device: compute_unique_statistics_for_all_metrics + the Aggregator on
small fields (7 members, 4 x 13 x 24) under a plain reduction, GridAreaWeighting with Regions x land / sea bins, a target mask, and
skipna with NaNs; torch-resident payloads; a recorded and replayed chunk loop; accumulation over chunks.

Bounds.  The fused route and the host route (lazy.FUSED_ENS_RPS = False: the parent commit's arithmetic) differ per point by at
most 16 * K * eps (about ten float64 operations on magnitudes <= 1 per threshold on the host route, one correctly rounded quotient
on the fused one), so an output that sums N points -- N = the product of the sizes of the dims the aggregator reduces -- by at
most 16 * K * eps * N, times the largest weight where the aggregator weighs; sums of weights are the same numbers in another order
(rtol 1e-12); a metric value is a weighted mean, with non-negative weights, of per-point values: 16 * K * eps whatever N is."""
import numpy as np
import pytest

import ens_rps_cases as EC
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
from weatherbenchx_amd.metrics import probabilistic

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
DIMS = ('time', 'latitude', 'longitude')
SHAPE = (4, 13, 24)
M = 7
THR = [0.1, 0.5, 1.0, 2.5, 4.0]
LAT = np.linspace(-90, 90, SHAPE[1])
LON = np.arange(SHAPE[2]) * (360.0 / SHAPE[2])
REGIONS = {'global': ((-90, 90), (0, 360)), 'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180))}


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.ens_rps_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


class _StatisticAsMetric(metrics_base.PerVariableMetric):

  def __init__(self, statistic):
    self._statistic = statistic

  @property
  def statistics(self):
    return {'s': self._statistic}

  def _values_from_mean_statistics_per_variable(self, statistic_values):
    return statistic_values['s']


def _rps(thresholds=None, suffix='s', **kw):
  thresholds = THR if thresholds is None else thresholds
  return probabilistic.EnsembleRankedProbabilityScore(thresholds, thresholds, 'bin', suffix, **kw)


def _inputs(dtype=np.float32, nans=False, mask=False, seed=11, variables=('u', 'v')):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(SHAPE[0]), 'latitude': LAT, 'longitude': LON}
  pred, targ = {}, {}
  for v in variables:
    p = (np.round(rng.gamma(2.0, size=(M,) + SHAPE) * 4) / 4).astype(dtype)  # ties with the thresholds
    t = (np.round(rng.gamma(2.0, size=SHAPE) * 4) / 4).astype(dtype)
    p[:4, 0, 0, 0] = [0.5, np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(0)), np.nextafter(np.float32(0.1), np.float32(1))]
    if nans:
      p[rng.random(p.shape) < 0.01] = np.nan
      t[rng.random(SHAPE) < 0.05] = np.nan
    tc = dict(cs)
    if mask:
      tc['mask'] = (DIMS[1:], rng.random(SHAPE[1:]) > 0.3)
    pred[v] = xr.DataArray(p, dims=('number',) + DIMS, coords=dict(cs, number=np.arange(M)), name=v)
    targ[v] = xr.DataArray(t, dims=DIMS, coords=tc, name=v)
  return pred, targ


def _lsm():
  land = (np.sin(np.deg2rad(LON) * 3)[None, :] * np.cos(np.deg2rad(LAT) * 2.5)[:, None]) > 0.1
  return xr.DataArray(land, dims=DIMS[1:], coords={'latitude': LAT, 'longitude': LON})


def _max_area_weight():
  probe = xr.DataArray(np.zeros(SHAPE[1:]), dims=DIMS[1:], coords={'latitude': LAT, 'longitude': LON})
  return float(np.asarray(weighting.GridAreaWeighting().weights(probe).values).max())


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyStatistic) and stat._group.kind == 'erps'  # pylint: disable=protected-access


CASES = {
    'plain': dict(reduce=DIMS, kw=lambda: {}, nans=False, mask=False, area=False),
    'keep-longitude': dict(reduce=('time', 'latitude'), kw=lambda: {}, nans=False, mask=False, area=False),
    'regions-x-landsea': dict(reduce=DIMS, kw=lambda: dict(weigh_by=[weighting.GridAreaWeighting()],
                                                           bin_by=[binning.Regions(REGIONS), binning.LandSea(_lsm().astype(np.float64))]),
                              nans=False, mask=False, area=True),
    'masked': dict(reduce=DIMS, kw=lambda: dict(masked=True, weigh_by=[weighting.GridAreaWeighting()]), nans=False, mask=True, area=True),
    'skipna': dict(reduce=('time', 'longitude'), kw=lambda: dict(skipna=True), nans=True, mask=False, area=False),
}


def _aggregator(case):
  return aggregation.Aggregator(reduce_dims=list(case['reduce']), **case['kw']())


def _points_per_output(case):
  """The product of the sizes of the reduced dims: no output sums more points (bins and masks leave fewer)."""
  return int(np.prod([SHAPE[DIMS.index(d)] for d in case['reduce']]))


@pytest.mark.parametrize('fair', [True, False], ids=['fair', 'unfair'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('which', list(CASES))
def test_scores_against_the_host_route_and_the_restatement(monkeypatch, which, dtype, fair):
  case = CASES[which]
  pred, targ = _inputs(dtype, nans=case['nans'], mask=case['mask'])
  metrics = {'rps': _StatisticAsMetric(_rps(fair=fair))}
  name = _rps(fair=fair).unique_name
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(metrics, pred, targ, _aggregator(case))
  assert all(_is_fused(s) and s.is_lazy for per_var in stats.values() for s in per_var.values())
  launches = [e for e in engine.S1_EVENT_LOG if e['kind'] == 'erps']
  assert len(launches) == 2 and len(engine.S1_EVENT_LOG) == 2, engine.S1_EVENT_LOG  # one launch per variable, nothing else
  if which == 'plain':  # the sum of everything is the restatement's integer sum over D (stage 2 adds a few partials)
    for var in ('u', 'v'):
      s = int(EC.numerators(pred[var].values, targ[var].values, THR, THR, fair, True).sum())
      got = float(np.asarray(state.sum_weighted_statistics[name][var].values))
      np.testing.assert_allclose(got, s / EC.denominator(M, fair), rtol=8 * EPS, atol=0)
  # the same evaluation on the host route
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats0, state0, values0 = _evaluate(metrics, pred, targ, _aggregator(case))
  assert not any(_is_fused(s) for per_var in stats0.values() for s in per_var.values())
  assert not [e for e in engine.S1_EVENT_LOG if e['kind'] == 'erps']
  bound = 16 * len(THR) * EPS * _points_per_output(case) * (_max_area_weight() if case['area'] else 1.0)
  for var in ('u', 'v'):
    x, y = state.sum_weighted_statistics[name][var], state0.sum_weighted_statistics[name][var]
    assert tuple(x.dims) == tuple(y.dims) and set(x.coords) == set(y.coords), (var, x.dims, y.dims)
    print(which, var, 'max |fused - host| of the sums:', float(np.nanmax(np.abs(np.asarray(x.values) - np.asarray(y.values)))), 'bound', bound)
    np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=0, atol=bound, equal_nan=True, err_msg=f'{which} {var} sums')
    assert np.isfinite(np.asarray(x.values)).all()
    x, y = state.sum_weights[name][var], state0.sum_weights[name][var]
    assert tuple(x.dims) == tuple(y.dims)
    np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=1e-12, atol=0, err_msg=f'{which} {var} weights')
  assert set(values) == set(values0)
  for key in values:
    assert tuple(values[key].dims) == tuple(values0[key].dims) and set(values[key].coords) == set(values0[key].coords)
    # a weighted mean, with non-negative weights, of per-point values that differ by at most 16 K eps each
    print(which, key, 'max |fused - host| of the means:', float(np.nanmax(np.abs(np.asarray(values[key].values) - np.asarray(values0[key].values)))),
          'bound', 16 * len(THR) * EPS)
    np.testing.assert_allclose(np.asarray(values[key].values), np.asarray(values0[key].values), rtol=0, atol=16 * len(THR) * EPS,
                               equal_nan=True, err_msg=key)


def test_a_list_with_a_duplicate_counts_it_twice_like_the_host_route(monkeypatch):
  """[1.0, 0.5, 1.0] on both sides with enforce_monotonicity=False: both routes sum three terms."""
  thr = [1.0, 0.5, 1.0]
  case = CASES['regions-x-landsea']
  pred, targ = _inputs(variables=('v',))
  stat = lambda: _rps(thr, enforce_monotonicity=False)
  metrics = {'rps': _StatisticAsMetric(stat())}
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(metrics, pred, targ, _aggregator(case))
  assert _is_fused(stats[stat().unique_name]['v']) and [e['kind'] for e in engine.S1_EVENT_LOG] == ['erps']
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', False)
  stats0, state0, values0 = _evaluate(metrics, pred, targ, _aggregator(case))
  assert not _is_fused(stats0[stat().unique_name]['v'])
  x, y = state.sum_weighted_statistics[stat().unique_name]['v'], state0.sum_weighted_statistics[stat().unique_name]['v']
  assert tuple(x.dims) == tuple(y.dims)
  np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=0, atol=16 * 3 * EPS * _points_per_output(case) * _max_area_weight())
  np.testing.assert_allclose(np.asarray(values['rps.v'].values), np.asarray(values0['rps.v'].values), rtol=0, atol=16 * 3 * EPS, equal_nan=True)


def test_a_nan_under_a_valid_point_poisons_and_under_the_mask_does_not(monkeypatch):
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', True)
  metrics = {'rps': _StatisticAsMetric(_rps())}
  name = _rps().unique_name
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
  bad = np.isnan(np.asarray(state.sum_weighted_statistics[name]['v'].values))
  assert bad[shown[0]] and not np.delete(bad, shown[0]).any()  # that latitude, nothing else


def test_torch_resident_payloads_give_the_same_bits(monkeypatch):
  import torch  # pylint: disable=g-import-not-at-top
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', True)
  metrics = {'rps': _StatisticAsMetric(_rps())}
  name = _rps().unique_name
  make = lambda: aggregation.Aggregator(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)])
  pred, targ = _inputs(variables=('v',))
  _, state, _ = _evaluate(metrics, pred, targ, make())
  on_dev = lambda da: xr.DataArray(torch.as_tensor(np.asarray(da.values)).cuda(), dims=da.dims, coords={d: da.coords[d].values for d in da.dims}, name=da.name)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state_t, _ = _evaluate(metrics, {'v': on_dev(pred['v'])}, {'v': on_dev(targ['v'])}, make())
  assert _is_fused(stats[name]['v']) and [e['kind'] for e in engine.S1_EVENT_LOG] == ['erps']
  np.testing.assert_array_equal(np.asarray(state_t.sum_weighted_statistics[name]['v'].values), np.asarray(state.sum_weighted_statistics[name]['v'].values))
  np.testing.assert_array_equal(np.asarray(state_t.sum_weights[name]['v'].values), np.asarray(state.sum_weights[name]['v'].values))


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
  metrics = {'rps': _StatisticAsMetric(_rps()), 'unfair': _StatisticAsMetric(_rps(fair=False, suffix='u'))}
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['recorded'] >= 1 and stats['replayed'] >= 1 and stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  for fair, suffix in ((True, 's'), (False, 'u')):
    name = _rps(fair=fair, suffix=suffix).unique_name
    got = state.sum_weighted_statistics[name]['v']
    np.testing.assert_array_equal(np.asarray(got.values), np.asarray(off.sum_weighted_statistics[name]['v'].values))
    np.testing.assert_array_equal(np.asarray(state.sum_weights[name]['v'].values), np.asarray(off.sum_weights[name]['v'].values))
    # ... and they are the restatement's numbers: per lead time, 8 x 13 x 24 area-weighted points
    p_all, t_all = np.asarray(whole[0]['v'].values), np.asarray(whole[1]['v'].values)
    rps = EC.rps_points(np.moveaxis(p_all, 2, 0), t_all, THR, THR, fair, True)  # [init, lead, lat, lon]
    probe = xr.DataArray(np.zeros(SHAPE[1:]), dims=DIMS[1:], coords={'latitude': LAT, 'longitude': LON})
    w = weighting.GridAreaWeighting().weights(probe)
    w = np.asarray(w.values, np.float64).reshape(-1, 1) * np.ones((1, SHAPE[2]))
    want = (rps * w[None, None]).sum(axis=(0, 2, 3))
    np.testing.assert_allclose(np.asarray(got.transpose('lead_time').values), want, rtol=0,
                               atol=16 * len(THR) * EPS * 8 * SHAPE[1] * SHAPE[2] * float(w.max()))


def test_accumulation_over_two_chunks_equals_the_one_shot_result(monkeypatch):
  """init_time survives, so every output belongs to one chunk: the accumulators of the deferred chunk loop hold exactly what one
  aggregation of the whole arrays gives."""
  times, load, agg, whole = _chunk_job(2, keep_init=True)
  metrics = {'rps': _StatisticAsMetric(_rps())}
  name = _rps().unique_name
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', None)
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  engine.clear_caches()
  stats, one, _ = _evaluate(metrics, whole[0], whole[1], agg)
  assert _is_fused(stats[name]['v'])
  for tree, tree1 in ((state.sum_weighted_statistics, one.sum_weighted_statistics), (state.sum_weights, one.sum_weights)):
    x, y = tree[name]['v'], tree1[name]['v']
    assert set(x.dims) == set(y.dims) == {'init_time', 'lead_time'}
    np.testing.assert_array_equal(np.asarray(x.transpose(*y.dims).values), np.asarray(y.values))
