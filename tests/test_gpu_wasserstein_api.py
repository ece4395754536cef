"""WassersteinDistance through the public API on the device: statistics + the Aggregator on small fields (5 against 3 members,
2 x 3 x 6 x 9) under a plain reduction, GridAreaWeighting with Regions bins, a target mask, and skipna with NaNs; with the fused
route on and off; NumPy and torch-resident payloads; every fallback condition; the largest ensembles; a recorded and replayed chunk
loop.

Bounds (tests/wasserstein_cases.py derives the per-point one, b, which covers the fused route and the restatement together; the
host route's pooled form sums M + N - 1 non-negative gap x width products of float64 quantities and is within the same relative
bound of the exact value).  A weighted sum over n points with non-negative weights W <= Wmax inherits Wmax * sum b plus
(n + 4) 2^-52 Wmax sum |value| for the float64 summations (stage 1, stage 2, the host's own); a plain mean is that over n."""
import functools

import numpy as np
import pytest

import wasserstein_cases as WC
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
DIMS = ('time', 'level', 'latitude', 'longitude')
SHAPE = (2, 3, 6, 9)
M, N = 5, 3
LAT = np.linspace(-75, 75, SHAPE[2])
LON = np.arange(SHAPE[3]) * (360.0 / SHAPE[3])
LEVEL = np.array([500.0, 700.0, 850.0])
REGIONS = {'global': ((-90, 90), (0, 360)), 'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180))}
REDUCE = ['time', 'latitude', 'longitude']


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.ens_wasserstein_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


@functools.lru_cache(maxsize=None)
def _arrays(dtype, nans, seed, m, n, shape):
  p, t = WC.values(seed, m, n, shape, dtype)
  rng = np.random.default_rng(seed + 1)
  if nans:
    p[rng.random(p.shape) < 0.01] = np.nan
    t[rng.random(t.shape) < 0.02] = np.nan
  valid = rng.random(shape[2:]) > 0.3
  t = np.ascontiguousarray(np.moveaxis(t, 0, -1))  # the targets' member axis innermost
  for a in (p, t, valid):
    a.setflags(write=False)
  return p, t, valid


def _inputs(dtype=np.float32, nans=False, mask=False, seed=11, m=M, n=N, shape=SHAPE, device=False):
  """p[number, time, level, latitude, longitude], t[time, level, latitude, longitude, number]: two sizes and two places of the
  member dim."""
  p, t, valid = _arrays(np.dtype(dtype).type, nans, seed, m, n, shape)
  cs = {'time': np.arange(shape[0]), 'level': np.arange(shape[1]) * 100.0 + 500.0, 'latitude': np.linspace(-75, 75, shape[2]),
        'longitude': np.arange(shape[3]) * (360.0 / shape[3])}
  tc = dict(cs)
  if mask:
    tc['mask'] = (('latitude', 'longitude'), valid.copy())
  if device:
    import torch  # pylint: disable=g-import-not-at-top
    load = lambda a: torch.as_tensor(np.array(a)).cuda()
  else:
    load = np.array
  return ({'v': xr.DataArray(load(p), dims=('number',) + DIMS, coords=dict(cs, number=np.arange(m)), name='v')},
          {'v': xr.DataArray(load(t), dims=DIMS + ('number',), coords=dict(tc, number=np.arange(n)), name='v')})


class _Metric(metrics_base.PerVariableMetric):
  """WassersteinDistance as a metric (the package has the statistic only)."""

  @property
  def statistics(self):
    return {'WassersteinDistance': probabilistic.WassersteinDistance('number')}

  def _values_from_mean_statistics_per_variable(self, statistic_values):
    return statistic_values['WassersteinDistance']


NAME = probabilistic.WassersteinDistance('number').unique_name


def _evaluate(pred, targ, aggregator):
  metrics = {'w': _Metric()}
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def compute_all_metrics(metrics, predictions, targets, reduce_dims, **kw):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, predictions, targets)
  return aggregation.Aggregator(reduce_dims=reduce_dims, **kw).aggregate_statistics(stats).metric_values(metrics)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyStatistic) and stat._group.kind == 'wass'  # pylint: disable=protected-access


def _launches():
  return [e for e in engine.S1_EVENT_LOG if e['kind'] == 'wass']


def _max_area_weight():
  probe = xr.DataArray(np.zeros(SHAPE[2:]), dims=DIMS[2:], coords={'latitude': LAT, 'longitude': LON})
  return float(np.asarray(weighting.GridAreaWeighting().weights(probe).values).max())


def _points(pred, targ):
  """The restatement per point over the frame [time, level, latitude, longitude], and its bound."""
  return WC.wasserstein_points(np.asarray(pred['v'].values), np.moveaxis(np.asarray(targ['v'].values), -1, 0))


def _same_labels(a, b):
  assert tuple(a.dims) == tuple(b.dims) and set(a.coords) == set(b.coords) and a.name == b.name, (a.dims, b.dims, set(a.coords), set(b.coords))
  for k in a.coords:
    np.testing.assert_array_equal(np.asarray(a.coords[k].values), np.asarray(b.coords[k].values))


CASES = {
    'plain': dict(kw=lambda: {}, nans=False, mask=False, area=False),
    'regions': dict(kw=lambda: dict(weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)]), nans=False, mask=False, area=True),
    'masked': dict(kw=lambda: dict(masked=True, weigh_by=[weighting.GridAreaWeighting()]), nans=False, mask=True, area=True),
    'skipna': dict(kw=lambda: dict(skipna=True), nans=True, mask=False, area=False),
}


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('case_name', list(CASES))
def test_scores_with_the_route_on_and_off_against_the_restatement(monkeypatch, case_name, dtype):
  case = CASES[case_name]
  pred, targ = _inputs(dtype, nans=case['nans'], mask=case['mask'])
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(pred, targ, aggregation.Aggregator(reduce_dims=REDUCE, **case['kw']()))
  assert list(stats) == [NAME] and _is_fused(stats[NAME]['v']) and stats[NAME]['v'].is_lazy
  # the fused route was taken: one launch of wbx_ens_wasserstein_partial and nothing else
  assert len(_launches()) == 1 and len(engine.S1_EVENT_LOG) == 1, engine.S1_EVENT_LOG
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  engine.clear_caches()
  stats0, state0, values0 = _evaluate(pred, targ, aggregation.Aggregator(reduce_dims=REDUCE, **case['kw']()))
  assert not _is_fused(stats0[NAME]['v']) and not _launches()
  # per point: labelled as the host route's result, NaN where the rule says, within the bound of the restatement
  a, b = stats[NAME]['v'], stats0[NAME]['v']
  _same_labels(a, b)
  stat, bound = _points(pred, targ)
  got = np.asarray(a.transpose(*DIMS).values)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(stat))
  assert case['nans'] == bool(np.isnan(stat).any())
  fin = np.isfinite(stat)
  assert (np.abs(got[fin] - stat[fin]) <= bound[fin]).all()
  host = np.asarray(b.transpose(*DIMS).values)
  np.testing.assert_array_equal(np.isnan(host), np.isnan(stat))
  assert (np.abs(host[fin] - stat[fin]) <= bound[fin]).all()
  # the sums: both routes against each other, labelled alike
  n = int(np.prod([a.sizes[d] for d in REDUCE]))
  wmax = _max_area_weight() if case['area'] else 1.0
  mag = float(np.nansum(np.abs(stat)))
  tol = wmax * (2 * float(bound.sum()) + (n + 4) * 2.0 ** -52 * mag)
  x, y = state.sum_weighted_statistics[NAME]['v'], state0.sum_weighted_statistics[NAME]['v']
  _same_labels(x, y)
  print(case_name, 'max |fused - host| of the sums:', float(np.nanmax(np.abs(np.asarray(x.values) - np.asarray(y.values)))), 'bound', tol)
  np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=0, atol=tol)
  assert np.isfinite(np.asarray(x.values)).all()
  np.testing.assert_allclose(np.asarray(state.sum_weights[NAME]['v'].values), np.asarray(state0.sum_weights[NAME]['v'].values), rtol=1e-12, atol=0)
  _same_labels(values['w.v'], values0['w.v'])
  # ... and the restatement's, where the aggregation is a plain or NaN-skipping mean over (time, latitude, longitude)
  if case_name in ('plain', 'skipna'):
    count = np.isfinite(stat).sum(axis=(0, 2, 3))
    want = np.nansum(stat, axis=(0, 2, 3)) / count
    tol = (bound.sum(axis=(0, 2, 3)) + (n + 4) * 2.0 ** -52 * np.nansum(np.abs(stat), axis=(0, 2, 3))) / count
    for which, res in (('fused', values), ('host', values0)):
      err = np.abs(np.asarray(res['w.v'].transpose('level').values) - want)
      print(case_name, which, 'max |route - restatement| / bound:', float((err / tol).max()))
      assert (err <= tol).all(), which


def test_compute_all_metrics_takes_the_fused_route(monkeypatch):
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  pred, targ = _inputs(mask=True)
  out = compute_all_metrics({'w': _Metric()}, pred, targ, reduce_dims=['longitude'])
  assert len(_launches()) == 1
  stat, bound = _points(pred, targ)
  want = stat.mean(axis=3)
  got = np.asarray(out['w.v'].transpose('time', 'level', 'latitude').values)
  assert (np.abs(got - want) <= bound.sum(axis=3) / SHAPE[3] + (SHAPE[3] + 4) * 2.0 ** -52 * want).all()
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', False)
  engine.clear_caches()
  out0 = compute_all_metrics({'w': _Metric()}, pred, targ, reduce_dims=['longitude'])
  _same_labels(out['w.v'], out0['w.v'])


def test_torch_resident_payloads_give_the_bits_of_numpy_payloads(monkeypatch):
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', True)
  # every output the sum of two points (the two times): the same bits whatever plan the storage order of the payload leads to
  make = lambda: aggregation.Aggregator(reduce_dims=['time'], weigh_by=[weighting.GridAreaWeighting()])
  pred, targ = _inputs()
  stats, state, _ = _evaluate(pred, targ, make())
  dpred, dtarg = _inputs(device=True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  dstats, state_t, _ = _evaluate(dpred, dtarg, make())
  assert _is_fused(dstats[NAME]['v']) and len(_launches()) == 1
  order = state.sum_weighted_statistics[NAME]['v'].dims
  np.testing.assert_array_equal(np.asarray(state_t.sum_weighted_statistics[NAME]['v'].transpose(*order).values),
                                np.asarray(state.sum_weighted_statistics[NAME]['v'].values))
  np.testing.assert_array_equal(np.asarray(state_t.sum_weights[NAME]['v'].transpose(*order).values), np.asarray(state.sum_weights[NAME]['v'].values))
  # and per point, where every dim is kept: a float64 tensor on the payload's device, as the host route gives
  import torch  # pylint: disable=g-import-not-at-top
  data = dstats[NAME]['v'].data
  assert torch.is_tensor(data) and data.is_cuda and data.dtype == torch.float64 and isinstance(stats[NAME]['v'].data, np.ndarray)
  np.testing.assert_array_equal(np.asarray(dstats[NAME]['v'].transpose(*DIMS).values), np.asarray(stats[NAME]['v'].transpose(*DIMS).values))
  np.testing.assert_array_equal(np.asarray(stats[NAME]['v'].transpose(*DIMS).values), WC.exact_points(
      np.asarray(pred['v'].values), np.moveaxis(np.asarray(targ['v'].values), -1, 0)))


FALLBACKS = {
    'switch off': dict(switch=False),
    'M = 65': dict(m=65),
    'N = 65': dict(n=65),
    'integer inputs': dict(dtype=np.int64),
    'two dtypes': dict(target_dtype=np.float64),
    'a dim the targets lack': dict(drop_level=True),
    'a mask along the member dim': dict(mask_dims=('latitude', 'number')),
    'nothing left of the frame': dict(point=True),
    'labels that differ': dict(shift_latitude=True),
}


@pytest.mark.parametrize('why', list(FALLBACKS))
def test_every_fallback_condition_gives_the_host_routes_result(monkeypatch, why):
  spec = FALLBACKS[why]
  pred, targ = _inputs(np.float32, m=spec.get('m', M), n=spec.get('n', N))
  if 'dtype' in spec:
    pred, targ = {'v': pred['v'].astype(spec['dtype'])}, {'v': targ['v'].astype(spec['dtype'])}
  if 'target_dtype' in spec:
    targ = {'v': targ['v'].astype(spec['target_dtype'])}
  if spec.get('drop_level'):
    targ = {'v': targ['v'].isel(level=0, drop=True)}
  if 'mask_dims' in spec:
    md = spec['mask_dims']
    targ = {'v': targ['v'].assign_coords(mask=(md, np.random.default_rng(1).random((SHAPE[2], N)) > 0.3))}
  if spec.get('point'):
    sel = dict(time=0, level=0, latitude=0, longitude=0)
    pred, targ = {'v': pred['v'].isel(**sel, drop=True)}, {'v': targ['v'].isel(**sel, drop=True)}
  if spec.get('shift_latitude'):
    targ = {'v': targ['v'].assign_coords(latitude=LAT + 1.0)}
  stat = probabilistic.WassersteinDistance('number')
  reduce_dims = [] if spec.get('point') else ['time', 'latitude', 'longitude']

  def run():
    per_var = stat.compute(pred, targ)
    state = aggregation.Aggregator(reduce_dims=reduce_dims).aggregate_statistics({stat.unique_name: per_var})
    return per_var['v'], state.sum_weighted_statistics[stat.unique_name]['v']
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', spec.get('switch', True))
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  points, sums = run()
  assert not _is_fused(points) and not _launches(), why
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', False)
  engine.clear_caches()
  points0, sums0 = run()
  _same_labels(points, points0)
  _same_labels(sums, sums0)
  np.testing.assert_array_equal(np.asarray(points.values), np.asarray(points0.values), err_msg=why)
  np.testing.assert_array_equal(np.asarray(sums.values), np.asarray(sums0.values), err_msg=why)


def test_64_members_a_side_are_fused_and_65_are_not(monkeypatch):
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stat = probabilistic.WassersteinDistance('number')
  for m, n, fused in ((64, 64, True), (1, 1, True), (65, 64, False), (64, 65, False)):
    pred, targ = _inputs(np.float32, m=m, n=n, shape=(2, 1, 2, 3))
    per_var = stat.compute(pred, targ)
    assert _is_fused(per_var['v']) == fused, (m, n)
    state = aggregation.Aggregator(reduce_dims=['time']).aggregate_statistics({stat.unique_name: per_var})
    want, bound = _points(pred, targ)
    got = np.asarray(state.sum_weighted_statistics[stat.unique_name]['v'].transpose('level', 'latitude', 'longitude').values)
    assert (np.abs(got - want.sum(axis=0)) <= bound.sum(axis=0) + 6 * 2.0 ** -52 * want.sum(axis=0)).all(), (m, n)
  assert len(_launches()) == 2


def _chunk_job(n_chunks, nlead=2):
  import torch  # pylint: disable=g-import-not-at-top
  rng = np.random.default_rng(23)
  p_all = (rng.integers(-64, 65, size=(n_chunks, nlead, M) + SHAPE[1:]) / 8.0).astype(np.float32)
  t_all = (rng.integers(-64, 65, size=(n_chunks, nlead, N) + SHAPE[1:]) / 8.0).astype(np.float32)
  lead = (np.arange(nlead) * 12).astype('timedelta64[h]').astype('timedelta64[ns]')
  inits = np.datetime64('2020-01-01T00', 'ns') + np.arange(n_chunks) * np.timedelta64(24, 'h')
  index = {int(t.astype('int64')): i for i, t in enumerate(inits)}
  dims = ('init_time', 'lead_time', 'number') + DIMS[1:]
  dev = [(torch.as_tensor(p_all[i:i + 1]).cuda(), torch.as_tensor(t_all[i:i + 1]).cuda()) for i in range(n_chunks)]

  def load(init_chunk, lead_chunk):
    del lead_chunk
    i = index[int(init_chunk[0].astype('int64'))]
    cs = {'init_time': init_chunk, 'lead_time': lead, 'level': LEVEL, 'latitude': LAT, 'longitude': LON}
    return {'v': xr.DataArray(dev[i][0], dims=dims, coords=cs)}, {'v': xr.DataArray(dev[i][1], dims=dims, coords=cs)}

  agg = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])
  return time_chunks.TimeChunks(inits, lead, init_time_chunk_size=1), load, agg, (p_all, t_all)


def test_chunk_loop_with_records_equals_the_unrecorded_loop(monkeypatch):
  """pipeline.evaluate_chunks over three one-init chunks of device-resident fields, with chunk records and without: the same
  accumulators bit for bit (the replay case of wbx_chunk_replay), and the restatement's numbers within the bound."""
  times, load, agg, (p_all, t_all) = _chunk_job(3)
  metrics = {'w': _Metric()}
  monkeypatch.setattr(lazy, 'FUSED_WASSERSTEIN', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  np.testing.assert_array_equal(np.asarray(state.sum_weighted_statistics[NAME]['v'].values), np.asarray(off.sum_weighted_statistics[NAME]['v'].values))
  np.testing.assert_array_equal(np.asarray(state.sum_weights[NAME]['v'].values), np.asarray(off.sum_weights[NAME]['v'].values))
  stat, bound = WC.wasserstein_points(np.moveaxis(p_all, 2, 0), np.moveaxis(t_all, 2, 0))  # [init, lead, level, lat, lon]
  probe = xr.DataArray(np.zeros(SHAPE[2:]), dims=DIMS[2:], coords={'latitude': LAT, 'longitude': LON})
  w = np.asarray(weighting.GridAreaWeighting().weights(probe).values, np.float64).reshape(-1, 1) * np.ones((1, SHAPE[3]))
  want = (stat * w[None, None, None]).sum(axis=(0, 3, 4))
  n = 3 * SHAPE[2] * SHAPE[3]
  tol = float(w.max()) * (bound.sum(axis=(0, 3, 4)) + (n + 4) * 2.0 ** -52 * stat.sum(axis=(0, 3, 4)))
  got = np.asarray(state.sum_weighted_statistics[NAME]['v'].transpose('lead_time', 'level').values)
  assert (np.abs(got - want) <= tol).all(), (got, want, tol)
