"""Bias, MAE, MSE and RMSE of ensemble quantiles through the public API on the device: compute_unique_statistics_for_all_metrics + the
Aggregator behind EnsembleQuantiles('predictions', quantiles), on small fields (7 members, 4 x 13 x 24) under a plain reduction,
GridAreaWeighting with Regions bins, a target mask and skipna with NaNs; NumPy and torch-resident payloads; more quantiles than a
launch holds; a recorded and replayed chunk loop.

Every check compares the fused route (WBX_FUSED_ENS_QUANTILES on: lazy.FUSED_ENS_QUANTILES) with the host route (off) by dim name:
dims, coordinates and NaN placement are identical, the sums of weights are the same numbers (rtol 1e-12: another order), and the
weighted sums agree within a bound that tests/quantile_error_cases.py and this module derive from the case's own values:
  NumPy payloads.  Both routes hold the same float64 value per point (NumPy's float64 quantiles of float32 members, the float64
    difference, |.| and square); they differ in the order of adding n weighted terms: n 2^-53 sum(w |v|) per output, sum(w |v|)
    from the restatement pushed through the oracle's float64 weighted sum.
  torch payloads.  torch.quantile works in the input dtype, float32 here: QC.host_float32_bounds bounds the difference per point from
    that route's rounding count and the point's magnitudes; the oracle's weighted sum of those bounds, plus the term above, bounds
    an output.
Metric values are functions of the two sums: Bias / MAE / MSE differ by at most bound / weights, RMSE by that over the sum of the two
roots (sqrt a - sqrt b = (a - b) / (sqrt a + sqrt b)); a few units in the last place are granted to the quotient and the root."""
import numpy as np
import pytest

import quantile_error_cases as QC
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
DIMS = ('time', 'latitude', 'longitude')
SHAPE = (4, 13, 24)
M = 7
QS = [0.1, 0.5, 0.9]
LAT = np.linspace(-90, 90, SHAPE[1])
LON = np.arange(SHAPE[2]) * (360.0 / SHAPE[2])
REGIONS = {'global': ((-90, 90), (0, 360)), 'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180))}
STAT_NAMES = ('Error', 'AbsoluteError', 'SquaredError')
ULPS = 8 * 2.0 ** -52  # relative: the quotient, the root and their operands' last places


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.ens_quantile_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


def _chain(qs=None):
  return [wrappers.EnsembleQuantiles('predictions', QS if qs is None else qs)]


def _metrics(qs=None):
  return {'mse': wrappers.WrappedMetric(deterministic.MSE(), _chain(qs)), 'rmse': wrappers.WrappedMetric(deterministic.RMSE(), _chain(qs)),
          'mae': wrappers.WrappedMetric(deterministic.MAE(), _chain(qs)), 'bias': wrappers.WrappedMetric(deterministic.Bias(), _chain(qs))}


def _unique_names(metrics):
  """base statistic name -> the unique name of the wrapped statistic."""
  out = {}
  for metric in metrics.values():
    for stat in metric.statistics.values():
      out[stat.unique_name.split('_')[0]] = stat.unique_name
  assert set(out) == set(STAT_NAMES), out
  return out


def _inputs(nans=False, mask=False, seed=11, variables=('u', 'v')):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(SHAPE[0]), 'latitude': LAT, 'longitude': LON}
  pred, targ = {}, {}
  for v in variables:
    p = (rng.standard_normal((M,) + SHAPE) * 3.0 + 280.0).astype(np.float32)
    t = (rng.standard_normal(SHAPE) * 3.0 + 280.0).astype(np.float32)
    p[M - 1] = np.where(rng.random(SHAPE) < 0.3, p[0], p[M - 1])  # ties
    if nans:
      p[rng.random(p.shape) < 0.01] = np.nan
      t[rng.random(SHAPE) < 0.05] = np.nan
    tc = dict(cs)
    if mask:
      tc['mask'] = (DIMS[1:], rng.random(SHAPE[1:]) > 0.3)
    pred[v] = xr.DataArray(p, dims=('number',) + DIMS, coords=dict(cs, number=np.arange(M)), name=v)
    targ[v] = xr.DataArray(t, dims=DIMS, coords=tc, name=v)
  return pred, targ


def _on_device(tree):
  import torch  # pylint: disable=g-import-not-at-top
  out = {}
  for name, da in tree.items():
    coords = {d: da.coords[d].values for d in da.dims}
    if 'mask' in da.coords:
      coords['mask'] = (da.coords['mask'].dims, np.asarray(da.coords['mask'].values))
    out[name] = xr.DataArray(torch.as_tensor(np.asarray(da.values)).cuda(), dims=da.dims, coords=coords, name=da.name)
  return out


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyQuantileError)


CASES = {
    'plain': dict(reduce=DIMS, kw=lambda: {}, nans=False, mask=False, area=False),
    'keep-longitude': dict(reduce=('time', 'latitude'), kw=lambda: {}, nans=False, mask=False, area=False),
    'area-x-regions': dict(reduce=DIMS, kw=lambda: dict(weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)]),
                           nans=False, mask=False, area=True, regions=True),
    'masked': dict(reduce=DIMS, kw=lambda: dict(masked=True, weigh_by=[weighting.GridAreaWeighting()]), nans=False, mask=True, area=True),
    'skipna': dict(reduce=('time', 'longitude'), kw=lambda: dict(skipna=True), nans=True, mask=False, area=False),
}


def _aggregator(case):
  return aggregation.Aggregator(reduce_dims=list(case['reduce']), **case['kw']())


def _region_masks():
  _, masks = O.region_masks(LAT, LON, REGIONS)
  return [('region', masks, ('region', 'latitude', 'longitude'))]


def _bounds(case, pred, targ, qs, float32_host):
  """{(statistic, variable): (bound on |difference| of the weighted sums, its dims)} for `case`: see the module docstring."""
  n = int(np.prod([SHAPE[DIMS.index(d)] for d in case['reduce']]))
  w = [(O.grid_area_weights(LAT), ('latitude',))] if case['area'] else []
  bins = _region_masks() if case.get('regions') else []
  sdims = ('quantile',) + DIMS
  out = {}
  for var in pred:
    p, t = np.asarray(pred[var].values), np.asarray(targ[var].values)
    pts = np.moveaxis(QC.points(p, t, qs).reshape(SHAPE + (3, len(qs))), -1, 0)  # [quantile, time, lat, lon, stat]
    mask = np.asarray(targ[var].coords['mask'].values, bool) if case['mask'] else None
    per_point = np.moveaxis(QC.host_float32_bounds(p, t, qs).reshape(SHAPE + (3, len(qs))), -1, 0) if float32_host else None
    for lane, sname in enumerate(STAT_NAMES):
      kw = dict(weights=w, bin_masks=bins, mask=mask, mask_dims=DIMS[1:])
      mag, _, od = O.aggregate(np.abs(pts[..., lane]), sdims, case['reduce'], skipna=case['nans'], **kw)
      bound = n * 2.0 ** -53 * mag
      if float32_host:
        gone = np.isnan(pts[..., lane])  # (points skipna counts out carry no difference)
        delta = np.where(gone, 0.0, per_point[..., lane])
        bound = bound + O.aggregate(delta, sdims, case['reduce'], **kw)[0]
      out[sname, var] = (bound, od)
  return out


def _compare(case, metrics, on, off, bounds, tag):
  names = _unique_names(metrics)
  (state, values), (state0, values0) = on, off
  for sname in STAT_NAMES:
    for var in ('u', 'v'):
      x, y = state.sum_weighted_statistics[names[sname]][var], state0.sum_weighted_statistics[names[sname]][var]
      wx, wy = state.sum_weights[names[sname]][var], state0.sum_weights[names[sname]][var]
      for a, b in ((x, y), (wx, wy)):
        assert tuple(a.dims) == tuple(b.dims) and set(a.coords) == set(b.coords), (tag, sname, var, a.dims, b.dims)
        for k in b.coords:
          np.testing.assert_array_equal(np.asarray(a.coords[k].values), np.asarray(b.coords[k].values), err_msg=f'{tag} {sname} {var}: {k}')
      assert x.dims[0] == 'quantile' and np.asarray(x.coords['quantile'].values).dtype == np.float64
      bound, od = bounds[sname, var]
      assert set(od) == set(x.dims), (od, x.dims)
      got, want = np.asarray(x.transpose(*od).values), np.asarray(y.transpose(*od).values)
      np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{tag} {sname} {var}')
      with np.errstate(all='ignore'):
        excess = np.nanmax(np.abs(got - want) - bound)
        print(tag, sname, var, 'max |fused - host| of the sums:', float(np.nanmax(np.abs(got - want))), 'largest bound', float(np.nanmax(bound)))
      assert not excess > 0.0, (tag, sname, var, excess)
      np.testing.assert_allclose(np.asarray(wx.values), np.asarray(wy.values), rtol=1e-12, atol=0)
  assert set(values) == set(values0) == {f'{m}.{v}' for m in metrics for v in ('u', 'v')}
  stat_of = {'mse': 'SquaredError', 'rmse': 'SquaredError', 'mae': 'AbsoluteError', 'bias': 'Error'}
  for key in values:
    a, b = values[key], values0[key]
    assert tuple(a.dims) == tuple(b.dims) and set(a.coords) == set(b.coords), (tag, key)
    metric, var = key.split('.')
    bound, od = bounds[stat_of[metric], var]
    sw = np.asarray(state0.sum_weights[names[stat_of[metric]]][var].transpose(*od).values)
    av, bv = np.asarray(a.transpose(*od).values, np.float64), np.asarray(b.transpose(*od).values, np.float64)
    np.testing.assert_array_equal(np.isnan(av), np.isnan(bv), err_msg=f'{tag} {key}')
    with np.errstate(all='ignore'):
      tol = bound / sw
      if metric == 'rmse':
        tol = tol / (av + bv)
      tol = tol + ULPS * np.abs(bv)
      assert not np.nanmax(np.abs(av - bv) - tol) > 0.0, (tag, key, float(np.nanmax(np.abs(av - bv))), float(np.nanmax(tol)))


@pytest.mark.parametrize('payload', ['numpy', 'torch'])
@pytest.mark.parametrize('which', list(CASES))
def test_scores_on_against_off(monkeypatch, which, payload):
  case = CASES[which]
  pred, targ = _inputs(nans=case['nans'], mask=case['mask'])
  bounds = _bounds(case, pred, targ, QS, float32_host=payload == 'torch')
  if payload == 'torch':
    pred, targ = _on_device(pred), _on_device(targ)
  metrics = _metrics()
  monkeypatch.setattr(lazy, 'FUSED_ENS_QUANTILES', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(metrics, pred, targ, _aggregator(case))
  assert all(_is_fused(s) and s.is_lazy for per_var in stats.values() for s in per_var.values())
  launches = [e for e in engine.S1_EVENT_LOG if e['kind'] == 'brier']
  # the three statistics of a variable: ONE stage-1 launch; one launch per variable, nothing else
  assert len(launches) == 2 and len(engine.S1_EVENT_LOG) == 2, engine.S1_EVENT_LOG
  monkeypatch.setattr(lazy, 'FUSED_ENS_QUANTILES', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats0, state0, values0 = _evaluate(metrics, pred, targ, _aggregator(case))
  assert not any(_is_fused(s) for per_var in stats0.values() for s in per_var.values())
  assert not [e for e in engine.S1_EVENT_LOG if e['kind'] == 'brier']
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', None)
  _compare(case, metrics, (state, values), (state0, values0), bounds, f'{which} {payload}')


def test_more_quantiles_than_a_launch_holds_are_cut_into_blocks(monkeypatch):
  qs = [float(q) for q in np.round(np.linspace(0.0, 1.0, 37), 4)]
  case = dict(CASES['area-x-regions'], reduce=('latitude', 'longitude'))
  pred, targ = _inputs()
  metrics = _metrics(qs)
  monkeypatch.setattr(lazy, 'FUSED_ENS_QUANTILES', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(metrics, pred, targ, _aggregator(case))
  assert all(_is_fused(s) for per_var in stats.values() for s in per_var.values())
  assert [e['kind'] for e in engine.S1_EVENT_LOG] == ['brier'] * 6  # three blocks of at most sixteen per variable
  monkeypatch.setattr(lazy, 'FUSED_ENS_QUANTILES', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', None)
  _, state0, values0 = _evaluate(metrics, pred, targ, _aggregator(case))
  for name in _unique_names(metrics).values():
    np.testing.assert_array_equal(np.asarray(state.sum_weighted_statistics[name]['v'].coords['quantile'].values), qs)
  _compare(case, metrics, (state, values), (state0, values0), _bounds(case, pred, targ, qs, False), '37 quantiles')


def test_reducing_the_quantile_dim_keeps_the_host_route(monkeypatch):
  pred, targ = _inputs()
  metrics = _metrics()
  monkeypatch.setattr(lazy, 'FUSED_ENS_QUANTILES', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  agg = aggregation.Aggregator(reduce_dims=['quantile', 'latitude', 'longitude'])
  stats, state, _ = _evaluate(metrics, pred, targ, agg)
  assert all(_is_fused(s) for per_var in stats.values() for s in per_var.values())
  assert not [e for e in engine.S1_EVENT_LOG if e['kind'] == 'brier']
  monkeypatch.setattr(lazy, 'FUSED_ENS_QUANTILES', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', None)
  _, state0, _ = _evaluate(metrics, pred, targ, agg)
  for name in _unique_names(metrics).values():
    x, y = state.sum_weighted_statistics[name]['v'], state0.sum_weighted_statistics[name]['v']
    assert tuple(x.dims) == tuple(y.dims) == ('time',)
    np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=1e-12, atol=0)


def _chunk_job(n, nlead=2):
  import torch  # pylint: disable=g-import-not-at-top
  rng = np.random.default_rng(23)
  shape = (n, nlead) + SHAPE[1:]
  p_all = (rng.standard_normal((n, nlead, M) + SHAPE[1:]) * 3.0 + 280.0).astype(np.float32)
  t_all = (rng.standard_normal(shape) * 3.0 + 280.0).astype(np.float32)
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

  agg = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])
  return time_chunks.TimeChunks(inits, lead, init_time_chunk_size=1), load, agg, (p_all, t_all)


def test_chunk_loop_records_and_replays_with_identical_bytes(monkeypatch):
  """pipeline.evaluate_chunks over 8 one-init chunks of device-resident fields: the launch is part of the chunk record (chunks
  alternate between two launch streams: of each one builds, one is recorded, the rest are replayed -- more than two chunks replay),
  nothing is refused, the same loop without records gives the same accumulators bit for bit, and they are the restatement's sums."""
  times, load, agg, (p_all, t_all) = _chunk_job(8)
  metrics = _metrics()
  names = _unique_names(metrics)
  monkeypatch.setattr(lazy, 'FUSED_ENS_QUANTILES', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['recorded'] >= 1 and stats['replayed'] >= 2 and stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  assert set(state.sum_weighted_statistics) == set(off.sum_weighted_statistics) and len(state.sum_weighted_statistics) == 3
  for name in state.sum_weighted_statistics:
    np.testing.assert_array_equal(np.asarray(state.sum_weighted_statistics[name]['v'].values), np.asarray(off.sum_weighted_statistics[name]['v'].values))
    np.testing.assert_array_equal(np.asarray(state.sum_weights[name]['v'].values), np.asarray(off.sum_weights[name]['v'].values))
  pts = QC.points(np.moveaxis(p_all, 2, 0), t_all, QS).reshape(t_all.shape + (3, len(QS)))  # [init, lead, lat, lon, stat, quantile]
  w = O.grid_area_weights(LAT)[None, None, :, None, None]
  npoints = 8 * SHAPE[1] * SHAPE[2]
  for lane, sname in enumerate(STAT_NAMES):
    want = (pts[..., lane, :] * w).sum(axis=(0, 2, 3))
    bound = npoints * 2.0 ** -53 * (np.abs(pts[..., lane, :]) * w).sum(axis=(0, 2, 3))
    got = np.asarray(state.sum_weighted_statistics[names[sname]]['v'].transpose('lead_time', 'quantile').values)
    assert (np.abs(got - want) <= bound).all(), (sname, np.abs(got - want).max(), bound.max())
