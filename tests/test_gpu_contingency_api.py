"""Thresholded contingency scores through the public API on the device: WrappedMetric(CSI / ETS / FrequencyBias / SEDI, behind
ContinuousToBinary('both', thresholds)) on small fields (4 x 13 x 24) under a plain reduction, GridAreaWeighting, LatitudeBins
with a target mask, and skipna with NaNs.

Every sum (sum_weighted_statistics, sum_weights) is compared with whole-array float64 NumPy and with the same evaluation on the
host route (lazy.FUSED_CONTINGENCY = False) at rtol 1e-12: a sum is of at most N = 4 * 13 * 24 = 1248 non-negative fp64 terms in
another order, (N + 2) * 2^-52 = 2.8e-13.  The scores are ratios and differences of those sums, of order one: 1e-11 relative, and
absolute where a score cancels to ~0."""
import numpy as np
import pytest

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
from weatherbenchx_amd.metrics import categorical
from weatherbenchx_amd.metrics import wrappers

pytestmark = pytest.mark.gpu
DIMS = ('time', 'latitude', 'longitude')
SHAPE = (4, 13, 24)
THR = [1.0, 2.5, 0.5, 0.1, 1.0]  # unsorted, a duplicate
LAT = np.linspace(-90, 90, SHAPE[1])
LON = np.arange(SHAPE[2]) * (360.0 / SHAPE[2])
CELLS = ('TruePositives', 'FalsePositives', 'FalseNegatives', 'TrueNegatives')
RTOL = 1e-12


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.contingency_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


def _metrics(thresholds=THR):
  return {name: wrappers.WrappedMetric(m, [wrappers.ContinuousToBinary('both', thresholds, 'threshold')])
          for name, m in (('csi', categorical.CSI()), ('ets', categorical.ETS()), ('bias', categorical.FrequencyBias()), ('sedi', categorical.SEDI()))}


def _inputs(dtype=np.float32, nans=False, mask=False, seed=11, variables=('u', 'v')):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(SHAPE[0]), 'latitude': LAT, 'longitude': LON}
  pred, targ = {}, {}
  for v in variables:
    p, t = rng.gamma(2.0, size=SHAPE).astype(dtype), rng.gamma(2.0, size=SHAPE).astype(dtype)
    p[0, 0, :4] = [1.0, 2.5, np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(0))]  # ties, and both sides of 0.1
    if nans:
      p[rng.random(SHAPE) < 0.05] = np.nan
      t[rng.random(SHAPE) < 0.05] = np.nan
    tc = dict(cs)
    if mask:
      tc['mask'] = (DIMS[1:], rng.random(SHAPE[1:]) > 0.3)
    pred[v] = xr.DataArray(p, dims=DIMS, coords=cs, name=v)
    targ[v] = xr.DataArray(t, dims=DIMS, coords=tc, name=v)
  return pred, targ


def _area_weights():
  probe = xr.DataArray(np.zeros(SHAPE[1:]), dims=DIMS[1:], coords={'latitude': LAT, 'longitude': LON})
  w = weighting.GridAreaWeighting().weights(probe)
  return np.asarray(w.transpose(*[d for d in DIMS[1:] if d in w.dims]).values, np.float64).reshape(-1, 1) * np.ones((1, SHAPE[2]))


def _numpy_sums(p, t, thresholds, w, valid, skipna, bins=None):
  """-> {cell: (sum of w * cell, sum of w)} per threshold [and bin], float64 on the whole arrays; NaN where a NaN statistic under a
  valid point is not skipped.  w, valid: [latitude, longitude]; bins: bool [nbin, latitude] or None."""
  p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
  nan = np.isnan(p) | np.isnan(t)
  ok = np.broadcast_to(valid[None], p.shape) & (~nan if skipna else True)
  poisoned = np.broadcast_to(valid[None], p.shape) & nan & (not skipna)
  out = {}
  member = np.ones((1, SHAPE[1]), bool) if bins is None else bins
  for cell, name in enumerate(CELLS):
    sums = np.empty((len(thresholds), member.shape[0]))
    cnts = np.empty_like(sums)
    for k, thr in enumerate(thresholds):
      P, O = p > thr, t > thr
      ind = [(P & O), (P & ~O), (~P & O), (~P & ~O)][cell]
      for b in range(member.shape[0]):
        sel = ok & member[b][None, :, None]
        sums[k, b] = (np.where(sel & ind, 1.0, 0.0) * w[None]).sum()
        cnts[k, b] = (np.where(sel, 1.0, 0.0) * w[None]).sum()
        if (poisoned & member[b][None, :, None]).any():
          sums[k, b] = np.nan
    out[name] = (sums if bins is not None else sums[:, 0], cnts if bins is not None else cnts[:, 0])
  return out


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def _stat_key(cell, thresholds=THR):
  return f'{cell}_both_threshold=' + ','.join(str(x) for x in thresholds)


CASES = {
    'plain': dict(make=lambda: aggregation.Aggregator(reduce_dims=list(DIMS)), weights=False, nans=False, mask=False, skipna=False, bins=False),
    'area': dict(make=lambda: aggregation.Aggregator(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()]),
                 weights=True, nans=False, mask=False, skipna=False, bins=False),
    'latitude-bins-masked': dict(make=lambda: aggregation.Aggregator(reduce_dims=list(DIMS), bin_by=[binning.LatitudeBins(30)], masked=True),
                                 weights=False, nans=False, mask=True, skipna=False, bins=True),
    'skipna': dict(make=lambda: aggregation.Aggregator(reduce_dims=list(DIMS), skipna=True),
                   weights=False, nans=True, mask=False, skipna=True, bins=False),
}


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('which', list(CASES))
def test_scores_against_numpy_and_the_host_route(monkeypatch, which, dtype):
  case = CASES[which]
  pred, targ = _inputs(dtype, nans=case['nans'], mask=case['mask'])
  metrics = _metrics()
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(metrics, pred, targ, case['make']())
  assert all(isinstance(s, lazy.LazyContingency) and s.is_lazy for per_var in stats.values() for s in per_var.values())
  launches = [e for e in engine.S1_EVENT_LOG if e['kind'] == 'cont']
  assert len(launches) == 2 and len(engine.S1_EVENT_LOG) == 2, engine.S1_EVENT_LOG  # one launch per variable and aggregator
  # whole-array float64 NumPy
  w = _area_weights() if case['weights'] else np.ones(SHAPE[1:])
  bins = None
  if case['bins']:
    got_bins = state.sum_weights[_stat_key(CELLS[0])]['u']
    bin_dim = [d for d in got_bins.dims if d != 'threshold'][0]
    probe = xr.DataArray(np.zeros(SHAPE[1:]), dims=DIMS[1:], coords={'latitude': LAT, 'longitude': LON})
    m = binning.LatitudeBins(30).create_bin_mask(probe)
    bins = np.asarray(m.transpose(bin_dim, 'latitude', 'longitude').values, bool)[:, :, 0]
  for var in ('u', 'v'):
    valid = np.asarray(targ[var].coords['mask'].values, bool) if case['mask'] else np.ones(SHAPE[1:], bool)
    want = _numpy_sums(pred[var].values, targ[var].values, THR, w, valid, case['skipna'], bins)
    for cell in CELLS:
      sws, sw = state.sum_weighted_statistics[_stat_key(cell)][var], state.sum_weights[_stat_key(cell)][var]
      order = ('threshold',) + tuple(d for d in sws.dims if d != 'threshold')
      np.testing.assert_allclose(np.asarray(sws.transpose(*order).values), want[cell][0], rtol=RTOL, atol=0, err_msg=f'{cell} {var} sums')
      np.testing.assert_allclose(np.asarray(sw.transpose(*order).values), want[cell][1], rtol=RTOL, atol=0, err_msg=f'{cell} {var} weights')
      assert np.isfinite(np.asarray(sws.values)).all()
  # the same evaluation on the host route
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats0, state0, values0 = _evaluate(metrics, pred, targ, case['make']())
  assert not any(isinstance(s, lazy.LazyContingency) for per_var in stats0.values() for s in per_var.values())
  assert not [e for e in engine.S1_EVENT_LOG if e['kind'] == 'cont']
  for tree, tree0 in ((state.sum_weighted_statistics, state0.sum_weighted_statistics), (state.sum_weights, state0.sum_weights)):
    assert set(tree) == set(tree0)
    for stat in tree:
      for var in tree[stat]:
        x, y = tree[stat][var], tree0[stat][var]
        assert tuple(x.dims) == tuple(y.dims), (stat, var, x.dims, y.dims)
        assert set(x.coords) == set(y.coords), (stat, var, sorted(map(str, x.coords)), sorted(map(str, y.coords)))
        np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=RTOL, atol=0, err_msg=f'{stat} {var} vs the host route')
  assert set(values) == set(values0)
  for key in values:
    assert tuple(values[key].dims) == tuple(values0[key].dims) and set(values[key].coords) == set(values0[key].coords)
    np.testing.assert_allclose(np.asarray(values[key].values), np.asarray(values0[key].values), rtol=1e-11, atol=1e-11, equal_nan=True, err_msg=key)


def test_a_nan_under_a_valid_point_poisons_and_under_the_mask_does_not(monkeypatch):
  pred, targ = _inputs(mask=True, variables=('v',))
  valid = np.asarray(targ['v'].coords['mask'].values, bool)
  hidden, shown = np.argwhere(~valid)[0], np.argwhere(valid)[0]
  metrics = {'csi': _metrics()['csi']}
  make = lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude'], masked=True)
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY', True)
  pred['v'].data[2, hidden[0], hidden[1]] = np.nan
  _, state, _ = _evaluate(metrics, pred, targ, make())
  assert np.isfinite(np.asarray(state.sum_weighted_statistics[_stat_key('TruePositives')]['v'].values)).all()
  pred, targ = _inputs(mask=True, variables=('v',))
  targ['v'].data[1, shown[0], shown[1]] = np.nan
  _, state, _ = _evaluate(metrics, pred, targ, make())
  tp = state.sum_weighted_statistics[_stat_key('TruePositives')]['v'].transpose('latitude', 'threshold')
  bad = np.isnan(np.asarray(tp.values))
  assert bad[shown[0]].all() and not np.delete(bad, shown[0], axis=0).any()  # that latitude's row, every threshold, nothing else


def test_chunk_loop_records_and_replays(monkeypatch):
  """pipeline.evaluate_chunks over 8 one-init chunks of device-resident fields: the contingency launch is part of the chunk record
  (chunks alternate between two launch streams: of each kind one builds, one is recorded, the rest are replayed), nothing is
  refused, and the accumulated sums equal whole-array NumPy."""
  import torch  # pylint: disable=g-import-not-at-top
  n, nlead = 8, 2
  rng = np.random.default_rng(23)
  shape = (n, nlead) + SHAPE[1:]
  p_all, t_all = rng.gamma(2.0, size=shape).astype(np.float32), rng.gamma(2.0, size=shape).astype(np.float32)
  lead = (np.arange(nlead) * 12).astype('timedelta64[h]').astype('timedelta64[ns]')
  inits = np.datetime64('2020-01-01T00', 'ns') + np.arange(n) * np.timedelta64(24, 'h')
  index = {int(t.astype('int64')): i for i, t in enumerate(inits)}
  dims = ('init_time', 'lead_time', 'latitude', 'longitude')
  dev = [(torch.as_tensor(p_all[i:i + 1]).cuda(), torch.as_tensor(t_all[i:i + 1]).cuda()) for i in range(n)]

  def load(init_chunk, lead_chunk):
    del lead_chunk
    i = index[int(init_chunk[0].astype('int64'))]
    cs = {'init_time': init_chunk, 'lead_time': lead, 'latitude': LAT, 'longitude': LON}
    return {'v': xr.DataArray(dev[i][0], dims=dims, coords=cs)}, {'v': xr.DataArray(dev[i][1], dims=dims, coords=cs)}

  metrics = _metrics()
  agg = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])
  times = time_chunks.TimeChunks(inits, lead, init_time_chunk_size=1)
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['recorded'] >= 1 and stats['replayed'] >= 1 and stats['refused'] == 0 and not stats['refusals'], stats
  w = _area_weights()
  for lead_i in range(nlead):
    want = _numpy_sums(p_all[:, lead_i], t_all[:, lead_i], THR, w, np.ones(SHAPE[1:], bool), False)
    for cell in CELLS:
      sws = state.sum_weighted_statistics[_stat_key(cell)]['v'].transpose('lead_time', 'threshold')
      sw = state.sum_weights[_stat_key(cell)]['v'].transpose('lead_time', 'threshold')
      np.testing.assert_allclose(np.asarray(sws.values)[lead_i], want[cell][0], rtol=RTOL, atol=0, err_msg=f'{cell} lead {lead_i}')
      np.testing.assert_allclose(np.asarray(sw.values)[lead_i], want[cell][1], rtol=RTOL, atol=0, err_msg=f'{cell} lead {lead_i} weights')
  # ... and the same loop without records gives the same accumulators bit for bit
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  for cell in CELLS:
    np.testing.assert_array_equal(np.asarray(state.sum_weighted_statistics[_stat_key(cell)]['v'].values),
                                  np.asarray(off.sum_weighted_statistics[_stat_key(cell)]['v'].values))
