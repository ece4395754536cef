"""Contingency tables of ensemble event probabilities through the public API on the device: the documented chain
ContinuousToBinary('both') -> EnsembleMean('predictions') -> ContinuousToBinary / ContinuousToBins('predictions') under CSI, ETS,
RelativeEconomicValue (with and without optimal thresholds, one block of pairs and two) and Reliability, through the Aggregator
with the switch on and off in one process, on NumPy and HBM payloads, under a plain reduction, GridAreaWeighting, Regions bins, a
target mask with masked=True and skipna=True; a recorded and replayed chunk loop against the one-shot result.

Bounds.  Every per-point statistic is 0 or 1 (or NaN) on both routes, the same number.  Without weights a sum is an integer below
2^53 whatever the order of summation: the two routes agree exactly, sums, counts and metric values.  With weights w_i >= 0 an output
is sum_i w_i s_i over the n points it reduces, formed in two different orders: the host route adds n exact products (s_i is 0 or
1), the fused route rounds one product w_r N_r per row of integer counts N_r and adds those.  A floating-point sum of at most n
non-negative terms, each possibly rounded once, is off its exact value by at most n 2^-53 sum_i |w_i| to first order, so the two
differ by at most 2 n 2^-53 sum|w|; n and sum|w| are taken over every point the aggregator reduces, which bins and masks only
make smaller.  The ratio scores of weighted means (CSI, Reliability) are held to what that bound allows them (derived where it is
asserted); ETS and the relative economic value subtract and select, no bound on them is claimed: NaN positions only."""
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
from weatherbenchx_amd.metrics import multivariate
from weatherbenchx_amd.metrics import wrappers

pytestmark = pytest.mark.gpu
DIMS = ('time', 'latitude', 'longitude')
SHAPE = (4, 13, 24)
M = 5
EVENTS = [0.5, 1.0, 2.5]
EVENTS4 = [0.5, 1.0, 2.5, 4.0]
TAUS = [0.0, 0.2, 0.5, 1.0]
LAT = np.linspace(-90, 90, SHAPE[1])
LON = np.arange(SHAPE[2]) * (360.0 / SHAPE[2])
REGIONS = {'global': ((-90, 90), (0, 360)), 'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180))}
RATIOS = np.array([0.1, 0.5, 0.9])


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.ens_prob_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


def _chain(events=None):
  return [wrappers.ContinuousToBinary('both', EVENTS if events is None else events, 'event'), wrappers.EnsembleMean('predictions', 'number')]


def _metrics():
  optimal = xr.DataArray(np.array([0.1, 0.5, 0.9]), dims=['cost_loss_ratio'], coords={'cost_loss_ratio': RATIOS})
  return {
      'csi': wrappers.WrappedMetric(categorical.CSI(), _chain() + [wrappers.ContinuousToBinary('predictions', TAUS, 'prob')]),
      'ets': wrappers.WrappedMetric(categorical.ETS(), _chain() + [wrappers.ContinuousToBinary('predictions', TAUS, 'prob')]),
      'rev': wrappers.WrappedMetric(multivariate.RelativeEconomicValue(ensemble_size=M, cost_loss_ratios=RATIOS), _chain()),
      'rev_opt': wrappers.WrappedMetric(multivariate.RelativeEconomicValue(ensemble_size=M, cost_loss_ratios=RATIOS, optimal_thresholds=optimal,
                                                                           optimal_thresholds_select_nearest=True), _chain()),
      'rev20': wrappers.WrappedMetric(multivariate.RelativeEconomicValue(ensemble_size=M, cost_loss_ratios=RATIOS), _chain(EVENTS4)),  # 4 x 5 pairs
      'reliability': wrappers.WrappedMetric(categorical.Reliability(), _chain()),  # 3 x 10 pairs
  }


# launches of one variable: CSI and ETS share a group (3 x 4), the two REV metrics share their statistics (3 x 5), REV at four event
# thresholds is two blocks (4 x 4, 4 x 1), Reliability two (3 x 5 each)
LAUNCHES = sorted([(3, 4), (3, 5), (4, 4), (4, 1), (3, 5), (3, 5)])


def _inputs(nans=False, mask=False, seed=11, device=False):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(SHAPE[0]), 'latitude': LAT, 'longitude': LON}
  p = (np.round(rng.gamma(2.0, size=(M,) + SHAPE) * 4) / 4).astype(np.float32)  # ties with the event thresholds
  t = (np.round(rng.gamma(2.0, size=SHAPE) * 4) / 4).astype(np.float32)
  if nans:
    p[rng.random(p.shape) < 0.01] = np.nan
    t[rng.random(SHAPE) < 0.05] = np.nan
  tc = dict(cs)
  if mask:
    tc['mask'] = (DIMS[1:], rng.random(SHAPE[1:]) > 0.3)
  if device:
    import torch  # pylint: disable=g-import-not-at-top
    p, t = torch.as_tensor(p).cuda(), torch.as_tensor(t).cuda()
  pred = {'v': xr.DataArray(p, dims=('number',) + DIMS, coords=dict(cs, number=np.arange(M)), name='v')}
  targ = {'v': xr.DataArray(t, dims=DIMS, coords=tc, name='v')}
  return pred, targ


def _weight_sum(reduce_dims):
  probe = xr.DataArray(np.zeros(SHAPE[1:]), dims=DIMS[1:], coords={'latitude': LAT, 'longitude': LON})
  w = np.abs(np.asarray(weighting.GridAreaWeighting().weights(probe).values, np.float64)).reshape(-1, 1) * np.ones((1, SHAPE[2]))
  total = float(w.sum()) if 'latitude' in reduce_dims else float(w.sum(axis=1).max())
  return total * (SHAPE[0] if 'time' in reduce_dims else 1)


CASES = {
    'plain': dict(reduce=DIMS, kw=lambda: {}, nans=False, mask=False, weighted=False),
    'area-weights': dict(reduce=('latitude', 'longitude'), kw=lambda: dict(weigh_by=[weighting.GridAreaWeighting()]), nans=False, mask=False,
                         weighted=True),
    'regions': dict(reduce=DIMS, kw=lambda: dict(bin_by=[binning.Regions(REGIONS)]), nans=False, mask=False, weighted=False),
    'masked': dict(reduce=('time', 'longitude'), kw=lambda: dict(masked=True), nans=False, mask=True, weighted=False),
    'skipna': dict(reduce=('time', 'longitude'), kw=lambda: dict(skipna=True), nans=True, mask=False, weighted=False),
}


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyEnsProbContingency)


@pytest.mark.parametrize('payload', ['numpy', 'hbm'])
@pytest.mark.parametrize('which', list(CASES))
def test_metrics_on_both_routes(monkeypatch, which, payload):
  case = CASES[which]
  pred, targ = _inputs(nans=case['nans'], mask=case['mask'], device=payload == 'hbm')
  metrics = _metrics()
  make = lambda: aggregation.Aggregator(reduce_dims=list(case['reduce']), **case['kw']())
  monkeypatch.setattr(lazy, 'FUSED_ENS_PROB', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  with np.errstate(all='ignore'):
    stats, state, values = _evaluate(metrics, pred, targ, make())
  assert all(_is_fused(s) and s.is_lazy for per_var in stats.values() for s in per_var.values())
  # the fused route launched, the four cells of a group one launch per block of pairs, and nothing else ran in stage 1
  assert [e['kind'] for e in engine.S1_EVENT_LOG] == ['epc'] * len(LAUNCHES), engine.S1_EVENT_LOG
  # the same evaluation on the host route
  monkeypatch.setattr(lazy, 'FUSED_ENS_PROB', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  with np.errstate(all='ignore'):
    stats0, state0, values0 = _evaluate(metrics, pred, targ, make())
  assert not any(_is_fused(s) for per_var in stats0.values() for s in per_var.values())
  assert not [e for e in engine.S1_EVENT_LOG if e['kind'] == 'epc']
  n = int(np.prod([SHAPE[DIMS.index(d)] for d in case['reduce']]))
  bound = 2 * n * 2.0 ** -53 * _weight_sum(case['reduce']) if case['weighted'] else 0.0
  assert set(state.sum_weighted_statistics) == set(state0.sum_weighted_statistics)
  for name in state0.sum_weighted_statistics:
    for tree, tree0, what in ((state.sum_weighted_statistics, state0.sum_weighted_statistics, 'sums'), (state.sum_weights, state0.sum_weights, 'weights')):
      x, y = tree[name]['v'], tree0[name]['v']
      assert tuple(x.dims) == tuple(y.dims) and set(x.coords) == set(y.coords), (name, what, x.dims, y.dims)
      for k in y.coords:
        np.testing.assert_array_equal(np.asarray(x.coords[k].values), np.asarray(y.coords[k].values), err_msg=f'{name} {what}: {k}')
      xv, yv = np.asarray(x.values, np.float64), np.asarray(y.values, np.float64)
      np.testing.assert_array_equal(np.isnan(xv), np.isnan(yv), err_msg=f'{which} {name} {what}: NaN positions')
      print(which, payload, name, what, 'max |fused - host|:', float(np.nanmax(np.abs(xv - yv))) if np.isfinite(xv).any() else 0.0, 'bound', bound)
      np.testing.assert_allclose(xv, yv, rtol=0, atol=bound, equal_nan=True, err_msg=f'{which} {name} {what}')
      assert np.isfinite(xv).any()
  assert set(values) == set(values0)
  for key in values:
    assert tuple(values[key].dims) == tuple(values0[key].dims) and set(values[key].coords) == set(values0[key].coords), key
    a, b = np.asarray(values[key].values, np.float64), np.asarray(values0[key].values, np.float64)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=key)
    if not case['weighted']:  # the same integers in, the same arithmetic on them
      np.testing.assert_array_equal(a, b, err_msg=key)
  if case['weighted']:
    # The ratio scores under weights, from the bound B on the sums.  A mean is x = S / W with 0 <= x <= 1 and S, W each within B of the
    # other route's: |dx| <= (B + x B) / (W - B) <= d = 2 B / (W - B).  A score v = a / s, a one mean and s the sum of nb means with
    # a <= s, 0 <= v <= 1: |dv| <= (d + v nb d) / (s - nb d) <= (1 + nb) d / (s - nb d) wherever s > nb d.
    for key, needs in (('csi.v', ('TruePositives', 'FalsePositives', 'FalseNegatives')), ('reliability.v', ('TruePositives', 'FalsePositives'))):
      names = [metrics[key.split('.')[0]].statistics[c].unique_name for c in needs]
      w_min = min(float(np.asarray(state0.sum_weights[n]['v'].values).min()) for n in names)
      d = 2 * bound / (w_min - bound)
      total = None
      for n in names:
        mean = state0.sum_weighted_statistics[n]['v'] / state0.sum_weights[n]['v']
        total = mean if total is None else total + mean
      s_ = np.asarray(total.transpose(*values0[key].dims).values, np.float64)
      nb = len(needs)
      ok = s_ > 2 * nb * d
      tol = np.where(ok, (1 + nb) * d / np.where(ok, s_ - nb * d, 1.0), np.inf)
      a, b = np.asarray(values[key].values, np.float64), np.asarray(values0[key].values, np.float64)
      diff = np.abs(a - b)
      assert ok.any(), key
      print(which, payload, key, 'max |fused - host| of the scores:', float(np.nanmax(diff[ok])), 'smallest tolerance', float(tol[ok].min()))
      assert (diff[ok] <= tol[ok]).all(), (key, float(np.nanmax(diff[ok] - tol[ok])))


def test_the_launches_are_one_per_block_of_pairs(monkeypatch):
  pred, targ = _inputs()
  monkeypatch.setattr(lazy, 'FUSED_ENS_PROB', True)
  seen = []
  real = engine._KINDS['epc']  # pylint: disable=protected-access

  def operands(ctx, devs, func, ens, cat, mdim):
    out = real.operands(ctx, devs, func, ens, cat, mdim)
    seen.append((out[2].nthr, out[2].nslot))
    return out
  monkeypatch.setitem(engine._KINDS, 'epc', real._replace(operands=operands))  # pylint: disable=protected-access
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  _evaluate(_metrics(), pred, targ, aggregation.Aggregator(reduce_dims=['latitude', 'longitude']))
  assert sorted(seen) == LAUNCHES and len(engine.S1_EVENT_LOG) == len(LAUNCHES)


def test_a_nan_under_a_valid_point_poisons_and_under_the_mask_does_not(monkeypatch):
  monkeypatch.setattr(lazy, 'FUSED_ENS_PROB', True)
  metrics = {'csi': _metrics()['csi']}
  make = lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude'], masked=True)
  pred, targ = _inputs(mask=True)
  valid = np.asarray(targ['v'].coords['mask'].values, bool)
  hidden, shown = np.argwhere(~valid)[0], np.argwhere(valid)[0]
  pred['v'].data[3, 2, hidden[0], hidden[1]] = np.nan  # one member, hidden
  _, state, _ = _evaluate(metrics, pred, targ, make())
  for tree in state.sum_weighted_statistics.values():
    assert np.isfinite(np.asarray(tree['v'].values)).all()
  pred, targ = _inputs(mask=True)
  pred['v'].data[4, 1, shown[0], shown[1]] = np.nan  # one member, under a valid point
  _, state, _ = _evaluate(metrics, pred, targ, make())
  for tree in state.sum_weighted_statistics.values():
    bad = np.isnan(np.asarray(tree['v'].transpose('latitude', 'event', 'prob').values))
    assert bad[shown[0]].all() and not np.delete(bad, shown[0], axis=0).any()  # that latitude, every lane; nothing else


def _chunk_job(n, nlead=2):
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

  agg = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'])
  whole = ({'v': xr.DataArray(p_all, dims=pd, coords={'init_time': inits, 'lead_time': lead, 'latitude': LAT, 'longitude': LON})},
           {'v': xr.DataArray(t_all, dims=td, coords={'init_time': inits, 'lead_time': lead, 'latitude': LAT, 'longitude': LON})})
  return time_chunks.TimeChunks(inits, lead, init_time_chunk_size=1), load, agg, whole


def test_chunked_equals_unchunked_with_records_on(monkeypatch):
  """pipeline.evaluate_chunks over 8 one-init chunks of device-resident fields: the launch is part of the chunk record (recorded
  once per launch stream, then replayed), nothing is refused, and the accumulators are the one-shot aggregation of the whole arrays
  bit for bit: unweighted integer sums."""
  times, load, agg, whole = _chunk_job(8)
  metrics = {'csi': _metrics()['csi'], 'rev': _metrics()['rev']}
  monkeypatch.setattr(lazy, 'FUSED_ENS_PROB', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['recorded'] >= 1 and stats['replayed'] >= 1 and stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  engine.clear_caches()
  stats1, one, _ = _evaluate(metrics, whole[0], whole[1], agg)
  assert all(_is_fused(s) for per_var in stats1.values() for s in per_var.values())
  for name in one.sum_weighted_statistics:
    for tree, tree_off, tree1 in ((state.sum_weighted_statistics, off.sum_weighted_statistics, one.sum_weighted_statistics),
                                  (state.sum_weights, off.sum_weights, one.sum_weights)):
      x, y, z = tree[name]['v'], tree_off[name]['v'], tree1[name]['v']
      assert set(x.dims) == set(z.dims)
      np.testing.assert_array_equal(np.asarray(x.values), np.asarray(y.values))
      np.testing.assert_array_equal(np.asarray(x.transpose(*z.dims).values), np.asarray(z.values))
      assert np.asarray(z.values).any()
