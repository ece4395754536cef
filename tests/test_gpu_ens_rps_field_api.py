"""EnsembleRankedProbabilityScore at climatological threshold fields through the public API on the device: a Dataset of
[bin, dayofyear, latitude, longitude] terciles (K = 2), 4 members, a 2 x 3 (init_time, lead_time) chunk that crosses a year end
(days 365, 366, 1, 2 of a leap year), a 7 x 12 grid; host and device payloads; with and without a mask; one field for both sides and
two different ones; a field with NaN places under enforce_monotonicity=False; fields without a time dim; every host-only case of
the gate (tests/ens_rps_field_gate_cases.py); a recorded and replayed chunk loop.

Bit for bit: under a reduction over longitude alone every output is ONE stage-1 partial, float64(S) / float64(D) of the
restatement's integer sum S (tests/ens_rps_field_cases.py), whatever D is.
Bounds against the host route (lazy.FUSED_ENS_RPS_FIELD = False), as in tests/test_gpu_ens_rps_api.py: the two routes differ per point
by at most 16 * K * eps, so an output that sums N points by at most 16 * K * eps * N, and a mean by 16 * K * eps."""
import numpy as np
import pytest

import ens_rps_cases as EC
import ens_rps_field_cases as FC
import ens_rps_field_gate_cases as GC
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import pipeline
from weatherbenchx_amd import replay
from weatherbenchx_amd import time_chunks
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import probabilistic

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
M, K = 4, 2
LAT, LON = np.linspace(-75, 75, 7), np.arange(12) * 30.0
DAY = np.timedelta64(24, 'h').astype('timedelta64[ns]')
INITS = np.array(['2020-12-30', '2020-12-31'], 'datetime64[ns]')
LEADS = np.arange(3) * DAY
DOY = np.array([[365, 366, 1], [366, 1, 2]])  # the day of year of every (init, lead): 2020 is a leap year
FDIMS = ('init_time', 'lead_time', 'latitude', 'longitude')
SHAPE = (2, 3, 7, 12)


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.ens_rps_field_available(_hip.default_context())
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


def _terciles(seed, dtype=np.float32, nans=False):
  """[bin, dayofyear, latitude, longitude] on the grid of quarters the data sits on (ties), strictly increasing along bin."""
  rng = np.random.default_rng(seed)
  lower = np.round(rng.gamma(2.0, size=(366, 7, 12)) * 2) / 4
  data = np.stack([lower, lower + 0.25 + np.round(rng.gamma(2.0, size=lower.shape) * 2) / 4]).astype(dtype)
  if nans:  # places without a climatology, on a day the chunk selects and on one it does not
    data[0, 365, 2, 3] = data[1, 0, 4, 5] = data[1, 100, 0, 0] = np.nan
  return xr.DataArray(data, dims=('bin', 'dayofyear', 'latitude', 'longitude'),
                      coords={'bin': np.arange(K), 'dayofyear': np.arange(1, 367), 'latitude': LAT, 'longitude': LON}, name='v')


def _inputs(dtype=np.float32, mask=False, seed=11, inits=INITS):
  rng = np.random.default_rng(seed)
  shape = (len(inits),) + SHAPE[1:]
  cs = {'init_time': inits, 'lead_time': LEADS, 'latitude': LAT, 'longitude': LON}
  p = (np.round(rng.gamma(2.0, size=(M,) + shape) * 4) / 4).astype(dtype)
  t = (np.round(rng.gamma(2.0, size=shape) * 4) / 4).astype(dtype)
  tc = dict(cs)
  if mask:
    tc['mask'] = (FDIMS[2:], rng.random(SHAPE[2:]) > 0.3)
  return ({'v': xr.DataArray(p, dims=('number',) + FDIMS, coords=dict(cs, number=np.arange(M)), name='v')},
          {'v': xr.DataArray(t, dims=FDIMS, coords=tc, name='v')})


def _on_device(da):
  import torch  # pylint: disable=g-import-not-at-top
  coords = {k: (tuple(da.coords[k].dims), np.asarray(da.coords[k].values)) for k in da.coords}
  return xr.DataArray(torch.as_tensor(np.asarray(da.values)).cuda(), dims=da.dims, coords=coords, name=da.name)


def _selected(field, doy=DOY):
  """The thresholds every point reads: [init, lead, lat, lon, K]."""
  return np.moveaxis(np.asarray(field.values)[:, doy - 1], 0, -1)


def _rps(pf, tf, suffix='s', **kw):
  return probabilistic.EnsembleRankedProbabilityScore(xr.Dataset({'v': pf}), xr.Dataset({'v': tf}), 'bin', suffix, **kw)


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyStatistic) and stat._group.kind == 'erpsf'  # pylint: disable=protected-access


VARIANTS = {
    'one-field': dict(two=False, mask=False, nans=False),
    'two-fields': dict(two=True, mask=False, nans=False),
    'two-fields+mask': dict(two=True, mask=True, nans=False),
    'one-field+mask': dict(two=False, mask=True, nans=False),
    'nan-places': dict(two=True, mask=False, nans=True),
    'nan-places+mask': dict(two=False, mask=True, nans=True),
}


@pytest.mark.parametrize('payload', ['host', 'device'])
@pytest.mark.parametrize('pair', [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32)],
                         ids=['float32-float32', 'float32-float64', 'float64-float32'])
@pytest.mark.parametrize('which', list(VARIANTS))
def test_scores_against_the_restatement_and_the_host_route(monkeypatch, which, pair, payload):
  v = VARIANTS[which]
  pred, targ = _inputs(pair[0], mask=v['mask'])
  pf = _terciles(3, pair[1], nans=v['nans'])
  tf = _terciles(4, pair[1], nans=v['nans']) if v['two'] else pf
  a, b = _selected(pf), _selected(tf)
  p_np, t_np = np.asarray(pred['v'].values), np.asarray(targ['v'].values)
  valid = np.asarray(targ['v'].coords['mask'].values, bool) if v['mask'] else np.ones(SHAPE[2:], bool)
  if payload == 'device':
    pred, targ = {'v': _on_device(pred['v'])}, {'v': _on_device(targ['v'])}
    pf, tf = (_on_device(pf), _on_device(tf)) if v['two'] else (_on_device(pf),) * 2
  for fair in (True, False):
    kw = dict(fair=fair, enforce_monotonicity=not v['nans'])
    metrics = {'rps': _StatisticAsMetric(_rps(pf, tf, **kw))}
    name = _rps(pf, tf, **kw).unique_name
    # every output one partial: bit for bit
    monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', True)
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    stats, state, _ = _evaluate(metrics, pred, targ, aggregation.Aggregator(reduce_dims=['longitude'], masked=v['mask']))
    assert _is_fused(stats[name]['v']) and stats[name]['v'].is_lazy
    assert [e['kind'] for e in engine.S1_EVENT_LOG] == ['erpsf'], engine.S1_EVENT_LOG
    num = FC.numerators(p_np, t_np, a, b, fair, True).astype(np.float64)
    nan = FC.nan_points(p_np, t_np, a, b)
    assert nan.any() == v['nans']
    num[nan] = np.nan
    want = np.where(valid[None, None], num, 0.0).sum(axis=-1) / EC.denominator(M, fair)
    got = state.sum_weighted_statistics[name]['v']
    np.testing.assert_array_equal(np.asarray(got.transpose(*FDIMS[:3]).values), want, err_msg=f'{which} fair={fair}')
    assert np.isnan(want).any() == (v['nans'] and (not v['mask'] or bool((nan & valid[None, None]).any())))
    # against the host route: everything reduced; with NaN places latitude is kept, so that a NaN under a valid point poisons its
    # latitude on both routes alike and the other latitudes still compare as numbers
    reduce_dims = [d for d in FDIMS if d != 'latitude'] if v['nans'] else list(FDIMS)
    npoint = int(np.prod([SHAPE[FDIMS.index(d)] for d in reduce_dims]))
    agg = lambda: aggregation.Aggregator(reduce_dims=reduce_dims, masked=v['mask'])
    _, state, values = _evaluate(metrics, pred, targ, agg())
    monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', False)
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    stats0, state0, values0 = _evaluate(metrics, pred, targ, agg())
    assert not _is_fused(stats0[name]['v']) and not [e for e in engine.S1_EVENT_LOG if e['kind'] == 'erpsf']
    x, y = state.sum_weighted_statistics[name]['v'], state0.sum_weighted_statistics[name]['v']
    assert tuple(x.dims) == tuple(y.dims)
    xv, yv = np.asarray(x.values), np.asarray(y.values)
    np.testing.assert_array_equal(np.isnan(xv), np.isnan(yv), err_msg=f'{which} fair={fair}: NaN positions')
    if v['nans']:
      poisoned = (nan & valid[None, None]).any(axis=(0, 1, 3))
      np.testing.assert_array_equal(np.isnan(np.asarray(x.transpose('latitude').values)), poisoned)
      assert not poisoned.all() and (poisoned.any() or v['mask'])
    bound = 16 * K * EPS * npoint
    print(which, payload, fair, 'max |fused - host| of the sums:', float(np.nanmax(np.abs(xv - yv))), 'bound', bound)
    np.testing.assert_allclose(xv, yv, rtol=0, atol=bound, equal_nan=True)
    np.testing.assert_allclose(np.asarray(state.sum_weights[name]['v'].values), np.asarray(state0.sum_weights[name]['v'].values), rtol=1e-12)
    np.testing.assert_allclose(np.asarray(values['rps.v'].values), np.asarray(values0['rps.v'].values), rtol=0, atol=16 * K * EPS, equal_nan=True)


@pytest.mark.parametrize('payload', ['host', 'device'])
def test_fields_without_a_time_dim_are_read_in_place_too(monkeypatch, payload):
  """[bin] and [bin, latitude, longitude] thresholds: nothing to gather (no gather table), zero strides along what the field does not
  vary over; one field and two stacked ones.  Every output one partial: bit for bit."""
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', True)
  pred, targ = _inputs()
  p_np, t_np = np.asarray(pred['v'].values), np.asarray(targ['v'].values)
  levels = xr.DataArray(np.array([0.75, 2.5], np.float64), dims=['bin'], name='v')
  places = _terciles(3).isel(dayofyear=0, drop=True)
  places2 = _terciles(4).isel(dayofyear=0, drop=True)
  if payload == 'device':
    pred, targ = {'v': _on_device(pred['v'])}, {'v': _on_device(targ['v'])}
  for pf, tf in ((levels, levels), (places, places), (places, places2)):
    a = np.broadcast_to(np.moveaxis(np.asarray(pf.values), 0, -1), SHAPE + (K,))
    b = np.broadcast_to(np.moveaxis(np.asarray(tf.values), 0, -1), SHAPE + (K,))
    if payload == 'device':
      pf, tf = (_on_device(pf),) * 2 if pf is tf else (_on_device(pf), _on_device(tf))
    for fair in (True, False):
      stat = _rps(pf, tf, fair=fair)
      monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
      stats, state, _ = _evaluate({'rps': _StatisticAsMetric(stat)}, pred, targ, aggregation.Aggregator(reduce_dims=['longitude']))
      assert _is_fused(stats[stat.unique_name]['v']) and [e['kind'] for e in engine.S1_EVENT_LOG] == ['erpsf']
      want = FC.numerators(p_np, t_np, a, b, fair, True).astype(np.float64).sum(axis=-1) / EC.denominator(M, fair)
      np.testing.assert_array_equal(np.asarray(state.sum_weighted_statistics[stat.unique_name]['v'].transpose(*FDIMS[:3]).values), want)


def _outcome(stat, p, t, agg):
  """What an evaluation gives: ('values', dims, the means, whether a statistic was fused, the kinds launched) or ('raises', the
  cause's type and text)."""
  engine.S1_EVENT_LOG = []
  try:
    with np.errstate(all='ignore'):
      stats, _, values = _evaluate({'rps': _StatisticAsMetric(stat)}, {'v': p}, {'v': t}, agg)
  except (ValueError, KeyError) as err:
    cause = err.__cause__ if err.__cause__ is not None else err
    return 'raises', type(cause).__name__, str(cause)
  out = values['rps.v']
  return 'values', tuple(out.dims), np.asarray(out.values), _is_fused(stats[stat.unique_name]['v']), [e['kind'] for e in engine.S1_EVENT_LOG]


@pytest.mark.parametrize('case', GC.host_cases(), ids=lambda c: c['what'].replace(' ', '-'))
def test_host_only_cases_fall_back_and_still_agree(monkeypatch, case):
  """Every case the gate (or what follows it in the statistic) keeps on the host, through the Aggregator on the device with the
  launch available: no 'erpsf' statistic, no such launch, and the outcome -- the means over (latitude, longitude), or the host
  route's exception -- is that of WBX_FUSED_ENS_RPS_FIELD=0, bit for bit, and within 16 K eps of the restatement where that applies
  to the case as it stands."""
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  kw = {k: v for k, v in case['kw'].items() if k != 'bin_dim'}
  stat = lambda: probabilistic.EnsembleRankedProbabilityScore(case['pf'], case['tf'], case['kw'].get('bin_dim', 'bin'), 's', **kw)
  agg = lambda: aggregation.Aggregator(reduce_dims=['latitude', 'longitude'])
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', True)
  got = _outcome(stat(), case['p'], case['t'], agg())
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', False)
  want = _outcome(stat(), case['p'], case['t'], agg())
  assert got[:2] == want[:2], (got[:2], want[:2])
  if got[0] == 'raises':
    assert got[2] == want[2]
    assert not case['restate']
    return
  assert not got[3] and 'erpsf' not in got[4], got[3:]
  np.testing.assert_array_equal(got[2], want[2])
  if case['restate']:
    p, t = case['p'], case['t']
    p_np, t_np = np.asarray(p.values), np.asarray(t.values)
    a, b = GC.selected(case['pf'], p, t.dims), GC.selected(case['tf'], t, t.dims)
    fair, k = case['kw'].get('fair', True), a.shape[-1]
    points = FC.numerators(p_np, t_np, a, b, fair, True) / EC.denominator(p_np.shape[0], fair)
    np.testing.assert_allclose(got[2], points.mean(axis=(-2, -1)), rtol=0, atol=16 * k * EPS)


def test_chunk_loop_records_and_replays_with_identical_bytes(monkeypatch):
  """pipeline.evaluate_chunks over 8 one-init chunks of device-resident fields across the year end: every chunk gathers other days
  of the field through its own gather table, the launch is part of the chunk record, nothing is refused, and the same loop without
  records gives the same accumulators bit for bit -- the restatement's numbers."""
  n = 8
  inits = np.datetime64('2020-12-27', 'ns') + np.arange(n) * DAY
  pred, targ = _inputs(inits=inits, seed=23)
  p_all, t_all = np.asarray(pred['v'].values), np.asarray(targ['v'].values)
  dev_p = [_on_device(pred['v'].isel(init_time=slice(i, i + 1))) for i in range(n)]
  dev_t = [_on_device(targ['v'].isel(init_time=slice(i, i + 1))) for i in range(n)]
  index = {int(t.astype('int64')): i for i, t in enumerate(inits)}

  def load(init_chunk, lead_chunk):
    del lead_chunk
    i = index[int(init_chunk[0].astype('int64'))]
    return {'v': dev_p[i]}, {'v': dev_t[i]}

  f, g = _on_device(_terciles(3)), _on_device(_terciles(4))
  metrics = {'rps': _StatisticAsMetric(_rps(f, g)), 'unfair': _StatisticAsMetric(_rps(f, f, suffix='u', fair=False))}
  times = time_chunks.TimeChunks(inits, LEADS, init_time_chunk_size=1)
  agg = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'])
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['recorded'] >= 1 and stats['replayed'] >= 1 and stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  valid = inits[:, None] + LEADS[None, :]
  doy = (valid.astype('datetime64[D]') - valid.astype('datetime64[Y]').astype('datetime64[D]')).astype(np.int64) + 1
  for stat, a, b, fair in ((_rps(f, g), _selected(_terciles(3), doy), _selected(_terciles(4), doy), True),
                           (_rps(f, f, suffix='u', fair=False), _selected(_terciles(3), doy), _selected(_terciles(3), doy), False)):
    name = stat.unique_name
    got = state.sum_weighted_statistics[name]['v']
    np.testing.assert_array_equal(np.asarray(got.values), np.asarray(off.sum_weighted_statistics[name]['v'].values))
    np.testing.assert_array_equal(np.asarray(state.sum_weights[name]['v'].values), np.asarray(off.sum_weights[name]['v'].values))
    want = FC.numerators(p_all, t_all, a, b, fair, True).sum(axis=(0, 2, 3)) / EC.denominator(M, fair)
    np.testing.assert_allclose(np.asarray(got.transpose('lead_time').values), want, rtol=8 * n * EPS, atol=0)  # (stage 2 and the chunks add partials)
