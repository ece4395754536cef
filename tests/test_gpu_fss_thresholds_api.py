"""FSS and its three statistics behind ContinuousToBinary('both', thresholds, dim) through the public API on the device: continuous
fields of 3 x 12 x 16 with ties at the thresholds and a few +-inf, the fused route (wbx_fss_threshold_partial) on and off, against
each other and against the oracle; with and without GridAreaWeighting and a `mask` coordinate, skipna, Regions bins, a scalar size and
a list, more than 16 thresholds, NumPy and torch-on-device payloads; the entry calls that were made; chunk loops that record and replay;
the declined cases on the host route.

Bound between the routes: that of tests/test_gpu_fss_api.py.  Both routes' fractions of a 0 / 1 field are within half an ulp of float32
of the exact quotient (the kernel's is the rounding of count / n^2, the host route's that of a float64 mean of means), so they differ
by at most one ulp; fss_cases.mean_bound_from_ulps carries one ulp per fraction through the three float32 squares, and a sum of n such
terms under weights W <= Wmax moves by at most Wmax (sum of the per-point bounds + (n + 4) 2^-52 sum |value|)."""
import numpy as np
import pytest

import fss_cases as FC
import fss_threshold_cases as TC
import test_gpu_fss_api as TA
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
from weatherbenchx_amd.metrics import spatial
from weatherbenchx_amd.metrics import wrappers

pytestmark = pytest.mark.gpu
V, DIMS, SHAPE, COORDS, REGIONS, TERMS = TA.V, TA.DIMS, TA.SHAPE, TA.COORDS, TA.REGIONS, TA.TERMS
THR = 'threshold'
ENTRY = 'wbx_fss_threshold_partial'
MANY = [round(0.04 + 0.05 * j, 2) for j in range(19)]  # more than a call holds: blocks of 16 and 3


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.fss_available(_hip.default_context())
  assert engine.fss_thresholds_available(_hip.default_context()), 'the library lacks wbx_fss_threshold_partial'
  engine.clear_caches()
  yield
  engine.clear_caches()


@pytest.fixture
def entry_calls(monkeypatch):
  """Every call of the entry, as (n, nthr), whoever makes it."""
  lib = _hip.load_library()
  real = getattr(lib, ENTRY)
  calls = []

  def counted(*args):
    calls.append((int(args[3]), int(args[4])))
    return real(*args)
  monkeypatch.setitem(lib.__dict__, ENTRY, counted)
  return calls


def fields(dtype, thresholds, seed=43):
  """Continuous, without NaN (a case adds its own): ties at every threshold, a few +-inf."""
  return TC.continuous_fields(SHAPE, dtype, seed, thresholds, nan_share=0.0)


def metric_of(sizes, wrap, thresholds, combine_mask=False):
  return wrappers.WrappedMetric(spatial.FSS(sizes, wrap_longitude=wrap, combine_mask=combine_mask),
                                [wrappers.ContinuousToBinary('both', list(thresholds), THR)])


def evaluate(pred, targ, sizes, wrap, thresholds, agg_kw, combine_mask=False):
  metrics = {'fss': metric_of(sizes, wrap, thresholds, combine_mask)}
  with np.errstate(all='ignore'):
    stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
    state = aggregation.Aggregator(**agg_kw).aggregate_statistics(stats)
    score = state.metric_values(metrics)[f'fss.{V}']
  names = {t: next(k for k in stats if k.startswith(t + '_')) for t in TERMS}
  return ({t: stats[names[t]][V] for t in TERMS}, {t: state.sum_weighted_statistics[names[t]][V] for t in TERMS},
          {t: state.sum_weights[names[t]][V] for t in TERMS}, score)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyFSS) and stat.threshold_dim == THR


SHORT = [0.1, 0.5, 0.75]
CASES = {
    'plain_list': dict(sizes=[1, 3, 5], wrap=True, kw=lambda: dict(reduce_dims=list(DIMS))),
    'plain_scalar_no_wrap': dict(sizes=5, wrap=False, thresholds=[0.5], kw=lambda: dict(reduce_dims=list(DIMS))),
    'area': dict(sizes=[1, 3, 5, 11], wrap=True, thresholds=TC.THRESHOLD_LISTS[TC.NAN_INF],
                 kw=lambda: dict(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()])),
    'area_many_thresholds': dict(sizes=[3, 5], wrap=True, thresholds=MANY,
                                 kw=lambda: dict(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()])),
    'keep_time': dict(sizes=[3, 5], wrap=False, kw=lambda: dict(reduce_dims=['latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])),
    'masked_nan_target': dict(sizes=3, wrap=True, nan_target=True, kw=lambda: dict(reduce_dims=list(DIMS), masked=True)),
    'masked_list_area': dict(sizes=[1, 3], wrap=True, nan_target=True, thresholds=TC.THRESHOLD_LISTS[7],
                             kw=lambda: dict(reduce_dims=list(DIMS), masked=True, weigh_by=[weighting.GridAreaWeighting()])),
    'combine_mask': dict(sizes=[3, 5], wrap=False, nan_target=True, p_mask=True, combine_mask=True,
                         kw=lambda: dict(reduce_dims=list(DIMS), masked=True)),
    'skipna': dict(sizes=[1, 3], wrap=True, nan_target=True, no_mask=True, kw=lambda: dict(reduce_dims=list(DIMS), skipna=True)),
    'skipna_scalar_many': dict(sizes=3, wrap=True, nan_target=True, no_mask=True, thresholds=MANY,
                               kw=lambda: dict(reduce_dims=list(DIMS), skipna=True)),
    'regions': dict(sizes=[3, 5], wrap=True, kw=lambda: dict(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()],
                                                            bin_by=[binning.Regions(REGIONS)])),
    'regions_masked': dict(sizes=3, wrap=True, nan_target=True,
                           kw=lambda: dict(reduce_dims=list(DIMS), masked=True, weigh_by=[weighting.GridAreaWeighting()],
                                           bin_by=[binning.Regions(REGIONS)])),
}
PAYLOADS = {'float32-numpy': (np.float32, False), 'float64-numpy': (np.float64, False), 'float32-torch': (np.float32, True)}


def _inputs(case, dtype, device):
  p, t = fields(dtype, case.get('thresholds', SHORT))
  t_mask = p_mask = None
  if case.get('nan_target'):
    t, valid = TA._nan_target(t)  # pylint: disable=protected-access
    t_mask = None if case.get('no_mask') else valid
  if case.get('p_mask'):
    p_mask = np.ones(p.shape, bool)
    p_mask[0, 2:4, 1:3] = False
  return p, t, TA.labelled(p, device, p_mask), TA.labelled(t, device, t_mask)


@pytest.mark.parametrize('payload', list(PAYLOADS))
@pytest.mark.parametrize('case_name', list(CASES))
def test_scores_with_the_route_on_and_off(monkeypatch, entry_calls, case_name, payload):
  case = CASES[case_name]
  dtype, device = PAYLOADS[payload]
  thresholds = case.get('thresholds', SHORT)
  p, t, pred, targ = _inputs(case, dtype, device)
  sizes, wrap = case['sizes'], case['wrap']
  size_list = sizes if isinstance(sizes, list) else [sizes]
  monkeypatch.setattr(lazy, 'FUSED_FSS', True)
  monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', True)
  a, x, wx, score = evaluate(pred, targ, sizes, wrap, thresholds, case['kw'](), case.get('combine_mask', False))
  assert all(_is_fused(a[k]) and a[k].is_lazy for k in TERMS)
  # the fused route was taken: ONE call of the entry per size and block of at most 16 thresholds for the three statistics
  blocks = [min(16, len(thresholds) - j) for j in range(0, len(thresholds), 16)]
  assert entry_calls == [(n, b) for n in size_list for b in blocks], entry_calls
  del entry_calls[:]
  monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', False)
  engine.clear_caches()
  b, y, wy, score0 = evaluate(pred, targ, sizes, wrap, thresholds, case['kw'](), case.get('combine_mask', False))
  assert not any(_is_fused(b[k]) for k in TERMS) and not entry_calls
  n = int(np.prod(SHAPE))
  kw = case['kw']()
  wmax = 1.0
  if kw.get('weigh_by'):
    probe = xr.DataArray(np.zeros(SHAPE[1:]), dims=DIMS[1:], coords={d: COORDS[d] for d in DIMS[1:]})
    wmax = float(np.asarray(weighting.GridAreaWeighting().weights(probe).values).max())
  pairs = [TC.binarized_pair(p, t, thr) for thr in thresholds]
  bounds = [FC.mean_bound_from_ulps(FC.fractions(pb, k, wrap), FC.fractions(tb, k, wrap)) for k in size_list for pb, tb in pairs]
  values = [FC.point_values(pb, tb, k, wrap) for k in size_list for pb, tb in pairs]
  for l, term in enumerate(TERMS):
    TA._same_labels(a[term], b[term])  # pylint: disable=protected-access
    TA._same_labels(x[term], y[term])  # pylint: disable=protected-access
    lead = ('neighborhood_size',) if isinstance(sizes, list) else ()
    assert tuple(a[term].dims) == lead + ('time', THR, 'latitude', 'longitude')
    assert THR in x[term].dims and x[term].sizes[THR] == len(thresholds)
    np.testing.assert_array_equal(np.asarray(x[term].coords[THR].values), np.asarray(thresholds))
    tol = wmax * max(float(np.nansum(bk[l])) + (n + 4) * 2.0 ** -52 * float(np.nansum(np.abs(vk[l]))) for bk, vk in zip(bounds, values))
    gx, gy = np.asarray(x[term].values), np.asarray(y[term].values)
    print(case_name, payload, term, 'max |fused - host| of the sums:', float(np.nanmax(np.abs(gx - gy))), 'bound', tol)
    np.testing.assert_array_equal(np.isnan(gx), np.isnan(gy))
    assert np.isfinite(gx).any() and np.nansum(np.abs(gx)) > 0
    np.testing.assert_allclose(gx, gy, rtol=0, atol=tol)
    np.testing.assert_allclose(np.asarray(wx[term].values), np.asarray(wy[term].values), rtol=1e-12, atol=0)
  TA._same_labels(score, score0)  # pylint: disable=protected-access
  np.testing.assert_allclose(np.asarray(score.values), np.asarray(score0.values), rtol=2e-6, equal_nan=True)
  if case_name in ('plain_list', 'plain_scalar_no_wrap'):  # both routes against the oracle
    for route in (score, score0):
      got = np.asarray(route.values).reshape(len(size_list), len(thresholds))
      with np.errstate(all='ignore'):
        want = [[O.fractions_skill_score(*TC.binarized_pair(p, t, thr), k, wrap) for thr in thresholds] for k in size_list]
      np.testing.assert_allclose(got, want, rtol=2e-6)


@pytest.mark.parametrize('term', TERMS)
def test_a_statistic_alone_through_the_aggregator(monkeypatch, entry_calls, term):
  thresholds = TC.THRESHOLD_LISTS[TC.KB + 1]
  p, t = fields(np.float32, thresholds)
  cls = getattr(spatial, term)
  out = {}
  for on in (True, False):
    monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', on)
    del entry_calls[:]
    engine.clear_caches()
    stat = wrappers.WrappedStatistic(cls([3, 5], wrap_longitude=True), wrappers.ContinuousToBinary('both', thresholds, THR))
    per_var = stat.compute(TA.labelled(p, False), TA.labelled(t, False))
    assert _is_fused(per_var[V]) == on
    state = aggregation.Aggregator(reduce_dims=['latitude', 'longitude']).aggregate_statistics({stat.unique_name: per_var})
    assert len(entry_calls) == (2 if on else 0)
    out[on] = state.mean_statistics()[stat.unique_name][V]
  TA._same_labels(out[True], out[False])  # pylint: disable=protected-access
  assert out[True].dims == ('neighborhood_size', 'time', THR)
  l = TERMS.index(term)
  for i, k in enumerate((3, 5)):
    want = TC.point_values(p, t, thresholds, k, True)[:, l].mean(axis=(2, 3)).T  # [time, K]
    np.testing.assert_allclose(np.asarray(out[True].values)[i], want, rtol=1e-12)
    np.testing.assert_allclose(np.asarray(out[False].values)[i], want, rtol=1e-6)


def test_one_call_per_size_and_block_and_none_for_a_second_aggregation(monkeypatch, entry_calls):
  """The test that fails without the feature: the three statistics of a variable share one call of wbx_fss_threshold_partial per size
  and block of thresholds, and no binarised field is reduced."""
  monkeypatch.setattr(lazy, 'FUSED_FSS', True)
  monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  p, t = fields(np.float32, MANY)
  metrics = {'fss': metric_of([1, 3, 5], True, MANY)}
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, TA.labelled(p, False), TA.labelled(t, False))
  assert len(stats) == 3 and all(_is_fused(s[V]) for s in stats.values())
  assert len({id(s[V]._group) for s in stats.values()}) == 1  # pylint: disable=protected-access
  agg = aggregation.Aggregator(reduce_dims=list(DIMS))
  agg.aggregate_statistics(stats)
  assert entry_calls == [(1, 16), (1, 3), (3, 16), (3, 3), (5, 16), (5, 3)]
  assert [e['kind'] for e in engine.S1_EVENT_LOG] == ['fss'] * 6, engine.S1_EVENT_LOG
  agg.aggregate_statistics(stats)
  assert len(entry_calls) == 6 and len(engine.S1_EVENT_LOG) == 6


def test_per_point_values_are_the_host_routes_with_their_type(monkeypatch, entry_calls):
  import torch  # pylint: disable=g-import-not-at-top
  p, t = fields(np.float32, SHORT)
  for device in (False, True):
    res = {}
    for on in (True, False):
      monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', on)
      stat = wrappers.WrappedStatistic(spatial.SquaredFractionsError([1, 3]), wrappers.ContinuousToBinary('both', SHORT, THR))
      res[on] = stat.compute(TA.labelled(p, device), TA.labelled(t, device))[V]
    a, b = res[True], res[False]
    assert _is_fused(a) and not _is_fused(b)
    TA._same_labels(a, b)  # pylint: disable=protected-access
    assert a.dims == b.dims == ('neighborhood_size', 'time', THR, 'latitude', 'longitude') and tuple(a.shape) == tuple(b.shape)
    da, db = a.data, b.data
    assert type(da) is type(db)
    if device:
      assert torch.is_tensor(da) and da.dtype == db.dtype and da.device == db.device
    assert FC.same_numbers(np.asarray(a.values, np.float64), np.asarray(b.values, np.float64))
    assert not entry_calls  # a reader of points gets the host route's array
    engine.clear_caches()


def _labelled_thresholds():
  return xr.DataArray(np.asarray(SHORT), dims=[THR], coords={THR: np.asarray(SHORT)})


DECLINED = {
    'labelled thresholds': dict(transform=lambda: wrappers.ContinuousToBinary('both', _labelled_thresholds(), THR, unique_name_suffix='s')),
    'the threshold dim reduced': dict(reduce_dims=list(DIMS) + [THR], counted='reduced'),
    'longitude not innermost': dict(order=('time', 'longitude', 'latitude')),
    'float16 inputs': dict(dtype=np.float16),
}


@pytest.mark.parametrize('why', list(DECLINED))
def test_a_declined_case_takes_the_host_route(monkeypatch, entry_calls, why):
  """No call of the entry, and the very numbers the route gives with the switch off."""
  case = DECLINED[why]
  p, t = fields(np.float32, SHORT)
  p, t = p.astype(case.get('dtype', np.float32)), t.astype(case.get('dtype', np.float32))
  pred, targ = TA.labelled(p, False), TA.labelled(t, False)
  if 'order' in case:
    pred = {V: xr.DataArray(np.ascontiguousarray(pred[V].transpose(*case['order']).values), dims=case['order'], coords=COORDS)}
    targ = {V: xr.DataArray(np.ascontiguousarray(targ[V].transpose(*case['order']).values), dims=case['order'], coords=COORDS)}
  transform = case.get('transform', lambda: wrappers.ContinuousToBinary('both', SHORT, THR))
  out = {}
  for on in (True, False):
    monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', on)
    monkeypatch.setattr(lazy, 'FSS_STATS', {'plan_declined': 0, 'reasons': []})
    engine.clear_caches()
    metrics = {'fss': wrappers.WrappedMetric(spatial.FSS([1, 3], wrap_longitude=True), [transform()])}
    with np.errstate(all='ignore'):
      stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
      state = aggregation.Aggregator(reduce_dims=case.get('reduce_dims', list(DIMS))).aggregate_statistics(stats)
    assert not entry_calls, why
    if on and case.get('counted'):
      assert lazy.FSS_STATS['plan_declined'] == 3 and case['counted'] in lazy.FSS_STATS['reasons'][0]  # (one per statistic)
    out[on] = {k: np.asarray(v[V].values) for k, v in state.sum_weighted_statistics.items()}
  assert len(out[True]) == 3
  for k in out[True]:
    assert np.isfinite(out[True][k]).any()
    np.testing.assert_array_equal(out[True][k], out[False][k])


def _chunk_job(n_chunks, sizes, thresholds):
  import torch  # pylint: disable=g-import-not-at-top
  cdims = ('init_time', 'lead_time', 'latitude', 'longitude')
  inits = np.array([f'2020-03-0{1 + i}T00' for i in range(n_chunks)], dtype='datetime64[ns]')
  lead = np.array([0, 6], dtype='timedelta64[h]').astype('timedelta64[ns]')
  index = {int(t.astype('int64')): i for i, t in enumerate(inits)}
  dev = []
  for i in range(n_chunks):
    p, t = TC.continuous_fields((1, 2) + SHAPE[1:], np.float32, 60 + i, thresholds, nan_share=0.0)
    dev.append((torch.as_tensor(p).cuda(), torch.as_tensor(t).cuda()))

  def load(init_chunk, lead_chunk):
    del lead_chunk
    i = index[int(init_chunk[0].astype('int64'))]
    cs = {'init_time': inits[i:i + 1], 'lead_time': lead, 'latitude': COORDS['latitude'], 'longitude': COORDS['longitude']}
    return ({V: xr.DataArray(dev[i][0], dims=cdims, coords=cs)}, {V: xr.DataArray(dev[i][1], dims=cdims, coords=cs)})

  agg = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])
  return time_chunks.TimeChunks(inits, lead, init_time_chunk_size=1), load, agg, {'fss': metric_of(sizes, True, thresholds)}


# equal per-point values, non-negative terms and weights: the routes' float64 sums over n points differ by (n + 4) 2^-52 of the sum
SUM_RTOL = TA.SUM_RTOL


def test_chunk_loop_with_records_equals_the_unrecorded_loop(monkeypatch, entry_calls):
  """pipeline.evaluate_chunks over three one-init chunks of device-resident fields, with chunk records and without: the same device
  accumulators bit for bit.  A chunk signature is built at its first meeting, recorded at its second and replayed at its third: the
  replayed chunk runs wbx_fss_threshold_partial out of the record (two calls from Python, three chunks' worth of sums)."""
  times, load, agg, metrics = _chunk_job(3, 3, SHORT)
  monkeypatch.setattr(lazy, 'FUSED_FSS', True)
  monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', True)
  monkeypatch.setattr(engine, 'ALTERNATE_CHUNKS', False)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['recorded'] >= 1 and stats['replayed'] >= 1 and stats['refused'] == 0 and not stats['refusals'], stats
  assert entry_calls == [(3, 3)] * (3 - stats['replayed']), (entry_calls, stats)
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', False)
  engine.clear_caches()
  host = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  assert len(state.sum_weighted_statistics) == 3
  for name in state.sum_weighted_statistics:
    got = np.asarray(state.sum_weighted_statistics[name][V].values)
    assert got.shape == (2, len(SHORT)) and np.isfinite(got).all() and np.abs(got).sum() > 0
    np.testing.assert_array_equal(got, np.asarray(off.sum_weighted_statistics[name][V].values))
    np.testing.assert_array_equal(np.asarray(state.sum_weights[name][V].values), np.asarray(off.sum_weights[name][V].values))
    np.testing.assert_allclose(got, np.asarray(host.sum_weighted_statistics[name][V].values), rtol=SUM_RTOL)


def test_chunk_loop_over_sizes_and_blocks_equals_the_host_route(monkeypatch):
  times, load, agg, metrics = _chunk_job(2, [1, 3, 5], MANY)
  out = {}
  for on in (True, False):
    monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', on)
    engine.clear_caches()
    state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
    out[on] = state.metric_values(metrics)[f'fss.{V}']
  TA._same_labels(out[True], out[False])  # pylint: disable=protected-access
  assert out[True].dims == ('neighborhood_size', 'lead_time', THR)
  # (the score is 1 - a / (b + c) of three such sums; a <= b + c)
  np.testing.assert_allclose(np.asarray(out[True].values), np.asarray(out[False].values), rtol=0, atol=4 * SUM_RTOL, equal_nan=True)
