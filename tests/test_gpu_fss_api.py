"""FSS and its three statistics through the public API on the device: 0 / 1 fields of 3 x 12 x 16 (the fields of
tests/test_spatial.py::test_fss_of_fields_through_the_aggregator) with the fused route on and off, against each other and against the
oracle; with and without GridAreaWeighting, masked=True with a NaN-masked target, combine_mask, skipna, Regions bins (x kept,
wbx_contract_bits), a scalar size and a list, NumPy and torch-on-device payloads; the launches that were made; a chunk loop that records
and replays.

Bound between the routes.  The kernel's fraction is the float32 rounding of S / n^2 with S exact; the host route's is the float32
rounding of a float64 mean of means: both are within half an ulp of float32 of the exact quotient, so they differ by at most one ulp,
2 v |F| with v = 2^-24 (tests/test_fss.py counts the points of these shapes at which they differ at all: none).  fss_cases.
mean_bound_from_ulps carries one ulp per fraction through the three float32 squares; a sum of n such terms under weights W <= Wmax
then moves by at most Wmax (sum of the per-point bounds + (n + 4) 2^-52 sum |value|), the second term for the float64 summations of
the two routes' stage 1 and stage 2."""
import numpy as np
import pytest

import fss_cases as FC
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

pytestmark = pytest.mark.gpu
V = 'rain'
DIMS = ('time', 'latitude', 'longitude')
SHAPE = (3, 12, 16)
COORDS = {'time': np.arange(3), 'latitude': np.linspace(-55, 55, 12), 'longitude': np.arange(16) * 22.5}
REGIONS = {'global': ((-90, 90), (0, 360)), 'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180)),
           'south': ((-90, -20), (0, 360)), 'west': ((-90, 90), (180, 360))}
TERMS = ('SquaredFractionsError', 'SquaredPredictionFraction', 'SquaredTargetFraction')


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.fss_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


def fields(dtype=np.float32, seed=43):
  rng = np.random.default_rng(seed)
  base = rng.random(SHAPE)
  return (base + 0.25 * rng.normal(size=SHAPE) > 0.7).astype(dtype), (base > 0.7).astype(dtype)


def labelled(a, device, mask=None):
  coords = dict(COORDS)
  if mask is not None:
    coords['mask'] = (DIMS, mask)
  if device:
    import torch  # pylint: disable=g-import-not-at-top
    a = torch.as_tensor(a).cuda()
  return {V: xr.DataArray(a, dims=DIMS, coords=coords)}


def _launches(kind='fss'):
  return [e for e in engine.S1_EVENT_LOG if e['kind'] == kind]


def _is_fused(stat):
  return isinstance(stat, lazy.LazyFSS)


def evaluate(pred, targ, sizes, wrap, agg_kw, combine_mask=False):
  metrics = {'fss': spatial.FSS(sizes, wrap_longitude=wrap, combine_mask=combine_mask)}
  with np.errstate(all='ignore'):
    stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
    state = aggregation.Aggregator(**agg_kw).aggregate_statistics(stats)
    score = state.metric_values(metrics)[f'fss.{V}']
  names = {t: next(k for k in stats if k.startswith(t + '_')) for t in TERMS}
  return ({t: stats[names[t]][V] for t in TERMS}, {t: state.sum_weighted_statistics[names[t]][V] for t in TERMS},
          {t: state.sum_weights[names[t]][V] for t in TERMS}, score)


def _same_labels(a, b):
  assert tuple(a.dims) == tuple(b.dims) and set(a.coords) == set(b.coords), (a.dims, b.dims, set(a.coords), set(b.coords))
  for k in a.coords:
    np.testing.assert_array_equal(np.asarray(a.coords[k].values), np.asarray(b.coords[k].values))


def _nan_target(t):
  valid = np.ones(t.shape, dtype=bool)
  valid[1, 4:7, 5:9] = False
  return np.where(valid, t, np.nan).astype(t.dtype), valid


CASES = {
    'plain_list': dict(sizes=[1, 3, 5], wrap=True, kw=lambda: dict(reduce_dims=list(DIMS))),
    'plain_scalar_no_wrap': dict(sizes=5, wrap=False, kw=lambda: dict(reduce_dims=list(DIMS))),
    'area': dict(sizes=[1, 3, 5, 11], wrap=True, kw=lambda: dict(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()])),
    'keep_time': dict(sizes=[3, 5], wrap=False, kw=lambda: dict(reduce_dims=['latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])),
    'masked_nan_target': dict(sizes=3, wrap=True, nan_target=True, kw=lambda: dict(reduce_dims=list(DIMS), masked=True)),
    'masked_list_area': dict(sizes=[1, 3], wrap=True, nan_target=True,
                             kw=lambda: dict(reduce_dims=list(DIMS), masked=True, weigh_by=[weighting.GridAreaWeighting()])),
    'combine_mask': dict(sizes=[3, 5], wrap=False, nan_target=True, p_mask=True, combine_mask=True,
                         kw=lambda: dict(reduce_dims=list(DIMS), masked=True)),
    'skipna': dict(sizes=[1, 3], wrap=True, nan_target=True, no_mask=True, kw=lambda: dict(reduce_dims=list(DIMS), skipna=True)),
    'regions': dict(sizes=[3, 5], wrap=True, kw=lambda: dict(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()],
                                                            bin_by=[binning.Regions(REGIONS)])),
    'regions_masked': dict(sizes=3, wrap=True, nan_target=True,
                           kw=lambda: dict(reduce_dims=list(DIMS), masked=True, weigh_by=[weighting.GridAreaWeighting()],
                                           bin_by=[binning.Regions(REGIONS)])),
}
PAYLOADS = {'float32-numpy': (np.float32, False), 'float64-numpy': (np.float64, False), 'float32-torch': (np.float32, True)}


def _inputs(case, dtype, device):
  p, t = fields(dtype)
  t_mask = p_mask = None
  if case.get('nan_target'):
    t, valid = _nan_target(t)
    t_mask = None if case.get('no_mask') else valid
  if case.get('p_mask'):
    p_mask = np.ones(p.shape, bool)
    p_mask[0, 2:4, 1:3] = False
  return p, t, labelled(p, device, p_mask), labelled(t, device, t_mask)


@pytest.mark.parametrize('payload', list(PAYLOADS))
@pytest.mark.parametrize('case_name', list(CASES))
def test_scores_with_the_route_on_and_off(monkeypatch, case_name, payload):
  case = CASES[case_name]
  dtype, device = PAYLOADS[payload]
  p, t, pred, targ = _inputs(case, dtype, device)
  sizes, wrap = case['sizes'], case['wrap']
  size_list = sizes if isinstance(sizes, list) else [sizes]
  monkeypatch.setattr(lazy, 'FUSED_FSS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  a, x, wx, score = evaluate(pred, targ, sizes, wrap, case['kw'](), case.get('combine_mask', False))
  assert all(_is_fused(a[k]) and a[k].is_lazy for k in TERMS)
  # the fused route was taken: ONE launch of wbx_fss_partial per size for the three statistics, no pass over a materialised statistic
  assert len(_launches()) == len(size_list) and len(engine.S1_EVENT_LOG) == len(size_list), engine.S1_EVENT_LOG
  monkeypatch.setattr(lazy, 'FUSED_FSS', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  engine.clear_caches()
  b, y, wy, score0 = evaluate(pred, targ, sizes, wrap, case['kw'](), case.get('combine_mask', False))
  assert not any(_is_fused(b[k]) for k in TERMS) and not _launches() and engine.S1_EVENT_LOG  # (passes over materialised statistics)
  n = int(np.prod(SHAPE))
  kw = case['kw']()
  wmax = 1.0
  if kw.get('weigh_by'):
    probe = xr.DataArray(np.zeros(SHAPE[1:]), dims=DIMS[1:], coords={d: COORDS[d] for d in DIMS[1:]})
    wmax = float(np.asarray(weighting.GridAreaWeighting().weights(probe).values).max())
  bounds = [FC.mean_bound_from_ulps(FC.fractions(p, k, wrap), FC.fractions(t, k, wrap)) for k in size_list]
  values = [FC.point_values(p, t, k, wrap) for k in size_list]
  for l, term in enumerate(TERMS):
    _same_labels(a[term], b[term])  # per point: labelled as the host route's result, its `mask` coordinate among the coordinates
    _same_labels(x[term], y[term])
    tol = wmax * max(float(np.nansum(bk[l])) + (n + 4) * 2.0 ** -52 * float(np.nansum(np.abs(vk[l]))) for bk, vk in zip(bounds, values))
    gx, gy = np.asarray(x[term].values), np.asarray(y[term].values)
    print(case_name, payload, term, 'max |fused - host| of the sums:', float(np.nanmax(np.abs(gx - gy))), 'bound', tol)
    np.testing.assert_array_equal(np.isnan(gx), np.isnan(gy))
    assert np.isfinite(gx).any() and np.nansum(np.abs(gx)) > 0
    np.testing.assert_allclose(gx, gy, rtol=0, atol=tol)
    np.testing.assert_allclose(np.asarray(wx[term].values), np.asarray(wy[term].values), rtol=1e-12, atol=0)
  _same_labels(score, score0)
  np.testing.assert_allclose(np.asarray(score.values), np.asarray(score0.values), rtol=2e-6, equal_nan=True)
  if case_name in ('plain_list', 'plain_scalar_no_wrap'):  # both routes against the oracle
    for route in (score, score0):
      got = np.asarray(route.values).reshape(-1)
      want = [O.fractions_skill_score(p, t, k, wrap) for k in size_list]
      np.testing.assert_allclose(got, want, rtol=2e-6)
  if case_name == 'masked_nan_target':  # the masked mean over the pixels whose whole neighbourhood is valid (tests/test_spatial.py)
    valid = _nan_target(fields(dtype)[1])[1]
    pf = np.stack([O.neighborhood_mean(f, 3, True) for f in p])
    tf = np.stack([O.neighborhood_mean(f, 3, True) for f in t])
    ok = np.isclose(np.stack([O.neighborhood_mean(f, 3, True) for f in valid.astype(float)]), 1.0)
    mean = lambda v: np.where(ok, v, 0).sum() / ok.sum()
    want = 1 - mean((pf - tf) ** 2) / (mean(pf ** 2) + mean(tf ** 2))
    for route in (score, score0):
      np.testing.assert_allclose(float(np.asarray(route.values)), want, rtol=2e-6)


@pytest.mark.parametrize('term', TERMS)
def test_a_statistic_alone_through_the_aggregator(monkeypatch, term):
  p, t = fields()
  cls = getattr(spatial, term)
  out = {}
  for on in (True, False):
    monkeypatch.setattr(lazy, 'FUSED_FSS', on)
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    engine.clear_caches()
    stat = cls([3, 5], wrap_longitude=True)
    per_var = stat.compute(labelled(p, False), labelled(t, False))
    assert _is_fused(per_var[V]) == on
    state = aggregation.Aggregator(reduce_dims=['latitude', 'longitude']).aggregate_statistics({stat.unique_name: per_var})
    assert len(_launches()) == (2 if on else 0)
    out[on] = state.mean_statistics()[stat.unique_name][V]
  _same_labels(out[True], out[False])
  assert out[True].dims == ('neighborhood_size', 'time')
  l = TERMS.index(term)
  for i, k in enumerate((3, 5)):
    want = FC.point_values(p, t, k, True)[l].mean(axis=(1, 2))
    np.testing.assert_allclose(np.asarray(out[True].values)[i], want, rtol=1e-12)
    np.testing.assert_allclose(np.asarray(out[False].values)[i], want, rtol=1e-6)


def test_one_launch_per_size_and_none_for_a_second_aggregation(monkeypatch):
  """The test that fails without the feature: the fused route launches wbx_fss_partial, once per size for all three statistics."""
  monkeypatch.setattr(lazy, 'FUSED_FSS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  p, t = fields()
  metrics = {'fss': spatial.FSS([1, 3, 5], wrap_longitude=True)}
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, labelled(p, False), labelled(t, False))
  assert len(stats) == 3 and all(_is_fused(s[V]) for s in stats.values())
  groups = {id(s[V]._group) for s in stats.values()}  # pylint: disable=protected-access
  assert len(groups) == 1
  agg = aggregation.Aggregator(reduce_dims=list(DIMS))
  agg.aggregate_statistics(stats)
  assert [e['kind'] for e in engine.S1_EVENT_LOG] == ['fss'] * 3, engine.S1_EVENT_LOG
  agg.aggregate_statistics(stats)
  assert len(engine.S1_EVENT_LOG) == 3


def test_per_point_values_are_the_host_routes_with_their_type(monkeypatch):
  import torch  # pylint: disable=g-import-not-at-top
  p, t = fields()
  for device in (False, True):
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    res = {}
    for on in (True, False):
      monkeypatch.setattr(lazy, 'FUSED_FSS', on)
      res[on] = spatial.SquaredFractionsError([1, 3]).compute(labelled(p, device), labelled(t, device))[V]
    a, b = res[True], res[False]
    assert _is_fused(a) and not _is_fused(b)
    _same_labels(a, b)
    assert a.dims == b.dims == ('neighborhood_size',) + DIMS and tuple(a.shape) == tuple(b.shape)
    da, db = a.data, b.data
    assert type(da) is type(db)
    if device:
      assert torch.is_tensor(da) and da.dtype == db.dtype and da.device == db.device
    assert FC.same_numbers(np.asarray(a.values, np.float64), np.asarray(b.values, np.float64))
    assert not _launches()  # a reader of points gets the host route's array
    engine.clear_caches()


def test_latitude_kept_under_weights_on_a_reduced_dim_takes_the_host_route(monkeypatch):
  """The one reduction the plan cannot serve: latitude kept while the weights depend on a reduced dim.  GridAreaWeighting needs
  latitude itself, so the weights here come from a weighting of this package's module over `time`."""

  class TimeWeights(weighting.Weighting):
    def weights(self, statistic):
      return xr.DataArray(np.arange(1.0, 4.0), dims=('time',))
  TimeWeights.__module__ = weighting.__name__
  p, t = fields()
  out = {}
  for on in (True, False):
    monkeypatch.setattr(lazy, 'FUSED_FSS', on)
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    engine.clear_caches()
    stat = spatial.SquaredFractionsError(3)
    per_var = stat.compute(labelled(p, False), labelled(t, False))
    state = aggregation.Aggregator(reduce_dims=['time', 'longitude'], weigh_by=[TimeWeights()]).aggregate_statistics({stat.unique_name: per_var})
    assert not _launches()
    out[on] = np.asarray(state.sum_weighted_statistics[stat.unique_name][V].values)
  np.testing.assert_array_equal(out[True], out[False])


def _chunk_job(n_chunks, sizes):
  import torch  # pylint: disable=g-import-not-at-top
  cdims = ('init_time', 'lead_time', 'latitude', 'longitude')
  inits = np.array([f'2020-03-0{1 + i}T00' for i in range(n_chunks)], dtype='datetime64[ns]')
  lead = np.array([0, 6], dtype='timedelta64[h]').astype('timedelta64[ns]')
  index = {int(t.astype('int64')): i for i, t in enumerate(inits)}
  dev = []
  for i in range(n_chunks):
    p, t = FC.indicator_fields((1, 2) + SHAPE[1:], np.float32, 60 + i)
    dev.append((torch.as_tensor(p).cuda(), torch.as_tensor(t).cuda()))

  def load(init_chunk, lead_chunk):
    del lead_chunk
    i = index[int(init_chunk[0].astype('int64'))]
    cs = {'init_time': inits[i:i + 1], 'lead_time': lead, 'latitude': COORDS['latitude'], 'longitude': COORDS['longitude']}
    return ({V: xr.DataArray(dev[i][0], dims=cdims, coords=cs)}, {V: xr.DataArray(dev[i][1], dims=cdims, coords=cs)})

  agg = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])
  for n in ([sizes] if not isinstance(sizes, list) else sizes):  # the two routes' fractions of these fields are the SAME numbers
    for f in dev:
      for x in f:
        host = spatial.convolve2d_wrap_longitude(x.cpu().numpy().copy(), n, True)
        assert FC.same_numbers(np.asarray(host, np.float64), np.asarray(FC.fractions(x.cpu().numpy(), n, True), np.float64))
  return time_chunks.TimeChunks(inits, lead, init_time_chunk_size=1), load, agg, {'fss': spatial.FSS(sizes, wrap_longitude=True)}


# equal per-point values, non-negative terms and weights: the routes' float64 sums over n points differ by (n + 4) 2^-52 of the sum
SUM_RTOL = (3 * 2 * SHAPE[1] * SHAPE[2] + 4) * 2.0 ** -52


def test_chunk_loop_with_records_equals_the_unrecorded_loop(monkeypatch):
  """pipeline.evaluate_chunks over three one-init chunks of device-resident fields, with chunk records and without: the same device
  accumulators bit for bit.  A chunk signature is built at its first meeting, recorded at its second and replayed at its third: the
  replayed chunk runs wbx_fss_partial out of the record."""
  times, load, agg, metrics = _chunk_job(3, 3)
  monkeypatch.setattr(lazy, 'FUSED_FSS', True)
  monkeypatch.setattr(engine, 'ALTERNATE_CHUNKS', False)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['recorded'] >= 1 and stats['replayed'] >= 1 and stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  monkeypatch.setattr(lazy, 'FUSED_FSS', False)
  engine.clear_caches()
  host = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  assert len(state.sum_weighted_statistics) == 3
  for name in state.sum_weighted_statistics:
    got = np.asarray(state.sum_weighted_statistics[name][V].values)
    assert np.isfinite(got).all() and np.abs(got).sum() > 0
    np.testing.assert_array_equal(got, np.asarray(off.sum_weighted_statistics[name][V].values))
    np.testing.assert_array_equal(np.asarray(state.sum_weights[name][V].values), np.asarray(off.sum_weights[name][V].values))
    np.testing.assert_allclose(got, np.asarray(host.sum_weighted_statistics[name][V].values), rtol=SUM_RTOL)


def test_chunk_loop_over_a_list_of_sizes_equals_the_host_route(monkeypatch):
  times, load, agg, metrics = _chunk_job(3, [1, 3, 5])
  out = {}
  for on in (True, False):
    monkeypatch.setattr(lazy, 'FUSED_FSS', on)
    engine.clear_caches()
    state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
    out[on] = state.metric_values(metrics)[f'fss.{V}']
  _same_labels(out[True], out[False])
  # (the score is 1 - a / (b + c) of three such sums; a <= b + c)
  np.testing.assert_allclose(np.asarray(out[True].values), np.asarray(out[False].values), rtol=0, atol=4 * SUM_RTOL)
