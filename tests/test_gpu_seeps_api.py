"""SEEPS through the public API on the device: the statistic + the Aggregator on small fields (3 x 2 x 6 x 8, a wet-threshold
climatology of 366 days x 4 hours gathered in place, dry fractions that are 0, 1, NaN and at and just outside the ends of the range at
some places) under masked=True alone, with GridAreaWeighting, with Regions bins on top, and with skipna over NaN inputs; with the
fused route on and off; NumPy and torch-resident payloads; one launch per variable; per-point values; every fallback condition; a
recorded and replayed chunk loop.

Bounds.  The per-point values of the two routes are IDENTICAL (tests/test_seeps.py pins the table and the restatement to the host
route bit for bit), so what is left is the term the interval API tests use for the float64 summations of the two routes' stage 1
and stage 2 over n points with non-negative weights W <= Wmax: (n + 4) 2^-52 Wmax sum |value|."""
import numpy as np
import pytest

import seeps_cases as SC
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

pytestmark = pytest.mark.gpu
V, DIMS = SC.VAR, SC.DIMS
SHAPE = (3, 2, 6, 8)
REGIONS = {'global': ((-90, 90), (0, 360)), 'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180))}
REDUCE = ['init_time', 'latitude', 'longitude']


class _AsMetric(metrics_base.Metric):

  def __init__(self, statistic):
    self._statistic = statistic

  @property
  def statistics(self):
    return {'s': self._statistic}

  def values_from_mean_statistics(self, statistic_values):
    return dict(statistic_values['s'])


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.seeps_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


def _stat(clim):
  return categorical.SEEPS([V], clim, SC.DRY_MM, SC.MIN_P1, SC.MAX_P1)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyStatistic) and stat._group.kind == 'seeps'  # pylint: disable=protected-access


def _launches(kind='seeps'):
  return [e for e in engine.S1_EVENT_LOG if e['kind'] == kind]


def _evaluate(pred, targ, clim, aggregator):
  stat = _stat(clim)
  with np.errstate(all='ignore'):
    per_var = stat.compute(pred, targ)
    state = aggregator.aggregate_statistics({stat.unique_name: per_var})
  name = stat.unique_name
  return per_var[V], state.sum_weighted_statistics[name][V], state.sum_weights[name][V], state.mean_statistics()[name][V]


def _restated(pred, targ, clim, wet, dtype):
  with np.errstate(all='ignore'):
    p1 = xr.as_dataarray(clim[f'{V}_seeps_dry_fraction']).mean(('hour', 'dayofyear'))
  table = categorical.seeps_score_table(p1, SC.MIN_P1, SC.MAX_P1)
  numpy = lambda da: np.asarray(xr.as_dataarray(da).values)
  return SC.point_values(numpy(pred[V]), numpy(targ[V]), wet, table.reshape((9, 1, 1) + table.shape[2:]), SC.DRY_THRESHOLD, dtype)


def _max_area_weight(pred):
  probe = xr.DataArray(np.zeros(SHAPE[2:]), dims=DIMS[2:], coords={d: np.asarray(pred[V].coords[d].values) for d in DIMS[2:]})
  return float(np.asarray(weighting.GridAreaWeighting().weights(probe).values).max())


def _same_labels(a, b):
  assert tuple(a.dims) == tuple(b.dims) and set(a.coords) == set(b.coords) and a.name == b.name, (a.dims, b.dims, set(a.coords), set(b.coords))
  for k in a.coords:
    np.testing.assert_array_equal(np.asarray(a.coords[k].values), np.asarray(b.coords[k].values))


CASES = {
    'masked': dict(kw=lambda: dict(masked=True), nans=False, area=False),
    'area': dict(kw=lambda: dict(masked=True, weigh_by=[weighting.GridAreaWeighting()]), nans=False, area=True),
    'regions': dict(kw=lambda: dict(masked=True, weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)]), nans=False, area=True),
    'skipna': dict(kw=lambda: dict(masked=True, skipna=True), nans=True, area=False),
}
PAYLOADS = {'float32-numpy': (np.float32, False), 'float64-numpy': (np.float64, False), 'float32-torch': (np.float32, True),
            'float64-torch': (np.float64, True)}


@pytest.mark.parametrize('payload', list(PAYLOADS))
@pytest.mark.parametrize('case_name', list(CASES))
def test_scores_with_the_route_on_and_off(monkeypatch, case_name, payload):
  case = CASES[case_name]
  dtype, device = PAYLOADS[payload]
  pred, targ, clim, wet = SC.labelled_case(dtype, 11, shape=SHAPE, mask_on='targets', nans=case['nans'], device=device)
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  a, x, wx, mean = _evaluate(pred, targ, clim, aggregation.Aggregator(reduce_dims=REDUCE, **case['kw']()))
  assert _is_fused(a) and a.is_lazy
  # the fused route was taken: ONE launch of wbx_seeps_partial for the variable and no pass over a materialised statistic
  assert len(_launches()) == 1 and len(engine.S1_EVENT_LOG) == 1, engine.S1_EVENT_LOG
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  engine.clear_caches()
  b, y, wy, mean0 = _evaluate(pred, targ, clim, aggregation.Aggregator(reduce_dims=REDUCE, **case['kw']()))
  assert not _is_fused(b) and not _launches() and engine.S1_EVENT_LOG  # (a pass over the materialised statistic)
  # per point: labelled as the host route's result, the same numbers, the restatement's; the same mask coordinate
  _same_labels(a, b)
  with np.errstate(all='ignore'):
    got, host = np.asarray(a.transpose(*DIMS).values), np.asarray(b.transpose(*DIMS).values)
  want = _restated(pred, targ, clim, wet, dtype)
  assert got.dtype == host.dtype == np.float64 and SC.same_numbers(got, host) and SC.same_numbers(got, want)
  mask = np.asarray(a.coords['mask'].values)
  assert mask.dtype == bool and mask.shape == SHAPE and 0.3 < mask.mean() < 0.9
  # the sums: both routes against each other, labelled alike
  _same_labels(x, y)
  counted = mask & ~np.isnan(want) if case['nans'] else mask
  assert np.isfinite(want[counted]).all()
  n = int(np.prod([SHAPE[DIMS.index(d)] for d in REDUCE]))
  wmax = _max_area_weight(pred) if case['area'] else 1.0
  tol = wmax * (n + 4) * 2.0 ** -52 * float(np.abs(want[counted]).sum())
  diff = float(np.abs(np.asarray(x.values) - np.asarray(y.values)).max())
  print(case_name, payload, 'max |fused - host| of the sums:', diff, 'bound', tol)
  assert np.isfinite(np.asarray(x.values)).all() and np.abs(np.asarray(x.values)).sum() > 0
  np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=0, atol=tol)
  np.testing.assert_allclose(np.asarray(wx.values), np.asarray(wy.values), rtol=1e-12, atol=0)
  _same_labels(mean, mean0)
  np.testing.assert_allclose(np.asarray(mean.values), np.asarray(mean0.values), rtol=1e-12, atol=1e-15)
  if case_name in ('masked', 'skipna'):  # the masked mean over (init, lat, lon) per lead, from the restatement
    ref = np.where(counted, want, 0).sum(axis=(0, 2, 3)) / counted.sum(axis=(0, 2, 3))
    np.testing.assert_allclose(np.asarray(mean.transpose('lead_time').values), ref, rtol=1e-12)


def test_one_launch_per_variable_and_none_for_a_second_aggregation(monkeypatch):
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  pred, targ, clim, _ = SC.labelled_case(np.float32, 3, shape=SHAPE, mask_on='predictions', nans=False)
  other = 'tp24'
  pred2, targ2, clim2, _ = SC.labelled_case(np.float32, 4, shape=SHAPE, mask_on='targets', nans=False)
  pred[other], targ[other] = pred2[V], targ2[V]
  clim = dict(clim, **{k.replace(V, other, 1): v for k, v in clim2.items()})
  stat = categorical.SEEPS([V, other], clim, SC.DRY_MM, SC.MIN_P1, SC.MAX_P1)
  per_var = stat.compute(pred, targ)
  assert all(_is_fused(per_var[v]) for v in (V, other))
  agg = aggregation.Aggregator(reduce_dims=list(DIMS), masked=True)
  state = agg.aggregate_statistics({stat.unique_name: per_var})
  assert len(_launches()) == 2 and len(engine.S1_EVENT_LOG) == 2, engine.S1_EVENT_LOG
  agg.aggregate_statistics({stat.unique_name: per_var})
  assert len(engine.S1_EVENT_LOG) == 2
  mean = state.mean_statistics()[stat.unique_name]
  assert np.isfinite(float(np.asarray(mean[V].values))) and np.isfinite(float(np.asarray(mean[other].values)))


def test_per_point_values_are_the_host_routes_with_their_type(monkeypatch):
  import torch  # pylint: disable=g-import-not-at-top
  for device in (False, True):
    pred, targ, clim, _ = SC.labelled_case(np.float32, 5, shape=SHAPE, mask_on='targets', device=device)
    monkeypatch.setattr(lazy, 'FUSED_SEEPS', True)
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    with np.errstate(all='ignore'):
      a = _stat(clim).compute(pred, targ)[V]
      monkeypatch.setattr(lazy, 'FUSED_SEEPS', False)
      b = _stat(clim).compute(pred, targ)[V]
      assert _is_fused(a) and not _is_fused(b)
      _same_labels(a, b)
      da, db = a.data, b.data
    assert type(da) is type(db) and tuple(a.shape) == tuple(b.shape)
    if device:
      assert torch.is_tensor(da) and da.dtype == db.dtype == torch.float64 and da.device == db.device
    assert SC.same_numbers(np.asarray(a.transpose(*DIMS).values), np.asarray(b.transpose(*DIMS).values))
    assert not _launches()  # a reader of points gets the host route's array
    engine.clear_caches()


@pytest.mark.parametrize('why', ['switch off'] + list(SC.decline_cases()))
def test_every_fallback_condition_gives_the_host_routes_result(monkeypatch, why):
  if why == 'switch off':
    pred, targ, clim, _ = SC.labelled_case(np.float32, 21, mask_on='targets')
  else:
    pred, targ, clim = SC.decline_cases()[why]
  stat = _stat(clim)

  def run():
    with np.errstate(all='ignore'):
      per_var = stat.compute(pred, targ)
      state = aggregation.Aggregator(reduce_dims=['init_time', 'longitude'], masked=True, skipna=True).aggregate_statistics({stat.unique_name: per_var})
    return per_var[V], state.sum_weighted_statistics[stat.unique_name][V]
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', why != 'switch off')
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  try:
    points, sums = run()
  except (KeyError, ValueError) as e:  # the host route itself refuses these inputs: with the switch off as well
    monkeypatch.setattr(lazy, 'FUSED_SEEPS', False)
    with pytest.raises(type(e)):
      run()
    return
  assert not _is_fused(points) and not _launches(), why
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', False)
  engine.clear_caches()
  points0, sums0 = run()
  _same_labels(points, points0)
  _same_labels(sums, sums0)
  assert SC.same_numbers(np.asarray(points.values), np.asarray(points0.values)), why
  np.testing.assert_array_equal(np.asarray(sums.values), np.asarray(sums0.values), err_msg=why)


def _chunk_job(n_chunks):
  import torch  # pylint: disable=g-import-not-at-top
  chunks = [SC.labelled_case(np.float32, 40, shape=(1,) + SHAPE[1:], first_day=f'2020-03-0{1 + i}T00', nans=False) for i in range(n_chunks)]
  fields = [SC.labelled_case(np.float32, 50 + i, shape=(1,) + SHAPE[1:], first_day=f'2020-03-0{1 + i}T00', nans=False) for i in range(n_chunks)]
  clim = chunks[0][2]  # one climatology for the whole job (seed 40); chunk i's fields are their own (seed 50 + i)
  clim = {k: xr.DataArray(torch.as_tensor(np.asarray(v.values)).cuda(), dims=v.dims, coords=dict(v.coords)) for k, v in clim.items()}
  inits = np.concatenate([np.asarray(c[0][V].coords['init_time'].values) for c in chunks])
  lead = np.asarray(chunks[0][0][V].coords['lead_time'].values)
  index = {int(t.astype('int64')): i for i, t in enumerate(inits)}
  dev = [(torch.as_tensor(np.asarray(f[0][V].values)).cuda(), torch.as_tensor(np.asarray(f[1][V].values)).cuda()) for f in fields]

  def load(init_chunk, lead_chunk):
    del lead_chunk
    i = index[int(init_chunk[0].astype('int64'))]
    cs = {d: np.asarray(chunks[i][0][V].coords[d].values) for d in DIMS}
    return ({V: xr.DataArray(dev[i][0], dims=DIMS, coords=cs)}, {V: xr.DataArray(dev[i][1], dims=DIMS, coords=cs)})

  agg = aggregation.Aggregator(reduce_dims=REDUCE, weigh_by=[weighting.GridAreaWeighting()], masked=True)
  return time_chunks.TimeChunks(inits, lead, init_time_chunk_size=1), load, agg, clim


@pytest.mark.parametrize('n_chunks,alternate', [(3, False), (7, True)], ids=['three_chunks_one_stream', 'seven_chunks_alternating'])
def test_chunk_loop_with_records_equals_the_unrecorded_loop(monkeypatch, n_chunks, alternate):
  """pipeline.evaluate_chunks over one-init chunks of device-resident fields whose valid times (the climatology's rows) differ, with
  chunk records and without: the same device accumulators bit for bit.  A chunk signature is built at its first meeting, recorded at
  its second and replayed from its third on: three chunks on one launch stream are build / record / replay; with consecutive chunks
  on alternating streams (the default, the stream is part of the signature) seven chunks replay the fifth, sixth and seventh.  A
  replayed chunk runs wbx_seeps_partial out of the record -- the dry threshold as the bits of a double, the shared range mask and
  the score table as memory the record keeps -- on a plan variant with ITS gather table."""
  times, load, agg, clim = _chunk_job(n_chunks)
  metrics = {'seeps': _AsMetric(_stat(clim))}
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', True)
  monkeypatch.setattr(engine, 'ALTERNATE_CHUNKS', alternate)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  with np.errstate(all='ignore'):
    state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['recorded'] >= 1 and stats['replayed'] >= (1 if n_chunks == 3 else 3) and stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  with np.errstate(all='ignore'):
    off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  for name in state.sum_weighted_statistics:
    got = np.asarray(state.sum_weighted_statistics[name][V].values)
    assert np.isfinite(got).all() and np.abs(got).sum() > 0
    np.testing.assert_array_equal(got, np.asarray(off.sum_weighted_statistics[name][V].values))
    np.testing.assert_array_equal(np.asarray(state.sum_weights[name][V].values), np.asarray(off.sum_weights[name][V].values))
  # ... and the host route's loop, within the summation bound
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', False)
  engine.clear_caches()
  with np.errstate(all='ignore'):
    host = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  for name in state.sum_weighted_statistics:
    x, y = np.asarray(state.sum_weighted_statistics[name][V].values), np.asarray(host.sum_weighted_statistics[name][V].values)
    n = n_chunks * SHAPE[2] * SHAPE[3]  # scores and weights are not negative: (n + 4) 2^-52 sum w |v| is that share of the sum itself
    np.testing.assert_allclose(x, y, rtol=(n + 4) * 2.0 ** -52, atol=0)
