"""Covered, Confident, JaccardDistant and Opportunism through the public API on the device: statistics + the Aggregator on small
fields (2 x 3 x 6 x 9, a climatology of 8 days x 2 hours x 7 quantile levels gathered in place) under a plain reduction,
GridAreaWeighting with Regions bins, a mask coordinate, and skipna with NaNs; with the fused route on and off; NumPy and
torch-resident payloads; one launch for the three statistics of an Opportunism; per-point values; a recorded and replayed chunk loop.

Bounds.  The indicators of the two routes are IDENTICAL on these inputs -- float64 payloads by construction of the kernel's
arithmetic (tests/test_intervals.py pins the restatement to the host routes), float32 payloads because they are chosen so that
float32 interpolation is exact (eighths around 280, 11 members, levels whose weight g is 0; `_exact32` asserts it on the CPU) -- so
the per-point term of the bound the Wasserstein API tests use is 0 here, and what is left is their term for the float64 summations
of the two routes' stage 1 and stage 2 over n points with non-negative weights W <= Wmax: (n + 4) 2^-52 Wmax sum |value|."""
import functools

import numpy as np
import pytest

import interval_cases as IC
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
DIMS = IC.API_DIMS
REGIONS = {'global': ((-90, 90), (0, 360)), 'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180))}
REDUCE = ['init_time', 'latitude', 'longitude']
CONF_LV, COV_LV, JAC_LV = (0.1, 0.9), (0.1, 0.9), (0.2, 0.7)
CONF_THR, JAC_THR = 0.75, 0.75


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.ens_interval_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


def _opportunism(clim, flags=(True, True, True)):
  return categorical.Opportunism('number', clim, *flags, confidence_quantile_boundaries=CONF_LV, coverage_quantile_boundaries=COV_LV,
                                 jaccard_distance_quantile_boundaries=JAC_LV, confidence_threshold=CONF_THR,
                                 jaccard_distance_threshold=JAC_THR)


def _restated(p, t, c):
  """{statistic: indicator field over DIMS} by the float64 restatement."""
  pick = lambda q: c[IC.LEVELS.index(q)]
  return {'Confident': IC.confident(p, pick(CONF_LV[0]), pick(CONF_LV[1]), CONF_LV, CONF_THR), 'Covered': IC.covered(p, t, COV_LV),
          'JaccardDistant': IC.jaccard_distant(p, pick(JAC_LV[0]), pick(JAC_LV[1]), JAC_LV, JAC_THR)}


@functools.lru_cache(maxsize=None)
def _exact32(m, seed, nans):
  """The float32 inputs are such that float32 interpolation is exact: the host route's float32 indicators are the float64
  restatement's (checked here, on the CPU, with the route switched off)."""
  pred, targ, clim, (p, t, c, _) = IC.api_inputs(np.float32, m, seed=seed, nans=nans)
  assert all(IC.bound(q, m)[1] in (0.0, 0.5) for q in CONF_LV + JAC_LV)
  fused, lazy.FUSED_INTERVALS = lazy.FUSED_INTERVALS, False
  try:
    stats = metrics_base.compute_unique_statistics_for_all_metrics({'o': _opportunism(clim)}, pred, targ)
  finally:
    lazy.FUSED_INTERVALS = fused
  want = _restated(p, t, c)
  for name, per_var in stats.items():
    np.testing.assert_array_equal(np.asarray(per_var['v'].transpose(*DIMS).values), want[name.split('_')[0]], err_msg=name)
  return True


def _evaluate(pred, targ, clim, aggregator, flags=(True, True, True)):
  metrics = {'o': _opportunism(clim, flags)}
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return {k.split('_')[0]: k for k in stats}, stats, state, state.metric_values(metrics)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyInterval) and stat._group.kind == 'ivl'  # pylint: disable=protected-access


def _launches():
  return [e for e in engine.S1_EVENT_LOG if e['kind'] == 'ivl']


def _max_area_weight():
  probe = xr.DataArray(np.zeros(IC.API_SHAPE[2:]), dims=DIMS[2:], coords={'latitude': IC.API_LAT, 'longitude': IC.API_LON})
  return float(np.asarray(weighting.GridAreaWeighting().weights(probe).values).max())


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
PAYLOADS = {'float32-numpy': (np.float32, 11, False), 'float64-numpy': (np.float64, 10, False), 'float32-torch': (np.float32, 11, True),
            'float64-torch': (np.float64, 11, True)}  # (float64 on torch: g = 0 too -- torch.lerp is not NumPy's order of operations)


@pytest.mark.parametrize('payload', list(PAYLOADS))
@pytest.mark.parametrize('case_name', list(CASES))
def test_scores_with_the_route_on_and_off(monkeypatch, case_name, payload):
  case = CASES[case_name]
  dtype, m, device = PAYLOADS[payload]
  if dtype == np.float32:
    assert _exact32(m, 11, case['nans'])
  pred, targ, clim, (p, t, c, _) = IC.api_inputs(dtype, m, nans=case['nans'], mask=case['mask'], device=device)
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  names, stats, state, values = _evaluate(pred, targ, clim, aggregation.Aggregator(reduce_dims=REDUCE, **case['kw']()))
  assert set(names) == {'Confident', 'Covered', 'JaccardDistant'} and all(_is_fused(stats[k]['v']) and stats[k]['v'].is_lazy for k in stats)
  # the fused route was taken: ONE launch of wbx_ens_interval_partial for the three statistics and nothing else
  assert len(_launches()) == 1 and len(engine.S1_EVENT_LOG) == 1, engine.S1_EVENT_LOG
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  engine.clear_caches()
  names0, stats0, state0, values0 = _evaluate(pred, targ, clim, aggregation.Aggregator(reduce_dims=REDUCE, **case['kw']()))
  assert names0 == names and not any(_is_fused(stats0[k]['v']) for k in stats0) and not _launches()
  want = _restated(p, t, c)
  n = int(np.prod([IC.API_SHAPE[DIMS.index(d)] for d in REDUCE]))
  wmax = _max_area_weight() if case['area'] else 1.0
  for which, name in names.items():
    a, b = stats[name]['v'], stats0[name]['v']
    # per point: labelled as the host route's result, the same Booleans, the restatement's
    _same_labels(a, b)
    got, host = np.asarray(a.transpose(*DIMS).values), np.asarray(b.transpose(*DIMS).values)
    assert got.dtype == host.dtype == bool
    np.testing.assert_array_equal(got, host, err_msg=which)
    np.testing.assert_array_equal(got, want[which], err_msg=which)
    # the sums: both routes against each other, labelled alike
    x, y = state.sum_weighted_statistics[name]['v'], state0.sum_weighted_statistics[name]['v']
    _same_labels(x, y)
    tol = wmax * (n + 4) * 2.0 ** -52 * float(want[which].sum())
    print(case_name, payload, which, 'max |fused - host| of the sums:', float(np.abs(np.asarray(x.values) - np.asarray(y.values)).max()), 'bound', tol)
    np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=0, atol=tol)
    assert np.isfinite(np.asarray(x.values)).all()
    np.testing.assert_allclose(np.asarray(state.sum_weights[name]['v'].values), np.asarray(state0.sum_weights[name]['v'].values), rtol=1e-12, atol=0)
  _same_labels(values['o.v'], values0['o.v'])
  np.testing.assert_allclose(np.asarray(values['o.v'].values), np.asarray(values0['o.v'].values), rtol=1e-12, atol=1e-15)
  if case_name in ('plain', 'skipna'):  # a mean over (init, lat, lon) per lead: the product of the restatement's three means
    mean = {k: v.mean(axis=(0, 2, 3)) for k, v in want.items()}
    np.testing.assert_allclose(np.asarray(values['o.v'].transpose('lead_time').values), mean['Confident'] * mean['Covered'] * mean['JaccardDistant'],
                               rtol=1e-12)


@pytest.mark.parametrize('flags', [(True, True, True), (False, None, True), (True, False, None), (True, None, None)])
def test_opportunism_is_one_stage_1_launch(monkeypatch, flags):
  """Whatever the flags: the statistics an Opportunism asks for are one group and one launch, also with levels and thresholds of
  their own, and a second aggregation of the same statistics launches nothing."""
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  pred, targ, clim, (p, t, c, _) = IC.api_inputs(np.float64, 10, mask=True)
  agg = aggregation.Aggregator(reduce_dims=list(DIMS), masked=True)
  names, stats, state, values = _evaluate(pred, targ, clim, agg, flags)
  assert len(_launches()) == 1 and len(engine.S1_EVENT_LOG) == 1, engine.S1_EVENT_LOG
  assert len({id(stats[k]['v']._group) for k in stats}) == 1  # pylint: disable=protected-access
  agg.aggregate_statistics(stats)
  assert len(engine.S1_EVENT_LOG) == 1
  want = _restated(p, t, c)
  valid = np.broadcast_to(np.asarray(pred['v'].coords['mask'].values), IC.API_SHAPE)
  product = 1.0
  for which, flag in zip(('Confident', 'Covered', 'JaccardDistant'), flags):
    if flag is not None:
      frac = want[which][valid].mean()
      product *= frac if flag else 1 - frac
  np.testing.assert_allclose(float(np.asarray(values['o.v'].values)), product, rtol=1e-12)


def test_per_point_values_are_the_host_routes_with_their_type(monkeypatch):
  """.values of the lazy statistics: Boolean, the host route's values; a Boolean tensor on the payload's device for torch payloads."""
  import torch  # pylint: disable=g-import-not-at-top
  for device in (False, True):
    pred, targ, clim, (p, t, c, _) = IC.api_inputs(np.float64, 11, seed=3, nans=True, device=device, member_last=True)
    monkeypatch.setattr(lazy, 'FUSED_INTERVALS', True)
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    stats = metrics_base.compute_unique_statistics_for_all_metrics({'o': _opportunism(clim)}, pred, targ)
    monkeypatch.setattr(lazy, 'FUSED_INTERVALS', False)
    stats0 = metrics_base.compute_unique_statistics_for_all_metrics({'o': _opportunism(clim)}, pred, targ)
    want = _restated(p, t, c)
    for name in stats:
      a, b = stats[name]['v'], stats0[name]['v']
      assert _is_fused(a) and not _is_fused(b)
      _same_labels(a, b)
      da, db = a.data, b.data
      if device:
        assert torch.is_tensor(da) and da.is_cuda and da.dtype == torch.bool and torch.is_tensor(db) and db.dtype == torch.bool
        assert da.device == db.device
      else:
        assert isinstance(da, np.ndarray) and da.dtype == db.dtype == np.dtype(bool)
      assert tuple(a.shape) == tuple(b.shape)
      np.testing.assert_array_equal(np.asarray(a.transpose(*DIMS).values), np.asarray(b.transpose(*DIMS).values), err_msg=name)
      np.testing.assert_array_equal(np.asarray(a.transpose(*DIMS).values), want[name.split('_')[0]], err_msg=name)
    assert len(_launches()) == 3  # every .data is a launch of its own (nothing is cached for a reader of points)
    engine.clear_caches()


FALLBACKS = {
    'switch off': dict(switch=False),
    'M = 65': dict(m=65),
    'integer inputs': dict(dtype=np.int64),
    'targets of another dtype': dict(target_dtype=np.float64),
    'a dim the targets lack': dict(drop_lead=True),
    'a mask along the member dim': dict(member_mask=True),
    'labels that differ': dict(shift_latitude=True),
}


@pytest.mark.parametrize('why', list(FALLBACKS))
def test_every_fallback_condition_gives_the_host_routes_result(monkeypatch, why):
  spec = FALLBACKS[why]
  pred, targ, clim, _ = IC.api_inputs(np.float32, spec.get('m', 11))
  if 'dtype' in spec:
    pred, targ = {'v': pred['v'].astype(spec['dtype'])}, {'v': targ['v'].astype(spec['dtype'])}
  if 'target_dtype' in spec:
    targ = {'v': targ['v'].astype(spec['target_dtype'])}
  if spec.get('drop_lead'):
    targ = {'v': targ['v'].isel(lead_time=0, drop=True)}
  if spec.get('member_mask'):
    pred = {'v': pred['v'].assign_coords(mask=(('latitude', 'number'), np.random.default_rng(1).random((IC.API_SHAPE[2], 11)) > 0.3))}
  if spec.get('shift_latitude'):
    targ = {'v': targ['v'].assign_coords(latitude=IC.API_LAT + 1.0)}
  stat = categorical.Covered('number', COV_LV)

  def run():
    per_var = stat.compute(pred, targ)
    state = aggregation.Aggregator(reduce_dims=['init_time', 'longitude']).aggregate_statistics({stat.unique_name: per_var})
    return per_var['v'], state.sum_weighted_statistics[stat.unique_name]['v']
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', spec.get('switch', True))
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  points, sums = run()
  assert not _is_fused(points) and not _launches(), why
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', False)
  engine.clear_caches()
  points0, sums0 = run()
  _same_labels(points, points0)
  _same_labels(sums, sums0)
  np.testing.assert_array_equal(np.asarray(points.values), np.asarray(points0.values), err_msg=why)
  np.testing.assert_array_equal(np.asarray(sums.values), np.asarray(sums0.values), err_msg=why)


def _chunk_job(n_chunks, m=11):
  import torch  # pylint: disable=g-import-not-at-top
  nlead = IC.API_SHAPE[1]
  p_all, t_all = [], []
  for i in range(n_chunks):
    p, t, _ = IC.values(40 + i, m, (1,) + IC.API_SHAPE[1:], np.float32)
    p_all.append(p)
    t_all.append(t)
  _, _, clim_ds, _ = IC.api_inputs(np.float32, m, device=True)
  clim = np.asarray(xr.as_dataarray(clim_ds['v']).values)  # [day, hour, level, lat, lon]
  inits = np.datetime64('2020-01-01T00', 'ns') + np.arange(n_chunks) * np.timedelta64(24, 'h')
  index = {int(t.astype('int64')): i for i, t in enumerate(inits)}
  dev = [(torch.as_tensor(p_all[i]).cuda(), torch.as_tensor(t_all[i]).cuda()) for i in range(n_chunks)]

  def load(init_chunk, lead_chunk):
    del lead_chunk
    i = index[int(init_chunk[0].astype('int64'))]
    cs = {'init_time': init_chunk, 'lead_time': IC.API_LEAD, 'latitude': IC.API_LAT, 'longitude': IC.API_LON}
    return ({'v': xr.DataArray(dev[i][0], dims=('number',) + DIMS, coords=dict(cs, number=np.arange(m)))},
            {'v': xr.DataArray(dev[i][1], dims=DIMS, coords=cs)})

  agg = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])
  # the restatement over all chunks: the climatology of chunk i's valid times
  want = {k: [] for k in ('Confident', 'Covered', 'JaccardDistant')}
  for i in range(n_chunks):
    valid = inits[i] + IC.API_LEAD
    day = (valid.astype('datetime64[D]') - valid.astype('datetime64[Y]').astype('datetime64[D]')).astype(int) + 1
    hour = (valid - valid.astype('datetime64[D]')).astype('timedelta64[h]').astype(int)
    c = np.moveaxis(clim[np.searchsorted(IC.API_DAYS, day), np.searchsorted(IC.API_HOURS, hour)], 1, 0)[:, None]  # [level, 1, lead, lat, lon]
    for k, v in _restated(p_all[i], t_all[i], c).items():
      want[k].append(v)
  assert nlead == len(IC.API_LEAD)
  return time_chunks.TimeChunks(inits, IC.API_LEAD, init_time_chunk_size=1), load, agg, clim_ds, {k: np.concatenate(v) for k, v in want.items()}


def test_chunk_loop_with_records_equals_the_unrecorded_loop_and_one_evaluation(monkeypatch):
  """pipeline.evaluate_chunks over three one-init chunks of device-resident fields whose climatology rows differ, with chunk records
  (the second and third chunk are replays of the first with their own gather table) and without: the same device accumulators bit
  for bit, and the restatement's weighted sums over all three chunks (integers times weights: within the summation bound)."""
  times, load, agg, clim, want = _chunk_job(3)
  metrics = {'o': _opportunism(clim)}
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  probe = xr.DataArray(np.zeros(IC.API_SHAPE[2:]), dims=DIMS[2:], coords={'latitude': IC.API_LAT, 'longitude': IC.API_LON})
  w = np.asarray(weighting.GridAreaWeighting().weights(probe).values, np.float64).reshape(-1, 1) * np.ones((1, IC.API_SHAPE[3]))
  n = 3 * IC.API_SHAPE[2] * IC.API_SHAPE[3]
  for name in state.sum_weighted_statistics:
    which = name.split('_')[0]
    got = np.asarray(state.sum_weighted_statistics[name]['v'].values)
    np.testing.assert_array_equal(got, np.asarray(off.sum_weighted_statistics[name]['v'].values))
    np.testing.assert_array_equal(np.asarray(state.sum_weights[name]['v'].values), np.asarray(off.sum_weights[name]['v'].values))
    ref = (want[which] * w[None, None]).sum(axis=(0, 2, 3))
    tol = float(w.max()) * (n + 4) * 2.0 ** -52 * want[which].sum(axis=(0, 2, 3))
    assert (np.abs(np.asarray(state.sum_weighted_statistics[name]['v'].transpose('lead_time').values) - ref) <= tol).all(), which
