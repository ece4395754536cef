"""VariogramScore / TiledVariogramScore through the public API on the device: statistics + the Aggregator on small fields
(5 members, 2 x 3 x 6 x 9) under a plain reduction, GridAreaWeighting with Regions bins, a target mask, and skipna with NaNs; NumPy
and torch-resident payloads; every fallback condition; two powers in one evaluation; a recorded and replayed chunk loop; the tiled
inputs shared with TiledEnergyScore.

Bounds (tests/variogram_cases.py derives the fused route's per point, b_f).  The host route on float64 copies of the payload forms
the same terms in float64 and adds the members in float64 too: it is within the same formula with u = 2^-53, b_64, doubled for
its pairwise table sums in another order.  A weighted sum over N points with non-negative weights W <= Wmax inherits
Wmax * sum (b_f + 2 b_64) plus (N + 4) 2^-52 Wmax sum |value| for the float64 summations (stage 1, stage 2, the host's own); a
plain mean is that over N."""
import functools

import numpy as np
import pytest

import variogram_cases as VC
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
from weatherbenchx_amd.metrics import wrappers

pytestmark = pytest.mark.gpu
DIMS = ('time', 'level', 'latitude', 'longitude')
SHAPE = (2, 3, 6, 9)
M = 5
LAT = np.linspace(-75, 75, SHAPE[2])
LON = np.arange(SHAPE[3]) * (360.0 / SHAPE[3])
LEVEL = np.array([500.0, 700.0, 850.0])
REGIONS = {'global': ((-90, 90), (0, 360)), 'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180))}
REDUCE = ['time', 'latitude', 'longitude']


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.ens_variogram_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


@functools.lru_cache(maxsize=None)
def _arrays(dtype, nans, seed, m, shape):
  rng = np.random.default_rng(seed)
  p = (rng.integers(-64, 65, size=(m,) + shape) / 8.0).astype(dtype)
  t = (rng.integers(-64, 65, size=shape) / 8.0).astype(dtype)
  if nans:
    p[rng.random(p.shape) < 0.004] = np.nan
    t[rng.random(t.shape) < 0.03] = np.nan
  valid = rng.random(shape[2:]) > 0.3
  for a in (p, t, valid):
    a.setflags(write=False)
  return p, t, valid


def _inputs(dtype=np.float32, nans=False, mask=False, seed=11, m=M, shape=SHAPE, device=False):
  p, t, valid = _arrays(np.dtype(dtype).type, nans, seed, m, shape)
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
          {'v': xr.DataArray(load(t), dims=DIMS, coords=tc, name='v')})


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyStatistic) and stat._group.kind == 'vgrm'  # pylint: disable=protected-access


def _launches():
  return [e for e in engine.S1_EVENT_LOG if e['kind'] == 'vgrm']


def _max_area_weight():
  probe = xr.DataArray(np.zeros(SHAPE[2:]), dims=DIMS[2:], coords={'latitude': LAT, 'longitude': LON})
  return float(np.asarray(weighting.GridAreaWeighting().weights(probe).values).max())


class _Level(metrics_base.PerVariableMetric):
  """VariogramScore along `level` as a metric (the package's own metric of this statistic is the tiled one)."""

  def __init__(self, p=0.5):
    self._p = p

  @property
  def statistics(self):
    return {'VariogramScore': probabilistic.VariogramScore(dim='level', ensemble_dim='number', p=self._p)}

  def _values_from_mean_statistics_per_variable(self, statistic_values):
    return statistic_values['VariogramScore']


METRICS = {
    'level': lambda p: _Level(p),
    'tiled': lambda p: probabilistic.TiledVariogramScore(window_size=3, ensemble_dim='number', p=p, wrap_longitude=True),
    'tiled-nowrap': lambda p: probabilistic.TiledVariogramScore(window_size=3, ensemble_dim='number', p=p, wrap_longitude=False),
}
CASES = {
    'plain': dict(kw=lambda: {}, nans=False, mask=False, area=False, power=0.5),
    'regions': dict(kw=lambda: dict(weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)]), nans=False, mask=False, area=True,
                    power=1.0),
    'masked': dict(kw=lambda: dict(masked=True, weigh_by=[weighting.GridAreaWeighting()]), nans=False, mask=True, area=True, power=2.0),
    'skipna': dict(kw=lambda: dict(skipna=True), nans=True, mask=False, area=False, power=0.5),
}


def _points(which, pred, targ, power, dtype):
  """Per-point score of the restatement on the float64-widened inputs over the metric's frame, [time, ...], with the bounds of a
  launch in `dtype` and of one in float64."""
  p, t = np.asarray(pred['v'].values), np.asarray(targ['v'].values)
  if which == 'level':
    pw, tw = np.moveaxis(p, 2, -1), np.moveaxis(t, 1, -1)                 # [number, time, lat, lon, level], [time, lat, lon, level]
  else:
    tile = lambda a, ilat: np.stack([np.roll(np.roll(a, i - 1, ilat), j - 1, ilat + 1) for i in range(3) for j in range(3)], axis=-1)
    pw, tw = tile(p, 3)[:, :, :, 1:-1], tile(t, 2)[:, :, 1:-1]            # [number, time, level, lat, lon, window]
    if which == 'tiled-nowrap':
      pw, tw = pw[:, :, :, :, 1:-1], tw[:, :, :, 1:-1]
  stat, bound = VC.variogram_points(pw, tw, power, dtype)
  return stat, bound, VC.variogram_points(pw, tw, power, np.float64)[1]


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('case_name', list(CASES))
@pytest.mark.parametrize('which', list(METRICS))
def test_scores_against_the_host_route_and_the_restatement(monkeypatch, which, case_name, dtype):
  case = CASES[case_name]
  power = case['power']
  pred, targ = _inputs(dtype, nans=case['nans'], mask=case['mask'])
  metrics = {'vs': METRICS[which](power)}
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(metrics, pred, targ, aggregation.Aggregator(reduce_dims=REDUCE, **case['kw']()))
  assert len(stats) == 1 and all(_is_fused(s) and s.is_lazy for per_var in stats.values() for s in per_var.values())
  # one statistic per variable, which carries the targets' mask: one launch, with or without a mask (the energy score has a second,
  # unmasked one for its spread, a statistic of the predictions alone)
  assert len(_launches()) == 1 and len(engine.S1_EVENT_LOG) == 1, engine.S1_EVENT_LOG
  # the host route, on float64 copies of the payload
  pred64 = {'v': pred['v'].astype(np.float64)}
  targ64 = {'v': targ['v'].astype(np.float64)}
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats64, state64, values64 = _evaluate(metrics, pred64, targ64, aggregation.Aggregator(reduce_dims=REDUCE, **case['kw']()))
  assert not any(_is_fused(s) for per_var in stats64.values() for s in per_var.values()) and not _launches()
  # what anybody reads per point is the host route's on the same payload, bit for bit
  stats0 = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  assert set(stats) == set(stats0) == set(stats64)
  (name,) = stats
  a, b = stats[name]['v'], stats0[name]['v']
  assert tuple(a.dims) == tuple(b.dims) and set(a.coords) == set(b.coords), (a.dims, b.dims)
  np.testing.assert_array_equal(np.asarray(a.values), np.asarray(b.values))
  stat, b_f, b_64 = _points(which, pred, targ, power, dtype)
  frame = tuple(d for d in DIMS if d != 'level') if which == 'level' else DIMS
  np.testing.assert_array_equal(np.isnan(np.asarray(a.transpose(*frame).values)), np.isnan(stat))  # any non-finite input: NaN, nothing else
  n =int(np.prod([a.sizes[d] for d in REDUCE]))
  wmax = _max_area_weight() if case['area'] else 1.0
  mag = float(np.nansum(np.abs(stat)))
  bound = wmax * (float(b_f.sum() + 2 * b_64.sum()) + (n + 4) * 2.0 ** -52 * mag)
  x, y = state.sum_weighted_statistics[name]['v'], state64.sum_weighted_statistics[name]['v']
  assert tuple(x.dims) == tuple(y.dims) and set(x.coords) == set(y.coords), (x.dims, y.dims)
  print(which, case_name, 'max |fused - host| of the sums:', float(np.nanmax(np.abs(np.asarray(x.values) - np.asarray(y.values)))), 'bound', bound)
  np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=0, atol=bound, equal_nan=True)
  assert np.isfinite(np.asarray(x.values)).all()
  np.testing.assert_allclose(np.asarray(state.sum_weights[name]['v'].values), np.asarray(state64.sum_weights[name]['v'].values), rtol=1e-12, atol=0)
  got, host = values['vs.v'], values64['vs.v']
  assert tuple(got.dims) == tuple(host.dims) and set(got.coords) == set(host.coords)
  # ... and the restatement's, where the aggregation is a plain or NaN-skipping mean over (time, latitude, longitude)
  if case_name in ('plain', 'skipna'):
    axes = (0, 2, 3) if which != 'level' else (0, 1, 2)  # [time, level, lat, lon] -> [level]; [time, lat, lon] -> a number
    count = np.isfinite(stat).sum(axis=axes)
    want = np.nansum(stat, axis=axes) / count
    tol = (b_f.sum(axis=axes) + (n + 4) * 2.0 ** -52 * np.nansum(np.abs(stat), axis=axes)) / count
    print(which, case_name, 'max |fused - restatement| / bound:', float((np.abs(np.asarray(got.values) - want) / tol).max()))
    assert (np.abs(np.asarray(got.values) - want) <= tol).all()


def test_compute_metric_values_for_single_chunk_takes_the_fused_route(monkeypatch):
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  pred, targ = _inputs(mask=True)
  metrics = {'vs': METRICS['tiled'](0.5), 'lv': METRICS['level'](0.5)}
  agg = aggregation.Aggregator(reduce_dims=REDUCE, masked=True, weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)])
  values = aggregation.compute_metric_values_for_single_chunk(metrics, agg, pred, targ)
  assert len(_launches()) == 2 and len(engine.S1_EVENT_LOG) == 2
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', False)
  engine.clear_caches()
  values0 = aggregation.compute_metric_values_for_single_chunk(metrics, agg, pred, targ)
  assert set(values) == set(values0) == {'vs.v', 'lv.v'}
  for key in values:
    assert tuple(values[key].dims) == tuple(values0[key].dims)
    np.testing.assert_allclose(np.asarray(values[key].values), np.asarray(values0[key].values), rtol=2e-5, atol=0)


@pytest.mark.parametrize('which', list(METRICS))
def test_torch_resident_payloads_give_the_same_bits(monkeypatch, which):
  import torch  # pylint: disable=g-import-not-at-top
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  metrics = {'vs': METRICS[which](0.5)}
  (name,) = [s.unique_name for s in metrics['vs'].statistics.values()]
  # every output the sum of two points (the two times): the same bits whatever plan the storage order of the payload leads to
  make = lambda: aggregation.Aggregator(reduce_dims=['time'], weigh_by=[weighting.GridAreaWeighting()])
  pred, targ = _inputs()
  _, state, _ = _evaluate(metrics, pred, targ, make())
  dpred, dtarg = _inputs(device=True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state_t, _ = _evaluate(metrics, dpred, dtarg, make())
  assert all(_is_fused(s) for per_var in stats.values() for s in per_var.values()) and len(_launches()) == 1
  order = state.sum_weighted_statistics[name]['v'].dims
  np.testing.assert_array_equal(np.asarray(state_t.sum_weighted_statistics[name]['v'].transpose(*order).values),
                                np.asarray(state.sum_weighted_statistics[name]['v'].values))
  np.testing.assert_array_equal(np.asarray(state_t.sum_weights[name]['v'].transpose(*order).values), np.asarray(state.sum_weights[name]['v'].values))
  # every dim reduced under region bins: the same bits where the storage order is the same (`level`); the windows of a device
  # payload are strided views of the stack -- another plan, another order of summation: within twice the fused route's bound
  full = lambda: aggregation.Aggregator(reduce_dims=REDUCE, weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)])
  _, state, values = _evaluate(metrics, *_inputs(), full())
  _, state_t, values_t = _evaluate(metrics, *_inputs(device=True), full())
  x, y = np.asarray(state_t.sum_weighted_statistics[name]['v'].values), np.asarray(state.sum_weighted_statistics[name]['v'].values)
  if which == 'level':
    np.testing.assert_array_equal(x, y)
  else:
    stat, b_f, _ = _points(which, pred, targ, 0.5, np.float32)
    np.testing.assert_allclose(x, y, rtol=0, atol=_max_area_weight() * 2 * (float(b_f.sum()) + (stat.size + 4) * 2.0 ** -52 * float(np.abs(stat).sum())))
  # reading the per-point values of a device payload gives a tensor back: the host route's on that payload, bit for bit
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', False)
  stats0 = metrics_base.compute_unique_statistics_for_all_metrics(metrics, dpred, dtarg)
  a, b = stats[name]['v'], stats0[name]['v']
  assert torch.is_tensor(a.data) and a.data.is_cuda and torch.is_tensor(b.data) and a.data.dtype == b.data.dtype and tuple(a.dims) == tuple(b.dims)
  np.testing.assert_array_equal(np.asarray(a.values), np.asarray(b.values))


def _expanded_run(pred, targ):
  """Device payloads whose `level` run has stride 0 (an expanded view): no strided run of the kernel's."""
  import torch  # pylint: disable=g-import-not-at-top
  view = lambda da, ax: xr.DataArray(torch.as_tensor(np.asarray(da.values)).cuda().select(ax, 0).unsqueeze(ax).expand(*np.asarray(da.values).shape),
                                     dims=da.dims, coords={d: da.coords[d].values for d in da.dims}, name='v')
  return {'v': view(pred['v'], 2)}, {'v': view(targ['v'], 1)}


FALLBACKS = {
    'switch off': dict(switch=False),
    'p = 0.3': dict(power=0.3),
    'L = 65': dict(shape=(2, 65, 3, 4)),
    'M = 65': dict(m=65),
    'a run that is not one strided run': dict(expanded=True),
    'integer inputs': dict(dtype=np.int64),
    'members in the targets': dict(members_in_targets=True),
    'a dim the targets lack': dict(drop_level=True),
    'targets with a dim of their own': dict(extra_target_dim=True),
    'a mask along dim': dict(mask_dims=('level', 'latitude')),
}


@pytest.mark.parametrize('why', list(FALLBACKS))
def test_every_fallback_condition_gives_the_host_routes_result(monkeypatch, why):
  spec = FALLBACKS[why]
  shape = spec.get('shape', SHAPE)
  pred, targ = _inputs(np.float32, m=spec.get('m', M), shape=shape)
  if 'dtype' in spec:
    pred = {'v': pred['v'].astype(spec['dtype'])}
  if spec.get('members_in_targets'):
    targ = {'v': pred['v'] * 0.5}
  if spec.get('drop_level'):
    targ = {'v': targ['v'].isel(level=0, drop=True)}
  if spec.get('extra_target_dim'):
    targ = {'v': xr.concat([targ['v'].expand_dims(realization=[0]), (targ['v'] + 1.0).expand_dims(realization=[1])], dim='realization')}
  if 'mask_dims' in spec:
    md = spec['mask_dims']
    targ = {'v': targ['v'].assign_coords(mask=(md, np.random.default_rng(1).random(tuple(shape[DIMS.index(d)] for d in md)) > 0.3))}
  if spec.get('expanded'):
    pred, targ = _expanded_run(pred, targ)
  stat = probabilistic.VariogramScore(dim='level', ensemble_dim='number', p=spec.get('power', 0.5))
  reduce_dims = ['time', 'latitude', 'longitude']

  def run():
    try:
      per_var = stat.compute(pred, targ)
    except Exception as e:  # pylint: disable=broad-except  (inputs the host route refuses: the same refusal on both sides)
      return type(e), None
    state = aggregation.Aggregator(reduce_dims=reduce_dims).aggregate_statistics({stat.unique_name: per_var})
    return per_var['v'], state.sum_weighted_statistics[stat.unique_name]['v']
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', spec.get('switch', True))
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  points, sums = run()
  assert not _is_fused(points) and not _launches(), why
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', False)
  engine.clear_caches()
  points0, sums0 = run()
  if sums is None:
    assert points is points0 and sums0 is None, why
    return
  np.testing.assert_array_equal(np.asarray(points.values), np.asarray(points0.values), err_msg=why)
  np.testing.assert_array_equal(np.asarray(sums.values), np.asarray(sums0.values), err_msg=why)
  if 'power' not in spec and not spec.get('expanded'):
    return
  # and the fused route does take the neighbouring case
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  near = probabilistic.VariogramScore(dim='level', ensemble_dim='number', p=0.5).compute(*_inputs(np.float32))['v']
  assert _is_fused(near)


def test_the_largest_run_and_ensemble_are_fused(monkeypatch):
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  for m, shape in ((64, (2, 64, 2, 3)), (1, (2, 1, 2, 3))):
    pred, targ = _inputs(np.float32, m=m, shape=shape)
    stat = probabilistic.VariogramScore(dim='level', ensemble_dim='number', p=1.0)
    per_var = stat.compute(pred, targ)
    assert _is_fused(per_var['v'])
    state = aggregation.Aggregator(reduce_dims=['time']).aggregate_statistics({stat.unique_name: per_var})
    want, bound = VC.variogram_points(np.moveaxis(pred['v'].values, 2, -1), np.moveaxis(targ['v'].values, 1, -1), 1.0)
    got = np.asarray(state.sum_weighted_statistics[stat.unique_name]['v'].transpose('latitude', 'longitude').values)
    assert (np.abs(got - want.sum(axis=0)) <= bound.sum(axis=0) + 6 * 2.0 ** -52 * want.sum(axis=0)).all()
  assert len(_launches()) == 2


def test_two_powers_in_one_evaluation_are_two_groups(monkeypatch):
  """The statistics' unique names do not tell the powers apart; the groups do."""
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  pred, targ = _inputs(np.float32)
  stats = {}
  for power in (0.5, 2.0):
    stat = probabilistic.VariogramScore(dim='level', ensemble_dim='number', p=power)
    stats[f'p={power}'] = stat.compute(pred, targ)
  a, b = stats['p=0.5']['v'], stats['p=2.0']['v']
  assert _is_fused(a) and _is_fused(b) and a._group is not b._group and a._group.p is b._group.p  # pylint: disable=protected-access
  state = aggregation.Aggregator(reduce_dims=REDUCE).aggregate_statistics(stats)
  assert len(_launches()) == 2
  for power in (0.5, 2.0):
    stat, bound, _ = _points('level', pred, targ, power, np.float32)
    got = float(np.asarray(state.sum_weighted_statistics[f'p={power}']['v'].values))
    assert abs(got - stat.sum()) <= bound.sum() + (stat.size + 4) * 2.0 ** -52 * stat.sum(), power
  assert float(np.asarray(state.sum_weighted_statistics['p=0.5']['v'].values)) != float(np.asarray(state.sum_weighted_statistics['p=2.0']['v'].values))


def test_tiled_energy_and_variogram_scores_share_the_tiled_inputs(monkeypatch):
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', True)
  calls = []
  real = wrappers.construct_tiles
  monkeypatch.setattr(wrappers, 'construct_tiles', lambda da, **kw: calls.append(id(da)) or real(da, **kw))
  pred, targ = _inputs(np.float32)
  metrics = {'es': probabilistic.TiledEnergyScore(window_size=3, ensemble_dim='number'),
             'vs': probabilistic.TiledVariogramScore(window_size=3, ensemble_dim='number')}
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, _, values = _evaluate(metrics, pred, targ, aggregation.Aggregator(reduce_dims=REDUCE))
  assert sorted(calls) == sorted([id(pred['v']), id(targ['v'])])  # three statistics, each source object tiled once
  groups = [s._group for per_var in stats.values() for s in per_var.values()]  # pylint: disable=protected-access
  assert len(groups) == 3 and {g.kind for g in groups} == {'enrg', 'vgrm'}
  assert len({id(g.p) for g in groups}) == 1 and len({id(g.t) for g in groups}) == 1
  assert len(engine.S1_EVENT_LOG) == 2 and len(_launches()) == 1
  assert set(values) == {'es.v', 'vs.v'} and np.isfinite(np.asarray(values['vs.v'].values)).all()


def _chunk_job(n, nlead=2):
  import torch  # pylint: disable=g-import-not-at-top
  rng = np.random.default_rng(23)
  p_all = (rng.integers(-64, 65, size=(n, nlead, M) + SHAPE[1:]) / 8.0).astype(np.float32)
  t_all = (rng.integers(-64, 65, size=(n, nlead) + SHAPE[1:]) / 8.0).astype(np.float32)
  lead = (np.arange(nlead) * 12).astype('timedelta64[h]').astype('timedelta64[ns]')
  inits = np.datetime64('2020-01-01T00', 'ns') + np.arange(n) * np.timedelta64(24, 'h')
  index = {int(t.astype('int64')): i for i, t in enumerate(inits)}
  pd, td = ('init_time', 'lead_time', 'number') + DIMS[1:], ('init_time', 'lead_time') + DIMS[1:]
  dev = [(torch.as_tensor(p_all[i:i + 1]).cuda(), torch.as_tensor(t_all[i:i + 1]).cuda()) for i in range(n)]

  def load(init_chunk, lead_chunk):
    del lead_chunk
    i = index[int(init_chunk[0].astype('int64'))]
    cs = {'init_time': init_chunk, 'lead_time': lead, 'level': LEVEL, 'latitude': LAT, 'longitude': LON}
    return {'v': xr.DataArray(dev[i][0], dims=pd, coords=cs)}, {'v': xr.DataArray(dev[i][1], dims=td, coords=cs)}

  agg = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])
  return time_chunks.TimeChunks(inits, lead, init_time_chunk_size=1), load, agg, (p_all, t_all)


def test_chunk_loop_with_records_equals_the_unrecorded_loop(monkeypatch):
  """pipeline.evaluate_chunks over three one-init chunks of device-resident fields, with chunk records and without: the same
  accumulators bit for bit, and the restatement's numbers within the bound."""
  times, load, agg, (p_all, t_all) = _chunk_job(3)
  metrics = {'vs': _Level(0.5)}
  monkeypatch.setattr(lazy, 'FUSED_VARIOGRAM', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  name = metrics['vs'].statistics['VariogramScore'].unique_name
  np.testing.assert_array_equal(np.asarray(state.sum_weighted_statistics[name]['v'].values), np.asarray(off.sum_weighted_statistics[name]['v'].values))
  np.testing.assert_array_equal(np.asarray(state.sum_weights[name]['v'].values), np.asarray(off.sum_weights[name]['v'].values))
  pw = np.moveaxis(np.moveaxis(p_all, 2, 0), 3, -1)   # [number, init, lead, lat, lon, level]
  tw = np.moveaxis(t_all, 2, -1)
  stat, bound = VC.variogram_points(pw, tw, 0.5)      # [init, lead, lat, lon]
  probe = xr.DataArray(np.zeros(SHAPE[2:]), dims=DIMS[2:], coords={'latitude': LAT, 'longitude': LON})
  w = np.asarray(weighting.GridAreaWeighting().weights(probe).values, np.float64).reshape(-1, 1) * np.ones((1, SHAPE[3]))
  want = (stat * w[None, None]).sum(axis=(0, 2, 3))
  n = 3 * SHAPE[2] * SHAPE[3]
  tol = float(w.max()) * (bound.sum(axis=(0, 2, 3)) + (n + 4) * 2.0 ** -52 * stat.sum(axis=(0, 2, 3)))
  got = np.asarray(state.sum_weighted_statistics[name]['v'].transpose('lead_time').values)
  assert (np.abs(got - want) <= tol).all(), (got, want, tol)
