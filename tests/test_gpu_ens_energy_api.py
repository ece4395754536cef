"""EnergyScore / TiledEnergyScore through the public API on the device: compute_unique_statistics_for_all_metrics + the Aggregator
on small fields (5 members, 2 x 3 x 6 x 9) under a plain reduction, GridAreaWeighting with Regions bins, a target mask, and skipna
with NaNs; NumPy and torch-resident payloads; every fallback condition; a recorded and replayed chunk loop.

Bounds (tests/energy_cases.py derives the fused route's): a per-point value of the fused route is within
r_f = (L / 2 + 4) u + (M^2 + 4) 2^-53 of the exact one, relatively, u = 2^-24 for float32 inputs and 2^-53 for float64 ones.  The
host route forms the same norms in the input type ((L / 2 + 4) u) and then adds them in the input type too: M terms for the skill
(M u more), M - 1 passes of M terms and the M - 1 pass sums for the spread (2 M u more), so it is within r_h = (L / 2 + 4 + 2 M) u.
The oracle is float64 throughout: r_o = (L / 2 + 4 + M^2) 2^-53.  Every per-point value is non-negative, so a weighted sum over N
points with non-negative weights W inherits the relative bound on sum W |value| <= N max W max |value|, plus (N + 4) 2^-53 of it
for the float64 summation (stage 1, stage 2); a metric value is a weighted mean of per-point values: the relative bounds times
max |value|, for the skill plus half the spread."""
import numpy as np
import pytest

import energy_cases as GC
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
from weatherbenchx_amd.metrics import probabilistic

pytestmark = pytest.mark.gpu
DIMS = ('time', 'level', 'latitude', 'longitude')
SHAPE = (2, 3, 6, 9)
M = 5
LAT = np.linspace(-75, 75, SHAPE[2])
LON = np.arange(SHAPE[3]) * (360.0 / SHAPE[3])
LEVEL = np.array([500.0, 700.0, 850.0])
REGIONS = {'global': ((-90, 90), (0, 360)), 'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'east': ((-90, 90), (0, 180))}


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  assert engine.ens_energy_available(_hip.default_context())
  engine.clear_caches()
  yield
  engine.clear_caches()


def _inputs(dtype=np.float32, nans=False, mask=False, seed=11, pdims=('number',) + DIMS, tdims=DIMS, m=M):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(SHAPE[0]), 'level': LEVEL, 'latitude': LAT, 'longitude': LON, 'number': np.arange(m)}
  sizes = dict(zip(DIMS, SHAPE), number=m)
  p = (rng.integers(-64, 65, size=tuple(sizes[d] for d in pdims)) / 8.0).astype(dtype)
  t = (rng.integers(-64, 65, size=tuple(sizes[d] for d in tdims)) / 8.0).astype(dtype)
  if nans:
    p[rng.random(p.shape) < 0.004] = np.nan
    t[rng.random(t.shape) < 0.03] = np.nan
  tc = {d: cs[d] for d in tdims}
  if mask:
    tc['mask'] = (('latitude', 'longitude'), rng.random(SHAPE[2:]) > 0.3)
  return ({'v': xr.DataArray(p, dims=pdims, coords={d: cs[d] for d in pdims}, name='v')},
          {'v': xr.DataArray(t, dims=tdims, coords=tc, name='v')})


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyStatistic) and stat._group.kind == 'enrg'  # pylint: disable=protected-access


def _launches():
  return [e for e in engine.S1_EVENT_LOG if e['kind'] == 'enrg']


def _max_area_weight():
  probe = xr.DataArray(np.zeros(SHAPE[2:]), dims=DIMS[2:], coords={'latitude': LAT, 'longitude': LON})
  return float(np.asarray(weighting.GridAreaWeighting().weights(probe).values).max())


def _unit(dtype):
  return GC.unit(dtype)


def _r_fused(nl, dtype, m=M):
  return GC.relative_bound(m, nl, dtype)


def _r_host(nl, dtype, m=M):
  return (nl / 2.0 + 4.0 + 2 * m) * _unit(dtype)


def _r_oracle(nl, m=M):
  return (nl / 2.0 + 4.0 + m * m) * 2.0 ** -53


METRICS = {
    'level': lambda fair: probabilistic.EnergyScore(dim='level', ensemble_dim='number', fair=fair),
    'tiled': lambda fair: probabilistic.TiledEnergyScore(window_size=3, ensemble_dim='number', fair=fair),
}
NORM_LEN = {'level': SHAPE[1], 'tiled': 9}
CASES = {
    'plain': dict(kw=lambda: {}, nans=False, mask=False, area=False),
    'regions': dict(kw=lambda: dict(weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)]), nans=False, mask=False, area=True),
    'masked': dict(kw=lambda: dict(masked=True, weigh_by=[weighting.GridAreaWeighting()]), nans=False, mask=True, area=True),
    'skipna': dict(kw=lambda: dict(skipna=True), nans=True, mask=False, area=False),
}


def _oracle_points(which, pred, targ, fair):
  """Per-point (skill, spread) of the oracle on the float64-widened inputs, over the metric's frame."""
  p, t = np.asarray(pred['v'].values, np.float64), np.asarray(targ['v'].values, np.float64)
  if which == 'tiled':
    tile = lambda a, ilat: np.stack([np.roll(np.roll(a, i - 1, ilat), j - 1, ilat + 1) for i in range(3) for j in range(3)])
    p, t = tile(p, 3), tile(t, 2)                       # [window, number, time, level, lat, lon], [window, time, level, lat, lon]
    p, t = p[..., 1:-1, :], t[..., 1:-1, :]
    with np.errstate(all='ignore'):
      return O.energy_score_skill(np.moveaxis(p, 1, 0), t[None], 1, 0), O.energy_score_spread(np.moveaxis(p, 1, 0), 1, 0, fair=fair)
  with np.errstate(all='ignore'):
    return O.energy_score_skill(p, t[None], 2, 0), O.energy_score_spread(p, 2, 0, fair=fair)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('case_name', list(CASES))
@pytest.mark.parametrize('which', list(METRICS))
def test_scores_against_the_host_route_and_the_oracle(monkeypatch, which, case_name, dtype):
  case, fair, nl = CASES[case_name], case_name != 'regions', NORM_LEN[which]
  reduce_dims = ['time', 'latitude', 'longitude']
  pred, targ = _inputs(dtype, nans=case['nans'], mask=case['mask'])
  metrics = {'es': METRICS[which](fair)}
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(metrics, pred, targ, aggregation.Aggregator(reduce_dims=reduce_dims, **case['kw']()))
  assert len(stats) == 2 and all(_is_fused(s) and s.is_lazy for per_var in stats.values() for s in per_var.values())
  # the skill and the spread of the pair share one launch -- unless only the skill carries the targets' mask: the spread is a
  # statistic of the predictions alone and is then reduced unmasked, as on the host route
  assert len(_launches()) == (2 if case['mask'] else 1) and len(engine.S1_EVENT_LOG) == len(_launches()), engine.S1_EVENT_LOG
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats0, state0, values0 = _evaluate(metrics, pred, targ, aggregation.Aggregator(reduce_dims=reduce_dims, **case['kw']()))
  assert not any(_is_fused(s) for per_var in stats0.values() for s in per_var.values()) and not _launches()
  # what anybody reads per point is the host route's, bit for bit
  assert set(stats) == set(stats0)
  for name in stats:
    a, b = stats[name]['v'], stats0[name]['v']
    assert tuple(a.dims) == tuple(b.dims) and set(a.coords) == set(b.coords), (name, a.dims, b.dims)
    np.testing.assert_array_equal(np.asarray(a.values), np.asarray(b.values), err_msg=name)
  skill, spread = _oracle_points(which, pred, targ, fair)
  vmax = {False: float(np.nanmax(skill)), True: float(np.nanmax(spread))}
  n = int(np.prod([SHAPE[DIMS.index(d)] for d in reduce_dims]))
  wmax = _max_area_weight() if case['area'] else 1.0
  rel = _r_fused(nl, dtype) + _r_host(nl, dtype) + (n + 4) * 2.0 ** -52
  for name in stats:
    is_spread = 'Spread' in name
    x, y = state.sum_weighted_statistics[name]['v'], state0.sum_weighted_statistics[name]['v']
    assert tuple(x.dims) == tuple(y.dims) and set(x.coords) == set(y.coords), (name, x.dims, y.dims)
    bound = rel * n * wmax * vmax[is_spread]
    print(which, case_name, name, 'max |fused - host| of the sums:', float(np.nanmax(np.abs(np.asarray(x.values) - np.asarray(y.values)))), 'bound', bound)
    np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=0, atol=bound, equal_nan=True, err_msg=f'{name} sums')
    assert np.isfinite(np.asarray(x.values)).all()
    x, y = state.sum_weights[name]['v'], state0.sum_weights[name]['v']
    np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=1e-12, atol=0, err_msg=f'{name} weights')
  assert set(values) == set(values0) == {'es.v'}
  got, host = values['es.v'], values0['es.v']
  assert tuple(got.dims) == tuple(host.dims) and set(got.coords) == set(host.coords)
  scale = vmax[False] + 0.5 * vmax[True]
  print(which, case_name, 'max |fused - host| of the score:', float(np.nanmax(np.abs(np.asarray(got.values) - np.asarray(host.values)))), 'bound', rel * scale)
  np.testing.assert_allclose(np.asarray(got.values), np.asarray(host.values), rtol=0, atol=rel * scale, equal_nan=True)
  # ... and the oracle's, where the aggregation is a plain or NaN-skipping mean over (time, latitude, longitude)
  if case_name in ('plain', 'skipna'):
    axes = (0, 2, 3) if which == 'tiled' else (0, 1, 2)  # [time, level, lat, lon] -> [level]; [time, lat, lon] -> a number
    with np.errstate(all='ignore'):
      want = np.nanmean(skill, axis=axes) - 0.5 * np.nanmean(spread, axis=axes)
    rel_o = _r_fused(nl, dtype) + _r_oracle(nl) + (n + 4) * 2.0 ** -52
    print(which, case_name, 'max |fused - oracle| of the score:', float(np.abs(np.asarray(got.values) - want).max()), 'bound', rel_o * scale)
    np.testing.assert_allclose(np.asarray(got.values), want, rtol=0, atol=rel_o * scale)


def test_norm_dims_that_are_no_single_run_keep_the_host_route(monkeypatch):
  """EnergyScore(dim=['latitude', 'longitude']): one run of the inputs as they come (fused), two runs with `level` stored between
  them (the host route); both give the same score within the bounds."""
  metrics = {'es': probabilistic.EnergyScore(dim=['latitude', 'longitude'], ensemble_dim='number')}
  agg = lambda: aggregation.Aggregator(reduce_dims=['time'])
  nl = SHAPE[2] * SHAPE[3]
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  pred, targ = _inputs(np.float32)
  stats, _, values = _evaluate(metrics, pred, targ, agg())
  assert all(_is_fused(s) for per_var in stats.values() for s in per_var.values()) and len(_launches()) == 1
  order = ('number', 'time', 'latitude', 'level', 'longitude')
  pred_t = {'v': pred['v'].transpose(*order)}
  pred_t = {'v': xr.DataArray(np.ascontiguousarray(pred_t['v'].values), dims=order, coords={d: pred['v'].coords[d].values for d in order}, name='v')}
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats_t, _, values_t = _evaluate(metrics, pred_t, targ, agg())
  assert not any(_is_fused(s) for per_var in stats_t.values() for s in per_var.values()) and not _launches()
  p64, t64 = np.asarray(pred['v'].values, np.float64), np.asarray(targ['v'].values, np.float64)
  want = (O.energy_score_skill(p64, t64[None], (3, 4), 0) - 0.5 * O.energy_score_spread(p64, (3, 4), 0)).mean(axis=0)
  scale = float(want.max()) * 2
  np.testing.assert_allclose(np.asarray(values['es.v'].transpose('level').values), want, rtol=0,
                             atol=(_r_fused(nl, np.float32) + _r_oracle(nl) + 8 * 2.0 ** -52) * scale)
  np.testing.assert_allclose(np.asarray(values_t['es.v'].transpose('level').values), want, rtol=0,
                             atol=(_r_host(nl, np.float32) + _r_oracle(nl) + 8 * 2.0 ** -52) * scale)


FALLBACKS = {
    'switch off': dict(switch=False),
    'integer inputs': dict(dtype=np.int64),
    'members in the targets': dict(tdims=('number',) + DIMS),
    'a norm dim the targets lack': dict(tdims=('time', 'latitude', 'longitude')),
    'targets with a dim of their own': dict(extra_target_dim=True),
    'nothing left of the frame': dict(norm=list(DIMS), reduce=[]),
    'a mask along the norm dim': dict(mask_dims=('level', 'latitude')),
    'one member': dict(m=1, fair=False),
    'more members than the kernel takes': dict(m=_hip.ENRG_MAX_MEMBERS + 1),
}


@pytest.mark.parametrize('why', list(FALLBACKS))
def test_every_fallback_condition_gives_the_host_routes_result(monkeypatch, why):
  spec = FALLBACKS[why]
  pred, targ = _inputs(np.float32, tdims=spec.get('tdims', DIMS), m=spec.get('m', M))
  if 'dtype' in spec:
    pred = {'v': pred['v'].astype(spec['dtype'])}
  if spec.get('extra_target_dim'):
    targ = {'v': xr.concat([targ['v'].expand_dims(realization=[0]), (targ['v'] + 1.0).expand_dims(realization=[1])], dim='realization')}
  if 'mask_dims' in spec:
    md = spec['mask_dims']
    shape = tuple(SHAPE[DIMS.index(d)] for d in md)
    targ = {'v': targ['v'].assign_coords(mask=(md, np.random.default_rng(1).random(shape) > 0.3))}
  metrics = {'es': probabilistic.EnergyScore(dim=spec.get('norm', 'level'), ensemble_dim='number', fair=spec.get('fair', True))}
  reduce_dims = spec.get('reduce', ['time', 'latitude', 'longitude'])
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', spec.get('switch', True))
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(metrics, pred, targ, aggregation.Aggregator(reduce_dims=reduce_dims))
  assert not any(_is_fused(s) for per_var in stats.values() for s in per_var.values()) and not _launches(), why
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', False)
  engine.clear_caches()
  stats0, state0, values0 = _evaluate(metrics, pred, targ, aggregation.Aggregator(reduce_dims=reduce_dims))
  for name in stats:
    np.testing.assert_array_equal(np.asarray(stats[name]['v'].values), np.asarray(stats0[name]['v'].values), err_msg=f'{why}: {name}')
  np.testing.assert_array_equal(np.asarray(values['es.v'].values), np.asarray(values0['es.v'].values), err_msg=why)


def test_a_nan_under_a_valid_point_poisons_its_lane_only(monkeypatch):
  """A NaN target poisons the skill of its output and leaves the spread alone; hidden by the mask it leaves no trace."""
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', True)
  metrics = {'es': probabilistic.EnergyScore(dim='level', ensemble_dim='number')}
  make = lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude'], masked=True)
  names = {k: s.unique_name for k, s in metrics['es'].statistics.items()}
  pred, targ = _inputs(mask=True)
  valid = np.asarray(targ['v'].coords['mask'].values, bool)
  hidden, shown = np.argwhere(~valid)[0], np.argwhere(valid)[0]
  targ['v'].data[1, 0, hidden[0], hidden[1]] = np.nan
  _, state, _ = _evaluate(metrics, pred, targ, make())
  for name in names.values():
    assert np.isfinite(np.asarray(state.sum_weighted_statistics[name]['v'].values)).all()
  pred, targ = _inputs(mask=True)
  targ['v'].data[1, 2, shown[0], shown[1]] = np.nan
  _, state, _ = _evaluate(metrics, pred, targ, make())
  bad = np.isnan(np.asarray(state.sum_weighted_statistics[names['EnergyScoreSkill']]['v'].transpose('latitude').values))
  assert bad[shown[0]] and not np.delete(bad, shown[0]).any()
  assert np.isfinite(np.asarray(state.sum_weighted_statistics[names['EnergyScoreSpread']]['v'].values)).all()


@pytest.mark.parametrize('which', list(METRICS))
def test_torch_resident_payloads_give_the_same_bits(monkeypatch, which):
  import torch  # pylint: disable=g-import-not-at-top
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', True)
  metrics = {'es': METRICS[which](True)}
  make = lambda: aggregation.Aggregator(reduce_dims=['time', 'latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()], bin_by=[binning.Regions(REGIONS)])
  pred, targ = _inputs()
  stats_h, state, values = _evaluate(metrics, pred, targ, make())
  on_dev = lambda da: xr.DataArray(torch.as_tensor(np.asarray(da.values)).cuda(), dims=da.dims, coords={d: da.coords[d].values for d in da.dims}, name=da.name)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state_t, values_t = _evaluate(metrics, {'v': on_dev(pred['v'])}, {'v': on_dev(targ['v'])}, make())
  assert all(_is_fused(s) for per_var in stats.values() for s in per_var.values()) and len(_launches()) == 1
  if which == 'level':  # the same storage order on both sides: the same plan, the same bits
    for name in stats:
      np.testing.assert_array_equal(np.asarray(state_t.sum_weighted_statistics[name]['v'].values), np.asarray(state.sum_weighted_statistics[name]['v'].values))
      np.testing.assert_array_equal(np.asarray(state_t.sum_weights[name]['v'].values), np.asarray(state.sum_weights[name]['v'].values))
  else:  # the windows of a device payload are strided views of the stack: another storage order, another order of summation
    scale = float(np.abs(np.asarray(values['es.v'].values)).max()) * 4
    np.testing.assert_allclose(np.asarray(values_t['es.v'].values), np.asarray(values['es.v'].values), rtol=0,
                               atol=2 * (_r_fused(9, np.float32) + 200 * 2.0 ** -52) * scale)
  # reading the per-point values of a device payload gives a tensor back: the host route's on that payload, bit for bit (torch
  # arithmetic on the device, which adds the squares and the members in another order than NumPy does on host arrays), and
  # within both routes' bounds of the host route's on the NumPy payload
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats0 = metrics_base.compute_unique_statistics_for_all_metrics(metrics, {'v': on_dev(pred['v'])}, {'v': on_dev(targ['v'])})
  assert set(stats0) == set(stats) == set(stats_h) and len(stats) == 2
  assert not any(_is_fused(s) for per_var in stats0.values() for s in per_var.values()) and not _launches()
  for name in stats:
    a, b, c = stats[name]['v'], stats0[name]['v'], stats_h[name]['v']
    assert torch.is_tensor(a.data) and a.data.is_cuda and torch.is_tensor(b.data) and a.data.dtype == b.data.dtype
    assert tuple(a.dims) == tuple(b.dims) == tuple(c.dims)
    np.testing.assert_array_equal(np.asarray(a.values), np.asarray(b.values), err_msg=name)
    scale = float(np.abs(np.asarray(c.values)).max())
    np.testing.assert_allclose(np.asarray(a.values), np.asarray(c.values), rtol=0,
                               atol=2 * _r_host(NORM_LEN[which], np.float32) * scale, err_msg=name)


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
  accumulators bit for bit, and the oracle's numbers within the bound."""
  times, load, agg, (p_all, t_all) = _chunk_job(3)
  metrics = {'es': probabilistic.EnergyScore(dim='level', ensemble_dim='number')}
  monkeypatch.setattr(lazy, 'FUSED_ENERGY', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  stats = dict(replay.STATS)
  assert stats['refused'] == 0 and not stats['refusals'], stats
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  for stat in metrics['es'].statistics.values():
    name = stat.unique_name
    np.testing.assert_array_equal(np.asarray(state.sum_weighted_statistics[name]['v'].values), np.asarray(off.sum_weighted_statistics[name]['v'].values))
    np.testing.assert_array_equal(np.asarray(state.sum_weights[name]['v'].values), np.asarray(off.sum_weights[name]['v'].values))
  p64, t64 = np.moveaxis(p_all, 2, 0).astype(np.float64), t_all.astype(np.float64)  # [number, init, lead, level, lat, lon]
  skill = O.energy_score_skill(p64, t64[None], 3, 0)                                  # [init, lead, lat, lon]
  probe = xr.DataArray(np.zeros(SHAPE[2:]), dims=DIMS[2:], coords={'latitude': LAT, 'longitude': LON})
  w = np.asarray(weighting.GridAreaWeighting().weights(probe).values, np.float64).reshape(-1, 1) * np.ones((1, SHAPE[3]))
  want = (skill * w[None, None]).sum(axis=(0, 2, 3))
  name = metrics['es'].statistics['EnergyScoreSkill'].unique_name
  n = 3 * SHAPE[2] * SHAPE[3]
  bound = (_r_fused(SHAPE[1], np.float32) + _r_oracle(SHAPE[1]) + (n + 4) * 2.0 ** -52) * n * float(w.max()) * float(skill.max())
  np.testing.assert_allclose(np.asarray(state.sum_weighted_statistics[name]['v'].transpose('lead_time').values), want, rtol=0, atol=bound)
