"""Contingency scores at threshold fields through the public API on the device: WrappedMetric(CSI / ETS / FrequencyBias behind
ContinuousToBinary('both', field, dim)) with the field a DataArray and a Dataset, on small fields (4 x 13 x 24).

Every evaluation goes through the Aggregator twice, lazy.FUSED_CONTINGENCY_FIELD on and off.  The aggregators weigh nothing (bins are
0 / 1 memberships), so every sum is an integer count below 2^53 on either route: the statistics, the weights and the metric values
are EQUAL BIT FOR BIT, NaN for NaN."""
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
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import categorical
from weatherbenchx_amd.metrics import wrappers

pytestmark = pytest.mark.gpu
DIMS = ('time', 'latitude', 'longitude')
SHAPE = (4, 13, 24)
LAT = np.linspace(-90, 90, SHAPE[1])
LON = np.arange(SHAPE[2]) * (360.0 / SHAPE[2])
PLACE = {'latitude': LAT, 'longitude': LON}
REGIONS = {'north': ((20, 90), (0, 360)), 'tropics': ((-20, 20), (0, 360)), 'box': ((-60, 10), (30, 200))}


@pytest.fixture(autouse=True)
def _device():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  engine.clear_caches()
  yield
  engine.clear_caches()


def test_the_library_exports_the_symbol_and_the_gate_opens():
  ctx = _hip.default_context()
  assert getattr(ctx.lib, 'wbx_contingency_field_partial', None) is not None
  assert engine.contingency_field_available(ctx) and lazy.FUSED_CONTINGENCY_FIELD and lazy.LazyContingencyField.launchable()


def _field(k=5, dtype=np.float64, dims=('percentile',) + DIMS[1:], seed=3, labelled=True):
  """Percentile-like thresholds of gamma(2) data, with the edges: NaN, +-inf, a tie with the data and the two sides of float32(0.1)."""
  rng = np.random.default_rng(seed)
  sizes = dict(zip(DIMS, SHAPE), percentile=k)
  levels = np.sort(rng.gamma(2.0, size=[k] + [sizes[d] for d in dims if d != 'percentile']), axis=0)
  values = np.ascontiguousarray(np.moveaxis(levels, 0, dims.index('percentile'))).astype(dtype)
  at = lambda j, *place: tuple({'percentile': j, **dict(zip(DIMS, (0,) + place))}[d] for d in dims)
  values[at(0, 0, 0)], values[at(1, 0, 1)], values[at(2, 0, 2)], values[at(0, 0, 3)] = np.nan, np.inf, -np.inf, 1.0
  values[at(1, 0, 4)] = 0.1 if np.dtype(dtype) == np.float64 else np.float32(0.1)
  cs = {d: PLACE[d] for d in dims if d in PLACE}
  if 'time' in dims:
    cs['time'] = np.arange(SHAPE[0])
  if labelled:
    cs['percentile'] = 100.0 - 10.0 / (1 + np.arange(k))
  return xr.DataArray(values, dims=dims, coords=cs)


def _inputs(dtype=np.float32, nans=False, mask=False, seed=11, variables=('u', 'v'), torch_payload=False):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(SHAPE[0]), **PLACE}
  pred, targ = {}, {}
  for v in variables:
    p, t = rng.gamma(2.0, size=SHAPE).astype(dtype), rng.gamma(2.0, size=SHAPE).astype(dtype)
    p[:, 0, 3], t[0, 0, 3] = 1.0, 1.0  # ties with the field
    p[:, 0, 4], t[:, 0, 4] = np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(0))  # both sides of 0.1
    if nans:
      p[rng.random(SHAPE) < 0.05] = np.nan
      t[rng.random(SHAPE) < 0.05] = np.nan
    tc = dict(cs)
    if mask:
      tc['mask'] = (DIMS[1:], rng.random(SHAPE[1:]) > 0.3)
    if torch_payload:
      import torch  # pylint: disable=g-import-not-at-top
      p, t = torch.as_tensor(p).cuda(), torch.as_tensor(t).cuda()
    pred[v] = xr.DataArray(p, dims=DIMS, coords=cs, name=v)
    targ[v] = xr.DataArray(t, dims=DIMS, coords=tc, name=v)
  return pred, targ


def _metrics(thresholds, dim='percentile'):
  binary = lambda: wrappers.ContinuousToBinary('both', thresholds, dim, unique_name_suffix='clim')
  return {name: wrappers.WrappedMetric(m, [binary()])
          for name, m in (('csi', categorical.CSI()), ('ets', categorical.ETS()), ('bias', categorical.FrequencyBias()))}


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def _on_and_off(monkeypatch, metrics, pred, targ, make, fused_expected=True, launches_per_variable=1):
  """The evaluation with the switch on and off: -> the fused route's state; everything is compared bit for bit in here."""
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY_FIELD', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats, state, values = _evaluate(metrics, pred, targ, make())
  launches = [e for e in engine.S1_EVENT_LOG if e['kind'] == 'cont']
  lazies = [s for per_var in stats.values() for s in per_var.values()]
  if fused_expected:
    assert all(isinstance(s, lazy.LazyContingencyField) and s._group.kind == 'cont' and s._group.clim is not None and s.is_lazy for s in lazies)  # pylint: disable=protected-access
    assert len(launches) == launches_per_variable * len(pred) == len(engine.S1_EVENT_LOG), engine.S1_EVENT_LOG
  else:
    assert not any(isinstance(s, lazy.LazyContingency) for s in lazies) and not launches
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY_FIELD', False)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  stats0, state0, values0 = _evaluate(metrics, pred, targ, make())
  assert not any(isinstance(s, lazy.LazyContingency) for per_var in stats0.values() for s in per_var.values())
  assert not [e for e in engine.S1_EVENT_LOG if e['kind'] == 'cont']
  finite = 0
  for tree, tree0 in ((state.sum_weighted_statistics, state0.sum_weighted_statistics), (state.sum_weights, state0.sum_weights)):
    assert set(tree) == set(tree0)
    for stat in tree:
      for var in tree[stat]:
        x, y = tree[stat][var], tree0[stat][var]
        assert tuple(x.dims) == tuple(y.dims), (stat, var, x.dims, y.dims)
        assert set(x.coords) == set(y.coords), (stat, var, sorted(map(str, x.coords)), sorted(map(str, y.coords)))
        for c in x.coords:
          np.testing.assert_array_equal(np.asarray(x.coords[c].values), np.asarray(y.coords[c].values))
        np.testing.assert_array_equal(np.asarray(x.values), np.asarray(y.values, np.float64), err_msg=f'{stat} {var} vs the host route')
        finite += int(np.isfinite(np.asarray(x.values)).sum())
  assert finite > 0
  assert set(values) == set(values0)
  for key in values:
    assert tuple(values[key].dims) == tuple(values0[key].dims) and set(values[key].coords) == set(values0[key].coords)
    np.testing.assert_array_equal(np.asarray(values[key].values), np.asarray(values0[key].values), err_msg=key)
  return state


CASES = {
    'plain': dict(make=lambda: aggregation.Aggregator(reduce_dims=list(DIMS)), nans=False, mask=False),
    'keep-latitude': dict(make=lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude']), nans=False, mask=False),
    'regions-masked': dict(make=lambda: aggregation.Aggregator(reduce_dims=list(DIMS), bin_by=[binning.Regions(REGIONS)], masked=True),
                           nans=False, mask=True),
    'skipna': dict(make=lambda: aggregation.Aggregator(reduce_dims=list(DIMS), skipna=True), nans=True, mask=False),
    'poisoned': dict(make=lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude']), nans=True, mask=False),
}


@pytest.mark.parametrize('as_dataset', [False, True], ids=['dataarray', 'dataset'])
@pytest.mark.parametrize('pair', [(np.float32, np.float64), (np.float32, np.float32), (np.float64, np.float32), (np.float64, np.float64)],
                         ids=['f32-at-f64', 'f32-at-f32', 'f64-at-f32', 'f64-at-f64'])
@pytest.mark.parametrize('which', list(CASES))
def test_scores_equal_the_host_route_bit_for_bit(monkeypatch, which, pair, as_dataset):
  case = CASES[which]
  pred, targ = _inputs(pair[0], nans=case['nans'], mask=case['mask'])
  field = _field(dtype=pair[1])
  thresholds = xr.Dataset({'u': field, 'v': _field(dtype=pair[1], seed=4)}) if as_dataset else field
  state = _on_and_off(monkeypatch, _metrics(thresholds), pred, targ, case['make'])
  some = next(iter(state.sum_weighted_statistics.values()))['u']
  assert 'percentile' in some.dims and 'percentile' in some.coords


def test_torch_payloads_and_a_field_in_hbm(monkeypatch):
  import torch  # pylint: disable=g-import-not-at-top
  pred, targ = _inputs(torch_payload=True, mask=True)
  field = _field(dtype=np.float64)
  on_device = xr.DataArray(torch.as_tensor(np.asarray(field.values)).cuda(), dims=field.dims, coords={d: field.coords[d].values for d in field.dims})
  make = lambda: aggregation.Aggregator(reduce_dims=list(DIMS), bin_by=[binning.Regions(REGIONS)], masked=True)
  for thresholds in (field, on_device):
    _on_and_off(monkeypatch, _metrics(thresholds), pred, targ, make)


def test_other_layouts_of_the_field(monkeypatch):
  """The threshold dim in the middle and innermost, a field over longitude only, over (time, latitude, longitude), unlabelled."""
  pred, targ = _inputs()
  make = lambda: aggregation.Aggregator(reduce_dims=list(DIMS))
  for dims in (('latitude', 'percentile', 'longitude'), ('latitude', 'longitude', 'percentile'), ('percentile', 'longitude'),
               ('percentile',) + DIMS, ('longitude', 'percentile', 'latitude')):
    for labelled in (True, False):
      state = _on_and_off(monkeypatch, _metrics(_field(dims=dims, labelled=labelled)), pred, targ, make)
      some = next(iter(state.sum_weighted_statistics.values()))['u']
      assert ('percentile' in some.coords) == labelled, (dims, labelled)


def test_a_field_broadcast_along_its_threshold_dim_keeps_the_host_route(monkeypatch):
  """A device tensor expanded along the threshold dim (stride 0, three thresholds) has no stride to step by: the host route, the
  same numbers; made contiguous it is fused."""
  import torch  # pylint: disable=g-import-not-at-top
  pred, targ = _inputs(variables=('v',))
  make = lambda: aggregation.Aggregator(reduce_dims=list(DIMS))
  one = torch.as_tensor(np.asarray(_field(k=3).values)[:1].copy()).cuda()
  for data, fused in ((one.expand(3, -1, -1), False), (one.expand(3, -1, -1).contiguous(), True), (one, True)):
    field = xr.DataArray(data, dims=('percentile',) + DIMS[1:], coords=PLACE)
    _on_and_off(monkeypatch, _metrics(field), pred, targ, make, fused_expected=fused)


def test_twenty_thresholds_are_two_launches(monkeypatch):
  pred, targ = _inputs(mask=True, nans=True)
  make = lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude'], masked=True, skipna=True)
  state = _on_and_off(monkeypatch, _metrics(_field(k=20)), pred, targ, make, launches_per_variable=2)
  assert next(iter(state.sum_weighted_statistics.values()))['u'].sizes['percentile'] == 20


def test_a_mutated_field_is_uploaded_again(monkeypatch):
  pred, targ = _inputs(variables=('v',))
  field = _field()
  make = lambda: aggregation.Aggregator(reduce_dims=list(DIMS))
  metrics = _metrics(field)
  first = _on_and_off(monkeypatch, metrics, pred, targ, make)
  dev = field.__dict__['_wbx_dev']
  _on_and_off(monkeypatch, metrics, *_inputs(variables=('v',), seed=12), make)
  assert field.__dict__['_wbx_dev'] is dev  # one upload per field object
  field[...] = np.asarray(field.values) + 0.5
  second = _on_and_off(monkeypatch, metrics, pred, targ, make)
  assert field.__dict__['_wbx_dev'] is not dev
  key = next(k for k in first.sum_weighted_statistics if k.startswith('TruePositives'))
  assert not np.array_equal(np.asarray(first.sum_weighted_statistics[key]['v'].values), np.asarray(second.sum_weighted_statistics[key]['v'].values))


def test_what_the_gate_declines_runs_on_the_host_route_on_the_device(monkeypatch):
  pred, targ = _inputs(variables=('v',))
  make = lambda: aggregation.Aggregator(reduce_dims=list(DIMS))
  declined = {
      'a labelled list': _field(dims=('percentile',)),
      'labels that differ': xr.DataArray(np.asarray(_field().values), dims=_field().dims, coords={'latitude': LAT[::-1].copy(), 'longitude': LON}),
      'unlabelled places': xr.DataArray(np.asarray(_field().values), dims=_field().dims),
      'a coordinate beyond its dims': xr.DataArray(np.asarray(_field().values), dims=_field().dims, coords=dict(PLACE, height=((), np.float64(2.0)))),
  }
  for why, field in declined.items():
    _on_and_off(monkeypatch, _metrics(field), pred, targ, make, fused_expected=False)
  # which = 'predictions' and a subclass of the transform
  class Mine(wrappers.ContinuousToBinary):
    pass
  for transform in (wrappers.ContinuousToBinary('predictions', _field(), 'percentile', unique_name_suffix='clim'),
                    Mine('both', _field(), 'percentile', unique_name_suffix='clim')):
    binary_targ = {'v': (targ['v'] > 1.0).astype(np.float32)} if transform.which == 'predictions' else targ
    _on_and_off(monkeypatch, {'csi': wrappers.WrappedMetric(categorical.CSI(), [transform])}, pred, binary_targ, make, fused_expected=False)
  # the whole family off: fields included
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY', False)
  _on_and_off(monkeypatch, _metrics(_field()), pred, targ, make, fused_expected=False)
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY', True)
  # a Dataset without the variable: the host route's assertion, raised by the host route, with the switch on and off
  for fused in (True, False):
    monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY_FIELD', fused)
    with pytest.raises(ValueError) as err:
      _evaluate(_metrics(xr.Dataset({'w': _field()})), pred, targ, make())
    assert isinstance(err.value.__cause__, AssertionError)


def test_chunk_loop_with_records_enabled(monkeypatch):
  """pipeline.evaluate_chunks over 8 one-init chunks of device-resident fields with chunk records enabled: the accumulated sums equal
  the loop's without records and on the host route bit for bit.  (The entry has no function id, so these chunks are evaluated call by
  call whether records are enabled or not: DESIGN 4.20.)"""
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
    return {'v': xr.DataArray(dev[i][0], dims=dims, coords=cs, name='v')}, {'v': xr.DataArray(dev[i][1], dims=dims, coords=cs, name='v')}

  metrics = _metrics(xr.Dataset({'v': _field()}))
  agg = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'], bin_by=[binning.Regions(REGIONS)])
  times = time_chunks.TimeChunks(inits, lead, init_time_chunk_size=1)
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY_FIELD', True)
  monkeypatch.setattr(replay, 'ENABLED', True)
  replay.reset_stats()
  state = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  engine.clear_caches()
  monkeypatch.setattr(replay, 'ENABLED', False)
  off = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  engine.clear_caches()
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY_FIELD', False)
  host = pipeline.evaluate_chunks(times, load, metrics, agg)[None]
  for key in host.sum_weighted_statistics:
    for other in (off, host):
      np.testing.assert_array_equal(np.asarray(state.sum_weighted_statistics[key]['v'].values),
                                    np.asarray(other.sum_weighted_statistics[key]['v'].values, np.float64), err_msg=key)
      np.testing.assert_array_equal(np.asarray(state.sum_weights[key]['v'].values), np.asarray(other.sum_weights[key]['v'].values, np.float64))
    assert np.isfinite(np.asarray(state.sum_weighted_statistics[key]['v'].values)).all()
