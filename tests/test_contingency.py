"""Thresholded contingency tables behind wrappers.ContinuousToBinary, without a device: the entry point's export and argument
checks, the eligibility rules of `_Indicator.compute_with_transform`, `LazyContingency` as a labelled array, and the host logic of
the fused route (one launch for the four cells, lane blocks, threshold blocks, the gate) with the launch itself stood in for by
the float64 restatement of tests/contingency_cases.py."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import contingency_cases as CC
import fake_device
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import binning
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import weighting
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import categorical
from weatherbenchx_amd.metrics import wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = ('time', 'latitude', 'longitude')
THR = [1.0, 2.5, 0.5]


# ---- the C ABI, no device ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_refuses_a_null_context():
  lib = _hip.load_library()
  assert 'wbx_contingency_partial' in _hip.EXPORTED_SYMBOLS and 'wbx_contingency_partial' in _hip.PROTOS
  assert lib.wbx_abi_version() == 13
  rc = lib.wbx_contingency_partial(None, None, _hip.F32, 1, None, None, None, None, None)
  assert rc == -1  # WBX_ERR_INVALID
  assert 'wbx_contingency_partial: ctx is NULL' in lib.wbx_last_error().decode()
  with pytest.raises(_hip.WbxError, match='ctx is NULL'):
    _hip.check(rc, 'wbx_contingency_partial')


def test_header_enum_matches_the_binding():
  with open(os.path.join(ROOT, 'include', 'wbx.h')) as f:
    header = f.read()
  assert int(re.search(r'WBX_FN_CONTINGENCY_PARTIAL\s*=\s*(\d+)', header).group(1)) == _hip.FN_IDS['wbx_contingency_partial'] == 20
  assert int(re.search(r'#define WBX_CONT_CELLS (\d+)', header).group(1)) == _hip.CONT_CELLS == 4
  assert int(re.search(r'#define WBX_CONT_MAX_THRESHOLDS (\d+)', header).group(1)) == _hip.CONT_MAX_THRESHOLDS
  assert int(re.search(r'#define WBX_ABI_VERSION (\d+)', header).group(1)) == 13
  assert len(set(_hip.FN_IDS.values())) == len(_hip.FN_IDS)
  # prototype: ctx, plan, dtype, nthr, p, t, thresholds, mask, partial_out
  assert len(_hip.load_library() and _hip.PROTOS['wbx_contingency_partial']) == 9
  assert lazy.CONT_CELL == {'TruePositives': 0, 'FalsePositives': 1, 'FalseNegatives': 2, 'TrueNegatives': 3}


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _inputs(dtype=np.float32, shape=(3, 8, 10), nans=False, mask=False, seed=37, variables=('v',)):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(shape[0]), 'latitude': np.linspace(-70, 70, shape[1]), 'longitude': np.arange(shape[2]) * (360.0 / shape[2])}
  pred, targ = {}, {}
  for v in variables:
    p, t = rng.gamma(2.0, size=shape).astype(dtype), rng.gamma(2.0, size=shape).astype(dtype)
    if nans:
      p[rng.random(shape) < 0.05] = np.nan
      t[rng.random(shape) < 0.05] = np.nan
    tc = dict(cs)
    if mask:
      tc['mask'] = (DIMS[1:], rng.random(shape[1:]) > 0.3)
    pred[v] = xr.DataArray(p, dims=DIMS, coords=cs, name=v)
    targ[v] = xr.DataArray(t, dims=DIMS, coords=tc, name=v)
  return pred, targ


def _ctb(thresholds=THR, which='both', dim='threshold', **kw):
  return wrappers.ContinuousToBinary(which, thresholds, dim, **kw)


# ---- eligibility ------------------------------------------------------------------------------------------------------------------
def test_plain_thresholds_on_both_sides_give_lazy_statistics():
  pred, targ = _inputs(variables=('u', 'v'))
  targ['only_targets'] = targ['v']
  for values in (THR, tuple(THR), np.array(THR), [1, 2.5, np.float32(0.5)], [3]):
    for cls, cell in ((categorical.TruePositives, 0), (categorical.FalsePositives, 1), (categorical.FalseNegatives, 2),
                      (categorical.TrueNegatives, 3)):
      out = cls().compute_with_transform(_ctb(values), pred, targ)
      assert set(out) == {'u', 'v'}
      for name, stat in out.items():
        assert isinstance(stat, lazy.LazyContingency) and stat.is_lazy and stat._cell == cell and stat.name == name  # pylint: disable=protected-access
        assert stat.dims == DIMS + ('threshold',) and stat.shape == (3, 8, 10, len(values))
  # through the public wrapper, and the four cells of a pair share one group
  stats = {c: wrappers.WrappedStatistic(cls(), _ctb()).compute(pred, targ)['v'] for c, cls in categorical._CELLS.items()}  # pylint: disable=protected-access
  assert len({id(s._group) for s in stats.values()}) == 1  # pylint: disable=protected-access
  other = wrappers.WrappedStatistic(categorical.TruePositives(), _ctb([1.0, 2.0])).compute(pred, targ)['v']
  assert other._group is not stats['tp']._group  # pylint: disable=protected-access
  # float64 payloads, targets on fewer dims than the predictions
  p64, t64 = _inputs(np.float64)
  t64 = {'v': t64['v'].isel(time=0, drop=True)}
  assert isinstance(categorical.TruePositives().compute_with_transform(_ctb(), p64, t64)['v'], lazy.LazyContingency)


def test_everything_else_keeps_the_unfused_route(monkeypatch):
  pred, targ = _inputs()
  tp = categorical.TruePositives()
  labelled = xr.DataArray(np.array(THR), dims=['threshold'], coords={'threshold': THR})
  not_eligible = [
      _ctb(which='predictions'), _ctb(which='targets'),                      # one side only
      _ctb(labelled, unique_name_suffix='x'),                                # labelled thresholds
      _ctb(xr.Dataset({'v': labelled}), unique_name_suffix='x'),
      _ctb(['1.0']), _ctb([True]), _ctb([1.0, 2.0j]), _ctb([2 ** 53 + 1]),   # not real numbers float64 holds exactly
      _ctb(iter(THR)),                                                       # not a plain sequence
      _ctb(dim='time'),                                                      # the dim exists on an input
      wrappers.ContinuousToBins('both', THR, 'threshold'),                   # another transform
  ]
  for transform in not_eligible:
    assert tp.compute_with_transform(transform, pred, targ) is None, transform

  class Mine(wrappers.ContinuousToBinary):  # a subclass may binarise differently
    pass
  assert tp.compute_with_transform(Mine('both', THR, 'threshold'), pred, targ) is None
  # targets with a dim the predictions lack; integer payloads
  tv = np.asarray(targ['v'].values)
  wide = {'v': xr.DataArray(np.stack([tv, tv]), dims=('level',) + DIMS, coords=dict(targ['v'].coords, level=[1, 2]), name='v')}
  assert tp.compute_with_transform(_ctb(), pred, wide) is None
  ints = {'v': xr.DataArray(np.asarray(pred['v'].values).astype(np.int32), dims=DIMS, coords=dict(pred['v'].coords), name='v')}
  assert tp.compute_with_transform(_ctb(), ints, targ) is None
  # predictions on fewer dims than the targets
  assert tp.compute_with_transform(_ctb(), {'v': pred['v'].isel(time=0, drop=True)}, targ) is None
  # the switch
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY', False)
  assert tp.compute_with_transform(_ctb(), pred, targ) is None
  # ... and whatever the route, the wrapper's answer is today's arithmetic
  out = wrappers.WrappedStatistic(tp, _ctb()).compute(pred, targ)['v']
  assert not isinstance(out, lazy.LazyContingency) and str(out.dtype) == 'float32'


def test_unique_names_do_not_change():
  stat = wrappers.WrappedStatistic(categorical.TruePositives(), _ctb([1e-3, 5e-3]))
  assert stat.unique_name == 'TruePositives_both_threshold=0.001,0.005'


# ---- the lazy statistic as a labelled array ---------------------------------------------------------------------------------------
def _unfused(cls, pred, targ, thresholds=THR):
  ctb = _ctb(thresholds)
  return cls().compute({k: ctb.transform_fn(v) for k, v in pred.items()}, {k: ctb.transform_fn(v) for k, v in targ.items()})


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_lazy_contingency_frame_values_and_pickle(dtype):
  pred, targ = _inputs(dtype, nans=True, mask=True)
  for cls in categorical._CELLS.values():  # pylint: disable=protected-access
    stat = wrappers.WrappedStatistic(cls(), _ctb()).compute(pred, targ)['v']
    want = _unfused(cls, pred, targ)['v']
    assert isinstance(stat, lazy.LazyContingency) and stat.is_lazy
    assert stat.dims == DIMS + ('threshold',) == tuple(want.dims)
    assert stat.shape == tuple(want.shape) and stat.dtype == np.float32 == want.dtype
    np.testing.assert_array_equal(np.asarray(stat.coords['threshold'].values), THR)
    for d in DIMS:
      np.testing.assert_array_equal(np.asarray(stat.coords[d].values), np.asarray(pred['v'].coords[d].values))
    assert tuple(stat.coords['mask'].dims) == DIMS[1:]
    np.testing.assert_array_equal(np.asarray(stat.coords['mask'].values), np.asarray(targ['v'].coords['mask'].values))
    assert stat.is_lazy  # (nothing so far read the payload)
    back = pickle.loads(pickle.dumps(stat))
    values = np.asarray(stat.values)
    assert values.dtype == np.float32 and not stat.is_lazy
    np.testing.assert_array_equal(values, np.asarray(want.values))
    assert np.isnan(values).any()
    assert tuple(back.dims) == stat.dims and str(back.dtype) == 'float32'
    np.testing.assert_array_equal(np.asarray(back.values), values)
    np.testing.assert_array_equal(np.asarray(back.coords['threshold'].values), THR)


# ---- host logic of the fused route, the launch stood in for -----------------------------------------------------------------------
def _run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=0, ens=None, cat=None, inputs=None, fold=None):
  """fake_device._run_s1 + kind 'cont': the lanes of wbx_contingency_partial from the float64 restatement."""
  if kind != 'cont':
    return fake_device._run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=func, ens=ens, cat=cat, inputs=inputs, fold=fold)  # pylint: disable=protected-access
  nthr, thr = cat
  thr = np.asarray(thr.ptr, np.float64)
  assert thr.shape == (nthr,) and nthr <= _hip.CONT_MAX_THRESHOLDS
  if engine.S1_EVENT_LOG is not None:
    engine.S1_EVENT_LOG.append({'kind': kind, 'flags': int(plan.flags), 'ms': 0.0, 'x_kept': plan.x_kept, 'nthr': nthr, 'vec': plan.vec})
  p = devs[0].ptr[fake_device._offsets(plan, 0)]  # pylint: disable=protected-access
  t = devs[1].ptr[fake_device._offsets(plan, 1)]  # pylint: disable=protected-access
  stat = CC.contingency_stat(p, t, thr)  # [key, depth, x, 4 * nthr]
  lanes = [stat[..., i] for i in range(stat.shape[-1])]
  valid = np.ones(lanes[0].shape, bool)
  if plan.flags & _hip.FLAG_MASKED:
    valid = devs[3].ptr[fake_device._offsets(plan, 3)] != 0  # pylint: disable=protected-access
  chunked = fake_device._chunked  # pylint: disable=protected-access
  with np.errstate(all='ignore'):
    if plan.flags & _hip.FLAG_SKIPNA:
      oks = [valid & ~np.isnan(l) for l in lanes]
      cols = [chunked(plan, np.where(ok, l, 0.0)) for ok, l in zip(oks, lanes)] + [chunked(plan, ok.astype(np.float64)) for ok in oks]
    elif plan.flags & _hip.FLAG_MASKED:
      cols = [chunked(plan, np.where(valid, l, 0.0)) for l in lanes] + [chunked(plan, valid.astype(np.float64))]
    else:
      cols = [chunked(plan, l) for l in lanes]
  partial = np.stack(cols, axis=2)
  assert partial.shape[2] == nlanes_total
  return fake_device._Buf(partial.reshape(plan.partial_shape(nlanes_total)))  # pylint: disable=protected-access


@pytest.fixture
def fused(monkeypatch):
  """The emulated backend with the contingency launch available: what a device context whose library exports the symbol gives."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(engine, '_run_s1', _run_s1)
  monkeypatch.setattr(engine, 'contingency_available', lambda ctx: True)
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  yield monkeypatch
  engine.clear_caches()


METRICS = lambda thresholds=THR: {  # pylint: disable=unnecessary-lambda-assignment
    name: wrappers.WrappedMetric(m, [wrappers.ContinuousToBinary('both', thresholds, 'threshold')])
    for name, m in (('csi', categorical.CSI()), ('ets', categorical.ETS()), ('bias', categorical.FrequencyBias()), ('sedi', categorical.SEDI()))}


def _evaluate(metrics, pred, targ, aggregator):
  stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  state = aggregator.aggregate_statistics(stats)
  return stats, state, state.metric_values(metrics)


def _launches(kind='cont'):
  return [e for e in engine.S1_EVENT_LOG if e['kind'] == kind]


def _assert_same_coords(x, y, what):
  """The full coordinate set: names, dims and values (a surviving `mask` among them)."""
  assert set(x.coords) == set(y.coords), (what, sorted(map(str, x.coords)), sorted(map(str, y.coords)))
  for name in x.coords:
    assert tuple(x.coords[name].dims) == tuple(y.coords[name].dims), (what, name)
    np.testing.assert_array_equal(np.asarray(x.coords[name].values), np.asarray(y.coords[name].values), err_msg=f'{what}: coordinate {name}')


def _assert_states_equal(a, b, rtol=0.0):
  assert set(a.sum_weighted_statistics) == set(b.sum_weighted_statistics)
  for table_a, table_b in ((a.sum_weighted_statistics, b.sum_weighted_statistics), (a.sum_weights, b.sum_weights)):
    for stat in table_a:
      assert set(table_a[stat]) == set(table_b[stat])
      for var in table_a[stat]:
        x, y = table_a[stat][var], table_b[stat][var]
        assert tuple(x.dims) == tuple(y.dims), (stat, var, x.dims, y.dims)
        _assert_same_coords(x, y, f'{stat} {var}')
        np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=rtol, atol=0, err_msg=f'{stat} {var}')


AGGREGATORS = {
    'plain': lambda: aggregation.Aggregator(reduce_dims=['time', 'latitude', 'longitude']),
    'keep-latitude': lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude']),
    'area': lambda: aggregation.Aggregator(reduce_dims=['time', 'latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()]),
    'masked': lambda: aggregation.Aggregator(reduce_dims=['time', 'latitude', 'longitude'], masked=True),
    'skipna': lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude'], skipna=True),
    # (LatitudeBins broadcasts its mask to every dim the statistic has: W is built on the frame without the threshold dim)
    'latitude-bins+masked': lambda: aggregation.Aggregator(reduce_dims=['time', 'latitude', 'longitude'], bin_by=[binning.LatitudeBins(30)],
                                                         masked=True),
    'masked+skipna+area': lambda: aggregation.Aggregator(reduce_dims=['time', 'latitude', 'longitude'], masked=True, skipna=True,
                                                       weigh_by=[weighting.GridAreaWeighting()]),
}


@pytest.mark.parametrize('which', list(AGGREGATORS))
def test_four_cells_one_launch_and_the_host_routes_numbers(fused, which):
  nans = 'skipna' in which
  pred, targ = _inputs(nans=nans, mask='masked' in which, variables=('u', 'v'))
  metrics = METRICS()
  stats, state, values = _evaluate(metrics, pred, targ, AGGREGATORS[which]())
  assert all(isinstance(s, lazy.LazyContingency) and s.is_lazy for per_var in stats.values() for s in per_var.values())
  assert len(stats) == 4  # TP, FP, FN, TN behind the one transform
  assert len(_launches()) == 2, engine.S1_EVENT_LOG  # one per variable: the four cells are lane blocks of it
  assert not _launches('det')
  # a second aggregator launches once per variable again; the first one's sums are not reused for it
  _evaluate(metrics, pred, targ, AGGREGATORS['keep-latitude' if which != 'keep-latitude' else 'plain']())
  assert len(_launches()) == 4
  # the same evaluation on the host route
  fused.setattr(lazy, 'FUSED_CONTINGENCY', False)
  fused.setattr(engine, 'S1_EVENT_LOG', [])
  stats0, state0, values0 = _evaluate(metrics, pred, targ, AGGREGATORS[which]())
  assert not any(isinstance(s, lazy.LazyContingency) for per_var in stats0.values() for s in per_var.values())
  assert not _launches() and len(_launches('det')) == 8  # four materialised statistics x two variables
  # sums of 0 / 1 (times area weights): equal to summation-order round-off, exactly equal without weights; the scores are
  # differences and ratios of those sums, of order one: an absolute 1e-11 where a score cancels to ~0
  _assert_states_equal(state, state0, rtol=1e-12 if 'area' in which else 0.0)
  assert set(values) == set(values0)
  for key in values:
    np.testing.assert_allclose(np.asarray(values[key].values), np.asarray(values0[key].values), rtol=1e-11, atol=1e-11, equal_nan=True, err_msg=key)
    assert 'threshold' in values[key].dims
    np.testing.assert_array_equal(np.asarray(values[key].coords['threshold'].values), THR)


@pytest.mark.parametrize('masked', [True, False], ids=['masked', 'unmasked'])
def test_a_mask_whose_dims_survive_stays_on_the_results_like_on_the_host_route(fused, masked):
  """reduce_dims = ['time'] with a target mask on (latitude, longitude): the sums, the weights and the metric values carry the
  `mask` coordinate exactly as the host route's do, whether or not the aggregator applies it."""
  pred, targ = _inputs(mask=True)
  metrics = METRICS()
  make = lambda: aggregation.Aggregator(reduce_dims=['time'], masked=masked)
  _, state, values = _evaluate(metrics, pred, targ, make())
  assert len(_launches()) == 1 and not _launches('det')
  fused.setattr(lazy, 'FUSED_CONTINGENCY', False)
  fused.setattr(engine, 'S1_EVENT_LOG', [])
  _, state0, values0 = _evaluate(metrics, pred, targ, make())
  assert not _launches() and _launches('det')
  _assert_states_equal(state, state0)
  want_mask = np.asarray(targ['v'].coords['mask'].values)
  for tree in (state.sum_weighted_statistics, state.sum_weights):
    for stat in tree:
      got = tree[stat]['v']
      assert set(got.coords) == {'latitude', 'longitude', 'mask', 'threshold'}, (stat, sorted(got.coords))
      assert tuple(got.coords['mask'].dims) == DIMS[1:]
      np.testing.assert_array_equal(np.asarray(got.coords['mask'].values), want_mask)
  assert set(values) == set(values0)
  for key in values:
    assert tuple(values[key].dims) == tuple(values0[key].dims)
    _assert_same_coords(values[key], values0[key], key)
    assert 'mask' in values[key].coords
    np.testing.assert_allclose(np.asarray(values[key].values), np.asarray(values0[key].values), rtol=1e-11, atol=1e-11, equal_nan=True, err_msg=key)


def test_lane_blocks_are_the_cells(fused):
  """Each statistic gets ITS block of the launch: against whole-array NumPy, cell by cell and threshold by threshold."""
  del fused
  pred, targ = _inputs()
  metrics = {'acc': wrappers.WrappedMetric(categorical.Accuracy(), [_ctb()])}
  _, state, _ = _evaluate(metrics, pred, targ, AGGREGATORS['plain']())
  p, t = np.asarray(pred['v'].values, np.float64), np.asarray(targ['v'].values, np.float64)
  suffix = 'both_threshold=' + ','.join(str(x) for x in THR)
  for cell, name in enumerate(('TruePositives', 'FalsePositives', 'FalseNegatives', 'TrueNegatives')):
    got = state.sum_weighted_statistics[f'{name}_{suffix}']['v']
    assert tuple(got.dims) == ('threshold',)
    for k, thr in enumerate(THR):
      P, O = p > thr, t > thr
      want = [(P & O), (P & ~O), (~P & O), (~P & ~O)][cell].sum()
      assert float(np.asarray(got.values)[k]) == float(want), (name, thr)
    np.testing.assert_array_equal(np.asarray(state.sum_weights[f'{name}_{suffix}']['v'].values), np.full(len(THR), float(p.size)))


def test_more_thresholds_than_a_launch_takes(fused):
  nthr = _hip.CONT_MAX_THRESHOLDS + 3
  thresholds = list(np.round(np.random.default_rng(3).gamma(2.0, size=nthr), 3))  # unsorted
  pred, targ = _inputs(nans=True)
  metrics = METRICS(thresholds)
  agg = lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude'], skipna=True, weigh_by=[weighting.GridAreaWeighting()])
  _, state, values = _evaluate(metrics, pred, targ, agg())
  launches = _launches()
  assert [e['nthr'] for e in launches] == [_hip.CONT_MAX_THRESHOLDS, 3]  # two blocks for the one variable, in order
  fused.setattr(lazy, 'FUSED_CONTINGENCY', False)
  _, state0, values0 = _evaluate(metrics, pred, targ, agg())
  _assert_states_equal(state, state0, rtol=1e-12)
  for key in values:
    np.testing.assert_array_equal(np.asarray(values[key].coords['threshold'].values), thresholds)
    np.testing.assert_allclose(np.asarray(values[key].values), np.asarray(values0[key].values), rtol=1e-11, atol=1e-11, equal_nan=True)


def test_more_thresholds_than_a_launch_takes_with_an_empty_kept_dim(fused):
  """The blocks are joined by their sizes, not by what is left over: a kept dim of length 0 leaves nothing over."""
  nthr = _hip.CONT_MAX_THRESHOLDS + 3
  thresholds = list(np.round(np.random.default_rng(3).gamma(2.0, size=nthr), 3))
  pred, targ = _inputs(shape=(3, 0, 10))
  agg = lambda: aggregation.Aggregator(reduce_dims=['time', 'longitude'])
  _, state, values = _evaluate(METRICS(thresholds), pred, targ, agg())
  assert [e['nthr'] for e in _launches()] == [_hip.CONT_MAX_THRESHOLDS, 3]
  fused.setattr(lazy, 'FUSED_CONTINGENCY', False)
  _, state0, values0 = _evaluate(METRICS(thresholds), pred, targ, agg())
  _assert_states_equal(state, state0)
  assert values and set(values) == set(values0)
  for key in values:
    assert values[key].shape == values0[key].shape and 0 in values[key].shape and nthr in values[key].shape, (key, values[key].shape)


def test_threshold_dim_reduced_or_weighted_takes_the_host_route(fused):
  pred, targ = _inputs()
  metrics = METRICS()
  agg = lambda: aggregation.Aggregator(reduce_dims=['time', 'latitude', 'longitude', 'threshold'])
  stats, state, _ = _evaluate(metrics, pred, targ, agg())
  assert all(isinstance(s, lazy.LazyContingency) for per_var in stats.values() for s in per_var.values())
  assert not _launches() and len(_launches('det')) == 4  # the four cells, each materialised and reduced
  fused.setattr(lazy, 'FUSED_CONTINGENCY', False)
  _, state0, _ = _evaluate(metrics, pred, targ, agg())
  _assert_states_equal(state, state0)


def test_a_context_without_the_library_keeps_the_host_route(monkeypatch):
  """The gate as shipped: the plan interpreter's context is no _hip.Context, so nothing asks it for the new launch."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  assert not engine.contingency_available(_hip.default_context())
  assert not engine.contingency_available(object())
  pred, targ = _inputs()
  log = []
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', log)
  stats, _, values = _evaluate(METRICS(), pred, targ, AGGREGATORS['plain']())
  assert all(isinstance(s, lazy.LazyContingency) for per_var in stats.values() for s in per_var.values())
  assert log and all(e['kind'] == 'det' for e in log)
  p, t = np.asarray(pred['v'].values), np.asarray(targ['v'].values)
  for k, thr in enumerate(THR):
    P, O = p > thr, t > thr
    tp, fp, fn = (P & O).sum(), (P & ~O).sum(), (~P & O).sum()
    np.testing.assert_allclose(float(np.asarray(values['csi.v'].values)[k]), tp / (tp + fp + fn), rtol=1e-12)
