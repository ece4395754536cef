"""Contingency tables at threshold fields without a device: the restatement of tests/contingency_field_cases.py against the host
route, against values worked by hand and against the mutants its cases must tell apart; the gate of categorical._Indicator decline by
decline; the lazy statistic through the Aggregator with the launch stood in for by the restatement; the ABI pins."""
import os
import re

import numpy as np
import pytest

import contingency_cases as CC
import contingency_field_cases as FC
import fake_device
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import categorical
from weatherbenchx_amd.metrics import wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'wbx_contingency_field_partial'
PAIRS = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]
DIMS = ('lead_time', 'latitude', 'longitude')
CELLS = (categorical.TruePositives, categorical.FalsePositives, categorical.FalseNegatives, categorical.TrueNegatives)


# ---- the ABI pins --------------------------------------------------------------------------------------------------------------------
def test_the_entry_joins_abi_13():
  header = open(os.path.join(ROOT, 'include', 'wbx.h')).read()
  assert int(re.search(r'#define\s+WBX_ABI_VERSION\s+(\d+)', header).group(1)) == 13
  assert NAME in _hip.EXPORTED_SYMBOLS
  decl = re.search(NAME + r'\(([^;]*)\);', header).group(1)
  assert len(re.sub(r'/\*.*?\*/', '', decl).split(',')) == 12 <= _hip.CALL_MAX_ARGS
  if os.path.exists(os.path.join(ROOT, 'weatherbenchx_amd', 'libwbx_hip.so')):
    assert len(_hip.load_library() and _hip.PROTOS[NAME]) == 12
  row = engine._KINDS['cont']  # pylint: disable=protected-access  (the field is the row's second arm: a `cat` tuple without a table)
  assert row.own_dtype2 and row.keep2 and row.vec4 and lazy._LAZY_KINDS['cont'].third == 'optional'  # pylint: disable=protected-access
  field_args = engine.ContFieldArgs(_hip.F64, 3, 35, 2)
  assert row.call(['p', 't', 'c', 'm'], 'out', _hip.F32, 0, None, field_args) == (NAME, (_hip.F32, _hip.F64, 3, 35, 2, 'p', 't', 'c', 'm', 'out'))
  assert row.call(['p', 't', None, 'm'], 'out', _hip.F32, 0, None, engine.ContArgs(3, type('Buf', (), {'ptr': 64})()))[0] == 'wbx_contingency_partial'


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _labelled(case, varies, labelled_thr=True):
  nlead, nrow, nx = case.p.shape
  cs = {'lead_time': np.arange(nlead), 'latitude': np.linspace(-40, 40, nrow), 'longitude': np.arange(nx) * 1.5}
  p = xr.DataArray(np.ascontiguousarray(case.p), dims=DIMS, coords=cs, name='v')
  t = xr.DataArray(np.ascontiguousarray(case.t), dims=DIMS, coords=cs, name='v')
  fdims = {'row_x': DIMS[1:], 'x': DIMS[2:], 'row': DIMS[1:2], 'lead_row_x': DIMS}[varies]
  thr = case.thresholds()  # [lead, row, x, K]
  take = tuple(slice(None) if d in fdims else 0 for d in DIMS)
  values = np.ascontiguousarray(np.moveaxis(thr[take], -1, 0))
  fcs = {d: cs[d] for d in fdims}
  if labelled_thr:
    fcs['threshold'] = np.arange(case.size) * 10
  field = xr.DataArray(values, dims=('threshold',) + fdims, coords=fcs, name='v')
  return p, t, field


@pytest.mark.parametrize('varies', FC.VARIES)
@pytest.mark.parametrize('pair', PAIRS, ids=[f'{np.dtype(d).name}-{np.dtype(c).name}' for d, c in PAIRS])
def test_restatement_equals_the_host_route_bit_for_bit(pair, varies):
  case = FC.field_case(11, 5, 2, 5, 9, pair[0], pair[1], 0, varies)
  p, t, field = _labelled(case, varies)
  _, stat = FC.expected(case, 0, 5, False)
  with np.errstate(invalid='ignore'):
    pb = wrappers.binarize_thresholds(p, field, 'threshold')
    tb = wrappers.binarize_thresholds(t, field, 'threshold')
    for cell, cls in enumerate(CELLS):
      host = categorical._indicator(pb, tb, cls._predicted, cls._observed).transpose(*DIMS, 'threshold')  # pylint: disable=protected-access
      mine = stat[..., cell * case.size:(cell + 1) * case.size]
      np.testing.assert_array_equal(np.asarray(host.values, np.float64), mine)
      np.testing.assert_array_equal(np.nansum(np.asarray(host.values, np.float64), axis=(0, 1, 2)), np.nansum(mine, axis=(0, 1, 2)))
  assert np.isnan(stat).any() and np.isfinite(stat).mean() > 0.9


def test_restatement_equals_values_worked_by_hand():
  tenth32, below = CC.F32_TENTH, CC.F32_BELOW_TENTH
  p = np.array([tenth32, tenth32, 0.25, -0.0, np.inf, 1.0, np.nan, below], np.float32)
  t = np.array([below, tenth32, 0.25, 0.5, 1.0, 2.0, 0.0, -np.inf], np.float32)
  thr = np.array([0.1, FC.F64_ABOVE_F32_TENTH, 0.25, 0.0, np.nan, np.inf, 0.0, -np.inf])[:, None]
  stat = FC.field_stat(p, t, thr)
  nan = np.nan
  # TP, FP, FN, TN
  want = np.array([[0, 1, 0, 0],   # float32(0.1) > 0.1 > its lower neighbour
                   [0, 0, 0, 1],   # neither exceeds the float64 just above float32(0.1)
                   [0, 0, 0, 1],   # ties: strict
                   [0, 0, 1, 0],   # -0.0 > 0.0 is false, 0.5 > 0.0
                   [0, 0, 0, 1],   # a NaN threshold: false on both sides, the point counts
                   [0, 0, 0, 1],   # nothing exceeds +inf
                   [nan] * 4,      # a NaN p
                   [0, 1, 0, 0]])  # every number exceeds -inf but -inf itself
  np.testing.assert_array_equal(stat, want)
  # float32 thresholds: the tie float32(0.1) > float32(0.1) is false; float64 data against them widen exactly
  np.testing.assert_array_equal(FC.field_stat(p[:1], t[:1], np.array([[tenth32]], np.float32)), [[0, 0, 0, 1]])
  np.testing.assert_array_equal(FC.field_stat(np.array([0.1]), np.array([0.2]), np.array([[tenth32]], np.float32)), [[0, 0, 1, 0]])


def _round_to_nearest_gt(x, thr):
  if x.dtype == np.float32 and thr.dtype == np.float64:
    with np.errstate(over='ignore', invalid='ignore'):
      return x[..., None] > thr.astype(np.float32)
  return FC.promoted_gt(x, thr)


def _ge(x, thr):
  rt = np.result_type(x.dtype, thr.dtype)
  with np.errstate(invalid='ignore'):
    return x.astype(rt)[..., None] >= thr.astype(rt)


MUTANTS = {
    'round to nearest': dict(gt=_round_to_nearest_gt), '>= for >': dict(gt=_ge), 'a NaN threshold is a NaN point': dict(nan_thr_is_nan=True),
    'no x stride': dict(ignore=('x',)), 'no thr_stride': dict(ignore=('thr',)), 'no depth offset': dict(ignore=('row',)),
}


@pytest.mark.parametrize('mutant', list(MUTANTS) + ['no thr_first'])
def test_the_cases_see_the_mutants(mutant):
  """Every mutant changes a partial of the cases the GPU tests run: x summed and kept, a float32 frame at a float64 field."""
  for varies in FC.VARIES:
    if (mutant == 'no x stride' and varies == 'row') or (mutant == 'no depth offset' and varies == 'x'):
      continue  # (the field has no such stride)
    for x_kept in (False, True):
      for inner in (False, True):
        case = FC.field_case(5, 3, 2, 5, 65, np.float32, np.float64, FC.FLAG_SKIPNA, varies, inner)
        want, _ = FC.expected(case, FC.FLAG_SKIPNA, 2, x_kept, first=1, nthr=2)
        if mutant == 'no thr_first':
          got, _ = FC.expected(case, FC.FLAG_SKIPNA, 2, x_kept, first=0, nthr=2)
        else:
          got, _ = FC.expected(case, FC.FLAG_SKIPNA, 2, x_kept, first=1, nthr=2, **MUTANTS[mutant])
        if mutant in ('round to nearest', '>= for >', 'a NaN threshold is a NaN point'):  # (the fixed points carry them)
          want, _ = FC.expected(case, FC.FLAG_SKIPNA, 2, x_kept)
          got, _ = FC.expected(case, FC.FLAG_SKIPNA, 2, x_kept, **MUTANTS[mutant])
        assert not np.array_equal(got, want), (mutant, varies, x_kept, inner)


# ---- the gate ------------------------------------------------------------------------------------------------------------------------
def _frame(dtype=np.float32, nlat=4, nlon=6, seed=0):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(3), 'latitude': np.linspace(-30, 30, nlat), 'longitude': np.arange(nlon) * 2.0}
  mk = lambda: xr.DataArray(np.round(rng.normal(size=(3, nlat, nlon)) * 4).astype(dtype) / 4, dims=('time', 'latitude', 'longitude'), coords=cs,
                            name='v')
  return mk(), mk()


def _field(k=3, dtype=np.float64, dims=('threshold', 'latitude', 'longitude'), nlat=4, nlon=6, seed=1, **coords):
  rng = np.random.default_rng(seed)
  sizes = {'threshold': k, 'latitude': nlat, 'longitude': nlon, 'time': 3, 'level': 2}
  cs = {'latitude': np.linspace(-30, 30, nlat), 'longitude': np.arange(nlon) * 2.0, 'time': np.arange(3), 'level': np.arange(2)}
  cs = {d: cs[d] for d in dims if d in cs}
  cs.update(coords)
  return xr.DataArray((np.round(rng.normal(size=[sizes[d] for d in dims]) * 4) / 4).astype(dtype), dims=dims, coords=cs, name='v')


def test_the_gate_decline_by_decline():
  p, t = _frame()
  route = lambda field, pp=p, tt=t, dim='threshold': categorical.contingency_field_route(pp, tt, field, dim)
  assert route(_field()) == ('fused', None)
  assert route(_field(dtype=np.float32)) == ('fused', None)
  assert route(_field(dims=('latitude', 'threshold', 'longitude'))) == ('fused', None)
  assert route(_field(dims=('threshold', 'longitude'))) == ('fused', None)
  assert route(_field(threshold=np.array([90, 95, 99]))) == ('fused', None)
  assert route(_field(dims=('threshold', 'time', 'latitude', 'longitude'))) == ('fused', None)
  declined = {
      'a labelled list': _field(dims=('threshold',)),
      'without the threshold dim': _field(dims=('latitude', 'longitude')),
      'not a dim of both inputs': _field(dims=('threshold', 'level', 'latitude', 'longitude')),
      'labels of': _field(latitude=np.linspace(-30, 30, 4)[::-1].copy()),
      'dtypes': _field(dtype=np.float16),
      'beyond those of its own dims': _field(height=((), np.float64(2.0))),
  }
  for why, field in declined.items():
    how, reason = route(field)
    assert how == 'host' and why in reason, (why, reason)
  assert route(_field(latitude=np.linspace(-30, 30, 4) + 1e-9))[0] == 'host'  # labels that differ keep the host route
  assert route(_field(nlat=5))[0] == 'host'  # another length
  assert route(_field(), dim='latitude')[0] == 'host'  # the threshold dim on the inputs
  assert route([0.5])[0] == 'host'
  # a field dim that the targets lack
  how, reason = route(_field(dims=('threshold', 'time', 'latitude', 'longitude')), tt=t.isel(time=0, drop=True))
  assert how == 'host' and 'not a dim of both inputs' in reason
  # other dtypes of the inputs
  assert route(_field(), pp=p.astype(np.float16))[0] == 'host'
  # unlabelled on one side only
  bare = xr.DataArray(np.asarray(_field().values), dims=('threshold', 'latitude', 'longitude'), name='v')
  assert route(bare)[0] == 'host'


def _stats(monkeypatch, transform, p, t, fused=True, available=True):
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY_FIELD', fused)
  monkeypatch.setattr(engine, 'contingency_field_available', lambda ctx: available)
  metric = wrappers.WrappedMetric(categorical.CSI(), [transform])
  return metrics_base.compute_unique_statistics_for_all_metrics({'csi': metric}, {'v': p}, {'v': t})


def _is_fused(stats):
  kinds = {(type(s), getattr(getattr(s, '_group', None), 'kind', None)) for per_var in stats.values() for s in per_var.values()}
  assert len(kinds) == 1
  return kinds == {(lazy.LazyContingencyField, 'cont')}


def test_the_statistic_follows_the_gate_and_the_switches(monkeypatch):
  engine.clear_caches()
  fake_device.install(monkeypatch)
  p, t = _frame()
  binary = lambda field, which='both': wrappers.ContinuousToBinary(which, field, 'threshold', unique_name_suffix='f')
  stats = _stats(monkeypatch, binary(_field()), p, t)
  assert _is_fused(stats)
  for per_var in stats.values():
    for s in per_var.values():
      assert isinstance(s, lazy.LazyContingency) and s.is_lazy and s.dims == p.dims + ('threshold',) and s.name == 'v'
      assert s._group is next(iter(next(iter(stats.values())).values()))._group  # pylint: disable=protected-access  (one group: one launch)
  assert _is_fused(_stats(monkeypatch, binary(xr.Dataset({'v': _field()})), p, t))
  # declines: every one of them computes on the host route, with the host route's outcome
  assert not _is_fused(_stats(monkeypatch, binary(_field()), p, t, fused=False))
  assert not _is_fused(_stats(monkeypatch, binary(_field()), p, t, available=False))
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY', False)
  assert not _is_fused(_stats(monkeypatch, binary(_field()), p, t))
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY', True)
  assert not _is_fused(_stats(monkeypatch, binary(_field(dims=('threshold',))), p, t))  # the 1-D labelled array
  assert not _is_fused(_stats(monkeypatch, binary(_field(latitude=np.linspace(-30, 30, 4)[::-1].copy())), p, t))
  assert not _is_fused(_stats(monkeypatch, binary(_field(), 'predictions'), p, t))
  assert not _is_fused(_stats(monkeypatch, binary(_field(dims=('threshold', 'time', 'latitude', 'longitude'))), p, t.isel(time=0, drop=True)))
  unnamed = xr.DataArray(np.asarray(p.values), dims=p.dims, coords={d: p.coords[d].values for d in p.dims})
  with pytest.raises(ValueError):  # an array without a name against a Dataset: the host route's assertion as well
    _stats(monkeypatch, binary(xr.Dataset({'v': _field()})), unnamed, t)
  assert _is_fused(_stats(monkeypatch, binary(_field()), unnamed, t))  # (a DataArray of thresholds asks for no name)
  with pytest.raises(ValueError) as err:  # (the host route's assertion, raised by the host route)
    _stats(monkeypatch, binary(xr.Dataset({'w': _field()})), p, t)
  assert isinstance(err.value.__cause__, AssertionError) and 'not found in thresholds' in str(err.value.__cause__)

  class Mine(wrappers.ContinuousToBinary):
    pass
  assert not _is_fused(_stats(monkeypatch, Mine('both', _field(), 'threshold', unique_name_suffix='f'), p, t))
  from weatherbenchx_amd import climatology_cache  # pylint: disable=g-import-not-at-top
  pooled = _field()
  monkeypatch.setattr(climatology_cache, 'cache_for', lambda f: object() if f is pooled else None)
  assert not _is_fused(_stats(monkeypatch, binary(pooled), p, t))
  engine.clear_caches()


def test_a_threshold_dim_without_a_stride_is_never_stepped_along():
  """A threshold dim of length 1 may have stride 0; a longer one that is a broadcast view is refused by the operands (the kernel
  would refuse thr_stride == 0 with nthr > 1) and by the statistic, whose caller then keeps the host route."""
  dev = lambda strides: [None, None, engine._Dev(0, engine.planner.InputLayout(strides=strides, itemsize=8), _hip.F64, None, 0), None]  # pylint: disable=protected-access
  cat = lambda size, **kw: dict({'threshold_dim': 'threshold', 'nthr': size, 'thr_first': 0, 'size': size}, **kw)
  assert engine._contf_operands(None, dev({'threshold': 0, 'x': 1}), 0, None, cat(1), None)[2].thr_stride == 1  # pylint: disable=protected-access
  assert engine._contf_operands(None, dev({'threshold': 7, 'x': 1}), 0, None, cat(3), None)[2] == engine.ContFieldArgs(_hip.F64, 3, 7, 0)  # pylint: disable=protected-access
  with pytest.raises(ValueError, match='stride 0'):
    engine._contf_operands(None, dev({'threshold': 0, 'x': 1}), 0, None, cat(3), None)  # pylint: disable=protected-access
  with pytest.raises(ValueError, match='not all on the field'):
    engine._contf_operands(None, dev({'threshold': 7, 'x': 1}), 0, None, cat(3, thr_first=1), None)  # pylint: disable=protected-access


# ---- host logic of the fused route, the launch stood in for -----------------------------------------------------------------------
def _run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=0, ens=None, cat=None, inputs=None, fold=None):
  """fake_device._run_s1 + kind 'cont' at a field: the partials of wbx_contingency_field_partial from the restatement, the thresholds read
  through the plan's addressing of input 2 and the launch's thr_stride / thr_first."""
  if kind != 'cont' or not isinstance(cat, engine.ContFieldArgs):
    return fake_device._run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=func, ens=ens, cat=cat, inputs=inputs, fold=fold)  # pylint: disable=protected-access
  thr_dtype, nthr, thr_stride, thr_first = cat
  assert devs[2].dtype_code == thr_dtype and devs[2].ptr.dtype == (np.float32 if thr_dtype == _hip.F32 else np.float64)
  assert devs[0].ptr.dtype == devs[1].ptr.dtype == (np.float32 if dtype_code == _hip.F32 else np.float64)
  assert plan.plane_rows == 0 and plan.x_weights is None and 1 <= nthr <= 16 and thr_first >= 0 and (thr_stride != 0 or nthr == 1)
  engine.S1_EVENT_LOG.append({'kind': 'cont at a field', 'flags': int(plan.flags), 'ms': 0.0, 'nthr': nthr, 'thr_first': thr_first, 'gather': plan.gather_tab is not None})
  p, t = devs[0].ptr[fake_device._offsets(plan, 0)], devs[1].ptr[fake_device._offsets(plan, 1)]  # pylint: disable=protected-access
  at = fake_device._offsets(plan, 2)[..., None] + (thr_first + np.arange(nthr)) * thr_stride  # pylint: disable=protected-access
  stat = FC.field_stat(p, t, devs[2].ptr[at])
  valid = devs[3].ptr[fake_device._offsets(plan, 3)] != 0 if plan.flags & _hip.FLAG_MASKED else np.ones(p.shape, bool)  # pylint: disable=protected-access
  chunked = fake_device._chunked  # pylint: disable=protected-access
  lanes = [stat[..., k] for k in range(stat.shape[-1])]
  if plan.flags & _hip.FLAG_SKIPNA:
    oks = [valid & ~np.isnan(l) for l in lanes]
    cols = [chunked(plan, np.where(ok, l, 0.0)) for ok, l in zip(oks, lanes)] + [chunked(plan, ok.astype(np.float64)) for ok in oks]
  elif plan.flags & _hip.FLAG_MASKED:
    cols = [chunked(plan, np.where(valid, l, 0.0)) for l in lanes] + [chunked(plan, valid.astype(np.float64))]
  else:
    cols = [chunked(plan, l) for l in lanes]
  return fake_device._Buf(np.stack(cols, axis=2).reshape(plan.partial_shape(nlanes_total)))  # pylint: disable=protected-access


@pytest.mark.parametrize('thr_dtype', [np.float32, np.float64], ids=['thr32', 'thr64'])
@pytest.mark.parametrize('which', ['plain', 'keep-times', 'masked', 'skipna', 'twenty'])
def test_through_the_aggregator_the_host_routes_numbers_bit_for_bit(monkeypatch, which, thr_dtype):
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(engine, '_run_s1', _run_s1)
  p, t = _frame()
  if which == 'skipna':
    p.values[1, 2, 3] = t.values[0, 1, 1] = np.nan
  if which == 'masked':
    t = xr.DataArray(np.asarray(t.values), dims=t.dims, coords=dict({d: t.coords[d].values for d in t.dims},
                                                                   mask=(t.dims[1:], np.random.default_rng(0).random(t.shape[1:]) > 0.3)), name='v')
  k = 20 if which == 'twenty' else 3
  field = _field(k=k, dtype=thr_dtype, threshold=np.arange(k) + 80)
  field.values[0, 0, 0] = np.nan
  reduce_dims = ['latitude', 'longitude'] if which == 'keep-times' else list(t.dims)
  metric = lambda: {'csi': wrappers.WrappedMetric(categorical.CSI(), [wrappers.ContinuousToBinary('both', xr.Dataset({'v': field}), 'threshold',
                                                                                                  unique_name_suffix='f')])}
  results = {}
  for fused in (True, False):
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    stats = _stats(monkeypatch, wrappers.ContinuousToBinary('both', xr.Dataset({'v': field}), 'threshold', unique_name_suffix='f'), p, t, fused=fused)
    assert _is_fused(stats) == fused
    monkeypatch.setattr(lazy.LazyContingencyField, 'launchable', staticmethod(lambda: fused))
    state = aggregation.Aggregator(reduce_dims=reduce_dims, masked=which == 'masked', skipna=which == 'skipna').aggregate_statistics(stats)
    launches = [e for e in engine.S1_EVENT_LOG if e['kind'] == 'cont at a field']
    if fused:  # the four cells share the launches: one per block of 16 thresholds, each advancing thr_first
      assert [(e['thr_first'], e['nthr']) for e in launches] == ([(0, 16), (16, 4)] if k == 20 else [(0, 3)]) and not launches[0]['gather']
      assert len(engine.S1_EVENT_LOG) == len(launches)
    else:
      assert not launches
    results[fused] = (state, state.metric_values(metric()))
  (state, values), (state0, values0) = results[True], results[False]
  for name in state0.sum_weighted_statistics:
    x, y = state.sum_weighted_statistics[name]['v'], state0.sum_weighted_statistics[name]['v']
    assert tuple(x.dims) == tuple(y.dims) and set(x.coords) == set(y.coords)
    np.testing.assert_array_equal(np.asarray(x.coords['threshold'].values), np.arange(k) + 80)
    np.testing.assert_array_equal(np.asarray(x.values), np.asarray(y.values, np.float64))
    np.testing.assert_array_equal(np.asarray(state.sum_weights[name]['v'].values), np.asarray(state0.sum_weights[name]['v'].values))
    assert np.isfinite(np.asarray(x.values)).any()
  assert tuple(values['csi.v'].dims) == tuple(values0['csi.v'].dims)
  np.testing.assert_array_equal(np.asarray(values['csi.v'].values), np.asarray(values0['csi.v'].values))
  engine.clear_caches()


def test_values_of_the_lazy_statistic_are_the_host_routes(monkeypatch):
  engine.clear_caches()
  fake_device.install(monkeypatch)
  p, t = _frame()
  p.values[0, 0, 0] = np.nan
  field = _field(dims=('latitude', 'threshold', 'longitude'))  # (the threshold dim in the middle of the field)
  transform = wrappers.ContinuousToBinary('both', field, 'threshold', unique_name_suffix='f')
  fused = _stats(monkeypatch, transform, p, t)
  host = _stats(monkeypatch, transform, p, t, fused=False)
  assert _is_fused(fused) and not _is_fused(host)
  for name in host:
    a, b = fused[name]['v'], host[name]['v']
    assert a.dims == b.dims and a.dtype == b.dtype and set(a.coords) == set(b.coords) and a.name == b.name and a.shape == b.shape
    np.testing.assert_array_equal(np.asarray(a.values), np.asarray(b.values))
  engine.clear_caches()
