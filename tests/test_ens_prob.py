"""The fused contingency tables of ensemble event probabilities (wbx_ens_prob_contingency_partial) without a device: the entry
point's export and argument checks, the integer restatement of tests/ens_prob_cases.py against the host route's float32 indicators
bit for bit, the slot tables at the edges of float32 and float64, the gate of `_Indicator.compute_with_chain`, the lazy statistic
as a labelled array, and the host logic of the fused route (one launch per block of pairs for the four cells, the blocks joined
cell by cell) through the Aggregator with the launch itself stood in for by the restatement."""
import os
import re

import numpy as np
import pytest

import ens_prob_cases as EP
import fake_device
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import binning
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import weighting
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import categorical
from weatherbenchx_amd.metrics import multivariate
from weatherbenchx_amd.metrics import wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = ('time', 'latitude', 'longitude')
SHAPE = (3, 8, 10)
M = 7
EVENTS = [0.5, 1.0, 2.5]
TAUS = [0.0, 2.0 / 7.0, 0.5, 1.0]
EDGES = (-np.inf, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.)  # Reliability's default
CELLS = (categorical.TruePositives, categorical.FalsePositives, categorical.FalseNegatives, categorical.TrueNegatives)


# ---- the C ABI, no device ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_refuses_a_null_context():
  lib = _hip.load_library()
  name = 'wbx_ens_prob_contingency_partial'
  assert name in _hip.EXPORTED_SYMBOLS and name in _hip.PROTOS
  rc = lib.wbx_ens_prob_contingency_partial(None, None, _hip.F32, 2, 1, 1, None, 1, None, None, None, None, None)
  assert rc == -1  # WBX_ERR_INVALID
  assert 'wbx_ens_prob_contingency_partial: ctx is NULL' in lib.wbx_last_error().decode()


def test_header_enum_matches_the_binding():
  with open(os.path.join(ROOT, 'include', 'wbx.h')) as f:
    header = f.read()
  assert int(re.search(r'WBX_FN_ENS_PROB_CONTINGENCY_PARTIAL\s*=\s*(\d+)', header).group(1)) == _hip.FN_IDS['wbx_ens_prob_contingency_partial'] == 26
  assert int(re.search(r'#define WBX_EPC_MAX_PAIRS (\d+)', header).group(1)) == _hip.EPC_MAX_PAIRS == 16
  assert int(re.search(r'#define WBX_EPC_MAX_MEMBERS (\d+)', header).group(1)) == _hip.EPC_MAX_MEMBERS == 256
  assert int(re.search(r'#define WBX_EPC_CELLS (\d+)', header).group(1)) == _hip.EPC_CELLS == 4
  assert len(set(_hip.FN_IDS.values())) == len(_hip.FN_IDS)
  # prototype: ctx, plan, dtype, M, member_stride, nthr, thresholds, nslot, slots, p, t, mask, partial_out
  assert len(_hip.load_library() and _hip.PROTOS['wbx_ens_prob_contingency_partial']) == 13
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_replay.hip')) as f:
    assert 'WBX_REPLAY_CASE(WBX_FN_ENS_PROB_CONTINGENCY_PARTIAL, wbx_ens_prob_contingency_partial)' in f.read()
  assert lazy.FUSED_ENS_PROB is True  # the default


# ---- inputs and the chain ---------------------------------------------------------------------------------------------------------
def _inputs(dtype=np.float32, nans=False, mask=False, seed=41, m=M, shape=SHAPE, torch_payload=False):
  rng = np.random.default_rng(seed)
  cs = {'time': np.arange(shape[0]), 'latitude': np.linspace(-70, 70, shape[1]), 'longitude': np.arange(shape[2]) * (360.0 / shape[2])}
  p = (np.round(rng.gamma(2.0, size=(m,) + shape) * 4) / 4).astype(dtype)  # ties with the event thresholds
  t = (np.round(rng.gamma(2.0, size=shape) * 4) / 4).astype(dtype)
  if nans:
    p[rng.random(p.shape) < 0.01] = np.nan
    t[rng.random(shape) < 0.05] = np.nan
  tc = dict(cs)
  if mask:
    tc['mask'] = (DIMS[1:], rng.random(shape[1:]) > 0.3)
  if torch_payload:
    import torch  # pylint: disable=g-import-not-at-top
    p, t = torch.as_tensor(p), torch.as_tensor(t)
  pred = {'v': xr.DataArray(p, dims=('number',) + DIMS, coords=dict(cs, number=np.arange(m)), name='v')}
  targ = {'v': xr.DataArray(t, dims=DIMS, coords=tc, name='v')}
  return pred, targ


def _outer(events=EVENTS, which='both', dim='event'):
  return wrappers.ContinuousToBinary(which, events, dim)


def _mean(which='predictions', **kw):
  return wrappers.EnsembleMean(which, 'number', **kw)


def _taus(taus=TAUS, which='predictions', dim='prob'):
  return wrappers.ContinuousToBinary(which, taus, dim)


def _bins(edges=EDGES, which='predictions', dim='rbin', **kw):
  return wrappers.ContinuousToBins(which, edges, dim, **kw)


def _chain(cell, transforms):
  stat = cell()
  for tr in reversed(transforms):
    stat = wrappers.WrappedStatistic(stat, tr)
  return stat


def _is_fused(stat):
  return isinstance(stat, lazy.LazyEnsProbContingency)


# ---- the restatement against the host route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 2, 3, 7, 50, 51, 64])
def test_restated_cells_are_the_host_routes_indicators_bit_for_bit(monkeypatch, m):
  monkeypatch.setattr(lazy, 'FUSED_ENS_PROB', False)
  for dtype in (np.float32, np.float64):
    pred, targ = _inputs(dtype, nans=True, m=m, seed=m, shape=(2, 4, 5))
    p, t = np.asarray(pred['v'].values), np.asarray(targ['v'].values)
    p[m // 2, 0, 0, 0] = p[0, 1, 2, 3] = t[1, 2, 3] = t[0, 3, 4] = np.nan  # a member only, both, the target only
    taus = [0.0, 1.0, np.nan, 0.5, 1.0 / m, float(np.float32(1.0) / np.float32(m)), (m - 1) / m]
    edges = list(EDGES)
    for inner, hit in ((_taus(taus), EP.hits_thresholds(m, taus)), (_bins(edges), EP.hits_bins(m, edges))):
      slots = EP.runs_of(hit)
      assert slots is not None
      k, j = len(EVENTS), len(slots)
      stat = EP.cells(p, t, EVENTS, slots).reshape(p.shape[1:] + (4, k, j))
      assert np.isnan(stat).any() and np.isfinite(stat).any()
      for cell, cls in enumerate(CELLS):
        host = _chain(cls, [_outer(), _mean(), inner]).compute(pred, targ)['v']
        assert not _is_fused(host) and str(host.dtype) == 'float32'
        assert tuple(host.dims) == DIMS + ('event', 'prob' if type(inner) is wrappers.ContinuousToBinary else 'rbin')
        got = np.asarray(host.values)
        np.testing.assert_array_equal(got.astype(np.float64), stat[..., cell, :, :], err_msg=f'M={m} {np.dtype(dtype).name} cell {cell}')


def test_the_host_route_keeps_nan_points_on_tensor_payloads(monkeypatch):
  """A NaN member or target is a NaN indicator on torch payloads as on NumPy ones (the NaN fill of a Boolean tensor used to turn
  into True): the two routes can only agree on HBM payloads under skipna if the host route itself does."""
  monkeypatch.setattr(lazy, 'FUSED_ENS_PROB', False)
  pred, targ = _inputs(nans=True)
  pred_t, targ_t = _inputs(nans=True, torch_payload=True)
  for inner in (_taus(), _bins()):
    for cls in CELLS:
      stat = _chain(cls, [_outer(), _mean(), inner])
      want = np.asarray(stat.compute(pred, targ)['v'].values)
      got = stat.compute(pred_t, targ_t)['v'].values
      assert np.isnan(want).any()
      np.testing.assert_array_equal(np.asarray(got), want)


# ---- slot tables ------------------------------------------------------------------------------------------------------------------
def _table(inner, m, like=None):
  dim = inner._threshold_dim if isinstance(inner, wrappers.ContinuousToBinary) else inner._bin_dim  # pylint: disable=protected-access
  return lazy.ens_prob_slot_table(_mean(), inner, m, 'number', dim, like=like)


@pytest.mark.parametrize('m', [1, 2, 3, 7, 50, 51, 64])
def test_slot_tables_at_the_edges_of_both_float_types(m):
  import torch  # pylint: disable=g-import-not-at-top
  for c in sorted({0, 1, m // 2, m - 1, m}):
    f32 = np.float32(c) / np.float32(m)  # what the member mean is
    exact = float(f32)
    taus = [exact,
            float(np.nextafter(f32, np.float32(-np.inf))), float(np.nextafter(f32, np.float32(np.inf))),  # float32 neighbours
            float(np.nextafter(exact, -np.inf)), float(np.nextafter(exact, np.inf)),                         # float64 neighbours
            c / m, 0.0, 1.0, np.nan]
    want = EP.runs_of(EP.hits_thresholds(m, taus))
    got, coords = _table(_taus(taus), m)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int32 and list(coords) == ['prob']
    np.testing.assert_array_equal(coords['prob'][1], np.asarray(taus))
    # strict >: the mean itself is not over tau == mean; one float64 step below it is
    assert tuple(got[0]) == ((c + 1, m) if c < m else (1, 0)) and tuple(got[3]) == (c, m)
    assert tuple(got[6]) == ((1, m) if m >= 1 else (1, 0)) and tuple(got[7]) == (1, 0) and tuple(got[8]) == (1, 0)  # tau 0, 1, NaN
    got_t, _ = _table(_taus(taus), m, like=torch.zeros(1))
    np.testing.assert_array_equal(got_t, want)
  # bins: Reliability's default edges (-inf: c = 0 is in the first bin), an empty bin, the labels and the two edge coordinates
  for edges in (EDGES, (-np.inf, 0.0, 1e-9, 0.5, 0.5 + 1e-12, 1.0), (0.0, 1.0)):
    want = EP.runs_of(EP.hits_bins(m, edges))
    got, coords = _table(_bins(edges), m)
    np.testing.assert_array_equal(got, want)
    assert set(coords) == {'rbin', 'rbin_left', 'rbin_right'}
    assert list(coords['rbin'][1]) == [f'{a:.2f} < p <= {b:.2f}' for a, b in zip(edges[:-1], edges[1:])]
    got_t, coords_t = _table(_bins(edges), m, like=torch.zeros(1))
    np.testing.assert_array_equal(got_t, want)
    assert set(coords_t) == set(coords)
  got, _ = _table(_bins(EDGES), m)
  assert got[0][0] == 0  # no member over the threshold: probability 0 sits in (-inf, 0.1]
  got, _ = _table(_bins((-np.inf, 0.0, 1e-9, 0.5, 0.5 + 1e-12, 1.0)), m)
  assert tuple(got[1]) == (1, 0) and tuple(got[0]) == (0, 0)  # (0, 1e-9] holds no c / M
  # every count 0..M is in exactly one of the default bins
  hit = EP.hits_bins(m, EDGES)
  assert (hit.sum(axis=1) == 1).all()


class _TwoRuns(wrappers.InputTransform):
  """An inner transform no bin between two edges gives: slot 0 holds the probabilities 0 and 1 and nothing between them."""

  def __init__(self):
    super().__init__('predictions')

  @property
  def unique_name_suffix(self):
    return 'two_runs'

  def transform_fn(self, da):
    da = xr.as_dataarray(da)
    ends = ((da <= 0.0) | (da >= 1.0)).astype(np.float32)
    inside = ((da > 0.0) & (da < 1.0)).astype(np.float32)
    return xr.concat([ends.expand_dims(prob=[0]), inside.expand_dims(prob=[1])], dim='prob')


def test_a_slot_that_is_not_one_run_is_declined():
  got = lazy.ens_prob_slot_table(_mean(), _TwoRuns(), 5, 'number', 'prob')
  assert got is None  # counts 0 and 5 without 1..4: no run lo <= c <= hi
  hit = np.zeros((6, 2), bool)
  hit[[0, 5], 0], hit[1:5, 1] = True, True
  assert EP.runs_of(hit) is None  # ... and the restatement says the same of the same hits
  # with one member the two ends are neighbours: a run, and a table
  got = lazy.ens_prob_slot_table(_mean(), _TwoRuns(), 1, 'number', 'prob')
  np.testing.assert_array_equal(got[0], [[0, 1], [1, 0]])
  # edges that do not increase still give one run per bin: [p <= 0.2] != [p <= 0.6] is 0.2 < p <= 0.6
  assert _table(_bins((0.6, 0.2, 0.8), enforce_monotonicity=False), 10) is not None


# ---- the stand-in for the launch --------------------------------------------------------------------------------------------------
def _run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=0, ens=None, cat=None, inputs=None, fold=None):
  """fake_device._run_s1 + kind 'epc': the partials of wbx_ens_prob_contingency_partial from the integer restatement."""
  if kind != 'epc':
    return fake_device._run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=func, ens=ens, cat=cat, inputs=inputs, fold=fold)  # pylint: disable=protected-access
  m, mstride = ens
  nthr, thr, nslot, slots = cat
  thr, slots = np.asarray(thr.ptr, np.float64), np.asarray(slots.ptr, np.int32).reshape(-1, 2)
  assert thr.shape == (nthr,) and slots.shape == (nslot, 2) and nthr * nslot <= _hip.EPC_MAX_PAIRS and 1 <= m <= _hip.EPC_MAX_MEMBERS
  assert plan.plane_rows == 0 and plan.x_weights is None and not plan.flags & ~(_hip.FLAG_MASKED | _hip.FLAG_SKIPNA)
  if engine.S1_EVENT_LOG is not None:
    engine.S1_EVENT_LOG.append({'kind': kind, 'flags': int(plan.flags), 'ms': 0.0, 'x_kept': plan.x_kept, 'nthr': nthr, 'nslot': nslot,
                                'vec': plan.vec})
  off = fake_device._offsets(plan, 0)  # pylint: disable=protected-access
  p = np.stack([devs[0].ptr[off + k * mstride] for k in range(m)], axis=0)
  t = devs[1].ptr[fake_device._offsets(plan, 1)]  # pylint: disable=protected-access
  stat = EP.cells(p, t, thr, slots)  # [key, depth, x, lane]
  lanes = [stat[..., l] for l in range(stat.shape[-1])]
  valid = np.ones(lanes[0].shape, bool)
  if plan.flags & _hip.FLAG_MASKED:
    valid = devs[3].ptr[fake_device._offsets(plan, 3)] != 0  # pylint: disable=protected-access
  chunked = fake_device._chunked  # pylint: disable=protected-access
  with np.errstate(all='ignore'):
    if plan.flags & _hip.FLAG_SKIPNA:
      oks = [valid & ~np.isnan(l) for l in lanes]
      cols = [chunked(plan, np.where(ok, l, 0.0)) for ok, l in zip(oks, lanes)] + [chunked(plan, ok.astype(np.float64)) for ok in oks]
    elif plan.flags & _hip.FLAG_MASKED:
      cols = [chunked(plan, np.where(valid, l, 0.0)) for l in lanes] + [chunked(plan, np.broadcast_to(valid, lanes[0].shape).astype(np.float64))]
    else:
      cols = [chunked(plan, l) for l in lanes]
  partial = np.stack(cols, axis=2)
  assert partial.shape[2] == nlanes_total
  return fake_device._Buf(partial.reshape(plan.partial_shape(nlanes_total)))  # pylint: disable=protected-access


@pytest.fixture
def fused(monkeypatch):
  """The emulated backend with the launch available: what a device context whose library exports the symbol gives."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(engine, '_run_s1', _run_s1)
  monkeypatch.setattr(engine, 'ens_prob_available', lambda ctx: True)
  monkeypatch.setattr(lazy, 'FUSED_ENS_PROB', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  yield monkeypatch
  engine.clear_caches()


def _launches(kind='epc'):
  return [e for e in engine.S1_EVENT_LOG if e['kind'] == kind]


def _host(fused, stat, pred, targ):
  fused.setattr(lazy, 'FUSED_ENS_PROB', False)
  try:
    return stat.compute(pred, targ)['v']
  finally:
    fused.setattr(lazy, 'FUSED_ENS_PROB', True)


def _same_labelled_array(got, want, what):
  assert tuple(got.dims) == tuple(want.dims), what
  assert got.name == want.name and str(got.dtype) == str(want.dtype), what
  assert set(got.coords) == set(want.coords), (what, set(got.coords) ^ set(want.coords))
  for k in want.coords:
    assert tuple(got.coords[k].dims) == tuple(want.coords[k].dims), (what, k)
    a, b = np.asarray(got.coords[k].values), np.asarray(want.coords[k].values)
    assert a.dtype.kind == b.dtype.kind, (what, k)
    np.testing.assert_array_equal(a, b, err_msg=f'{what}: {k}')


# ---- the lazy statistic -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_the_chain_gives_a_lazy_statistic_with_the_host_routes_frame_and_values(fused, dtype):
  pred, targ = _inputs(dtype, nans=True, mask=True)
  for inner in (_taus(), _bins(), _taus(np.array(TAUS)), _taus([0.5, np.nan])):
    group = None
    for cell, cls in enumerate(CELLS):
      stat = _chain(cls, [_outer(), _mean(), inner])
      got = stat.compute(pred, targ)['v']
      assert _is_fused(got) and got.is_lazy and got._cell == cell  # pylint: disable=protected-access
      group = group or got._group  # pylint: disable=protected-access
      assert got._group is group and group.kind == 'epc'  # pylint: disable=protected-access  (the four cells share a group)
      want = _host(fused, stat, pred, targ)
      assert not _is_fused(want)
      _same_labelled_array(got, want, f'{type(inner).__name__} cell {cell}')
      assert got.shape == want.shape
      values = np.asarray(got.values)
      assert not got.is_lazy and values.dtype == np.float32
      np.testing.assert_array_equal(values, np.asarray(want.values))
      assert np.isnan(values).any() and (values == 1).any()
  assert not _launches()  # reading values launches nothing
  # another inner transform, other event thresholds: groups of their own
  a = _chain(CELLS[0], [_outer(), _mean(), _taus()]).compute(pred, targ)['v']
  for other in ([_outer(), _mean(), _taus([0.5])], [_outer([0.5]), _mean(), _taus()], [_outer(), _mean(), _bins()]):
    assert _chain(CELLS[0], other).compute(pred, targ)['v']._group is not a._group  # pylint: disable=protected-access
  # targets on fewer dims than the predictions
  assert _is_fused(_chain(CELLS[0], [_outer(), _mean(), _taus()]).compute(pred, {'v': targ['v'].isel(time=0, drop=True)})['v'])
  # behind a renamed statistic (WrappedMetric with a suffix)
  metric = wrappers.WrappedMetric(categorical.CSI(), [_outer(), _mean(), _taus()], unique_name_suffix='x')
  assert all(_is_fused(s.compute(pred, targ)['v']) for s in metric.statistics.values())


def test_every_decline_returns_the_host_objects(fused):
  pred, targ = _inputs(nans=True, mask=True)
  labelled = xr.DataArray(np.array(EVENTS), dims=['event'], coords={'event': np.arange(3)})
  labelled_tau = xr.DataArray(np.array(TAUS), dims=['prob'], coords={'prob': np.arange(4)})
  ens_t = {'v': xr.DataArray(np.asarray(pred['v'].values)[:3], dims=('number',) + DIMS, coords=dict(targ['v'].coords, number=np.arange(3)), name='v')}
  no_ens = {'v': pred['v'].isel(number=0, drop=True)}
  ints = {'v': xr.DataArray(np.asarray(np.nan_to_num(pred['v'].values)).astype(np.int32), dims=pred['v'].dims, coords=dict(pred['v'].coords), name='v')}
  big_p, big_t = _inputs(m=257, shape=(1, 2, 3))
  t_extra = {'v': targ['v'].expand_dims(extra=[0, 1])}
  p_event = {'v': pred['v'].rename({'time': 'event'})}
  t_event = {'v': targ['v'].rename({'time': 'event'})}
  std = [_outer(), _mean(), _taus()]
  declined = [
      ('two wrappers', [_outer(), _mean()], pred, targ),
      ('another order', [_mean(), _outer(), _taus()], pred, targ),
      ('an Inline in the chain', [_outer(), _mean(), wrappers.Inline('predictions', lambda da: da > 0.5, 'gt')], pred, targ),
      ('EnsembleMean(skipna=True)', [_outer(), _mean(skipna=True), _taus()], pred, targ),
      ("EnsembleMean('both')", [_outer(), _mean('both', skip_if_ensemble_dim_missing=True), _taus()], pred, targ),
      ("outer which='predictions'", [_outer(which='predictions'), _mean(), _taus()], pred, {'v': (targ['v'] > 1.0).astype(np.float32).expand_dims(event=EVENTS)}),
      ("inner which='both'", [_outer(), _mean(), _taus(which='both')], pred, targ),
      ('labelled event thresholds', [wrappers.ContinuousToBinary('both', labelled, 'event', unique_name_suffix='l'), _mean(), _taus()], pred, targ),
      ('labelled probability thresholds', [_outer(), _mean(), wrappers.ContinuousToBinary('predictions', labelled_tau, 'prob', unique_name_suffix='l')], pred, targ),
      ('NaN bin edges', [_outer(), _mean(), _bins((-np.inf, 0.5, np.nan), enforce_monotonicity=False)], pred, targ),
      ('an ensemble of targets', std, pred, ens_t),
      ('integer payloads', std, ints, targ),
      ('more than 256 members', std, big_p, big_t),
      ('target dims beyond the predictions', std, pred, t_extra),
      ('the event dim on the inputs', std, p_event, t_event),
  ]
  for what, transforms, p, t in declined:
    stat = _chain(CELLS[0], transforms)
    with np.errstate(all='ignore'):
      got = stat.compute(p, t)['v']
      assert not _is_fused(got), what
      want = _host(fused, stat, p, t)
      _same_labelled_array(got, want, what)
      np.testing.assert_array_equal(np.asarray(got.values), np.asarray(want.values), err_msg=what)
    assert not _launches(), what
  # no ensemble dim on the predictions: the host route raises, and so does the gated one
  for switch in (True, False):
    fused.setattr(lazy, 'FUSED_ENS_PROB', switch)
    with pytest.raises(ValueError, match='number'):
      _chain(CELLS[0], std).compute(no_ens, targ)
  fused.setattr(lazy, 'FUSED_ENS_PROB', True)
  # the switch, a context without the symbol, no device at all
  fused.setattr(lazy, 'FUSED_ENS_PROB', False)
  assert not _is_fused(_chain(CELLS[0], std).compute(pred, targ)['v'])
  fused.setattr(lazy, 'FUSED_ENS_PROB', True)
  assert _is_fused(_chain(CELLS[0], std).compute(pred, targ)['v'])
  fused.setattr(engine, 'ens_prob_available', lambda ctx: False)
  assert not _is_fused(_chain(CELLS[0], std).compute(pred, targ)['v'])
  fused.setattr(engine, 'ens_prob_available', lambda ctx: True)

  def no_device(device_id=None):
    raise _hip.WbxUnavailableError('no device')
  fused.setattr(_hip, 'default_context', no_device)
  assert not _is_fused(_chain(CELLS[0], std).compute(pred, targ)['v'])


def test_a_context_without_the_library_keeps_the_host_route(monkeypatch):
  """The gate as shipped: the plan interpreter's context is no _hip.Context, so nothing asks it for the new launch."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  assert not engine.ens_prob_available(_hip.default_context()) and not engine.ens_prob_available(object())
  pred, targ = _inputs()
  assert not _is_fused(_chain(CELLS[0], [_outer(), _mean(), _taus()]).compute(pred, targ)['v'])
  engine.clear_caches()


# ---- through the Aggregator -------------------------------------------------------------------------------------------------------
def _evaluate(metrics, pred, targ, aggregator):
  return aggregation.compute_metric_values_for_single_chunk(metrics, aggregator, pred, targ)


def _both_routes(fused, metrics, pred, targ, make_aggregator):
  engine.S1_EVENT_LOG.clear()
  on = _evaluate(metrics, pred, targ, make_aggregator())
  launches = list(_launches())
  fused.setattr(lazy, 'FUSED_ENS_PROB', False)
  engine.S1_EVENT_LOG.clear()
  off = _evaluate(metrics, pred, targ, make_aggregator())
  assert not _launches()
  fused.setattr(lazy, 'FUSED_ENS_PROB', True)
  return on, off, launches


def _assert_same_values(on, off, exact):
  assert set(on) == set(off)
  for name in on:  # 'metric.variable' -> DataArray
    a, b = on[name], off[name]
    assert tuple(a.dims) == tuple(b.dims), name
    assert set(a.coords) == set(b.coords), name
    for k in b.coords:
      np.testing.assert_array_equal(np.asarray(a.coords[k].values), np.asarray(b.coords[k].values), err_msg=f'{name}: {k}')
    av, bv = np.asarray(a.values, np.float64), np.asarray(b.values, np.float64)
    if exact:
      np.testing.assert_array_equal(av, bv, err_msg=name)
    else:
      np.testing.assert_allclose(av, bv, rtol=1e-12, atol=1e-13, equal_nan=True, err_msg=name)


AGGREGATORS = {
    'plain': lambda: aggregation.Aggregator(reduce_dims=list(DIMS)),
    'keep time': lambda: aggregation.Aggregator(reduce_dims=['latitude', 'longitude']),
    'area weights': lambda: aggregation.Aggregator(reduce_dims=['latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()]),
    'regions': lambda: aggregation.Aggregator(reduce_dims=list(DIMS), bin_by=[binning.Regions({'north': ((0, 90), (0, 360)), 'all': ((-90, 90), (0, 360))})]),
    'masked': lambda: aggregation.Aggregator(reduce_dims=list(DIMS), masked=True),
    'skipna': lambda: aggregation.Aggregator(reduce_dims=list(DIMS), skipna=True),
}


@pytest.mark.parametrize('how', list(AGGREGATORS))
def test_metrics_agree_with_the_switch_on_and_off(fused, how):
  nans = how == 'skipna'
  pred, targ = _inputs(m=5, nans=nans, mask=True)
  two = [_outer(), _mean()]
  metrics = {
      'csi': wrappers.WrappedMetric(categorical.CSI(), two + [_taus()]),
      'ets': wrappers.WrappedMetric(categorical.ETS(), two + [_taus()]),
      'rev': wrappers.WrappedMetric(multivariate.RelativeEconomicValue(ensemble_size=5), two),
      'reliability': wrappers.WrappedMetric(categorical.Reliability(), two),
  }
  with np.errstate(all='ignore'):
    on, off, launches = _both_routes(fused, metrics, pred, targ, AGGREGATORS[how])
  # one launch per group: CSI and ETS share (the same objects, thresholds and inner transform), REV's four cells one, Reliability's two one
  # (Reliability's 3 x 10 pairs are two blocks of 3 x 5)
  assert sorted((e['nthr'], e['nslot']) for e in launches) == [(3, 4), (3, 5), (3, 5), (3, 5)], launches
  _assert_same_values(on, off, exact=how not in ('area weights',))
  some = np.asarray(on['rev.v'].values)
  assert np.isfinite(some).any()


def test_more_than_sixteen_pairs_are_cut_into_blocks_and_joined_cell_by_cell(fused):
  pred, targ = _inputs(m=5)
  agg = lambda: aggregation.Aggregator(reduce_dims=['latitude', 'longitude'])
  # 4 x 5 = 20 pairs: cut along j (4 x 4 and 4 x 1)
  events = [0.5, 1.0, 2.5, 4.0]
  m1 = {'rev': wrappers.WrappedMetric(multivariate.RelativeEconomicValue(ensemble_size=5), [_outer(events), _mean()])}
  on, off, launches = _both_routes(fused, m1, pred, targ, agg)
  assert [(e['nthr'], e['nslot']) for e in launches] == [(4, 4), (4, 1)]
  _assert_same_values(on, off, exact=True)
  # 17 thresholds x 2 slots: cut along k too (16 x 1, 16 x 1, 1 x 1, 1 x 1)
  events = list(np.arange(17) * 0.25)
  m2 = {'csi': wrappers.WrappedMetric(categorical.CSI(), [_outer(events), _mean(), _taus([0.25, 0.75])])}
  on, off, launches = _both_routes(fused, m2, pred, targ, agg)
  assert [(e['nthr'], e['nslot']) for e in launches] == [(16, 1), (16, 1), (1, 1), (1, 1)]
  _assert_same_values(on, off, exact=True)


class _EventWeights(weighting.Weighting):
  """Weights along the event dim, whatever frame it is asked with."""

  def weights(self, statistic):
    return xr.DataArray(np.array([1.0, 2.0, 0.5]), dims=['event'], coords={'event': np.asarray(EVENTS)})


class _ProbHalves(binning.Binning):
  """Two bins of the probability thresholds, read from the statistic's `prob` coordinate."""

  def __init__(self):
    super().__init__('half')

  def create_bin_mask(self, statistic):
    prob = np.asarray(xr.as_dataarray(statistic).coords['prob'].values)
    return xr.DataArray(np.stack([prob < 0.4, prob >= 0.4]), dims=['half', 'prob'], coords={'half': ['low', 'high'], 'prob': prob})


def test_a_threshold_dim_that_is_reduced_weighted_or_binned_keeps_the_host_route(fused):
  pred, targ = _inputs(m=5)
  metrics = {'csi': wrappers.WrappedMetric(categorical.CSI(), [_outer(), _mean(), _taus()])}
  for dim in ('event', 'prob'):
    on, off, launches = _both_routes(fused, metrics, pred, targ, lambda: aggregation.Aggregator(reduce_dims=list(DIMS) + [dim]))  # pylint: disable=cell-var-from-loop
    assert not launches
    _assert_same_values(on, off, exact=True)
  # plugins from outside the package may look at anything: the host route
  for kw in (dict(weigh_by=[_EventWeights()]), dict(bin_by=[_ProbHalves()])):
    on, off, launches = _both_routes(fused, metrics, pred, targ, lambda: aggregation.Aggregator(reduce_dims=list(DIMS), **kw))  # pylint: disable=cell-var-from-loop
    assert not launches, kw
    _assert_same_values(on, off, exact=True)
  # the package's own: W over the event dim (found in W's dims), bins of the slot coordinate (which the frame without it lacks)
  fused.setattr(_EventWeights, '__module__', weighting.__name__)
  fused.setattr(_ProbHalves, '__module__', binning.__name__)
  for kw, dims in ((dict(weigh_by=[_EventWeights()]), ('event', 'prob')), (dict(bin_by=[_ProbHalves()]), ('event', 'prob', 'half'))):
    on, off, launches = _both_routes(fused, metrics, pred, targ, lambda: aggregation.Aggregator(reduce_dims=list(DIMS), **kw))  # pylint: disable=cell-var-from-loop
    assert not launches, kw
    _assert_same_values(on, off, exact=True)
    assert set(on['csi.v'].dims) == set(dims), on['csi.v'].dims
  # ... while W on the frame alone launches
  _, _, launches = _both_routes(fused, metrics, pred, targ, lambda: aggregation.Aggregator(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()]))
  assert len(launches) == 1


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------------
def test_cases_hold_the_edges_and_leave_three_quarters_of_the_partials_finite():
  thr = EP.event_thresholds(16)
  assert np.isnan(thr).any() and np.inf in thr and -np.inf in thr and 0.1 in thr and 1e40 in thr
  assert any(v == 0 and np.signbit(v) for v in thr) and any(v == 0 and not np.signbit(v) for v in thr)
  for nslot in (1, 4, 5, 16):
    for m in (1, 7, 8, 9, 51, 256):
      s = EP.slot_runs(nslot, m)
      assert s.shape == (nslot, 2) and s.dtype == np.int32
  assert (EP.slot_runs(16, 9)[:, 0] > EP.slot_runs(16, 9)[:, 1]).any()  # an empty slot
  for flags in (0, EP.FLAG_MASKED, EP.FLAG_SKIPNA, EP.FLAG_MASKED | EP.FLAG_SKIPNA):
    for x_kept in (False, True):
      for dc in (5, 2):
        for dtype in (np.float32, np.float64):
          p, t, mask = EP.ens_prob_case(3, 9, 2, 5, 65, dtype, flags, dc, x_kept, thr)
          slots = EP.slot_runs(1, 9)
          want = EP.expected(p, t, thr, slots, mask, flags, dc, x_kept)
          nl = 4 * 16
          assert want.shape == (2, -(-5 // dc), nl if not flags else (2 * nl if flags & EP.FLAG_SKIPNA else nl + 1), 65 if x_kept else 1)
          for v in (np.float32(0.1), np.inf, -np.inf):
            assert (p == v).any()
          assert np.signbit(p[p == 0]).any()
          if flags & EP.FLAG_SKIPNA:
            assert np.isfinite(want).all() and EP.nan_points(p, t).any()
          else:  # the restatement alone: the non-NaN share is the case's own
            assert np.isfinite(want[:, :, :nl]).all(axis=2).mean() >= 0.75
          if flags == EP.FLAG_MASKED:  # NaN points beneath mask = 0 leave no trace
            hidden = EP.nan_points(p, t) & ~mask[None]
            assert hidden.any()
