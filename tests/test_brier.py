"""The fused Brier-type errors of event probabilities (wbx_ens_brier_partial) without a device: the entry point's export and
argument checks, the integer restatement of tests/brier_cases.py against the host route of the chain and the oracle, the gates of
deterministic.Error / AbsoluteError / SquaredError, the lazy statistic as a labelled array, and the host logic of the fused route
(one launch for the three statistics, blocks of thresholds joined statistic by statistic) through the Aggregator with the launch
itself stood in for by the restatement."""
import os
import re

import numpy as np
import pytest

import brier_cases as BC
import fake_device
from oracle import wbx_oracle as O
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import binning
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import weighting
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import deterministic
from weatherbenchx_amd.metrics import wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = ('time', 'latitude', 'longitude')
SHAPE = (3, 8, 10)
M = 7
EVENTS = [0.5, 1.0, 2.5]
STATS = (deterministic.Error, deterministic.AbsoluteError, deterministic.SquaredError)
NAME = 'wbx_ens_brier_partial'


# ---- the C ABI, no device ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_refuses_a_null_context():
  lib = _hip.load_library()
  assert NAME in _hip.EXPORTED_SYMBOLS and NAME in _hip.PROTOS
  rc = lib.wbx_ens_brier_partial(None, None, _hip.F32, 2, 1, 2, 1, None, None, None, None, None)
  assert rc == -1  # WBX_ERR_INVALID
  assert 'wbx_ens_brier_partial: ctx is NULL' in lib.wbx_last_error().decode()


def test_header_declares_the_entry_and_the_binding_matches():
  with open(os.path.join(ROOT, 'include', 'wbx.h')) as f:
    header = f.read()
  proto = re.search(r'int wbx_ens_brier_partial\((.*?)\);', header, re.S).group(1)
  args = [a.split()[-1].lstrip('*') for a in re.sub(r'/\*.*?\*/', '', proto, flags=re.S).split(',')]
  assert args == ['ctx', 'plan', 'dtype', 'M', 'member_stride', 'denom', 'nthr', 'thresholds', 'p', 't', 'mask', 'partial_out']
  assert int(re.search(r'WBX_FN_ENS_BRIER_PARTIAL\s*=\s*(\d+)', header).group(1)) == _hip.FN_IDS[NAME] == 29
  assert int(re.search(r'#define WBX_BRIER_STATS (\d+)', header).group(1)) == _hip.BRIER_STATS == 3
  assert int(re.search(r'#define WBX_BRIER_MAX_THRESHOLDS (\d+)', header).group(1)) == _hip.BRIER_MAX_THRESHOLDS == 16
  assert int(re.search(r'#define WBX_BRIER_MAX_MEMBERS (\d+)', header).group(1)) == _hip.BRIER_MAX_MEMBERS == 256
  assert int(re.search(r'#define WBX_ABI_VERSION (\d+)', header).group(1)) == 13
  assert len(set(_hip.FN_IDS.values())) == len(_hip.FN_IDS)
  # prototype: ctx, plan, dtype, M, member_stride, denom, nthr, thresholds, p, t, mask, partial_out
  assert len(_hip.load_library() and _hip.PROTOS[NAME]) == 12
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_replay.hip')) as f:
    assert 'WBX_REPLAY_CASE(WBX_FN_ENS_BRIER_PARTIAL, wbx_ens_brier_partial)' in f.read()
  with open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'Makefile')) as f:
    assert 'wbx_ens_brier.hip' in f.read()
  assert lazy.FUSED_BRIER is True  # the default
  assert lazy.BRIER_STAT == {'Error': BC.ERR, 'AbsoluteError': BC.ABS, 'SquaredError': BC.SQ}


def test_the_readme_switch_table_holds_the_row():
  with open(os.path.join(ROOT, 'README.md')) as f:
    rows = [l for l in f.read().splitlines() if l.startswith('| `WBX_FUSED_BRIER` |')]
  assert len(rows) == 1 and 'wbx_ens_brier_partial' in rows[0] and rows[0].split('|')[2].strip() == '1'


# ---- inputs and the chains --------------------------------------------------------------------------------------------------------
def _inputs(dtype=np.float32, nans=False, mask=False, seed=41, m=M, shape=SHAPE, ensemble=True):
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
  if ensemble:
    pred = {'v': xr.DataArray(p, dims=('number',) + DIMS, coords=dict(cs, number=np.arange(m)), name='v')}
  else:
    pred = {'v': xr.DataArray(p[0], dims=DIMS, coords=cs, name='v')}
  return pred, {'v': xr.DataArray(t, dims=DIMS, coords=tc, name='v')}


def _outer(events=EVENTS, which='both', dim='event'):
  return wrappers.ContinuousToBinary(which, events, dim)


def _mean(which='predictions', **kw):
  return wrappers.EnsembleMean(which, 'number', **kw)


def _weibull(**kw):
  return wrappers.WeibullEnsembleToProbabilistic('predictions', 'number', **kw)


def _chain(cls, transforms):
  stat = cls()
  for tr in reversed(transforms):
    stat = wrappers.WrappedStatistic(stat, tr)
  return stat


def _is_fused(stat):
  return isinstance(stat, lazy.LazyBrier)


FORMS = {'mean': (lambda: [_outer(), _mean()], lambda m: m, True), 'weibull': (lambda: [_outer(), _weibull()], lambda m: m + 1, True),
         'single': (lambda: [_outer()], lambda m: 1, False)}


# ---- the restatement against the host route and the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 2, 7, 51])
@pytest.mark.parametrize('form', ['mean', 'weibull'])
def test_the_restatement_is_the_host_route_of_the_chain(form, m):
  """The transforms applied as they stand, then float64 NumPy: the probability is a float32 quotient (one rounding, 2^-24 relative),
  so the three statistics agree within 2^-22; with the probability formed in float64 they agree with the oracle within a few ulps."""
  chain, denom_of, _ = FORMS[form]
  denom = denom_of(m)
  for dtype in (np.float32, np.float64):
    pred, targ = _inputs(dtype, nans=True, m=m, seed=m, shape=(2, 4, 5))
    p, t = np.asarray(pred['v'].values), np.asarray(targ['v'].values)
    p[m // 2, 0, 0, 0] = p[0, 1, 2, 3] = t[1, 2, 3] = t[0, 3, 4] = np.nan  # a member only, both, the target only
    outer, mean = chain()
    prob = mean.transform_fn(outer.transform_fn(pred['v']))
    event = outer.transform_fn(targ['v'])
    assert tuple(prob.dims) == DIMS + ('event',) and tuple(event.dims) == DIMS + ('event',)
    pb, ob = np.asarray(prob.values, np.float64), np.asarray(event.values, np.float64)
    want = BC.points(p, t, EVENTS, denom).reshape(p.shape[1:] + (3, len(EVENTS)))
    assert np.isnan(want).any() and np.isfinite(want).any()
    with np.errstate(invalid='ignore'):
      host = (pb - ob, np.abs(pb - ob), (pb - ob) ** 2)
    for stat in range(3):
      np.testing.assert_array_equal(np.isnan(host[stat]), np.isnan(want[..., stat, :]))
      np.testing.assert_allclose(host[stat], want[..., stat, :], rtol=0, atol=2.0 ** -22, equal_nan=True)
    # the oracle's pieces on the exact probability c / D
    c = BC.counts(p, EVENTS).astype(np.float64) / denom
    o = BC.observed(t, EVENTS).astype(np.float64)
    bad = BC.nan_points(p, t)
    for stat, fn in enumerate((O.error, O.absolute_error, O.squared_error)):
      ref = fn(c, o)
      ref[bad] = np.nan
      np.testing.assert_allclose(ref, want[..., stat, :], rtol=0, atol=4 * np.finfo(np.float64).eps, equal_nan=True)


def test_the_restatement_is_exact_where_it_can_be_checked_by_hand():
  thr = [0.1, 0.0, np.nan]
  tenth = np.float32(0.1)
  p = np.array([[tenth, -0.0, np.inf], [np.nextafter(tenth, np.float32(-1)), 0.0, -np.inf], [0.5, -1.0, np.nan]], np.float32)  # [M = 3, x = 3]
  t = np.array([tenth, -0.0, 1.0], np.float32)
  np.testing.assert_array_equal(BC.counts(p, thr), [[2, 3, 0], [0, 0, 0], [1, 1, 0]])  # float32(0.1) > 0.1; -0.0 > 0.0 is false
  np.testing.assert_array_equal(BC.observed(t, thr), [[1, 1, 0], [0, 0, 0], [1, 1, 0]])
  num = BC.numerators(p, t, thr, 4)  # Weibull: D = 4
  np.testing.assert_array_equal(num[0], [-2, -1, 0, 2, 1, 0, 4, 1, 0])
  np.testing.assert_array_equal(num[1], [0] * 9)
  pts = BC.points(p, t, thr, 4)
  assert np.isnan(pts[2]).all()  # a NaN member
  np.testing.assert_array_equal(pts[0], [-0.5, -0.25, 0, 0.5, 0.25, 0, 0.25, 1 / 16, 0])
  want = BC.expected(p[:, None, None, :], t[None, None, :], thr, 4, None, BC.FLAG_SKIPNA, 1, False)
  assert want.shape == (1, 1, 18, 1)
  np.testing.assert_array_equal(want[0, 0, :, 0], [-0.5, -0.25, 0, 0.5, 0.25, 0, 0.25, 1 / 16, 0] + [2.0] * 9)
  want = BC.expected(p[:, None, None, :], t[None, None, :], thr, 4, None, 0, 1, False)
  assert np.isnan(want).all()  # the NaN point poisons the one partial


# ---- the stand-in for the launch --------------------------------------------------------------------------------------------------
def _run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=0, ens=None, cat=None, inputs=None, fold=None):
  """fake_device._run_s1 + kind 'brier': the partials of wbx_ens_brier_partial from the integer restatement."""
  if kind != 'brier':
    return fake_device._run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=func, ens=ens, cat=cat, inputs=inputs, fold=fold)  # pylint: disable=protected-access
  m, mstride, denom = ens
  nthr, thr = cat
  thr = np.asarray(thr.ptr, np.float64)
  assert thr.shape == (nthr,) and 1 <= nthr <= _hip.BRIER_MAX_THRESHOLDS and 1 <= m <= _hip.BRIER_MAX_MEMBERS
  assert denom == 1 if m == 1 else denom in (m, m + 1)
  assert plan.plane_rows == 0 and plan.x_weights is None and not plan.flags & ~(_hip.FLAG_MASKED | _hip.FLAG_SKIPNA)
  if engine.S1_EVENT_LOG is not None:
    engine.S1_EVENT_LOG.append({'kind': kind, 'flags': int(plan.flags), 'ms': 0.0, 'x_kept': plan.x_kept, 'nthr': nthr, 'M': m, 'denom': denom})
  off = fake_device._offsets(plan, 0)  # pylint: disable=protected-access
  p = np.stack([devs[0].ptr[off + k * mstride] for k in range(m)], axis=0)
  t = devs[1].ptr[fake_device._offsets(plan, 1)]  # pylint: disable=protected-access
  stat = BC.points(p, t, thr, denom)  # [key, depth, x, lane]
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
  monkeypatch.setattr(engine, 'brier_available', lambda ctx: True)
  monkeypatch.setattr(lazy, 'FUSED_BRIER', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  yield monkeypatch
  engine.clear_caches()


def _launches(kind='brier'):
  return [e for e in engine.S1_EVENT_LOG if e['kind'] == kind]


def _host(fused, stat, pred, targ):
  fused.setattr(lazy, 'FUSED_BRIER', False)
  try:
    return stat.compute(pred, targ)['v']
  finally:
    fused.setattr(lazy, 'FUSED_BRIER', True)


def _same_frame(got, want, what):
  assert tuple(got.dims) == tuple(want.dims), (what, got.dims, want.dims)
  assert got.name == want.name and tuple(got.shape) == tuple(want.shape), what
  assert set(got.coords) == set(want.coords), (what, set(got.coords) ^ set(want.coords))
  for k in want.coords:
    assert tuple(got.coords[k].dims) == tuple(want.coords[k].dims), (what, k)
    a, b = np.asarray(got.coords[k].values), np.asarray(want.coords[k].values)
    assert a.dtype.kind == b.dtype.kind, (what, k)
    np.testing.assert_array_equal(a, b, err_msg=f'{what}: {k}')


# ---- the lazy statistic -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_the_gates_give_lazy_statistics_with_the_host_routes_frame_and_values(fused, dtype, form):
  chain, denom_of, ensemble = FORMS[form]
  pred, targ = _inputs(dtype, nans=True, mask=True, ensemble=ensemble)
  group = None
  for lane, cls in enumerate(STATS):
    stat = _chain(cls, chain())
    got = stat.compute(pred, targ)['v']
    assert _is_fused(got) and got.is_lazy and got._cell == lane  # pylint: disable=protected-access
    group = group or got._group  # pylint: disable=protected-access
    assert got._group is group and group.kind == 'brier'  # pylint: disable=protected-access  (the three statistics share a group)
    assert group.cat['denom'] == denom_of(M) and (group.ens is not None) == ensemble
    want = _host(fused, stat, pred, targ)
    assert not _is_fused(want)
    _same_frame(got, want, f'{form} {cls.__name__}')
    assert tuple(got.dims) == DIMS + ('event',)
    np.testing.assert_array_equal(np.asarray(got.coords['event'].values), EVENTS)
    values, ref = np.asarray(got.values, np.float64), np.asarray(want.values, np.float64)
    assert not got.is_lazy
    np.testing.assert_array_equal(np.isnan(values), np.isnan(ref))
    np.testing.assert_allclose(values, ref, rtol=0, atol=2.0 ** -22, equal_nan=True)  # (float32 indicator arithmetic on both sides)
    assert np.isnan(values).any() and np.isfinite(values).any()
  assert not _launches()  # reading values launches nothing
  a = _chain(STATS[0], chain()).compute(pred, targ)['v']
  other = [_outer([0.5])] + chain()[1:]
  assert _chain(STATS[0], other).compute(pred, targ)['v']._group is not a._group  # pylint: disable=protected-access
  if ensemble:  # the other denominator: a group of its own
    swapped = [_outer(), _weibull() if form == 'mean' else _mean()]
    assert _chain(STATS[0], swapped).compute(pred, targ)['v']._group is not a._group  # pylint: disable=protected-access
    # targets on fewer dims than the predictions
    assert _is_fused(_chain(STATS[0], chain()).compute(pred, {'v': targ['v'].isel(time=0, drop=True)})['v'])
  # behind a renamed statistic (WrappedMetric with a suffix), and every metric of the family
  for metric in (deterministic.MSE(), deterministic.RMSE(), deterministic.MAE(), deterministic.Bias()):
    wrapped = wrappers.WrappedMetric(metric, chain(), unique_name_suffix='x')
    assert all(_is_fused(s.compute(pred, targ)['v']) for s in wrapped.statistics.values())


def test_every_decline_returns_the_host_objects(fused):
  pred, targ = _inputs(nans=True, mask=True)
  det_p, _ = _inputs(nans=True, mask=True, ensemble=False)
  labelled = xr.DataArray(np.array(EVENTS), dims=['event'], coords={'event': np.arange(3)})
  ens_t = {'v': xr.DataArray(np.asarray(pred['v'].values)[:3], dims=('number',) + DIMS, coords=dict(targ['v'].coords, number=np.arange(3)), name='v')}
  ints = {'v': xr.DataArray(np.asarray(np.nan_to_num(pred['v'].values)).astype(np.int32), dims=pred['v'].dims, coords=dict(pred['v'].coords), name='v')}
  det_ints = {'v': ints['v'].isel(number=0, drop=True)}
  big_p, big_t = _inputs(m=257, shape=(1, 2, 3))
  one_p, one_t = _inputs(m=1, shape=(1, 2, 3))
  t_extra = {'v': targ['v'].expand_dims(extra=[0, 1])}
  p_event, t_event = {'v': pred['v'].rename({'time': 'event'})}, {'v': targ['v'].rename({'time': 'event'})}
  det_p_event = {'v': det_p['v'].rename({'time': 'event'})}
  std = [_outer(), _mean()]
  declined = [
      ('three wrappers', [_outer(), _mean(), wrappers.ReLU('predictions')], pred, targ),
      ('an Inline for the mean', [_outer(), wrappers.Inline('predictions', lambda da: da.mean('number', skipna=False), 'm')], pred, targ),
      ('EnsembleMean(skipna=True)', [_outer(), _mean(skipna=True)], pred, targ),
      ('Weibull(skipna=True)', [_outer(), _weibull(skipna=True)], pred, targ),
      ("EnsembleMean('both')", [_outer(), _mean('both', skip_if_ensemble_dim_missing=True)], pred, targ),
      ('skip_if_ensemble_dim_missing with the dim missing', [_outer(), _mean(skip_if_ensemble_dim_missing=True)], det_p, targ),
      ("which='predictions'", [_outer(which='predictions'), _mean()], pred, {'v': (targ['v'] > 1.0).astype(np.float32).expand_dims(event=EVENTS).transpose(*DIMS, 'event')}),
      ("which='targets', single", [_outer(which='targets')], {'v': (det_p['v'] > 1.0).astype(np.float32).expand_dims(event=EVENTS).transpose(*DIMS, 'event')}, targ),
      ('labelled thresholds', [wrappers.ContinuousToBinary('both', labelled, 'event', unique_name_suffix='l'), _mean()], pred, targ),
      ('labelled thresholds, single', [wrappers.ContinuousToBinary('both', labelled, 'event', unique_name_suffix='l')], det_p, targ),
      ('an ensemble of targets', std, pred, ens_t),
      ('an ensemble dim on the predictions, single', [_outer()], pred, targ),
      ('the threshold dim is the ensemble dim', [_outer(dim='number'), _mean()], pred, targ),
      ('integer payloads', std, ints, targ),
      ('integer payloads, single', [_outer()], det_ints, targ),
      ('more than 256 members', std, big_p, big_t),
      ('one member under the plotting position', [_outer(), _weibull()], one_p, one_t),
      ('target dims beyond the predictions', std, pred, t_extra),
      ('target dims beyond the predictions, single', [_outer()], det_p, t_extra),
      # (where the host route raises, the gated route raises the same)
      ('the threshold dim on the inputs', std, p_event, t_event),
      ('the threshold dim on the inputs, single', [_outer()], det_p_event, t_event),
      ('no ensemble dim on the predictions', std, det_p, targ),
      ('no ensemble dim on the predictions, Weibull', [_outer(), _weibull()], det_p, targ),
  ]
  for what, transforms, p, t in declined:
    for cls in STATS:
      stat = _chain(cls, transforms)
      with np.errstate(all='ignore'):
        try:
          want, raised = _host(fused, stat, p, t), None
        except Exception as e:  # pylint: disable=broad-except  (what the host route raises, the gated route raises)
          want, raised = None, type(e)
        if raised is not None:
          with pytest.raises(raised):
            stat.compute(p, t)
          continue
        got = stat.compute(p, t)['v']
        assert not _is_fused(got), what
        _same_frame(got, want, what)
        np.testing.assert_array_equal(np.asarray(got.values), np.asarray(want.values), err_msg=what)
    assert not _launches(), what
  # the other order is no chain: the mean runs on the host, and what is left is a deterministic pair behind the one transform
  got = _chain(STATS[2], [_mean(), _outer()]).compute(pred, targ)['v']
  assert _is_fused(got) and got._group.ens is None and got._group.cat['denom'] == 1  # pylint: disable=protected-access
  # the hooks themselves: None, never an exception
  for cls in STATS:
    assert cls().compute_with_chain((_outer(), _mean(), _outer(dim='prob', which='predictions')), pred, targ) is None
    assert cls().compute_with_chain((_outer(),), det_p, targ) is None
    assert cls().compute_with_transform(_mean(), pred, targ) is None
    assert cls().compute_with_transform(_outer(), pred, targ) is None
    assert cls().compute_with_chain((_outer(), _mean()), det_p, targ) is None
    assert cls().compute_with_chain((_outer(), _mean()), p_event, t_event) is None

    class Sub(cls):  # a subclass may compute something else
      pass
    assert Sub().compute_with_transform(_outer(), det_p, targ) is None
  # the switch, a context without the symbol, no device at all
  for transforms, p in ((std, pred), ([_outer(), _weibull()], pred), ([_outer()], det_p)):
    stat = _chain(STATS[2], transforms)
    fused.setattr(lazy, 'FUSED_BRIER', False)
    assert not _is_fused(stat.compute(p, targ)['v'])
    fused.setattr(lazy, 'FUSED_BRIER', True)
    assert _is_fused(stat.compute(p, targ)['v'])
    fused.setattr(engine, 'brier_available', lambda ctx: False)
    assert not _is_fused(stat.compute(p, targ)['v'])
    fused.setattr(engine, 'brier_available', lambda ctx: True)

  def no_device(device_id=None):
    raise _hip.WbxUnavailableError('no device')
  fused.setattr(_hip, 'default_context', no_device)
  for transforms, p in ((std, pred), ([_outer()], det_p)):
    assert not _is_fused(_chain(STATS[2], transforms).compute(p, targ)['v'])


def test_a_context_without_the_library_keeps_the_host_route(monkeypatch):
  """The gate as shipped: the plan interpreter's context is no _hip.Context, so nothing asks it for the new launch, and the three
  statistics return what they returned before the gates existed -- the same objects' dims, coordinates and values."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  assert not engine.brier_available(_hip.default_context()) and not engine.brier_available(object())
  for form, (chain, _, ensemble) in FORMS.items():
    pred, targ = _inputs(nans=True, mask=True, ensemble=ensemble)
    for cls in STATS:
      got = _chain(cls, chain()).compute(pred, targ)['v']
      assert not _is_fused(got), form
      # by hand: the transforms, then the statistic
      p, t = pred['v'], targ['v']
      for tr in chain():
        p = tr.transform_fn(p) if tr.which in ('predictions', 'both') else p
        t = tr.transform_fn(t) if tr.which in ('targets', 'both') else t
      want = cls().compute({'v': p}, {'v': t})['v']
      _same_frame(got, want, form)
      np.testing.assert_array_equal(np.asarray(got.values), np.asarray(want.values))
  engine.clear_caches()


# ---- through the Aggregator -------------------------------------------------------------------------------------------------------
def _evaluate(metrics, pred, targ, aggregator):
  return aggregation.compute_metric_values_for_single_chunk(metrics, aggregator, pred, targ)


AGGREGATORS = {
    'plain': lambda: aggregation.Aggregator(reduce_dims=list(DIMS)),
    'keep time': lambda: aggregation.Aggregator(reduce_dims=['latitude', 'longitude']),
    'keep longitude': lambda: aggregation.Aggregator(reduce_dims=['time', 'latitude']),
    'area weights': lambda: aggregation.Aggregator(reduce_dims=['latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()]),
    'regions': lambda: aggregation.Aggregator(reduce_dims=list(DIMS), bin_by=[binning.Regions({'north': ((0, 90), (0, 360)), 'all': ((-90, 90), (0, 360))})]),
    'masked': lambda: aggregation.Aggregator(reduce_dims=list(DIMS), masked=True),
    'skipna': lambda: aggregation.Aggregator(reduce_dims=list(DIMS), skipna=True),
}


def _metrics(chain):
  return {'mse': wrappers.WrappedMetric(deterministic.MSE(), chain()), 'rmse': wrappers.WrappedMetric(deterministic.RMSE(), chain()),
          'mae': wrappers.WrappedMetric(deterministic.MAE(), chain()), 'bias': wrappers.WrappedMetric(deterministic.Bias(), chain())}


@pytest.mark.parametrize('how', list(AGGREGATORS))
@pytest.mark.parametrize('form', list(FORMS))
def test_metrics_agree_with_the_switch_on_and_off(fused, form, how):
  chain, _, ensemble = FORMS[form]
  pred, targ = _inputs(nans=how == 'skipna', mask=how == 'masked', ensemble=ensemble)
  metrics = _metrics(chain)
  engine.S1_EVENT_LOG.clear()
  on = _evaluate(metrics, pred, targ, AGGREGATORS[how]())
  assert len(_launches()) == 1, _launches()  # MSE, RMSE, MAE and Bias: three statistics, ONE launch
  fused.setattr(lazy, 'FUSED_BRIER', False)
  engine.S1_EVENT_LOG.clear()
  off = _evaluate(metrics, pred, targ, AGGREGATORS[how]())
  assert not _launches()
  assert set(on) == set(off) == {f'{k}.v' for k in metrics}
  for name in on:
    a, b = on[name], off[name]
    assert tuple(a.dims) == tuple(b.dims), name
    assert set(a.coords) == set(b.coords), name
    for k in b.coords:
      np.testing.assert_array_equal(np.asarray(a.coords[k].values), np.asarray(b.coords[k].values), err_msg=f'{name}: {k}')
    av, bv = np.asarray(a.values, np.float64), np.asarray(b.values, np.float64)
    np.testing.assert_array_equal(np.isnan(av), np.isnan(bv), err_msg=name)
    # (the host route's probability is a float32 quotient: 2^-24 relative on each point)
    np.testing.assert_allclose(av, bv, rtol=1e-6, atol=1e-7, equal_nan=True, err_msg=name)


def test_more_than_sixteen_thresholds_are_cut_into_blocks_and_joined_statistic_by_statistic(fused):
  events = list(np.round(np.linspace(0.25, 6.0, 37), 3))
  pred, targ = _inputs(nans=True)
  chain = lambda: [_outer(events), _mean()]
  metrics = _metrics(chain)
  make = lambda: aggregation.Aggregator(reduce_dims=['latitude', 'longitude'], skipna=True)
  engine.S1_EVENT_LOG.clear()
  on = _evaluate(metrics, pred, targ, make())
  assert [e['nthr'] for e in _launches()] == [16, 16, 5]
  fused.setattr(lazy, 'FUSED_BRIER', False)
  off = _evaluate(metrics, pred, targ, make())
  for name in on:
    assert tuple(on[name].dims) == tuple(off[name].dims) and on[name].shape == off[name].shape == (3, 37), name
    np.testing.assert_array_equal(np.asarray(on[name].coords['event'].values), events)
    np.testing.assert_allclose(np.asarray(on[name].values), np.asarray(off[name].values), rtol=1e-6, atol=1e-7, err_msg=name)


def test_a_threshold_dim_that_is_reduced_keeps_the_host_route(fused):
  pred, targ = _inputs()
  metrics = _metrics(FORMS['mean'][0])
  engine.S1_EVENT_LOG.clear()
  out = _evaluate(metrics, pred, targ, aggregation.Aggregator(reduce_dims=list(DIMS) + ['event']))
  assert not _launches() and out['mse.v'].shape == ()


def test_cases_hold_the_edges():
  a = BC.thresholds(16)
  assert np.isnan(a).sum() == 1 and np.isinf(a).sum() == 2 and (np.abs(a) > 3e38).sum() == 4 and len(set(a[~np.isnan(a)])) < 15
  for axis in (0, 1, 3):
    p, t, mask = BC.brier_case(5, 7, 2, 5, 65, np.float32, BC.FLAG_MASKED, 3, False, a, member_axis=axis)
    assert p.shape == (7, 2, 5, 65) and t.shape == (2, 5, 65) and mask.shape == (5, 65)
    assert p.strides[0] == {0: 4 * 2 * 5 * 65, 1: 4 * 5 * 65, 3: 4}[axis]
    assert np.isinf(p).any() and np.signbit(p[p == 0]).any() and (p == BC.thresholds(16)[0]).any() and (p == np.float32(0.1)).any()
    want = BC.expected(p, t, a, 8, mask, BC.FLAG_MASKED, 3, False)
    assert want.shape == (2, 2, 49, 1) and np.isfinite(want).mean() > 0.5
