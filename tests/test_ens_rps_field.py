"""The ranked probability score of ensembles at threshold FIELDS (wbx_ens_rps_field_partial) without a device: the entry point's
export and argument checks, `wrappers.bin_threshold_positions` against `select_bin_thresholds_by_time_from_chunk` rule by rule, the
gate `multivariate.rps_field_route` case by case, the restatement of tests/ens_rps_field_cases.py against the host route and the
oracle, and the mutants the generated cases must tell from the restatement.

Bounds.  Per point the restatement and the float64 arithmetic of the oracle / the host route agree within 16 * K * eps absolute, as
in tests/test_ens_rps.py."""
import os
import re

import numpy as np
import pytest

import ens_rps_cases as EC
import ens_rps_field_cases as FC
import ens_rps_field_gate_cases as GC
import fake_device
from oracle import wbx_oracle as O
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import multivariate
from weatherbenchx_amd.metrics import probabilistic
from weatherbenchx_amd.metrics import wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
DAY, LAT, LON, INITS, LEADS = GC.DAY, GC.LAT, GC.LON, GC.INITS, GC.LEADS
_field, _chunk, _pair, _terciles = GC.field, GC.chunk, GC.pair, GC.terciles


# ---- the C ABI, no device ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_refuses_a_null_context():
  lib = _hip.load_library()
  assert 'wbx_ens_rps_field_partial' in _hip.EXPORTED_SYMBOLS and 'wbx_ens_rps_field_partial' in _hip.PROTOS
  assert lib.wbx_abi_version() == 13
  rc = lib.wbx_ens_rps_field_partial(None, None, _hip.F32, _hip.F32, 2, 1, 1, 1, 0, 1, None, None, None, None, None)
  assert rc == -1  # WBX_ERR_INVALID
  assert 'wbx_ens_rps_field_partial: ctx is NULL' in lib.wbx_last_error().decode()


def test_header_enum_matches_the_binding():
  with open(os.path.join(ROOT, 'include', 'wbx.h')) as f:
    header = f.read()
  assert int(re.search(r'WBX_FN_ENS_RPS_FIELD_PARTIAL\s*=\s*(\d+)', header).group(1)) == _hip.FN_IDS['wbx_ens_rps_field_partial'] == 31
  assert len(set(_hip.FN_IDS.values())) == len(_hip.FN_IDS)
  # ctx, plan, dtype, thr_dtype, M, member_stride, nthr, thr_stride, t_off, right_inclusive, p, t, c, mask, partial_out
  assert len(_hip.load_library() and _hip.PROTOS['wbx_ens_rps_field_partial']) == 15 <= _hip.CALL_MAX_ARGS


# ---- bin_threshold_positions ------------------------------------------------------------------------------------------------------
def _valid_times():
  return np.unique((INITS[:, None] + LEADS[None, :]).reshape(-1))


RULES = {
    'valid_time': lambda: ({'valid_time': _valid_times()[::-1].copy()}, ('init+lead', 'sparse', 'valid_time', 'sparse-time')),
    'time': lambda: ({'time': _valid_times()}, ('init+lead', 'sparse', 'time')),
    # (a sparse chunk against two dims to select along: the selection raises, test_what_the_selection_refuses)
    'init_time+lead_time': lambda: ({'lead_time': LEADS[::-1].copy(), 'init_time': INITS}, ('init+lead',)),
    'dayofyear+lead_time': lambda: ({'dayofyear': np.arange(1, 367), 'lead_time': LEADS}, ('init+lead',)),
    'dayofyear': lambda: ({'dayofyear': np.arange(1, 367)[::-1].copy()}, ('init+lead', 'sparse', 'valid_time', 'time', 'sparse-time')),
    'no time dim': lambda: ({}, ('init+lead', 'sparse', 'valid_time', 'none')),
}


@pytest.mark.parametrize('rule', list(RULES))
def test_positions_are_the_selection_as_an_index_table(rule):
  time_dims, chunks = RULES[rule]()
  field = _field(time_dims, np.random.default_rng(len(rule)))
  for kind in chunks:
    chunk = _chunk(kind)
    want = wrappers.select_bin_thresholds_by_time_from_chunk(field, chunk)
    over_dims, positions = wrappers.bin_threshold_positions(field, chunk)
    what = f'{rule} / {kind}'
    if not time_dims:
      assert over_dims == () and positions == {}, what
    else:
      assert set(positions) == set(time_dims) and all(over_dims and np.asarray(v).shape == tuple(chunk.sizes[d] for d in over_dims)
                                                     for v in positions.values()), what
    got = lazy.ClimatologyRef(field, over_dims, positions).aligned_view()
    assert set(got.dims) == set(want.dims), (what, got.dims, want.dims)
    a, b = np.asarray(got.transpose(*want.dims).values), np.asarray(want.values)
    assert a.dtype == b.dtype and np.isnan(b).any(), what
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64), err_msg=what)  # bit for bit
  # the day of year of the INIT time where the thresholds carry lead_time, of the valid time where they do not
  if rule.startswith('dayofyear'):
    _, positions = wrappers.bin_threshold_positions(field, _chunk('init+lead'))
    days = np.asarray(field.coords['dayofyear'].values)[positions['dayofyear']]
    want_days = [[365, 365, 365], [366, 366, 366], [2, 2, 2]] if rule == 'dayofyear+lead_time' else [[365, 366, 2], [366, 1, 3], [2, 3, 5]]
    np.testing.assert_array_equal(days, want_days)


def test_labels_that_are_not_found_raise_as_the_selection_does():
  field = _field({'valid_time': _valid_times()[:-1]}, np.random.default_rng(1))
  chunk = _chunk('init+lead')
  with pytest.raises(KeyError, match='not all values found') as want:
    wrappers.select_bin_thresholds_by_time_from_chunk(field, chunk)
  with pytest.raises(KeyError, match='not all values found') as got:
    wrappers.bin_threshold_positions(field, chunk)
  assert str(got.value) == str(want.value)


def test_what_the_selection_refuses_is_refused():
  for rule in ('init_time+lead_time', 'dayofyear+lead_time'):
    field = _field(RULES[rule]()[0], np.random.default_rng(2))
    with pytest.raises(ValueError, match='duplicate dimension names'):
      wrappers.select_bin_thresholds_by_time_from_chunk(field, _chunk('sparse'))
    with pytest.raises(ValueError, match='duplicate dimension names'):
      wrappers.bin_threshold_positions(field, _chunk('sparse'))


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
def _route(p, t, pf, tf, **kw):
  args = dict(ensemble_dim='number', bin_dim='bin', skipna_ensemble=False, fair=True)
  args.update(kw)
  return multivariate.rps_field_route(p, t, pf, tf, **args)


def test_the_gate_case_by_case():
  p, t = _pair()
  f = _terciles()
  route, how = _route(p, t, f, f)
  assert route == 'fused' and not how['stacked'] and how['over_dims'] == ('init_time', 'lead_time') and set(how['positions']) == {'dayofyear'}
  g = _terciles(seed=6)
  route, how = _route(p, t, f, g)
  assert route == 'fused' and how['stacked']
  # fields without a time dim, without bin labels, float64 thresholds against float32 data, float64 data
  plain = xr.DataArray(np.array([0.5, 1.0]), dims=['bin'])
  assert _route(p, t, plain, plain) == ('fused', {'over_dims': (), 'positions': {}, 'stacked': False})
  assert _route(p, t, _terciles(dtype=np.float64), _terciles(dtype=np.float64, seed=8))[0] == 'fused'
  assert _route(*_pair(dtype=np.float64), f, g)[0] == 'fused'
  assert _route(*_pair(m=1), f, f, fair=False)[0] == 'fused'
  for case in GC.host_cases():
    route, why = _route(case['p'], case['t'], case['pf'], case['tf'], **{k: v for k, v in case['kw'].items() if k != 'enforce_monotonicity'})
    if case['by'] == 'route':
      assert route == 'host' and isinstance(why, str) and why, case['what']
    else:  # the gate lets it pass; the statistic declines on the field's values or the frame
      assert route == 'fused', case['what']


def test_every_host_case_leaves_the_group_and_gives_the_host_routes_outcome(monkeypatch):
  """Every case through Statistic.compute with the launch available: no statistic of kind 'erpsf', and the values -- or the
  exception -- are those of WBX_FUSED_ENS_RPS_FIELD=0."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(engine, 'ens_rps_field_available', lambda ctx: True)
  for case in GC.host_cases():
    outcomes = []
    for fused in (True, False):
      monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', fused)
      stat = probabilistic.EnsembleRankedProbabilityScore(case['pf'], case['tf'], case['kw'].get('bin_dim', 'bin'), 's',
                                                          **{k: v for k, v in case['kw'].items() if k != 'bin_dim'})
      try:
        with np.errstate(all='ignore'):
          out = stat.compute({'v': case['p']}, {'v': case['t']})['v']
          assert not (isinstance(out, lazy.LazyStatistic) and out._group.kind == 'erpsf'), case['what']  # pylint: disable=protected-access
          outcomes.append(('values', tuple(out.dims), np.asarray(out.values)))
      except (ValueError, KeyError) as err:
        outcomes.append(('raises', type(err).__name__, str(err)))
    assert outcomes[0][:2] == outcomes[1][:2], (case['what'], outcomes[0][:2], outcomes[1][:2])
    if outcomes[0][0] == 'values':
      np.testing.assert_array_equal(outcomes[0][2], outcomes[1][2], err_msg=case['what'])
    else:
      assert outcomes[0][2] == outcomes[1][2], case['what']
  engine.clear_caches()


def test_the_statistic_follows_the_gate_the_switch_and_monotonicity(monkeypatch):
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(engine, 'ens_rps_field_available', lambda ctx: True)
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', True)
  p, t = _pair()
  f, g = _terciles(), _terciles(seed=6)
  rps = lambda a, b, **kw: probabilistic.EnsembleRankedProbabilityScore(a, b, 'bin', 's', **kw)
  is_fused = lambda s: isinstance(s, lazy.LazyStatistic) and s._group.kind == 'erpsf'  # pylint: disable=protected-access
  for a, b in ((f, f), (f, g), (xr.Dataset({'v': f}), xr.Dataset({'v': g}))):
    stat = rps(a, b).compute({'v': p}, {'v': t})['v']
    assert is_fused(stat) and stat.is_lazy and stat.dims == t.dims and stat.dtype == np.float64
    assert stat._group.clim is not None and stat._group.cat['nthr'] == 2  # pylint: disable=protected-access
  # two different fields are stacked once per statistic and pair of field objects
  stat_obj = rps(f, g)
  s1, s2 = (stat_obj.compute({'v': p}, {'v': t})['v'] for _ in range(2))
  src = s1._group.clim.source  # pylint: disable=protected-access
  assert src.dims == (lazy.ERPSF_SIDE_DIM,) + f.dims and s2._group.clim.source is src  # pylint: disable=protected-access
  np.testing.assert_array_equal(np.asarray(src.values), np.stack([np.asarray(f.values), np.asarray(g.values)]))
  # values are the host route's, bit for bit
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', False)
  want = rps(f, g).compute({'v': p}, {'v': t})['v']
  assert not is_fused(want)
  np.testing.assert_array_equal(np.asarray(s1.values), np.asarray(want.values))
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', True)
  # monotonicity: a field that is not strictly increasing, or holds a NaN, keeps the host route when it is enforced
  bad = xr.DataArray(np.asarray(f.values)[::-1].copy(), dims=f.dims, coords={d: f.coords[d].values for d in f.dims}, name='v')
  nan = xr.DataArray(np.asarray(f.values).copy(), dims=f.dims, coords={d: f.coords[d].values for d in f.dims}, name='v')
  nan.values[1, 200, 0, 0] = np.nan  # (a day the chunk does not select)
  assert rps(bad, bad)._fused_per_variable(p, t) is None and rps(nan, nan)._fused_per_variable(p, t) is None  # pylint: disable=protected-access
  with pytest.raises(ValueError, match='monotonically increasing'):  # (the host route raises by the chunk's own selection, as before)
    rps(bad, bad).compute({'v': p}, {'v': t})
  assert not is_fused(rps(nan, nan).compute({'v': p}, {'v': t})['v'])  # (the NaN sits on a day the chunk does not select)
  assert is_fused(rps(bad, bad, enforce_monotonicity=False).compute({'v': p}, {'v': t})['v'])
  assert is_fused(rps(nan, nan, enforce_monotonicity=False).compute({'v': p}, {'v': t})['v'])
  # the list switch does not reach fields, the field switch does not reach lists; a context without the symbol
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', False)
  assert is_fused(rps(f, f).compute({'v': p}, {'v': t})['v'])
  monkeypatch.setattr(lazy, 'FUSED_ENS_RPS', True)
  monkeypatch.setattr(engine, 'ens_rps_field_available', lambda ctx: False)
  assert not is_fused(rps(f, f).compute({'v': p}, {'v': t})['v'])
  engine.clear_caches()


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_oracle_and_the_host_route(monkeypatch):
  """Per point, thresholds that differ from point to point and between the sides: |restatement - oracle| <= 16 K eps, and the host
  route's values (its selection of the chunk's thresholds, the two ContinuousToCDF transforms) within the same bound."""
  rng = np.random.default_rng(11)
  for case in range(60):
    m, k = int(rng.integers(2, 40)), int(rng.integers(1, 17))
    fair, right = bool(case & 1), bool(case & 2)
    p = (rng.integers(-16, 17, size=(m, 6)) / 8.0).astype(np.float32 if case & 4 else np.float64)
    t = (rng.integers(-16, 17, size=6) / 8.0).astype(p.dtype)
    a = rng.integers(-12, 13, size=(6, k)) / 8.0
    b = a if case % 3 else rng.integers(-12, 13, size=(6, k)) / 8.0
    got = FC.numerators(p, t, a, b, fair, right) / EC.denominator(m, fair)
    if b is a:  # the oracle takes one list for both sides: one point at a time, each with its own
      want = np.array([O.ensemble_rps(p[:, j], t[j], a[j], fair=fair, right_inclusive=right) for j in range(6)])
    else:  # two fields: every point's members against a, its target against b
      cmp = np.less_equal if right else np.less
      cp, ct = cmp(p.astype(np.float64)[:, :, None], a[None]).astype(np.float64), cmp(t.astype(np.float64)[:, None], b).astype(np.float64)
      want = ((cp.mean(axis=0) - ct) ** 2 - (cp.var(axis=0, ddof=1) / m if fair else 0.0)).sum(axis=-1)
    assert float(np.abs(got - want).max()) <= 16 * k * EPS, (case, m, k)
  # the host route through the statistic, on the plan interpreter
  engine.clear_caches()
  fake_device.install(monkeypatch)
  p, t = _pair(m=5, dtype=np.float32)
  p.values[...] = np.round(np.asarray(p.values) * 4) / 4
  t.values[...] = np.round(np.asarray(t.values) * 4) / 4
  f = _terciles(dtype=np.float64)
  g = _terciles(seed=6, dtype=np.float64)
  f.values[...] = np.round(np.asarray(f.values) * 4) / 4
  g.values[...] = np.round(np.asarray(g.values) * 4) / 4
  g.values[0, 365, 1, 2] = np.nan  # day 366: (init 2020-12-31, lead 0) and (init 2020-12-30, lead 1)
  for fair in (True, False):
    for right in (True, False):
      host = probabilistic.EnsembleRankedProbabilityScore(f, g, 'bin', 's', fair=fair, right_inclusive=right, enforce_monotonicity=False)
      want = np.asarray(host.host_per_variable(p, t).transpose(*t.dims).values)
      sel = lambda field: np.moveaxis(np.asarray(lazy.ClimatologyRef(field, *wrappers.bin_threshold_positions(field, p)).aligned_view()
                                                 .transpose('bin', *t.dims).values), 0, -1)
      a, b = sel(f), sel(g)
      got = FC.numerators(np.asarray(p.values), np.asarray(t.values), a, b, fair, right) / EC.denominator(5, fair)
      got[FC.nan_points(np.asarray(p.values), np.asarray(t.values), a, b)] = np.nan
      assert np.isnan(want[0, 1, 1, 2]) and np.isnan(want[1, 0, 1, 2]) and np.isnan(want).sum() == 2
      np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
      np.testing.assert_allclose(got, want, rtol=0, atol=16 * 2 * EPS, equal_nan=True)
  engine.clear_caches()


# ---- the mutants the cases must see -----------------------------------------------------------------------------------------------
def _mutant_cases():
  """A handful of generated cases: every (data, threshold) dtype pair, stacked fields that vary over (day, row, x)."""
  for j, (dtype, thr_dtype) in enumerate([(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]):
    yield FC.field_case(500 + j, 7, 5, 2, 5, 65, dtype, thr_dtype, 0, 5, True, 'all', bool(j & 1), True, extra_bins=1)


def _differs(case, a, b, right=True, nan=None):
  want, _ = FC.expected(case.p, case.t, case.selected(0), case.selected(1), True, True, case.mask, 0, 5, True)
  stat = FC.numerators(case.p, case.t, a, b, True, right).astype(np.float64)
  stat[FC.nan_points(case.p, case.t, a, b) if nan is None else nan] = np.nan
  got = EC.expected_partials(stat[..., None], case.mask, 0, 5, True)
  got[:, :, 0] /= EC.denominator(7, True)
  return not np.array_equal(got, want, equal_nan=True)


def test_the_cases_see_the_mutants():
  seen = {k: 0 for k in ('sides swapped', '< for <=', 'rounding to nearest', 'gather ignored', 'NaN thresholds ignored', 'padding slots counted')}
  for case in _mutant_cases():
    a, b = case.selected(0), case.selected(1)
    seen['sides swapped'] += _differs(case, b, a)
    seen['< for <='] += _differs(case, a, b, right=False)
    if case.p.dtype == np.float32 and case.root.dtype == np.float64:
      with np.errstate(over='ignore'):
        near = lambda v: v.astype(np.float32).astype(np.float64)
        seen['rounding to nearest'] += _differs(case, near(a), near(b), nan=FC.nan_points(case.p, case.t, a, b))
      # ... while the directed rounding the kernel uses decides like float64 everywhere
      assert not _differs(case, FC.round_to_float32(a, True).astype(np.float64), FC.round_to_float32(b, True).astype(np.float64))
    seen['gather ignored'] += _differs(case, case.selected(0, days=(0, 1)), case.selected(1, days=(0, 1)))
    seen['NaN thresholds ignored'] += _differs(case, a, b, nan=EC.nan_points(case.p, case.t))
    seen['padding slots counted'] += _differs(case, case.selected(0, nthr=6), case.selected(1, nthr=6), nan=FC.nan_points(case.p, case.t, a, b))
  assert seen.pop('rounding to nearest') == 1 and all(v == 4 for v in seen.values()), seen


# ---- host logic of the fused route, the launch stood in for -----------------------------------------------------------------------
def _run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=0, ens=None, cat=None, inputs=None, fold=None):
  """fake_device._run_s1 + kind 'erpsf': the partials of wbx_ens_rps_field_partial from the restatement, the thresholds read through
  the plan's addressing of input 2 (offset tables, gather table) and the launch's thr_stride / t_off."""
  if kind != 'erpsf':
    return fake_device._run_s1(ctx, kind, dplan, plan, devs, dtype_code, nlanes_total, func=func, ens=ens, cat=cat, inputs=inputs, fold=fold)  # pylint: disable=protected-access
  m, mstride = ens
  thr_dtype, nthr, thr_stride, t_off, right = cat
  assert devs[2].dtype_code == thr_dtype and devs[2].ptr.dtype == (np.float32 if thr_dtype == _hip.F32 else np.float64)
  assert devs[0].ptr.dtype == devs[1].ptr.dtype == (np.float32 if dtype_code == _hip.F32 else np.float64)
  assert plan.plane_rows == 0 and plan.x_weights is None and plan.vec == 1 and (thr_stride != 0 or nthr == 1)
  fair = bool(plan.flags & _hip.FLAG_FAIR)
  engine.S1_EVENT_LOG.append({'kind': kind, 'flags': int(plan.flags), 'ms': 0.0, 'nthr': nthr, 't_off': t_off, 'gather': plan.gather_tab is not None})
  p = np.stack([devs[0].ptr[fake_device._offsets(plan, 0) + k * mstride] for k in range(m)], axis=0)  # pylint: disable=protected-access
  t = devs[1].ptr[fake_device._offsets(plan, 1)]  # pylint: disable=protected-access
  at = fake_device._offsets(plan, 2)[..., None] + np.arange(nthr) * thr_stride  # pylint: disable=protected-access
  a, b = devs[2].ptr[at], devs[2].ptr[at + t_off]
  stat = FC.numerators(p, t, a, b, fair, bool(right)).astype(np.float64)
  stat[FC.nan_points(p, t, a, b)] = np.nan
  valid = devs[3].ptr[fake_device._offsets(plan, 3)] != 0 if plan.flags & _hip.FLAG_MASKED else np.ones(stat.shape, bool)  # pylint: disable=protected-access
  chunked, denom = fake_device._chunked, EC.denominator(m, fair)  # pylint: disable=protected-access
  with np.errstate(all='ignore'):
    if plan.flags & _hip.FLAG_SKIPNA:
      ok = valid & ~np.isnan(stat)
      cols = [chunked(plan, np.where(ok, stat, 0.0)) / denom, chunked(plan, ok.astype(np.float64))]
    elif plan.flags & _hip.FLAG_MASKED:
      cols = [chunked(plan, np.where(valid, stat, 0.0)) / denom, chunked(plan, valid.astype(np.float64))]
    else:
      cols = [chunked(plan, stat) / denom]
  return fake_device._Buf(np.stack(cols, axis=2).reshape(plan.partial_shape(nlanes_total)))  # pylint: disable=protected-access


class _StatisticAsMetric(metrics_base.PerVariableMetric):

  def __init__(self, statistic):
    self._statistic = statistic

  @property
  def statistics(self):
    return {'s': self._statistic}

  def _values_from_mean_statistics_per_variable(self, statistic_values):
    return statistic_values['s']


@pytest.mark.parametrize('thr_dtype', [np.float32, np.float64], ids=['thr32', 'thr64'])
@pytest.mark.parametrize('which', ['plain', 'keep-times', 'masked', 'skipna'])
def test_through_the_aggregator_one_launch_and_the_host_routes_numbers(monkeypatch, which, thr_dtype):
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(engine, '_run_s1', _run_s1)
  monkeypatch.setattr(engine, 'ens_rps_field_available', lambda ctx: True)
  p, t = _pair(m=5)
  p.values[...] = np.round(np.asarray(p.values) * 4) / 4
  t.values[...] = np.round(np.asarray(t.values) * 4) / 4
  if which == 'skipna':
    p.values[2, 1, 1, 2, 3] = t.values[0, 2, 1, 1] = np.nan
  if which == 'masked':
    t = xr.DataArray(np.asarray(t.values), dims=t.dims, coords=dict({d: t.coords[d].values for d in t.dims},
                                                                   mask=(t.dims[2:], np.random.default_rng(0).random(t.shape[2:]) > 0.3)), name='v')
  f, g = _terciles(dtype=thr_dtype), _terciles(seed=6, dtype=thr_dtype)
  for field in (f, g):
    field.values[...] = np.round(np.asarray(field.values) * 4) / 4
  reduce_dims = ['latitude', 'longitude'] if which == 'keep-times' else list(t.dims)
  agg = lambda: aggregation.Aggregator(reduce_dims=reduce_dims, masked=which == 'masked', skipna=which == 'skipna')
  for tf, fair in ((f, True), (g, True), (g, False)):
    stat = lambda: probabilistic.EnsembleRankedProbabilityScore(xr.Dataset({'v': f}), xr.Dataset({'v': tf}), 'bin', 's', fair=fair)
    metrics = {'rps': _StatisticAsMetric(stat())}
    results = {}
    for fused in (True, False):
      monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', fused)
      monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
      stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, {'v': p}, {'v': t})
      state = agg().aggregate_statistics(stats)
      launches = [e for e in engine.S1_EVENT_LOG if e['kind'] == 'erpsf']
      if fused:
        assert len(launches) == 1 == len(engine.S1_EVENT_LOG) and launches[0]['gather'] and (launches[0]['t_off'] != 0) == (tf is not f)
        assert bool(launches[0]['flags'] & _hip.FLAG_FAIR) == fair and launches[0]['nthr'] == 2
      else:
        assert not launches
      results[fused] = (state, state.metric_values(metrics))
    name = stat().unique_name
    (state, values), (state0, values0) = results[True], results[False]
    x, y = state.sum_weighted_statistics[name]['v'], state0.sum_weighted_statistics[name]['v']
    assert tuple(x.dims) == tuple(y.dims)
    np.testing.assert_allclose(np.asarray(x.values), np.asarray(y.values), rtol=0, atol=16 * 2 * EPS * t.size)
    assert np.isfinite(np.asarray(x.values)).all()
    np.testing.assert_allclose(np.asarray(state.sum_weights[name]['v'].values), np.asarray(state0.sum_weights[name]['v'].values), rtol=1e-12)
    assert tuple(values['rps.v'].dims) == tuple(values0['rps.v'].dims)
    np.testing.assert_allclose(np.asarray(values['rps.v'].values), np.asarray(values0['rps.v'].values), rtol=0, atol=16 * 2 * EPS)
  engine.clear_caches()


def _fused_and_host(monkeypatch, stat, p, t, reduce_dims):
  """-> (the launches of kind 'erpsf', the fused route's sums, the host route's) of one statistic through the Aggregator."""
  out = []
  for fused in (True, False):
    monkeypatch.setattr(lazy, 'FUSED_ENS_RPS_FIELD', fused)
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    stats = metrics_base.compute_unique_statistics_for_all_metrics({'rps': _StatisticAsMetric(stat)}, {'v': p}, {'v': t})
    state = aggregation.Aggregator(reduce_dims=reduce_dims).aggregate_statistics(stats)
    out.append(([e for e in engine.S1_EVENT_LOG if e['kind'] == 'erpsf'], np.asarray(state.sum_weighted_statistics[stat.unique_name]['v'].values)))
  return out[0][0], out[0][1], out[1][1], out[1][0]


def test_a_field_without_a_time_dim_goes_the_whole_way_without_a_gather_table(monkeypatch):
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(engine, '_run_s1', _run_s1)
  monkeypatch.setattr(engine, 'ens_rps_field_available', lambda ctx: True)
  p, t = _pair(m=5)
  levels = xr.DataArray(np.array([-0.25, 0.5]), dims=['bin'], name='v')
  places, places2 = _terciles().isel(dayofyear=0, drop=True), _terciles(seed=6).isel(dayofyear=3, drop=True)
  for pf, tf in ((levels, levels), (places, places), (places, places2)):
    stat = probabilistic.EnsembleRankedProbabilityScore(pf, tf, 'bin', 's')
    launches, got, want, host_launches = _fused_and_host(monkeypatch, stat, p, t, ['latitude', 'longitude'])
    assert len(launches) == 1 and not launches[0]['gather'] and (launches[0]['t_off'] != 0) == (pf is not tf) and not host_launches
    np.testing.assert_allclose(got, want, rtol=0, atol=16 * 2 * EPS * 20)
    a = np.moveaxis(np.asarray(pf.values, np.float64), 0, -1)
    b = np.moveaxis(np.asarray(tf.values, np.float64), 0, -1)
    shape = t.shape + (2,)
    s = FC.numerators(np.asarray(p.values), np.asarray(t.values), np.broadcast_to(a, shape), np.broadcast_to(b, shape), True, True)
    np.testing.assert_allclose(got, s.sum(axis=(-2, -1)) / EC.denominator(5, True), rtol=4 * EPS, atol=0)
  engine.clear_caches()


def test_a_field_behind_a_slab_pool_is_gathered_slab_by_slab_or_keeps_the_host_route(monkeypatch):
  """climatology_cache.cached() on the field (what a memory map or a very large array gets by itself): with a time dim the launch
  reads the pool's slabs through its slot table; without one, or where two such fields would have to be stacked, the host route."""
  from weatherbenchx_amd import climatology_cache  # pylint: disable=g-import-not-at-top
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(engine, '_run_s1', _run_s1)
  monkeypatch.setattr(engine, 'ens_rps_field_available', lambda ctx: True)
  p, t = _pair(m=5)
  f = climatology_cache.cached(_terciles(), slots=8)
  stat = probabilistic.EnsembleRankedProbabilityScore(f, f, 'bin', 's')
  launches, got, want, _ = _fused_and_host(monkeypatch, stat, p, t, ['latitude', 'longitude'])
  assert len(launches) == 1 and launches[0]['gather'] and launches[0]['t_off'] == 0
  assert climatology_cache.cache_for(f) is not None and climatology_cache.cache_for(f).stats['uploads'] == 6  # days 365, 366, 1, 2, 3, 5
  np.testing.assert_allclose(got, want, rtol=0, atol=16 * 2 * EPS * 20)
  # no time dim: the pool has nothing to select along; two pooled fields: stacking would read them whole
  flat = climatology_cache.cached(_terciles().isel(dayofyear=0, drop=True), slots=1)
  g = climatology_cache.cached(_terciles(seed=6), slots=8)
  for pf, tf in ((flat, flat), (f, g)):
    stat = probabilistic.EnsembleRankedProbabilityScore(pf, tf, 'bin', 's')
    launches, got, want, _ = _fused_and_host(monkeypatch, stat, p, t, ['latitude', 'longitude'])
    assert not launches
    np.testing.assert_array_equal(got, want)
  engine.clear_caches()
