"""The interval statistics' restatement (tests/interval_cases.py) against np.quantile and the three host routes, the (k, g) the Python
layer sends, the group the three statistics of an Opportunism share, and the gate of the fused route: everything that needs no
device."""
import os

import numpy as np
import pytest

import fake_device
import interval_cases as IC
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import planner
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import categorical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 4, 5, 10, 11, 50, 51, 64)
LEVELS = (0, 0.1, 0.25, 0.5, 0.9, 1)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', SIZES)
def test_the_restated_quantile_is_np_quantile_bit_for_bit(m):
  rng = np.random.default_rng(m)
  p = rng.normal(size=(m, 300)) * 10.0 ** rng.integers(-3, 4, size=(1, 300))
  p[:, :40] = np.round(p[:, :40]) + 0.0  # ties (and no negative zero: a lone member -0.0 is np.quantile's -0.0 and the formula's +0.0)
  if m > 1:
    p[0, 5], p[m - 1, 6], p[0, 7], p[m // 2, 8] = np.inf, -np.inf, np.nan, np.inf
    p[:2, 9] = np.inf
  for q in LEVELS + (0.2, 0.7, 0.15, 0.33):
    with np.errstate(all='ignore'):
      want = np.quantile(p, q, axis=0)
    assert IC.ens_quantile(p, q).tobytes() == want.tobytes(), (m, q)
  # float32 members: sorted in their type, interpolated in float64 -- np.quantile of the float64 copy
  p32 = p.astype(np.float32)
  with np.errstate(all='ignore'):
    assert IC.ens_quantile(p32, 0.1).tobytes() == np.quantile(p32.astype(np.float64), 0.1, axis=0).tobytes()


def test_the_python_layers_ranks_and_weights_are_the_restatements():
  for m in range(1, 65):
    for q in LEVELS + (0.2, 0.7, 0.15, 0.33, 0.05, 0.95, 0.999):
      k, g = engine.ivl_bound(q, m)
      assert (k, g) == IC.bound(q, m) and 0 <= k < m and 0.0 <= g < 1.0, (m, q)
  assert IC.bound(0.1, 51) == (5, 0.0) and IC.bound(0.9, 11) == (9, 0.0) and IC.bound(0.5, 4) == (1, 0.5) and IC.bound(1.0, 7) == (6, 0.0)
  assert [IC.padded(m) for m in (1, 4, 5, 8, 9, 16, 17, 32, 33, 50, 51, 52, 64)] == [4, 4, 8, 8, 16, 16, 32, 32, 50, 50, 51, 64, 64]
  assert IC.bound_table((0.1, 0.9), 10) == [IC.bound(0.1, 10), IC.bound(0.9, 10)]


def test_the_operands_builder_sends_ranks_weights_and_element_offsets():
  lay = lambda **st: type('Dev', (), {'layout': planner.InputLayout(strides=st)})()
  devs = [lay(number=1, x=10), lay(x=1), lay(quantile=35, x=1), None]
  ens = {'member_dim': 'number', 'M': 10, 'fair': False}
  cat = {'lanes': 7, 'quantile_dim': 'quantile', 'params': {
      1: {'bounds': (0.1, 0.9), 'threshold': None, 'q_index': None},
      2: {'bounds': (0.2, 0.7), 'threshold': 0.7, 'q_index': (2, 4)},
      4: {'bounds': (0.0, 1.0), 'threshold': 0.75, 'q_index': (0, 6)}}}
  nl, ens_args, cat_args = engine._KINDS['ivl'].operands(None, devs, 0, ens, cat, 'number')  # pylint: disable=protected-access
  assert nl == 3 and tuple(ens_args) == (10, 1, 7) and engine._KINDS['ivl'].keep == ()  # pylint: disable=protected-access
  got = [(b.k, b.g, b.c_off) for lane in cat_args.params for b in (lane.lo, lane.hi)]
  assert got == [IC.bound(0.1, 10) + (0,), IC.bound(0.9, 10) + (0,), IC.bound(0.2, 10) + (70,), IC.bound(0.7, 10) + (140,),
                 IC.bound(0.0, 10) + (0,), IC.bound(1.0, 10) + (210,)]
  assert [lane.threshold for lane in cat_args.params] == [0.0, 0.7, 0.75]
  name, args = engine._KINDS['ivl'].call(['p', 't', 'c', 'm'], 'out', _hip.F32, 0, ens_args, cat_args)  # pylint: disable=protected-access
  assert name == 'wbx_ens_interval_partial' and args == (_hip.F32, 10, 1, 7, cat_args.params, 'p', 't', 'c', 'm', 'out')
  # what the launch would refuse is raised here
  for bad_ens, bad_cat, message in (
      (dict(ens, M=0), cat, '1..64 members'), (dict(ens, M=65), cat, '1..64 members'), (ens, dict(cat, lanes=0), 'non-empty set'),
      (ens, dict(cat, lanes=8), 'non-empty set'),
      (ens, dict(cat, lanes=1, params={1: {'bounds': (0.1, 1.5), 'threshold': None, 'q_index': None}}), 'outside'),
      (ens, dict(cat, lanes=1, params={1: {'bounds': (-0.1, 0.5), 'threshold': None, 'q_index': None}}), 'outside')):
    with pytest.raises(ValueError, match=message):
      engine._KINDS['ivl'].operands(None, devs, 0, bad_ens, bad_cat, 'number')  # pylint: disable=protected-access
  with pytest.raises(ValueError, match='need the climatology'):
    engine._KINDS['ivl'].operands(None, devs[:2] + [None, None], 0, ens, cat, 'number')  # pylint: disable=protected-access
  assert _hip.FN_IDS['wbx_ens_interval_partial'] == 25 and 'wbx_ens_interval_partial' in _hip.EXPORTED_SYMBOLS
  assert (_hip.IVL_COVERED, _hip.IVL_CONFIDENT, _hip.IVL_JACCARD) == IC.BITS and _hip.IVL_MAX_MEMBERS == IC.SIZES[-1]


def test_the_case_set_holds_points_that_a_fused_multiply_add_would_flip():
  """interval_cases.fma_flip_point, which the C-ABI tests launch: with exact rational arithmetic, the bound rounded once (a
  contracted A + d g or B - d (1 - g)) and the bound rounded twice (NumPy, the header) lie on different sides of the target."""
  for m, q in ((10, 0.1), (10, 0.15)):
    k, g = IC.bound(q, m)
    assert (g < 0.5) == (q == 0.15) and g != 0.0  # both branches
    for seed in range(8):
      x, target, levels, stated, fused = IC.fma_flip_point(m, q, np.float64, seed)
      xs = np.sort(x)
      plain = float(IC.quantile_sorted(xs, k, g))
      assert plain == float(np.quantile(x, q)) and IC.fma_quantile(xs, k, g) != plain
      assert stated != fused and stated == bool(IC.covered(x[:, None], np.array([target]), levels)[0])
      assert stated == (plain <= float(target)) and fused == (IC.fma_quantile(xs, k, g) <= float(target))


# ---- the host routes ---------------------------------------------------------------------------------------------------------------
STATS = {
    'Covered': lambda clim, lv=(0.1, 0.9): categorical.Covered('number', lv),
    'Confident': lambda clim, lv=(0.1, 0.9): categorical.Confident('number', clim, lv, 0.7),
    'JaccardDistant': lambda clim, lv=(0.2, 0.7): categorical.JaccardDistant('number', clim, 0.75, lv),
}


def _restated(which, p, t, c, levels=None):
  pick = lambda q: c[IC.LEVELS.index(q)]
  if which == 'Covered':
    return IC.covered(p, t, levels or (0.1, 0.9))
  if which == 'Confident':
    lv = levels or (0.1, 0.9)
    return IC.confident(p, pick(lv[0]), pick(lv[1]), lv, 0.7)
  lv = levels or (0.2, 0.7)
  return IC.jaccard_distant(p, pick(lv[0]), pick(lv[1]), lv, 0.75)


@pytest.mark.parametrize('which', list(STATS))
@pytest.mark.parametrize('m', (1, 4, 10, 11, 51))
def test_the_restatement_is_the_host_route_on_float64_exactly(which, m):
  pred, targ, clim, (p, t, c, _) = IC.api_inputs(np.float64, m, seed=m, nans=True)
  rng = np.random.default_rng(m)
  for j, kind in enumerate(IC.EDGE_KINDS):  # the edge points too (the climatology's are NaNs of `nans`)
    if kind not in ('nan_clim', 'equal_members_point_clim'):
      IC.put_edge(p, t, c, (j % 2, j % 3, j % 6, j % 9), kind, {IC.COVERED: ((0.1, 0.9), None)}, rng)
  pred = {'v': xr.DataArray(p, dims=pred['v'].dims, coords={k: v for k, v in pred['v'].coords.items()}, name='v')}
  targ = {'v': xr.DataArray(t, dims=targ['v'].dims, coords={k: v for k, v in targ['v'].coords.items()}, name='v')}
  got = STATS[which](clim).compute(pred, targ)['v']
  assert not isinstance(got, lazy.LazyStatistic) and got.dtype == bool and got.dims == IC.API_DIMS and got.name == 'v'
  want = _restated(which, p, t, c)
  np.testing.assert_array_equal(np.asarray(got.values), want)
  assert 0 < want.sum() < want.size or m == 1


def test_float32_inputs_on_which_float32_interpolation_is_exact():
  """What the public-API tests feed both routes in float32: eighths around 280, M = 11 or 51 with levels whose g is 0."""
  for m in (11, 51):
    assert all(IC.bound(q, m)[1] == 0.0 for q in (0.1, 0.9, 0.2, 0.7))
    pred, targ, clim, (p, t, c, _) = IC.api_inputs(np.float32, m)
    for which in STATS:
      thr = {'Confident': lambda cl: categorical.Confident('number', cl, (0.1, 0.9), 0.75)}.get(which, STATS[which])
      got = thr(clim).compute(pred, targ)['v']
      want = _restated(which, p, t, c) if which != 'Confident' else IC.confident(p, c[1], c[5], (0.1, 0.9), 0.75)
      np.testing.assert_array_equal(np.asarray(got.values), want, err_msg=f'{which} M={m}')


# ---- the gating --------------------------------------------------------------------------------------------------------------------
def _same(a, b):
  """Values, dims, coordinates, name and dtype of two results."""
  assert a.dims == b.dims and a.name == b.name and a.dtype == b.dtype
  np.testing.assert_array_equal(np.asarray(a.values), np.asarray(b.values))
  assert set(a.coords) == set(b.coords)
  for k in a.coords:
    assert a.coords[k].dims == b.coords[k].dims
    np.testing.assert_array_equal(np.asarray(a.coords[k].values), np.asarray(b.coords[k].values))


class _Ctx(_hip.Context):  # a context the gate may ask: nothing is launched on it
  def __init__(self):  # pylint: disable=super-init-not-called
    self.lib = type('Lib', (), {'wbx_ens_interval_partial': staticmethod(lambda *a: 0)})()

  def __del__(self):
    pass


def _host(which, clim, pred, targ):
  stat = STATS[which](clim)
  if which == 'Covered':
    return stat.host_per_variable(pred['v'], targ['v'])
  ref = metrics_base.PerVariableStatisticWithClimatology.resolve_climatology(pred['v'], xr.as_dataarray(clim['v']))
  return stat.host_per_variable(pred['v'], targ['v'], ref)


def _is_fused(stat):
  return isinstance(stat, lazy.LazyInterval) and stat._group.kind == 'ivl'  # pylint: disable=protected-access


@pytest.mark.parametrize('which', list(STATS))
def test_the_gate_takes_the_plain_case_and_labels_it_as_the_host_route(monkeypatch, which):
  monkeypatch.setattr(_hip, 'default_context', _Ctx)
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', True)
  for kw in (dict(), dict(mask=True), dict(member_last=True)):
    pred, targ, clim, _ = IC.api_inputs(np.float32, 11, **kw)
    got = STATS[which](clim).compute(pred, targ)['v']
    host = _host(which, clim, pred, targ)
    assert _is_fused(got) and got.is_lazy
    assert got.dims == host.dims == IC.API_DIMS and got.name == host.name == 'v' and got.dtype == host.dtype == bool
    assert got.shape == host.shape and set(got.coords) == set(host.coords)
    for k in host.coords:
      np.testing.assert_array_equal(np.asarray(got.coords[k].values), np.asarray(host.coords[k].values))
    assert ('mask' in got.coords) == bool(kw.get('mask'))
  for m, dtype in ((1, np.float32), (64, np.float64)):
    pred, targ, clim, _ = IC.api_inputs(dtype, m)
    assert _is_fused(STATS[which](clim).compute(pred, targ)['v']), m


def test_the_three_statistics_of_an_opportunism_share_one_group(monkeypatch):
  monkeypatch.setattr(_hip, 'default_context', _Ctx)
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', True)
  pred, targ, clim, _ = IC.api_inputs(np.float32, 11)
  metric = categorical.Opportunism('number', clim, True, True, True, confidence_quantile_boundaries=(0.2, 0.7),
                                   jaccard_distance_quantile_boundaries=(0.0, 1.0), confidence_threshold=0.6)
  stats = metrics_base.compute_unique_statistics_for_all_metrics({'o': metric}, pred, targ)
  by = {k.split('_')[0]: v['v'] for k, v in stats.items()}
  assert set(by) == {'Confident', 'Covered', 'JaccardDistant'} and all(_is_fused(s) for s in by.values())
  grp = by['Covered']._group  # pylint: disable=protected-access
  assert all(s._group is grp for s in by.values()) and grp.cat['lanes'] == 7 and grp.clim is not None  # pylint: disable=protected-access
  assert [by[k]._lane for k in ('Covered', 'Confident', 'JaccardDistant')] == [0, 1, 2]  # pylint: disable=protected-access
  assert grp.cat['params'][2] == {'bounds': (0.2, 0.7), 'threshold': 0.6, 'q_index': (2, 4)}
  assert grp.cat['params'][4] == {'bounds': (0.0, 1.0), 'threshold': 0.75, 'q_index': (0, 6)}
  assert grp.cat['params'][1] == {'bounds': (0.1, 0.9), 'threshold': None, 'q_index': None}
  assert grp.ens == {'member_dim': 'number', 'M': 11, 'fair': False} and len(grp.inputs_and_func()[0]) == 3
  # the value lane is the statistic's place among the lanes that have joined: it moves when a lane joins in front of it
  pred, targ, clim, _ = IC.api_inputs(np.float32, 11, seed=5)
  jac = STATS['JaccardDistant'](clim).compute(pred, targ)['v']
  assert jac._lane == 0 and jac._group.cat['lanes'] == 4  # pylint: disable=protected-access
  jac._group.cache['sums of a launch of one lane'] = None  # pylint: disable=protected-access
  cov = STATS['Covered'](clim).compute(pred, targ)['v']
  assert cov._group is jac._group and (cov._lane, jac._lane) == (0, 1) and not jac._group.cache  # pylint: disable=protected-access
  # the same statistic again joins its lane; other levels or another threshold of one kind open a group of their own
  again = STATS['Covered'](clim).compute(pred, targ)['v']
  other = STATS['Covered'](clim, (0.2, 0.7)).compute(pred, targ)['v']
  assert again._group is cov._group and _is_fused(other) and other._group is not cov._group  # pylint: disable=protected-access
  assert other._group.cat['lanes'] == 1 and other._lane == 0  # pylint: disable=protected-access


def _decline_cases(pred, targ, clim):
  p, t = pred['v'], targ['v']
  rename = lambda ds, **kw: xr.Dataset({'v': xr.as_dataarray(ds['v']).rename(kw)})
  cl = xr.as_dataarray(clim['v'])
  return {
      'integer inputs': ({'v': p.astype(np.int64)}, {'v': t.astype(np.int64)}, clim),
      'float16 inputs': ({'v': p.astype(np.float16)}, {'v': t.astype(np.float16)}, clim),
      'targets of another dtype': (pred, {'v': t.astype(np.float64)}, clim),
      'a climatology of another dtype': (pred, targ, xr.Dataset({'v': cl.astype(np.float64)})),
      '65 members': IC.api_inputs(np.float32, 65)[:3],
      'a mask along the member dim': ({'v': p.assign_coords(mask=(('number',), np.ones(p.sizes['number'], bool)))}, targ, clim),
      'a dim the targets lack': (pred, {'v': t.isel(lead_time=0, drop=True)}, clim),
      'latitude labels that differ': (pred, {'v': t.assign_coords(latitude=IC.API_LAT + 1.0)}, clim),
      'a climatology without one of the levels': (pred, targ, xr.Dataset({'v': cl.isel(quantile=[0, 2, 3, 5, 6])})),
  }


@pytest.mark.parametrize('which', list(STATS))
def test_the_gate_declines_every_fallback_condition_without_a_device(monkeypatch, which):
  monkeypatch.setattr(_hip, 'default_context', _Ctx)
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', True)
  pred, targ, clim, _ = IC.api_inputs(np.float32, 11)
  for why, (a, b, cl) in _decline_cases(pred, targ, clim).items():
    stat = STATS[which](cl)
    try:
      want = _host(which, cl, a, b)
    except (KeyError, ValueError) as e:  # the host route itself refuses (a level the climatology lacks): so does compute()
      with pytest.raises(type(e)):
        stat.compute(a, b)
      continue
    got = stat.compute(a, b)['v']
    if which == 'Covered' and 'climatology' in why:
      assert _is_fused(got), why  # Covered does not look at the climatology
      continue
    assert not isinstance(got, lazy.LazyStatistic), why
    _same(got, want)
  # nothing left of the frame
  sel = dict(init_time=0, lead_time=0, latitude=0, longitude=0)
  if which == 'Covered':
    a, b = {'v': pred['v'].isel(**sel, drop=True)}, {'v': targ['v'].isel(**sel, drop=True)}
    got = STATS[which](clim).compute(a, b)['v']
    assert not isinstance(got, lazy.LazyStatistic) and got.dims == ()
  # the switch
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', False)
  got = STATS[which](clim).compute(pred, targ)['v']
  assert not isinstance(got, lazy.LazyStatistic)
  _same(got, _host(which, clim, pred, targ))


def test_a_library_without_the_symbol_or_no_device_keep_the_host_route(monkeypatch):
  class Old(_Ctx):
    def __init__(self):  # pylint: disable=super-init-not-called
      self.lib = type('Lib', (), {})()
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', True)
  pred, targ, clim, _ = IC.api_inputs(np.float32, 11)
  monkeypatch.setattr(_hip, 'default_context', Old)
  assert not any(_is_fused(STATS[w](clim).compute(pred, targ)['v']) for w in STATS)

  def no_device(*a, **k):
    raise _hip.WbxUnavailableError('no device')
  monkeypatch.setattr(_hip, 'default_context', no_device)
  assert not any(_is_fused(STATS[w](clim).compute(pred, targ)['v']) for w in STATS)
  assert not engine.ens_interval_available(object()) and engine.ens_interval_available(_Ctx())


def test_a_context_without_the_library_keeps_the_host_route(monkeypatch):
  """The plan interpreter's context is no _hip.Context, so nothing asks it for the new launch: Opportunism through the Aggregator is
  the product of the restatement's three means."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(lazy, 'FUSED_INTERVALS', True)
  log = []
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', log)
  pred, targ, clim, (p, t, c, _) = IC.api_inputs(np.float64, 10)
  metric = categorical.Opportunism('number', clim, True, False, True)
  stats = metrics_base.compute_unique_statistics_for_all_metrics({'o': metric}, pred, targ)
  assert not any(isinstance(v['v'], lazy.LazyStatistic) for v in stats.values())
  out = aggregation.Aggregator(reduce_dims=list(IC.API_DIMS)).aggregate_statistics(stats).metric_values({'o': metric})
  assert not [e for e in log if e['kind'] == 'ivl']
  want = (IC.confident(p, c[1], c[5], (0.1, 0.9), 0.7).mean() * (1 - IC.covered(p, t, (0.1, 0.9)).mean())
          * IC.jaccard_distant(p, c[1], c[5], (0.1, 0.9), 0.75).mean())
  np.testing.assert_allclose(float(np.asarray(out['o.v'].values)), want, rtol=1e-12)
  engine.clear_caches()


def test_the_switch_reads_the_environment_and_the_readme_documents_it():
  assert lazy.FUSED_INTERVALS == (os.environ.get('WBX_FUSED_INTERVALS', '1') != '0')
  with open(os.path.join(ROOT, 'README.md')) as f:
    readme = f.read()
  row = [line for line in readme.splitlines() if line.startswith('| `WBX_FUSED_INTERVALS` |')]
  assert len(row) == 1 and 'wbx_ens_interval_partial' in row[0] and 'tools/bench_intervals.py' in row[0]
  assert 'interval statistics' in [line for line in readme.splitlines() if line.startswith('| hot kernels |')][0]
