"""The fused route of FSS behind ContinuousToBinary without a device: the restatement of tests/fss_threshold_cases.py against the host
chain (wrappers.binarize_thresholds -> the statistic's host route) and the oracle, the mutants of the restatement that the cases must
see, the gate of `_FractionStatistic.compute_with_transform`, the labels of the lazy result, the lane bookkeeping of the group's
reduction under a stand-in for the launch, what the threshold dim declines at the Aggregator, and the ABI constants."""
import os
import re

import numpy as np
import pytest

import fss_cases as FC
import fss_threshold_cases as TC
from oracle import wbx_oracle as O
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import binning
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import weighting
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import spatial
from weatherbenchx_amd.metrics import wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = ('time', 'latitude', 'longitude')
THR = 'threshold'
TERMS = ('SquaredFractionsError', 'SquaredPredictionFraction', 'SquaredTargetFraction')
CLASSES = [getattr(spatial, name) for name in TERMS]


def _pair(shape=(2, 9, 11), dims=DIMS, dtype=np.float32, t_dtype=None, seed=3, mask=False, thresholds=(0.1, 0.5)):
  p, t = TC.continuous_fields(shape, dtype, seed, list(thresholds)) if np.dtype(dtype).kind == 'f' and np.dtype(dtype).itemsize >= 4 \
      else (np.ones(shape, dtype), np.ones(shape, dtype))
  cs = {d: np.arange(n, dtype=np.float64) for d, n in zip(dims, shape)}
  tc = dict(cs)
  if mask:
    tc['mask'] = (dims, np.random.default_rng(seed).random(shape) > 0.2)
  return xr.DataArray(p, dims=dims, coords=cs), xr.DataArray(t.astype(t_dtype or dtype), dims=dims, coords=tc)


def _host_chain(cls, sizes, wrap, p, t, thresholds, dim=THR):
  """What the route without the gate computes: both inputs binarised, then the statistic's host route."""
  stat = cls(sizes, wrap_longitude=wrap)
  return stat.host_per_variable(wrappers.binarize_thresholds(p, list(thresholds), dim), wrappers.binarize_thresholds(t, list(thresholds), dim))


# ---- the restatement ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_the_restatement_is_the_host_chain_point_by_point(dtype):
  """Every threshold list, several shapes and sizes, both wrap settings: NaN placement and every value, bit for bit (the fractions of
  0 / 1 fields are the same numbers on both sides, tests/test_fss.py)."""
  points = 0
  for i, (nlat, nlon) in enumerate(((9, 11), (12, 16), (5, 300))):
    for k, thresholds in TC.THRESHOLD_LISTS.items():
      p, t = _pair(shape=(2, nlat, nlon), dtype=dtype, seed=10 * i + k, thresholds=thresholds)
      sizes = TC.sizes_for(nlat, nlon)
      wrap = bool((i + k) & 1)
      for l, cls in enumerate(CLASSES):
        host = _host_chain(cls, sizes, wrap, p, t, thresholds)
        assert host.dims == ('neighborhood_size', 'time', THR, 'latitude', 'longitude') and host.dtype == np.float32
        got = np.asarray(host.values, np.float64)
        for s, n in enumerate(sizes):
          want = TC.point_values(np.asarray(p.values), np.asarray(t.values), thresholds, n, wrap)[:, l]  # [K, time, lat, lon]
          assert FC.same_numbers(got[s], np.moveaxis(want, 0, 1)), (nlat, nlon, k, n, cls.__name__)
          points += want.size
  assert points > 100000


def test_the_restatement_against_the_oracle():
  """The oracle covers FSS of binary fields with plain means: clean continuous fields, thresholded on the host."""
  rng = np.random.default_rng(5)
  p, t = rng.random((2, 7, 9)), rng.random((2, 7, 9)) * 0.9
  thresholds = [0.3, 0.5, 0.8]
  for n in (1, 3, 5):
    for wrap in (False, True):
      v = TC.point_values(p, t, thresholds, n, wrap)
      for k, thr in enumerate(thresholds):
        want = O.fractions_skill_score((p > thr).astype(float), (t > thr).astype(float), n, wrap)
        got = 1 - v[k, 0].mean() / (v[k, 1].mean() + v[k, 2].mean())
        np.testing.assert_allclose(got, want, rtol=2e-6)


def test_lanes_and_partials_of_the_restatement():
  thresholds = TC.THRESHOLD_LISTS[TC.NAN_INF]
  p, t = TC.continuous_fields((2, 3, 9, 11), np.float32, 1, thresholds)
  v = TC.point_values(p, t, thresholds, 3, True)
  assert v.shape == (5, 3, 2, 3, 9, 11)
  assert (np.nan_to_num(v[1]) == 0).all() and (np.nan_to_num(v[3]) == 0).all()  # a NaN and a +inf threshold: never exceeded
  assert np.isnan(v[1]).any()  # ... but a NaN member is a NaN fraction whatever the threshold is
  mask = (np.arange(99).reshape(9, 11) % 3 != 0).astype(np.uint8)
  for flags, nl in ((0, 15), (1, 16), (2, 30), (3, 30)):
    want, mag, nterm = TC.partials(v, mask, flags, 2, False)
    assert want.shape == (2, 9, 2, nl, 1) and mag.shape == nterm.shape == (2, 9, 2, 15, 1) and TC.lanes_total(flags, 5) == nl
    for k in range(5):
      one = FC.partials(v[k], mask, flags, 2, False)[0]
      assert FC.same_numbers(TC.slice_of(want, flags, 5, k), one)


MUTANTS = ('ge', 'nearest', 'nan_zero', 'shared_nan')


@pytest.mark.parametrize('mutant', MUTANTS)
def test_every_mutant_of_the_restatement_is_seen(mutant):
  """Each wrong restatement differs from the host chain on the cases' own fields, at the shapes the GPU tests use."""
  seen = []
  for dtype in (np.float32, np.float64):
    for k, thresholds in TC.THRESHOLD_LISTS.items():
      p, t = TC.continuous_fields((2, 9, 11), dtype, 40 + k, thresholds)
      for n in (1, 3):
        right = TC.point_values(p, t, thresholds, n, True)
        wrong = TC.point_values(p, t, thresholds, n, True, mutant=mutant)
        seen.append(not FC.same_numbers(right, wrong))
        host = np.asarray(_host_chain(spatial.SquaredFractionsError, n, True, xr.DataArray(p, dims=DIMS), xr.DataArray(t, dims=DIMS),
                                      thresholds).values, np.float64)
        assert FC.same_numbers(np.moveaxis(right[:, 0], 0, 1), host)  # (the right one IS the host chain)
  print(mutant, 'seen by', sum(seen), 'of', len(seen), 'cases')
  assert any(seen), mutant
  if mutant == 'nearest':  # only float32 inputs can see it, and only under a threshold that is no float32
    p, t = TC.continuous_fields((2, 9, 11), np.float32, 41, [0.1])
    assert (p == np.float32(0.1)).any()
    assert not FC.same_numbers(TC.point_values(p, t, [0.1], 1, True), TC.point_values(p, t, [0.1], 1, True, mutant=mutant))


# ---- the gate -----------------------------------------------------------------------------------------------------------------

class _FakeContext:
  device_id = 0


@pytest.fixture
def device(monkeypatch):
  """A launch context that exists and has both entry points, as far as the gate asks."""
  monkeypatch.setattr(lazy, 'FUSED_FSS', True)
  monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', True)
  monkeypatch.setattr(_hip, 'default_context', lambda *a, **k: _FakeContext())
  monkeypatch.setattr(engine, 'fss_available', lambda ctx: True)
  monkeypatch.setattr(engine, 'fss_thresholds_available', lambda ctx: True)


def _transform(values=(0.1, 0.5), which='both', dim=THR, **kw):
  return wrappers.ContinuousToBinary(which, values if isinstance(values, (xr.DataArray, xr.Dataset)) else list(values), dim, **kw)


def test_the_gate_takes_what_the_kernel_serves(device):
  for sizes in (3, [1, 3, 5], (3, 9), np.array([1, 9])):
    for cls in CLASSES:
      for dtype in (np.float32, np.float64):
        p, t = _pair(dtype=dtype)
        out = cls(sizes, wrap_longitude=True).compute_with_transform(_transform(), {'v': p}, {'v': t})
        assert set(out) == {'v'} and isinstance(out['v'], lazy.LazyFSS) and out['v'].is_lazy and out['v'].threshold_dim == THR
        assert out['v']._cell == lazy.FSS_TERM[cls.__name__]  # pylint: disable=protected-access
  # variables of the predictions that the targets lack are dropped, as PerVariableStatistic drops them
  p, t = _pair()
  out = spatial.SquaredFractionsError(3).compute_with_transform(_transform(), {'v': p, 'w': p}, {'v': t})
  assert set(out) == {'v'}


class _OtherBinary(wrappers.ContinuousToBinary):
  pass


def _labelled_thresholds():
  return xr.DataArray(np.array([0.1, 0.5]), dims=[THR], coords={THR: np.array([0.1, 0.5])})


# why -> (monkeypatch) -> (p, t[, sizes[, transform]])
DECLINES = {
    'switch off': lambda mp: (mp.setattr(lazy, 'FUSED_FSS_THRESHOLDS', False), _pair())[1],
    'the FSS switch off': lambda mp: (mp.setattr(lazy, 'FUSED_FSS', False), _pair())[1],
    'no device': lambda mp: (mp.setattr(_hip, 'default_context', lambda *a, **k: (_ for _ in ()).throw(_hip.WbxUnavailableError('none'))), _pair())[1],
    'no entry point': lambda mp: (mp.setattr(engine, 'fss_thresholds_available', lambda ctx: False), _pair())[1],
    'no FSS entry point': lambda mp: (mp.setattr(engine, 'fss_available', lambda ctx: False), _pair())[1],
    'another transform': lambda mp: _pair() + ([1, 3], wrappers.EnsembleMean('both', 'time')),
    'a subclass of the transform': lambda mp: _pair() + ([1, 3], _OtherBinary('both', [0.1, 0.5], THR)),
    'predictions only': lambda mp: _pair() + ([1, 3], _transform(which='predictions')),
    'targets only': lambda mp: _pair() + ([1, 3], _transform(which='targets')),
    'labelled thresholds': lambda mp: _pair() + ([1, 3], _transform(_labelled_thresholds(), unique_name_suffix='x')),
    'thresholds that are no numbers': lambda mp: _pair() + ([1, 3], _transform(['a', 'b'])),
    'the threshold dim on the predictions': lambda mp: _pair() + ([1, 3], _transform(dim='time')),
    'the threshold dim on the targets alone': lambda mp: (_pair()[0], _pair()[1].rename({'time': THR})),
    'float16': lambda mp: _pair(dtype=np.float16),
    'integers': lambda mp: _pair(dtype=np.int32),
    'dtypes differ': lambda mp: _pair(t_dtype=np.float64),
    'frames differ': lambda mp: (_pair()[0], _pair(shape=(3, 9, 11))[1]),
    'labels differ': lambda mp: (_pair()[0], _pair()[1].assign_coords(latitude=np.arange(9.0) + 1)),
    'a dim the targets lack': lambda mp: (_pair()[0], _pair()[1].isel(time=0, drop=True)),
    'no latitude': lambda mp: _pair(dims=('time', 'y', 'longitude')),
    'longitude not innermost': lambda mp: _pair(shape=(2, 11, 9), dims=('time', 'longitude', 'latitude')),
    'more than 2048 longitudes': lambda mp: _pair(shape=(1, 3, 2049)),
    'a size below 1': lambda mp: _pair() + (-3,),
    'a size above the field': lambda mp: _pair() + ([3, 11],),
    'an even size': lambda mp: _pair() + (4,),
    'a generator of sizes': lambda mp: _pair() + ((n for n in (1, 3)),),
}


@pytest.mark.parametrize('why', list(DECLINES))
def test_the_gate_declines_and_never_raises(monkeypatch, device, why):
  got = DECLINES[why](monkeypatch)
  p, t = got[:2]
  sizes = got[2] if len(got) > 2 else [1, 3]
  transform = got[3] if len(got) > 3 else _transform()
  assert spatial.SquaredFractionsError(sizes).compute_with_transform(transform, {'v': p}, {'v': t}) is None, why


def test_a_declined_case_is_the_route_before_the_entry(monkeypatch, device):
  """WrappedStatistic.compute falls through to transform-and-compute: with the switch off the statistic sees the binarised fields, the
  threshold dim in their frame, as before; an even size raises as before."""
  p, t = _pair()
  wrapped = wrappers.WrappedStatistic(spatial.SquaredFractionsError([1, 3]), _transform())
  on = wrapped.compute({'v': p}, {'v': t})['v']
  monkeypatch.setattr(lazy, 'FUSED_FSS_THRESHOLDS', False)
  off = wrapped.compute({'v': p}, {'v': t})['v']
  assert on.threshold_dim == THR and THR not in on._group.dims  # pylint: disable=protected-access
  assert getattr(off, 'threshold_dim', None) is None  # (a LazyFSS of the binarised fields where their layout allows, else an array)
  assert tuple(on.dims) == tuple(off.dims)
  assert FC.same_numbers(np.asarray(on.values, np.float64), np.asarray(off.values, np.float64))
  with pytest.raises(ValueError, match='must be odd'):
    wrappers.WrappedStatistic(spatial.SquaredFractionsError(4), _transform()).compute({'v': p}, {'v': t})


# ---- labels -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('sizes', [3, [1, 3, 5]], ids=['scalar', 'list'])
def test_fused_objects_are_labelled_like_the_host_routes(monkeypatch, device, sizes):
  p, t = _pair(dims=('latitude', 'time', 'longitude'), shape=(9, 2, 11), mask=True)
  values = [0.5, 0.1, 0.75]
  for cls in CLASSES:
    wrapped = wrappers.WrappedStatistic(cls(sizes, wrap_longitude=True), _transform(values))
    fused = wrapped.compute({'v': p}, {'v': t})['v']
    monkeypatch.setattr(lazy, 'FUSED_FSS', False)
    host = wrapped.compute({'v': p}, {'v': t})['v']
    monkeypatch.setattr(lazy, 'FUSED_FSS', True)
    assert isinstance(fused, lazy.LazyFSS) and not isinstance(host, lazy.LazyFSS) and fused.name == host.name == 'v'
    lead = ('neighborhood_size',) if isinstance(sizes, list) else ()
    assert tuple(fused.dims) == tuple(host.dims) == lead + ('time', THR, 'latitude', 'longitude')
    assert tuple(fused.shape) == tuple(host.shape) and fused.dtype == host.dtype == np.float32
    assert set(fused.coords) == set(host.coords) and 'mask' in fused.coords and THR in fused.coords
    for k in host.coords:
      assert tuple(fused.coords[k].dims) == tuple(host.coords[k].dims), k
      np.testing.assert_array_equal(np.asarray(fused.coords[k].values), np.asarray(host.coords[k].values))
    assert THR not in fused.coords['mask'].dims  # one mask for every threshold
    assert FC.same_numbers(np.asarray(fused.values, np.float64), np.asarray(host.values, np.float64))  # `.values`: the host route's array


def test_float64_inputs_at_size_one_are_float32_behind_the_transform(device):
  p, t = _pair(dtype=np.float64)
  out = spatial.SquaredFractionsError([1, 3]).compute_with_transform(_transform(), {'v': p}, {'v': t})['v']
  assert out.dtype == np.float32 == out.values.dtype  # (binarised fields are float32 whatever the inputs are)


def test_the_three_terms_of_one_fss_share_a_group(device):
  p, t = _pair()
  metric = wrappers.WrappedMetric(spatial.FSS([1, 3], wrap_longitude=True), [_transform()])
  stats = metrics_base.compute_unique_statistics_for_all_metrics({'fss': metric}, {'v': p}, {'v': t})
  outs = [s['v'] for s in stats.values()]
  assert len(outs) == 3 and all(isinstance(o, lazy.LazyFSS) and o.threshold_dim == THR for o in outs)
  assert len({id(o._group) for o in outs}) == 1 and sorted(o._cell for o in outs) == [0, 1, 2]  # pylint: disable=protected-access
  other = spatial.SquaredFractionsError([1, 3], wrap_longitude=True).compute_with_transform(_transform([0.1, 0.6]), {'v': p}, {'v': t})['v']
  assert other._group is not outs[0]._group  # pylint: disable=protected-access
  binary = spatial.SquaredFractionsError([1, 3], wrap_longitude=True).compute({'v': p}, {'v': t})['v']
  assert binary._group is not outs[0]._group and binary.threshold_dim is None  # pylint: disable=protected-access


# ---- the group's reduction under a stand-in for the launch -------------------------------------------------------------------

def _stand_in(calls):
  """engine.reduce_statistics of kind 'fss' as far as the lane bookkeeping goes: every reduced dim gone, the value of lane 3 j + term
  of a call at size n and thresholds a_j is 1000 n + 10 term + a_j, its count n + a_j."""
  def reduce_statistics(kind, inputs, dims, sizes, reduce_dims, w_da, bin_dims, mask=None, skipna=False, cat=None, **kw):
    assert kind == 'fss'
    calls.append(dict(cat, mask=mask))
    thr = np.asarray(cat['thresholds'], np.float64)
    assert 1 <= thr.size <= _hip.FSS_THR_MAX
    out_dims = tuple(d for d in dims if d not in set(reduce_dims))
    shape = tuple(sizes[d] for d in out_dims)
    lanes = np.array([1000.0 * cat['n'] + 10 * term + a for a in thr for term in range(3)])
    counts = np.array([cat['n'] + a for a in thr for term in range(3)])
    full = lambda v: np.broadcast_to(v.reshape((-1,) + (1,) * len(shape)), (v.size,) + shape).copy()
    return full(lanes), full(counts), out_dims
  return reduce_statistics


@pytest.mark.parametrize('nthr', [3, 16, 17, 37])
@pytest.mark.parametrize('sizes', [5, [5], [1, 3, 5]], ids=['scalar', 'list_of_one', 'list'])
def test_lanes_of_every_call_land_at_their_size_and_threshold(monkeypatch, device, sizes, nthr):
  """One call per size and block of at most 16 thresholds; the Aggregator's result has the host route's dims and coordinates, and
  every (term, size, threshold) holds the number its call wrote -- joined on the host, or one call's lanes taken as they are."""
  calls = []
  monkeypatch.setattr(engine, 'reduce_statistics', _stand_in(calls))
  values = [round(0.01 * (j + 1), 2) for j in range(nthr)]
  p, t = _pair(mask=True)
  metric = wrappers.WrappedMetric(spatial.FSS(sizes, wrap_longitude=True), [_transform(values)])
  stats = metrics_base.compute_unique_statistics_for_all_metrics({'fss': metric}, {'v': p}, {'v': t})
  for keep in ((), ('time',)):
    calls.clear()
    agg = aggregation.Aggregator(reduce_dims=[d for d in DIMS if d not in keep], masked=True)
    state = agg.aggregate_statistics(stats)
    size_list = sizes if isinstance(sizes, list) else [sizes]
    blocks = -(-nthr // _hip.FSS_THR_MAX)
    assert len(calls) == len(size_list) * blocks  # the three terms share them
    assert [c['n'] for c in calls] == [n for n in size_list for _ in range(blocks)]
    assert all(c['mask'] is not None and THR not in c['mask'].dims and 'neighborhood_size' not in c['mask'].dims for c in calls)
    assert sum(len(c['thresholds']) for c in calls) == nthr * len(size_list)
    for name, per_var in state.sum_weighted_statistics.items():
      term = TERMS.index(name.split('_')[0])
      got, cnt = per_var['v'], state.sum_weights[name]['v']
      lead = ('neighborhood_size',) if isinstance(sizes, list) else ()
      assert tuple(got.dims) == lead + keep + (THR,) == tuple(cnt.dims)
      np.testing.assert_array_equal(np.asarray(got.coords[THR].values), values)
      want = np.array([[1000.0 * n + 10 * term + a for a in values] for n in size_list])
      wcnt = np.array([[n + a for a in values] for n in size_list])
      g, c = np.asarray(got.values), np.asarray(cnt.values)
      if keep:
        g, c = np.moveaxis(g, -2, 0)[0], np.moveaxis(c, -2, 0)[0]
      np.testing.assert_array_equal(g.reshape(want.shape), want)
      np.testing.assert_array_equal(c.reshape(want.shape), wcnt)


# ---- what the threshold dim declines at the Aggregator ---------------------------------------------------------------------

def test_a_threshold_dim_that_is_reduced_weighted_or_binned_takes_the_host_route_and_is_counted(monkeypatch, device):
  class ThresholdWeights(weighting.Weighting):
    def weights(self, statistic):
      return xr.DataArray(np.arange(1.0, 3.0), dims=(THR,))
  ThresholdWeights.__module__ = weighting.__name__

  class ThresholdBins(binning.Binning):
    def create_bin_mask(self, statistic):
      return xr.DataArray(np.eye(2, dtype=bool), dims=('which', THR), coords={'which': [0, 1]})
  ThresholdBins.__module__ = binning.__name__
  monkeypatch.setattr(engine, 'reduce_statistics', lambda *a, **k: pytest.fail('a launch'))
  p, t = _pair()
  stat = spatial.SquaredFractionsError(3).compute_with_transform(_transform(), {'v': p}, {'v': t})['v']
  assert stat.launchable()
  for how, reduce_dims, kw in (('reduced', list(DIMS) + [THR], {}),
                               ('weighted or binned', list(DIMS), dict(weigh_by=[ThresholdWeights()])),
                               ('weighted or binned', list(DIMS), dict(bin_by=[ThresholdBins('which')]))):
    monkeypatch.setattr(lazy, 'FSS_STATS', {'plan_declined': 0, 'reasons': []})
    agg = aggregation.Aggregator(reduce_dims=reduce_dims, **kw)
    assert agg._try_contingency(stat, set(reduce_dims), False, False) is None, kw  # pylint: disable=protected-access
    assert lazy.FSS_STATS['plan_declined'] == 1 and how in lazy.FSS_STATS['reasons'][0] and THR in lazy.FSS_STATS['reasons'][0]
  # a reduced size dim is no business of the threshold's, and a binary statistic counts nothing here
  monkeypatch.setattr(lazy, 'FSS_STATS', {'plan_declined': 0, 'reasons': []})
  many = spatial.SquaredFractionsError([1, 3]).compute_with_transform(_transform(), {'v': p}, {'v': t})['v']
  assert aggregation.Aggregator(reduce_dims=['neighborhood_size'])._try_contingency(many, {'neighborhood_size'}, False, False) is None  # pylint: disable=protected-access
  assert lazy.FSS_STATS['plan_declined'] == 0


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

def test_abi_constants():
  header = open(os.path.join(ROOT, 'include', 'wbx.h')).read()
  assert re.search(r'#define WBX_ABI_VERSION 13\b', header)
  assert re.search(r'WBX_FN_FSS_THRESHOLD_PARTIAL = 30\b', header) and _hip.FN_IDS['wbx_fss_threshold_partial'] == 30
  assert len(set(_hip.FN_IDS.values())) == len(_hip.FN_IDS)
  assert re.search(r'#define WBX_FSS_THR_MAX 16\b', header) and _hip.FSS_THR_MAX == 16 == TC.THR_MAX
  replay_src = open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_replay.hip')).read()
  assert 'WBX_REPLAY_CASE(WBX_FN_FSS_THRESHOLD_PARTIAL, wbx_fss_threshold_partial)' in replay_src
  assert 'wbx_fss_threshold_partial' in _hip.EXPORTED_SYMBOLS
  proto = re.search(r'int wbx_fss_threshold_partial\(([^;]*)\);', header).group(1)
  assert len(re.sub(r'/\*.*?\*/', '', proto).split(',')) == 10 <= _hip.CALL_MAX_ARGS
  kernel_src = open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_fss_thresholds.hip')).read()
  assert re.search(rf'constexpr int FSS_KB = {TC.KB};', kernel_src)
  assert 'wbx_fss_thresholds.hip' in open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'Makefile')).read()


def test_the_library_exports_the_entry_with_its_prototype():
  lib = _hip.load_library()
  assert lib.wbx_abi_version() == 13
  assert len(_hip.PROTOS['wbx_fss_threshold_partial']) == 10
  assert getattr(lib, 'wbx_fss_threshold_partial', None) is not None
