"""The fused FSS route without a device: the restatement of tests/fss_cases.py against the host route and the oracle, the plan of
wbx_fss_partial, the gate of `_FractionStatistic._fused`, the ABI constants, and the labels of the fused route's objects."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fss_cases as FC
from oracle import wbx_oracle as O
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import planner
from weatherbenchx_amd import weighting
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import spatial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = ('time', 'latitude', 'longitude')
ULP32 = lambda f: 2.0 ** -23 * np.maximum(np.abs(f), 2.0 ** -126)  # at least one ulp of float32 at |f|


# ---- the restatement ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('payload', ['numpy', 'torch'])
def test_restated_fractions_against_the_host_route(payload, dtype):
  """NaN placement identical, values within 1 ulp of float32 everywhere; on 0 / 1 fields the number of points that differ AT ALL is
  zero at every tested shape, size and wrap setting (the shapes of the GPU tests and of the API tests' chunk loop)."""
  torch = pytest.importorskip('torch') if payload == 'torch' else None
  points = differing = 0
  for i, (nlat, nlon) in enumerate(FC.SHAPES + ((12, 16),)):
    for kind in ('indicator', 'indicator_nan', 'gaussian'):
      shape = (2, nlat, nlon)
      if kind == 'gaussian':
        x = FC.gaussian_fields(shape, dtype, 20 + i)[0]
        x[np.random.default_rng(i).random(shape) < 0.05] = np.nan
      else:
        x = FC.indicator_fields(shape, dtype, 60 + i, nan_share=0.08 if kind == 'indicator_nan' else 0.0)[i % 2]
      for n in FC.sizes_for(nlat, nlon):
        for wrap in (False, True):
          want = FC.fractions(x, n, wrap)
          arg = torch.from_numpy(x.copy()) if torch is not None else x.copy()
          got = spatial.convolve2d_wrap_longitude(arg, n, wrap)
          got = got.numpy() if torch is not None else np.asarray(got)
          assert got.dtype == want.dtype == (x.dtype if n == 1 else np.float32)
          np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
          ok = ~np.isnan(want)
          assert (np.abs(got[ok].astype(np.float64) - want[ok]) <= ULP32(want[ok])).all(), (nlat, nlon, n, wrap, kind)
          if kind != 'gaussian':
            points += int(ok.sum())
            differing += int((got[ok] != want[ok]).sum())
  print(f'0 / 1 fields: {differing} of {points} fractions differ between the restatement and the host route')
  assert points > 100000 and differing == 0


@pytest.mark.parametrize('seed', range(4))
def test_restated_fractions_against_the_oracle(seed):
  rng = np.random.default_rng(300 + seed)
  nlat, nlon = int(rng.integers(5, 12)), int(rng.integers(5, 14))
  x = rng.normal(size=(2, nlat, nlon))
  x[rng.random(x.shape) < 0.08] = np.nan
  for n in (3, 5):
    for wrap in (False, True):
      want = np.stack([O.neighborhood_mean(f, n, wrap) for f in x])
      got = FC.fractions(x, n, wrap)
      np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
      np.testing.assert_allclose(got, want, atol=2e-6, equal_nan=True)  # (the tolerance tests/test_spatial.py holds the host route to)


def test_restated_lanes_and_partials():
  p, t = FC.indicator_fields((2, 3, 9, 11), np.float32, 1, nan_share=0.1)
  v = FC.point_values(p, t, 3, True)
  pf, tf = FC.fractions(p, 3, True), FC.fractions(t, 3, True)
  assert v.shape == (3, 2, 3, 9, 11) and v.dtype == np.float64
  assert FC.same_numbers(v[1], (pf * pf).astype(np.float64)) and FC.same_numbers(v[0], ((pf - tf) * (pf - tf)).astype(np.float64))
  assert (v[:, :, :, 0] == 0).all() and (v[:, :, :, -1] == 0).all()  # border rows are 0 whatever the window holds
  assert np.isnan(v[1]).any() and (np.isnan(v[1]) & ~np.isnan(v[2])).any()  # lane 1 does not depend on t's NaNs
  mask = (np.arange(99).reshape(9, 11) % 3 != 0).astype(np.uint8)
  for flags, nl in ((0, 3), (1, 4), (2, 6), (3, 6)):
    want, mag, nterm = FC.partials(v, mask, flags, 2, False)
    assert want.shape == (2, 9, 2, nl, 1) and mag.shape == nterm.shape == (2, 9, 2, 3, 1)
    assert (nterm[:, :, 0] == 22).all() and (nterm[:, :, 1] == 11).all()  # a ragged last chunk
  want, _, _ = FC.partials(v, mask, 3, 2, True)
  assert want.shape == (2, 9, 2, 6, 11) and (want[:, :, :, 3:, :][:, :, :, :, mask[0] == 0][:, 0] == 0).all()
  d64 = FC.point_values(p.astype(np.float64) * 0.1, t.astype(np.float64), 1, False)  # n == 1 stays in the input type
  assert FC.same_numbers(d64[1], (p.astype(np.float64) * 0.1) ** 2)


# ---- the plan -----------------------------------------------------------------------------------------------------------------

def _lay(dims, shape, itemsize=4):
  st, step = {}, 1
  for d, n in zip(reversed(dims), reversed(shape)):
    st[d] = step
    step *= n
  return planner.InputLayout(strides=st, itemsize=itemsize)


def test_the_plan_puts_latitude_last_among_the_keys():
  dims = ('latitude', 'level', 'time', 'longitude')  # stored latitude-outermost
  sizes = dict(zip(dims, (7, 2, 3, 16)))
  lay = _lay(dims, (7, 2, 3, 16))
  mlay = _lay(('latitude', 'longitude'), (7, 16), 1)
  fp = planner.build_fss_plan(dims, sizes, [lay, lay, mlay], ['time', 'latitude', 'longitude'], wdep_dims=(), flags=1, wrap_longitude=True)
  s1 = fp.s1
  assert s1.key_dims == ('level', 'latitude') and s1.depth_dims == ('time',) and s1.x_dim == 'longitude' and not fp.x_kept
  assert (fp.nkey, fp.ndepth, fp.nlat, fp.nlon) == (2, 3, 7, 16) and s1.nkey == 14 and s1.nx == 16
  assert (s1.nchunk, s1.depth_chunk) == (fp.nchunk, fp.depth_chunk) and fp.nchunk * fp.depth_chunk >= 3
  np.testing.assert_array_equal(fp.key_off[0], [0, 48])
  np.testing.assert_array_equal(fp.depth_off[0], [0, 16, 32])
  assert fp.lat_stride == [96, 96, 16] and fp.lon_stride == [1, 1, 1]
  assert fp.key_off[2] is None and fp.depth_off[2] is None  # a (latitude, longitude) mask: two strides and no tables
  assert s1.partial_shape(4) == (2, 1, 7, fp.nchunk, 4, 1)  # A = level, Br = latitude: stage 2 sums latitude under its weights
  # weights on latitude, longitude in the bins: x kept
  fp = planner.build_fss_plan(dims, sizes, [lay, lay, None], ['time', 'latitude', 'longitude'], wdep_dims=('latitude', 'longitude'))
  assert fp.x_kept and fp.s1.sum_j and fp.s1.key_dims == ('level', 'latitude')
  # latitude kept, nothing reduced among the weights' dims: Bk
  fp = planner.build_fss_plan(dims, sizes, [lay, lay, None], ['time', 'longitude'], wdep_dims=('latitude',))
  assert fp.s1.bk_dims == ('latitude',) and fp.s1.a_dims == ('level',) and not fp.s1.br_dims


def test_the_plan_declines_latitude_kept_under_weights_on_a_reduced_dim():
  dims = ('time', 'latitude', 'longitude')
  sizes = dict(zip(dims, (3, 7, 16)))
  lay = _lay(dims, (3, 7, 16))
  with pytest.raises(planner.FssPlanError, match='last key dim'):
    planner.build_fss_plan(dims, sizes, [lay, lay, None], ['time', 'longitude'], wdep_dims=('time',))
  with pytest.raises(planner.FssPlanError, match='lacks'):
    planner.build_fss_plan(('time', 'longitude'), {'time': 3, 'longitude': 16}, [None, None, None], ['time'])


def test_band_rows_follow_the_headers_rule():
  assert _hip.fss_band_rows(1, 1, 43, 3) == 8 and _hip.fss_band_rows(1, 1, 43, 5) == 8 and _hip.fss_band_rows(1, 1, 43, 7) == 16
  assert _hip.fss_band_rows(1, 1, 43, 23) == 64
  assert _hip.fss_band_rows(1, 6, 721, 3) == 8 and _hip.fss_band_rows(4096, 1, 721, 3) == 64


# ---- the gate -----------------------------------------------------------------------------------------------------------------

class _FakeContext:
  device_id = 0


@pytest.fixture
def device(monkeypatch):
  """A launch context that exists and has the entry point, as far as the gate asks."""
  monkeypatch.setattr(lazy, 'FUSED_FSS', True)
  monkeypatch.setattr(_hip, 'default_context', lambda *a, **k: _FakeContext())
  monkeypatch.setattr(engine, 'fss_available', lambda ctx: True)


def _pair(shape=(2, 9, 11), dims=DIMS, dtype=np.float32, t_dtype=None, seed=3, mask=False):
  p, t = FC.indicator_fields(shape, dtype, seed)
  cs = {d: np.arange(n, dtype=np.float64) for d, n in zip(dims, shape)}
  tc = dict(cs)
  if mask:
    tc['mask'] = (dims, np.random.default_rng(seed).random(shape) > 0.2)
  return xr.DataArray(p, dims=dims, coords=cs), xr.DataArray(t.astype(t_dtype or dtype), dims=dims, coords=tc)


def test_the_gate_takes_what_the_kernel_serves(device):
  for sizes in (3, [1, 3, 5], (3, 9), np.array([1, 9])):
    for cls in (spatial.SquaredFractionsError, spatial.SquaredPredictionFraction, spatial.SquaredTargetFraction):
      for dtype in (np.float32, np.float64):
        p, t = _pair(dtype=dtype)
        out = cls(sizes, wrap_longitude=True)._fused(p, t)  # pylint: disable=protected-access
        assert isinstance(out, lazy.LazyFSS) and out.is_lazy and out._cell == lazy.FSS_TERM[cls.__name__]  # pylint: disable=protected-access


DECLINES = {
    'switch off': lambda mp: (mp.setattr(lazy, 'FUSED_FSS', False), _pair())[1],
    'no device': lambda mp: (mp.setattr(_hip, 'default_context', lambda *a, **k: (_ for _ in ()).throw(_hip.WbxUnavailableError('none'))), _pair())[1],
    'no entry point': lambda mp: (mp.setattr(engine, 'fss_available', lambda ctx: False), _pair())[1],
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
    'a generator of sizes': lambda mp: _pair() + ((n for n in (1, 3)),),
}


@pytest.mark.parametrize('why', list(DECLINES))
def test_the_gate_declines(monkeypatch, device, why):
  got = DECLINES[why](monkeypatch)
  p, t = got[:2]
  sizes = got[2] if len(got) > 2 else [1, 3]
  assert spatial.SquaredFractionsError(sizes)._fused(p, t) is None, why  # pylint: disable=protected-access


def test_an_even_size_raises_as_before(device):
  p, t = _pair()
  for sizes in (4, [3, 4]):
    with pytest.raises(ValueError, match='must be odd'):
      spatial.SquaredFractionsError(sizes).compute({'v': p}, {'v': t})


def test_a_weighting_or_binning_from_outside_the_package_keeps_the_host_route(device):
  from weatherbenchx_amd import binning  # pylint: disable=g-import-not-at-top

  class MyWeights(weighting.Weighting):
    def weights(self, statistic):
      return xr.DataArray(np.ones(9), dims=('latitude',))

  class MyBins(binning.Binning):
    def create_bin_mask(self, statistic):
      return xr.DataArray(np.ones((2, 9), bool), dims=('half', 'latitude'), coords={'half': [0, 1]})
  p, t = _pair()
  stat = spatial.SquaredFractionsError(3)._fused(p, t)  # pylint: disable=protected-access
  assert stat.launchable()
  for kw in (dict(weigh_by=[MyWeights()]), dict(bin_by=[MyBins('half')]), dict(weigh_by=[weighting.GridAreaWeighting()], bin_by=[MyBins('half')])):
    agg = aggregation.Aggregator(reduce_dims=list(DIMS), **kw)
    assert agg._try_contingency(stat, set(DIMS), False, False) is None, kw  # pylint: disable=protected-access


def test_a_reduction_the_plan_declines_is_counted(monkeypatch, device):
  """latitude kept while the weights depend on a reduced dim: the Aggregator's fused route gives way to the host route and
  lazy.FSS_STATS says so."""
  class TimeWeights(weighting.Weighting):
    def weights(self, statistic):
      return xr.DataArray(np.arange(1.0, 3.0), dims=('time',))
  TimeWeights.__module__ = weighting.__name__
  monkeypatch.setattr(lazy, 'FSS_STATS', {'plan_declined': 0, 'reasons': []})

  def refuse(*a, **k):  # (what engine.reduce_statistics('fss') raises for this reduction, without a device)
    p, t = _pair()
    lay = lazy.payload_layout(p)
    planner.build_fss_plan(p.dims, dict(p.sizes), [lay, lay, None], ['time', 'longitude'], wdep_dims=('time',))
  p, t = _pair()
  stat = spatial.SquaredFractionsError(3)._fused(p, t)  # pylint: disable=protected-access
  monkeypatch.setattr(stat._group, 'reduce', refuse)  # pylint: disable=protected-access
  agg = aggregation.Aggregator(reduce_dims=['time', 'longitude'], weigh_by=[TimeWeights()])
  assert agg._try_contingency(stat, {'time', 'longitude'}, False, False) is None  # pylint: disable=protected-access
  assert lazy.FSS_STATS['plan_declined'] == 1 and 'last key dim' in lazy.FSS_STATS['reasons'][0]


# ---- labels -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('sizes', [3, [1, 3, 5]], ids=['scalar', 'list'])
def test_fused_objects_are_labelled_like_the_host_routes(monkeypatch, device, sizes):
  p, t = _pair(dims=('latitude', 'time', 'longitude'), shape=(9, 2, 11), mask=True)
  for cls in (spatial.SquaredFractionsError, spatial.SquaredPredictionFraction, spatial.SquaredTargetFraction):
    stat = cls(sizes, wrap_longitude=True, combine_mask=False)
    fused = stat.compute({'v': p}, {'v': t})['v']
    monkeypatch.setattr(lazy, 'FUSED_FSS', False)
    host = stat.compute({'v': p}, {'v': t})['v']
    monkeypatch.setattr(lazy, 'FUSED_FSS', True)
    assert isinstance(fused, lazy.LazyFSS) and not isinstance(host, lazy.LazyFSS)
    assert stat.unique_name == f'{cls.__name__}_{spatial.get_suffix(sizes, True)}'
    assert tuple(fused.dims) == tuple(host.dims) and tuple(fused.shape) == tuple(host.shape) and fused.dtype == host.dtype
    assert set(fused.coords) == set(host.coords) and 'mask' in fused.coords
    for k in host.coords:
      assert tuple(fused.coords[k].dims) == tuple(host.coords[k].dims), k
      np.testing.assert_array_equal(np.asarray(fused.coords[k].values), np.asarray(host.coords[k].values))
    assert np.asarray(fused.coords['mask'].values).dtype == bool
    assert FC.same_numbers(np.asarray(fused.values, np.float64), np.asarray(host.values, np.float64))  # `.values`: the host route's array


def test_the_three_terms_of_one_fss_share_a_group(device):
  p, t = _pair()
  stats = spatial.FSS([1, 3], wrap_longitude=True).statistics
  outs = [s.compute({'v': p}, {'v': t})['v'] for s in stats.values()]
  assert len({id(o._group) for o in outs}) == 1 and sorted(o._cell for o in outs) == [0, 1, 2]  # pylint: disable=protected-access
  other = spatial.SquaredFractionsError([1, 3], wrap_longitude=False).compute({'v': p}, {'v': t})['v']
  assert other._group is not outs[0]._group  # pylint: disable=protected-access


def test_torch_payloads_stay_tensors_on_the_fused_object(device):
  torch = pytest.importorskip('torch')
  p, t = _pair()
  tp = xr.DataArray(torch.from_numpy(np.asarray(p.values)), dims=DIMS)
  tt = xr.DataArray(torch.from_numpy(np.asarray(t.values)), dims=DIMS)
  out = spatial.SquaredFractionsError([1, 3]).compute({'v': tp}, {'v': tt})['v']
  assert isinstance(out, lazy.LazyFSS) and xr._is_torch(out.data) and out.dims == ('neighborhood_size',) + DIMS  # pylint: disable=protected-access


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

def test_abi_constants():
  header = open(os.path.join(ROOT, 'include', 'wbx.h')).read()
  assert re.search(r'#define WBX_ABI_VERSION 13\b', header)
  assert re.search(r'WBX_FN_FSS_PARTIAL = 28\b', header) and _hip.FN_IDS['wbx_fss_partial'] == 28
  assert re.search(r'#define WBX_FSS_LANES 3\b', header) and _hip.FSS_LANES == 3 == len(lazy.FSS_TERM)
  assert re.search(r'#define WBX_FSS_MAX_NLON 2048\b', header) and _hip.FSS_MAX_NLON == 2048
  for name, value in (('MAX_BAND_ROWS', _hip.FSS_MAX_BAND_ROWS), ('MIN_BAND_ROWS', _hip.FSS_MIN_BAND_ROWS), ('TARGET_BLOCKS', _hip.FSS_TARGET_BLOCKS)):
    assert re.search(rf'#define WBX_FSS_{name} {value}\b', header)
  replay_src = open(os.path.join(ROOT, 'weatherbenchx_amd', 'csrc', 'wbx_replay.hip')).read()
  assert 'WBX_REPLAY_CASE(WBX_FN_FSS_PARTIAL, wbx_fss_partial)' in replay_src
  assert 'wbx_fss_partial' in _hip.EXPORTED_SYMBOLS
  proto = re.search(r'int wbx_fss_partial\(([^;]*)\);', header).group(1)
  assert len(proto.split(',')) == 8 <= _hip.CALL_MAX_ARGS
  assert C.sizeof(_hip.FssPlanStruct) == 4 * 8 + 2 * 4 + 8 + 4 * 3 * 8 + 2 * 4


def test_the_library_exports_the_entry_with_its_prototype():
  lib = _hip.load_library()
  assert lib.wbx_abi_version() == 13
  assert len(_hip.PROTOS['wbx_fss_partial']) == 8
  assert getattr(lib, 'wbx_fss_partial', None) is not None
