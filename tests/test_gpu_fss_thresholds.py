"""wbx_fss_threshold_partial through the raw C ABI: EVERY partial `partial[key][lat][chunk][lane][j]`, three ways.

1. Against the restatement (tests/fss_threshold_cases.py: tests/fss_cases.py on the binarised fields).  The restated point values ARE
   the kernel's (window sums of 0 / 1 fields are exact in any order), so a partial is bit for bit where its sum is exact -- n = 1
   (every lane a small integer), and any n where x is kept and every field is its own chunk (0.0 + one point) -- and otherwise within
   the first-order bound N 2^-53 sum |v_i| of a float64 sum of N terms, the bound tests/test_gpu_fss.py uses.
2. Against wbx_fss_partial on the uploaded float32 fields (p > thr_k), (t > thr_k) with NaN kept, under the same plan, layout, mask
   and n: bit for bit, every case, lane slice by lane slice -- the contract that makes the two entries interchangeable.
3. Every refusal leaves a sentinel-filled output untouched.

Frames, memory orders (plain, fields interleaved, every other longitude, latitude fastest: strides with key and depth tables) and
masks are those of tests/test_gpu_fss.py, whose helpers this file borrows."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import fss_cases as FC
import fss_threshold_cases as TC
import test_gpu_fss as TG

pytestmark = pytest.mark.gpu
MODES, SDIMS, LAYOUTS, SENTINEL = TG.MODES, TG.SDIMS, TG.LAYOUTS, TG.SENTINEL
LISTS = list(TC.THRESHOLD_LISTS.values())


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def launch(ctx, p, t, thresholds, n, wrap, x_kept, depth_chunk, flags, mask=None, how='plain', dtype_code=None, with_mask=True,
           sentinel=None, zero=None, nthr=None, with_thresholds=True, repeat=1):
  """p, t [key, depth, lat, lon] continuous; mask [lat, lon] or [key, depth, lat, lon] (uint8) -> (rc, plan, [partials])."""
  nkey, ndepth, nlat, nlon = p.shape
  sizes = dict(zip(SDIMS, p.shape))
  pv, proot, poff = TG.stored(p, how)
  tv, troot, toff = TG.stored(t, how)
  lay_m = mask_buf = None
  if flags & _hip.FLAG_MASKED:
    m = np.ascontiguousarray(mask, np.uint8)
    lay_m = TG._layout(m, SDIMS[-m.ndim:])  # pylint: disable=protected-access
    mask_buf = ctx.upload(m) if with_mask else None
  reduce_dims = (TG.DEPTH,) if x_kept else (TG.DEPTH, TG.LON)
  fp = planner.build_fss_plan(SDIMS, sizes, [TG._layout(pv, SDIMS), TG._layout(tv, SDIMS), lay_m], reduce_dims, flags=flags & 3,  # pylint: disable=protected-access
                              wrap_longitude=wrap)
  dc = max(1, min(depth_chunk, ndepth))
  fp = dataclasses.replace(fp, depth_chunk=dc, nchunk=-(-ndepth // dc), flags=flags,
                           s1=dataclasses.replace(fp.s1, depth_chunk=dc, nchunk=-(-ndepth // dc)))
  k = len(thresholds)
  shape = (nkey, nlat, fp.nchunk, TC.lanes_total(flags, k), nlon if x_kept else 1)
  if zero:
    fp = dataclasses.replace(fp, **{zero: 0})
  dplan = engine._FssPlanOnDevice(ctx, fp)  # pylint: disable=protected-access
  bufs = [ctx.upload(proot), ctx.upload(troot)]
  thr_buf = ctx.upload(np.asarray(thresholds, np.float64)) if with_thresholds else None
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  size = int(np.prod(shape))
  outs, rc = [], 0
  for _ in range(repeat):
    out = ctx.upload(np.full(size, sentinel, np.float64)) if sentinel is not None else ctx.alloc(size * 8)
    rc = ctx.lib.wbx_fss_threshold_partial(ctx.handle, C.byref(dplan.struct), dtype_code, int(n), k if nthr is None else int(nthr),
                                           TG._ptr(thr_buf), TG._ptr(bufs[0], poff * p.itemsize), TG._ptr(bufs[1], toff * t.itemsize),  # pylint: disable=protected-access
                                           TG._ptr(mask_buf), TG._ptr(out))  # pylint: disable=protected-access
    outs.append(ctx.download(out.ptr, shape, np.float64))
  return rc, fp, outs


def check_three_ways(ctx, got, p, t, thresholds, n, wrap, mask, flags, depth_chunk, x_kept, how, what):
  k = len(thresholds)
  dc = max(1, min(depth_chunk, p.shape[1]))
  # 1. the restatement
  want, mag, nterm = TC.partials(TC.point_values(p, t, thresholds, n, wrap), mask, flags, dc, x_kept)
  assert got.shape == want.shape, what
  nv = FC.LANES * k
  np.testing.assert_array_equal(got[..., nv:, :], want[..., nv:, :], err_msg=f'{what}: the count lanes')
  g, w = got[..., :nv, :], want[..., :nv, :]
  np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f'{what}: NaN placement')
  if n == 1 or (x_kept and dc == 1):
    assert FC.same_numbers(g, w), f'{what}: bit for bit against the restatement'
  else:
    fin = np.isfinite(w)
    err = np.abs(g[fin] - w[fin])
    assert (nterm * (nterm - 1.0) * FC.U <= 1).all()
    bound = (nterm[fin] + 1) * FC.U * mag[fin]
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
    print(f'{what}: worst |d| / bound = {worst:.3g} over {int(fin.sum())} finite partials')
    assert (err <= bound).all(), f'{what}: worst ratio {worst}'
  # 2. wbx_fss_partial on the binarised fields, slice by slice
  for j, thr in enumerate(thresholds):
    pb, tb = TC.binarized_pair(p, t, thr)
    rc, _, (ref,) = TG.launch(ctx, pb, tb, n, wrap, x_kept, depth_chunk, flags, mask=mask, how=how)
    _hip.check(rc, f'{what}: wbx_fss_partial')
    assert FC.same_numbers(TC.slice_of(got, flags, k, j), ref), f'{what}: threshold {j} ({thr}) against wbx_fss_partial'


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_three_ways(ctx, mode, dtype):
  """Continuous fields with ties, NaN and +-inf at every shape and size: both wrap settings, x summed and kept, nkey, ndepth and nchunk
  above 1 with a ragged last chunk, the four memory orders in rotation and two of the six threshold lists per case."""
  flags = MODES[mode]
  turn = 0
  seen = set()
  for i, (nlat, nlon) in enumerate(TC.SHAPES):
    nkey, ndepth = (2, 3) if nlon < TC.WIDE else (1, 2)
    shape = (nkey, ndepth, nlat, nlon)
    rng = np.random.default_rng(100 * i + flags)
    for n in TC.sizes_for(nlat, nlon):
      turn += 1
      wrap, x_kept, how = bool(turn & 1), bool((turn >> 1) & 1), LAYOUTS[(turn + turn // 4) % 4]
      depth_chunk = 2 if turn % 3 else ndepth  # 3 fields in chunks of 2: a ragged last chunk
      mask = TG._mask_for(rng, shape, per_point=bool((turn // 3) & 1))  # pylint: disable=protected-access
      first = (turn + turn // 8 + i) % len(LISTS)
      for thresholds in (LISTS[first], LISTS[(first + len(LISTS) // 2) % len(LISTS)]):  # two of the lists per case
        p, t = TC.continuous_fields(shape, dtype, 13 * i + flags + n, thresholds)
        what = (f'{nlat}x{nlon} n={n} K={len(thresholds)} wrap={wrap} x_kept={x_kept} {how} chunk={depth_chunk} {mode} '
                f'{np.dtype(dtype).name}')
        rc, _, (got,) = launch(ctx, p, t, thresholds, n, wrap, x_kept, depth_chunk, flags, mask=mask, how=how)
        _hip.check(rc, what)
        check_three_ways(ctx, got, p, t, thresholds, n, wrap, mask, flags, depth_chunk, x_kept, how, what)
        seen.add((len(thresholds), x_kept, wrap))
  assert {k for k, _, _ in seen} == set(TC.THRESHOLD_LISTS) and {(x, w) for _, x, w in seen} == {(a, b) for a in (False, True) for b in (False, True)}


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_every_dim_kept_is_the_point_bit_for_bit(ctx, dtype):
  """x kept and every field its own chunk: a partial is 0.0 + one point, at any n and every list."""
  for i, (nlat, nlon) in enumerate(TC.SHAPES):
    shape = (2, 2, nlat, nlon) if nlon < TC.WIDE else (1, 2, nlat, nlon)
    rng = np.random.default_rng(i)
    for j, n in enumerate(TC.sizes_for(nlat, nlon)):
      thresholds = LISTS[(i + j) % len(LISTS)]
      flags = list(MODES.values())[(i + 2 * j) % 4]
      p, t = TC.continuous_fields(shape, dtype, 50 + i, thresholds)
      mask = TG._mask_for(rng, shape, per_point=bool(j & 1))  # pylint: disable=protected-access
      wrap, how = bool((i + j) & 1), LAYOUTS[(i + j) % 4]
      what = f'every dim kept {nlat}x{nlon} n={n} K={len(thresholds)} flags={flags}'
      rc, _, (got,) = launch(ctx, p, t, thresholds, n, wrap, True, 1, flags, mask=mask, how=how)
      _hip.check(rc, what)
      check_three_ways(ctx, got, p, t, thresholds, n, wrap, mask, flags, 1, True, how, what)


def test_ties_nan_and_infinite_thresholds(ctx):
  """What the fields are built to hold, said once: a point equal to a threshold does not exceed it, float32(0.1) exceeds 0.1, a NaN
  threshold is never exceeded, +inf exceeds everything but +inf and NaN, -inf exceeds nothing."""
  x = np.array([0.5, np.float32(0.1), np.inf, -np.inf, np.nan, 0.75, 0.0, -0.0, 1.0], np.float32)
  p = np.tile(x, (1, 1, 1, 1))  # [1, 1, 1, 9]
  t = np.zeros_like(p)
  thresholds = [0.5, 0.1, float('nan'), float('inf'), float('-inf'), 0.0]
  rc, _, (got,) = launch(ctx, p, t, thresholds, 1, False, True, 1, 0)
  _hip.check(rc, 'ties')
  pf2 = got[0, 0, 0, 1::3, :]  # lane 3 k + 1 = Pf^2 = the indicator
  nan = np.nan
  np.testing.assert_array_equal(pf2, np.array([
      [0, 0, 1, 0, nan, 1, 0, 0, 1],    # > 0.5
      [1, 1, 1, 0, nan, 1, 0, 0, 1],    # > 0.1: float32(0.1) does
      [0, 0, 0, 0, nan, 0, 0, 0, 0],    # > NaN
      [0, 0, 0, 0, nan, 0, 0, 0, 0],    # > +inf
      [1, 1, 1, 0, nan, 1, 1, 1, 1],    # > -inf
      [1, 1, 1, 0, nan, 1, 0, 0, 1],    # > 0: neither zero does
  ], np.float64))
  p64 = p.astype(np.float64)
  p64[0, 0, 0, 1] = 0.1  # the float64 0.1 does not exceed 0.1
  rc, _, (got,) = launch(ctx, p64, t.astype(np.float64), thresholds, 1, False, True, 1, 0)
  _hip.check(rc, 'ties float64')
  assert got[0, 0, 0, 3 * 1 + 1, 1] == 0.0 and got[0, 0, 0, 3 * 1 + 1, 0] == 1.0


def test_two_calls_of_one_case_are_bit_equal(ctx):
  for (nlat, nlon), x_kept, flags, dtype in (((43, 24), False, 0, np.float32), ((5, 300), True, _hip.FLAG_SKIPNA, np.float64),
                                            ((12, 16), False, _hip.FLAG_MASKED, np.float32)):
    shape = (2, 3, nlat, nlon)
    thresholds = TC.THRESHOLD_LISTS[TC.NAN_INF]
    p, t = TC.continuous_fields(shape, dtype, 5, thresholds)
    mask = TG._mask_for(np.random.default_rng(1), shape, True)  # pylint: disable=protected-access
    rc, _, (a, b) = launch(ctx, p, t, thresholds, 3, True, x_kept, 2, flags, mask=mask, repeat=2)
    _hip.check(rc, 'repeat')
    assert a.tobytes() == b.tobytes(), (nlat, nlon)


def test_partials_feed_the_contraction_unchanged(ctx):
  rng = np.random.default_rng(8)
  thresholds = TC.THRESHOLD_LISTS[TC.NAN_INF]
  p, t = TC.continuous_fields((2, 3, 9, 11), np.float32, 31, thresholds, nan_share=0.0)
  p, t = np.nan_to_num(p, posinf=2.0, neginf=-2.0), np.nan_to_num(t, posinf=2.0, neginf=-2.0)
  nv = FC.LANES * len(thresholds)
  for x_kept in (True, False):
    nkey, ndepth, nlat, nlon = p.shape
    rc, fp, (got,) = launch(ctx, p, t, thresholds, 1, False, x_kept, 2, _hip.FLAG_SKIPNA)
    _hip.check(rc, 'partial')
    _, _, nchunk, nlane, nj = got.shape
    n_out = C.c_int64(0)
    sp = engine._PlanOnDevice(ctx, fp.s1)  # pylint: disable=protected-access
    _hip.check(ctx.lib.wbx_s1_partial_len(C.byref(sp.struct), nv, C.byref(n_out)), 'wbx_s1_partial_len')
    assert n_out.value == got.size
    w = rng.integers(1, 9, size=(1, nlat, nj, 2)).astype(np.float64)  # [nBk][nBr][nj][nbin]: latitude is the last key dim
    st = _hip.S2PlanStruct(nkey, 1, nlat, nchunk, nlane, nj, 2, 1)
    res = ctx.alloc(nkey * nlane * 2 * 8)
    _hip.check(ctx.lib.wbx_contract(ctx.handle, C.byref(st), C.c_void_p(ctx.upload(got).ptr), C.c_void_p(ctx.upload(w).ptr),
                                    C.c_void_p(res.ptr)), 'wbx_contract')
    have = ctx.download(res.ptr, (nkey, 1, nlane, 1, 2), np.float64)
    np.testing.assert_array_equal(have[:, 0, :, 0, :], np.einsum('kyclj,yjn->kln', got, w[0]))  # n = 1: small integers, exact


def test_refusals_leave_the_output_untouched(ctx):
  thresholds = TC.THRESHOLD_LISTS[TC.KB]
  p, t = TC.continuous_fields((2, 3, 9, 11), np.float32, 9, thresholds)
  wide = np.zeros((1, 1, 3, 2049), np.float32)
  mask = np.ones((9, 11), np.uint8)
  cases = [
      ('must be odd', p, dict(n=4)),
      ('must be odd', p, dict(n=0)),
      ('must be odd', p, dict(n=-3)),
      ('larger than the field', p, dict(n=11)),  # min(9, 11) = 9
      ('exceeds 2048', wide, dict(n=1)),
      ('unknown dtype', p, dict(dtype_code=7)),
      ('flags other than MASKED', p, dict(flags=_hip.FLAG_FAIR)),
      ('flags other than MASKED', p, dict(flags=_hip.FLAG_SKIPNA_ENS)),
      ('mask is NULL', p, dict(flags=_hip.FLAG_MASKED, with_mask=False)),
      ('thresholds per call', p, dict(nthr=0)),
      ('thresholds per call', p, dict(nthr=-1)),
      ('thresholds per call', p, dict(nthr=_hip.FSS_THR_MAX + 1)),
      ('threshold table is NULL', p, dict(with_thresholds=False)),
  ]
  for message, field, kw in cases:
    kw = dict(kw)
    rc, _, (got,) = launch(ctx, field, field, thresholds, kw.pop('n', 3), True, False, 3, kw.pop('flags', 0), mask=mask,
                           sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message
  rc, _, (got,) = launch(ctx, wide[..., :2048], wide[..., :2048], TC.THRESHOLD_LISTS[_hip.FSS_THR_MAX], 3, True, False, 1, 0,
                         sentinel=SENTINEL)  # 2048 longitudes and 16 thresholds themselves are served
  _hip.check(rc, 'nlon = 2048, 16 thresholds')
  assert not (got == SENTINEL).any()


@pytest.mark.parametrize('mode', list(MODES))
def test_empty_extents_zero_the_partial_and_no_keys_touch_nothing(ctx, mode):
  thresholds = TC.THRESHOLD_LISTS[TC.NAN_INF]
  p, t = TC.continuous_fields((2, 3, 9, 11), np.float32, 4, thresholds)
  mask = np.ones((9, 11), np.uint8)
  for x_kept in (False, True):
    for zero in ('ndepth', 'nlon') if not x_kept else ('ndepth',):
      rc, _, (got,) = launch(ctx, p, t, thresholds, 3, False, x_kept, 3, MODES[mode], mask=mask, sentinel=SENTINEL, zero=zero)
      _hip.check(rc, zero)
      assert (got == 0.0).all() and not np.signbit(got).any(), zero
  rc, _, (got,) = launch(ctx, p, t, thresholds, 3, False, False, 3, MODES[mode], mask=mask, sentinel=SENTINEL, zero='nkey')
  _hip.check(rc, 'nkey == 0')
  assert (got == SENTINEL).all()
