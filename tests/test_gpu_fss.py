"""wbx_fss_partial through the raw C ABI: EVERY partial `partial[key][lat][chunk][lane][j]` against the restatement (tests/fss_cases.py).

Frame (key, depth, lat, lon): p[key, depth, lat, lon] and t likewise, stored in four memory orders -- plain C order, fields interleaved
(the field index fastest: lon stride = nkey * ndepth), every other longitude (lon stride 2) and latitude-fastest.  The mask is either
a (lat, lon) field (two strides and no tables) or one byte per point.

Bit for bit where the restated values sum exactly: 0 / 1 and small-integer fields at n = 1 (every lane is a small integer), and at
any n where x is kept and every field is its own chunk (a partial is 0.0 + one point).  Otherwise a partial lies within the first-order
bound N 2^-53 sum |v_i| of the float64 sum of the restated values -- on 0 / 1 and small-integer fields the kernel's per-point values
ARE the restated ones, the window sums being exact in any order -- and on Gaussian fields within that plus the per-point bounds that
tests/fss_cases.py derives from the header's |dS|."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import fss_cases as FC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked_skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
KEY, DEPTH, LAT, LON = 'key', 'depth', 'latitude', 'longitude'
SDIMS = (KEY, DEPTH, LAT, LON)
LAYOUTS = ('plain', 'interleaved', 'lon2', 'lat_fastest')
SENTINEL = -77.0


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def stored(a, how):
  """`a` [key, depth, lat, lon] as a view of memory in the order `how` -> (view, root array, element offset)."""
  k, d, y, x = a.shape
  if how == 'plain':
    root = np.ascontiguousarray(a)
    view = root
  elif how == 'interleaved':  # [lat, lon, key, depth]
    root = np.ascontiguousarray(a.transpose(2, 3, 0, 1))
    view = root.transpose(2, 3, 0, 1)
  elif how == 'lon2':  # every other element of rows twice as long, starting at the second
    root = np.full((k, d, y, 2 * x), np.nan, a.dtype)
    root[..., 1::2] = a
    view = root[..., 1::2]
  else:  # [key, depth, lon, lat]
    root = np.ascontiguousarray(a.transpose(0, 1, 3, 2))
    view = root.transpose(0, 1, 3, 2)
  assert np.array_equal(view, a, equal_nan=True)
  return view, root, (view.__array_interface__['data'][0] - root.__array_interface__['data'][0]) // a.itemsize


def _layout(a, dims):
  lay = planner.layout_of(a, dims)
  return planner.InputLayout(strides=dict(lay.strides), itemsize=lay.itemsize, base_alignment=lay.itemsize)


def _ptr(buf, offset=0):
  return None if buf is None else C.c_void_p(buf.ptr + offset)


def launch(ctx, p, t, n, wrap, x_kept, depth_chunk, flags, mask=None, how='plain', dtype_code=None, with_mask=True, sentinel=None,
           repeat=1, zero=None, keep_out=False):
  """p, t [key, depth, lat, lon]; mask [lat, lon] or [key, depth, lat, lon] (uint8) -> (rc, plan, [partials], [device out])."""
  nkey, ndepth, nlat, nlon = p.shape
  sizes = dict(zip(SDIMS, p.shape))
  pv, proot, poff = stored(p, how)
  tv, troot, toff = stored(t, how)
  lay_m = mask_buf = None
  if flags & _hip.FLAG_MASKED:
    m = np.ascontiguousarray(mask, np.uint8)
    lay_m = _layout(m, SDIMS[-m.ndim:])
    mask_buf = ctx.upload(m) if with_mask else None
  reduce_dims = (DEPTH,) if x_kept else (DEPTH, LON)
  fp = planner.build_fss_plan(SDIMS, sizes, [_layout(pv, SDIMS), _layout(tv, SDIMS), lay_m], reduce_dims, flags=flags & 3, wrap_longitude=wrap)
  assert fp.x_kept == x_kept and fp.nkey == nkey and fp.ndepth == ndepth and (fp.nlat, fp.nlon) == (nlat, nlon), fp
  assert fp.s1.key_dims == (KEY, LAT) and fp.s1.nkey == nkey * nlat
  dc = max(1, min(depth_chunk, ndepth))
  fp = dataclasses.replace(fp, depth_chunk=dc, nchunk=-(-ndepth // dc), flags=flags,
                           s1=dataclasses.replace(fp.s1, depth_chunk=dc, nchunk=-(-ndepth // dc)))
  nacc = FC.lanes_total(flags)
  shape = (nkey, nlat, fp.nchunk, nacc, nlon if x_kept else 1)
  if zero:
    fp = dataclasses.replace(fp, **{zero: 0})
  if lay_m is not None and len(lay_m.strides) == 2:
    assert fp.key_off[2] is None and fp.depth_off[2] is None  # a (latitude, longitude) mask: two strides and no tables
  dplan = engine._FssPlanOnDevice(ctx, fp)  # pylint: disable=protected-access
  bufs = [ctx.upload(proot), ctx.upload(troot)]
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  size = int(np.prod(shape))
  outs, rc, out = [], 0, None
  for _ in range(repeat):
    out = ctx.upload(np.full(size, sentinel, np.float64)) if sentinel is not None else ctx.alloc(size * 8)
    rc = ctx.lib.wbx_fss_partial(ctx.handle, C.byref(dplan.struct), dtype_code, int(n), _ptr(bufs[0], poff * p.itemsize),
                                 _ptr(bufs[1], toff * t.itemsize), _ptr(mask_buf), _ptr(out))
    outs.append(ctx.download(out.ptr, shape, np.float64))
  return (rc, fp, outs, out) if keep_out else (rc, fp, outs)


def check_partials(got, p, t, n, wrap, mask, flags, depth_chunk, x_kept, exact, what, gaussian=False):
  values = FC.point_values(p, t, n, wrap)
  dc = max(1, min(depth_chunk, p.shape[1]))
  if gaussian:
    want, mag, nterm, slack = FC.partials(values, mask, flags, dc, x_kept, bounds=FC.point_bounds(p, t, n, wrap))
  else:
    want, mag, nterm = FC.partials(values, mask, flags, dc, x_kept)
    slack = np.zeros_like(mag)
  assert got.shape == want.shape, what
  np.testing.assert_array_equal(got[..., FC.LANES:, :], want[..., FC.LANES:, :], err_msg=f'{what}: the count lanes')
  g, w = got[..., :FC.LANES, :], want[..., :FC.LANES, :]
  np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f'{what}: NaN placement')
  if exact:
    assert FC.same_numbers(g, w), f'{what}: bit for bit'
    return
  fin = np.isfinite(w)
  err = np.abs(g[fin] - w[fin])
  assert (nterm * (nterm - 1.0) * FC.U <= 1).all()
  bound = (nterm[fin] + 1) * FC.U * (mag[fin] + slack[fin]) + slack[fin]
  worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
  print(f'{what}: worst |d| / bound = {worst:.3g} over {int(fin.sum())} finite partials')
  assert (err <= bound).all(), f'{what}: worst ratio {worst}'


def _mask_for(rng, shape, per_point):
  return (rng.integers(0, 4, size=shape if per_point else shape[-2:]) != 0).astype(np.uint8)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_against_the_restatement(ctx, mode, dtype):
  """0 / 1 fields with 8 % NaN (and a clean small-integer field) at every shape and size, both wrap settings, x summed and kept,
  nkey, ndepth and nchunk above 1 with a ragged last chunk, the four memory orders in rotation."""
  flags = MODES[mode]
  turn = 0
  for i, (nlat, nlon) in enumerate(FC.SHAPES):
    nkey, ndepth = (2, 3) if nlon < FC.WIDE else (1, 2)
    shape = (nkey, ndepth, nlat, nlon)
    rng = np.random.default_rng(100 * i + flags)
    for kind in ('indicator', 'integer'):
      p, t = (FC.indicator_fields(shape, dtype, 7 * i + flags, nan_share=0.08) if kind == 'indicator'
              else FC.integer_fields(shape, dtype, 11 * i + flags))
      for n in FC.sizes_for(nlat, nlon):
        turn += 1
        wrap, x_kept, how = bool(turn & 1), bool((turn >> 1) & 1), LAYOUTS[(turn + turn // 4) % 4]
        depth_chunk = 2 if turn % 3 else ndepth  # 3 fields in chunks of 2: a ragged last chunk
        mask = _mask_for(rng, shape, per_point=bool((turn // 3) & 1))
        what = f'{nlat}x{nlon} n={n} wrap={wrap} x_kept={x_kept} {how} chunk={depth_chunk} {mode} {np.dtype(dtype).name} {kind}'
        rc, _, (got,) = launch(ctx, p, t, n, wrap, x_kept, depth_chunk, flags, mask=mask, how=how)
        _hip.check(rc, what)
        check_partials(got, p, t, n, wrap, mask, flags, depth_chunk, x_kept, n == 1, what)  # n == 1: every lane a small integer


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_every_dim_kept_is_the_point_bit_for_bit(ctx, dtype):
  """x kept and every field its own chunk: a partial is 0.0 + one point, at any n."""
  for i, (nlat, nlon) in enumerate(FC.SHAPES):
    shape = (2, 2, nlat, nlon) if nlon < FC.WIDE else (1, 2, nlat, nlon)
    p, t = FC.indicator_fields(shape, dtype, 50 + i, nan_share=0.08)
    rng = np.random.default_rng(i)
    for n in FC.sizes_for(nlat, nlon):
      for j, flags in enumerate(MODES.values()):
        mask = _mask_for(rng, shape, per_point=bool(j & 1))
        wrap = bool((i + j) & 1)
        rc, _, (got,) = launch(ctx, p, t, n, wrap, True, 1, flags, mask=mask, how=LAYOUTS[(i + j) % 4])
        _hip.check(rc, 'every dim kept')
        check_partials(got, p, t, n, wrap, mask, flags, 1, True, True, f'{nlat}x{nlon} n={n} flags={flags}')


def test_gaussian_fields_within_the_derived_bound(ctx):
  for i, (nlat, nlon) in enumerate(FC.SHAPES):
    shape = (2, 3, nlat, nlon) if nlon < FC.WIDE else (1, 2, nlat, nlon)
    for dtype in (np.float32, np.float64):
      p, t = FC.gaussian_fields(shape, dtype, 300 + i)
      for n in FC.sizes_for(nlat, nlon):
        for x_kept in (False, True):
          wrap = bool((n // 2 + i) & 1)
          rc, _, (got,) = launch(ctx, p, t, n, wrap, x_kept, 2, 0, how=LAYOUTS[(i + n) % 4])
          _hip.check(rc, 'gaussian')
          check_partials(got, p, t, n, wrap, None, 0, 2, x_kept, False, f'gaussian {nlat}x{nlon} n={n} x_kept={x_kept} {np.dtype(dtype).name}',
                         gaussian=n > 1)


def test_nans_inside_the_border_give_zero_not_nan(ctx):
  """A NaN in a border row or column, and one whose window wraps the date line; an all-NaN field."""
  p = np.zeros((1, 2, 9, 11), np.float32)
  t = np.ones((1, 2, 9, 11), np.float32)
  p[0, 0, 0, 3] = np.nan   # border row
  p[0, 0, 4, 0] = np.nan   # first column: border without wrap, and its window wraps the date line with it
  t[0, 1] = np.nan         # an all-NaN field
  for wrap in (False, True):
    for n in (3, 5):
      rc, _, (got,) = launch(ctx, p, t, n, wrap, True, 1, 0)
      _hip.check(rc, 'border')
      check_partials(got, p, t, n, wrap, None, 0, 1, True, True, f'border n={n} wrap={wrap}')
      h = n // 2
      lane1 = got[0, :, 0, 1, :]  # Pf^2 of field 0
      assert not np.isnan(lane1[:h]).any() and not np.isnan(lane1[-h:]).any() and (lane1[:h] == 0).all()
      assert np.isnan(lane1[4, 10]) == wrap  # the point across the date line sees the NaN only where longitude wraps
      inner = got[0, h:9 - h, 1, 2, h:11 - h]  # Tf^2 of the all-NaN field away from the border
      assert np.isnan(inner).all() and (got[0, :h, 1, 2, :] == 0).all()


def test_two_launches_of_one_case_are_bit_equal(ctx):
  for (nlat, nlon), x_kept, flags, dtype in (((43, 24), False, 0, np.float32), ((5, 300), True, _hip.FLAG_SKIPNA, np.float64),
                                            ((12, 16), False, _hip.FLAG_MASKED, np.float32)):
    shape = (2, 3, nlat, nlon)
    p, t = FC.gaussian_fields(shape, dtype, 5)
    mask = _mask_for(np.random.default_rng(1), shape, True)
    rc, _, (a, b) = launch(ctx, p, t, 3, True, x_kept, 2, flags, mask=mask, repeat=2)
    _hip.check(rc, 'repeat')
    assert a.tobytes() == b.tobytes(), (nlat, nlon)


def test_partials_feed_the_contraction_unchanged(ctx):
  rng = np.random.default_rng(8)
  p, t = FC.integer_fields((2, 3, 9, 11), np.float32, 31)
  for x_kept in (True, False):
    rc, fp, (got,), out = launch(ctx, p, t, 1, False, x_kept, 2, _hip.FLAG_SKIPNA, keep_out=True)
    _hip.check(rc, 'partial')
    nkey, nlat, nchunk, nlane, nj = got.shape
    n_out = C.c_int64(0)
    sp = engine._PlanOnDevice(ctx, fp.s1)  # pylint: disable=protected-access
    _hip.check(ctx.lib.wbx_s1_partial_len(C.byref(sp.struct), FC.LANES, C.byref(n_out)), 'wbx_s1_partial_len')
    assert n_out.value == got.size
    w = rng.integers(1, 9, size=(1, nlat, nj, 2)).astype(np.float64)  # [nBk][nBr][nj][nbin]: latitude is the last key dim
    st = _hip.S2PlanStruct(nkey, 1, nlat, nchunk, nlane, nj, 2, 1)
    res = ctx.alloc(nkey * nlane * 2 * 8)
    _hip.check(ctx.lib.wbx_contract(ctx.handle, C.byref(st), C.c_void_p(out.ptr), C.c_void_p(ctx.upload(w).ptr), C.c_void_p(res.ptr)),
               'wbx_contract')
    have = ctx.download(res.ptr, (nkey, 1, nlane, 1, 2), np.float64)
    np.testing.assert_array_equal(have[:, 0, :, 0, :], np.einsum('kyclj,yjn->kln', got, w[0]))  # small integers: exact


def test_refusals_leave_the_output_untouched(ctx):
  p, t = FC.indicator_fields((2, 3, 9, 11), np.float32, 9)
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
  ]
  for message, field, kw in cases:
    kw = dict(kw)
    rc, _, (got,) = launch(ctx, field, field, kw.pop('n', 3), True, False, 3, kw.pop('flags', 0), mask=mask, sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message
  rc, _, (got,) = launch(ctx, wide[..., :2048], wide[..., :2048], 3, True, False, 1, 0, sentinel=SENTINEL)  # 2048 itself is served
  _hip.check(rc, 'nlon = 2048')
  assert (got == 0.0).all()


@pytest.mark.parametrize('mode', list(MODES))
def test_empty_extents_zero_the_partial_and_no_keys_touch_nothing(ctx, mode):
  p, t = FC.indicator_fields((2, 3, 9, 11), np.float32, 4)
  mask = np.ones((9, 11), np.uint8)
  for x_kept in (False, True):
    for zero in ('ndepth', 'nlon') if not x_kept else ('ndepth',):
      rc, _, (got,) = launch(ctx, p, t, 3, False, x_kept, 3, MODES[mode], mask=mask, sentinel=SENTINEL, zero=zero)
      _hip.check(rc, zero)
      assert (got == 0.0).all() and not np.signbit(got).any(), zero
  rc, _, (got,) = launch(ctx, p, t, 3, False, False, 3, MODES[mode], mask=mask, sentinel=SENTINEL, zero='nkey')
  _hip.check(rc, 'nkey == 0')
  assert (got == SENTINEL).all()
