"""wbx_contingency_field_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the restatement with
per-point thresholds (tests/contingency_field_cases.py), bit for bit -- every output is an integer held in fp64, or NaN.

Extents are those of tests/test_gpu_contingency.py: frame (lead = 2, row = 5, x), x summed and kept, all rows per partial and 2 (a
ragged last chunk), the four flag modes, row lengths 1, 63, 64, 65, 257 with plan.vec == 1 and 4, 256, 260 with plan.vec == 4 where
the field's x stride allows it, transposed inputs (x stride 5).  New ground, dealt over the (width, rows per partial, x mode)
combinations in a rotating schedule (`_schedule`): the four (data, field) dtype pairs; the field over (row, x), x, row and (lead,
row, x); its threshold axis outermost and innermost; rows of the field padded by one element, so that under plan.vec == 4 neither its
row stride nor thr_stride is a multiple of 4.  nthr is 1, 3 and 16, the last also as slots 2..17 of an axis of 19 (thr_first = 2)."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import contingency_cases as CC
import contingency_field_cases as FC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked+skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
LEAD, ROW, X = 'lead_time', 'row', 'x'
SDIMS = (LEAD, ROW, X)
NLEAD, NROW = 2, 5
SENTINEL = -77.0
CODES = {np.dtype(np.float32): _hip.F32, np.dtype(np.float64): _hip.F64}
PAIRS = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]  # (data, field)
NX_DWORD = (1, 63, 64, 65, 257)
NX_VEC4 = (4, 256, 260)
NTHR = [(1, 0, 1), (3, 0, 3), (16, 0, 16), (16, 2, 19)]  # (nthr, thr_first, thresholds along the field's axis)
COMBOS = list(itertools.product(NX_DWORD + NX_VEC4, (NROW, 2), (False, True)))  # (nx, depth_chunk, x_kept)


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def test_the_library_exports_the_entry_point(ctx):
  assert getattr(ctx.lib, 'wbx_contingency_field_partial', None) is not None and engine.contingency_field_available(ctx)
  assert ctx.lib.wbx_abi_version() == 13


def _root(a):
  """The contiguous array `a` is a (transposed) view of; `a` starts at its first element."""
  r = a
  while r.base is not None:
    r = r.base
  assert r.flags.c_contiguous and r.__array_interface__['data'][0] == a.__array_interface__['data'][0]
  return r


def _layout(a, dims):
  lay = planner.layout_of(a, dims)
  return planner.InputLayout(strides=dict(lay.strides), itemsize=lay.itemsize, base_alignment=256)


def _ptr(buf):
  return None if buf is None else C.c_void_p(buf.ptr)


def _plan(case, x_kept, depth_chunk, flags, vec4=False, ndepth0=False):
  nlead, nrow, nx = case.t.shape
  lay_m = planner.InputLayout(strides={ROW: nx, X: 1}, itemsize=1, base_alignment=256) if flags & _hip.FLAG_MASKED else None
  s = case.strides
  lay_c = planner.InputLayout(strides={LEAD: s['lead'], ROW: s['row'], X: s['x']}, itemsize=case.root.itemsize, base_alignment=256)
  plan = planner.build_s1_plan(SDIMS, {LEAD: nlead, ROW: nrow, X: nx}, [_layout(case.p, SDIMS), _layout(case.t, SDIMS), lay_c, lay_m],
                               (ROW,) if x_kept else (ROW, X), wdep_dims=set(), flags=flags, allow_vec4=False, force_x_dim=X)
  dc = min(depth_chunk, plan.ndepth)
  plan = dataclasses.replace(plan, depth_chunk=dc, nchunk=-(-plan.ndepth // dc), vec=4 if vec4 else 1)
  assert plan.x_kept == x_kept and plan.a_dims == (LEAD,) and plan.depth_dims == (ROW,) and plan.plane_rows == 0, plan
  assert plan.xstride[2] == s['x']
  if ndepth0:
    plan = dataclasses.replace(plan, ndepth=0)
  return plan


def _launch(ctx, case, x_kept, depth_chunk, flags, nthr, first=0, vec4=False, dtype_code=None, thr_code=None, thr_stride=None,
            with_mask=True, with_field=True, sentinel=None, ndepth0=False, lanes_for=None):
  """-> (rc, plan, partial[lead][chunk][lane][j]) of one launch on the case's arrays as they are stored."""
  plan = _plan(case, x_kept, depth_chunk, flags, vec4, ndepth0)
  k = nthr if lanes_for is None else lanes_for
  nl = CC.CELLS * k
  lanes = 2 * nl if flags & _hip.FLAG_SKIPNA else (nl + 1 if flags & _hip.FLAG_MASKED else nl)
  shape = (case.t.shape[0], plan.nchunk, lanes, plan.nj)
  mask_buf = ctx.upload(np.ascontiguousarray(case.mask, np.uint8)) if flags & _hip.FLAG_MASKED and with_mask else None
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  n = int(np.prod(shape))
  out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
  bufs = ctx.upload(_root(case.p)), ctx.upload(_root(case.t)), ctx.upload(case.root)
  rc = ctx.lib.wbx_contingency_field_partial(
      ctx.handle, C.byref(dplan.struct), CODES[case.p.dtype] if dtype_code is None else dtype_code,
      CODES[case.root.dtype] if thr_code is None else thr_code, nthr, case.strides['thr'] if thr_stride is None else thr_stride, first,
      _ptr(bufs[0]), _ptr(bufs[1]), _ptr(bufs[2]) if with_field else None, _ptr(mask_buf), _ptr(out))
  return rc, plan, ctx.download(out.ptr, shape, np.float64)


def _schedule(case_index, j):
  """The variant combination j of parametrised case `case_index` runs: (pair, varies, threshold axis innermost, transposed)."""
  s = 5 * case_index + j
  v = s % 8
  return PAIRS[(s // 8) % 4], FC.VARIES[v % 4], bool(v // 4), (s // 3) % 4 == 0


def _cases():
  return [(mode, k) for mode in MODES for k in range(len(NTHR))]


def test_the_schedule_meets_every_combination():
  """Every variant (what the field varies over, where its threshold axis sits) meets every dtype pair and both x modes; transposed
  inputs and 16-byte loads meet both x modes and every pair."""
  met = set()
  for ci in range(len(_cases())):
    for j, (nx, _, x_kept) in enumerate(COMBOS):
      pair, varies, inner, transposed = _schedule(ci, j)
      variant = (varies, inner)
      vec4 = nx in NX_VEC4 and not transposed and (not inner or varies == 'row')  # (the field's x stride is 1 or 0)
      met |= {(variant, 'pair', PAIRS.index(pair)), (variant, 'x_kept', x_kept), ('transposed', transposed, x_kept, PAIRS.index(pair)),
              ('vec4', vec4, x_kept, PAIRS.index(pair))}
  for variant in itertools.product(FC.VARIES, (False, True)):
    for what, values in (('pair', range(4)), ('x_kept', (False, True))):
      for v in values:
        assert (variant, what, v) in met, (variant, what, v)
  for x_kept, pair in itertools.product((False, True), range(4)):
    assert ('transposed', True, x_kept, pair) in met and ('vec4', True, x_kept, pair) in met


@pytest.mark.parametrize('k', range(len(NTHR)), ids=[f'K{n}-first{f}' for n, f, _ in NTHR])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_bit_equal(ctx, mode, k):
  nthr, first, size = NTHR[k]
  flags = MODES[mode]
  ci = _cases().index((mode, k))
  nvec4 = nodd = 0
  for j, (nx, depth_chunk, x_kept) in enumerate(COMBOS):
    (dtype, thr_dtype), varies, inner, transposed = _schedule(ci, j)
    vec4 = nx in NX_VEC4 and not transposed
    case = FC.field_case(1000 * ci + j, size, NLEAD, NROW, nx, dtype, thr_dtype, flags, varies, inner, pad=1 if vec4 else 0,
                         transposed=transposed)
    vec4 = vec4 and case.strides['x'] in (0, 1)
    what = (f'K={nthr} first={first} nx={nx} dc={depth_chunk} x_kept={x_kept} {mode} data={np.dtype(dtype).name} '
            f'field={np.dtype(thr_dtype).name} varies={varies} thr_innermost={inner} transposed={transposed} vec4={vec4} {case.strides}')
    want, _ = FC.expected(case, flags, depth_chunk, x_kept, first, nthr)
    FC.assert_not_all_nan(want, flags, what)  # the restatement alone: where the NaNs went
    rc, plan, got = _launch(ctx, case, x_kept, depth_chunk, flags, nthr, first, vec4=vec4)
    _hip.check(rc, what)
    nvec4 += plan.vec == 4
    nodd += plan.vec == 4 and case.strides['x'] == 1 and case.strides['thr'] % 4 != 0
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{what}: NaN positions')
    np.testing.assert_array_equal(got, want, err_msg=what)  # (assert_array_equal takes NaN == NaN) every lane, bit for bit
  assert nvec4 > 0 and (nodd > 0 or nthr == 1), (nvec4, nodd)


@pytest.mark.parametrize('pair', PAIRS, ids=[f'{np.dtype(d).name}-{np.dtype(c).name}' for d, c in PAIRS])
def test_a_field_constant_in_space_gives_the_list_kernels_partials(ctx, pair):
  """A field that holds the same K numbers everywhere: the partials of wbx_contingency_partial on the same list, bit for bit."""
  dtype, thr_dtype = pair
  for nthr, x_kept, nx in ((16, False, 65), (3, True, 65), (1, False, 65), (16, False, 256)):
    thr = CC.thresholds(nthr)
    if np.dtype(thr_dtype) == np.float32:
      with np.errstate(over='ignore'):  # (what a float32 field can hold: +-1e40 become +-inf)
        thr = thr.astype(np.float32).astype(np.float64)
    for flags in (0, _hip.FLAG_MASKED | _hip.FLAG_SKIPNA):
      p, t, mask = CC.contingency_case(31 + nthr, NLEAD, NROW, nx, dtype, flags, 2, x_kept)
      root = thr.astype(thr_dtype)  # [K], read with zero lead, row and x strides
      case = FC.FieldCase(p, t, mask, root, {'thr': 1, 'lead': 0, 'row': 0, 'x': 0}, nthr)
      vec4 = nx == 256
      rc, plan, got = _launch(ctx, case, x_kept, 2, flags, nthr, vec4=vec4)
      _hip.check(rc, 'field')
      dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
      out = ctx.alloc(got.size * 8)
      bufs = ctx.upload(p), ctx.upload(t), ctx.upload(thr), ctx.upload(np.ascontiguousarray(mask, np.uint8))
      _hip.check(ctx.lib.wbx_contingency_partial(ctx.handle, C.byref(dplan.struct), CODES[p.dtype], nthr, _ptr(bufs[0]), _ptr(bufs[1]),
                                                 _ptr(bufs[2]), _ptr(bufs[3]) if flags & _hip.FLAG_MASKED else None, _ptr(out)), 'list')
      np.testing.assert_array_equal(got, ctx.download(out.ptr, got.shape, np.float64), err_msg=f'K={nthr} flags={flags} vec4={vec4}')
      want, _ = FC.expected(case, flags, 2, x_kept)
      np.testing.assert_array_equal(got, want)


def test_padding_slots_do_not_count(ctx):
  """K = 2, 5 and 9 run in the kernels built for 4, 8 and 16 slots, from thr_first = 1: the slots beyond K leave no trace in the K
  thresholds' lanes, and no lane is written for them (the partial has 4 K value lanes).  Where those slots read is not seen here:
  their counters are never written."""
  for nthr, pair in zip((2, 5, 9), PAIRS[1:]):
    for x_kept in (False, True):
      case = FC.field_case(77 + nthr, nthr + 1, NLEAD, NROW, 65, pair[0], pair[1], 0, 'row_x', False)
      want, _ = FC.expected(case, 0, NROW, x_kept, 1, nthr)
      rc, _, got = _launch(ctx, case, x_kept, NROW, 0, nthr, 1)
      _hip.check(rc, f'K={nthr}')
      np.testing.assert_array_equal(got, want, err_msg=f'K={nthr} x_kept={x_kept}')


def test_refusals_leave_the_output_untouched(ctx):
  case = FC.field_case(9, 16, NLEAD, NROW, 65, np.float32, np.float64, 0, 'row_x', False)
  cases = [
      ('thresholds per launch', dict(nthr=17, lanes_for=16)),
      ('thresholds per launch', dict(nthr=0, lanes_for=16)),
      ('unknown dtype', dict(dtype_code=7)),
      ('unknown thr_dtype', dict(thr_code=7)),
      ('c is NULL', dict(with_field=False)),
      ('thr_stride is 0', dict(thr_stride=0)),
      ('thr_first is negative', dict(first=-1)),
      ('mask is NULL', dict(flags=_hip.FLAG_MASKED, with_mask=False)),
      ('flags other than MASKED', dict(flags=_hip.FLAG_SKIPNA_ENS)),
      ('flags other than MASKED', dict(flags=_hip.FLAG_FAIR)),
  ]
  for message, kw in cases:
    kw = dict(dict(nthr=16, flags=0), **kw)
    rc, _, got = _launch(ctx, case, False, NROW, kw.pop('flags'), kw.pop('nthr'), sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message
  # plane mode, folded x weights and 2^32 points per partial: what wbx_contingency_partial refuses of a plan
  plan = _plan(case, False, NROW, 0)
  for message, bad in (('no plane mode', dataclasses.replace(plan, plane_rows=5)),
                       ('no plane mode', dataclasses.replace(plan, x_weights=np.ones(65))),
                       ('2\\^32 or more points per partial', dataclasses.replace(plan, depth_chunk=2 ** 40, nchunk=1))):
    dplan = engine._PlanOnDevice(ctx, bad)  # pylint: disable=protected-access
    out = ctx.upload(np.full(NLEAD * 64, SENTINEL, np.float64))
    bufs = ctx.upload(case.p), ctx.upload(case.t), ctx.upload(case.root)
    rc = ctx.lib.wbx_contingency_field_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, _hip.F64, 16, case.strides['thr'], 0, _ptr(bufs[0]),
                                               _ptr(bufs[1]), _ptr(bufs[2]), None, _ptr(out))
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (ctx.download(out.ptr, (NLEAD * 64,), np.float64) == SENTINEL).all()
  assert ctx.lib.wbx_contingency_field_partial(None, None, _hip.F32, _hip.F64, 1, 1, 0, None, None, None, None, None) == -1
  # a zero threshold stride is fine for one threshold
  rc, _, got = _launch(ctx, case, False, NROW, 0, 1, 3, thr_stride=0, sentinel=SENTINEL)
  _hip.check(rc, 'K = 1')
  want, _ = FC.expected(dataclasses.replace(case, strides=dict(case.strides, thr=0)), 0, NROW, False, 3, 1)
  np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('mode', list(MODES))
def test_no_rows_zero_the_partial_whatever_the_field_is(ctx, mode):
  case = FC.field_case(4, 3, NLEAD, NROW, 65, np.float32, np.float32, 0, 'row_x', False)
  for x_kept in (False, True):
    rc, _, got = _launch(ctx, case, x_kept, NROW, MODES[mode], 3, sentinel=SENTINEL, ndepth0=True, with_field=False)
    _hip.check(rc, 'ndepth == 0')
    assert (got == 0.0).all() and not np.signbit(got).any()
