"""wbx_ens_rps_field_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the integer restatement
with per-point thresholds (tests/ens_rps_field_cases.py), bit for bit -- a partial is float64(S) / float64(D) of an exact integer sum.

Extents are those of tests/test_gpu_ens_rps.py: frame (lead = 2, row = 5, x), x summed and kept, all rows per partial and 2 (a
ragged last chunk), the four flag modes, fair and unfair, right- and left-inclusive, the member axis outermost and innermost, (M, K) in
(1, 1), (2, 1), (3, 2), (51, 5), (64, 16), (256, 16) -- the last at row lengths 65 and 256 only -- row lengths 1, 63, 64, 65, 257 with
plan.vec == 1 and 4, 256, 260 with plan.vec == 4 where the field's x stride allows it.
New ground, dealt over the (width, rows per partial, x mode) combinations in a rotating schedule (`_schedule`): the four (data,
threshold) dtype pairs; the bin axis outermost [K, day, row, x] and innermost [day, row, x, K]; a source of 3 days of which the two
leads gather days (2, 0) (the third holds NaN throughout); fields that vary over (day, row, x), over x only and not at all; one field
for both sides (t_off = 0) and two stacked ones.  test_the_schedule_meets_every_combination says what met what."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import ens_rps_cases as EC
import ens_rps_field_cases as FC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked+skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
MEMBER, LEAD, ROW, X = 'number', 'lead_time', 'row', 'x'
SDIMS = (LEAD, ROW, X)
NLEAD, NROW = 2, 5
SENTINEL = -77.0
CODES = {np.dtype(np.float32): _hip.F32, np.dtype(np.float64): _hip.F64}
PAIRS = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]  # (data, thresholds)
NX_DWORD = (1, 63, 64, 65, 257)
NX_VEC4 = (4, 256, 260)
MK = [(2, 1), (3, 2), (51, 5), (64, 16), (256, 16), (1, 1)]


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


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
  lay_p = _layout(case.p, (MEMBER,) + SDIMS)
  lay_c = planner.InputLayout(strides={ROW: case.row_stride, X: case.x_stride}, itemsize=case.root.itemsize, base_alignment=256)
  gather = planner.GatherSpec((LEAD,), np.array([d * case.day_stride for d in FC.DAYS], np.int64)) if case.day_stride else None
  plan = planner.build_s1_plan(SDIMS, {LEAD: nlead, ROW: nrow, X: nx}, [lay_p, _layout(case.t, SDIMS), lay_c, lay_m],
                               (ROW,) if x_kept else (ROW, X), wdep_dims=set(), gather=gather,
                               flags=flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA), allow_vec4=False, force_x_dim=X)
  dc = min(depth_chunk, plan.ndepth)
  plan = dataclasses.replace(plan, depth_chunk=dc, nchunk=-(-plan.ndepth // dc), flags=flags, vec=4 if vec4 else 1)
  assert plan.x_kept == x_kept and plan.a_dims == (LEAD,) and plan.depth_dims == (ROW,) and plan.plane_rows == 0, plan
  shape = (nlead, plan.nchunk, 2 if flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA) else 1, plan.nj)
  if ndepth0:
    plan = dataclasses.replace(plan, ndepth=0)
  return plan, lay_p, shape


def _launch(ctx, case, x_kept, depth_chunk, flags, right=True, vec4=False, nthr=None, m=None, dtype_code=None, thr_code=None,
            thr_stride=None, with_mask=True, with_field=True, sentinel=None, ndepth0=False):
  """-> (rc, plan, partial[lead][chunk][lane][j]) of one launch on the case's arrays as they are stored."""
  plan, lay_p, shape = _plan(case, x_kept, depth_chunk, flags, vec4, ndepth0)
  mask_buf = ctx.upload(np.ascontiguousarray(case.mask, np.uint8)) if flags & _hip.FLAG_MASKED and with_mask else None
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  n = int(np.prod(shape))
  out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
  bufs = ctx.upload(_root(case.p)), ctx.upload(_root(case.t)), ctx.upload(case.root)
  rc = ctx.lib.wbx_ens_rps_field_partial(
      ctx.handle, C.byref(dplan.struct), CODES[case.p.dtype] if dtype_code is None else dtype_code,
      CODES[case.root.dtype] if thr_code is None else thr_code, case.p.shape[0] if m is None else m, lay_p.stride(MEMBER),
      case.nthr if nthr is None else nthr, case.thr_stride if thr_stride is None else thr_stride, case.t_off, int(right), _ptr(bufs[0]),
      _ptr(bufs[1]), _ptr(bufs[2]) if with_field else None, _ptr(mask_buf), _ptr(out))
  return rc, plan, ctx.download(out.ptr, shape, np.float64)


def _combos(m):
  widths = (65, 256) if m == 256 else NX_DWORD + NX_VEC4
  return list(itertools.product(widths, (NROW, 2), (False, True)))


def _schedule(case_index, j):
  """The variant combination j of parametrised case `case_index` runs: (pair, varies, bin innermost, stacked)."""
  s = 5 * case_index + j
  v = s % 6
  return PAIRS[(s // 6) % 4], FC.VARIES[v % 3], bool(v // 3), bool((s // 24 + s // 6 + s) % 2)


def _cases():
  return [(mode, mk) for mode in MODES for mk in MK]


def test_the_schedule_meets_every_combination():
  """Every variant (what the field varies over, where its bin axis sits) meets every dtype pair, both x modes and both t_off forms."""
  met = set()
  for ci, (_, (m, _)) in enumerate(_cases()):
    for j, (_, _, x_kept) in enumerate(_combos(m)):
      pair, varies, inner, stacked = _schedule(ci, j)
      variant = (varies, inner)
      met |= {(variant, 'pair', PAIRS.index(pair)), (variant, 'x_kept', x_kept), (variant, 'stacked', stacked)}
  for variant in itertools.product(FC.VARIES, (False, True)):
    for what, values in (('pair', range(4)), ('x_kept', (False, True)), ('stacked', (False, True))):
      for v in values:
        assert (variant, what, v) in met, (variant, what, v)


@pytest.mark.parametrize('mk', MK, ids=[f'M{m}-K{k}' for m, k in MK])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_bit_equal(ctx, mode, mk):
  m, nthr = mk
  flags = MODES[mode]
  ci = _cases().index((mode, mk))
  launches = nvec4 = 0
  combos = _combos(m)
  for j, (nx, depth_chunk, x_kept) in enumerate(combos):
    (dtype, thr_dtype), varies, inner, stacked = _schedule(ci, j)
    case = FC.field_case(100000 * m + 100 * ci + j, m, nthr, NLEAD, NROW, nx, dtype, thr_dtype, flags, depth_chunk, x_kept, varies, inner,
                         stacked)
    a, b = case.selected(0), case.selected(1)
    nan = FC.nan_points(case.p, case.t, a, b)
    assert (case.t_off != 0) == stacked
    for right in (True, False):
      for fair in ((False,) if m == 1 else (True, False)):
        what = (f'M={m} K={nthr} nx={nx} dc={depth_chunk} x_kept={x_kept} {mode} data={np.dtype(dtype).name} thr={np.dtype(thr_dtype).name} '
                f'varies={varies} bin_innermost={inner} stacked={stacked} fair={fair} right={right}')
        want, _ = FC.expected(case.p, case.t, a, b, fair, right, case.mask, flags, depth_chunk, x_kept)
        # the restatement alone: where the NaNs went
        if flags & _hip.FLAG_SKIPNA:
          assert np.isfinite(want).all() and nan.any(), what
        else:
          share = float(np.isfinite(want[:, :, 0]).mean())
          assert share >= 0.8, (what, 'finite share of the value lane', share)
        for innermost in (False, True):
          run = dataclasses.replace(case, p=np.moveaxis(np.ascontiguousarray(np.moveaxis(case.p, 0, -1)), -1, 0)) if innermost else case
          vec4 = nx in NX_VEC4 and not innermost and case.x_stride in (0, 1)
          rc, plan, got = _launch(ctx, run, x_kept, depth_chunk, flags | (_hip.FLAG_FAIR if fair else 0), right=right, vec4=vec4)
          _hip.check(rc, what)
          launches += 1
          nvec4 += plan.vec == 4
          tag = f'{what} innermost={innermost} vec={plan.vec}'
          assert got.shape == want.shape, (tag, got.shape, want.shape)
          np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{tag}: NaN positions')
          np.testing.assert_array_equal(got, want, err_msg=tag)  # (assert_array_equal takes NaN == NaN) every lane, bit for bit
  assert launches == len(combos) * 2 * (1 if m == 1 else 2) * 2
  assert nvec4 > 0 or m == 256


@pytest.mark.parametrize('pair', PAIRS, ids=[f'{np.dtype(d).name}-{np.dtype(c).name}' for d, c in PAIRS])
def test_a_constant_field_gives_the_list_kernels_partials(ctx, pair):
  """A field that holds the same K numbers everywhere: the partials of wbx_ens_rps_partial on the same inputs, bit for bit."""
  dtype, thr_dtype = pair
  for nthr, x_kept, stacked in ((16, False, True), (5, True, False), (1, False, False)):
    a, b = EC.thresholds(nthr)
    if np.dtype(thr_dtype) == np.float32:
      with np.errstate(over='ignore'):  # (what a float32 field can hold: +-1e40 become +-inf)
        a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    if not stacked:
      b = a
    for flags in (0, _hip.FLAG_MASKED | _hip.FLAG_SKIPNA):
      p, t, mask = EC.ens_rps_case(31 + nthr, 7, NLEAD, NROW, 65, dtype, flags, 2, x_kept, a)
      root = np.stack([a, b] if stacked else [a]).astype(thr_dtype)  # [side, K], read with zero day, row and x strides
      case = FC.FieldCase(p, t, mask, root, root[:, :, None, None, None], nthr, 'none', False)
      for fair, right in itertools.product((True, False), repeat=2):
        f = flags | (_hip.FLAG_FAIR if fair else 0)
        rc, plan, got = _launch(ctx, case, x_kept, 2, f, right=right)
        _hip.check(rc, 'field')
        dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
        out = ctx.alloc(got.size * 8)
        bufs = ctx.upload(p), ctx.upload(t), ctx.upload(a), ctx.upload(b), ctx.upload(np.ascontiguousarray(mask, np.uint8))
        _hip.check(ctx.lib.wbx_ens_rps_partial(ctx.handle, C.byref(dplan.struct), CODES[p.dtype], 7, NLEAD * NROW * 65, nthr, _ptr(bufs[2]),
                                               _ptr(bufs[3]), int(right), _ptr(bufs[0]), _ptr(bufs[1]),
                                               _ptr(bufs[4]) if flags & _hip.FLAG_MASKED else None, _ptr(out)), 'list')
        np.testing.assert_array_equal(got, ctx.download(out.ptr, got.shape, np.float64), err_msg=f'K={nthr} fair={fair} right={right}')
        want, _ = FC.expected(p, t, case.selected(0), case.selected(1), fair, right, mask, flags, 2, x_kept)
        np.testing.assert_array_equal(got, want)


def test_padding_slots_do_not_count(ctx):
  """K = 2, 5 and 9 run in the kernels built for 4, 8 and 16 slots.  The element behind the K-th threshold of every point is a NaN
  (the bin axis innermost: it is the very next element); members and targets at -inf / +inf meet no phantom threshold either."""
  for nthr, pair in zip((2, 5, 9), PAIRS[1:]):
    for stacked in (False, True):
      case = FC.field_case(77 + nthr, 5, nthr, NLEAD, NROW, 65, pair[0], pair[1], 0, NROW, True, 'all', True, stacked, extra_bins=1)
      case.view[:, nthr] = np.nan
      assert case.thr_stride == 1 and np.isnan(case.root[..., nthr]).all()
      case.p[:, 0, 0, :8], case.t[0, 0, :8] = -np.inf, -np.inf
      case.p[:, 0, 1, :8], case.t[0, 1, :8] = np.inf, np.inf
      for fair in (True, False):
        want, _ = FC.expected(case.p, case.t, case.selected(0), case.selected(1), fair, True, case.mask, 0, NROW, True)
        assert np.isfinite(want).mean() >= 0.8
        rc, _, got = _launch(ctx, case, True, NROW, _hip.FLAG_FAIR if fair else 0)
        _hip.check(rc, f'K={nthr}')
        np.testing.assert_array_equal(got, want, err_msg=f'K={nthr} fair={fair} stacked={stacked}')


def test_refusals_leave_the_output_untouched(ctx):
  case = FC.field_case(9, 3, 16, NLEAD, NROW, 65, np.float32, np.float64, 0, NROW, False, 'all', False, True, extra_bins=1)
  fair = _hip.FLAG_FAIR
  cases = [
      ('thresholds per launch', dict(flags=fair, nthr=17)),
      ('thresholds per launch', dict(flags=fair, nthr=0)),
      ('members', dict(flags=fair, m=257)),
      ('members', dict(flags=0, m=0)),
      ('at least 2 members', dict(flags=fair, m=1)),
      ('unknown dtype', dict(flags=fair, dtype_code=7)),
      ('unknown thr_dtype', dict(flags=fair, thr_code=7)),
      ('c is NULL', dict(flags=fair, with_field=False)),
      ('thr_stride is 0', dict(flags=fair, thr_stride=0)),
      ('mask is NULL', dict(flags=fair | _hip.FLAG_MASKED, with_mask=False)),
      ('flags other than MASKED', dict(flags=fair | _hip.FLAG_SKIPNA_ENS)),
  ]
  for message, kw in cases:
    rc, _, got = _launch(ctx, case, False, NROW, kw.pop('flags'), sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message
  # a zero threshold stride is fine for one threshold, and one member where the score is not fair
  one = dataclasses.replace(case, p=case.p[:1], nthr=1)
  rc, _, got = _launch(ctx, one, False, NROW, 0, thr_stride=0, sentinel=SENTINEL)
  _hip.check(rc, 'K = 1, M = 1, unfair')
  want, _ = FC.expected(one.p, one.t, one.selected(0), one.selected(1), False, True, one.mask, 0, NROW, False)
  np.testing.assert_array_equal(got, want)


def test_an_exact_sum_is_required_of_the_plan(ctx):
  """depth_chunk * nx * nthr * (M - 1) * M^2 >= 2^53 is refused: S would not survive the conversion to fp64."""
  case = FC.field_case(9, 3, 16, NLEAD, NROW, 65, np.float32, np.float32, 0, NROW, False, 'all', False, False)
  plan, _, _ = _plan(case, False, NROW, 0)
  plan = dataclasses.replace(plan, depth_chunk=2 ** 40, nchunk=1, flags=_hip.FLAG_FAIR)
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  out = ctx.upload(np.full(NLEAD, SENTINEL, np.float64))
  bufs = ctx.upload(case.p), ctx.upload(case.t), ctx.upload(case.root)
  rc = ctx.lib.wbx_ens_rps_field_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, _hip.F32, 256, NLEAD * NROW * 65, 16, case.thr_stride, 0,
                                         1, _ptr(bufs[0]), _ptr(bufs[1]), _ptr(bufs[2]), None, _ptr(out))
  with pytest.raises(_hip.WbxError, match='2\\^53 or more per partial'):
    _hip.check(rc, 'too much for one partial')
  assert (ctx.download(out.ptr, (NLEAD,), np.float64) == SENTINEL).all()


@pytest.mark.parametrize('mode', list(MODES))
def test_no_rows_zero_the_partial(ctx, mode):
  case = FC.field_case(4, 3, 2, NLEAD, NROW, 65, np.float32, np.float32, 0, NROW, False, 'all', False, True)
  for x_kept in (False, True):
    rc, _, got = _launch(ctx, case, x_kept, NROW, MODES[mode] | _hip.FLAG_FAIR, sentinel=SENTINEL, ndepth0=True)
    _hip.check(rc, 'ndepth == 0')
    assert (got == 0.0).all() and not np.signbit(got).any()
