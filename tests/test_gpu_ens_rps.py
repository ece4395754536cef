"""wbx_ens_rps_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the integer restatement
(tests/ens_rps_cases.py), bit for bit -- a partial is float64(S) / float64(D) of an exact integer sum S, so no tolerance applies.

Frame (lead = 2, row = 5, x); x summed and kept; all rows per partial and 2 (a ragged last chunk); plain / masked / skipna /
masked + skipna; float32 and float64; fair and unfair; right- and left-inclusive; the member axis outermost (stride = lead * row * x)
and innermost (stride 1, x stride M); the mask depends on (row, x) only.  (M, K) in (2, 1), (3, 3), (51, 5), (64, 16), (256, 16) --
the last at row lengths 65 and 256 only -- and (1, 1) unfair.  Row lengths 1, 63, 64, 65, 257 with plan.vec == 1 and 4, 256, 260
with plan.vec == 4 (accepted, read with dword loads).  NaN outputs (a NaN member or target under a valid point poisons its partial
unless skipna counts it out) must be NaN on both sides at the same positions, at least 80 % of the expected partials of a plain /
masked case are finite, and under skipna every output is finite while the statistic itself holds NaNs."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import ens_rps_cases as EC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked+skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
MEMBER, LEAD, ROW, X = 'number', 'lead_time', 'row', 'x'
SDIMS = (LEAD, ROW, X)
NLEAD, NROW = 2, 5
SENTINEL = -77.0


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


def _launch(ctx, p, t, mask, a, b, x_kept, depth_chunk, flags, right=True, vec4=False, nthr=None, m=None, dtype_code=None,
            with_mask=True, sentinel=None, ndepth0=False):
  """-> (rc, plan, partial[lead][chunk][lane][j]) of one launch on p[M, lead, row, x], t[lead, row, x] (any strides), mask[row, x]."""
  nlead, nrow, nx = t.shape
  sizes = {LEAD: nlead, ROW: nrow, X: nx}
  lay_m = mask_buf = None
  if flags & _hip.FLAG_MASKED:
    lay_m = planner.InputLayout(strides={ROW: nx, X: 1}, itemsize=1, base_alignment=256)  # zero stride along lead
    mask_buf = ctx.upload(np.ascontiguousarray(mask, np.uint8)) if with_mask else None
  reduce_dims = (ROW,) if x_kept else (ROW, X)
  lay_p = _layout(p, (MEMBER,) + SDIMS)
  plan = planner.build_s1_plan(SDIMS, sizes, [lay_p, _layout(t, SDIMS), None, lay_m], reduce_dims, wdep_dims=set(),
                               flags=flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA), allow_vec4=vec4 and p.dtype == np.float32, force_x_dim=X)
  dc = min(depth_chunk, plan.ndepth)
  plan = dataclasses.replace(plan, depth_chunk=dc, nchunk=-(-plan.ndepth // dc), flags=flags)
  if vec4 and p.dtype == np.float64:  # (the planner keeps 16-byte loads to 4-byte elements; the ABI takes vec = 4 for float64 too)
    plan = dataclasses.replace(plan, vec=4)
  if vec4:
    assert plan.vec == 4 and plan.plane_rows == 0, plan
  assert plan.x_kept == x_kept and plan.a_dims == (LEAD,) and plan.depth_dims == (ROW,) and not plan.bk_dims and not plan.br_dims, plan
  shape = (nlead, plan.nchunk, 2 if flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA) else 1, plan.nj)
  if ndepth0:
    plan = dataclasses.replace(plan, ndepth=0)
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  n = int(np.prod(shape))
  out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
  bufs = ctx.upload(_root(p)), ctx.upload(_root(t))
  abuf, bbuf = ctx.upload(np.asarray(a, np.float64)), ctx.upload(np.asarray(b, np.float64))
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  rc = ctx.lib.wbx_ens_rps_partial(ctx.handle, C.byref(dplan.struct), dtype_code, p.shape[0] if m is None else m, lay_p.stride(MEMBER),
                                   len(a) if nthr is None else nthr, _ptr(abuf), _ptr(bbuf), int(right), _ptr(bufs[0]), _ptr(bufs[1]),
                                   _ptr(mask_buf), _ptr(out))
  return rc, plan, ctx.download(out.ptr, shape, np.float64)


NX_DWORD = (1, 63, 64, 65, 257)
NX_VEC4 = (4, 256, 260)
MK = [(2, 1), (3, 3), (51, 5), (64, 16), (256, 16), (1, 1)]


@pytest.mark.parametrize('mk', MK, ids=[f'M{m}-K{k}' for m, k in MK])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_bit_equal(ctx, mode, dtype, mk):
  m, nthr = mk
  flags = MODES[mode]
  a, b = EC.thresholds(nthr)
  widths = (65, 256) if m == 256 else NX_DWORD + NX_VEC4
  seed, launches = 0, 0
  for nx in widths:
    for depth_chunk in (NROW, 2):
      for x_kept in (False, True):
        seed += 1
        p0, t, mask = EC.ens_rps_case(1000 * m + seed, m, NLEAD, NROW, nx, dtype, flags, depth_chunk, x_kept, a)
        nan = EC.nan_points(p0, t)
        for right in (True, False):
          for fair in ((False,) if m == 1 else (True, False)):
            what = f'M={m} K={nthr} nx={nx} dc={depth_chunk} x_kept={x_kept} {mode} {np.dtype(dtype).name} fair={fair} right={right}'
            want, _ = EC.expected(p0, t, a, b, fair, right, mask, flags, depth_chunk, x_kept)
            # the restatement alone: where the NaNs went
            if flags & _hip.FLAG_SKIPNA:
              assert np.isfinite(want).all() and nan.any(), what
            else:
              share = float(np.isfinite(want[:, :, 0]).mean())
              assert share >= 0.8, (what, 'finite share of the value lane', share)
            for innermost in (False, True):
              p = np.moveaxis(np.ascontiguousarray(np.moveaxis(p0, 0, -1)), -1, 0) if innermost else p0
              if m > 1:
                assert p.strides[0] == (p.itemsize if innermost else p.itemsize * NLEAD * NROW * nx), what
              vec4 = nx in NX_VEC4 and not innermost
              rc, plan, got = _launch(ctx, p, t, mask, a, b, x_kept, depth_chunk, flags | (_hip.FLAG_FAIR if fair else 0), right=right,
                                      vec4=vec4)
              _hip.check(rc, what)
              launches += 1
              tag = f'{what} innermost={innermost} vec={plan.vec}'
              assert got.shape == want.shape, (tag, got.shape, want.shape)
              np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{tag}: NaN positions')
              np.testing.assert_array_equal(got, want, err_msg=tag)  # (assert_array_equal takes NaN == NaN) every lane, bit for bit
  assert launches == len(widths) * 2 * 2 * 2 * (1 if m == 1 else 2) * 2


def test_padding_slots_do_not_count(ctx):
  """K = 2, 5 and 9 run in the kernels built for 4, 8 and 16 slots; members and targets at -inf / +inf meet no phantom threshold."""
  a16, b16 = EC.thresholds(16)
  for nthr in (2, 5, 9):
    a, b = a16[:nthr].copy(), b16[:nthr].copy()
    p, t, mask = EC.ens_rps_case(77 + nthr, 5, NLEAD, NROW, 65, np.float32, 0, NROW, True, a)
    p[:, 0, 0, :8], t[0, 0, :8] = -np.inf, -np.inf
    p[:, 0, 1, :8], t[0, 1, :8] = np.inf, np.inf
    for fair in (True, False):
      want, _ = EC.expected(p, t, a, b, fair, True, mask, 0, NROW, True)
      rc, _, got = _launch(ctx, p, t, mask, a, b, True, NROW, _hip.FLAG_FAIR if fair else 0)
      _hip.check(rc, f'K={nthr}')
      np.testing.assert_array_equal(got, want, err_msg=f'K={nthr} fair={fair}')


def test_refusals_leave_the_output_untouched(ctx):
  a, b = EC.thresholds(16)
  p, t, mask = EC.ens_rps_case(9, 3, NLEAD, NROW, 65, np.float32, 0, NROW, False, a)
  fair = _hip.FLAG_FAIR
  a17, b17 = np.concatenate([a, [0.5]]), np.concatenate([b, [0.5]])
  cases = [
      ('thresholds per launch', dict(a=a17, b=b17, flags=fair)),
      ('thresholds per launch', dict(a=a, b=b, flags=fair, nthr=0)),
      ('members', dict(a=a, b=b, flags=fair, m=257)),
      ('members', dict(a=a, b=b, flags=0, m=0)),
      ('at least 2 members', dict(a=a, b=b, flags=fair, m=1)),
      ('unknown dtype', dict(a=a, b=b, flags=fair, dtype_code=7)),
      ('mask is NULL', dict(a=a, b=b, flags=fair | _hip.FLAG_MASKED, with_mask=False)),
      ('flags other than MASKED', dict(a=a, b=b, flags=fair | _hip.FLAG_SKIPNA_ENS)),
  ]
  for message, kw in cases:
    flags = kw.pop('flags')
    rc, _, got = _launch(ctx, p, t, mask, kw.pop('a'), kw.pop('b'), False, NROW, flags, sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message
  # one member is fine where the score is not fair
  rc, _, got = _launch(ctx, p[:1], t, mask, a, b, False, NROW, 0, sentinel=SENTINEL)
  _hip.check(rc, 'M = 1, unfair')
  want, _ = EC.expected(p[:1], t, a, b, False, True, mask, 0, NROW, False)
  np.testing.assert_array_equal(got, want)


def test_an_exact_sum_is_required_of_the_plan(ctx):
  """depth_chunk * nx * nthr * (M - 1) * M^2 >= 2^53 is refused: S would not survive the conversion to fp64."""
  a, b = EC.thresholds(16)
  p, t, mask = EC.ens_rps_case(9, 3, NLEAD, NROW, 65, np.float32, 0, NROW, False, a)
  nlead, nrow, nx = t.shape
  plan = planner.build_s1_plan(SDIMS, {LEAD: nlead, ROW: nrow, X: nx}, [_layout(p, (MEMBER,) + SDIMS), _layout(t, SDIMS), None, None],
                               (ROW, X), wdep_dims=set(), flags=0, allow_vec4=False, force_x_dim=X)
  plan = dataclasses.replace(plan, depth_chunk=2 ** 40, nchunk=1, flags=_hip.FLAG_FAIR)
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  out = ctx.upload(np.full(nlead, SENTINEL, np.float64))
  bufs = ctx.upload(p), ctx.upload(t), ctx.upload(a), ctx.upload(b)
  rc = ctx.lib.wbx_ens_rps_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, 256, nlead * nrow * nx, 16, _ptr(bufs[2]), _ptr(bufs[3]), 1,
                                   _ptr(bufs[0]), _ptr(bufs[1]), None, _ptr(out))
  with pytest.raises(_hip.WbxError, match='2\\^53 or more per partial'):
    _hip.check(rc, 'too much for one partial')
  assert (ctx.download(out.ptr, (nlead,), np.float64) == SENTINEL).all()


@pytest.mark.parametrize('mode', list(MODES))
def test_no_rows_zero_the_partial(ctx, mode):
  a, b = EC.thresholds(3)
  p, t, mask = EC.ens_rps_case(4, 3, NLEAD, NROW, 65, np.float32, 0, NROW, False, a)
  for x_kept in (False, True):
    rc, _, got = _launch(ctx, p, t, mask, a, b, x_kept, NROW, MODES[mode] | _hip.FLAG_FAIR, sentinel=SENTINEL, ndepth0=True)
    _hip.check(rc, 'ndepth == 0')
    assert (got == 0.0).all() and not np.signbit(got).any()
