"""wbx_contingency_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the float64 restatement
(tests/contingency_cases.py), bit for bit -- the outputs are integer counts below 2^53 held in fp64, so no tolerance applies.

Frame (lead = 2, row = 5, x); x summed and kept; all rows per partial and 2 (a ragged last chunk); plain / masked / skipna /
masked + skipna; float32 and float64; contiguous inputs and transposed views (x stride = 5); the mask depends on (row, x) only;
1, 3 and WBX_CONT_MAX_THRESHOLDS thresholds.  Row lengths 1, 63, 64, 65, 257 on dword loads and 4, 256, 260 on the 16-byte loads
of plan.vec == 4.  NaN outputs (a NaN under a valid point poisons its partial unless skipna counts it out) must be NaN on both
sides at the same positions, at least 80 % of the expected partials of a plain / masked case are finite, and under skipna every
output is finite."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import contingency_cases as CC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked+skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
LEAD, ROW, X = 'lead_time', 'row', 'x'
SDIMS = (LEAD, ROW, X)
NLEAD, NROW = 2, 5
KMAX = _hip.CONT_MAX_THRESHOLDS


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


def _layout(a):
  lay = planner.layout_of(a, SDIMS)
  return planner.InputLayout(strides=dict(lay.strides), itemsize=lay.itemsize, base_alignment=256)


def _ptr(buf):
  return None if buf is None else C.c_void_p(buf.ptr)


def _lanes_total(nl, flags):
  return 2 * nl if flags & _hip.FLAG_SKIPNA else (nl + 1 if flags & _hip.FLAG_MASKED else nl)


def _launch(ctx, p, t, mask, thr, x_kept, depth_chunk, flags, vec4=False, nthr=None, dtype_code=None, with_mask=True, sentinel=None):
  """-> (rc, plan, partial[lead][chunk][lane][j]) of one launch on p, t[lead, row, x] (any strides), mask[row, x]."""
  nlead, nrow, nx = p.shape
  sizes = {LEAD: nlead, ROW: nrow, X: nx}
  lay_m = mask_buf = None
  if flags & _hip.FLAG_MASKED:
    lay_m = planner.InputLayout(strides={ROW: nx, X: 1}, itemsize=1, base_alignment=256)  # zero stride along lead
    mask_buf = ctx.upload(np.ascontiguousarray(mask, np.uint8)) if with_mask else None
  reduce_dims = (ROW,) if x_kept else (ROW, X)
  plan = planner.build_s1_plan(SDIMS, sizes, [_layout(p), _layout(t), None, lay_m], reduce_dims, wdep_dims=set(), flags=flags,
                               allow_vec4=vec4 and p.dtype == np.float32, force_x_dim=X)
  dc = min(depth_chunk, plan.ndepth)
  plan = dataclasses.replace(plan, depth_chunk=dc, nchunk=-(-plan.ndepth // dc))
  if vec4 and p.dtype == np.float64:  # (the planner keeps 16-byte loads to 4-byte elements; the ABI takes them for float64 too)
    plan = dataclasses.replace(plan, vec=4)
  if vec4:
    assert plan.vec == 4 and plan.plane_rows == 0, plan
  assert plan.x_kept == x_kept and plan.a_dims == (LEAD,) and plan.depth_dims == (ROW,) and not plan.bk_dims and not plan.br_dims, plan
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  nthr = len(thr) if nthr is None else nthr
  shape = (nlead, plan.nchunk, _lanes_total(_hip.CONT_CELLS * min(nthr, len(thr)), flags), plan.nj)
  n = int(np.prod(shape))
  out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
  bufs = ctx.upload(_root(p)), ctx.upload(_root(t))
  tbuf = ctx.upload(np.asarray(thr, np.float64))
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  rc = ctx.lib.wbx_contingency_partial(ctx.handle, C.byref(dplan.struct), dtype_code, nthr, _ptr(bufs[0]), _ptr(bufs[1]), _ptr(tbuf),
                                       _ptr(mask_buf), _ptr(out))
  return rc, plan, ctx.download(out.ptr, shape, np.float64)


def _compare(ctx, seed, nx, dtype, mode, nthr, x_kept, depth_chunk, transposed, vec4, what):
  flags = MODES[mode]
  thr = CC.thresholds(nthr)
  p, t, mask = CC.contingency_case(seed, NLEAD, NROW, nx, dtype, flags, depth_chunk, x_kept, transposed=transposed)
  if nx > 1:  # (a row of one element has no x stride to speak of)
    assert (p.strides[2] != p.itemsize) == transposed
  stat = CC.contingency_stat(p, t, thr)
  want = CC.expected_partials(stat, mask, flags, depth_chunk, x_kept)
  # the restatement alone: where the NaNs went
  if flags & _hip.FLAG_SKIPNA:
    assert np.isfinite(want).all(), what
    assert np.isnan(stat).any(), what
  else:
    share = float(np.isfinite(want[:, :, :_hip.CONT_CELLS * nthr]).mean())
    assert share >= 0.8, (what, 'finite share of the value lanes', share)
  rc, plan, got = _launch(ctx, p, t, mask, thr, x_kept, depth_chunk, flags, vec4=vec4)
  _hip.check(rc, what)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{what}: NaN positions')
  np.testing.assert_array_equal(got, want, err_msg=what)  # (assert_array_equal takes NaN == NaN) every lane, bit for bit
  # the table of every threshold adds up to the count
  k = nthr
  cells = got[:, :, :4 * k].reshape(got.shape[0], got.shape[1], 4, k, got.shape[3])
  total = cells.sum(axis=2)
  if flags & _hip.FLAG_SKIPNA:
    count = got[:, :, 4 * k:5 * k]
  elif flags & _hip.FLAG_MASKED:
    count = np.broadcast_to(got[:, :, 4 * k:4 * k + 1], total.shape)
  else:
    rows = np.minimum(depth_chunk, NROW - depth_chunk * np.arange(plan.nchunk))
    count = np.broadcast_to((rows * (1 if x_kept else nx)).astype(np.float64)[None, :, None, None], total.shape)
  fin = np.isfinite(total)
  np.testing.assert_array_equal(total[fin], count[fin], err_msg=f'{what}: TP + FP + FN + TN == count')
  return plan


NX_DWORD = (1, 63, 64, 65, 257)
NX_VEC4 = (4, 256, 260)


@pytest.mark.parametrize('nthr', [1, 3, KMAX])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_bit_equal(ctx, mode, dtype, nthr):
  seed = 0
  for nx in NX_DWORD + NX_VEC4:
    for depth_chunk in (NROW, 2):
      for x_kept in (False, True):
        for transposed in (False, True):
          seed += 1
          vec4 = nx in NX_VEC4 and not transposed
          what = f'nx={nx} dc={depth_chunk} x_kept={x_kept} transposed={transposed} vec4={vec4} {mode} {np.dtype(dtype).name} K={nthr}'
          plan = _compare(ctx, 1000 * nthr + seed, nx, dtype, mode, nthr, x_kept, depth_chunk, transposed, vec4, what)
          if vec4:
            assert plan.vec == 4, what  # the 16-byte path was reached


def test_nan_threshold_counts_every_good_point_as_true_negative(ctx):
  """... and +inf is exceeded by nothing: both thresholds' TN lanes hold the count of good points."""
  thr = np.array([np.nan, np.inf])
  p, t, mask = CC.contingency_case(5, NLEAD, NROW, 65, np.float32, _hip.FLAG_SKIPNA, NROW, False)
  rc, _, got = _launch(ctx, p, t, mask, thr, False, NROW, _hip.FLAG_SKIPNA)
  _hip.check(rc, 'nan threshold')
  good = (~np.isnan(p) & ~np.isnan(t)).sum(axis=(1, 2)).astype(np.float64)
  for k in range(2):
    np.testing.assert_array_equal(got[:, 0, 3 * 2 + k, 0], good)  # TN
    for cell in range(3):
      assert (got[:, 0, cell * 2 + k, 0] == 0).all()


def test_refusals(ctx):
  thr = CC.thresholds(KMAX)
  p, t, mask = CC.contingency_case(9, NLEAD, NROW, 65, np.float32, 0, NROW, False)
  many = np.concatenate([thr, [0.5]])
  rc, _, got = _launch(ctx, p, t, mask, many, False, NROW, 0, nthr=KMAX + 1, sentinel=-77.0)
  with pytest.raises(_hip.WbxError, match='thresholds per launch'):
    _hip.check(rc, 'too many thresholds')
  assert (got == -77.0).all()
  rc, _, got = _launch(ctx, p, t, mask, thr, False, NROW, 0, dtype_code=7, sentinel=-77.0)
  with pytest.raises(_hip.WbxError, match='unknown dtype'):
    _hip.check(rc, 'bad dtype')
  assert (got == -77.0).all()
  rc, _, got = _launch(ctx, p, t, mask, thr, False, NROW, _hip.FLAG_MASKED, with_mask=False, sentinel=-77.0)
  with pytest.raises(_hip.WbxError, match='mask is NULL'):
    _hip.check(rc, 'masked without a mask')
  assert (got == -77.0).all()
