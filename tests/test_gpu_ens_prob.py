"""wbx_ens_prob_contingency_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the integer
restatement (tests/ens_prob_cases.py), bit for bit -- a partial is an integer count held in float64 (or NaN), so no tolerance applies.

Frame (lead = 2, row = 5, x); x summed and kept; all rows per partial and 2 (a ragged last chunk); plain / masked / skipna /
masked + skipna; float32 and float64; the member axis outermost (stride = lead * row * x) and innermost (stride 1, x stride M); the
mask depends on (row, x) only.  M in 1, 7, 8, 9, 51, 256 (whole groups of eight member loads, a remainder, both); row lengths 1, 63,
64, 65, 257 with plan.vec == 1 and 4, 256 with plan.vec == 4 (accepted, read with dword loads) at every M; (event
thresholds, slots) in (1, 1), (1, 5), (4, 4), (16, 1), (1, 16), (3, 5), every one of them in every mode, dtype and kernel at M = 9
and dealt round over the launches of the other M.  The event thresholds hold a NaN, +-inf, +-1e40, -0.0 beside 0.0 and 0.1, which
float32 cannot hold, with float32(0.1) and its neighbours among the inputs; the slots hold an empty one and runs beyond 0..M.  NaN
outputs (a NaN member or target under a valid point poisons its partial unless skipna counts it out) must be NaN on both sides at
the same positions, at least three quarters of the expected partials of a plain / masked case are finite, and under skipna every
output is finite while the statistic itself holds NaNs."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import ens_prob_cases as EP

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked+skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
MEMBER, LEAD, ROW, X = 'number', 'lead_time', 'row', 'x'
SDIMS = (LEAD, ROW, X)
NLEAD, NROW = 2, 5
SENTINEL = -77.0
PAIRS = [(1, 1), (1, 5), (4, 4), (16, 1), (1, 16), (3, 5)]  # (nthr, nslot)
NX_DWORD = (1, 63, 64, 65, 257)
NX_VEC4 = (4, 256)


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


def _launch(ctx, p, t, mask, thr, slots, x_kept, depth_chunk, flags, vec4=False, nthr=None, nslot=None, m=None, dtype_code=None,
            with_mask=True, sentinel=None, ndepth0=False, plan_edit=None):
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
  slots = np.ascontiguousarray(slots, np.int32).reshape(-1, 2)
  k, j = len(thr), len(slots)
  nl = _hip.EPC_CELLS * k * j
  lanes = 2 * nl if flags & _hip.FLAG_SKIPNA else (nl + 1 if flags & _hip.FLAG_MASKED else nl)
  shape = (nlead, plan.nchunk, lanes, plan.nj)
  if ndepth0:
    plan = dataclasses.replace(plan, ndepth=0)
  if plan_edit:
    plan = dataclasses.replace(plan, **plan_edit)
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  n = int(np.prod(shape))
  out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
  bufs = ctx.upload(_root(p)), ctx.upload(_root(t))
  tbuf, sbuf = ctx.upload(np.asarray(thr, np.float64)), ctx.upload(slots)
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  rc = ctx.lib.wbx_ens_prob_contingency_partial(ctx.handle, C.byref(dplan.struct), dtype_code, p.shape[0] if m is None else m,
                                                lay_p.stride(MEMBER), k if nthr is None else nthr, _ptr(tbuf), j if nslot is None else nslot,
                                                _ptr(sbuf), _ptr(bufs[0]), _ptr(bufs[1]), _ptr(mask_buf), _ptr(out))
  return rc, plan, ctx.download(out.ptr, shape, np.float64)


def _check(got, want, tag):
  assert got.shape == want.shape, (tag, got.shape, want.shape)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{tag}: NaN positions')
  np.testing.assert_array_equal(got, want, err_msg=tag)  # (assert_array_equal takes NaN == NaN) every lane, bit for bit


def _finite_share(want, flags, nl, nan, what):
  """The restatement alone: where the NaNs went."""
  if flags & _hip.FLAG_SKIPNA:
    assert np.isfinite(want).all() and nan.any(), what
  else:
    share = float(np.isfinite(want[:, :, :nl]).all(axis=2).mean())
    assert share >= 0.75, (what, 'finite share of the partials', share)


@pytest.mark.parametrize('m', [1, 7, 8, 9, 51, 256])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_bit_equal(ctx, mode, dtype, m):
  flags = MODES[mode]
  widths = NX_DWORD + NX_VEC4
  seed, launches = 0, 0
  for nx in widths:
    for depth_chunk in (NROW, 2):
      for x_kept in (False, True):
        seed += 1
        nthr, nslot = PAIRS[(seed + m) % len(PAIRS)]
        thr, slots = EP.event_thresholds(nthr), EP.slot_runs(nslot, m)
        p0, t, mask = EP.ens_prob_case(1000 * m + seed, m, NLEAD, NROW, nx, dtype, flags, depth_chunk, x_kept, thr)
        what = f'M={m} K={nthr} J={nslot} nx={nx} dc={depth_chunk} x_kept={x_kept} {mode} {np.dtype(dtype).name}'
        want = EP.expected(p0, t, thr, slots, mask, flags, depth_chunk, x_kept)
        _finite_share(want, flags, 4 * nthr * nslot, EP.nan_points(p0, t), what)
        for innermost in (False, True):
          p = np.moveaxis(np.ascontiguousarray(np.moveaxis(p0, 0, -1)), -1, 0) if innermost else p0
          if m > 1:
            assert p.strides[0] == (p.itemsize if innermost else p.itemsize * NLEAD * NROW * nx), what
          vec4 = nx in NX_VEC4 and not innermost
          rc, plan, got = _launch(ctx, p, t, mask, thr, slots, x_kept, depth_chunk, flags, vec4=vec4)
          _hip.check(rc, what)
          launches += 1
          _check(got, want, f'{what} innermost={innermost} vec={plan.vec}')
  assert launches == len(widths) * 2 * 2 * 2


@pytest.mark.parametrize('pair', PAIRS, ids=[f'K{k}-J{j}' for k, j in PAIRS])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_pair_count_in_every_mode_dtype_and_kernel(ctx, mode, pair):
  nthr, nslot = pair
  flags = MODES[mode]
  thr, slots = EP.event_thresholds(nthr), EP.slot_runs(nslot, 9)
  for dtype in (np.float32, np.float64):
    for x_kept in (False, True):
      for depth_chunk in (NROW, 2):
        p, t, mask = EP.ens_prob_case(31 + nthr + nslot, 9, NLEAD, NROW, 65, dtype, flags, depth_chunk, x_kept, thr)
        what = f'K={nthr} J={nslot} {mode} {np.dtype(dtype).name} x_kept={x_kept} dc={depth_chunk}'
        want = EP.expected(p, t, thr, slots, mask, flags, depth_chunk, x_kept)
        _finite_share(want, flags, 4 * nthr * nslot, EP.nan_points(p, t), what)
        rc, _, got = _launch(ctx, p, t, mask, thr, slots, x_kept, depth_chunk, flags)
        _hip.check(rc, what)
        _check(got, want, what)


def test_padding_slots_and_the_float32_threshold(ctx):
  """K = 2, 3, 5 and 9 run in the kernels built for 4, 4, 8 and 16 threshold slots and J = 2, 3 in those built for more pairs: members
  and targets at +inf meet no phantom threshold.  float32(0.1) exceeds the threshold 0.1, its lower neighbour does not; -0.0 does
  not exceed 0.0; nothing exceeds a NaN threshold."""
  thr16 = EP.event_thresholds(16)
  for nthr, nslot in ((2, 2), (3, 3), (5, 3), (9, 1), (2, 8)):
    thr, slots = thr16[:nthr].copy(), EP.slot_runs(16, 5)[:nslot]
    p, t, mask = EP.ens_prob_case(77 + nthr, 5, NLEAD, NROW, 65, np.float32, 0, NROW, True, thr)
    p[:, 0, 1, :8], t[0, 1, :8] = np.inf, np.inf
    want = EP.expected(p, t, thr, slots, mask, 0, NROW, True)
    rc, _, got = _launch(ctx, p, t, mask, thr, slots, True, NROW, 0)
    _hip.check(rc, f'K={nthr} J={nslot}')
    _check(got, want, f'K={nthr} J={nslot}')
  thr = np.array([0.1, 0.0, np.nan])
  slots = np.array([[1, 3], [0, 0]], np.int32)
  tenth = np.float32(0.1)
  p = np.empty((3, 1, 1, 4), np.float32)
  p[:, 0, 0, 0] = (tenth, np.nextafter(tenth, np.float32(-1)), np.nextafter(tenth, np.float32(1)))  # c = 2, 3, 0 (NaN: none)
  p[:, 0, 0, 1] = (-0.0, 0.0, -1.0)                                                                # c = 0, 0, 0
  p[:, 0, 0, 2] = (np.inf, -np.inf, 1e-45)                                                         # c = 1, 2, 0
  p[:, 0, 0, 3] = (0.5, 0.5, 0.5)                                                                  # c = 3, 3, 0
  t = np.array([[[tenth, -0.0, np.nextafter(tenth, np.float32(-1)), 1.0]]], np.float32)
  p, t = np.tile(p, (1, NLEAD, 2, 1)), np.tile(t, (NLEAD, 2, 1))  # (two keys, two rows of the same four points)
  np.testing.assert_array_equal(EP.counts(p, thr)[0, 0], [[2, 3, 0], [0, 0, 0], [1, 2, 0], [3, 3, 0]])
  np.testing.assert_array_equal(EP.observed(t, thr)[0, 0], [[1, 1, 0], [0, 0, 0], [0, 1, 0], [1, 1, 0]])
  for x_kept in (True, False):
    want = EP.expected(p, t, thr, slots, None, 0, 2, x_kept)
    rc, _, got = _launch(ctx, p, t, None, thr, slots, x_kept, 2, 0)
    _hip.check(rc, 'edges')
    _check(got, want, f'edges x_kept={x_kept}')
  p64, t64 = p.astype(np.float64), t.astype(np.float64)
  p64[0, :, :, 0], p64[1, :, :, 0], p64[2, :, :, 0] = 0.1, np.nextafter(0.1, 1), np.nextafter(0.1, -1)  # c_0 = 1 (0.1 > 0.1 is false)
  assert EP.counts(p64, thr)[0, 0, 0, 0] == 1
  want = EP.expected(p64, t64, thr, slots, None, 0, 2, True)
  rc, _, got = _launch(ctx, p64, t64, None, thr, slots, True, 2, 0)
  _hip.check(rc, 'edges, float64')
  _check(got, want, 'edges float64')


def test_refusals_leave_the_output_untouched(ctx):
  thr, slots = EP.event_thresholds(16), EP.slot_runs(1, 3)
  p, t, mask = EP.ens_prob_case(9, 3, NLEAD, NROW, 65, np.float32, 0, NROW, False, thr)
  thr4, slots4, slots5 = EP.event_thresholds(4), EP.slot_runs(4, 3), EP.slot_runs(5, 3)
  cases = [
      ('pairs per launch', dict(thr=thr4, slots=slots5, flags=0)),                       # 4 x 5 = 20
      ('pairs per launch', dict(thr=np.concatenate([thr, [0.5]]), slots=slots, flags=0)),  # 17 x 1
      ('pairs per launch', dict(thr=thr, slots=slots, flags=0, nthr=0)),
      ('pairs per launch', dict(thr=thr, slots=slots, flags=0, nslot=0)),
      ('pairs per launch', dict(thr=thr, slots=slots, flags=0, nslot=-1)),
      ('members', dict(thr=thr, slots=slots, flags=0, m=257)),
      ('members', dict(thr=thr, slots=slots, flags=0, m=0)),
      ('unknown dtype', dict(thr=thr, slots=slots, flags=0, dtype_code=7)),
      ('mask is NULL', dict(thr=thr, slots=slots, flags=_hip.FLAG_MASKED, with_mask=False)),
      ('flags other than MASKED', dict(thr=thr, slots=slots, flags=_hip.FLAG_FAIR)),
      ('flags other than MASKED', dict(thr=thr, slots=slots, flags=_hip.FLAG_SKIPNA_ENS)),
      ('no plane mode', dict(thr=thr4, slots=slots4, flags=0, plan_edit={'plane_rows': 1})),
      ('2\\^32 or more points', dict(thr=thr4, slots=slots4, flags=0, plan_edit={'depth_chunk': 2 ** 26, 'nchunk': 1})),  # x 65 >= 2^32
  ]
  for message, kw in cases:
    flags = kw.pop('flags')
    rc, _, got = _launch(ctx, p, t, mask, kw.pop('thr'), kw.pop('slots'), False, NROW, flags, sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message
  # sixteen pairs are fine
  rc, _, got = _launch(ctx, p, t, mask, thr4, slots4, False, NROW, 0, sentinel=SENTINEL)
  _hip.check(rc, '4 x 4')
  _check(got, EP.expected(p, t, thr4, slots4, mask, 0, NROW, False), '4 x 4')


@pytest.mark.parametrize('mode', list(MODES))
def test_empty_extents(ctx, mode):
  thr, slots = EP.event_thresholds(3), EP.slot_runs(5, 3)
  p, t, mask = EP.ens_prob_case(4, 3, NLEAD, NROW, 65, np.float32, 0, NROW, False, thr)
  for x_kept in (False, True):
    rc, _, got = _launch(ctx, p, t, mask, thr, slots, x_kept, NROW, MODES[mode], sentinel=SENTINEL, ndepth0=True)
    _hip.check(rc, 'ndepth == 0')
    assert (got == 0.0).all() and not np.signbit(got).any()
    rc, _, got = _launch(ctx, p, t, mask, thr, slots, x_kept, NROW, MODES[mode], sentinel=SENTINEL, plan_edit={'nkey': 0})
    _hip.check(rc, 'nkey == 0')
    assert (got == SENTINEL).all()
  rc, _, got = _launch(ctx, p, t, mask, thr, slots, False, NROW, MODES[mode], sentinel=SENTINEL, plan_edit={'nx': 0})
  _hip.check(rc, 'nx == 0')
  assert (got == 0.0).all()
