"""wbx_ens_brier_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the integer restatement
(tests/brier_cases.py), bit for bit -- a partial is float64(S) / float64(D) or float64(S) / float64(D * D) of an exact integer sum
S, so no tolerance applies.

Frame (lead = 2, row, x): two keys; rows 1 (one chunk), 3 (one chunk) and 5 in chunks of 3 (two chunks, the last ragged); row
lengths 1, 63, 64, 65, 130; x summed and kept; plain / masked / skipna / masked + skipna; float32 and float64; M in 1, 2, 7, 8, 9,
51, 256 (the kernel walks the members in groups of 8); the denominator M and M + 1 (1 for M = 1); the member axis stored
outermost, in the middle and innermost (member stride 1, x stride M); the mask depends on (row, x) only.  K in 1, 2, 4, 5, 8, 9, 16
-- the kernels are built for 1, 4, 8 and 16 threshold slots -- goes round the cases of a parameter set, the full list against
every M.  The 16 thresholds hold +-inf, +-1e40 (beyond the float32 range), 0.1 (no float32), 0.0 and -0.0, a NaN, a duplicate,
unsorted; the inputs hold values equal to a threshold, float32(0.1) and its neighbours, +-inf, +-0.0 and NaNs by mode.  One
chunk of 260 rows (more than the 64 x 4 a 256-thread block deals in one batch) at row length 3; plan.vec == 4 at row lengths 4,
256, 260.  NaN outputs must be NaN on both sides at the same positions."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import brier_cases as BC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked+skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
MEMBER, LEAD, ROW, X = 'number', 'lead_time', 'row', 'x'
SDIMS = (LEAD, ROW, X)
NLEAD = 2
SENTINEL = -77.0
NX = (1, 63, 64, 65, 130)
ROWS = ((1, 1), (3, 3), (5, 3))  # (rows, rows per chunk)
NTHRS = (1, 2, 4, 5, 8, 9, 16)
MEMBERS = (1, 2, 7, 8, 9, 51, 256)


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


def _launch(ctx, p, t, mask, thr, denom, x_kept, depth_chunk, flags, vec4=False, nthr=None, m=None, dtype_code=None, with_mask=True,
            with_thr=True, sentinel=None, plan_edit=None):
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
  nl = _hip.BRIER_STATS * len(thr)
  lanes = 2 * nl if flags & _hip.FLAG_SKIPNA else (nl + 1 if flags & _hip.FLAG_MASKED else nl)
  shape = (nlead, plan.nchunk, lanes, plan.nj)
  if plan_edit:
    plan = dataclasses.replace(plan, **plan_edit)
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  n = int(np.prod(shape))
  out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
  bufs = ctx.upload(_root(p)), ctx.upload(_root(t))
  tbuf = ctx.upload(np.asarray(thr, np.float64)) if with_thr else None
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  rc = ctx.lib.wbx_ens_brier_partial(ctx.handle, C.byref(dplan.struct), dtype_code, p.shape[0] if m is None else m, lay_p.stride(MEMBER),
                                     denom, len(thr) if nthr is None else nthr, _ptr(tbuf), _ptr(bufs[0]), _ptr(bufs[1]), _ptr(mask_buf),
                                     _ptr(out))
  return rc, plan, ctx.download(out.ptr, shape, np.float64)


def _check(got, want, tag):
  assert got.shape == want.shape, (tag, got.shape, want.shape)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{tag}: NaN positions')
  np.testing.assert_array_equal(got, want, err_msg=tag)  # (assert_array_equal takes NaN == NaN) every lane, bit for bit


@pytest.mark.parametrize('m', MEMBERS, ids=[f'M{m}' for m in MEMBERS])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_bit_equal(ctx, mode, dtype, m):
  flags = MODES[mode]
  denoms = (1,) if m == 1 else (m, m + 1)
  axes = (0,) if m == 1 else (0, 1, 3)
  turn = MEMBERS.index(m) + (3 if dtype == np.float64 else 0) + list(MODES).index(mode)  # (where the K go round from)
  seed, launches, poisoned, counted_out = 0, 0, 0, 0
  for nx in NX:
    for nrow, depth_chunk in ROWS:
      for x_kept in (False, True):
        nthr = NTHRS[(turn + seed) % len(NTHRS)]
        seed += 1
        thr = BC.thresholds(nthr)
        p0, t, mask = BC.brier_case(1000 * m + seed, m, NLEAD, nrow, nx, dtype, flags, depth_chunk, x_kept, thr)
        counted_out += int(BC.nan_points(p0, t).sum())
        for denom in denoms:
          what = f'M={m} D={denom} K={nthr} nx={nx} rows={nrow}/{depth_chunk} x_kept={x_kept} {mode} {np.dtype(dtype).name}'
          want = BC.expected(p0, t, thr, denom, mask, flags, depth_chunk, x_kept)
          if flags & _hip.FLAG_SKIPNA:
            assert np.isfinite(want).all(), what
          else:
            poisoned += int(np.isnan(want).sum())
          for axis in axes:
            p = BC.member_view(p0, axis)
            if m > 1:
              assert p.strides[0] == p.itemsize * {0: NLEAD * nrow * nx, 1: nrow * nx, 3: 1}[axis], what
            rc, plan, got = _launch(ctx, p, t, mask, thr, denom, x_kept, depth_chunk, flags)
            _hip.check(rc, what)
            launches += 1
            assert plan.nchunk == -(-nrow // depth_chunk)
            _check(got, want, f'{what} member axis {axis}')
  assert launches == len(NX) * len(ROWS) * 2 * len(denoms) * len(axes)
  assert counted_out if flags & _hip.FLAG_SKIPNA else poisoned  # the NaNs were there


@pytest.mark.parametrize('nthr', NTHRS)
def test_every_threshold_count_and_slot_size(ctx, nthr):
  """K at every slot size the kernels are built for and one past each; members and targets at -inf / +inf meet no phantom
  threshold in the padding slots."""
  thr = BC.thresholds(nthr)
  for dtype in (np.float32, np.float64):
    for flags in (0, _hip.FLAG_MASKED | _hip.FLAG_SKIPNA):
      p, t, mask = BC.brier_case(77 + nthr, 9, NLEAD, 5, 65, dtype, flags, 3, True, thr)
      p[:, 0, 0, :8], t[0, 0, :8] = -np.inf, -np.inf
      p[:, 0, 1, :8], t[0, 1, :8] = np.inf, np.inf
      for x_kept in (True, False):
        for denom in (9, 10):
          want = BC.expected(p, t, thr, denom, mask, flags, 3, x_kept)
          rc, _, got = _launch(ctx, p, t, mask, thr, denom, x_kept, 3, flags)
          _hip.check(rc, f'K={nthr}')
          _check(got, want, f'K={nthr} D={denom} x_kept={x_kept} flags={flags} {np.dtype(dtype).name}')


def test_a_chunk_taller_than_one_batch_of_rows(ctx):
  """260 rows in one chunk: a 256-thread block deals 64 rows to each of its 4 waves per batch, so the second batch is a short one."""
  thr = BC.thresholds(5)
  for mode, flags in MODES.items():
    p, t, mask = BC.brier_case(5, 7, NLEAD, 260, 3, np.float32, flags, 260, False, thr)
    for x_kept in (False, True):
      for denom in (7, 8):
        want = BC.expected(p, t, thr, denom, mask, flags, 260, x_kept)
        rc, plan, got = _launch(ctx, p, t, mask, thr, denom, x_kept, 260, flags)
        _hip.check(rc, mode)
        assert plan.nchunk == 1 and plan.depth_chunk == 260
        _check(got, want, f'260 rows {mode} x_kept={x_kept} D={denom}')


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_vec4_plans_are_accepted(ctx, dtype):
  thr = BC.thresholds(4)
  for nx in (4, 256, 260):
    for mode, flags in MODES.items():
      for x_kept in (False, True):
        p, t, mask = BC.brier_case(nx, 8, NLEAD, 5, nx, dtype, flags, 3, x_kept, thr)
        want = BC.expected(p, t, thr, 8, mask, flags, 3, x_kept)
        rc, plan, got = _launch(ctx, p, t, mask, thr, 8, x_kept, 3, flags, vec4=True)
        _hip.check(rc, mode)
        assert plan.vec == 4
        _check(got, want, f'vec4 nx={nx} {mode} x_kept={x_kept}')


def test_edges_by_hand(ctx):
  """Values worked out by hand, not by the restatement: float32(0.1) exceeds 0.1 and its lower neighbour does not; -0.0 > 0.0 is
  false; +inf exceeds every finite threshold and 1e40, -inf nothing but no threshold either; a NaN threshold is never exceeded; a
  duplicate threshold repeats its lane."""
  tenth = np.float32(0.1)
  thr = np.array([0.1, 0.0, np.nan, 1e40, 0.1])
  p = np.empty((3, 1, 1, 4), np.float32)
  p[:, 0, 0, 0] = (tenth, np.nextafter(tenth, np.float32(-1)), 0.5)      # c = 2, 3, 0, 0, 2
  p[:, 0, 0, 1] = (-0.0, 0.0, -1.0)                                      # c = 0, 0, 0, 0, 0
  p[:, 0, 0, 2] = (np.inf, -np.inf, 1e-45)                               # c = 1, 2, 0, 1, 1
  p[:, 0, 0, 3] = (0.5, 0.5, 0.5)                                        # c = 3, 3, 0, 0, 3
  t = np.array([[[tenth, -0.0, np.inf, np.nextafter(tenth, np.float32(-1))]]], np.float32)  # o = 11001, 00000, 11011, 01000
  e = np.array([[2 - 3, 3 - 3, 0, 0, 2 - 3], [0, 0, 0, 0, 0], [1 - 3, 2 - 3, 0, 1 - 3, 1 - 3], [3, 3 - 3, 0, 0, 3]], np.int64)  # D = 3
  np.testing.assert_array_equal(BC.counts(p, thr)[0, 0] - 3 * BC.observed(t, thr)[0, 0], e)
  rc, _, got = _launch(ctx, p, t, None, thr, 3, True, 1, 0)
  _hip.check(rc, 'edges')
  want = np.concatenate([e / 3.0, np.abs(e) / 3.0, e * e / 9.0], axis=1).T  # [lane, x]
  _check(got[0, 0], want, 'edges, x kept')
  rc, _, got = _launch(ctx, p, t, None, thr, 3, False, 1, 0)
  _hip.check(rc, 'edges')
  s = np.concatenate([e, np.abs(e), e * e], axis=1).sum(axis=0).astype(np.float64)
  _check(got[0, 0, :, 0], s / np.array([3.0] * 10 + [9.0] * 5), 'edges, x summed')
  # the plotting position: D = 4
  rc, _, got = _launch(ctx, p, t, None, thr, 4, True, 1, 0)
  _hip.check(rc, 'edges')
  e4 = BC.counts(p, thr)[0, 0] - 4 * BC.observed(t, thr)[0, 0]
  _check(got[0, 0], np.concatenate([e4 / 4.0, np.abs(e4) / 4.0, e4 * e4 / 16.0], axis=1).T, 'edges, D = 4')
  # float64: 0.1 > 0.1 is false, its upper neighbour exceeds it
  p64, t64 = p.astype(np.float64), t.astype(np.float64)
  p64[:, 0, 0, 0] = (0.1, np.nextafter(0.1, 1), np.nextafter(0.1, -1))
  assert BC.counts(p64, thr)[0, 0, 0, 0] == 1
  rc, _, got = _launch(ctx, p64, t64, None, thr, 3, True, 1, 0)
  _hip.check(rc, 'edges, float64')
  _check(got, BC.expected(p64, t64, thr, 3, None, 0, 1, True), 'edges float64')
  # a NaN member, a NaN target; under a masked-out point they leave no trace
  pn, tn = np.tile(p, (1, 1, 2, 1)), np.tile(t, (1, 2, 1))
  pn[1, 0, 0, 0], tn[0, 1, 2] = np.nan, np.nan
  hide = np.ones((2, 4), bool)
  hide[0, 0] = hide[1, 2] = False
  for flags, mask in ((0, None), (_hip.FLAG_MASKED, hide), (_hip.FLAG_MASKED, ~hide), (_hip.FLAG_SKIPNA, None)):
    rc, _, got = _launch(ctx, pn, tn, mask, thr, 3, True, 2, flags)
    _hip.check(rc, 'NaNs')
    _check(got, BC.expected(pn, tn, thr, 3, mask, flags, 2, True), f'NaNs flags={flags}')
    nl = 15
    if flags == 0:
      assert np.isnan(got[0, 0, :nl, 0]).all() and np.isnan(got[0, 0, :nl, 2]).all() and np.isfinite(got[0, 0, :, (1, 3)]).all()
    elif mask is hide:
      assert np.isfinite(got).all() and (got[0, 0, nl] == [1, 2, 1, 2]).all()
    elif flags == _hip.FLAG_MASKED:
      assert np.isnan(got[0, 0, :nl, 0]).all() and (got[0, 0, :nl, 1] == 0).all() and (got[0, 0, nl] == [1, 0, 1, 0]).all()
    else:
      assert np.isfinite(got).all() and (got[0, 0, nl:] == [1, 2, 1, 2]).all()


def test_refusals_leave_the_output_untouched(ctx):
  thr = BC.thresholds(16)
  p, t, mask = BC.brier_case(9, 3, NLEAD, 5, 65, np.float32, 0, 5, False, thr)
  thr4 = BC.thresholds(4)
  cases = [
      ('thresholds per launch', dict(thr=np.concatenate([thr, [0.5]]), denom=3, flags=0)),
      ('thresholds per launch', dict(thr=thr, denom=3, flags=0, nthr=0)),
      ('thresholds per launch', dict(thr=thr, denom=3, flags=0, nthr=-1)),
      ('members', dict(thr=thr, denom=257, flags=0, m=257)),
      ('members', dict(thr=thr, denom=0, flags=0, m=0)),
      ('denom is M or M \\+ 1', dict(thr=thr, denom=2, flags=0)),
      ('denom is M or M \\+ 1', dict(thr=thr, denom=5, flags=0)),
      ('denom is M or M \\+ 1', dict(thr=thr, denom=2, flags=0, m=1)),  # one member: the deterministic pair, D = 1
      ('unknown dtype', dict(thr=thr, denom=3, flags=0, dtype_code=7)),
      ('flags other than MASKED', dict(thr=thr, denom=3, flags=_hip.FLAG_FAIR)),
      ('flags other than MASKED', dict(thr=thr, denom=3, flags=_hip.FLAG_SKIPNA_ENS)),
      ('mask is NULL', dict(thr=thr, denom=3, flags=_hip.FLAG_MASKED, with_mask=False)),
      ('no plane mode', dict(thr=thr4, denom=3, flags=0, plan_edit={'plane_rows': 1})),
      ('threshold table is NULL', dict(thr=thr4, denom=3, flags=0, with_thr=False)),
      ('2\\^53 or more per partial', dict(thr=thr4, denom=4, flags=0, plan_edit={'depth_chunk': 2 ** 43, 'nchunk': 1})),  # x 65 x 16 >= 2^53
  ]
  for message, kw in cases:
    flags = kw.pop('flags')
    rc, _, got = _launch(ctx, p, t, mask, kw.pop('thr'), kw.pop('denom'), False, 5, flags, sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message
  # folded x weights
  rc, _, got = _launch(ctx, p, t, mask, thr4, 3, False, 5, 0, sentinel=SENTINEL, plan_edit={'x_weights': np.ones(65)})
  assert rc == -1 and (got == SENTINEL).all()
  with pytest.raises(_hip.WbxError, match='no folded x weights'):
    _hip.check(rc, 'x weights')
  # sixteen thresholds and one member are fine
  rc, _, got = _launch(ctx, p, t, mask, thr, 3, False, 5, 0, sentinel=SENTINEL)
  _hip.check(rc, '16 thresholds')
  _check(got, BC.expected(p, t, thr, 3, mask, 0, 5, False), '16 thresholds')
  rc, _, got = _launch(ctx, p[:1], t, mask, thr4, 1, False, 5, 0, sentinel=SENTINEL)
  _hip.check(rc, 'M = 1')
  _check(got, BC.expected(p[:1], t, thr4, 1, mask, 0, 5, False), 'M = 1')


@pytest.mark.parametrize('mode', list(MODES))
def test_empty_extents(ctx, mode):
  thr = BC.thresholds(4)
  p, t, mask = BC.brier_case(4, 3, NLEAD, 5, 65, np.float32, 0, 5, False, thr)
  for x_kept in (False, True):
    rc, _, got = _launch(ctx, p, t, mask, thr, 3, x_kept, 5, MODES[mode], sentinel=SENTINEL, plan_edit={'ndepth': 0})
    _hip.check(rc, 'ndepth == 0')
    assert (got == 0.0).all() and not np.signbit(got).any()
    rc, _, got = _launch(ctx, p, t, mask, thr, 3, x_kept, 5, MODES[mode], sentinel=SENTINEL, plan_edit={'nkey': 0})
    _hip.check(rc, 'nkey == 0')
    assert (got == SENTINEL).all()
  rc, _, got = _launch(ctx, p, t, mask, thr, 3, False, 5, MODES[mode], sentinel=SENTINEL, plan_edit={'nx': 0})
  _hip.check(rc, 'nx == 0')
  assert (got == 0.0).all()
