"""wbx_ens_quantile_error_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the float64 restatement
(tests/quantile_error_cases.py: np.quantile of the float64 members, q - t, |.|, (.)^2, masked / skipna sums).

How a partial is compared (the cases module derives it): x kept -- a lane adds its rows in order, bit for bit; exactly summable
inputs (small integers, levels that are multiples of 1/8) -- bit for bit whatever the order; x summed over general values -- within
n 2^-53 sum|v| of the correctly rounded sum, from the case's own values.  Count lanes are integers: bit for bit.  NaN and
infinite partials must be the same on both sides at the same positions.

Frame (lead = 2, row, x): two keys (three in one test); rows 1 (one chunk), 3 (one chunk) and 5 in chunks of 3 (two chunks, the last
ragged); row lengths 1, 63, 64, 65, 130; x summed and kept; plain / masked / skipna / masked + skipna; float32 and float64; M at
every generated network size and on both sides of every padding step; the member axis stored outermost and innermost (member
stride 1, x stride M) and a row-fastest frame (x strided); Q in 1, 2, 3, 5, 9, 16 -- the kernels are built for 1, 4, 8 and 16
quantile slots -- goes round the cases of a parameter set.  The levels hold 0, 1 (the upper rank clamps), 0.5, 0.1, 0.9, 1/3 and one
with g just under and one just over 0.5; the inputs hold ties, a NaN member, a NaN target, a +inf and a -inf member (inf * 0 at
g == 0), points whose members are all +inf, a NaN that the mask hides, and x = 0 masked out whole."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import quantile_error_cases as QC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked+skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
MEMBER, LEAD, ROW, X = 'number', 'lead_time', 'row', 'x'
SDIMS = (LEAD, ROW, X)
NLEAD = 2
SENTINEL = -77.0
NX = (1, 63, 64, 65, 130)
ROWS = ((1, 1), (3, 3), (5, 3))  # (rows, rows per chunk)
NQS = (1, 2, 3, 5, 9, 16)
STORED = ('outer', 'inner', 'row_fastest')  # how p is stored; t is row-fastest with the last, C order else


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


def _bounds(q, m):
  arr = (_hip.IvlBoundStruct * max(len(q), 1))()
  for b, level in zip(arr, q):
    b.k, b.g = QC.bound(level, m)
    b.c_off = 1 << 40  # ignored by the entry
  return arr


def _stored(p, t, how):
  if how == 'outer':
    return QC.member_view(p, 0), np.ascontiguousarray(t)
  if how == 'inner':
    return QC.member_view(p, 3), np.ascontiguousarray(t)
  return QC.row_fastest(p), QC.row_fastest(t)


def _launch(ctx, p, t, mask, q, x_kept, depth_chunk, flags, nq=None, m=None, dtype_code=None, with_mask=True, bounds='table',
            with_t=True, sentinel=None, plan_edit=None, block_threads=None):
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
                               flags=flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA), allow_vec4=False, force_x_dim=X)
  dc = min(depth_chunk, plan.ndepth)
  plan = dataclasses.replace(plan, depth_chunk=dc, nchunk=-(-plan.ndepth // dc), flags=flags)
  if block_threads is not None:
    plan = dataclasses.replace(plan, block_threads=block_threads)
  assert plan.x_kept == x_kept and plan.a_dims == (LEAD,) and plan.depth_dims == (ROW,) and not plan.bk_dims and not plan.br_dims, plan
  nl = _hip.QERR_STATS * len(q)
  lanes = 2 * nl if flags & _hip.FLAG_SKIPNA else (nl + 1 if flags & _hip.FLAG_MASKED else nl)
  shape = (nlead, plan.nchunk, lanes, plan.nj)
  if plan_edit:
    plan = dataclasses.replace(plan, **plan_edit)
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  n = int(np.prod(shape))
  out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
  bufs = ctx.upload(_root(p)), ctx.upload(_root(t))
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  mm = p.shape[0] if m is None else m
  table = _bounds(q, p.shape[0]) if isinstance(bounds, str) else bounds
  rc = ctx.lib.wbx_ens_quantile_error_partial(ctx.handle, C.byref(dplan.struct), dtype_code, mm, lay_p.stride(MEMBER),
                                              len(q) if nq is None else nq, table, _ptr(bufs[0]), _ptr(bufs[1]) if with_t else None,
                                              _ptr(mask_buf), _ptr(out))
  return rc, plan, ctx.download(out.ptr, shape, np.float64)


def _check(got, want, tol, tag):
  """Every lane of every partial: NaN and infinities as they are, finite numbers within `tol` (0: bit for bit)."""
  assert got.shape == want.shape == tol.shape, (tag, got.shape, want.shape)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{tag}: NaN positions')
  fin = np.isfinite(want)
  np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=f'{tag}: infinities')
  err = np.abs(got[fin] - want[fin])
  worst = (err - tol[fin]).max() if err.size else 0.0
  assert worst <= 0.0, (tag, 'largest excess over the bound', worst, 'largest error', err.max(), 'largest bound', tol[fin].max())


@pytest.mark.parametrize('m', QC.MEMBERS, ids=[f'M{m}' for m in QC.MEMBERS])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_against_float64(ctx, mode, dtype, m):
  flags = MODES[mode]
  turn = QC.MEMBERS.index(m) + (3 if dtype == np.float64 else 0) + list(MODES).index(mode)  # (where Q and the storage go round from)
  seed, launches, nonfinite, counted_out, exact_partials = 0, 0, 0, 0, 0
  for nx in NX:
    for nrow, depth_chunk in ROWS:
      for x_kept in (False, True):
        nq = NQS[(turn + seed) % len(NQS)]
        how = STORED[(turn // 2 + seed) % len(STORED)] if m > 1 else ('outer', 'row_fastest')[seed % 2]
        exact = (seed + turn) % 3 == 0
        seed += 1
        q = QC.levels(nq, m, exact)
        p0, t0, mask = QC.case(1000 * m + seed, m, NLEAD, nrow, nx, dtype, flags, exact=exact)
        what = f'M={m} Q={nq} nx={nx} rows={nrow}/{depth_chunk} x_kept={x_kept} {how} exact={exact} {mode} {np.dtype(dtype).name}'
        want, tol = QC.expected(p0, t0, q, mask, flags, depth_chunk, x_kept)
        if exact or x_kept:
          tol = np.zeros_like(tol)  # (any order of adding gives these sums; x kept adds in the restatement's order)
          exact_partials += want.size
        if flags & _hip.FLAG_SKIPNA:
          assert not np.isnan(want).any(), what
          counted_out += int(np.isnan(p0).any() or np.isnan(t0).any())
        else:
          nonfinite += int((~np.isfinite(want)).sum())
        p, t = _stored(p0, t0, how)
        if how == 'inner' and m > 1:
          assert p.strides[0] == p.itemsize and p.strides[3] == m * p.itemsize, what
        if how == 'row_fastest' and nrow > 1 and nx > 1:
          assert p.strides[2] == p.itemsize and t.strides[1] == t.itemsize and t.strides[2] == nrow * t.itemsize, what
        rc, plan, got = _launch(ctx, p, t, mask, q, x_kept, depth_chunk, flags)
        _hip.check(rc, what)
        launches += 1
        assert plan.nchunk == -(-nrow // depth_chunk)
        _check(got, want, tol, what)
  assert launches == len(NX) * len(ROWS) * 2 and exact_partials
  assert counted_out if flags & _hip.FLAG_SKIPNA else nonfinite  # the NaNs were there


@pytest.mark.parametrize('nq', (1, 2, 3, 4, 5, 8, 9, 16))
def test_every_quantile_count_and_slot_size(ctx, nq):
  """Q at every slot size the kernels are built for and one past each, three keys, both block sizes a float32 plan may name."""
  for dtype in (np.float32, np.float64):
    for flags in (0, _hip.FLAG_MASKED | _hip.FLAG_SKIPNA):
      q = QC.levels(nq, 9) if nq <= 3 else QC.levels(16, 9)[:nq]
      p, t, mask = QC.case(77 + nq, 9, 3, 5, 65, dtype, flags)
      for x_kept in (True, False):
        want, tol = QC.expected(p, t, q, mask, flags, 3, x_kept)
        for threads in (64, 256):
          rc, _, got = _launch(ctx, p, t, mask, q, x_kept, 3, flags, block_threads=threads)
          _hip.check(rc, f'Q={nq}')
          _check(got, want, tol, f'Q={nq} x_kept={x_kept} flags={flags} threads={threads} {np.dtype(dtype).name}')


def test_edges_by_hand(ctx):
  """Values worked out by hand, not by the restatement.  Five members 1, 2, 4, 8, 16 (stored unsorted), target 3:
  q = 0 -> 1, q = 1 -> 16 (the upper rank clamps at the last member), q = 0.5 -> 4, q = 0.125 -> h = 0.5: 2 - 1 * 0.5 = 1.5,
  q = 0.875 -> h = 3.5: 16 - 8 * 0.5 = 12.  A NaN member makes every quantile NaN; members (1, +inf) at q = 0: 1 + inf * 0 = NaN, at
  q = 1: d = inf - inf = NaN, at q = 0.5: inf - inf * 0.5 = NaN -- what NumPy gives; (-inf, 1) at q = 0: -inf + inf * 0 = NaN, at q = 1:
  k = 1, d = 0: 1 + 0 * 0 = 1, at q = 0.5: 1 - inf * 0.5 = -inf."""
  q = np.array([0.0, 1.0, 0.5, 0.125, 0.875])
  p = np.empty((5, 1, 1, 2), np.float32)
  p[:, 0, 0, 0] = (8, 1, 16, 4, 2)
  p[:, 0, 0, 1] = (8, 1, np.nan, 4, 2)
  t = np.array([[[3.0, 3.0]]], np.float32)
  e = np.array([1.0, 16.0, 4.0, 1.5, 12.0]) - 3.0
  want = np.concatenate([e, np.abs(e), e * e])
  for dtype in (np.float32, np.float64):
    rc, _, got = _launch(ctx, p.astype(dtype), t.astype(dtype), None, q, True, 1, 0)
    _hip.check(rc, 'edges')
    np.testing.assert_array_equal(got[0, 0, :, 0], want)
    assert np.isnan(got[0, 0, :, 1]).all()
    np.testing.assert_array_equal(QC.points(p.astype(dtype), t.astype(dtype), q)[0, 0, 0], want)  # (and the restatement agrees)
    rc, _, got = _launch(ctx, p.astype(dtype), t.astype(dtype), None, q, True, 1, _hip.FLAG_SKIPNA)
    _hip.check(rc, 'edges, skipna')
    np.testing.assert_array_equal(got[0, 0, :, 0], np.concatenate([want, np.ones(15)]))
    np.testing.assert_array_equal(got[0, 0, :, 1], np.zeros(30))
  q2 = np.array([0.0, 1.0, 0.5])
  p2 = np.array([[np.inf, 1.0], [1.0, -np.inf]], np.float64).reshape(2, 1, 1, 2)  # points (inf, 1) and (1, -inf)
  t2 = np.zeros((1, 1, 2))
  rc, _, got = _launch(ctx, p2, t2, None, q2, True, 1, 0)
  _hip.check(rc, 'infinities')
  assert np.isnan(got[0, 0, :, 0]).all()  # (1, inf): every level meets inf * 0 or inf - inf
  np.testing.assert_array_equal(got[0, 0, (1, 4, 7), 1], [1.0, 1.0, 1.0])  # (-inf, 1) at q = 1
  np.testing.assert_array_equal(got[0, 0, (2, 5, 8), 1], [-np.inf, np.inf, np.inf])  # at q = 0.5
  assert np.isnan(got[0, 0, (0, 3, 6), 1]).all()
  np.testing.assert_array_equal(np.isnan(got[0, 0]), np.isnan(QC.points(p2, t2, q2)[0, 0].T))
  # under skipna the lanes of q = 0 count no point and those of q = 1 and q = 0.5 the second: one count lane per value lane
  rc, _, got = _launch(ctx, p2, t2, None, q2, False, 1, _hip.FLAG_SKIPNA)
  _hip.check(rc, 'infinities, skipna')
  np.testing.assert_array_equal(got[0, 0, 9:, 0], [0, 1, 1] * 3)
  np.testing.assert_array_equal(got[0, 0, :9, 0], [0, 1, -np.inf, 0, 1, np.inf, 0, 1, np.inf])


def test_an_all_masked_partial_is_zero(ctx):
  q = QC.levels(3, 5)
  p, t, mask = QC.case(3, 5, NLEAD, 3, 65, np.float32, _hip.FLAG_MASKED)
  mask[:] = False
  p[0, 0, 0, 0], t[1, 1, 1] = np.nan, np.nan
  for flags in (_hip.FLAG_MASKED, _hip.FLAG_MASKED | _hip.FLAG_SKIPNA):
    for x_kept in (False, True):
      rc, _, got = _launch(ctx, p, t, mask, q, x_kept, 3, flags, sentinel=SENTINEL)
      _hip.check(rc, 'all masked')
      assert (got == 0.0).all() and not np.signbit(got).any()


def test_two_runs_of_one_case_are_bit_identical(ctx):
  q = QC.levels(16, 51)
  for dtype in (np.float32, np.float64):
    p, t, mask = QC.case(51, 51, NLEAD, 5, 130, dtype, 0, clean=True)
    for x_kept in (False, True):
      runs = [_launch(ctx, p, t, mask, q, x_kept, 3, _hip.FLAG_MASKED, sentinel=s)[2] for s in (SENTINEL, 5.0)]
      assert np.isfinite(runs[0]).all()
      np.testing.assert_array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))


def test_refusals_leave_the_output_untouched(ctx):
  q = QC.levels(16, 3)
  p, t, mask = QC.case(9, 3, NLEAD, 5, 65, np.float32, 0)
  q4 = q[:4]

  def table(k, g):
    arr = _bounds(q4, 3)
    arr[2].k, arr[2].g = k, g
    return arr
  cases = [
      ('quantiles per launch', dict(q=np.concatenate([q, [0.5]]))),
      ('quantiles per launch', dict(q=q, nq=0)),
      ('quantiles per launch', dict(q=q, nq=-1)),
      ('members', dict(q=q4, m=65)),
      ('members', dict(q=q4, m=0)),
      ('rank 3 outside 0..2', dict(q=q4, bounds=table(3, 0.0))),
      ('rank -1 outside 0..2', dict(q=q4, bounds=table(-1, 0.0))),
      ('weight 1 outside', dict(q=q4, bounds=table(1, 1.0))),
      ('weight -0.25 outside', dict(q=q4, bounds=table(1, -0.25))),
      ('weight nan outside', dict(q=q4, bounds=table(1, float('nan')))),
      ('bounds is NULL', dict(q=q4, bounds=None)),
      ('unknown dtype', dict(q=q4, dtype_code=7)),
      ('flags other than MASKED', dict(q=q4, flags=_hip.FLAG_FAIR)),
      ('flags other than MASKED', dict(q=q4, flags=_hip.FLAG_SKIPNA_ENS)),
      ('mask is NULL', dict(q=q4, flags=_hip.FLAG_MASKED, with_mask=False)),
      ('no plane mode', dict(q=q4, plan_edit={'plane_rows': 1})),
      ('p/t is NULL', dict(q=q4, with_t=False)),
  ]
  for message, kw in cases:
    rc, _, got = _launch(ctx, p, t, mask, kw.pop('q'), False, 5, kw.pop('flags', 0), sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message
  # folded x weights
  rc, _, got = _launch(ctx, p, t, mask, q4, False, 5, 0, sentinel=SENTINEL, plan_edit={'x_weights': np.ones(65)})
  assert rc == -1 and (got == SENTINEL).all()
  with pytest.raises(_hip.WbxError, match='no folded x weights'):
    _hip.check(rc, 'x weights')
  # sixteen quantiles, sixty-four members and one member are fine
  want, tol = QC.expected(p, t, q, mask, 0, 5, False)
  rc, _, got = _launch(ctx, p, t, mask, q, False, 5, 0, sentinel=SENTINEL)
  _hip.check(rc, '16 quantiles')
  _check(got, want, tol, '16 quantiles')
  for m in (1, 64):
    pm, tm, _ = QC.case(m, m, NLEAD, 5, 65, np.float32, 0)
    qm = QC.levels(16, m)
    want, tol = QC.expected(pm, tm, qm, mask, 0, 5, False)
    rc, _, got = _launch(ctx, pm, tm, mask, qm, False, 5, 0, sentinel=SENTINEL)
    _hip.check(rc, f'M = {m}')
    _check(got, want, tol, f'M = {m}')


@pytest.mark.parametrize('mode', list(MODES))
def test_empty_extents(ctx, mode):
  q = QC.levels(3, 3)
  p, t, mask = QC.case(4, 3, NLEAD, 5, 65, np.float32, 0)
  for x_kept in (False, True):
    rc, _, got = _launch(ctx, p, t, mask, q, x_kept, 5, MODES[mode], sentinel=SENTINEL, plan_edit={'ndepth': 0})
    _hip.check(rc, 'ndepth == 0')
    assert (got == 0.0).all() and not np.signbit(got).any()
    rc, _, got = _launch(ctx, p, t, mask, q, x_kept, 5, MODES[mode], sentinel=SENTINEL, plan_edit={'nkey': 0})
    _hip.check(rc, 'nkey == 0')
    assert (got == SENTINEL).all()
  rc, _, got = _launch(ctx, p, t, mask, q, False, 5, MODES[mode], sentinel=SENTINEL, plan_edit={'nx': 0})
  _hip.check(rc, 'nx == 0')
  assert (got == 0.0).all()
