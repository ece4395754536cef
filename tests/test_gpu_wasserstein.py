"""wbx_ens_wasserstein_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the float64 restatement
(tests/wasserstein_cases.py), within the bound derived there from the kernel's arithmetic; with every dim kept bit for bit against
the exact evaluation; NaN and +inf at the same places; count lanes bit for bit.

Frame (lead = 2, row = 3..5, x); p[M, lead, row, x], t[N, lead, row, x].  (M, N): one member a side, one against the largest, the
smallest walk with three pieces, sizes at and one past a network size on either side (4, 8, 16, 32, 50, 51, 64), M > N and M < N,
a common divisor (6, 4), both at the largest.  Row lengths 1, 63, 70 and 130: a partial wave, a wave and a part, a block of 128 and
two more points.  A test is one (mode, dtype, (M, N)); its 4 launches walk the row lengths while x kept / summed, the chunking (all
rows, or 2 with a ragged last chunk), the block size and the 9 storage orders rotate."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import wasserstein_cases as WC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA}
MEMBER, LEAD, ROW, X = 'number', 'lead_time', 'row', 'x'
SDIMS = (LEAD, ROW, X)
NLEAD = 2
SENTINEL = -77.0
PAIRS = ((1, 1), (1, 64), (64, 1), (2, 3), (3, 4), (4, 5), (7, 5), (8, 8), (6, 4), (16, 17), (33, 32), (50, 51), (51, 51), (51, 10),
         (64, 63), (64, 64))
WIDTHS = (1, 63, 70, 130)
ARRANGEMENTS = [(a, b) for a in WC.MEMBER_AXES for b in WC.MEMBER_AXES]


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def _root(a):
  """The contiguous array `a` is a (transposed) view of, and the byte offset of `a`'s first element in it."""
  r = a
  while r.base is not None:
    r = r.base
  assert r.flags.c_contiguous
  return r, a.__array_interface__['data'][0] - r.__array_interface__['data'][0]


def _layout(a, dims):
  lay = planner.layout_of(a, dims)
  return planner.InputLayout(strides=dict(lay.strides), itemsize=lay.itemsize, base_alignment=lay.itemsize)


def _ptr(buf, offset=0):
  return None if buf is None else C.c_void_p(buf.ptr + offset)


def _launch(ctx, p, t, mask, x_kept, depth_chunk, flags, threads=256, m=None, n=None, dtype_code=None, with_mask=True, sentinel=None,
            ndepth0=False, nx0=False, plane_rows=0, repeat=1, x_weights=False, nkey0=False, null_inputs=False, vec=1):
  """-> (rc, plan, [partial[lead][chunk][lane][j] per repetition]) on p[M, lead, row, x], t[N, lead, row, x] (any strides),
  mask[row, x]."""
  _, nlead, nrow, nx = t.shape
  sizes = {LEAD: nlead, ROW: nrow, X: nx}
  lay_m = mask_buf = None
  if flags & _hip.FLAG_MASKED:
    lay_m = planner.InputLayout(strides={ROW: nx, X: 1}, itemsize=1, base_alignment=256)  # zero stride along lead
    mask_buf = ctx.upload(np.ascontiguousarray(mask, np.uint8)) if with_mask else None
  reduce_dims = (ROW,) if x_kept else (ROW, X)
  lay_p, lay_t = _layout(p, (MEMBER,) + SDIMS), _layout(t, (MEMBER,) + SDIMS)
  plan = planner.build_s1_plan(SDIMS, sizes, [lay_p, lay_t, None, lay_m], reduce_dims, wdep_dims=set(),
                               flags=flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA), allow_vec4=False, force_x_dim=X)
  dc = min(depth_chunk, plan.ndepth)
  plan = dataclasses.replace(plan, depth_chunk=dc, nchunk=-(-plan.ndepth // dc), flags=flags, block_threads=threads, plane_rows=plane_rows,
                             vec=vec)
  assert plan.x_kept == x_kept and plan.a_dims == (LEAD,) and plan.depth_dims == (ROW,) and not plan.bk_dims and not plan.br_dims, plan
  nacc = 2 if flags & (_hip.FLAG_SKIPNA | _hip.FLAG_MASKED) else 1
  shape = (nlead, plan.nchunk, nacc, plan.nj)
  if ndepth0:
    plan = dataclasses.replace(plan, ndepth=0)
  if nx0:
    plan = dataclasses.replace(plan, nx=0)
  if nkey0:
    plan = dataclasses.replace(plan, nkey=0)
  if x_weights:
    plan = dataclasses.replace(plan, x_weights=np.ones(nx))
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  size = int(np.prod(shape))
  (rp, op), (rt, ot) = _root(p), _root(t)
  bufs = ctx.upload(rp), ctx.upload(rt)
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  outs, rc = [], 0
  for _ in range(repeat):
    out = ctx.upload(np.full(size, sentinel, np.float64)) if sentinel is not None else ctx.alloc(size * 8)
    rc = ctx.lib.wbx_ens_wasserstein_partial(
        ctx.handle, C.byref(dplan.struct), dtype_code, p.shape[0] if m is None else m, lay_p.stride(MEMBER),
        t.shape[0] if n is None else n, lay_t.stride(MEMBER), None if null_inputs else _ptr(bufs[0], op),
        None if null_inputs else _ptr(bufs[1], ot), _ptr(mask_buf), _ptr(out))
    outs.append(ctx.download(out.ptr, shape, np.float64))
  return rc, plan, outs


@pytest.mark.parametrize('pair', PAIRS, ids=[f'M{m}-N{n}' for m, n in PAIRS])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_within_its_bound(ctx, mode, dtype, pair):
  flags = MODES[mode]
  m, n = pair
  k0 = PAIRS.index(pair)
  seen = {'dc': set(), 'kept': set()}
  for i, nx in enumerate(WIDTHS):
    nrow = 3 + (i + k0) % 3
    x_kept = bool((i + k0) % 2)
    depth_chunk = (nrow, 2)[(i + i // 2 + k0) % 2]
    pa, ta = ARRANGEMENTS[(4 * i + k0) % len(ARRANGEMENTS)]
    threads = (256, 128, 64)[(i + k0) % 3]
    what = f'M={m} N={n} nrow={nrow} nx={nx} dc={depth_chunk} x_kept={x_kept} {mode} {np.dtype(dtype).name} p={pa} t={ta} threads={threads}'
    p0, t0, mask, want, bound, _ = WC.wasserstein_case(1000 * m + 10 * n + i, m, n, NLEAD, nrow, nx, dtype, flags, depth_chunk, x_kept)
    rc, _, (got,) = _launch(ctx, WC.arrange(p0, pa), WC.arrange(t0, ta), mask, x_kept, depth_chunk, flags, threads=threads)
    _hip.check(rc, what)
    err = WC.check(got, want, bound, what)
    nl = WC.NLANE
    np.testing.assert_array_equal(got[:, :, nl:], want[:, :, nl:], err_msg=f'{what}: count lanes')
    fin = np.isfinite(want) & (bound > 0)
    print(f'{what}: largest error {err:.3e}, largest error / bound {float((np.abs(got - want)[fin] / bound[fin]).max()) if fin.any() else 0.0:.3f}')
    seen['dc'].add(depth_chunk == nrow)
    seen['kept'].add(x_kept)
  assert seen['dc'] == {True, False} and seen['kept'] == {True, False}


def test_the_rotation_reaches_every_storage_order_and_block_size():
  hit = {ARRANGEMENTS[(4 * i + k0) % len(ARRANGEMENTS)] for k0 in range(len(PAIRS)) for i in range(len(WIDTHS))}
  assert hit == set(ARRANGEMENTS)
  assert {(256, 128, 64)[(i + k0) % 3] for k0 in range(len(PAIRS)) for i in range(len(WIDTHS))} == {256, 128, 64}


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_every_dim_kept_is_the_exact_value_bit_for_bit(ctx, dtype):
  """x kept and every row its own chunk: a partial is one point.  The value classes are all on dyadic grids, so the kernel's sum is
  exact and its value is float(S) / float(M N); NaN-making points are NaN, single infinities +inf, and nothing else is either."""
  for k, (m, n) in enumerate(PAIRS):
    nx = (65, 5, 9)[k % 3]
    rng = np.random.default_rng(k)
    p, t = WC.values(300 + k, m, n, (NLEAD, 3, nx), dtype)
    exact = WC.exact_points(p, t)
    spots = rng.choice(exact.size, size=min(9, exact.size), replace=False)
    for q, kind in zip(spots, WC.NAN_KINDS + WC.INF_KINDS):
      at = tuple(int(v) for v in np.unravel_index(q, exact.shape))
      WC.put(p, t, rng, at, kind)
    stat, _ = WC.wasserstein_points(p, t)
    nan_at, inf_at = np.isnan(stat), np.isinf(stat)
    assert nan_at.sum() >= 4 and (inf_at.sum() >= 3 or exact.size < 9) and (stat[inf_at] == np.inf).all()
    pa, ta = ARRANGEMENTS[k % len(ARRANGEMENTS)]
    rc, _, (got,) = _launch(ctx, WC.arrange(p, pa), WC.arrange(t, ta), None, True, 1, 0, threads=(64, 128, 256)[k % 3])
    _hip.check(rc, 'every dim kept')
    got = got[:, :, 0, :]
    np.testing.assert_array_equal(np.isnan(got), nan_at, err_msg=f'M={m} N={n}: NaN positions')
    np.testing.assert_array_equal(got == np.inf, inf_at, err_msg=f'M={m} N={n}: +inf positions')
    fin = ~(nan_at | inf_at)
    assert got[fin].tobytes() == exact[fin].tobytes(), (m, n, float(np.abs(got[fin] - exact[fin]).max()))
    assert not np.signbit(got[fin]).any()


def test_equal_members_are_exactly_zero(ctx):
  rng = np.random.default_rng(5)
  for m, n, dtype in ((51, 10, np.float32), (4, 17, np.float64), (64, 64, np.float32)):
    v = (280.0 + rng.integers(0, 1024, size=(NLEAD, 4, 17)) * 2.0 ** -10).astype(dtype)
    p, t = np.broadcast_to(v[None], (m,) + v.shape).copy(), np.broadcast_to(v[None], (n,) + v.shape).copy()
    for x_kept in (False, True):
      rc, _, (got,) = _launch(ctx, p, t, None, x_kept, 3, 0)
      _hip.check(rc, 'equal members')
      assert (got == 0.0).all() and not np.signbit(got).any(), (m, n, x_kept)


def test_two_launches_of_one_case_are_bit_equal(ctx):
  for m, n, nx, x_kept, flags, dtype in ((51, 51, 130, False, 0, np.float32), (64, 63, 70, True, _hip.FLAG_SKIPNA, np.float64),
                                         (7, 5, 63, False, _hip.FLAG_MASKED, np.float32)):
    p0, t0, mask, _, _, _ = WC.wasserstein_case(77 + m, m, n, NLEAD, 5, nx, dtype, flags, 2, x_kept)
    rc, _, (a, b) = _launch(ctx, WC.arrange(p0, 'middle'), WC.arrange(t0, 'inner'), mask, x_kept, 2, flags, repeat=2)
    _hip.check(rc, 'repeat')
    assert a.tobytes() == b.tobytes(), (m, n, nx)


def test_vec_4_is_accepted_and_ignored(ctx):
  p0, t0, mask, want, bound, _ = WC.wasserstein_case(12, 7, 5, NLEAD, 4, 8, np.float32, 0, 4, False)
  rc, _, (got,) = _launch(ctx, p0, t0, mask, False, 4, 0, vec=4)
  _hip.check(rc, 'vec = 4')
  WC.check(got, want, bound, 'vec = 4')


def test_refusals_leave_the_output_untouched(ctx):
  p, t, mask, _, _, _ = WC.wasserstein_case(9, 3, 5, NLEAD, 4, 9, np.float32, 0, 4, False)
  cases = [
      ('members a side', dict(m=0)),
      ('members a side', dict(m=_hip.WASS_MAX_MEMBERS + 1)),
      ('members a side', dict(n=0)),
      ('members a side', dict(n=_hip.WASS_MAX_MEMBERS + 1)),
      ('unknown dtype', dict(dtype_code=7)),
      ('mask is NULL', dict(flags=_hip.FLAG_MASKED, with_mask=False)),
      ('flags other than MASKED', dict(flags=_hip.FLAG_FAIR)),
      ('flags other than MASKED', dict(flags=_hip.FLAG_SKIPNA_ENS)),
      ('no plane mode', dict(plane_rows=4)),
      ('no folded x weights', dict(x_weights=True)),
      ('p/t is NULL', dict(null_inputs=True)),
  ]
  for message, kw in cases:
    kw = dict(kw)
    flags = kw.pop('flags', 0)
    rc, _, (got,) = _launch(ctx, p, t, mask, False, 4, flags, sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message


@pytest.mark.parametrize('mode', list(MODES))
def test_no_rows_or_no_x_zero_the_partial(ctx, mode):
  p, t, mask, _, _, _ = WC.wasserstein_case(4, 3, 5, NLEAD, 4, 9, np.float32, 0, 4, False)
  for x_kept in (False, True):
    rc, _, (got,) = _launch(ctx, p, t, mask, x_kept, 4, MODES[mode], sentinel=SENTINEL, ndepth0=True)
    _hip.check(rc, 'ndepth == 0')
    assert (got == 0.0).all() and not np.signbit(got).any()
  rc, _, (got,) = _launch(ctx, p, t, mask, False, 4, MODES[mode], sentinel=SENTINEL, nx0=True)
  _hip.check(rc, 'nx == 0')
  assert (got == 0.0).all() and not np.signbit(got).any()


def test_no_keys_touch_nothing(ctx):
  p, t, mask, _, _, _ = WC.wasserstein_case(4, 3, 5, NLEAD, 4, 9, np.float32, 0, 4, False)
  rc, _, (got,) = _launch(ctx, p, t, mask, False, 4, 0, sentinel=SENTINEL, nkey0=True, null_inputs=True)
  _hip.check(rc, 'nkey == 0')
  assert (got == SENTINEL).all()
