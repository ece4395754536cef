"""wbx_ens_variogram_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the float64 restatement
(tests/variogram_cases.py), within the bound derived there from the kernel's arithmetic; NaN at the same places; count lanes bit
for bit.

Frame (lead = 2, row = 5, x); p[M, lead, row, x, l], t[lead, row, x, l].  (M, L) in (1, 1), (2, 2), (3, 9), (5, 17), (51, 9),
(64, 64): no pairs, one pair, the 3 x 3 window, several tiles per row, the member chunk (51 members are staged 12 at a time at
L = 9), the largest run (one point per tile, every item of a block in use).  Row lengths per L: 1, a row that ends in the middle of
a tile, one tile and one point (P + 1, P = variogram_cases.tile_points(L)), and a row of several tiles.  A test is one (mode, dtype,
(M, L)); its 8 launches walk the row lengths with x kept and summed while the power, the chunking (all 5 rows, or 2 with a ragged
last chunk) and the 8 storage orders rotate so that every value of each occurs in every test.  Blocks of 256 threads throughout
(8 items per thread), 64 and 128 (32 items per thread, another instantiation) in a test of their own."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import variogram_cases as VC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked+skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
MEMBER, LEAD, ROW, X, RUN = 'number', 'lead_time', 'row', 'x', 'window'
SDIMS = (LEAD, ROW, X)
NLEAD, NROW = 2, 5
SENTINEL = -77.0
SHAPES = ((1, 1), (2, 2), (3, 9), (5, 17), (51, 9), (64, 64))
POWERS = (0.5, 1.0, 2.0)
ARRANGEMENTS = [(m, n) for m in VC.MEMBER_AXES for n in VC.RUN_AXES]


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def _root(a):
  """The contiguous array `a` is a (transposed, possibly reversed) view of, and the byte offset of `a`'s first element in it."""
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


def _launch(ctx, p, t, mask, x_kept, depth_chunk, flags, power, threads=256, m=None, run_len=None, dtype_code=None, with_mask=True,
            sentinel=None, ndepth0=False, plane_rows=0, repeat=1, x_weights=False, nkey0=False, null_inputs=False):
  """-> (rc, plan, [partial[lead][chunk][lane][j] per repetition]) on p[M, lead, row, x, l], t[lead, row, x, l] (any strides),
  mask[row, x]."""
  nlead, nrow, nx, nl = t.shape
  sizes = {LEAD: nlead, ROW: nrow, X: nx}
  lay_m = mask_buf = None
  if flags & _hip.FLAG_MASKED:
    lay_m = planner.InputLayout(strides={ROW: nx, X: 1}, itemsize=1, base_alignment=256)  # zero stride along lead
    mask_buf = ctx.upload(np.ascontiguousarray(mask, np.uint8)) if with_mask else None
  reduce_dims = (ROW,) if x_kept else (ROW, X)
  lay_p, lay_t = _layout(p, (MEMBER,) + SDIMS + (RUN,)), _layout(t, SDIMS + (RUN,))
  plan = planner.build_s1_plan(SDIMS, sizes, [lay_p, lay_t, None, lay_m], reduce_dims, wdep_dims=set(),
                               flags=flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA), allow_vec4=False, force_x_dim=X)
  dc = min(depth_chunk, plan.ndepth)
  plan = dataclasses.replace(plan, depth_chunk=dc, nchunk=-(-plan.ndepth // dc), flags=flags, block_threads=threads, plane_rows=plane_rows)
  assert plan.x_kept == x_kept and plan.a_dims == (LEAD,) and plan.depth_dims == (ROW,) and not plan.bk_dims and not plan.br_dims, plan
  nacc = 2 if flags & (_hip.FLAG_SKIPNA | _hip.FLAG_MASKED) else 1
  shape = (nlead, plan.nchunk, nacc, plan.nj)
  if ndepth0:
    plan = dataclasses.replace(plan, ndepth=0)
  if nkey0:
    plan = dataclasses.replace(plan, nkey=0)
  if x_weights:
    plan = dataclasses.replace(plan, x_weights=np.ones(nx))
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  n = int(np.prod(shape))
  (rp, op), (rt, ot) = _root(p), _root(t)
  bufs = ctx.upload(rp), ctx.upload(rt)
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  outs, rc = [], 0
  for _ in range(repeat):
    out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
    rc = ctx.lib.wbx_ens_variogram_partial(
        ctx.handle, C.byref(dplan.struct), dtype_code, p.shape[0] if m is None else m, lay_p.stride(MEMBER), nl if run_len is None else run_len,
        lay_p.stride(RUN), lay_t.stride(RUN), VC.POWERS[power] if power in VC.POWERS else power,
        None if null_inputs else _ptr(bufs[0], op), None if null_inputs else _ptr(bufs[1], ot), _ptr(mask_buf), _ptr(out))
    outs.append(ctx.download(out.ptr, shape, np.float64))
  return rc, plan, outs


def _widths(l):
  tile = VC.tile_points(l)
  mid = tile // 2 + 2 if tile > 3 else 2
  return [1, mid, tile + 1, 2 * tile + mid], tile


def test_the_tile_sizes_and_member_chunks_the_cases_are_built_around():
  """Points per tile and members per chunk: what 2048 items, 512 target elements and 6144 staged elements hold
  (csrc/wbx_ens_variogram.hip); the bindings' copies agree."""
  assert [VC.tile_points(l) for _, l in SHAPES] == [64, 64, 56, 15, 56, 1]
  assert [VC.member_chunk(m, l) for m, l in SHAPES] == [1, 2, 3, 5, 12, 64]  # (51, 9) crosses the member chunk
  assert VC.member_chunk(64, 33) == 62 and VC.tile_points(33) == 3
  for l in range(1, VC.MAX_RUN + 1):
    assert VC.tile_points(l) == _hip.vgram_tile_points(l)
    for m in (1, 13, 51, 64):
      assert VC.member_chunk(m, l) == _hip.vgram_member_chunk(m, l)


@pytest.mark.parametrize('shape', SHAPES, ids=[f'M{m}-L{l}' for m, l in SHAPES])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_within_its_bound(ctx, mode, dtype, shape):
  flags = MODES[mode]
  m, nl = shape
  widths, tile = _widths(nl)
  seen = {'p': set(), 'dc': set(), 'arr': set(), 'kept': set()}
  worst = 0.0
  for i in range(2 * len(widths)):
    nx, x_kept = widths[i // 2], bool(i % 2)
    power = POWERS[(i + i // 3 + m) % 3]
    depth_chunk = (NROW, 2)[(i + i // 4) % 2]
    member, run = ARRANGEMENTS[(5 * i + m) % len(ARRANGEMENTS)]
    what = f'M={m} L={nl} nx={nx} (tile {tile}) dc={depth_chunk} x_kept={x_kept} {mode} {np.dtype(dtype).name} p={power} member={member} run={run}'
    p0, t0, mask, want, bound, _ = VC.variogram_case(1000 * m + 10 * nl + i, m, nl, NLEAD, NROW, nx, dtype, flags, depth_chunk, x_kept, power)
    p, t = VC.arrange(p0, t0, member, run)
    rc, _, (got,) = _launch(ctx, p, t, mask, x_kept, depth_chunk, flags, power)
    _hip.check(rc, what)
    err = VC.check(got, want, bound, what)
    fin = np.isfinite(want) & (bound > 0)
    print(f'{what}: largest error {err:.3e}, largest error / bound {float((np.abs(got - want)[fin] / bound[fin]).max()) if fin.any() else 0.0:.3f}')
    worst = max(worst, err)
    for key, value in (('p', power), ('dc', depth_chunk), ('arr', (member, run)), ('kept', x_kept)):
      seen[key].add(value)
  assert seen['p'] == set(POWERS) and seen['dc'] == {NROW, 2} and seen['kept'] == {True, False} and seen['arr'] == set(ARRANGEMENTS)


@pytest.mark.parametrize('threads', [64, 128])
def test_smaller_blocks_take_more_items_per_thread(ctx, threads):
  for (m, nl), power in zip(((3, 9), (51, 9), (64, 64), (5, 17)), (0.5, 1.0, 2.0, 0.5)):
    widths, tile = _widths(nl)
    for nx, x_kept in ((widths[2], False), (widths[3], True)):
      p0, t0, mask, want, bound, _ = VC.variogram_case(m + nx, m, nl, NLEAD, NROW, nx, np.float32, 0, 2, x_kept, power)
      rc, _, (got,) = _launch(ctx, p0, t0, mask, x_kept, 2, 0, power, threads=threads)
      _hip.check(rc, f'threads={threads}')
      VC.check(got, want, bound, f'threads={threads} M={m} L={nl} nx={nx} (tile {tile}) x_kept={x_kept}')


def test_rows_longer_than_a_block_of_x(ctx):
  """x kept: a block covers 256 positions in tiles; 257 positions need a second block with a one-point tile."""
  p0, t0, mask, want, bound, _ = VC.variogram_case(3, 4, 3, NLEAD, NROW, 257, np.float32, _hip.FLAG_MASKED, 2, True, 0.5)
  rc, _, (got,) = _launch(ctx, p0, t0, mask, True, 2, _hip.FLAG_MASKED, 0.5)
  _hip.check(rc, 'nx = 257')
  VC.check(got, want, bound, 'nx = 257')


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_a_negative_run_stride_walks_down(ctx, dtype):
  """The predictions' run stored backwards (stride -1, the pointer at the run's last stored element), the targets' forwards."""
  for m, nl, nx, power in ((3, 9, 57, 0.5), (51, 9, 7, 1.0), (5, 17, 16, 2.0)):
    for x_kept in (False, True):
      p0, t0, mask, _, _, _ = VC.variogram_case(50 + m, m, nl, NLEAD, NROW, nx, dtype, 0, NROW, x_kept, power)
      p = p0[..., ::-1]
      assert p.strides[-1] == -p.itemsize
      want, bound, _ = VC.expected(np.ascontiguousarray(p), t0, power, mask, 0, NROW, x_kept)
      assert np.isfinite(want).mean() >= 0.8
      rc, _, (got,) = _launch(ctx, p, t0, mask, x_kept, NROW, 0, power)
      _hip.check(rc, 'negative stride')
      VC.check(got, want, bound, f'negative run stride M={m} L={nl} nx={nx} x_kept={x_kept}')


@pytest.mark.parametrize('power', POWERS)
def test_every_non_finite_kind_gives_nan_and_nothing_else_does(ctx, power):
  """One point per kind, x kept and every row its own chunk, so that each point is its own partial."""
  rng = np.random.default_rng(8)
  for m, nl, dtype in ((3, 9, np.float32), (51, 9, np.float64), (2, 1, np.float32), (4, 64, np.float32)):
    p = (rng.integers(-64, 65, size=(m, 1, NROW, 6, nl)) / 8.0).astype(dtype)
    t = (rng.integers(-64, 65, size=(1, NROW, 6, nl)) / 8.0).astype(dtype)
    e = nl - 1
    p[m - 1, 0, 0, 1, e] = np.inf
    p[0, 0, 1, 2, e] = p[m - 1, 0, 1, 2, e] = np.inf
    p[0, 0, 2, 3, 0] = np.nan
    t[0, 3, 4, e] = np.nan
    p[0, 0, 4, 5, 0] = -np.inf
    t[0, 4, 0, 0] = np.inf
    bad = np.zeros((NROW, 6), bool)
    bad[[0, 1, 2, 3, 4, 4], [1, 2, 3, 4, 5, 0]] = True
    rc, _, (got,) = _launch(ctx, p, t, None, True, 1, 0, power)
    _hip.check(rc, 'non-finite kinds')
    np.testing.assert_array_equal(np.isnan(got[0, :, 0, :]), bad)
    assert np.isfinite(got[0, :, 0, :][~bad]).all()


def test_equal_members_score_exactly_zero(ctx):
  """Every member equal to the target (finite values): every partial is exactly +0 where M equal terms add up to M times the term
  without a rounding -- float32 terms in the float64 member sum, and |d| on a dyadic grid in float64."""
  rng = np.random.default_rng(5)
  for (m, nl, dtype), power in zip(((51, 9, np.float32), (4, 17, np.float64), (64, 3, np.float32)), POWERS):
    t = (280.0 + rng.integers(0, 1024, size=(NLEAD, NROW, 17, nl)) * 2.0 ** -10).astype(dtype)
    p = np.broadcast_to(t[None], (m,) + t.shape).copy()
    for x_kept in (False, True):
      rc, _, (got,) = _launch(ctx, p, t, None, x_kept, 2, 0, power)
      _hip.check(rc, 'equal members')
      assert (got == 0.0).all() and not np.signbit(got).any(), (m, nl, x_kept)


def test_two_launches_of_one_case_are_bit_equal(ctx):
  for m, nl, nx, x_kept, flags, power in ((51, 9, 113, False, 0, 0.5), (64, 64, 3, True, _hip.FLAG_SKIPNA, 2.0), (5, 17, 37, False, _hip.FLAG_MASKED, 1.0)):
    p0, t0, mask, _, _, _ = VC.variogram_case(77 + m, m, nl, NLEAD, NROW, nx, np.float32, flags, NROW, x_kept, power)
    p, t = VC.arrange(p0, t0, 'outer', 'middle')
    rc, _, (a, b) = _launch(ctx, p, t, mask, x_kept, NROW, flags, power, repeat=2)
    _hip.check(rc, 'repeat')
    assert a.tobytes() == b.tobytes(), (m, nl, nx)


def test_refusals_leave_the_output_untouched(ctx):
  p, t, mask, _, _, _ = VC.variogram_case(9, 3, 5, NLEAD, NROW, 9, np.float32, 0, NROW, False, 0.5)
  cases = [
      ('members', dict(m=0)),
      ('members', dict(m=_hip.VGRAM_MAX_MEMBERS + 1)),
      ('a run of 1', dict(run_len=0)),
      ('a run of 1', dict(run_len=_hip.VGRAM_MAX_RUN + 1)),
      ('unknown power code', dict(power=3)),
      ('unknown power code', dict(power=-1)),
      ('unknown dtype', dict(dtype_code=7)),
      ('mask is NULL', dict(flags=_hip.FLAG_MASKED, with_mask=False)),
      ('flags other than MASKED', dict(flags=_hip.FLAG_FAIR)),
      ('flags other than MASKED', dict(flags=_hip.FLAG_SKIPNA_ENS)),
      ('no plane mode', dict(plane_rows=5)),
      ('no folded x weights', dict(x_weights=True)),
      ('p/t is NULL', dict(null_inputs=True)),
  ]
  for message, kw in cases:
    kw = dict(kw)
    flags, power = kw.pop('flags', 0), kw.pop('power', 0.5)
    rc, _, (got,) = _launch(ctx, p, t, mask, False, NROW, flags, power, sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message


@pytest.mark.parametrize('mode', list(MODES))
def test_no_rows_zero_the_partial(ctx, mode):
  p, t, mask, _, _, _ = VC.variogram_case(4, 3, 5, NLEAD, NROW, 9, np.float32, 0, NROW, False, 1.0)
  for x_kept in (False, True):
    rc, _, (got,) = _launch(ctx, p, t, mask, x_kept, NROW, MODES[mode], 1.0, sentinel=SENTINEL, ndepth0=True)
    _hip.check(rc, 'ndepth == 0')
    assert (got == 0.0).all() and not np.signbit(got).any()


def test_no_keys_touch_nothing(ctx):
  p, t, mask, _, _, _ = VC.variogram_case(4, 3, 5, NLEAD, NROW, 9, np.float32, 0, NROW, False, 1.0)
  rc, _, (got,) = _launch(ctx, p, t, mask, False, NROW, 0, 1.0, sentinel=SENTINEL, nkey0=True, null_inputs=True)
  _hip.check(rc, 'nkey == 0')
  assert (got == SENTINEL).all()
