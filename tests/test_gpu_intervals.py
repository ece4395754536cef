"""wbx_ens_interval_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the float64 restatement
(tests/interval_cases.py) bit for bit -- the restatement performs the header's float64 operations one by one, and a partial is a sum
of zeros and ones -- and every partial an integer.

Frame (key = 1..2, row = 1..3, x); p[M, key, row, x], t[key, row, x], c[level, key, row, x] with the seven levels of
interval_cases.LEVELS.  M walks every network size and one past it; the row lengths 1, 63, 64, 65, 129 and 200 a partial wave, a
wave and its neighbours, a block of 128 and a point, and several blocks.  A test is one (mode, dtype, M); its 6 launches walk the
row lengths while x kept / summed, keys, rows, the chunking, the block size, the member axis, the climatology's zero strides, the
lane subset and the level pairs rotate."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import interval_cases as IC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA}
MEMBER, LEVEL, KEY, ROW, X = 'number', 'quantile', 'key', 'row', 'x'
SDIMS = (KEY, ROW, X)
SENTINEL = -77.0
MEMBERS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 50, 51, 52, 64)
WIDTHS = (1, 63, 64, 65, 129, 200)
SUBSETS = (7, 1, 2, 4, 3, 5, 6)  # every lane subset
PAIRS = ((0.1, 0.9), (0.0, 1.0), (0.5, 0.5), (0.2, 0.7))  # g on both sides of 0.5 for most M, 0 for M = 11, 51 and at the ends
C_MODES = ('full', 'no_row', 'no_key')  # the climatology varies along every dim / has zero stride along the rows / along the keys


def params_for(pairs, thresholds=(0.7, 0.75)):
  """{bit: (levels, threshold)}: one level pair per lane."""
  return {IC.COVERED: (pairs[0], None), IC.CONFIDENT: (pairs[1], thresholds[0]), IC.JACCARD: (pairs[2], thresholds[1])}


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def _root(a):
  """The contiguous array `a` is a (transposed, broadcast) view of, and the byte offset of `a`'s first element in it."""
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


def lane_structs(m, lanes, params, level_stride, tweak=None):
  """The three wbx_ivl_lane of a launch from {bit: (levels, threshold)}; `tweak(struct array)` edits them (refusals)."""
  arr = (_hip.IvlLaneStruct * 3)()
  for slot, bit in enumerate(IC.BITS):
    if not lanes & bit:
      continue
    levels, thr = params[bit]
    for b, q in zip((arr[slot].lo, arr[slot].hi), levels):
      b.k, b.g = IC.bound(q, m)
      b.c_off = IC.LEVELS.index(q) * level_stride if bit != IC.COVERED else 0
    arr[slot].threshold = 0.0 if thr is None else thr
  if tweak is not None:
    tweak(arr)
  return arr


def _launch(ctx, p, t, c, mask, lanes, params, x_kept, depth_chunk, flags, threads=256, m=None, dtype_code=None, with_mask=True,
            sentinel=None, ndepth0=False, nx0=False, nkey0=False, plane_rows=0, repeat=1, x_weights=False, null=(), vec=1, tweak=None,
            keep_out=False):
  """-> (rc, plan, [partial[key][chunk][lane][j] per repetition]) on p[M, key, row, x], t[key, row, x], c[level, key, row, x] (any
  strides, c may be None), mask[row, x]."""
  nkey, nrow, nx = t.shape
  sizes = {KEY: nkey, ROW: nrow, X: nx}
  lay_m = mask_buf = None
  if flags & _hip.FLAG_MASKED:
    lay_m = planner.InputLayout(strides={ROW: nx, X: 1}, itemsize=1, base_alignment=256)  # zero stride along the keys
    mask_buf = ctx.upload(np.ascontiguousarray(mask, np.uint8)) if with_mask else None
  reduce_dims = (ROW,) if x_kept else (ROW, X)
  lay_p, lay_t = _layout(p, (MEMBER,) + SDIMS), _layout(t, SDIMS)
  lay_c = _layout(c, (LEVEL,) + SDIMS) if c is not None else None
  plan = planner.build_s1_plan(SDIMS, sizes, [lay_p, lay_t, lay_c, lay_m], reduce_dims, wdep_dims=set(),
                               flags=flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA), allow_vec4=False, force_x_dim=X)
  dc = min(depth_chunk, plan.ndepth)
  plan = dataclasses.replace(plan, depth_chunk=dc, nchunk=-(-plan.ndepth // dc), flags=flags, block_threads=threads, plane_rows=plane_rows,
                             vec=vec)
  assert plan.x_kept == x_kept and plan.a_dims == (KEY,) and plan.depth_dims == (ROW,) and not plan.bk_dims and not plan.br_dims, plan
  nval = bin(lanes & 7).count('1') or 1
  nacc = 2 * nval if flags & _hip.FLAG_SKIPNA else (nval + 1 if flags & _hip.FLAG_MASKED else nval)
  shape = (nkey, plan.nchunk, nacc, plan.nj)
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
  bufs = [ctx.upload(rp), ctx.upload(rt), None]
  oc = 0
  if c is not None:
    rc_, oc = _root(c)
    bufs[2] = ctx.upload(rc_)
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  m = p.shape[0] if m is None else m
  structs = lane_structs(min(max(m, 1), 64), lanes & 7, params, lay_c.stride(LEVEL) if lay_c is not None else 0, tweak)
  outs, rc, out = [], 0, None
  for _ in range(repeat):
    out = ctx.upload(np.full(size, sentinel, np.float64)) if sentinel is not None else ctx.alloc(size * 8)
    rc = ctx.lib.wbx_ens_interval_partial(
        ctx.handle, C.byref(dplan.struct), dtype_code, m, lay_p.stride(MEMBER), lanes, structs,
        None if 'p' in null else _ptr(bufs[0], op), None if 't' in null else _ptr(bufs[1], ot),
        None if 'c' in null else _ptr(bufs[2], oc), _ptr(mask_buf), _ptr(out))
    outs.append(ctx.download(out.ptr, shape, np.float64))
  if keep_out:
    return rc, plan, outs, out
  return rc, plan, outs


def _c_mode(c, mode):
  if mode == 'no_row':
    return np.broadcast_to(np.ascontiguousarray(c[:, :, :1]), c.shape)
  if mode == 'no_key':
    return np.broadcast_to(np.ascontiguousarray(c[:, :1]), c.shape)
  return c


def _rotation(i, k0):
  """The launch's settings besides M and the row length."""
  return dict(nkey=1 + (i + k0) % 2, nrow=(1, 3)[(i // 2 + k0) % 2], x_kept=bool((i + k0 // 2) % 2), two_chunks=bool((i + k0) % 3 == 0),
              where=IC.MEMBER_AXES[(i + k0 // 3) % 2], c_mode=C_MODES[(i + k0) % 3], lanes=SUBSETS[(i + 2 * k0) % len(SUBSETS)],
              pairs=tuple(PAIRS[(i + k0 + j) % len(PAIRS)] for j in range(3)), threads=(256, 128, 64)[(i + k0) % 3])


@pytest.mark.parametrize('m', MEMBERS, ids=[f'M{m}' for m in MEMBERS])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_bit_for_bit(ctx, mode, dtype, m):
  flags = MODES[mode]
  k0 = MEMBERS.index(m) + 5 * list(MODES).index(mode)
  for i, nx in enumerate(WIDTHS):
    r = _rotation(i, k0)
    depth_chunk = 2 if r['two_chunks'] else r['nrow']
    params = params_for(r['pairs'])
    p0, t0, c0, mask, _ = IC.interval_case(1000 * m + i, m, r['nkey'], r['nrow'], nx, dtype, r['lanes'], params, flags, depth_chunk,
                                           r['x_kept'])
    c = _c_mode(c0, r['c_mode'])
    want = IC.partials(IC.indicators(p0, t0, c, r['lanes'], params), mask, flags, depth_chunk, r['x_kept'])
    covered_alone = r['lanes'] == IC.COVERED
    what = f'M={m} nx={nx} {mode} {np.dtype(dtype).name} {r}'
    rc, _, (got,) = _launch(ctx, IC.arrange(p0, r['where']), t0, None if covered_alone else c, mask, r['lanes'], params, r['x_kept'],
                            depth_chunk, flags, threads=r['threads'], null=('c',) if covered_alone else ())
    _hip.check(rc, what)
    assert got.shape == want.shape, what
    assert (got == np.round(got)).all() and (got >= 0).all(), f'{what}: every partial is a count'
    np.testing.assert_array_equal(got, want, err_msg=what)
    assert got.tobytes() == want.tobytes(), what
    print(f'{what}: {got.size} partials equal, value lanes sum to {got[:, :, :bin(r["lanes"]).count("1")].sum(axis=(0, 1, 3))}')


def test_the_rotation_reaches_every_setting():
  seen = [_rotation(i, MEMBERS.index(m) + 5 * j) for m in MEMBERS for j in range(3) for i in range(len(WIDTHS))]
  for key, all_of in (('nkey', {1, 2}), ('nrow', {1, 3}), ('x_kept', {True, False}), ('two_chunks', {True, False}), ('where', set(IC.MEMBER_AXES)),
                      ('c_mode', set(C_MODES)), ('lanes', set(SUBSETS)), ('threads', {256, 128, 64})):
    assert {r[key] for r in seen} == all_of, key
  assert {pair for r in seen for pair in r['pairs']} == set(PAIRS)
  sides = {IC.bound(q, m)[1] < 0.5 for m in MEMBERS for pair in PAIRS for q in pair}
  assert sides == {True, False}  # g on both sides of 0.5
  assert {IC.padded(m) for m in MEMBERS} == set(IC.SIZES)


EDGE_PARAMS = params_for(((0.1, 0.9), (0.1, 0.9), (0.2, 0.7)))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('m', (1, 2, 11, 51, 10, 64))
def test_edge_points_one_by_one(ctx, dtype, m):
  """x kept and every row its own chunk: a partial is one point.  Every edge kind of interval_cases.EDGE_KINDS at several points,
  all three lanes, against the restatement; the hand-known ones against what they must give."""
  nx = 67
  rng = np.random.default_rng(m)
  p, t, c = IC.values(50 + m, m, (2, 3, nx), dtype)
  kinds = {}
  for j, s in enumerate(rng.choice(2 * 3 * nx, size=4 * len(IC.EDGE_KINDS), replace=False)):
    at = tuple(int(v) for v in np.unravel_index(s, (2, 3, nx)))
    kinds[at] = IC.EDGE_KINDS[j % len(IC.EDGE_KINDS)]
    IC.put_edge(p, t, c, at, kinds[at], EDGE_PARAMS, rng)
  want = np.stack(IC.indicators(p, t, c, 7, EDGE_PARAMS), axis=2)  # [key, row, lane, x]
  rc, _, (got,) = _launch(ctx, IC.arrange(p, 'inner'), t, c, None, 7, EDGE_PARAMS, True, 1, 0, threads=128)
  _hip.check(rc, 'edge points')
  assert not np.isnan(got).any()
  np.testing.assert_array_equal(got, want)
  for (k, r, x), kind in kinds.items():
    cov, conf, jac = got[k, r, :, x]
    if kind in ('nan_member', 'nan_target'):
      assert cov == 0, kind
    if kind in ('nan_member', 'nan_clim'):
      assert conf == 0, kind  # NaN < x is false (nan_clim: the lower level of Confident's pair is NaN)
    if kind == 'nan_member':
      assert jac == 0, kind  # union > 0 is false for NaN: index = 1, distance 0
    if kind == 'equal_members_point_clim':
      assert (conf, jac) == (0, 0), kind  # 0 < thr * 0 is false; union 0 -> index 1 -> distance 0
    if kind == 'target_on_low' and dtype == np.float64 and not np.isnan(p[:, k, r, x]).any():
      assert cov == 1, kind  # both ends are included
    if kind == 'two_pos_inf' and m >= 2 and IC.bound(0.9, m)[0] >= m - 2 and IC.bound(0.9, m)[1] > 0:
      assert cov == 0, kind  # hi = inf - (inf - inf) * (1 - g) is NaN


def test_a_contracted_multiply_add_would_flip_covered(ctx):
  """The points of interval_cases.fma_flip_point: A + d g rounded twice covers (or does not cover) the target, rounded once it is the
  other way round.  The kernel must side with the two roundings, on both branches of the interpolation."""
  for m, q in ((10, 0.1), (10, 0.15)):
    xs, ts, wants = [], [], []
    for seed in range(8):
      x, target, levels, stated, fused = IC.fma_flip_point(m, q, np.float64, seed)
      assert stated != fused
      xs.append(x)
      ts.append(target)
      wants.append(float(stated))
    p = np.stack(xs, axis=1)[:, None, None, :]  # [M, 1, 1, 8]
    t = np.array(ts)[None, None, :]
    params = {IC.COVERED: (levels, None)}
    np.testing.assert_array_equal(IC.indicators(p, t, None, 1, params)[0][0, 0], wants)
    for x_kept in (True, False):
      rc, _, (got,) = _launch(ctx, p, t, None, None, 1, params, x_kept, 1, 0, null=('c',))
      _hip.check(rc, 'flip points')
      np.testing.assert_array_equal(got[0, 0, 0], wants if x_kept else [sum(wants)])


def test_two_launches_of_one_case_are_bit_equal(ctx):
  for m, nx, x_kept, flags, dtype in ((51, 129, False, 0, np.float32), (64, 65, True, _hip.FLAG_SKIPNA, np.float64),
                                      (7, 63, False, _hip.FLAG_MASKED, np.float32)):
    p0, t0, c0, mask, want = IC.interval_case(77 + m, m, 2, 3, nx, dtype, 7, EDGE_PARAMS, flags, 2, x_kept)
    rc, _, (a, b) = _launch(ctx, IC.arrange(p0, 'inner'), t0, c0, mask, 7, EDGE_PARAMS, x_kept, 2, flags, repeat=2)
    _hip.check(rc, 'repeat')
    assert a.tobytes() == b.tobytes() == want.tobytes(), (m, nx)


def test_partials_feed_the_contraction_unchanged(ctx):
  """wbx_contract on the partial: the weighted sums of the three indicators and of the mask's count lane."""
  rng = np.random.default_rng(8)
  for x_kept in (True, False):
    p0, t0, c0, mask, want = IC.interval_case(31, 11, 2, 3, 70, np.float32, 7, EDGE_PARAMS, _hip.FLAG_MASKED, 2, x_kept)
    rc, plan, (got,), out = _launch(ctx, p0, t0, c0, mask, 7, EDGE_PARAMS, x_kept, 2, _hip.FLAG_MASKED, keep_out=True)
    _hip.check(rc, 'partial')
    nkey, nchunk, nlane, nj = got.shape
    w = rng.integers(1, 9, size=(1, 1, nj, 2)).astype(np.float64)  # [nBk][nBr][nj][nbin]
    st = _hip.S2PlanStruct(nkey, 1, 1, nchunk, nlane, nj, 2, 1)
    res = ctx.alloc(nkey * nlane * 2 * 8)
    _hip.check(ctx.lib.wbx_contract(ctx.handle, C.byref(st), C.c_void_p(out.ptr), C.c_void_p(ctx.upload(w).ptr), C.c_void_p(res.ptr)),
               'wbx_contract')
    have = ctx.download(res.ptr, (nkey, 1, nlane, 1, 2), np.float64)
    np.testing.assert_array_equal(have[:, 0, :, 0, :], np.einsum('kclj,jn->kln', want, w[0, 0]))  # small integers: exact


def test_vec_4_is_accepted_and_ignored(ctx):
  p0, t0, c0, mask, want = IC.interval_case(12, 7, 2, 3, 8, np.float32, 7, EDGE_PARAMS, 0, 3, False)
  rc, _, (got,) = _launch(ctx, p0, t0, c0, mask, 7, EDGE_PARAMS, False, 3, 0, vec=4)
  _hip.check(rc, 'vec = 4')
  np.testing.assert_array_equal(got, want)


def _set(slot, end, field, value):
  def tweak(arr):
    setattr(getattr(arr[slot], end), field, value)
  return tweak


def test_refusals_leave_the_output_untouched(ctx):
  p, t, c, mask, _ = IC.interval_case(9, 5, 2, 3, 9, np.float32, 7, EDGE_PARAMS, 0, 3, False)
  cases = [
      ('1..64 members', dict(m=0)),
      ('1..64 members', dict(m=_hip.IVL_MAX_MEMBERS + 1)),
      ('non-empty set of WBX_IVL', dict(lanes=0)),
      ('non-empty set of WBX_IVL', dict(lanes=8)),
      ('non-empty set of WBX_IVL', dict(lanes=15)),
      ('rank -1 outside', dict(tweak=_set(0, 'lo', 'k', -1))),
      ('rank 5 outside', dict(tweak=_set(1, 'hi', 'k', 5))),
      ('outside \\[0, 1\\)', dict(tweak=_set(2, 'lo', 'g', 1.0))),
      ('outside \\[0, 1\\)', dict(tweak=_set(0, 'hi', 'g', -0.25))),
      ('outside \\[0, 1\\)', dict(tweak=_set(1, 'lo', 'g', float('nan')))),
      ('unknown dtype', dict(dtype_code=7)),
      ('mask is NULL', dict(flags=_hip.FLAG_MASKED, with_mask=False)),
      ('flags other than MASKED', dict(flags=_hip.FLAG_FAIR)),
      ('flags other than MASKED', dict(flags=_hip.FLAG_SKIPNA_ENS)),
      ('no plane mode', dict(plane_rows=3)),
      ('no folded x weights', dict(x_weights=True)),
      ('p is NULL', dict(null=('p',))),
      ('t is NULL', dict(null=('t',))),
      ('c is NULL', dict(null=('c',))),
      ('c is NULL', dict(null=('c',), lanes=IC.JACCARD)),
  ]
  for message, kw in cases:
    kw = dict(kw)
    flags, lanes = kw.pop('flags', 0), kw.pop('lanes', 7)
    rc, _, (got,) = _launch(ctx, p, t, c, mask, lanes, EDGE_PARAMS, False, 3, flags, sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message
  # a bound of a lane that is not asked for is not looked at, and Confident alone needs no targets
  rc, _, _ = _launch(ctx, p, t, c, mask, IC.COVERED, EDGE_PARAMS, False, 3, 0, tweak=_set(1, 'lo', 'k', 99))
  _hip.check(rc, 'an unused lane')
  rc, _, (got,) = _launch(ctx, p, t, c, mask, IC.CONFIDENT, EDGE_PARAMS, False, 3, 0, null=('t',))
  _hip.check(rc, 'Confident without targets')
  np.testing.assert_array_equal(got, IC.partials(IC.indicators(p, t, c, IC.CONFIDENT, EDGE_PARAMS), mask, 0, 3, False))


@pytest.mark.parametrize('mode', list(MODES))
def test_no_rows_or_no_x_zero_the_partial(ctx, mode):
  p, t, c, mask, _ = IC.interval_case(4, 5, 2, 3, 9, np.float32, 7, EDGE_PARAMS, 0, 3, False)
  for x_kept in (False, True):
    rc, _, (got,) = _launch(ctx, p, t, c, mask, 7, EDGE_PARAMS, x_kept, 3, MODES[mode], sentinel=SENTINEL, ndepth0=True)
    _hip.check(rc, 'ndepth == 0')
    assert (got == 0.0).all() and not np.signbit(got).any()
  rc, _, (got,) = _launch(ctx, p, t, c, mask, 7, EDGE_PARAMS, False, 3, MODES[mode], sentinel=SENTINEL, nx0=True)
  _hip.check(rc, 'nx == 0')
  assert (got == 0.0).all() and not np.signbit(got).any()


def test_no_keys_touch_nothing(ctx):
  p, t, c, mask, _ = IC.interval_case(4, 5, 2, 3, 9, np.float32, 7, EDGE_PARAMS, 0, 3, False)
  rc, _, (got,) = _launch(ctx, p, t, c, mask, 7, EDGE_PARAMS, False, 3, 0, sentinel=SENTINEL, nkey0=True, null=('p', 't', 'c'))
  _hip.check(rc, 'nkey == 0')
  assert (got == SENTINEL).all()
