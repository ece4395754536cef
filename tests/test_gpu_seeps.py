"""wbx_seeps_partial through the raw C ABI: EVERY partial `partial[key][chunk][lane][j]` against the restatement (tests/seeps_cases.py).

Frame (key = 1..2, row = 1..3, x); p[key, row, x], t[key, row, x].  The wet thresholds are a source ws[G, place...] behind a gather
table with repeated and out-of-order positions -- over the keys (a place is (row, x)), over the rows (a place is (key, x)) or over
both (a place is x) -- once with the places stored x-fastest and once transposed (x stride = rows); the score table lies on the same
places, nine cells of `cell_stride` = one slab apart.  A table address that wrongly included the gather term would read another place's
scores, or beyond the cell.  Tables of small integers make every sum exact: bit for bit.  With arbitrary tables, inf and NaN entries
included, a partial of one point is bit for bit and a sum of N points lies within N * 2^-53 * sum |v_i| of the sum rounded once (the
first-order bound of a float64 sum of N terms in any order; N (N - 1) 2^-53 <= 1 for every N here), with NaN and inf where the
restatement has them."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import seeps_cases as SC

pytestmark = pytest.mark.gpu
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked_skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
KEY, ROW, X = 'key', 'row', 'x'
SDIMS = (KEY, ROW, X)
SENTINEL = -77.0
WIDTHS, GATHERS, TABLE_KINDS = SC.WIDTHS, SC.GATHERS, SC.TABLE_KINDS
rotation, _vec = SC.rotation, SC.launch_vec
NG = 5  # gather positions in the source
DRY = SC.DRY_THRESHOLD


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def _root(a):
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


def make_case(seed, nkey, nrow, nx, dtype, gather, transposed, table_kind):
  """-> dict: p, t [key, row, x]; `ws` the wet source [G, place...] as a view whose memory order is x-fastest or transposed;
  `place_dims`; `positions` (the gather's positions over its dims); `table` [9, place...] in the same memory order; `wet`, `table9`:
  what a point sees, over the frame; mask [row, x]; values [key, row, x] by the restatement.  `table_kind`: 'int' small integers,
  'real' arbitrary numbers with inf, NaN and -0.0 among them, 'finite' arbitrary finite numbers under inputs without NaN."""
  rng = np.random.default_rng(seed)
  shape = (nkey, nrow, nx)
  place_dims = {'keys': (ROW, X), 'rows': (KEY, X), 'both': (X,)}[gather]
  gdims = {'keys': (KEY,), 'rows': (ROW,), 'both': (KEY, ROW)}[gather]
  sizes = dict(zip(SDIMS, shape))
  mem_dims = tuple(reversed(place_dims)) if transposed else place_dims  # memory order of a slab
  mshape = tuple(sizes[d] for d in mem_dims)
  back = [mem_dims.index(d) for d in place_dims]
  ws_mem = SC.wet_thresholds((NG,) + mshape, dtype, seed + 1)
  ws = ws_mem.transpose([0] + [1 + i for i in back])  # [G, place dims]
  if table_kind == 'int':
    tab_mem = rng.integers(-3, 6, size=(9,) + mshape).astype(np.float64)
  else:
    tab_mem = rng.normal(size=(9,) + mshape) * 10.0 ** rng.integers(-3, 4, size=(9,) + mshape)
    odd = rng.integers(0, 24, size=tab_mem.shape)
    for code, val in enumerate((np.inf, -np.inf, np.nan, -0.0) if table_kind == 'real' else (-0.0,)):
      tab_mem[odd == code] = val
  table = tab_mem.transpose([0] + [1 + i for i in back])
  gshape = tuple(sizes[d] for d in gdims)
  positions = rng.integers(0, NG, size=gshape)  # out of order as they come
  if positions.size > 1:
    positions.flat[-1] = positions.flat[0]  # a repeated position
  # what a point sees
  expand = lambda a: np.broadcast_to(a.reshape([a.shape[0]] + [sizes[d] if d in place_dims else 1 for d in SDIMS]), (a.shape[0],) + shape)
  pos_full = np.broadcast_to(positions.reshape([sizes[d] if d in gdims else 1 for d in SDIMS]), shape)
  wet = np.take_along_axis(expand(ws), pos_full[None], axis=0)[0]
  table9 = expand(table)
  p = SC.field_values(shape, wet, dtype, seed + 3)
  t = SC.field_values(shape, wet, dtype, seed + 4)
  if table_kind == 'finite':  # sums that stay finite in every mode: no NaN input, no inf or NaN score
    p, t = np.where(np.isnan(p), dtype(0.001), p), np.where(np.isnan(t), dtype(0.02), t)
  mask = (rng.integers(0, 4, size=(nrow, nx)) != 0).astype(np.uint8)
  values = SC.point_values(p, t, wet, table9, DRY, dtype)
  if p.size >= 300 and table_kind != 'finite':  # (a handful of points cannot hold every cell)
    SC.assert_case_is_telling(p, t, wet, values, DRY, dtype)
  return dict(p=p, t=t, ws=ws, table=table, place_dims=place_dims, gdims=gdims, positions=positions, wet=wet, table9=table9, mask=mask,
              values=values, sizes=sizes)


def launch(ctx, case, x_kept, depth_chunk, flags, threads=256, vec=1, dtype_code=None, with_mask=True, sentinel=None, ndepth0=False,
           nx0=False, nkey0=False, plane_rows=0, repeat=1, x_weights=False, null=(), keep_out=False):
  p, t, ws, table = case['p'], case['t'], case['ws'], case['table']
  sizes = case['sizes']
  nkey, nrow, nx = p.shape
  lay_m = mask_buf = None
  if flags & _hip.FLAG_MASKED:
    lay_m = planner.InputLayout(strides={ROW: nx, X: 1}, itemsize=1, base_alignment=256)  # zero stride along the keys
    mask_buf = ctx.upload(np.ascontiguousarray(case['mask'], np.uint8)) if with_mask else None
  reduce_dims = (ROW,) if x_kept else (ROW, X)
  lay_w = _layout(ws[0], case['place_dims'])  # zero strides along the dims the gather runs over
  slab = int(np.prod(ws.shape[1:]))
  spec = planner.GatherSpec(dims=case['gdims'], table=case['positions'].astype(np.int64) * slab)
  plan = planner.build_s1_plan(SDIMS, sizes, [_layout(p, SDIMS), _layout(t, SDIMS), lay_w, lay_m], reduce_dims, wdep_dims=set(),
                               gather=spec, flags=flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA), allow_vec4=False, force_x_dim=X)
  dc = min(depth_chunk, plan.ndepth)
  plan = dataclasses.replace(plan, depth_chunk=dc, nchunk=-(-plan.ndepth // dc), flags=flags, block_threads=threads, plane_rows=plane_rows,
                             vec=vec)
  assert plan.x_kept == x_kept and plan.a_dims == (KEY,) and plan.depth_dims == (ROW,) and not plan.bk_dims and not plan.br_dims, plan
  nacc = 2 if flags & (_hip.FLAG_SKIPNA | _hip.FLAG_MASKED) else 1
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
  (rp, op), (rt, ot), (rw, ow), (rtab, otab) = _root(p), _root(t), _root(ws), _root(table)
  assert ow == 0 and otab == 0 and rtab.shape[0] == 9 and rtab.size == 9 * slab  # every table read lies inside its cell: < slab
  bufs = [ctx.upload(rp), ctx.upload(rt), ctx.upload(rw), ctx.upload(rtab)]
  if dtype_code is None:
    dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  outs, rc, out = [], 0, None
  for _ in range(repeat):
    out = ctx.upload(np.full(size, sentinel, np.float64)) if sentinel is not None else ctx.alloc(size * 8)
    rc = ctx.lib.wbx_seeps_partial(
        ctx.handle, C.byref(dplan.struct), dtype_code, C.c_double(DRY), None if 'p' in null else _ptr(bufs[0], op),
        None if 't' in null else _ptr(bufs[1], ot), None if 'wet' in null else _ptr(bufs[2]),
        None if 'table' in null else _ptr(bufs[3]), slab, _ptr(mask_buf), _ptr(out))
    outs.append(ctx.download(out.ptr, shape, np.float64))
  if keep_out:
    return rc, plan, outs, out
  return rc, plan, outs


def check_partials(got, case, flags, depth_chunk, x_kept, exact, what):
  want, mag, nterm = SC.partials(case['values'], case['mask'], flags, depth_chunk, x_kept)
  assert got.shape == want.shape, what
  if flags:
    np.testing.assert_array_equal(got[:, :, 1], want[:, :, 1], err_msg=f'{what}: the count lane')
  g, w = got[:, :, 0], want[:, :, 0]
  np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f'{what}: NaN placement')
  np.testing.assert_array_equal(np.isinf(g), np.isinf(w), err_msg=f'{what}: inf placement')
  np.testing.assert_array_equal(g[np.isinf(w)], w[np.isinf(w)], err_msg=f'{what}: the sign of inf')
  if exact or (nterm == 1).all():
    assert SC.same_numbers(g, w), f'{what}: bit for bit'
    return 0.0
  fin = np.isfinite(w)
  err = np.abs(g[fin] - w[fin])
  bound = nterm[fin] * 2.0 ** -53 * mag[fin]
  assert (nterm * (nterm - 1.0) * 2.0 ** -53 <= 1).all()
  worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
  print(f'{what}: worst |d| / bound = {worst:.3g} over {int(fin.sum())} finite partials')
  assert (err <= bound).all(), f'{what}: |d| <= N 2^-53 sum |v|, worst ratio {worst}'
  return worst


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('mode', list(MODES))
def test_every_partial_against_the_restatement(ctx, mode, dtype):
  flags = MODES[mode]
  k0 = 3 * list(MODES).index(mode) + (dtype == np.float64)
  for j, table_kind in enumerate(TABLE_KINDS):
    for i, nx in enumerate(WIDTHS):
      r = rotation(i + 7 * j, k0)
      depth_chunk = 2 if r['two_chunks'] else r['nrow']
      case = make_case(1000 * k0 + 10 * i + j, r['nkey'], r['nrow'], nx, dtype, r['gather'], r['transposed'], table_kind)
      what = f'nx={nx} {mode} {np.dtype(dtype).name} {table_kind} {r}'
      rc, _, (got,) = launch(ctx, case, r['x_kept'], depth_chunk, flags, threads=r['threads'], vec=_vec(r, nx))
      _hip.check(rc, what)
      check_partials(got, case, flags, depth_chunk, r['x_kept'], table_kind == 'int', what)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_every_dim_kept_is_the_table_entry_bit_for_bit(ctx, dtype):
  """x kept and every row its own chunk: a partial is one point, 0.0 + its value, whatever the table holds."""
  for gather, transposed in (('keys', False), ('keys', True), ('rows', True), ('both', False)):
    case = make_case(77, 2, 3, 131, dtype, gather, transposed, 'real')
    SC.assert_case_is_telling(case['p'], case['t'], case['wet'], case['values'], DRY, dtype)
    for flags in MODES.values():
      rc, _, (got,) = launch(ctx, case, True, 1, flags, threads=128)
      _hip.check(rc, 'every dim kept')
      check_partials(got, case, flags, 1, True, True, f'{gather} transposed={transposed} flags={flags}')
    assert np.isinf(case['values']).any() and np.isnan(case['table']).any()


def test_the_float32_dry_threshold_itself_is_dry(ctx):
  """float32(0.00025) > 0.00025: the float64 comparison would call the value light.  Table cell (f, o) holds 3 f + o."""
  at = np.float32(DRY)
  assert float(at) > DRY
  lo, _, hi = SC.next_to(DRY, np.float32)
  p = np.array([lo, at, hi, -0.0, np.inf, -np.inf, 0.005, 0.004], np.float32).reshape(1, 1, 8)
  t = np.full((1, 1, 8), at, np.float32)
  ws = np.full((NG, 8), 0.005, np.float32)
  ws[:, 7] = np.nan  # a NaN threshold under a value that is not dry: none -> cell (0, 0)
  table = np.broadcast_to(np.arange(9.0).reshape(9, 1), (9, 8)).copy()
  case = dict(p=p, t=t, ws=ws, table=table, place_dims=(X,), gdims=(KEY, ROW), positions=np.array([[2]]), sizes={KEY: 1, ROW: 1, X: 8})
  rc, _, (got,) = launch(ctx, case, True, 1, 0)
  _hip.check(rc, 'thresholds')
  np.testing.assert_array_equal(got[0, 0, 0], [0, 0, 3, 0, 6, 0, 6, 0])


def test_two_launches_of_one_case_are_bit_equal(ctx):
  for nx, x_kept, flags, dtype in ((129, False, 0, np.float32), (65, True, _hip.FLAG_SKIPNA, np.float64), (200, False, _hip.FLAG_MASKED, np.float32)):
    case = make_case(5 + nx, 2, 3, nx, dtype, 'keys', False, 'real')
    rc, _, (a, b) = launch(ctx, case, x_kept, 2, flags, repeat=2)
    _hip.check(rc, 'repeat')
    assert a.tobytes() == b.tobytes(), nx


def test_partials_feed_the_contraction_unchanged(ctx):
  rng = np.random.default_rng(8)
  for x_kept in (True, False):
    case = make_case(31, 2, 3, 70, np.float32, 'rows', False, 'int')
    rc, _, (got,), out = launch(ctx, case, x_kept, 2, _hip.FLAG_SKIPNA, keep_out=True)
    _hip.check(rc, 'partial')
    nkey, nchunk, nlane, nj = got.shape
    w = rng.integers(1, 9, size=(1, 1, nj, 2)).astype(np.float64)  # [nBk][nBr][nj][nbin]
    st = _hip.S2PlanStruct(nkey, 1, 1, nchunk, nlane, nj, 2, 1)
    res = ctx.alloc(nkey * nlane * 2 * 8)
    _hip.check(ctx.lib.wbx_contract(ctx.handle, C.byref(st), C.c_void_p(out.ptr), C.c_void_p(ctx.upload(w).ptr), C.c_void_p(res.ptr)),
               'wbx_contract')
    have = ctx.download(res.ptr, (nkey, 1, nlane, 1, 2), np.float64)
    want, _, _ = SC.partials(case['values'], case['mask'], _hip.FLAG_SKIPNA, 2, x_kept)
    np.testing.assert_array_equal(have[:, 0, :, 0, :], np.einsum('kclj,jn->kln', want, w[0, 0]))  # small integers: exact


def test_refusals_leave_the_output_untouched(ctx):
  case = make_case(9, 2, 3, 12, np.float32, 'keys', False, 'int')
  cases = [
      ('unknown dtype', dict(dtype_code=7)),
      ('mask is NULL', dict(flags=_hip.FLAG_MASKED, with_mask=False)),
      ('flags other than MASKED', dict(flags=_hip.FLAG_FAIR)),
      ('flags other than MASKED', dict(flags=_hip.FLAG_SKIPNA_ENS)),
      ('no plane mode', dict(plane_rows=3)),
      ('no folded x weights', dict(x_weights=True)),
      ('p/t is NULL', dict(null=('p',))),
      ('p/t is NULL', dict(null=('t',))),
      ('wet is NULL', dict(null=('wet',))),
      ('table is NULL', dict(null=('table',))),
  ]
  for message, kw in cases:
    kw = dict(kw)
    flags = kw.pop('flags', 0)
    rc, _, (got,) = launch(ctx, case, False, 3, flags, sentinel=SENTINEL, **kw)
    assert rc == -1, message
    with pytest.raises(_hip.WbxError, match=message):
      _hip.check(rc, message)
    assert (got == SENTINEL).all(), message


@pytest.mark.parametrize('mode', list(MODES))
def test_no_rows_or_no_x_zero_the_partial(ctx, mode):
  case = make_case(4, 2, 3, 9, np.float32, 'keys', False, 'int')
  for x_kept in (False, True):
    rc, _, (got,) = launch(ctx, case, x_kept, 3, MODES[mode], sentinel=SENTINEL, ndepth0=True)
    _hip.check(rc, 'ndepth == 0')
    assert (got == 0.0).all() and not np.signbit(got).any()
  rc, _, (got,) = launch(ctx, case, False, 3, MODES[mode], sentinel=SENTINEL, nx0=True)
  _hip.check(rc, 'nx == 0')
  assert (got == 0.0).all() and not np.signbit(got).any()


def test_no_keys_touch_nothing(ctx):
  case = make_case(4, 2, 3, 9, np.float32, 'keys', False, 'int')
  rc, _, (got,) = launch(ctx, case, False, 3, 0, sentinel=SENTINEL, nkey0=True)
  _hip.check(rc, 'nkey == 0')
  assert (got == SENTINEL).all()
