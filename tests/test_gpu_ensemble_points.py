"""The five ensemble lanes (CRPS skill, CRPS spread, ensemble variance, unbiased ensemble-mean MSE, ensemble-mean squared error)
through the raw C ABI on EVERY kernel that can compute them, point by point against the float64 oracle: wbx_ens_map (every
point of every lane), and every partial `partial[key][chunk][lane][j]` of s1_xk_kernel, s1_xr_kernel, ens_pipe_kernel and its
FLAT flavour, s1_xf1_kernel, the EnsMasked wrappers and ens_atoms_kernel (wbx_ens_binned).  Each test asserts from its plan
that it runs the route it names (the rules of launch_ens_bucket / ens_pipe_ok / ens_pipe_flat_ok, restated in `_route`).

Two kinds of case (tests/ensemble_cases.py): DENSE -- every point is live, dyadic values (ties are ties, sums exact) and
anomaly-like values (N(0, 1), a share of points spanning 1e-6 .. 1e6, a variant whose target cancels against the ensemble
mean: the data on which fp32 chains round) -- and ONE LIVE POINT PER PARTIAL: every other point has all members equal to its
target, so all its lanes are exactly 0 on every route and an x-summed partial IS its live point's value.  Partials without a
live point must be bit-exact zeros: that is the check on the staging buffer, the one-tile-ahead registers, the tail lanes and
the ragged tiles of the pipelined sweeps.

Expectation and bounds: ensemble_cases.expected_lanes / lane_bounds (derived from the arithmetic, see there and include/wbx.h).
NaN and +-inf sit at the same positions on both sides; a dense plain-mode case keeps >= 80 % of its outputs finite, under
skipna every output is finite; count lanes are bit-equal."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import ensemble_cases as EC
import test_gpu_indicators as GI
import test_gpu_round4 as R4

pytestmark = pytest.mark.gpu
EPS = EC.EPS
LEAD, ROW, X = GI.LEAD, GI.ROW, GI.X
NL = EC.NLANE
M_CASES = [(m, np.float32) for m in EC.M_F32] + [(m, np.float64) for m in EC.M_F64]
M_IDS = [f'M{m}-{np.dtype(d).name}' for m, d in M_CASES]
M_REG = [m for m in EC.M_F32 if m <= 64]  # float32 members in registers: the sizes the pipelined sweeps take


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def _route(plan, m, dtype, algo):
  """The kernel wbx_ens_partial launches for this plan (launch_ens_bucket, launch_ens_op, launch_partial)."""
  assert os.environ.get('WBX_ENS_PIPE', '1') != '0', 'the routes are named for the default WBX_ENS_PIPE'
  wrapped = bool(plan.flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA))
  registers = np.dtype(dtype) == np.float32 and m <= 64
  if registers and algo == EC.SORT and not wrapped and not plan.x_kept and plan.block_threads == 64 and not (plan.flags & _hip.FLAG_SKIPNA_ENS):
    if plan.x_weights is None:
      return 'pipe'
    if plan.plane_rows > 0 and plan.ndepth % plan.plane_rows == 0 and plan.xstride[0] == 1 and plan.xstride[1] == 1:
      return 'flat'
  if plan.x_weights is not None:
    return 'xf1+masked' if wrapped else 'xf1'
  return ('xk' if plan.x_kept else 'xr') + ('+masked' if wrapped else '')


def _plans(ctx, p, t, x_kept, depth_chunk, flags, block=None, flat=None):
  """GI._plan on p[lead, member, row, x] / t[lead, row, x], then the block size and (flat = (R, weights)) the folded x weights."""
  nlead, _, nrow, nx = p.shape
  sizes = {LEAD: nlead, ROW: nrow, X: nx}
  lay_p, mstride = GI._layout(p, GI.PD)  # pylint: disable=protected-access
  lay_t, _ = GI._layout(t, GI.SDIMS)  # pylint: disable=protected-access
  lay_m = planner.InputLayout(strides={ROW: nx, X: 1}, itemsize=1, base_alignment=256) if flags & _hip.FLAG_MASKED else None
  plan, dplan = GI._plan(ctx, sizes, [lay_p, lay_t, None, lay_m], x_kept, depth_chunk, flags)  # pylint: disable=protected-access
  if block is not None or flat is not None:
    plan = dataclasses.replace(plan, block_threads=plan.block_threads if block is None else block)
    if flat is not None:
      plan = dataclasses.replace(plan, plane_rows=flat[0])
      plan.x_weights = np.ascontiguousarray(flat[1], np.float64)
    dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  return plan, dplan, mstride


def _run_partial(ctx, p, t, mask, plan, dplan, mstride, algo, sentinel=None):
  m = p.shape[1]
  shape = (p.shape[0], plan.nchunk, GI._lanes_total(NL, plan.flags), plan.nj)  # pylint: disable=protected-access
  n = int(np.prod(shape))
  out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
  bufs = ctx.upload(GI._root(p)), ctx.upload(GI._root(t))  # pylint: disable=protected-access
  mask_buf = ctx.upload(np.ascontiguousarray(mask, np.uint8)) if plan.flags & _hip.FLAG_MASKED else None
  dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  _hip.check(ctx.lib.wbx_ens_partial(ctx.handle, C.byref(dplan.struct), dtype_code, m, mstride, algo, GI._ptr(bufs[0]), GI._ptr(bufs[1]),  # pylint: disable=protected-access
                                     GI._ptr(mask_buf), GI._ptr(out)), 'wbx_ens_partial')  # pylint: disable=protected-access
  return ctx.download(out.ptr, shape, np.float64)


def _run_map(ctx, p, t, plan, dplan, mstride, algo):
  """-> [lead, row, x, lane]: one wbx_ens_map launch per lane."""
  nlead, m, nrow, nx = p.shape
  bufs = ctx.upload(GI._root(p)), ctx.upload(GI._root(t))  # pylint: disable=protected-access
  dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  out = ctx.alloc(nlead * nrow * nx * 8)
  lanes = []
  for lane in range(NL):
    _hip.check(ctx.lib.wbx_ens_map(ctx.handle, C.byref(dplan.struct), dtype_code, m, mstride, algo, lane, GI._ptr(bufs[0]), GI._ptr(bufs[1]),  # pylint: disable=protected-access
                                   GI._ptr(out)), 'wbx_ens_map')  # pylint: disable=protected-access
    lanes.append(ctx.download(out.ptr, (nlead, nrow, nx), np.float64))
  return np.stack(lanes, axis=-1)


def _assert_within(got, want, tol, what):
  """NaN and +-inf at the same positions on both sides, every finite value within its bound."""
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{what}: NaN positions')
  inf = np.isinf(want)
  np.testing.assert_array_equal(np.isinf(got), inf, err_msg=f'{what}: inf positions')
  np.testing.assert_array_equal(got[inf], want[inf], err_msg=f'{what}: signs of the infinities')
  fin = np.isfinite(want)
  with np.errstate(invalid='ignore'):  # (inf - inf at the positions just compared)
    err = np.abs(got - want)
    bad = fin & ~(err <= tol)
  if bad.any():
    i = tuple(np.argwhere(bad)[0])
    ratio = np.where(fin & (tol > 0), err / np.where(tol > 0, tol, 1.0), np.where(fin & (err > 0), np.inf, 0.0))
    raise AssertionError(f'{what}: {int(bad.sum())} of {int(fin.sum())} outputs outside their bound; first at [.., lane, j] = {i}: got '
                         f'{got[i]!r} want {want[i]!r} bound {tol[i]!r}; worst error / bound {float(ratio.max()):.3g}')


def _check_partials(got, plan, stat, bound, mask, what, weights=None, dense_mode=None, share_lanes=slice(0, NL)):
  """got[lead][chunk][lanes][j] against stat / bound [lead, row, x, 5] summed the way the plan sums them."""
  flags = plan.flags
  w = 1.0 if weights is None else np.asarray(weights)[None, None, :, None]
  want = GI._expected_partials(plan, stat * w, mask, flags)  # pylint: disable=protected-access
  assert got.shape == want.shape, (what, got.shape, want.shape)
  if dense_mode is not None:
    if flags & _hip.FLAG_SKIPNA:
      assert np.isfinite(want).all(), what
    else:
      share = EC.finite_share(want, share_lanes)
      assert share >= 0.8, (what, 'finite share', share)
  GI._check_counts(got, want, NL, flags, what)  # pylint: disable=protected-access
  with np.errstate(invalid='ignore'):
    per_point = np.where(np.isfinite(stat), bound, np.nan) * w
    size = np.where(np.isfinite(stat), np.abs(stat), np.nan) * w
  # (the same validity as the values: what the mask hides or skipna counts out adds nothing to a partial's bound)
  vflags = flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA)
  b = GI._expected_partials(plan, per_point, mask, vflags)[:, :, :NL]  # pylint: disable=protected-access
  s = GI._expected_partials(plan, size, mask, vflags)[:, :, :NL]  # pylint: disable=protected-access
  n = GI._points_per_partial(plan)  # pylint: disable=protected-access
  _assert_within(got[:, :, :NL], want[:, :, :NL], b + (n + 2) * EPS * s, what)
  return want


def _flags(mode, fair):
  return GI.MODES[mode] | (_hip.FLAG_FAIR if fair else 0)


def _share_lanes(m, fair):
  """The lanes that are finite at an ordinary point: all five -- but with a single member variance and unbiased MSE are NaN by
  definition (ddof = 1) and so is the fair spread."""
  return slice(0, NL) if m > 1 else ([0, 4] if fair else [0, 1, 4])


def _dense(seed, m, dtype, grid, values, mode, x_kept, fam, all_exposed=False):
  name, nlead, nrow, nx, dc, layout = grid
  if all_exposed:  # the map writes every point: nothing poisons anything
    poison = exposed = tuple(range(0, nrow, 7))
  else:
    poison, exposed = GI._poison_rows(mode, nrow, nx, x_kept, dc)  # pylint: disable=protected-access
  inf_members = fam in ('sorted64', 'chain32')
  return EC.dense_case(seed, m, nlead, nrow, nx, values=values, dtype=dtype, layout=layout, poison_rows=poison, exposed_rows=exposed,
                       inf_members=inf_members)


# (name, leads, rows, x, rows per partial (None: all), member layout)
GRIDS = [
    ('x1-1row', 2, 7, 1, 1, 'member_outside'),
    ('x63-3rows', 2, 7, 63, 3, 'ifs'),
    ('x64-all', 2, 5, 64, None, 'member_outside'),
    ('x65-1row', 2, 7, 65, 1, 'ifs'),
    ('x130-3rows', 2, 7, 130, 3, 'member_outside'),
    ('x181-1row', 2, 6, 181, 1, 'ifs'),
]
VALUES = ('dyadic', 'anomaly', 'cancel')


def _dense_inputs(route, m, dtype, mode, x_kept, algo=EC.SORT, grids=GRIDS, values=VALUES):
  """The dense cases of a route: (i + j, grid, values, fair, family, p, t, mask)."""
  fam = EC.family(route.split('+')[0], m, dtype, algo)
  for i, grid in enumerate(grids):
    for j, vals in enumerate(values):
      p, t, mask = _dense(100 * m + 10 * i + j, m, dtype, grid, vals, mode, x_kept, fam)
      yield i + j, grid, vals, EC.fair_of(m, i + j), fam, p, t, mask


def _dense_partials(ctx, route, m, dtype, mode, x_kept, algo=EC.SORT, blocks=(None,), grids=GRIDS, values=VALUES):
  for k, grid, vals, fair, fam, p, t, mask in _dense_inputs(route, m, dtype, mode, x_kept, algo, grids, values):
    block = blocks[k % len(blocks)]
    plan, dplan, mstride = _plans(ctx, p, t, x_kept, grid[4], _flags(mode, fair), block=block)
    assert _route(plan, m, dtype, algo) == route, (route, _route(plan, m, dtype, algo), plan.block_threads)
    got = _run_partial(ctx, p, t, mask, plan, dplan, mstride, algo)
    stat = EC.expected_lanes(fam, p, t, fair)
    _check_partials(got, plan, stat, EC.lane_bounds(fam, p, t, stat), mask, f'{route} {grid[0]} {vals} M={m} {mode} fair={fair} block={block}',
                    dense_mode=mode, share_lanes=_share_lanes(m, fair))


# ---- dense: one parametrised test per route --------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,dtype', M_CASES, ids=M_IDS)
def test_map_every_point_every_lane(ctx, m, dtype):
  """wbx_ens_map (s1_map_kernel): fp64 sums (stats64) for every float32 M <= 64 -- M = 50 / 51 too: the map never runs the
  fp32 chains --, the generic operator above and for float64; the rank form and (M <= 64) the pair form."""
  for algo in (EC.SORT, EC.PAIRWISE):
    fam = EC.family('map', m, dtype, algo)
    if algo == EC.PAIRWISE and fam != 'pair':
      continue
    for i, grid in enumerate(GRIDS[1::2] if algo == EC.SORT else GRIDS[4:5]):
      for j, vals in enumerate(VALUES):
        fair = EC.fair_of(m, i + j)
        p, t, _ = _dense(300 * m + 10 * i + j, m, dtype, grid, vals, 'plain', True, fam, all_exposed=True)
        plan, dplan, mstride = _plans(ctx, p, t, True, grid[4], _flags('plain', fair))
        got = _run_map(ctx, p, t, plan, dplan, mstride, algo)
        stat = EC.expected_lanes(fam, p, t, fair)
        assert EC.finite_share(stat[..., _share_lanes(m, fair)]) >= 0.8
        _assert_within(got, stat, EC.lane_bounds(fam, p, t, stat), f'map {grid[0]} {vals} M={m} algo={algo} fair={fair}')


@pytest.mark.parametrize('m,dtype', M_CASES, ids=M_IDS)
def test_x_kept_every_partial(ctx, m, dtype):
  """s1_xk_kernel: one partial per (lead, chunk of rows, x)."""
  _dense_partials(ctx, 'xk', m, dtype, 'plain', True)


@pytest.mark.parametrize('m,dtype', M_CASES, ids=M_IDS)
def test_x_summed_wide_blocks_every_partial(ctx, m, dtype):
  """s1_xr_kernel: x summed by blocks of 128 and 256 threads (ens_pipe_ok wants 64); the generic operator also at 64."""
  blocks = (128, 256) if EC.family('xr', m, dtype) != 'generic' else (64, 128, 256)
  _dense_partials(ctx, 'xr', m, dtype, 'plain', False, blocks=blocks)


@pytest.mark.parametrize('m', M_REG)
def test_pair_form_every_partial(ctx, m):
  """WBX_ENS_PAIRWISE: x summed by one-wave blocks stays on s1_xr_kernel (the pipelined sweep takes the rank form only), and
  x kept; the spread's |x_i - x_j| rows are fp32."""
  _dense_partials(ctx, 'xr', m, np.float32, 'plain', False, algo=EC.PAIRWISE, blocks=(64,), grids=GRIDS[3:5])
  _dense_partials(ctx, 'xk', m, np.float32, 'plain', True, algo=EC.PAIRWISE, grids=GRIDS[1:2])


@pytest.mark.parametrize('m', M_REG)
def test_pipelined_sweep_every_partial(ctx, m):
  """ens_pipe_kernel<.., false>: one-wave blocks, rank form.  M = 50 / 51: the fp32 chains (stats32) on data that makes them
  round; every other M: stats64 behind the same staging buffer."""
  _dense_partials(ctx, 'pipe', m, np.float32, 'plain', False, blocks=(64,))


FLAT_GRIDS = [  # (name, leads, rows, x, rows per partial, layout, R)
    ('x24-R3', 2, 6, 24, 2, 'member_outside', 3),
    ('x64-R1', 2, 6, 64, 2, 'ifs', 1),
    ('x91-R4', 2, 8, 91, 2, 'member_outside', 4),
    ('x91-R3', 2, 6, 91, 2, 'ifs', 3),
]


def _flat_weights(nx, seed):
  return np.random.default_rng(seed).integers(1, 17, size=nx) / 8.0  # dyadic: weight x value adds no rounding of its own


def _flat_inputs(route, m, dtype):
  fam = EC.family(route, m, dtype)
  for i, grid in enumerate(FLAT_GRIDS):
    for j, vals in enumerate(VALUES[:2]):
      p, t, mask = _dense(500 * m + 10 * i + j, m, dtype, grid[:6], vals, 'plain', False, fam)
      yield grid, vals, EC.fair_of(m, i + j), fam, p, t, mask, _flat_weights(grid[3], m + i)


@pytest.mark.parametrize('block,route', [(64, 'flat'), (128, 'xf1')])
@pytest.mark.parametrize('m,dtype', M_CASES, ids=M_IDS)
def test_flat_weighted_sweeps_every_partial(ctx, m, dtype, block, route):
  """plan->x_weights over contiguous planes of R rows: ens_pipe_kernel<.., true> (one-wave blocks, float32 M <= 64) and
  s1_xf1_kernel (128 threads; any M and dtype).  Two rows per chunk with R = 3: a chunk starts inside a plane and its first
  tile starts in front of e0."""
  if route == 'flat' and (dtype == np.float64 or m > 64):
    route = 'xf1'  # (the generic operator has no pipelined flavour: s1_xf1_kernel with one-wave blocks)
  for grid, vals, fair, fam, p, t, mask, w in _flat_inputs(route, m, dtype):
    plan, dplan, mstride = _plans(ctx, p, t, False, grid[4], _flags('plain', fair), block=block, flat=(grid[6], w))
    assert _route(plan, m, dtype, EC.SORT) == route and plan.depth_chunk == 2, (route, plan)
    got = _run_partial(ctx, p, t, mask, plan, dplan, mstride, EC.SORT)
    stat = EC.expected_lanes(fam, p, t, fair)
    _check_partials(got, plan, stat, EC.lane_bounds(fam, p, t, stat), mask, f'{route} {grid[0]} {vals} M={m} fair={fair}', weights=w,
                    dense_mode='plain', share_lanes=_share_lanes(m, fair))


@pytest.mark.parametrize('x_kept', [True, False], ids=['xkept', 'xsummed'])
@pytest.mark.parametrize('mode', ['masked', 'skipna', 'masked+skipna'])
@pytest.mark.parametrize('m,dtype', M_CASES, ids=M_IDS)
def test_masked_and_skipna_wrappers_every_partial(ctx, m, dtype, mode, x_kept):
  """EnsMasked<Core, false / true> on x kept and on x summed (one-wave blocks: the wrappers keep the sweep off the pipelined
  kernel): fp64 cores, the count lanes bit-equal."""
  _dense_partials(ctx, ('xk' if x_kept else 'xr') + '+masked', m, dtype, mode, x_kept, blocks=(None,) if x_kept else (64, 128),
                  grids=GRIDS[1:5], values=VALUES[:2])


# ---- one live point per partial ---------------------------------------------------------------------------------------------------
M_LIVE = [2, 5, 17, 33, 50, 51, 64]


def _one_live(ctx, route, m, dtype, nrow, nx, dc, x_kept, mode='plain', block=None, flat=None, algo=EC.SORT, shift=0, layout='member_outside',
              kinds=None, positions=None):
  fam = EC.family(route.split('+')[0], m, dtype, algo)
  fair = EC.fair_of(m, shift)
  kinds = EC.live_points(m) if kinds is None else kinds
  p, t, live = EC.one_live_case(m, 2, nrow, nx, dc, kinds, shift=shift, layout=layout, dtype=dtype, positions=positions)
  mask = np.ones((nrow, nx), bool)
  plan, dplan, mstride = _plans(ctx, p, t, x_kept, dc, _flags(mode, fair), block=block, flat=flat)
  assert _route(plan, m, dtype, algo) == route, (route, _route(plan, m, dtype, algo))
  got = _run_partial(ctx, p, t, mask, plan, dplan, mstride, algo, sentinel=-77.0)
  stat = EC.expected_lanes(fam, p, t, fair)
  is_live = np.zeros(t.shape, bool)
  for lead, row, x, _ in live:
    is_live[lead, row, x] = True
  assert (stat[~is_live] == 0.0).all()  # every other point: five exact zeros
  what = f'one live point: {route} M={m} nx={nx} rows/partial={dc} {mode} shift={shift} kinds={[k[3] for k in live]}'
  want = _check_partials(got, plan, stat, EC.lane_bounds(fam, p, t, stat), mask, what, weights=None if flat is None else flat[1])
  # a partial without a live point: bit-exact zeros, whatever its neighbours hold
  has_live = GI._expected_partials(plan, is_live[..., None].astype(np.float64), mask, 0)[:, :, 0] > 0  # pylint: disable=protected-access
  assert has_live.any() and (~has_live).any()
  quiet = got[:, :, :NL][np.broadcast_to(~has_live[:, :, None], got[:, :, :NL].shape)]
  assert (quiet == 0.0).all() and not np.signbit(quiet).any(), (what, 'a partial without a live point is not +0.0', quiet[quiet != 0][:4])
  assert (want[:, :, :NL][np.broadcast_to(~has_live[:, :, None], want[:, :, :NL].shape)] == 0.0).all()


@pytest.mark.parametrize('m', M_LIVE)
def test_pipelined_sweep_one_live_point_per_partial(ctx, m):
  """ens_pipe_kernel: the live point at lane 0, at lane 63, in the last ragged tile (130 = 2 x 64 + 2; 65 = 64 + 1), in the
  first and in the last row of a chunk; 1 and 3 rows per partial.  At M = 50 / 51 the threshold points decide between the fp32
  chains and the wave-uniform fp64 redo, and a NaN / infinite member has to survive the redo (apply_poison)."""
  nk = len(EC.live_points(m))
  for shift, (nx, dc) in enumerate(((130, 3), (65, 1), (181, 3), (64, 1))):
    _one_live(ctx, 'pipe', m, np.float32, nk * dc, nx, dc, False, block=64, shift=shift, layout='ifs' if shift & 1 else 'member_outside')


ESCAPES = ('range_2^-51', 'big_2^101', 'pinf_target')  # outside compute<FAST32>'s thresholds: the whole tile is redone in fp64


@pytest.mark.parametrize('route', ['pipe', 'flat'])
@pytest.mark.parametrize('m', [50, 51])
def test_escape_and_ordinary_point_in_one_tile(ctx, m, route):
  """M = 50 / 51 on ens_pipe_kernel and its FLAT flavour: a point outside the fp32 thresholds (range 2^-51; a magnitude of
  2^101; a +inf target) makes its whole 64-lane tile redo the point in fp64 -- the ordinary live point two lanes away is
  redone with it and must come out within its bound, and an infinite member in such a tile still poisons all five lanes of
  its own partial only.  On these two kernels one wave owns one (lead, chunk), so points of one tile share a partial: the
  pair is held through the partial's sum (rows of one 64-lane tile, one row per partial; FLAT: planes of three such rows,
  the sum weighted), the poisoned point sits in the next row.  ens_atoms_kernel, whose tile spans several bins, holds them
  per point: test_binned_escape_and_ordinary_point_in_one_tile.  (A NaN target is no escape -- the kernel's fmaxf drops
  it -- and is held by the one-live-point cases.)"""
  kinds = {k[0]: k for k in EC.live_points(m)}
  fam = EC.family(route, m, np.float32)
  assert fam == 'chain32'
  nrow, nx = 6, 64
  flat = (3, _flat_weights(nx, m)) if route == 'flat' else None
  for escape in ESCAPES:
    for fair in (False, True):
      rng = np.random.default_rng(m)
      t = EC.IC.gridded(rng, (2, nrow, nx), -2, 2)
      p = np.empty((2, m, nrow, nx), np.float32)
      p[...] = t[:, None]
      for row, names, xs in ((1, (escape, 'ordinary'), (10, 12)), (2, (escape, 'pinf_member'), (63, 0)), (4, ('ordinary', escape), (0, 63))):
        for name, x in zip(names, xs):
          p[1, :, row, x], t[1, row, x] = kinds[name][1], kinds[name][2]
      plan, dplan, mstride = _plans(ctx, p, t, False, 1, _flags('plain', fair), block=64, flat=flat)
      assert _route(plan, m, np.float32, EC.SORT) == route and plan.depth_chunk == 1
      mask = np.ones((nrow, nx), bool)
      got = _run_partial(ctx, p, t, mask, plan, dplan, mstride, EC.SORT, sentinel=-77.0)
      stat = EC.expected_lanes(fam, p, t, fair)
      want = _check_partials(got, plan, stat, EC.lane_bounds(fam, p, t, stat), mask, f'mixed tile {route} {escape} M={m} fair={fair}',
                             weights=None if flat is None else flat[1])
      assert np.isnan(want[1, 2, :NL]).all() and (got[0] == 0.0).all() and (got[1, [0, 3, 5]] == 0.0).all()
      # the pair's partials: finite and not 0 (with a +inf target: the lanes that never look at the target)
      pair = want[1, [1, 4]][:, [1, 2] if escape == 'pinf_target' else slice(0, NL)]
      assert np.isfinite(pair).all() and (pair[:, 0] > 0).all()


@pytest.mark.parametrize('block,route', [(64, 'flat'), (128, 'xf1')])
@pytest.mark.parametrize('m', M_LIVE)
def test_flat_weighted_sweeps_one_live_point_per_partial(ctx, m, block, route):
  """FLAT: two rows per chunk over planes of R = 3 rows (and R = 1, 4): the live point at a chunk's first element -- in the tile
  whose lanes in front of e0 are dropped and re-read e0 itself --, at its last element (the tail lanes behind e1 re-read it), at
  lane 0 and lane 63 of a tile: the re-read copies of a live point must be counted out.  The partial is weight x value."""
  nk = len(EC.live_points(m))
  rows = -(-nk * 2 // 12) * 12
  for shift, (nx, R) in enumerate(((24, 3), (91, 3), (64, 1), (91, 4))):
    w = _flat_weights(nx, m + shift)
    _one_live(ctx, route, m, np.float32, rows, nx, 2, False, block=block, flat=(R, w), shift=shift)


@pytest.mark.parametrize('m,dtype', [(m, np.float32) for m in M_LIVE + [65]] + [(8, np.float64)])
def test_block_kernels_one_live_point_per_partial(ctx, m, dtype):
  """s1_xr_kernel (128 threads), s1_xk_kernel and the wrappers on the same cases: with x kept every other x column of the live
  point's chunk is a partial of its own and must stay exactly 0."""
  nk = len(EC.live_points(m))
  _one_live(ctx, 'xr', m, dtype, nk * 3, 130, 3, False, block=128, shift=1)
  _one_live(ctx, 'xk', m, dtype, nk, 65, 1, True, shift=2)
  # (under skipna a NaN lane is counted out and reads 0 with count 0: the count lanes say which)
  _one_live(ctx, 'xr+masked', m, dtype, nk, 130, 1, False, mode='skipna', block=64, shift=3)
  _one_live(ctx, 'xk+masked', m, dtype, nk, 63, 1, True, mode='masked', shift=4)
  if dtype == np.float32 and m <= 64:
    _one_live(ctx, 'xr', m, dtype, nk, 65, 1, False, block=64, algo=EC.PAIRWISE, shift=5)


# ---- wbx_ens_binned (ens_atoms_kernel) -----------------------------------------------------------------------------------------
def _launch_binned(ctx, plan, dplan, p, t, m, mstride, wrow, bits, nbin, sentinel):
  nlead, nrow = p.shape[0], p.shape[2]
  n = nlead * 6 * nbin
  out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
  bufs = ctx.upload(GI._root(p)), ctx.upload(GI._root(t)), ctx.upload(np.asarray(wrow, np.float64)), ctx.upload(bits)  # pylint: disable=protected-access
  rc = R4._raw_call(ctx, plan, dplan, m, mstride, bufs[0], bufs[1], None, bufs[2], bufs[3], nlead, 1, nrow,  # pylint: disable=protected-access
                    _hip.BINNED_W_ON_X | _hip.BINNED_WT_ROW_ONLY, nbin, None, out)
  return rc, ctx.download(out.ptr, (nlead, 6, nbin), np.float64)


def _binned(ctx, p, t, wrow, nbin_x, fair, m=None, sentinel=None):
  """One raw wbx_ens_binned launch on p[lead, member, row, x]: bins = disjoint runs of `nbin_x` consecutive x, weights per row
  -> (rc, out[lead][6][nbin], member[x, bin])."""
  nlead, mm, nrow, nx = p.shape
  sizes = {LEAD: nlead, ROW: nrow, X: nx}
  lay_p, mstride = GI._layout(p, GI.PD)  # pylint: disable=protected-access
  lay_t, _ = GI._layout(t, GI.SDIMS)  # pylint: disable=protected-access
  plan = planner.build_s1_plan(GI.SDIMS, sizes, [lay_p, lay_t, None, None], (ROW, X), wdep_dims={ROW, X}, flags=_hip.FLAG_FAIR if fair else 0,
                               allow_vec4=False, force_x_dim=X)
  assert plan.a_dims == (LEAD,) and plan.br_dims == (ROW,) and plan.x_dim == X
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  nbin = -(-nx // nbin_x)
  member = (np.arange(nx)[:, None] // nbin_x) == np.arange(nbin)[None, :]
  bits = np.ascontiguousarray(np.broadcast_to((np.uint64(1) << (np.arange(nx) // nbin_x).astype(np.uint64))[None, :], (nrow, nx)))
  rc, out = _launch_binned(ctx, plan, dplan, p, t, mm if m is None else m, mstride, wrow, bits, nbin, sentinel)
  return rc, out, member.astype(np.float64)


def _check_binned(got, stat, bound, wrow, member, what):
  """out[lead][lane][bin] = sum over rows and x of value x weight x membership (0.0 / 1.0: NaN x 0 = NaN, so a non-finite value
  reaches every bin of its lead and lane, like the reference's xr.dot); lane 5 = the sum of the weights of the bin's points."""
  with np.errstate(invalid='ignore'):
    want = np.einsum('ayxl,y,xb->alb', stat, wrow, member)
    fin = np.isfinite(stat)
    b = np.einsum('ayxl,y,xb->alb', np.where(fin, bound, 0.0), wrow, member)
    s = np.einsum('ayxl,y,xb->alb', np.where(fin, np.abs(stat), 0.0), wrow, member)
  cnt = np.einsum('y,xb->b', wrow, member)
  np.testing.assert_array_equal(got[:, 5], np.broadcast_to(cnt, got[:, 5].shape), err_msg=f'{what}: count lane')
  n = stat.shape[1] * int(member.sum(axis=0).max())
  # lane 3 is formed per (patch, bin) as lane 4 - lane 2 / M from the sums: the bounds of both, which is lane 3's own row
  _assert_within(got[:, :NL], want, b + (n + 2) * EPS * s, what)
  return want


def _binned_inputs(m):
  fam = EC.family('binned', m, np.float32)
  # (rows of 130: the ragged-row flavour, four waves per block; rows of 64: whole cache lines, one wave per block)
  for i, (nrow, nx, nbin_x, layout) in enumerate(((5, 130, 8, 'member_outside'), (7, 64, 5, 'ifs'))):
    for j, vals in enumerate(VALUES):
      p, t, _ = EC.dense_case(700 * m + 10 * i + j, m, 2, nrow, nx, values=vals, layout=layout)
      yield nx, nbin_x, vals, EC.fair_of(m, i + j), fam, p, t, np.random.default_rng(i).integers(1, 17, size=nrow) / 8.0


@pytest.mark.parametrize('m', EC.M_BINNED)
def test_binned_dense_every_bin(ctx, m):
  """ens_atoms_kernel: the arithmetic of wbx_ens_partial for the same M (fp32 chains at 50 / 51, stats64 in the buckets), bins of
  8 and 5 consecutive x over rows of 130 and 64, dyadic row weights."""
  for nx, nbin_x, vals, fair, fam, p, t, wrow in _binned_inputs(m):
    rc, got, member = _binned(ctx, p, t, wrow, nbin_x, fair)
    _hip.check(rc, 'wbx_ens_binned')
    stat = EC.expected_lanes(fam, p, t, fair)
    want = _check_binned(got, stat, EC.lane_bounds(fam, p, t, stat), wrow, member, f'binned {nx} {vals} M={m} fair={fair}')
    assert np.isfinite(want).all()


@pytest.mark.parametrize('m', EC.M_BINNED)
def test_binned_one_live_point_per_bin(ctx, m):
  """Every second bin of a lead holds one live point, the others none: their value lanes are exactly 0 and their count lane the
  sum of the weights.  A lead of its own for every kind that is not finite: it turns that lane NaN in every bin of its lead
  (NaN x 0) and leaves the other leads alone."""
  fam = EC.family('binned', m, np.float32)
  kinds = EC.live_points(m)
  nrow, nx, nbin_x = 5, 130, 8
  nbin = -(-nx // nbin_x)
  fair = EC.fair_of(m)
  probe = np.stack([EC.expected_lanes(fam, k[1][None, :, None, None], np.array(k[2], np.float32).reshape(1, 1, 1), fair)[0, 0, 0] for k in kinds])
  finite = [k for k, v in zip(kinds, probe) if np.isfinite(v).all()]
  others = [k for k, v in zip(kinds, probe) if not np.isfinite(v).all()]
  nlead = -(-len(finite) // (nbin // 2)) + len(others)
  rng = np.random.default_rng(m)
  t = EC.IC.gridded(rng, (nlead, nrow, nx), -2, 2)
  p = np.empty((nlead, m, nrow, nx), np.float32)
  p[...] = t[:, None]
  live = np.zeros(t.shape, bool)
  for k, kind in enumerate(finite):
    lead, b = divmod(k, nbin // 2)
    row, x = (k * 3) % nrow, min(2 * b * nbin_x + (k % nbin_x), nx - 1)
    p[lead, :, row, x], t[lead, row, x], live[lead, row, x] = kind[1], kind[2], True
  for k, kind in enumerate(others):
    lead = nlead - len(others) + k
    row, x = k % nrow, (37 * k + 63) % nx
    p[lead, :, row, x], t[lead, row, x], live[lead, row, x] = kind[1], kind[2], True
  wrow = rng.integers(1, 17, size=nrow) / 8.0
  rc, got, member = _binned(ctx, p, t, wrow, nbin_x, fair, sentinel=-77.0)
  _hip.check(rc, 'wbx_ens_binned')
  stat = EC.expected_lanes(fam, p, t, fair)
  assert (stat[~live] == 0.0).all()
  want = _check_binned(got, stat, EC.lane_bounds(fam, p, t, stat), wrow, member, f'binned one live point M={m}')
  has_live = np.einsum('ayx,xb->ab', live.astype(np.float64), member) > 0
  quiet = ~has_live[:, None, :] & np.isfinite(want)
  assert (~has_live).sum() >= 2 and has_live.sum() >= 2
  assert (got[:, :NL][quiet] == 0.0).all(), 'a bin without a live point is not 0'


@pytest.mark.parametrize('m', [50, 51])
def test_binned_escape_and_ordinary_point_in_one_tile(ctx, m):
  """ens_atoms_kernel's tile is 64 consecutive x of one row and spans eight bins of 8: the escape point, the ordinary point and
  the infinite-member point of one tile sit in bins of their own, so each is held PER POINT -- the ordinary point redone in
  fp64 with its tile within its bound, every other bin of the lead exactly 0.  A value that is not finite reaches every bin of
  its lead and lane (NaN x 0): a +inf target leaves only lanes 1 and 2 per bin, and the infinite member in an escaping tile
  must turn all five lanes of every bin of its lead NaN (a poison lost in the redo would leave +inf in its own bin) and no
  other lead.  First and second x tile of rows of 130, and whole rows of 64."""
  fam = EC.family('binned', m, np.float32)
  kinds = {k[0]: k for k in EC.live_points(m)}
  nbin_x = 8
  for nrow, nx, x0 in ((5, 130, 0), (5, 130, 64), (3, 64, 0)):
    fair = EC.fair_of(m, x0 // 64)
    nlead = 2 * len(ESCAPES) + 1
    rng = np.random.default_rng(m + nx)
    t = EC.IC.gridded(rng, (nlead, nrow, nx), -2, 2)
    p = np.empty((nlead, m, nrow, nx), np.float32)
    p[...] = t[:, None]
    for k, escape in enumerate(ESCAPES):
      for lead, row, names, xs in ((2 * k, 1, (escape, 'ordinary'), (3, 17)), (2 * k + 1, 2, (escape, 'pinf_member', 'ordinary'), (60, 33, 10))):
        for name, x in zip(names, xs):
          p[lead, :, row, x0 + x], t[lead, row, x0 + x] = kinds[name][1], kinds[name][2]
    wrow = rng.integers(1, 17, size=nrow) / 8.0
    rc, got, member = _binned(ctx, p, t, wrow, nbin_x, fair, sentinel=-77.0)
    _hip.check(rc, 'wbx_ens_binned')
    stat = EC.expected_lanes(fam, p, t, fair)
    want = _check_binned(got, stat, EC.lane_bounds(fam, p, t, stat), wrow, member, f'binned mixed tile M={m} nx={nx} x0={x0}')
    b0 = x0 // nbin_x
    for k, escape in enumerate(ESCAPES):
      lanes = [1, 2] if escape == 'pinf_target' else list(range(NL))
      pair = want[2 * k][lanes]
      assert np.isfinite(pair).all() and (pair[0, [b0, b0 + 2]] > 0).all(), escape
      quiet = np.ones(pair.shape[1], bool)
      quiet[[b0, b0 + 2]] = False
      assert (got[2 * k][lanes][:, quiet] == 0.0).all(), (escape, 'a bin without a live point is not 0')
      assert np.isnan(want[2 * k + 1, :NL]).all(), escape
    assert (got[nlead - 1, :NL] == 0.0).all()


def test_binned_refuses_more_members_than_the_registers_hold(ctx):
  """M = 65: WBX_ERR_INVALID with a message, the output untouched."""
  p, t, _ = EC.dense_case(1, 65, 1, 3, 64)
  rc, got, _ = _binned(ctx, p, t, np.ones(3), 8, True, sentinel=-77.0)
  assert rc == -1 and '2..64 members' in ctx.lib.wbx_last_error().decode(), (rc, ctx.lib.wbx_last_error())
  assert (got == -77.0).all()
  rc, got, _ = _binned(ctx, p, t, np.ones(3), 8, True, m=1, sentinel=-77.0)
  assert rc == -1 and (got == -77.0).all()


# ---- WBX_FLAG_SKIPNA_ENS: what is new for it -------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', EC.M_SKIPNA_ENS_EDGES)
def test_skipna_ensemble_at_the_register_bucket_edges(ctx, m):
  """The per-point test of the skipna_ensemble register kernel (tests/test_gpu_round4.py: points without a member, with one, with
  two, with all, an infinite member, a NaN and an infinite target; every lane per point on wbx_ens_map) at both sides of every
  padded bucket's edge, where the padding behind the M members and the per-lane member count meet."""
  R4.test_skipna_ensemble_register_kernel_against_the_oracle(ctx, m)
