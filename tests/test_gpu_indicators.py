"""The indicator kernels (s1_cat_kernel: RankHistogram, EnsembleErrorExceedance, ErrorExceedance -- wbx_cat_partial,
wbx_cat_exceed_field) and the two-ensemble kernel (Ens2Op -- wbx_ens2_partial) through the raw C ABI, at the member counts,
row lengths, threshold counts and edges that run: EVERY partial `partial[key][chunk][lane]` (and `[..][x]` with x kept) against
the float64 oracle, so nothing hides in a mean.  Inputs: tests/indicator_cases.py (dyadic values: ties are real ties).

Tolerances (none of them fitted to what the kernels give):
  * rank-histogram partials and every count lane are sums of 0 / 1 in fp64 of fewer than 2^53 terms: bit-equal;
  * exceedance partials: a point's value is cnt * (1 / n) against the oracle's cnt / n (at most 1 ulp apart), then N
    non-negative terms are added in an order that is not the oracle's: (N + 2) * 2^-52 relative, N = points of the partial
    (2 ulp where a partial is a single point);
  * two-ensemble lane 0 (non-negative terms, fp64): rtol 1e-9 (tests/test_gpu_round3.py gives the fp64 ops the same); lane 1 is a
    difference: |d| <= 1e-9 * sum over the partial's points of (md^2 + var_p / n_p + var_t / n_t), the form include/wbx.h uses.
NaN outputs (plain mode: a NaN statistic poisons its partial) must be NaN on both sides at the same positions, and at least
80 % of a plain-mode case's outputs are finite; under skipna every output is finite."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import wbx_oracle as O
from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import indicator_cases as IC

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
MODES = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA, 'masked+skipna': _hip.FLAG_MASKED | _hip.FLAG_SKIPNA}
LEAD, MEMBER, ROW, X = 'lead_time', 'number', 'row', 'x'
SDIMS = (LEAD, ROW, X)


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


# ---- plumbing: named views of contiguous arrays -> plan -> launch -> [key][chunk][lane][j] ------------------------------------
def _root(a):
  """The contiguous array `a` is a (transposed) view of; `a` must start at its first element."""
  r = a
  while r.base is not None:
    r = r.base
  assert r.flags.c_contiguous and r.__array_interface__['data'][0] == a.__array_interface__['data'][0]
  return r


def _layout(a, dims):
  lay = planner.layout_of(a, dims)
  return planner.InputLayout(strides={d: s for d, s in lay.strides.items() if d != MEMBER}, itemsize=lay.itemsize,
                             base_alignment=256), lay.strides.get(MEMBER, 0)


def _plan(ctx, sizes, layouts, x_kept, depth_chunk, flags):
  """The statistic's frame is (lead_time, row, x); rows are reduced, x is summed or kept; `depth_chunk` rows per partial
  (None: all of them)."""
  reduce_dims = (ROW,) if x_kept else (ROW, X)
  plan = planner.build_s1_plan(SDIMS, sizes, layouts, reduce_dims, wdep_dims=set(), flags=flags, allow_vec4=False, force_x_dim=X)
  dc = plan.ndepth if depth_chunk is None else min(depth_chunk, plan.ndepth)
  plan = dataclasses.replace(plan, depth_chunk=dc, nchunk=-(-plan.ndepth // dc))
  assert plan.x_kept == x_kept and plan.a_dims == (LEAD,) and plan.depth_dims == (ROW,) and not plan.bk_dims and not plan.br_dims, plan
  return plan, engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access


def _ptr(buf):
  return None if buf is None else C.c_void_p(buf.ptr)


def _lanes_total(nl, flags):
  return 2 * nl if flags & _hip.FLAG_SKIPNA else (nl + 1 if flags & _hip.FLAG_MASKED else nl)


def _expected_partials(plan, stat, valid, flags):
  """stat[lead, row, x, lane] (float64, NaN where the statistic is NaN), valid[row, x] or None -> what stage 1 writes,
  [lead][chunk][lane][j]: the value lanes, then the count lanes (one shared under a mask alone, one per lane under skipna)."""
  ok = np.ones(stat.shape, bool) if valid is None or not (flags & _hip.FLAG_MASKED) else np.broadcast_to(valid[None, :, :, None], stat.shape)
  if flags & _hip.FLAG_SKIPNA:
    ok = ok & ~np.isnan(stat)
    lanes = np.concatenate([np.where(ok, stat, 0.0), ok.astype(np.float64)], axis=-1)
  elif flags & _hip.FLAG_MASKED:
    lanes = np.concatenate([np.where(ok, stat, 0.0), ok[..., :1].astype(np.float64)], axis=-1)
  else:
    lanes = stat
  nlead, nrow, nx, nl = lanes.shape
  pad = plan.nchunk * plan.depth_chunk - nrow
  a = np.pad(lanes, ((0, 0), (0, pad), (0, 0), (0, 0))).reshape(nlead, plan.nchunk, plan.depth_chunk, nx, nl)
  out = a.sum(axis=2) if plan.x_kept else a.sum(axis=(2, 3))[:, :, None, :]  # [lead, chunk, j, lane]
  return np.ascontiguousarray(np.moveaxis(out, -1, 2))


def _points_per_partial(plan):
  return plan.depth_chunk * (1 if plan.x_kept else plan.nx)


def _check_nan_pattern(got, want, flags, what, lanes=None):
  """NaN at the same positions on both sides; under skipna nowhere (NaN statistics are counted out), else on at most 20 % of
  the outputs of `lanes` (default: all value lanes; a NaN threshold's lane is NaN at every valid point by definition)."""
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{what}: NaN positions')
  if flags & _hip.FLAG_SKIPNA:
    assert np.isfinite(want).all(), what
  else:
    share = float(np.isfinite(want if lanes is None else want[:, :, lanes]).mean())
    assert share >= 0.8, (what, 'finite share', share)


def _check_counts(got, want, nl, flags, what):
  if flags & (_hip.FLAG_MASKED | _hip.FLAG_SKIPNA):
    np.testing.assert_array_equal(got[:, :, nl:], want[:, :, nl:], err_msg=f'{what}: count lanes')


def _check_sums_of_fractions(got, want, nl, n_points, what):
  g, w = got[:, :, :nl], want[:, :, :nl]
  fin = np.isfinite(w)
  err = np.abs(g[fin] - w[fin])
  # (a partial of ONE point -- x kept, one row -- is the point's own value: 2 ulp)
  bound = (n_points + 2) * EPS * np.abs(w[fin]) if n_points > 1 else 2 * np.spacing(np.abs(w[fin]))
  worst = float((err / np.maximum(np.abs(w[fin]), 1e-300)).max()) if err.size else 0.0
  assert (err <= bound).all(), (what, 'worst relative error', worst, 'bound', (n_points + 2) * EPS)


def _poison_rows(mode, nrow, nx, x_kept, depth_chunk):
  """-> (rows that carry the special points, those of them whose NaN points may be VALID).  Every 7th row carries them.  A valid
  NaN statistic poisons its whole partial unless skipna counts it out, so without skipna valid NaN points only go where at
  least 80 % of the outputs stay finite: one row per partial, or x kept on rows long enough.  Plain mode (no mask to hide
  them): the other rows carry no special points at all; under a mask they carry them hidden."""
  rows = tuple(range(0, nrow, 7))
  if 'skipna' in mode:
    return rows, rows
  if x_kept:
    exposed = rows if nx >= 63 else ()
  else:
    exposed = rows if depth_chunk == 1 else ()
  return (exposed if mode == 'plain' else rows), exposed


def _run_cat(ctx, func, p, t, mask, thr, x_kept, depth_chunk, flags, field=None, sentinel=None):
  """One wbx_cat_partial / wbx_cat_exceed_field launch on p[lead, member, row, x] (any strides), t[lead, row, x], mask[row, x];
  field = (float64 array, {dim: element stride}, category stride, ncat) -> (rc, plan, partial[lead][chunk][lane][j])."""
  nlead, m, nrow, nx = p.shape
  sizes = {LEAD: nlead, ROW: nrow, X: nx}
  lay_p, mstride = _layout(p, PD)
  lay_t, _ = _layout(t, SDIMS)
  lay_m = lay_f = mask_buf = fbuf = None
  if flags & _hip.FLAG_MASKED:
    lay_m = planner.InputLayout(strides={ROW: nx, X: 1}, itemsize=1, base_alignment=256)
    mask_buf = ctx.upload(np.ascontiguousarray(mask, np.uint8))
  if field is not None:
    lay_f = planner.InputLayout(strides=field[1], itemsize=8, base_alignment=256)
    fbuf = ctx.upload(field[0])
  plan, dplan = _plan(ctx, sizes, [lay_p, lay_t, lay_f, lay_m], x_kept, depth_chunk, flags)
  ncat = m + 1 if func == _hip.CAT_RANK else (len(thr) if field is None else field[3])
  shape = (nlead, plan.nchunk, _lanes_total(ncat, flags), plan.nj)
  n = int(np.prod(shape))
  dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  out = ctx.upload(np.full(n, sentinel, np.float64)) if sentinel is not None else ctx.alloc(n * 8)
  bufs = ctx.upload(_root(p)), ctx.upload(_root(t))
  if field is not None:
    rc = ctx.lib.wbx_cat_exceed_field(ctx.handle, C.byref(dplan.struct), dtype_code, ncat, m, mstride, _ptr(bufs[0]), _ptr(bufs[1]),
                                      _ptr(fbuf), field[2], _ptr(mask_buf), _ptr(out))
  else:
    tbuf = ctx.upload(np.asarray(thr, np.float64)) if thr is not None else None
    rc = ctx.lib.wbx_cat_partial(ctx.handle, C.byref(dplan.struct), func, dtype_code, ncat, m, mstride, _ptr(bufs[0]), _ptr(bufs[1]),
                                 _ptr(tbuf), _ptr(mask_buf), _ptr(out))
  return rc, plan, ctx.download(out.ptr, shape, np.float64)


PD = (LEAD, MEMBER, ROW, X)


def _in_row_slabs(fn, p, t, lanes):
  """fn on slabs of rows, so that no temporary of the oracle ([lead, rows, x, member, lane] float64) passes ~0.5 GB."""
  per_row = p.shape[0] * t.shape[2] * p.shape[1] * lanes * 8
  slab = max(1, int(5e8 // per_row))
  with np.errstate(invalid='ignore'):  # (inf - inf at the special points)
    return np.concatenate([fn(p[:, :, r:r + slab], t[:, r:r + slab]) for r in range(0, t.shape[1], slab)], axis=1)


def _oracle_rank(p, t):
  """[lead, row, x, M + 1]"""
  return _in_row_slabs(lambda pp, tt: O.rank_histogram(pp, PD, tt, SDIMS, MEMBER)[0], p, t, 2)


def _oracle_exceed(p, t, thr):
  """[lead, row, x, len(thr)]"""
  return _in_row_slabs(lambda pp, tt: O.ensemble_error_exceedance(pp, PD, tt, SDIMS, thr, MEMBER)[0], p, t, len(thr))


def _compare_cat(ctx, func, p, t, mask, thr, x_kept, depth_chunk, mode, what, stat=None):
  flags = MODES[mode]
  rc, plan, got = _run_cat(ctx, func, p, t, mask, thr, x_kept, depth_chunk, flags)
  _hip.check(rc, what)
  if func == _hip.CAT_RANK:
    stat = _oracle_rank(p, t) if stat is None else stat
    want = _expected_partials(plan, stat, mask, flags)
    assert not np.isnan(want).any()
    np.testing.assert_array_equal(got, want, err_msg=what)  # counts of 0 / 1 in fp64: every lane, every partial, bit for bit
    return
  stat = _oracle_exceed(p, t, thr) if stat is None else stat
  want = _expected_partials(plan, stat, mask, flags)
  _check_nan_pattern(got, want, flags, what, lanes=np.flatnonzero(~np.isnan(thr)))
  _check_counts(got, want, len(thr), flags, what)
  _check_sums_of_fractions(got, want, len(thr), _points_per_partial(plan), what)


def _case(seed, m, nlead, nrow, nx, mode, x_kept, dc, **kw):
  poison, exposed = _poison_rows(mode, nrow, nx, x_kept, dc)
  return IC.indicator_case(seed, m, nlead, nrow, nx, poison_rows=poison, exposed_rows=exposed, **kw)


# (name, leads, rows, x, x kept, rows per partial (None: all), member layout).  1440 and 181 / 91 are the row lengths of the
# 0.25 and 1 / 2 degree grids, longitude- and latitude-fastest: 181 and 91 put a row's end inside a 64-lane tile.  (Whole grids:
# test_whole_grids_every_rank_bin; a few rows of each length here, so that the whole list of member counts runs in seconds.)
GRIDS = [
    ('x1440-summed-1row', 2, 14, 1440, False, 1, 'member_outside'),
    ('x1440-summed-all', 2, 5, 1440, False, None, 'ifs'),
    ('x1440-kept-3rows', 2, 7, 1440, True, 3, 'ifs'),
    ('x181-summed-3rows', 2, 22, 181, False, 3, 'ifs'),
    ('x181-kept-all', 2, 22, 181, True, None, 'member_outside'),
    ('x91-summed-1row', 2, 21, 91, False, 1, 'member_outside'),
    ('x91-kept-1row', 2, 15, 91, True, 1, 'ifs'),
    ('x1-summed-3rows', 2, 19, 1, False, 3, 'member_outside'),
    ('x63-kept-1row', 2, 19, 63, True, 1, 'ifs'),
    ('x64-summed-all', 2, 19, 64, False, None, 'member_outside'),
    ('x65-kept-3rows', 2, 19, 65, True, 3, 'member_outside'),
    ('x130-summed-1row', 2, 19, 130, False, 1, 'ifs'),
]
THR5 = np.array([0.25, -0.25, np.nan, 1.0, np.inf])  # ties at 0.25 and 1.0; a negative, a NaN and an infinite threshold
M_CASES = [(m, np.float32) for m in (1, 2, 8, 9, 49, 50, 51, 52, 64, 65, 100)] + [(8, np.float64), (51, np.float64)]


@pytest.mark.parametrize('mode', ['plain', 'masked', 'skipna'])
@pytest.mark.parametrize('m,dtype', M_CASES, ids=[f'M{m}-{np.dtype(d).name}' for m, d in M_CASES])
def test_rank_histogram_and_exceedance_every_partial(ctx, m, dtype, mode):
  """Fixed (MF = 50, 51) and generic member loops, the sizes around them and around the 64-member register buckets, M = 100
  above them; NaN / infinite / -0.0 members, ties p_m == t and |p_m - t| == thr, all-NaN points, a single valid member,
  inf - inf, NaN targets under a mask that hides them and one that does not; both member layouts; x summed and kept; 1, 3 and
  all rows per partial."""
  for i, (name, nlead, nrow, nx, x_kept, dc, layout) in enumerate(GRIDS):
    p, t, mask = _case(1000 * m + i, m, nlead, nrow, nx, mode, x_kept, dc, dtype=dtype, layout=layout)
    for func in (_hip.CAT_RANK, _hip.CAT_EXCEED):
      _compare_cat(ctx, func, p, t, mask, THR5, x_kept, dc, mode, f'{name} M={m} {mode} func={func}')


@pytest.mark.parametrize('layout,nrow,nx', [('lon_fastest', 91, 1440), ('lat_fastest', 360, 181)])
@pytest.mark.parametrize('m', [50, 51, 100])
def test_whole_grids_every_rank_bin(ctx, m, layout, nrow, nx):
  """[2 leads, M, 91, 1440] (longitude fastest) and [2, M, 360, 181] (latitude fastest, the IFS member layout): every rank
  bin is filled (a wrong column index for any rank shows) and every row's partial is compared, x summed and x kept."""
  rows = tuple(range(0, nrow, 7))
  p, t, mask = IC.indicator_case(7 * m + nx, m, 2, nrow, nx, poison_rows=rows, layout='ifs' if layout == 'lat_fastest' else 'member_outside',
                                   t_range=(-3.25, 3.25))  # (targets below and above every member: ranks 0 .. M)
  rank = _oracle_rank(p, t)
  assert (rank.sum(axis=(0, 1, 2)) > 0).all()  # every one of the M + 1 bins occurs
  thr = THR5[[0, 2, 3]]
  exceed = _oracle_exceed(p, t, thr)
  for x_kept, dc in ((False, 1), (True, None)):
    _compare_cat(ctx, _hip.CAT_RANK, p, t, mask, None, x_kept, dc, 'masked', f'{layout} rank x_kept={x_kept}', stat=rank)
    _compare_cat(ctx, _hip.CAT_EXCEED, p, t, mask, thr, x_kept, dc, 'masked+skipna', f'{layout} exceed x_kept={x_kept}', stat=exceed)


def _ncat_cases():
  out = []
  for m in (51, 5, 1):
    for mode, top in (('plain', 128), ('masked', 127), ('skipna', 64), ('masked+skipna', 64)):
      for ncat in (1, 7, 8, 9, 16, 17, 40, 64, 127, 128):
        if ncat <= top and (ncat != 127 or mode == 'masked'):
          out.append((m, mode, ncat))
  return out


@pytest.mark.parametrize('m,mode,ncat', _ncat_cases())
def test_threshold_count_blocks_of_eight(ctx, m, mode, ncat):
  """The exceedance loop walks the thresholds in blocks of 8: one block, a full block, a tail of one, several blocks, and the
  most one launch holds -- 128 lanes of fp64 columns = 65 536 bytes of dynamic LDS exactly (128 thresholds plain, 127 + the
  shared count lane under a mask, 64 + 64 under skipna).  One threshold is NaN, one negative, one +inf; M = 1 is the
  deterministic ErrorExceedance."""
  thr = IC.thresholds(ncat)
  nrow = 7
  for x_kept, dc, nx in ((False, 1, 130), (True, None, 65)):
    p, t, mask = _case(31 * ncat + m, m, 2, nrow, nx, mode, x_kept, dc)
    _compare_cat(ctx, _hip.CAT_EXCEED, p, t, mask, thr, x_kept, dc, mode, f'ncat={ncat} M={m} {mode} x_kept={x_kept}')


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('m', [1, 51])
@pytest.mark.parametrize('ncat', [1, 9, 17])
def test_threshold_fields_with_their_own_strides(ctx, ncat, m, dtype, mode):
  """wbx_cat_exceed_field: thresholds per (lead, row), stored [row][category][lead] -- row-major, with strides of their own along
  every dim and broadcast along x.  A NaN threshold under valid points (row 3: it poisons that lane of that row, or is counted
  out of it) and, where there is a mask, under points the mask hides (row 4: no trace)."""
  nlead, nrow, nx = 2, 19, 130
  rng = np.random.default_rng(5 * ncat + m)
  flags = MODES[mode]
  for x_kept, dc in ((False, 1), (True, 3)):
    p, t, mask = _case(77 * ncat + m, m, nlead, nrow, nx, mode, x_kept, dc, dtype=dtype)
    field = IC.gridded(rng, (nrow, ncat, nlead), 0, 3, dtype=np.float64)
    mask[3, :], mask[4, :] = True, False
    field[3, ncat // 2, 0] = np.nan
    if flags & _hip.FLAG_MASKED:
      field[4, 0, 1] = np.nan
    rc, plan, got = _run_cat(ctx, _hip.CAT_EXCEED, p, t, mask, None, x_kept, dc, flags,
                             field=(field, {ROW: ncat * nlead, LEAD: 1}, nlead, ncat))
    what = f'field ncat={ncat} M={m} {mode} x_kept={x_kept}'
    _hip.check(rc, what)
    stat = np.empty((nlead, nrow, nx, ncat))
    for lead in range(nlead):  # per (lead, row) its own thresholds: the oracle with constant thresholds, row by row
      for r in range(nrow):
        with np.errstate(invalid='ignore'):
          stat[lead, r] = O.ensemble_error_exceedance(p[lead:lead + 1, :, r:r + 1], PD, t[lead:lead + 1, r:r + 1], SDIMS,
                                                      field[r, :, lead], MEMBER)[0][0, 0]
    want = _expected_partials(plan, stat, mask, flags)
    _check_nan_pattern(got, want, flags, what, lanes=np.arange(ncat))
    _check_counts(got, want, ncat, flags, what)
    _check_sums_of_fractions(got, want, ncat, _points_per_partial(plan), what)


@pytest.mark.parametrize('func,m,ncat', [(_hip.CAT_EXCEED, 5, 65), (_hip.CAT_RANK, 128, 129)])
def test_more_lanes_than_the_lds_columns_hold_is_refused(ctx, func, m, ncat):
  """65 thresholds under skipna = 130 fp64 columns, a rank histogram of 128 members under skipna = 258 uint32 columns: more
  than 64 KB of LDS.  WBX_ERR_INVALID with a message in front of any launch, the output untouched.  One lane fewer is the
  exact fit, and runs."""
  p, t, mask = IC.indicator_case(3, m, 1, 3, 65)
  thr = IC.thresholds(ncat) if func == _hip.CAT_EXCEED else None
  rc, _, got = _run_cat(ctx, func, p, t, mask, thr, False, None, _hip.FLAG_SKIPNA, sentinel=-77.0)
  assert rc == -1 and 'too many categories' in ctx.lib.wbx_last_error().decode(), (rc, ctx.lib.wbx_last_error())
  assert (got == -77.0).all()
  p, t, mask = IC.indicator_case(3, m - (func == _hip.CAT_RANK), 1, 3, 65)
  _compare_cat(ctx, func, p, t, mask, None if thr is None else thr[:64], False, None, 'skipna', 'exact fit')


# ---- two ensembles: wbx_ens2_partial -------------------------------------------------------------------------------------------
TD = (LEAD, ROW, X, MEMBER)  # targets are stored member-fastest: a member stride of 1 against the predictions' rows * x


def _ens2_nan_rows(mode, skip, nans, m, n, x_kept):
  """Rows that may carry NaN members (None: all).  A NaN statistic -- any NaN member without skipna_ensemble; with it a side
  without a member (lane 0) or with fewer than two (lane 1) -- poisons its partial unless the aggregator's skipna counts it
  out.  Without that NaNs go where at least 80 % of the outputs stay finite: everywhere if the 15 % share practically never
  empties a side, else into one row of seven with x summed (one row per partial), nowhere with x kept."""
  if 'skipna' in mode:
    return None
  if skip and nans == 'some' and min(m, n) >= (4 if x_kept else 10):
    return None
  return () if x_kept else (0,)


def _ens2_case(seed, m, n, nlead, nrow, nx, dtype, nans, tight=False, nan_rows=None):
  """p[lead, member, row, x], t[lead, row, x, member].  nans: 'none', 'some' (15 % of the members of each side) or 'single'
  (the points of a row keep a single valid member on the prediction side -- its variance is NaN by ddof = 1 -- or, on every
  other such row, on the target side).  NaNs only go into `nan_rows` (None: every row)."""
  rng = np.random.default_rng(seed)
  if tight:  # geopotential-like: 5.5e4 +- 30
    c = rng.normal(size=(nlead, 1, nrow, nx)) * 300 + 5.5e4
    p = (c + rng.normal(size=(nlead, m, nrow, nx)) * 30).astype(dtype)
    t = (np.moveaxis(c, 1, -1) + rng.normal(size=(nlead, nrow, nx, n)) * 30).astype(dtype)
  else:
    p = IC.gridded(rng, (nlead, m, nrow, nx), -3, 3, dtype=dtype)
    t = IC.gridded(rng, (nlead, nrow, nx, n), -2, 2, dtype=dtype)
  rows = np.arange(nrow) if nan_rows is None else np.asarray(nan_rows, int)
  if nans == 'some' and rows.size:
    p[:, :, rows] = np.where(rng.random(p[:, :, rows].shape) < 0.15, np.nan, p[:, :, rows])
    t[:, rows] = np.where(rng.random(t[:, rows].shape) < 0.15, np.nan, t[:, rows])
  elif nans == 'single':
    for i, r in enumerate(rows):
      if i % 2 == 0:
        p[:, :m - 1, r] = np.nan
      else:
        t[:, r, :, 1:] = np.nan
  mask = rng.random((nrow, nx)) > 0.3
  return p, t, mask


def _run_ens2(ctx, p, t, mask, x_kept, depth_chunk, flags, reverse_targets=False, target_stride=None):
  nlead, m, nrow, nx = p.shape
  n = t.shape[-1]
  sizes = {LEAD: nlead, ROW: nrow, X: nx}
  lay_p, mstride = _layout(p, PD)
  lay_t, tstride = _layout(t, TD)
  lay_m = mask_buf = None
  if flags & _hip.FLAG_MASKED:
    lay_m = planner.InputLayout(strides={ROW: nx, X: 1}, itemsize=1, base_alignment=256)
    mask_buf = ctx.upload(np.ascontiguousarray(mask, np.uint8))
  plan, dplan = _plan(ctx, sizes, [lay_p, lay_t, None, lay_m], x_kept, depth_chunk, flags)
  shape = (nlead, plan.nchunk, _lanes_total(_hip.ENS2_LANES, flags), plan.nj)
  out = ctx.alloc(int(np.prod(shape)) * 8)
  bufs = ctx.upload(_root(p)), ctx.upload(_root(t))
  dtype_code = _hip.F32 if p.dtype == np.float32 else _hip.F64
  tptr = bufs[1].ptr
  if reverse_targets:  # the same members walked from the last one down: a negative member stride
    tptr, tstride = tptr + (n - 1) * tstride * t.dtype.itemsize, -tstride
  if target_stride is not None:
    tstride = target_stride
  _hip.check(ctx.lib.wbx_ens2_partial(ctx.handle, C.byref(dplan.struct), dtype_code, m, mstride, n, tstride, _ptr(bufs[0]),
                                      C.c_void_p(tptr), _ptr(mask_buf), _ptr(out)), 'wbx_ens2_partial')
  return plan, ctx.download(out.ptr, shape, np.float64)


def _ens2_oracle(p, t, skip):
  """(stat[lead, row, x, 2], scale[lead, row, x]): the two lanes and lane 1's scale md^2 + var_p / n_p + var_t / n_t."""
  with np.errstate(all='ignore'):
    skill, d0 = O.crps_skill(p, PD, t, TD, MEMBER, skipna_ensemble=skip)
    uemse, d1 = O.unbiased_ensemble_mean_squared_error(p, PD, t, TD, MEMBER, skipna_ensemble=skip)
    assert d0 == SDIMS and d1 == SDIMS
    pm, pb, _ = O._ensemble_moments(p, PD, MEMBER, skip)  # pylint: disable=protected-access
    tm, tb, _ = O._ensemble_moments(t, TD, MEMBER, skip)  # pylint: disable=protected-access
    scale = (pm - tm) ** 2 + pb + tb
  if not skip:  # skipna=False: a NaN member on either side makes the point NaN (both lanes: the kernel's `poison`)
    bad = np.isnan(p).any(axis=1) | np.isnan(t).any(axis=-1)
    assert np.isnan(skill[bad]).all() and np.isnan(uemse[bad]).all()
  return np.stack([skill, uemse], axis=-1), scale


def _compare_ens2(ctx, p, t, mask, x_kept, dc, mode, skip, what, reverse_targets=False, target_stride=None):
  flags = MODES[mode] | (_hip.FLAG_SKIPNA_ENS if skip else 0)
  plan, got = _run_ens2(ctx, p, t, mask, x_kept, dc, flags, reverse_targets, target_stride)
  stat, scale = _ens2_oracle(p, t, skip)
  want = _expected_partials(plan, stat, mask, flags)
  m, n = p.shape[1], t.shape[-1]
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{what}: NaN positions')
  if 'skipna' in mode:
    assert np.isfinite(want).all(), what
  else:  # (fewer than two members on a side: lane 1 is NaN at every point by definition, ddof = 1)
    for l in ((0, 1) if min(m, n) >= 2 else (0,)):
      assert np.isfinite(want[:, :, l]).mean() >= 0.8, (what, l, float(np.isfinite(want[:, :, l]).mean()))
  _check_counts(got, want, 2, flags, what)
  fin = np.isfinite(want[:, :, 0])
  np.testing.assert_allclose(got[:, :, 0][fin], want[:, :, 0][fin], rtol=1e-9, atol=0, err_msg=f'{what}: lane 0')
  # lane 1's bound: its scale summed over the points that enter the partial
  sc = np.where(np.isnan(stat[..., 1]), 0.0, scale)[..., None]
  scale_sum = _expected_partials(plan, sc, mask, flags & _hip.FLAG_MASKED)[:, :, 0]
  fin = np.isfinite(want[:, :, 1])
  d = np.abs(got[:, :, 1] - want[:, :, 1])[fin]
  assert (d <= 1e-9 * scale_sum[fin]).all(), (what, 'lane 1', float((d / np.maximum(scale_sum[fin], 1e-300)).max()))


ENS2_SIZES = [(51, 10), (50, 50), (2, 1), (1, 2), (6, 4)]


@pytest.mark.parametrize('mode', ['plain', 'masked', 'skipna'])
@pytest.mark.parametrize('skip', [True, False], ids=['skipna_ens', 'strict'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('m,n', ENS2_SIZES)
def test_two_ensembles_every_partial(ctx, m, n, dtype, skip, mode):
  """Archive-sized and degenerate member counts on both sides, targets member-fastest (a member stride unlike the
  predictions'), x kept on rows of 130 and x summed on rows of 1440 (several 64-lane tiles per row; 1 and 3 rows per partial),
  NaN shares 0 %, 15 % and 'a single valid member on one side'; with WBX_FLAG_SKIPNA_ENS off a NaN member makes the point
  NaN."""
  for nans, x_kept, dc, nlead, nrow, nx in (('none', True, 3, 2, 7, 130), ('some', True, 3, 2, 7, 130), ('single', True, 1, 2, 7, 130),
                                             ('some', False, 1, 1, 2, 1440), ('single', False, 1, 1, 2, 1440), ('none', False, 3, 1, 4, 1440)):
    nan_rows = _ens2_nan_rows(mode, skip, nans, m, n, x_kept)
    nrow = 7 if nan_rows == (0,) else nrow  # (one poisoned row of seven)
    p, t, mask = _ens2_case(100 * m + n, m, n, nlead, nrow, nx, dtype, nans, nan_rows=nan_rows)
    _compare_ens2(ctx, p, t, mask, x_kept, dc, mode, skip, f'M={m} N={n} {nans} {mode} skip={skip} x_kept={x_kept}')


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_two_tight_ensembles_at_a_large_offset(ctx, dtype):
  """M = 51, N = 10 at 5.5e4 +- 30 (geopotential-like): the one-pass moments on x - first valid member hold lane 1's bound.
  (The oracle itself sits 9.3e-13 of lane 1's scale from a longdouble restatement of the formula on such inputs: 1e-9 leaves
  it a factor 1000.)"""
  for nans in ('none', 'some'):
    p, t, mask = _ens2_case(9, 51, 10, 1, 7, 1440, dtype, nans, tight=True)
    _compare_ens2(ctx, p, t, mask, False, 3, 'skipna', True, f'tight {nans}')
  p, t, mask = _ens2_case(10, 51, 10, 2, 7, 130, dtype, 'none', tight=True)
  _compare_ens2(ctx, p, t, mask, True, None, 'plain', False, 'tight strict')


def test_target_member_stride_is_a_signed_64_bit_element_count(ctx):
  """Like the predictions' member stride, the targets' is carried as int64 and not judged: the target members walked from the
  last one down (pointer at the last member, stride -1) are the same ensemble; and with N = 1 the stride is never used, so a
  value no 32-bit integer holds, of either sign, gives what stride 1 gives."""
  p, t, mask = _ens2_case(11, 6, 4, 2, 7, 130, np.float32, 'some')
  _compare_ens2(ctx, p, t, mask, True, 3, 'skipna', True, 'reversed targets', reverse_targets=True)
  p, t, mask = _ens2_case(12, 2, 1, 2, 7, 130, np.float32, 'some')
  for stride in (-(1 << 31) - 8, (1 << 40) + 3):
    _compare_ens2(ctx, p, t, mask, True, 3, 'skipna', True, f'N = 1, stride {stride}', target_stride=stride)
