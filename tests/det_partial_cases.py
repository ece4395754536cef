"""Inputs, the float64 restatement, the error bounds and the routes of the deterministic stage-1 kernels (wbx_det_partial and
wbx_det_map: DetOp<T, FUNC, MM> of csrc/wbx_det.hip on s1_xr / s1_xk / s1_xp / s1_xf / s1_map_kernel of csrc/wbx_s1.hpp), plain NumPy.

Frame.  A case is one launch: a plan (nkey, ndepth, nx, chunks, offset tables, gather tables, x strides, flags, block, vec,
plane_rows, x_weights) and the flat arrays behind its pointers.  `build` lays the inputs out as the case asks (rows unevenly spaced
and out of order, keys in another order in every input, a gathered climatology, broadcast or strided x, contiguous planes with a
lead of 0..3 elements in front of every key's span) and fills every element NO point reads with NaN (mask bytes: 1), so a stray read
poisons its output.

Restatement (`expected`).  Written from include/wbx.h and deterministic.py, not from the kernels: the element of input i at
(key k, depth d, x) is flat[key_off[i][k] + depth_off[i][d] + x * xstride[i]], for i == 2 plus
gather_tab[gather_key[k] * n_gather_depth + gather_depth[d]]; the inputs are widened to float64; the lanes are e = p - t, |e|, e^2,
(p - c)^2, (t - c)^2, (p - c)(t - c) (DET3: the first three, PASS1: p alone); under WBX_FLAG_MASKED alone a point whose mask byte is
0 contributes exactly 0 to every lane whatever it holds and ONE count lane sums the validity; under WBX_FLAG_SKIPNA a lane value that
is NaN is dropped from ITS lane and every value lane has a count lane of its own that sums `not NaN and valid`; x_weights[x]
multiplies value and count lanes alike and x is summed; partial[key][chunk][lane][j] sums rows [chunk * depth_chunk,
min((chunk + 1) * depth_chunk, ndepth)), j = x where x is kept.  wbx_det_map: out[key][d][x] = the requested lane, no sum.

Value classes.
  exact      p, t, c are integers in [-8, 8] and the weights k / 8 with k in 1..16: every lane value is an integer of at most 256, every
             term a multiple of 1/8 of at most 512, every partial sum of at most MAX_POINTS terms below 2^28 -- exact in float64 in
             any order, fused or not (`build` asserts the magnitudes).  The kernels must match bit for bit.
  rounded    geopotential-like fields 5.5e4 + 300 N(0, 1) in the case's dtype: the offsets cancel in every lane and lane 0 sums
             terms of both signs.
  nonfinite  a rounded case with chosen NaN / +inf / -inf points (`special`); the expected placement is what the restatement gives
             under np.errstate.  NaN positions must match exactly, infinities must be equal.

Bound of the rounded class (`Expected.bound`, per output; derived, never fitted).  The widened inputs are exact.  A lane value
carries at most 3 roundings (two differences and their product), each relative u = 2^-53.  A sum of N terms in any order, with or
without fused multiply-adds, adds at most (N - 1) u S, S = sum |term| (the weights included where they are folded in).  So the
kernel is within (N + 3) u S of the exact sum; the factor 1.01 covers the second-order terms and the rounding of S itself.  The
reference here is a plain float64 evaluation -- the lane values and the products with the weights rounded like any float64 code
rounds them, the sum taken by math.fsum -- so it carries its own error of the same kind, and the allowance is 2 x (N + 3) u S x 1.01.
N is the number of points of the partial (rows of the chunk, times nx where x is summed), masked-out ones included.  Count lanes
without weights are sums of ones and are compared exactly.

Routes (`route`): a restatement of dispatch_partial (wbx_det.hip), check_plan, launch_partial, launch_plane, launch_flat_weighted and
launch_map (wbx_s1.hpp) -- the kernel, V, MROW, the block and the grid, or the words of the refusal.  Every case names the route it
is aimed at; tests/test_det_partial_cases.py holds the claim against `route`, so a change of the dispatch fails there instead of
un-aiming a case.  Every list is the smallest shape that reaches its branch; no case has more than MAX_POINTS points."""
import dataclasses
import functools
import math
import types

import numpy as np

DET3, DET6, PASS1 = 0, 1, 2
F32, F64 = 0, 1
FLAG_MASKED, FLAG_SKIPNA = 1, 2
NLANES = {DET3: 3, DET6: 6, PASS1: 1}
NINPUTS = {DET3: 2, DET6: 3, PASS1: 1}
FUNCS = {'det3': DET3, 'det6': DET6, 'pass1': PASS1}
MODES = {'plain': 0, 'masked': FLAG_MASKED, 'skipna': FLAG_SKIPNA, 'masked+skipna': FLAG_MASKED | FLAG_SKIPNA}  # MM 0, 1, 2, 3
NAMES = ('p', 't', 'c', 'mask')
U = 2.0 ** -53
MAX_POINTS = 300_000  # points (nkey * ndepth * nx) of the largest case

# The constants of the dispatch, each with the source line it restates.
MROW_MAX = 8192     # wbx_s1.hpp: constexpr int WBX_MROW_MAX = 8192;
XW_MAX = 2048       # wbx_s1.hpp: constexpr int WBX_XW_MAX = 2048;   (launch_flat_weighted: plan->nx + 3 <= WBX_XW_MAX)
PLANE_THREADS_MAX = 1024  # launch_plane: threads = (nx + 63) / 64 * 64;  WBX_REQUIRE(plan->x_kept && R > 0 && threads <= 1024, ...)
PLANE_MAXV = 2      # launch_plane: nvec = (R * nx + 6) / 4;  WBX_REQUIRE(nvec <= 2 * threads, ...)
PLANE_LDS_MAX = 80 * 1024  # launch_plane: WBX_REQUIRE(lds <= 80 * 1024, ...)
PLANE_LDS_ATTR = 48 * 1024  # launch_plane: if (lds > 48 * 1024) hipFuncSetAttribute(... MaxDynamicSharedMemorySize ...)
MAP_THREADS = 256   # launch_map: a.nxtile = (nx + 255) / 256;  dim3(256)

REFUSED = {
    'plan_block': 'block_threads must be 64, 128 or 256',
    'plan_vec4': 'vec=4 with x summed needs nx % 4 == 0',
    'plan_vec4_stride': 'vec=4 needs unit/zero x strides',
    'flat_skipna': 'flat x-weighted mode does not take the skipna flag',
    'flat_inputs': 'flat x-weighted mode needs unit x stride and 16-byte aligned inputs',
    'flat_mask': 'flat x-weighted mode needs a unit-stride, 4-byte aligned mask',
    'flat_f64': 'flat x-weighted mode is fp32 only',
    'flat_shape': 'flat x-weighted mode needs x summed, plane_rows % 4 == 0 and nx <= 2045',
    'flat_chunks': 'flat x-weighted mode needs depth_chunk % 4 == 0 and whole planes',
    'weights_alone': 'x_weights needs the flat mode (plane_rows > 0, fp32, no mask)',
    'plane_skipna': 'plane mode does not take the skipna flag',
    'plane_inputs': 'plane mode needs unit x stride and 16-byte aligned inputs',
    'plane_mask': 'plane mode needs a unit-stride, 4-byte aligned mask',
    'plane_f64': 'plane mode is fp32 only',
    'plane_shape': 'plane mode needs x kept and nx <= 1024',
    'plane_chunks': 'plane mode needs depth_chunk % plane_rows == 0',
    'plane_block': 'plane_rows too large for the block (R*nx/4 > 2*threads)',
    'plane_lds': 'exceeds 80 KiB (two blocks per CU)',
    'map_lane': 'out of range for family',
}


def lanes_total(func, flags):
  nl = NLANES[func]
  return 2 * nl if flags & FLAG_SKIPNA else (nl + 1 if flags & FLAG_MASKED else nl)


@dataclasses.dataclass
class Plan:
  """wbx_s1_plan with host tables (engine._PlanOnDevice uploads them; tests/fake_device.py reads them as they are)."""
  nkey: int
  ndepth: int
  nx: int
  x_kept: bool
  nchunk: int
  depth_chunk: int
  xstride: list
  key_off: list
  depth_off: list
  gather_key: object = None
  gather_depth: object = None
  gather_tab: object = None
  n_gather_depth: int = 0
  flags: int = 0
  block_threads: int = 64
  vec: int = 1
  plane_rows: int = 0
  x_weights: object = None

  @property
  def nj(self):
    return self.nx if self.x_kept else 1

  def partial_shape(self, nlanes_total):
    return (self.nkey, self.nchunk, nlanes_total, self.nj)

  def chunk_rows(self, c):
    d0 = c * self.depth_chunk
    return d0, max(d0, min(d0 + self.depth_chunk, self.ndepth))


@dataclasses.dataclass(frozen=True)
class Case:
  """One launch.  `kernel`, `mrow` (and vec, bt, R) name the route the case is aimed at."""
  name: str
  kernel: str              # 'xr' | 'xk' | 'xp' | 'xf' | 'map' | 'none' (an empty extent: zeros, nothing launched)
  func: int = DET3
  flags: int = 0
  dtype: str = 'float32'
  nkey: int = 3
  D: int = 5
  nx: int = 65
  dchunk: int = 0          # rows per chunk; 0: one chunk of D rows
  nchunk: int = 0          # 0: ceil(D / dchunk); more: trailing chunks without rows
  bt: int = 64             # block_threads
  vec: int = 1
  R: int = 0               # plane_rows
  weights: bool = False    # x_weights (the flat sweep)
  klass: str = 'rounded'   # 'exact' | 'rounded' | 'nonfinite'
  contig: bool = False     # rows of a key back to back (what plane_rows promises), keys 16-byte aligned plus `leads`
  leads: tuple = (0, 0, 0, 0)  # contig: elements in front of key k's span of input i: (leads[i] + k) % 4 if lead_walk else leads[i]
  lead_walk: bool = False
  uneven: bool = False     # depth rows out of order with gaps of differing size (an unevenly spaced depth_off)
  gather: str = ''         # '' | 'kd' | 'k' (gather_depth NULL) | 'd' (gather_key NULL): c through the gather tables
  xs: int = 1              # xstride of p, t, c
  bcast: str = ''          # the inputs (letters of 'ptcm') with xstride 0
  mask_depth: bool = True  # the mask depends on the depth row; False: depth_off[3] NULL, one mask row per key
  mask_zero_tab: bool = False  # ... but with a depth_off[3] table of zeros all the same
  row_pad: int = 0         # unused elements behind every row
  mask_tail: int = 0       # the last columns masked out in every row
  lane: int = 0            # wbx_det_map
  keep_x: bool = False     # kernel 'none': x kept
  special: str = ''        # klass 'nonfinite': see _inject
  mrow: bool = False       # s1_xr_kernel<Op, V, true>: the key's mask row staged in LDS
  seed: int = 0

  @property
  def npoint(self):
    return self.nkey * self.D * self.nx

  @property
  def plan_dchunk(self):
    return self.dchunk or max(self.D, 1)

  @property
  def plan_nchunk(self):
    return self.nchunk or max(1, -(-self.D // self.plan_dchunk))


# ---------------------------------------------------------------------------------------------------------------------
# addressing (include/wbx.h, "element address of input i at (key k, depth d, x)")


def addresses(plan, i, swap_gather=False):
  """-> int64 [nkey][ndepth][nx]: the element of input i every point reads."""
  ko = plan.key_off[i] if plan.key_off[i] is not None else np.zeros(plan.nkey, np.int64)
  do = plan.depth_off[i] if plan.depth_off[i] is not None else np.zeros(plan.ndepth, np.int64)
  off = ko[:, None, None] + do[None, :, None] + (np.arange(plan.nx, dtype=np.int64) * plan.xstride[i])[None, None, :]
  if i == 2 and plan.gather_tab is not None:
    gk = plan.gather_key.astype(np.int64) if plan.gather_key is not None else np.zeros(plan.nkey, np.int64)
    gd = plan.gather_depth.astype(np.int64) if plan.gather_depth is not None else np.zeros(plan.ndepth, np.int64)
    ngd = plan.n_gather_depth if plan.n_gather_depth > 0 else 1
    if swap_gather:  # (a mutant: row and column of the table swapped)
      ngk = plan.gather_tab.size // ngd
      sel = (gd[None, :] * ngk + gk[:, None]) % plan.gather_tab.size
    else:
      sel = gk[:, None] * ngd + gd[None, :]
    off = off + plan.gather_tab[sel][:, :, None]
  return off


def _round_up(n, m):
  return -(-n // m) * m


def build(case):
  """-> namespace: case, plan, flat[name] (the array behind each pointer), idx[name] (addresses), xw."""
  assert case.npoint <= MAX_POINTS, (case.name, case.npoint)
  rng = np.random.default_rng(7000 + case.seed)
  dt = np.dtype(case.dtype)
  nkey, D, nx = case.nkey, case.D, case.nx
  nin = NINPUTS[case.func]
  masked = bool(case.flags & FLAG_MASKED)
  skipna = bool(case.flags & FLAG_SKIPNA)
  xs = [case.xs, case.xs, case.xs, 1]
  for ch in case.bcast:
    xs['ptcm'.index(ch)] = 0
  plan = Plan(nkey=nkey, ndepth=D, nx=nx, x_kept=case.kernel in ('xk', 'xp') or case.keep_x,
              nchunk=case.plan_nchunk, depth_chunk=case.plan_dchunk, xstride=xs, key_off=[None] * 4, depth_off=[None] * 4, flags=case.flags,
              block_threads=case.bt, vec=case.vec, plane_rows=case.R)
  sizes = {}
  for i, name in enumerate(NAMES):
    if (i < 3 and i >= nin) or (i == 3 and not masked):
      continue
    kperm = rng.permutation(nkey).astype(np.int64)  # (another order of the keys in every input)
    width = 1 if xs[i] == 0 else (max(nx, 1) - 1) * abs(xs[i]) + 1
    base = (max(nx, 1) - 1) * -xs[i] if xs[i] < 0 else 0  # a reversed row starts at its last element
    if case.contig:
      assert xs[i] == 1 and not case.uneven and not (i == 2 and case.gather) and case.mask_depth
      kspan = _round_up(D * nx + 3, 4) + 4
      lead = (case.leads[i] + (np.arange(nkey) if case.lead_walk else 0)) % 4
      plan.key_off[i] = kperm * kspan + lead
      plan.depth_off[i] = np.arange(D, dtype=np.int64) * nx
      sizes[name] = nkey * kspan
      continue
    rs = _round_up(width + case.row_pad, 4)  # (rows start at multiples of 4 elements: vec = 4 reads four mask bytes as one dword)
    if i == 2 and case.gather:
      ngk, ngd = (2 if 'k' in case.gather else 1), (3 if 'd' in case.gather else 1)
      plan.key_off[i] = kperm * rs + base
      plan.gather_key = (np.arange(nkey) % 2).astype(np.int32) if 'k' in case.gather else None
      plan.gather_depth = ((2 * np.arange(D) + 1) % 3).astype(np.int32) if 'd' in case.gather else None
      plan.n_gather_depth = ngd
      plan.gather_tab = rng.permutation(ngk * ngd).astype(np.int64) * (nkey * rs)  # the slice of a [slice][key][x] climatology
      sizes[name] = ngk * ngd * nkey * rs
      continue
    per_depth = not (i == 3 and not case.mask_depth)
    nslot = D if per_depth else 1
    if case.uneven and per_depth:
      slots = nslot + 3
      pos = rng.permutation(slots)[:nslot].astype(np.int64)
    else:
      slots, pos = max(nslot, 1), np.arange(nslot, dtype=np.int64)
    plan.key_off[i] = kperm * (slots * rs) + base
    if per_depth:
      plan.depth_off[i] = pos * rs
    elif case.mask_zero_tab:
      plan.depth_off[i] = np.zeros(D, np.int64)
    sizes[name] = nkey * slots * rs
  if case.weights:
    nw, wrng = max(nx, 1), np.random.default_rng(9000 + case.seed)  # (a generator of their own: the same data with and without them)
    plan.x_weights = wrng.integers(1, 17, size=nw) / 8.0 if case.klass == 'exact' else 0.25 + wrng.random(nw)  # differ per latitude

  flat, idx = {}, {}
  for i, name in enumerate(NAMES):
    if name not in sizes:
      continue
    n = max(sizes[name], 4)
    a = addresses(plan, i)
    if a.size:
      assert a.min() >= 0 and a.max() < n, (case.name, name, int(a.min()), int(a.max()), n)
      if case.vec == 4 and xs[i] == 1 and not plan.x_kept:
        assert nx % 4 == 0
      if case.vec == 4 and i == 3 and xs[i] == 1:
        assert (a[:, :, 0] % 4 == 0).all(), (case.name, 'vec = 4 reads four mask bytes as one aligned dword')
      if case.weights:
        assert (a[:, ::max(case.R, 1), 0] % 4 == 0).all(), (case.name, 'the flat sweep reads aligned float4s')
    used = np.zeros(n, bool)
    used[a.reshape(-1)] = True
    if i < 3:
      if case.klass == 'exact':
        vals = rng.integers(-8, 9, size=n).astype(dt)
      else:
        vals = (5.5e4 + 300.0 * rng.normal(size=n)).astype(dt)
      if skipna:
        vals[rng.random(n) < (0.02 if case.klass == 'nonfinite' else 0.04)] = np.nan
      flat[name] = np.where(used, vals, np.nan).astype(dt)
    else:
      vals = ((rng.random(n) < (0.9 if case.klass == 'nonfinite' else 0.7)) * rng.choice([1, 2, 255], size=n)).astype(np.uint8)  # nonzero = valid
      flat[name] = np.where(used, vals, 1).astype(np.uint8)
      if case.mask_tail:
        flat[name][a[:, :, nx - case.mask_tail:].reshape(-1)] = 0
    idx[name] = a
  if masked and not skipna and case.klass != 'exact' and case.npoint:
    # what the mask hides leaves no trace: NaN / inf in elements that only masked-out points read
    valid = flat['mask'][idx['mask']] != 0
    for name, bad in (('p', np.nan), ('t', np.inf), ('c', -np.inf)):
      if name in flat:
        seen = np.zeros(flat[name].size, bool)
        seen[idx[name][valid]] = True
        hide = ~seen & (rng.random(seen.size) < 0.3)
        used = np.zeros(seen.size, bool)
        used[idx[name].reshape(-1)] = True
        flat[name][hide & used] = bad
  inp = types.SimpleNamespace(case=case, plan=plan, flat=flat, idx=idx, xw=plan.x_weights)
  if case.special:
    _inject(inp)
  if case.klass == 'exact':
    big = max([float(np.nanmax(np.abs(flat[n][idx[n]]))) for n in ('p', 't', 'c') if n in flat and case.npoint and not np.isnan(flat[n][idx[n]]).all()] + [0.0])
    wmax = float(plan.x_weights.max()) if case.weights and nx else 1.0
    assert big <= 8 and wmax <= 2 and (2 * big) ** 2 * wmax * MAX_POINTS * 8 < 2 ** 53, (case.name, big, wmax)
    if case.weights:
      assert (plan.x_weights * 8 == np.round(plan.x_weights * 8)).all()
  return inp


TARGET_KEY = 1  # the key the chosen non-finite values go into (its first chunk)


def _inject(inp):
  """klass 'nonfinite'.  All in key TARGET_KEY, chunk 0, column x0 (so that the same partial is hit where x is kept):
  'nan' / 'pinf' / 'ninf': one such p;  'inf_pair': p = +inf and, one row on, p = -inf;  'hidden': NaN, +inf, -inf in p / t / c at
  points the mask hides;  'c_nan': one NaN climatology (skipna: lanes 3-5 lose the point, 0-2 keep it);  'all_nan': every p of the
  partial NaN (skipna: sum 0, count 0 in every lane that reads p)."""
  case, plan, flat, idx = inp.case, inp.plan, inp.flat, inp.idx
  sp = case.special
  k0, x0 = TARGET_KEY, case.nx // 3
  d0, d1 = plan.chunk_rows(0)
  assert d1 - d0 >= 2 and case.nkey > k0 and not case.bcast
  at = lambda name, d, x=x0: idx[name][k0, d, x]
  if 'mask' in flat and sp != 'hidden':  # the two chosen points are valid ones (and hold nothing the mask was hiding)
    for d in (d0, d0 + 1):
      flat['mask'][at('mask', d)] = 1
      for name, v in (('p', 5.51e4), ('t', 5.5e4), ('c', 5.49e4)):
        if name in flat:
          flat[name][at(name, d)] = v + d
  if sp in ('nan', 'pinf', 'ninf'):
    flat['p'][at('p', d0)] = {'nan': np.nan, 'pinf': np.inf, 'ninf': -np.inf}[sp]
  elif sp == 'inf_pair':
    flat['p'][at('p', d0)] = np.inf
    flat['p'][at('p', d0 + 1)] = -np.inf
  elif sp == 'hidden':
    for name, d, bad in (('p', d0, np.nan), ('t', d0 + 1, np.inf), ('c', d0, -np.inf)):
      if name in flat:
        flat['mask'][at('mask', d)] = 0
        flat[name][at(name, d)] = bad
  elif sp == 'c_nan':
    assert case.flags & FLAG_SKIPNA and case.func == DET6
    flat['p'][at('p', d0)] = flat['t'][at('t', d0)] = 5.5e4
    flat['c'][at('c', d0)] = np.nan
  elif sp == 'all_nan':
    assert case.flags & FLAG_SKIPNA
    xsel = slice(x0, x0 + 1) if plan.x_kept else slice(None)
    flat['p'][idx['p'][k0, d0:d1, xsel].reshape(-1)] = np.nan
  else:
    raise ValueError(sp)


# ---------------------------------------------------------------------------------------------------------------------
# restatement


def stat(func, p, t=None, c=None):
  """The value lanes in float64 from the widened inputs: a list of arrays."""
  with np.errstate(all='ignore'):
    p = np.asarray(p).astype(np.float64)
    if func == PASS1:
      return [p]
    t = np.asarray(t).astype(np.float64)
    e = p - t
    out = [e, np.abs(e), e * e]
    if func == DET6:
      c = np.asarray(c).astype(np.float64)
      pa, ta = p - c, t - c
      out += [pa * pa, ta * ta, pa * ta]
    return out


MUTANTS = {
    'xr': ('drop_last_row', 'first_batch_only', 'count_from_lane0', 'mask_not_on_c', 'gather_swapped'),
    'xk': ('drop_last_row', 'drop_tail_lane', 'count_from_lane0', 'mask_not_on_c', 'gather_swapped'),
    'xp': ('drop_last_row', 'lead_data', 'lead_mask', 'mask_not_on_c'),
    'xf': ('drop_last_row', 'weight_next_latitude', 'weight_wrap', 'mask_not_on_c'),
    'map': ('gather_swapped',),
}


@dataclasses.dataclass
class Expected:
  want: np.ndarray   # [nkey][nchunk][lanes_total][nj]  (wbx_det_map: [nkey][ndepth][nx])
  bound: np.ndarray  # same shape; 0 where the output must be exact
  terms: int         # the largest N of the bound


def point_lanes(inp, mutant=''):
  """-> (lanes: the list of [nkey][D][nx] float64 terms of every lane of the partial, count lanes included, the weights not yet;
  nvalue: how many of them are value lanes)."""
  case, plan, flat = inp.case, inp.plan, inp.flat
  shape = (plan.nkey, plan.ndepth, plan.nx)
  nin = NINPUTS[case.func]

  def read(i, shift=0):
    a = addresses(plan, i, swap_gather=(mutant == 'gather_swapped'))
    return flat[NAMES[i]][np.minimum(a + shift, flat[NAMES[i]].size - 1)]

  v = [read(i, 1 if (mutant == 'lead_data' and i == 0) else 0).astype(np.float64) for i in range(nin)] + [None] * (3 - nin)
  valid = np.ones(shape, bool)
  if case.flags & FLAG_MASKED:
    valid = read(3, 1 if mutant == 'lead_mask' else 0) != 0
    v = [None if a is None else (a if (mutant == 'mask_not_on_c' and i == 2) else np.where(valid, a, 0.0)) for i, a in enumerate(v)]
  vals = stat(case.func, *v)
  if case.flags & FLAG_SKIPNA:
    oks = [valid & ~np.isnan(a) for a in vals]
    cnt = [oks[0]] * len(oks) if mutant == 'count_from_lane0' else oks
    return [np.where(ok, a, 0.0) for ok, a in zip(oks, vals)] + [ok.astype(np.float64) for ok in cnt], len(vals)
  if case.flags & FLAG_MASKED:
    return vals + [valid.astype(np.float64)], len(vals)
  return vals, len(vals)


def _sums(rows, exact):
  """rows [nout][nterm] -> [nout]: exact sums where every term is finite (math.fsum; the exact class needs none), IEEE sums else."""
  with np.errstate(all='ignore'):
    out = rows.sum(axis=1)
  if exact or rows.shape[1] == 0:
    return out
  fin = np.isfinite(rows).all(axis=1)
  if fin.any():
    out[fin] = [math.fsum(r) for r in rows[fin].tolist()]
  return out


def expected(inp, mutant=''):
  """The float64 restatement of wbx_det_partial for the launch `inp` describes.  `mutant`: one wrong reading of the plan (MUTANTS),
  for tests/test_det_partial_cases.py to show that the cases can see it."""
  case, plan = inp.case, inp.plan
  nkey, D, nx = plan.nkey, plan.ndepth, plan.nx
  lanes, nvalue = point_lanes(inp, mutant)
  nl = len(lanes)
  assert nl == lanes_total(case.func, case.flags)
  w = None
  if plan.x_weights is not None:
    d, x = np.meshgrid(np.arange(D), np.arange(nx), indexing='ij')
    wi = x
    if mutant == 'weight_next_latitude':
      wi = (x + 1) % nx
    elif mutant == 'weight_wrap':  # a float4 of the flat sweep that runs over a row's end takes the row's last weight beyond it
      e = (d % plan.plane_rows) * nx + x
      wi = np.where((e // 4 * 4) % nx + e % 4 >= nx, nx - 1, x)
    w = np.asarray(plan.x_weights)[wi][None, :, :]
  keep = np.ones((D, nx), bool)
  for c in range(plan.nchunk):
    d0, d1 = plan.chunk_rows(c)
    if mutant == 'drop_last_row' and d1 > d0:
      keep[d1 - 1] = False
    if mutant == 'first_batch_only':
      keep[d0 + 64 * (plan.block_threads // 64):d1] = False
  if mutant == 'drop_tail_lane' and plan.vec == 4:
    keep[:, nx // 4 * 4:] = False
  want = np.zeros(plan.partial_shape(nl))
  bound = np.zeros_like(want)
  nmax = 0
  exact = case.klass == 'exact'
  with np.errstate(all='ignore'):
    for l, lane in enumerate(lanes):
      terms = lane if w is None else lane * w  # (the rounded products)
      terms = np.where(keep[None], terms, 0.0)
      for c in range(plan.nchunk):
        d0, d1 = plan.chunk_rows(c)
        blk = terms[:, d0:d1, :]
        rows = np.moveaxis(blk, 1, 2).reshape(nkey * nx, d1 - d0) if plan.x_kept else blk.reshape(nkey, (d1 - d0) * nx)
        n = rows.shape[1]
        nmax = max(nmax, n)
        want[:, c, l, :] = _sums(rows, exact).reshape(nkey, plan.nj)
        if not exact and not (l >= nvalue and w is None):  # (count lanes without weights: sums of ones, exact)
          s = np.where(np.isfinite(rows), np.abs(rows), 0.0).sum(axis=1)
          bound[:, c, l, :] = (2 * (n + 3) * U * 1.01 * s).reshape(nkey, plan.nj)
  return Expected(want=want, bound=bound, terms=nmax)


def expected_map(inp, mutant=''):
  """wbx_det_map: out[key][d][x] = lane `case.lane` of the point, NaN and all.  At most 3 roundings: 3 u |value| x 1.01 against the
  restatement's own evaluation of the same formula (twice that; the exact class bit for bit)."""
  case = inp.case
  lanes, _ = point_lanes(inp, mutant)
  want = lanes[case.lane]
  with np.errstate(all='ignore'):
    bound = np.zeros_like(want) if case.klass == 'exact' else 2 * 3 * U * 1.01 * np.where(np.isfinite(want), np.abs(want), 0.0)
  return Expected(want=want, bound=bound, terms=1)


@functools.lru_cache(maxsize=None)
def prepared(case):
  """-> (inputs, Expected), computed once per session and left unchanged."""
  inp = build(case)
  for a in inp.flat.values():
    a.setflags(write=False)
  exp = expected_map(inp) if case.kernel == 'map' else expected(inp)
  exp.want.setflags(write=False)
  exp.bound.setflags(write=False)
  return inp, exp


def differs(got, exp):
  """Does `got` leave the restatement `exp`: another NaN pattern, another infinity, or a finite output beyond its bound?"""
  want, bound = exp.want, exp.bound
  if (np.isnan(got) != np.isnan(want)).any():
    return True
  ok = ~np.isnan(want)
  inf = ok & np.isinf(want)
  if (got[inf] != want[inf]).any():
    return True
  fin = ok & ~inf
  with np.errstate(all='ignore'):
    return bool((np.abs(got[fin] - want[fin]) > bound[fin]).any())


# ---------------------------------------------------------------------------------------------------------------------
# routes


def route(plan, func, dtype, map_lane=None, misaligned=()):
  """What det_common does with this call -> dict(refused=None or the words, kernel, V, mrow, threads, grid, lds, lds_attr).
  `misaligned`: the inputs (names) whose pointer is not 16-byte (mask: 4-byte) aligned."""
  r = dict(refused=None, kernel=None, V=plan.vec, mrow=False, threads=plan.block_threads, grid=0, lds=0, lds_attr=False)

  def refuse(why):
    r['refused'] = REFUSED[why]
    return r

  nl = NLANES[func]
  if map_lane is not None and not 0 <= map_lane < nl:  # wbx_det_map: if (lane < 0 || lane >= nl) return fail(...)
    return refuse('map_lane')
  # check_plan
  if plan.block_threads not in (64, 128, 256):
    return refuse('plan_block')
  if plan.vec == 4:
    if not (plan.x_kept or plan.nx % 4 == 0):
      return refuse('plan_vec4')
    if any(s not in (0, 1) for s in plan.xstride):
      return refuse('plan_vec4_stride')
  empty = plan.nkey == 0 or plan.ndepth == 0 or plan.nx == 0
  nin = NINPUTS[func]
  masked, skipna = bool(plan.flags & FLAG_MASKED), bool(plan.flags & FLAG_SKIPNA)
  if map_lane is not None:  # dispatch_func: map ? launch_map<DetOp<T, FUNC, 0>>
    if empty:
      return dict(r, kernel='none')
    return dict(r, kernel='map', V=1, threads=MAP_THREADS, grid=plan.nkey * plan.ndepth * (-(-plan.nx // MAP_THREADS)))
  R = plan.plane_rows
  if (plan.x_weights is not None and R > 0) or R > 0:  # dispatch_partial: the flat sweep, then plane mode
    flat = plan.x_weights is not None
    mode = 'flat' if flat else 'plane'
    if dtype != F32:
      return refuse(mode + '_f64')
    if skipna:
      return refuse(mode + '_skipna')
    if any(plan.xstride[i] != 1 or NAMES[i] in misaligned for i in range(nin)):
      return refuse(mode + '_inputs')
    if masked and (plan.xstride[3] != 1 or 'mask' in misaligned):
      return refuse(mode + '_mask')
    if empty:
      return dict(r, kernel='none')
    if flat:  # launch_flat_weighted
      if not (not plan.x_kept and R % 4 == 0 and plan.nx + 3 <= XW_MAX):
        return refuse('flat_shape')
      if not (plan.depth_chunk % 4 == 0 and plan.ndepth % R == 0):
        return refuse('flat_chunks')
      return dict(r, kernel='xf', V=4, grid=plan.nkey * plan.nchunk)
    threads = -(-plan.nx // 64) * 64  # launch_plane
    if not (plan.x_kept and threads <= PLANE_THREADS_MAX):
      return refuse('plane_shape')
    if not (plan.depth_chunk % R == 0 or plan.nchunk == 1):
      return refuse('plane_chunks')
    nvec = (R * plan.nx + 6) // 4
    if nvec > PLANE_MAXV * threads:
      return refuse('plane_block')
    lds = nin * (R * plan.nx + 8) * 4 + ((R * plan.nx + 16) if masked else 0)
    if lds > PLANE_LDS_MAX:
      return refuse('plane_lds')
    return dict(r, kernel='xp', V=4, threads=threads, grid=plan.nkey * plan.nchunk, lds=lds, lds_attr=lds > PLANE_LDS_ATTR,
                second_vec=nvec > threads)
  if plan.x_weights is not None:
    return refuse('weights_alone')
  if empty:  # launch_partial: s1_zero_if_empty
    return dict(r, kernel='none')
  if plan.x_kept:  # s1_grid: nxtile = ceil(nx / (block_threads * V))
    return dict(r, kernel='xk', grid=plan.nkey * plan.nchunk * (-(-plan.nx // (plan.block_threads * plan.vec))))
  mrow = (masked and not skipna and plan.depth_off[3] is None and plan.xstride[3] == 1 and plan.nx <= MROW_MAX and plan.ndepth > 1)
  return dict(r, kernel='xr', mrow=mrow, grid=plan.nkey * plan.nchunk)


def route_of(inp):
  case = inp.case
  return route(inp.plan, case.func, F32 if case.dtype == 'float32' else F64, map_lane=case.lane if case.kernel == 'map' else None)


# ---------------------------------------------------------------------------------------------------------------------
# the cases


def _name(*parts):
  return '-'.join(str(p) for p in parts)


def _both(**kw):
  """The rounded and the exact flavour of one shape."""
  name = kw.pop('name')
  return [Case(name=name + '-rnd', klass='rounded', **kw), Case(name=name + '-int', klass='exact', **kw)]


def xr_matrix_cases():
  """f32 / f64 x DET3 / DET6 / PASS1 x MM 0..3 x vec 1 / 4: nkey 3, 5 rows in chunks of 2 (a ragged last chunk), nx = 68 (not a
  multiple of 64 V), rows unevenly spaced, keys in another order in every input."""
  out, seed = [], 0
  for dtype in ('float32', 'float64'):
    for fname, func in FUNCS.items():
      for mode, flags in MODES.items():
        seed += 1  # (vec 1 and vec 4 on the same data)
        for vec in (1, 4):
          out += _both(name=_name('xr', fname, mode, dtype, 'vec%d' % vec), kernel='xr', func=func, flags=flags, dtype=dtype, vec=vec, nx=68,
                       D=5, dchunk=2, uneven=True, seed=seed)
  return out


def xr_shape_cases():
  out = []
  kw = dict(kernel='xr', func=DET6, flags=FLAG_MASKED | FLAG_SKIPNA)
  for bt in (64, 128, 256):  # rows not a multiple of the wave count
    out += _both(name=_name('xr-block', bt), bt=bt, nx=65, D=7, seed=100 + bt, **kw)
  for nx, vec in ((1, 1), (63, 1), (65, 1), (4, 4), (4, 1), (260, 4), (300, 4)):  # 260, 300: not multiples of 64 V = 256
    out += _both(name=_name('xr-nx', nx, 'vec%d' % vec), nx=nx, vec=vec, D=3, seed=200 + nx + vec, **kw)
  for rows in (1, 63, 64, 65):  # one wave: the batch of 64 rows, its neighbours, a second batch of one row
    out += _both(name=_name('xr-rows', rows), nkey=2, nx=5, D=rows, uneven=True, seed=300 + rows, **kw)
  # four waves: 257 rows are a whole first batch (4 x 64) and a second one of a single row
  out += _both(name='xr-rows-257-four-waves', nkey=2, nx=5, D=257, bt=256, uneven=True, seed=557, **kw)
  out += _both(name='xr-rows-130-two-waves', nkey=2, nx=5, D=130, bt=128, uneven=True, seed=558, **kw)  # 128 + a partial batch
  out += _both(name='xr-ragged-chunks', nx=9, D=11, dchunk=4, bt=128, seed=559, **kw)
  out += _both(name='xr-empty-trailing-chunks', nx=9, D=5, dchunk=2, nchunk=5, seed=560, **kw)
  out += _both(name='xr-chunk-of-70-rows', nkey=2, nx=3, D=140, dchunk=70, uneven=True, seed=561, **kw)
  return out


def xr_address_cases():
  out = []
  kw = dict(kernel='xr', func=DET6, nx=12, D=4, dchunk=3)
  for g in ('kd', 'k', 'd'):
    for vec in (1, 4):
      out += _both(name=_name('xr-gather', g, 'vec%d' % vec), gather=g, vec=vec, flags=FLAG_MASKED, nkey=4, seed=600, **kw)
  for vec in (1, 4):
    out += _both(name=_name('xr-bcast-c', 'vec%d' % vec), bcast='c', vec=vec, flags=FLAG_SKIPNA, seed=610, **kw)
    out += _both(name=_name('xr-bcast-t-mask', 'vec%d' % vec), bcast='tm', vec=vec, flags=FLAG_MASKED, uneven=True, seed=611, **kw)
    out += _both(name=_name('xr-bcast-mask-f64', 'vec%d' % vec), bcast='m', vec=vec, flags=FLAG_MASKED | FLAG_SKIPNA, dtype='float64', seed=612, **kw)
  for xs in (2, -1):
    out += _both(name=_name('xr-xstride', xs), xs=xs, flags=FLAG_MASKED, uneven=True, seed=620, **kw)
    out += _both(name=_name('xr-xstride', xs, 'f64'), xs=xs, flags=0, dtype='float64', gather='kd', seed=621, **kw)
  return out


def xr_mrow_pair():
  """The mask row in LDS at nx = 8192 and, on the SAME storage (rows of 8196 elements), the plain route at nx = 8196 with the last
  four columns masked out: the same sums, bit for bit on the exact class."""
  kw = dict(kernel='xr', func=DET6, flags=FLAG_MASKED, nkey=2, D=2, vec=4, mask_depth=False, seed=700)
  return [(Case(name=_name('xr-mrow-on-8192', k), nx=8192, row_pad=4, mrow=True, klass=kl, **kw),
           Case(name=_name('xr-mrow-off-8196', k), nx=8196, mask_tail=4, klass=kl, **kw)) for k, kl in (('rnd', 'rounded'), ('int', 'exact'))]


def xr_mrow_cases():
  out = []
  kw = dict(kernel='xr', flags=FLAG_MASKED, mask_depth=False, nx=68, D=5, dchunk=2)
  for fname, func in FUNCS.items():
    for vec in (1, 4):
      for dtype in ('float32', 'float64'):
        out += _both(name=_name('xr-mrow', fname, dtype, 'vec%d' % vec), func=func, dtype=dtype, vec=vec, mrow=True, seed=710, **kw)
  out += _both(name='xr-mrow-odd-nx', func=DET6, vec=1, mrow=True, seed=711, **dict(kw, nx=67))
  out += _both(name='xr-mrow-off-one-row', func=DET6, vec=4, seed=712, **dict(kw, D=1, dchunk=0))  # ndepth = 1
  out += _both(name='xr-mrow-off-zero-table', func=DET6, vec=4, mask_zero_tab=True, seed=710, **kw)  # a depth_off[3], all zeros
  out += _both(name='xr-mrow-off-skipna', func=DET6, vec=4, seed=713, **dict(kw, flags=FLAG_MASKED | FLAG_SKIPNA))
  return out


def xr_mrow_twins():
  """(LDS mask row, the same data with a depth_off[3] table of zeros): bit-identical on the exact class."""
  cases = {c.name: c for c in xr_mrow_cases()}
  return [(cases[_name('xr-mrow-det6-float32-vec4', k)], cases[_name('xr-mrow-off-zero-table', k)]) for k in ('rnd', 'int')]


def xk_cases():
  out = []
  for mode, flags in MODES.items():
    for dtype in ('float32', 'float64'):
      for vec, nx in ((1, 70), (4, 68), (4, 69), (4, 70), (4, 71)):  # nx % 4 = 1, 2, 3: the nvalid < V lane
        out += _both(name=_name('xk', mode, dtype, 'vec%d' % vec, 'nx%d' % nx), kernel='xk', func=DET6, flags=flags, dtype=dtype, vec=vec, nx=nx,
                     D=6, dchunk=4, uneven=True, gather='kd' if mode == 'plain' else '', seed=800 + nx)
  for fname in ('det3', 'pass1'):
    out += _both(name=_name('xk', fname), kernel='xk', func=FUNCS[fname], flags=FLAG_MASKED | FLAG_SKIPNA, vec=4, nx=7, D=3, seed=820)
  for rows in (1, 2, 3, 4, 5, 7):  # around the 4 x unrolled row loop
    out += _both(name=_name('xk-rows', rows), kernel='xk', func=DET3, flags=FLAG_SKIPNA, vec=4, nx=10, D=rows, uneven=True, seed=830 + rows)
    out += _both(name=_name('xk-rows', rows, 'ragged-lane'), kernel='xk', func=DET6, flags=FLAG_MASKED, vec=4, nx=3, D=rows, seed=840 + rows)
  # two x tiles and idle lanes past nx: 64 * 1 < 100 <= 128; 64 * 4 < 258 <= 512 (its last live lane is a ragged one)
  out += _both(name='xk-two-tiles-vec1', kernel='xk', func=DET6, flags=FLAG_MASKED, vec=1, nx=100, D=3, dchunk=2, seed=850)
  out += _both(name='xk-two-tiles-vec4', kernel='xk', func=DET6, flags=FLAG_SKIPNA, vec=4, nx=258, D=3, dchunk=2, seed=851)
  out += _both(name='xk-block-256', kernel='xk', func=DET3, vec=1, bt=256, nx=300, D=2, seed=852)
  out += _both(name='xk-bcast-c', kernel='xk', func=DET6, vec=4, bcast='c', nx=9, D=3, seed=853)
  out += _both(name='xk-xstride-2', kernel='xk', func=DET6, flags=FLAG_MASKED, xs=2, nx=9, D=3, seed=854)
  out += _both(name='xk-empty-trailing-chunk', kernel='xk', func=DET3, flags=FLAG_MASKED, nx=9, D=3, dchunk=2, nchunk=4, seed=855)
  return out


def xp_cases():
  """Plane mode: contiguous rows, a lead of (leads[i] + key) % 4 elements in front of key's span, another for every input and the
  mask; nkey = 4, so every input meets the leads 0, 1, 2, 3."""
  out = []
  kw = dict(kernel='xp', contig=True, lead_walk=True, nkey=4)
  for nx, R, D, dchunk in ((64, 2, 5, 0), (64, 3, 7, 0), (65, 5, 10, 5), (65, 8, 19, 0), (721, 2, 4, 2), (721, 3, 5, 0), (1024, 2, 3, 0),
                           (1024, 3, 6, 3)):
    for mode in ('plain', 'masked'):
      out += _both(name=_name('xp', nx, 'R%d' % R, 'D%d' % D, mode), func=DET3, flags=MODES[mode], nx=nx, R=R, D=D, dchunk=dchunk,
                   leads=(0, 1, 2, 3), seed=900 + nx + R, **kw)
  for fname, func in FUNCS.items():
    for mode in ('plain', 'masked'):
      out += _both(name=_name('xp', fname, mode), func=func, flags=MODES[mode], nx=67, R=4, D=10, dchunk=4, leads=(3, 1, 0, 2), seed=940, **kw)
  # DET6 at nx = 721, R = 8: 3 * (5768 + 8) * 4 = 69312 B (+ 5784 mask bytes) > 48 KiB, the attribute branch
  for mode in ('plain', 'masked'):
    out += _both(name=_name('xp-det6-721-R8', mode), func=DET6, flags=MODES[mode], nx=721, R=8, D=12, leads=(1, 2, 3, 1), seed=950,
                 **dict(kw, nkey=4))
  # the second float4 of a thread: nvec = (R nx + 6) / 4 against threads = round_up(nx, 64): used at (65, R = 8: 131 > 128) and
  # (64, R = 5: 81 > 64), not used at (65, R = 5: 82 <= 128) or (64, R = 3: 49 <= 64)
  out += _both(name='xp-64-R5-second-float4', func=DET6, flags=FLAG_MASKED, nx=64, R=5, D=10, dchunk=5, leads=(2, 0, 1, 3), seed=960, **kw)
  # the straddling float4: lead + rows * nx not a multiple of 4 at the span's end (nx = 65, a last group of 1 row, lead 0..3)
  out += _both(name='xp-65-straddle', func=DET3, flags=FLAG_MASKED, nx=65, R=2, D=3, leads=(0, 2, 1, 3), seed=961, **kw)
  out += _both(name='xp-1-column', func=DET3, flags=FLAG_MASKED, nx=1, R=3, D=7, leads=(0, 1, 2, 3), seed=962, **kw)
  return out


def xp_route_twins():
  """Plane cases that s1_xk_kernel serves from the same data (plane_rows = 0): the same bits on the exact class."""
  pick = ('xp-65-R5-D10-masked', 'xp-721-R3-D5-plain', 'xp-det6-masked', 'xp-det6-721-R8-masked', 'xp-64-R5-second-float4', 'xp-65-straddle')
  cases = {c.name: c for c in xp_cases()}
  return [(cases[_name(n, k)], dataclasses.replace(cases[_name(n, k)], name=_name(n, k, 'as-xk'), kernel='xk', R=0)) for n in pick
          for k in ('rnd', 'int')]


def xf_cases():
  out = []
  kw = dict(kernel='xf', contig=True, weights=True)
  for fname, func in FUNCS.items():
    for mode in ('plain', 'masked'):
      for bt in (64, 128, 256):
        out += _both(name=_name('xf', fname, mode, bt), func=func, flags=MODES[mode], bt=bt, nx=67, R=8, D=16, dchunk=8, seed=1000 + bt, **kw)
  for nx in (1, 2, 3, 7, 67, 721):  # 1, 2: the 3-element wrap pad wraps more than once
    for R, D, dchunk in ((4, 8, 8), (8, 16, 4)):  # two planes per chunk; a chunk boundary inside a plane
      for mode in ('plain', 'masked'):
        out += _both(name=_name('xf-nx', nx, 'R%d' % R, 'chunk%d' % dchunk, mode), func=DET6, flags=MODES[mode], bt=128, nx=nx, R=R, D=D,
                     dchunk=dchunk, seed=1100 + nx + R, **kw)
  # fewer float4s in a segment than threads: one row quad of nx = 7 is 7 float4s under 64 .. 256 threads (above: nx = 1 .. 67 too);
  # more than one trip: 721 float4s per quad, 1442 per plane of 8 rows
  out += _both(name='xf-empty-trailing-chunk', func=DET3, nx=7, R=4, D=8, dchunk=4, nchunk=3, seed=1200, **kw)
  return out


def xf_route_twins():
  """Flat cases with their s1_xk twin (no weights, x kept): sum_x w[x] * partial[..][x] on the host, exact on the exact class."""
  cases = {c.name: c for c in xf_cases()}
  pick = ('xf-det6-masked-128', 'xf-nx-721-R8-chunk4-plain', 'xf-nx-2-R4-chunk8-masked', 'xf-nx-1-R8-chunk4-masked', 'xf-nx-3-R4-chunk8-plain')
  return [(cases[n + '-int'], dataclasses.replace(cases[n + '-int'], name=n + '-int-as-xk', kernel='xk', R=0, weights=False)) for n in pick]


def map_cases():
  out = []
  for dtype in ('float32', 'float64'):
    for fname, func in FUNCS.items():
      for lane in range(NLANES[func]):
        nx = (1, 256, 257)[lane % 3]
        out += _both(name=_name('map', fname, 'lane%d' % lane, dtype, 'nx%d' % nx), kernel='map', func=func, dtype=dtype, lane=lane, nx=nx, D=3,
                     nkey=2, uneven=True, gather='kd' if func == DET6 else '', xs=2 if lane % 2 else 1, seed=1300 + lane)
  return out


def nonfinite_cases():
  """One chosen set of non-finite points in key TARGET_KEY, chunk 0 of 4 keys x 2 chunks."""
  out = []
  shapes = {'xr': dict(nx=12, D=6, dchunk=3, uneven=True), 'xr-vec4': dict(kernel='xr', nx=12, D=6, dchunk=3, vec=4),
            'xk': dict(nx=6, D=8, dchunk=4, vec=4), 'xp': dict(nx=9, D=8, dchunk=4, R=2, contig=True, lead_walk=True, leads=(1, 2, 3, 0)),
            'xf': dict(nx=9, D=8, dchunk=4, R=4, contig=True, weights=True)}
  for tag, shape in shapes.items():
    kw = dict(dict(kernel=tag, func=DET6, nkey=4, klass='nonfinite'), **shape)
    for sp in ('nan', 'pinf', 'ninf', 'inf_pair'):
      for mode in ('plain', 'masked'):
        out.append(Case(name=_name('nf', tag, sp, mode), flags=MODES[mode], special=sp, seed=1400, **kw))
    out.append(Case(name=_name('nf', tag, 'hidden'), flags=FLAG_MASKED, special='hidden', seed=1401, **kw))
    if tag in ('xr', 'xr-vec4', 'xk'):
      for mode in ('skipna', 'masked+skipna'):
        for sp in ('c_nan', 'all_nan', 'pinf', 'inf_pair'):
          out.append(Case(name=_name('nf', tag, sp, mode), flags=MODES[mode], special=sp, seed=1402, **kw))
  for sp in ('nan', 'pinf'):
    out.append(Case(name=_name('nf-map', sp), kernel='map', func=DET6, nkey=4, klass='nonfinite', nx=12, D=6, dchunk=3, lane=5, special=sp, seed=1403))
  return out


def empty_cases():
  """nkey / ndepth / nx = 0 on the plain, the plane and the flat plans: zeros of the right length, nothing launched."""
  out = []
  for tag, kw in (('xr', dict()), ('xk', dict(keep_x=True)), ('plane', dict(R=2, contig=True, keep_x=True)), ('flat', dict(R=4, contig=True, weights=True, dchunk=4))):
    for mode in ('plain', 'masked'):
      for zero in ('nkey', 'D', 'nx'):
        dims = dict(dict(nkey=3, D=4, nx=8), **{zero: 0})
        out.append(Case(name=_name('empty', tag, mode, zero), kernel='none', func=DET6, flags=MODES[mode], klass='exact', **dict(kw, **dims)))
  return out


@dataclasses.dataclass(frozen=True)
class Refusal:
  """A valid case with ONE requirement broken: fields of the plan replaced, a pointer moved, another dtype or lane."""
  name: str
  base: str              # 'plane' | 'flat' | 'map'
  why: str               # key of REFUSED
  plan: tuple = ()       # ((field, value), ...); 'xstride1' = xstride[1]
  dtype: int = F32
  shift: tuple = ()      # ((input name, bytes), ...)
  lane: object = None


REFUSAL_BASES = {
    'plane': Case(name='refusal-base-plane', kernel='xp', func=DET6, flags=FLAG_MASKED, nkey=2, nx=64, R=2, D=4, dchunk=2, contig=True),
    'flat': Case(name='refusal-base-flat', kernel='xf', func=DET6, flags=FLAG_MASKED, nkey=2, nx=64, R=4, D=8, dchunk=4, contig=True, weights=True),
    'map': Case(name='refusal-base-map', kernel='map', func=DET3, nkey=2, nx=64, D=4, lane=2),
}


def refusals():
  F = FLAG_MASKED | FLAG_SKIPNA
  return [
      Refusal('skipna-on-plane', 'plane', 'plane_skipna', plan=(('flags', F),)),
      Refusal('skipna-on-flat', 'flat', 'flat_skipna', plan=(('flags', F),)),
      Refusal('f64-on-plane', 'plane', 'plane_f64', dtype=F64),
      Refusal('f64-on-flat', 'flat', 'flat_f64', dtype=F64),
      Refusal('weights-without-plane-rows', 'flat', 'weights_alone', plan=(('plane_rows', 0),)),
      Refusal('plane-pointer-off-16-bytes', 'plane', 'plane_inputs', shift=(('t', 4),)),
      Refusal('flat-pointer-off-16-bytes', 'flat', 'flat_inputs', shift=(('c', 8),)),
      Refusal('plane-mask-off-4-bytes', 'plane', 'plane_mask', shift=(('mask', 1),)),
      Refusal('flat-mask-off-4-bytes', 'flat', 'flat_mask', shift=(('mask', 2),)),
      Refusal('plane-xstride-2', 'plane', 'plane_inputs', plan=(('xstride1', 2),)),
      Refusal('flat-xstride-0', 'flat', 'flat_inputs', plan=(('xstride1', 0),)),
      Refusal('plane-mask-xstride-0', 'plane', 'plane_mask', plan=(('xstride3', 0),)),
      Refusal('plane-with-x-summed', 'plane', 'plane_shape', plan=(('x_kept', False),)),
      Refusal('plane-nx-1025', 'plane', 'plane_shape', plan=(('nx', 1025),)),
      Refusal('plane-rows-over-the-block', 'plane', 'plane_block', plan=(('plane_rows', 8), ('nchunk', 1), ('depth_chunk', 4))),  # (8 * 64 + 6) / 4 = 129 > 128
      # nx = 1024, R = 7: nvec = 1793 <= 2048, 3 * (7168 + 8) * 4 + 7184 = 93296 B
      Refusal('plane-lds-over-80-kib', 'plane', 'plane_lds', plan=(('nx', 1024), ('plane_rows', 7), ('nchunk', 1), ('depth_chunk', 4))),
      Refusal('plane-chunk-not-whole-groups', 'plane', 'plane_chunks', plan=(('plane_rows', 3),)),
      Refusal('flat-with-x-kept', 'flat', 'flat_shape', plan=(('x_kept', True),)),
      Refusal('flat-rows-not-quads', 'flat', 'flat_shape', plan=(('plane_rows', 2),)),
      Refusal('flat-nx-2046', 'flat', 'flat_shape', plan=(('nx', 2046),)),
      Refusal('flat-chunk-not-quads', 'flat', 'flat_chunks', plan=(('depth_chunk', 6), ('nchunk', 2))),
      Refusal('flat-depth-not-whole-planes', 'flat', 'flat_chunks', plan=(('plane_rows', 16), ('depth_chunk', 8), ('nchunk', 1))),
      Refusal('map-lane-out-of-range', 'map', 'map_lane', lane=3),
      Refusal('map-lane-negative', 'map', 'map_lane', lane=-1),
  ]


def refused_plan(plan, ref):
  """A copy of `plan` (the tables shared) with the refusal's fields replaced."""
  new = dataclasses.replace(plan, xstride=list(plan.xstride))
  for field, value in ref.plan:
    if field.startswith('xstride'):
      new.xstride[int(field[-1])] = value
    else:
      setattr(new, field, value)
  return new


def partial_cases():
  """Every case of wbx_det_partial that is compared output by output."""
  pairs = [c for pair in xr_mrow_pair() for c in pair]
  return xr_matrix_cases() + xr_shape_cases() + xr_address_cases() + xr_mrow_cases() + pairs + xk_cases() + xp_cases() + xf_cases()


def all_cases():
  twins = [t for _, t in xp_route_twins() + xf_route_twins()]
  return partial_cases() + twins + map_cases() + nonfinite_cases() + empty_cases()
