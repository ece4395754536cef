"""Inputs, the float64 expectation, the per-output error bounds and the restated geometry for the fused binned ensemble reduction
(wbx_ens_binned: binned_atoms_kernel, aid_merge_kernel / aid_merge_points_kernel, ens_atoms_kernel), plain NumPy:
tests/test_gpu_ens_binned.py runs every case on the GPU, tests/test_ens_binned_cases.py holds the cases themselves on the CPU.

Frame.  Dims (a, bk, br, d, x): `a` kept, `bk` kept and W-dependent, `br` reduced and W-dependent, `d` reduced only, `x` reduced and
summed (W-dependent unless the case says `w_on_x = False`).  A cell is (a, bk), a row of a cell is r = br * D + d.  The members are
stored [a][m][bk][br][d][x] ('member_outside') or [m][a][bk][br][d][x] ('ifs'), with `d` outside `bk` where the case says `d_outer`,
with an x stride of 1 or 2 (the gaps of a strided row hold NaN); the targets alike, or one value per row (x stride 0).

Expectation (`expected`).  The five lanes per point are ensemble_cases.expected_lanes for the `binned` family of that M (the float64
oracle on the widened inputs + the conventions of include/wbx.h), times the factored weight w_x[bk][x] * w_row[bk][br] (one factor is
1), summed over the valid points of each cell with the 0.0 / 1.0 membership factor: a term that is not finite under a valid point
turns its lane NaN in EVERY bin of its cell (NaN x 0), whatever the point's membership.  The sums run in extended precision
(numpy.longdouble, 2^-64) grouped by membership word, and are rounded to float64 once.  Laid out as include/wbx.h documents:
  6 lanes            the five lanes + the count lane (the sum of the weights of the valid points of the bin)
  12 lanes (twin)    the six with the mask applied, then the six over ALL points
  10 lanes (skipna)  five values and their five counts; skill, unbiased MSE and MSE of the mean leave out the points with a NaN target
                     or a NaN / infinite member, spread and variance those with a NaN / infinite member, whatever the target
  20 lanes (skipna + twin)  the ten over the valid points of the mask with lanes 1, 2 NaN, then the ten over all points with lanes 0, 3,
                     4 NaN (`Expected.layout_nan`); the count lanes of a NaN lane repeat those of its ten's live lanes
A count lane never turns NaN: it sums weights.

Bound (`Expected.bound`, per output; derived from the arithmetic, never from what a kernel gives):
    sum_i w_i * lane_bounds_i + (N + 4) 2^-53 sum_i |w_i lane_i|,   N = the points of the cell that are valid and in the bin
  * the first term is the error of the kernel's per-point values (ensemble_cases.lane_bounds: fp64 sums in the register buckets, fp32
    chains at M = 50 / 51), which the weighted sum passes on linearly;
  * the second holds in ANY order of the sums -- a lane's fma chain down its column, the DPP wave sums of a flush, the adds into a
    touched table row, the three levels over patches: every rounded addition merges two non-empty sets of the bin's N terms, so there
    are at most N - 1 of them, each erring by at most 2^-53 of the sum of the magnitudes; an added zero (a lane outside the group, a
    word outside the bin) rounds nothing.  The rest covers the final rounding of the expectation and second-order terms;
  * lane 3 is formed per (group of patches, word) as lane 4 - lane 2 / M from the sums: its bound is lane 4's plus lane 2's / M plus
    4 x 2^-53 (sum |w lane 4| + sum |w lane 2| / M) for the rounding of 1 / M, of the product and of the difference;
  * count lanes: B = 0, the same (N + 4) 2^-53 sum w.  With dyadic weights (the 'dyadic' value family, and wt = NULL) every partial
    sum of weights is exact and the count lanes are compared bit for bit (`Expected.exact`); so is lane 0 of the 'dyadic' family at a
    power-of-two M (|x - t| on a grid of 0.25, the sum, 1 / M and the weight k / 8 are all exact in float64).
An output whose expectation is NaN is compared by class and position; no case here makes an infinite output (an infinite member is
poisoned to NaN by the rank form, an infinite target is left to the per-point tests of tests/test_gpu_ensemble_points.py: its lanes
would be +inf in some bins and NaN in the others by the NaN x 0 rule, which the documented NaN rule of wbx_det_binned words).

Geometry (`geometry`): patch_geometry with rows_hint = ENS_ATOMS_ROWS = 16 and patch_taper of csrc/wbx_patch.hpp restated, the group
sizes ENS_ATOMS_G1 = 4 / ENS_ATOMS_G2 = 16 and ATOM_MAX = 32 of csrc/wbx_ens_atoms.hpp, the route rule of launch_ens_atoms (`ragged`),
atoms_carve (`Geometry.atoms_bytes`, held against wbx_ens_binned_atoms_size on the GPU) and the lane bookkeeping of ens_atoms_patch
(`flush_profile`: how often a wave flushes mid-patch and whether a flush adds into a table row that was written before)."""
import dataclasses
import functools
import types

import numpy as np

import ensemble_cases as EC

FLAG_MASKED, FLAG_SKIPNA, FLAG_FAIR = 1, 2, 4
W_ON_X, WT_X_ONLY, WT_ROW_ONLY, MASK_ON_W, TWIN_MASK, ACCUMULATE = 1, 2, 4, 8, 16, 32
DIMS = ('a', 'bk', 'br', 'd', 'x')
ROWS_HINT, G1, G2, ATOM_MAX, SPLIT_MAX = 16, 4, 16, 32, 255
U = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -60, 'the expectation sums in extended precision'

# name -> (plan flags, WBX_BINNED_* flags, the mask: None | 'w' (on bk, br, x) | 'point' (strides along a and d too))
MODES = {
    'plain': (0, 0, None),
    'masked-w': (FLAG_MASKED, MASK_ON_W, 'w'),
    'masked-w-twin': (FLAG_MASKED, MASK_ON_W | TWIN_MASK, 'w'),
    'masked-pt': (FLAG_MASKED, 0, 'point'),
    'masked-pt-twin': (FLAG_MASKED, TWIN_MASK, 'point'),
    'skipna': (FLAG_SKIPNA, 0, None),
    'skipna-masked-w': (FLAG_SKIPNA | FLAG_MASKED, MASK_ON_W, 'w'),
    'skipna-masked-pt': (FLAG_SKIPNA | FLAG_MASKED, 0, 'point'),
    'skipna-masked-w-twin': (FLAG_SKIPNA | FLAG_MASKED, MASK_ON_W | TWIN_MASK, 'w'),
    'skipna-masked-pt-twin': (FLAG_SKIPNA | FLAG_MASKED, TWIN_MASK, 'point'),
}
MODE_NAMES = tuple(MODES)
# the register buckets of launch_ens_atoms_m* (wbx_ens_binned) and the member counts that run in each
BUCKETS = {'m4': (2, 4), 'm8': (5, 8), 'm16': (9, 16), 'm32': (17, 32), 'm64': (33, 64), 'm50': (50,), 'm51': (51,)}
BUCKET_NAMES = tuple(BUCKETS)
MEMBER_COUNTS = (2, 4, 5, 8, 9, 16, 17, 32, 33, 50, 51, 64)
VALUES = ('dyadic', 'anomaly', 'cancel')  # (test_gpu_ensemble_points.VALUES)
LAYOUTS = ('member_outside', 'ifs')
WEIGHTS = ('row', 'x', 'null')
PATTERNS = ('boxes', 'row-stripes', 'checker')
SPECIAL_KINDS = ('nan_member', 'pinf_member', 'nan_target')
SPECIAL_PLACES = ('valid', 'masked_out', 'no_bin', 'tail')


def bucket_of(m):
  if m in (50, 51):
    return f'm{m}'
  return next(b for b in ('m4', 'm8', 'm16', 'm32', 'm64') if m <= max(BUCKETS[b]))


def kernel_mode(mode):
  """The MODE template argument launch_ens_atoms picks: 2 under skipna, 1 for a per-point mask, else 0."""
  flags, _, kind = MODES[mode]
  return 2 if flags & FLAG_SKIPNA else (1 if kind == 'point' else 0)


def lanes_total(mode):
  flags, bflags, _ = MODES[mode]
  return (10 if flags & FLAG_SKIPNA else 6) * (2 if bflags & TWIN_MASK else 1)


@dataclasses.dataclass(frozen=True)
class Case:
  """One launch."""
  name: str
  mode: str = 'plain'
  M: int = 8
  fair: bool = True
  nA: int = 2
  nBk: int = 1
  nBr: int = 5
  D: int = 1
  nx: int = 130
  layout: str = 'member_outside'
  p_xs: int = 1            # x stride of the members (2: every second element of a row twice as long)
  t_xs: int = 1            # x stride of the targets (0: one target per row)
  d_outer: bool = False    # p, t and a per-point mask are stored with d outside bk / br
  values: str = 'anomaly'
  wl: str = 'row'          # 'row' wt[nBk][nBr] (WT_ROW_ONLY) | 'x' wt[nBk][nx] (WT_X_ONLY) | 'null' (wt = NULL: ones)
  w_on_x: bool = True      # False: bits[nBk][nBr][1] (nj = 1)
  bins: str = 'boxes'
  nbin: int = 6
  special: bool = False    # one special point (SPECIAL_KINDS x SPECIAL_PLACES) in each of the first twelve cells
  geom: str = ''           # the geometry the case is named for (geometry_property holds it to the restated rules)
  seed: int = 0

  @property
  def nj(self):
    return self.nx if self.w_on_x else 1

  @property
  def ncell(self):
    return self.nA * self.nBk

  @property
  def R(self):
    return self.nBr * self.D

  @property
  def plan_flags(self):
    return MODES[self.mode][0] | (FLAG_FAIR if self.fair else 0)

  @property
  def w_flags(self):
    return (W_ON_X if self.w_on_x else 0) | {'row': WT_ROW_ONLY, 'x': WT_X_ONLY, 'null': 0}[self.wl] | MODES[self.mode][1]

  @property
  def ragged(self):
    """launch_ens_atoms: rows that are not whole 128-byte lines, or strided -> four waves per block, no non-temporal loads."""
    return (self.nx * self.p_xs * 4) % 128 != 0 or self.p_xs != 1

  @property
  def dyadic_weights(self):
    return self.values == 'dyadic' or self.wl == 'null'


# ---------------------------------------------------------------------------------------------------------------------
# geometry


def patch_taper(nBr, s0):
  """patch_taper of wbx_patch.hpp -> the split table [nrs + 1] in Br rows, or None where the uniform splits stay."""
  if s0 < 4 or nBr < 8 * 2 * s0:
    return None
  longest = (nBr + 7) // 8
  sizes, done = [], 0
  half, quarter = s0 // 2, s0 // 4
  while (done + s0) * 10 <= longest * 7:
    sizes.append(s0)
    done += s0
  while (done + half) * 10 <= longest * 9:
    sizes.append(half)
    done += half
  while done + quarter <= longest:
    sizes.append(quarter)
    done += quarter
  if done < longest:
    sizes.append(longest - done)
  if not sizes or sizes[0] < 2:
    return None
  per = len(sizes)
  if per * 8 > SPLIT_MAX:
    return None
  tab, at = [], 0
  for seg in range(8):
    shave = longest - (nBr // 8 + (1 if seg < nBr % 8 else 0))
    for i, n in enumerate(sizes):
      tab.append(at)
      at += n - (shave if i == 0 else 0)
  tab.append(at)
  return tuple(tab) if at == nBr else None


@dataclasses.dataclass(frozen=True)
class Geometry:
  nBk: int
  nBr: int
  nj: int
  D: int
  nx: int
  nxt: int
  nrs: int
  rows_per_split: int
  taper: bool
  split_br: tuple  # [nrs + 1]: split rs = Br rows [split_br[rs], split_br[rs + 1])

  @property
  def npatch(self):
    return self.nrs * self.nxt

  @property
  def ng1(self):
    return -(-self.npatch // G1)

  @property
  def ng2(self):
    return -(-self.ng1 // G2)

  @property
  def atoms_bytes(self):
    """atoms_carve: uni | words | nwords | aid | the split table of a tapered geometry, each padded to 8 bytes."""
    n = self.nBk * self.npatch
    return (n + n * ATOM_MAX + (n + 1) // 2 + (self.nBk * self.nBr * self.nj + 7) // 8 + ((SPLIT_MAX + 2) // 2 if self.taper else 0)) * 8

  def live(self, xt):
    return min(64, self.nx - 64 * xt)

  def words(self, bits):
    """bits[nBk][nBr][nj] -> the number of distinct membership words of every patch, [nBk][nrs][nxt] (live x only)."""
    bits = np.asarray(bits, np.uint64).reshape(self.nBk, self.nBr, self.nj)
    out = np.zeros((self.nBk, self.nrs, self.nxt), np.int64)
    for rs in range(self.nrs):
      for xt in range(self.nxt):
        xs = slice(xt * 64, xt * 64 + self.live(xt)) if self.nj > 1 else slice(0, 1)
        for bk in range(self.nBk):
          out[bk, rs, xt] = np.unique(bits[bk, self.split_br[rs]:self.split_br[rs + 1], xs]).size
    return out


def geometry(nBk, nBr, nj, D, nx):
  """patch_geometry(rows_hint = 16) + patch_taper: the patches of one cell (they do not depend on the number of cells)."""
  rows = nBr * D
  nxt = (nx + 63) // 64
  want = (rows + ROWS_HINT - 1) // ROWS_HINT
  rps = (rows + want - 1) // want
  rps = (rps + D - 1) // D * D
  nrs = (rows + rps - 1) // rps
  tab = patch_taper(nBr, rps // D)
  taper = tab is not None
  if taper:
    nrs = len(tab) - 1
  else:
    tab = tuple(min(rs * (rps // D), nBr) for rs in range(nrs + 1))
  return Geometry(nBk=nBk, nBr=nBr, nj=nj, D=D, nx=nx, nxt=nxt, nrs=nrs, rows_per_split=rps, taper=taper, split_br=tab)


def geometry_of(case):
  return geometry(case.nBk, case.nBr, case.nj, case.D, case.nx)


def geometry_property(case):
  """Asserts from the restated rules that `case` has the property its `geom` names; -> the Geometry."""
  g = geometry_of(case)
  sizes = [b - a for a, b in zip(g.split_br, g.split_br[1:])]
  assert all(n >= 1 for n in sizes) and g.split_br[0] == 0 and g.split_br[-1] == case.nBr, g
  name = case.geom
  if name == 'one-patch':
    assert g.npatch == 1 and g.ng1 == 1 and not case.ragged and not g.taper, g
  elif name == 'ragged-3-tiles':
    # one four-wave block per (cell, row split): its fourth wave has no patch; the last tile has 2 live lanes; one group of 3
    assert case.ragged and g.nxt == 3 and g.nrs == 1 and g.live(2) == 2 and g.ng1 == 1 and g.npatch == 3, g
  elif name == 'strided-x':
    assert case.p_xs == 2 and (case.nx * 4) % 128 == 0 and case.ragged, g
  elif name == 'target-without-x':
    assert case.t_xs == 0, case
  elif name in ('two-level-2-groups', 'two-level-2-groups-ragged'):
    assert case.D == 1 and not g.taper and g.ng2 == 2 and g.ng1 % G2 not in (0, 1) and g.ng1 > G2, g
    assert case.ragged == (name == 'two-level-2-groups-ragged'), g
    if name == 'two-level-2-groups':
      assert (g.nrs, g.nxt, g.npatch, g.ng1) == (9, 8, 72, 18), g  # 9 splits x 8 tiles; the last level-2 group has 2 records
  elif name == 'tapered':
    per = g.nrs // 8
    assert g.taper and case.D > 1 and g.nrs == 8 * per, g
    assert case.nBr % 8 != 0, 'some segment is one Br row short: its first split is shaved'
    first = [sizes[seg * per] for seg in range(8)]
    assert len(set(first)) == 2 and max(first) - min(first) == 1, first
    assert len(set(sizes[:per])) >= 3, ('full, half and quarter splits', sizes[:per])
    if (case.nBr, case.D) == (70, 4):
      assert sizes[:4] == [4, 2, 2, 1] and first == [4] * 6 + [3] * 2 and g.rows_per_split == 16, sizes
  elif name == 'depth-2-untapered':
    assert case.D == 2 and not g.taper and g.nrs >= 2 and g.rows_per_split % case.D == 0, g
  elif name == 'nBk-3':
    assert case.nBk == 3 and case.nA >= 2
  elif name == 'nj-1':
    assert case.nj == 1 and MODES[case.mode][2] is None
  elif name == 'nbin-64':
    assert case.nbin == 64
  elif name == 'nbin-1':
    assert case.nbin == 1
  else:
    raise ValueError(name)
  return g


# ---------------------------------------------------------------------------------------------------------------------
# bins


def make_bits(case):
  """-> bits[nBk][nBr][nj] uint64"""
  nBk, nBr, nj, nbin = case.nBk, case.nBr, case.nj, case.nbin
  bk = np.arange(nBk, dtype=np.int64)[:, None, None]
  br = np.arange(nBr, dtype=np.int64)[None, :, None]
  x = np.arange(nj, dtype=np.int64)[None, None, :]
  shape = (nBk, nBr, nj)
  one = np.uint64(1)
  kind = case.bins
  if kind == 'boxes':
    # nbin - 1 boxes that overlap (a third of the row wide, half of the rows high, wrapping along x) and one 'global' bin with
    # holes: there are points in no bin, in one and in several
    bits = np.zeros(shape, np.uint64)
    for b in range(nbin - 1):
      r0 = (b * nBr) // nbin
      x0 = (b * 37 + 11 * bk) % max(nj, 1)
      inside = (br >= r0) & (br < r0 + max(nBr // 2, 1)) & (((x - x0) % max(nj, 1)) < max(nj // 3, 1))
      bits |= np.broadcast_to(inside, shape).astype(np.uint64) << np.uint64(b)
    hole = ((br + bk) % 3 == 1) & (x % 16 < 5)
    bits |= np.broadcast_to(~hole, shape).astype(np.uint64) << np.uint64(nbin - 1)
    return bits
  if kind == 'row-stripes':  # three words cycling row by row: every lane meets a third atom every third row
    words = np.array([0b0011, 0b0110, 0b1101], np.uint64)
    return np.broadcast_to(words[(br + bk) % 3], shape).copy()
  if kind == 'checker':  # four words alternating along x and along the rows
    words = np.array([0b0001, 0b0010, 0b0100, 0b1001], np.uint64)
    return np.broadcast_to(words[((br + bk) % 2) * 2 + x % 2], shape).copy()
  if kind == 'exactly-32-words':  # nbin = 5: the word IS the value 0 .. 31; a tile of 64 x meets all 32, and a new one every row
    return np.broadcast_to(((x // 2 + br + bk) % 32).astype(np.uint64), shape).copy()
  if kind == '33-words':  # nbin = 6; bk = 0 as above, every whole tile of bk >= 1 meets 33 words
    v = np.where(bk == 0, (x // 2 + br) % 32, ((x % 64) * 33 // 64 + br) % 33)
    return np.broadcast_to(v.astype(np.uint64), shape).copy()
  if kind == 'bits-64':  # 16 words of four bins each, bit 63 among them
    v = ((x // 4 + br + bk) % 16).astype(np.uint64)
    w = np.zeros(np.broadcast(v, np.empty(shape)).shape, np.uint64)
    for j in range(4):
      w |= one << (v + np.uint64(16 * j))
    return np.broadcast_to(w, shape).copy()
  if kind == 'bit-0':
    return np.broadcast_to(((x + br + bk) % 3 != 0).astype(np.uint64), shape).copy()
  raise ValueError(kind)


def member_of(words, nbin):
  """words[...] -> bool [..., nbin]"""
  return ((np.asarray(words, np.uint64)[..., None] >> np.arange(nbin, dtype=np.uint64)) & np.uint64(1)).astype(bool)


# ---------------------------------------------------------------------------------------------------------------------
# inputs


def _store(logical, dims, order, xs=1, fill=None):
  """logical indexed by `dims` (x last) -> (flat storage in `order`, element strides by dim): an x stride of 2 leaves gaps that hold
  `fill`; an x stride of 0 keeps one element per row."""
  perm = [dims.index(d) for d in order]
  arr = np.transpose(logical, perm)
  assert order[-1] == 'x'
  if xs == 0:
    st = np.ascontiguousarray(arr[..., :1])
  elif xs == 1:
    st = np.ascontiguousarray(arr)
  else:
    st = np.full(arr.shape[:-1] + (arr.shape[-1] * xs,), fill, arr.dtype)
    st[..., ::xs] = arr
  strides = {d: s // st.itemsize for d, s in zip(order, st.strides)}
  strides['x'] = xs
  for d, n in zip(order, arr.shape):
    if n == 1 and d != 'x':
      strides[d] = 0
  return st.reshape(-1), strides


def build(case):
  """-> namespace: P[cell, M, R, nx] / T[cell, R, nx] float32 as the kernel indexes them (cell = a * nBk + bk, R = nBr * D rows),
  valid[cell, R, nx] bool, W[nBk, R, nx] (the weight of every point), wt (as handed over, or None), bits[nBk][nBr][nj],
  words[nBk, R, nx] (every point's membership word), store[name] = (flat array, element strides), mstride, special =
  {cell: (kind, place, r, x)}."""
  rng = np.random.default_rng(4000 + case.seed)
  nA, nBk, nBr, D, nx, nj, M = case.nA, case.nBk, case.nBr, case.D, case.nx, case.nj, case.M
  ncell, R = case.ncell, case.R
  P, T, _ = EC.dense_case(9000 + case.seed, M, ncell, R, nx, values=case.values)
  P, T = np.ascontiguousarray(P), np.ascontiguousarray(T)
  if case.t_xs == 0:  # one target per row: the kernel reads the same element for every x
    T = np.ascontiguousarray(np.broadcast_to(T[:, :, :1], T.shape))
    if case.values == 'cancel':
      T = np.ascontiguousarray(np.broadcast_to(P.astype(np.float64).mean(axis=(1, 3))[:, :, None], T.shape).astype(np.float32))
  bits = make_bits(case)
  kind = MODES[case.mode][2]
  mask = None
  if kind == 'w':
    mask = (rng.random((1, nBk, nBr, 1, nx)) > 0.3).astype(np.uint8)
  elif kind == 'point':
    mask = (rng.random((nA, nBk, nBr, D, nx)) > 0.3).astype(np.uint8)
  skipna = bool(MODES[case.mode][0] & FLAG_SKIPNA)
  if skipna and not case.special:  # 3 % NaN targets, 3 % NaN members, 1 % infinite members (counted out like NaN)
    T[rng.random(T.shape) < 0.03] = np.nan
    u = rng.random(T.shape)
    mi = rng.integers(0, M, size=T.shape)
    ci, ri, xi = np.nonzero(u < 0.04)
    P[ci, mi[ci, ri, xi], ri, xi] = np.where(u[ci, ri, xi] < 0.03, np.nan, np.inf).astype(np.float32)
  elif mask is not None and not case.special:  # NaN members that the mask hides: no trace in lanes 0-5
    hide = (rng.random(T.shape) < 0.1) & (np.broadcast_to(mask, (nA, nBk, nBr, D, nx)).reshape(ncell, R, nx) == 0)
    if not MODES[case.mode][1] & TWIN_MASK:  # (with twin output they would turn lanes 6-10 NaN: the special cases hold that)
      P[:, 0][hide] = np.nan

  special = {}
  if case.special:
    assert ncell >= 14 and R >= 3 and nx > 70
    kinds = {k[0]: k for k in EC.live_points(M)}
    places = {'valid': (1, 5), 'masked_out': (R - 2, 66), 'no_bin': (0, 17), 'tail': (R - 1, nx - 1)}
    for i, (k, pl) in enumerate((k, pl) for k in SPECIAL_KINDS for pl in SPECIAL_PLACES):
      r, x = places[pl]
      P[i, :, r, x], T[i, r, x] = kinds[k][1], kinds[k][2]
      special[i] = (k, pl, r, x)
    for pl, (r, x) in places.items():
      br, xj = r // D, (x if nj > 1 else 0)
      if mask is not None:  # (the same place in every cell: a mask on the W dims is shared by them)
        mask[:, :, br, :, x] = 0 if pl == 'masked_out' else 1
      if pl == 'no_bin':
        bits[:, br, xj] = 0
  valid = np.ones((ncell, R, nx), bool) if mask is None else (np.broadcast_to(mask, (nA, nBk, nBr, D, nx)).reshape(ncell, R, nx) != 0)

  if case.wl == 'null':
    wt, W = None, np.ones((nBk, nBr, nx))
  else:
    n = nBk * (nBr if case.wl == 'row' else nx)
    w = rng.integers(1, 17, size=n) / 8.0 if case.values == 'dyadic' else 0.5 + (rng.permutation(n) + rng.random(n)) / n
    wt = w.reshape(nBk, -1)
    W = np.broadcast_to(wt[:, :, None] if case.wl == 'row' else wt[:, None, :], (nBk, nBr, nx))
  assert case.w_on_x or case.wl != 'x'
  W = np.ascontiguousarray(np.repeat(W, D, axis=1))  # [nBk, R, nx]
  words = np.ascontiguousarray(np.repeat(np.broadcast_to(bits, (nBk, nBr, nx)), D, axis=1))

  order = ('a', 'd', 'bk', 'br', 'x') if case.d_outer else DIMS
  p6 = P.reshape(nA, nBk, M, nBr, D, nx)
  porder = tuple(o for o in order if o != 'x')
  porder = (('m',) + porder if case.layout == 'ifs' else (porder[0], 'm') + porder[1:]) + ('x',)
  pflat, pst = _store(p6, ('a', 'bk', 'm', 'br', 'd', 'x'), porder, case.p_xs, np.nan)
  mstride = pst.pop('m')
  store = {'p': (pflat, pst), 't': _store(T.reshape(nA, nBk, nBr, D, nx), DIMS, order, case.t_xs, np.nan)}
  if mask is not None:
    mflat, mst = _store(mask, DIMS, order if kind == 'point' else DIMS)
    if kind == 'w':
      mst['a'] = mst['d'] = 0
    store['mask'] = (mflat, mst)
  return types.SimpleNamespace(case=case, P=P, T=T, valid=valid, W=W, wt=None if wt is None else np.ascontiguousarray(wt), bits=np.ascontiguousarray(bits),
                               words=words, store=store, mstride=int(mstride), special=special, geometry=geometry_of(case))


def plan_for(inp, flags=None):
  """build_s1_plan(dims, sizes, layouts, reduce_dims = (br, d, x), wdep_dims = {bk, br[, x]}, force_x_dim = x, allow_vec4 = False)."""
  from weatherbenchx_amd import planner  # pylint: disable=g-import-not-at-top
  case = inp.case
  sizes = dict(zip(DIMS, (case.nA, case.nBk, case.nBr, case.D, case.nx)))
  layouts = []
  for name in ('p', 't', 'c', 'mask'):
    if name in inp.store:
      flat, st = inp.store[name]
      layouts.append(planner.InputLayout(strides=dict(st), itemsize=flat.itemsize, base_alignment=256))
    else:
      layouts.append(None)
  wdep = {'bk', 'br', 'x'} if case.w_on_x else {'bk', 'br'}
  plan = planner.build_s1_plan(DIMS, sizes, layouts, reduce_dims=('br', 'd', 'x'), wdep_dims=wdep, flags=case.plan_flags if flags is None else flags,
                               allow_vec4=False, force_x_dim='x')
  assert plan.a_dims == ('a',) and plan.bk_dims == ('bk',) and plan.br_dims == ('br',) and plan.depth_dims == ('d',), plan
  assert plan.nkey == case.nA * case.nBk * case.nBr and plan.ndepth == case.D and plan.nx == case.nx, plan
  return plan


def read_back(inp, name):
  """What strides + member stride address of input `name`, as the kernel indexes it: P[cell, M, R, nx], T / mask [cell, R, nx]."""
  case = inp.case
  flat, st = inp.store[name]
  off = np.zeros((), np.int64)
  for d, n in zip(DIMS, (case.nA, case.nBk, case.nBr, case.D, case.nx)):
    off = off[..., None] + np.arange(n, dtype=np.int64) * st.get(d, 0)
  off = off.reshape(case.ncell, case.R, case.nx)
  if name == 'p':
    off = off[:, None] + (np.arange(case.M, dtype=np.int64) * inp.mstride)[None, :, None, None]
  assert off.min() >= 0 and off.max() < flat.size, (name, off.min(), off.max(), flat.size)
  return flat[off]


# ---------------------------------------------------------------------------------------------------------------------
# expectation


@dataclasses.dataclass
class Expected:
  want: np.ndarray        # [nA][nBk][lanes_total][nbin]
  bound: np.ndarray       # same shape (0 where the output is compared exactly or by class)
  exact: np.ndarray       # bool: compared bit for bit
  layout_nan: np.ndarray  # bool [lanes_total]: the lanes include/wbx.h documents as NaN (skipna + twin)
  nterms: np.ndarray      # the N of the bound
  scale: np.ndarray       # sum |w lane| over the same points


def point_selections(inp):
  """-> (bad, tnan): the points with a NaN / infinite member, with a NaN target, [cell, R, nx]."""
  return ~np.isfinite(inp.P).all(axis=1), np.isnan(inp.T)


def expected(inp):
  case = inp.case
  M, nbin, ncell, nBk = case.M, case.nbin, case.ncell, case.nBk
  fam = EC.family('binned', M, np.float32)
  stat = EC.expected_lanes(fam, inp.P, inp.T, case.fair)  # [cell, R, nx, 5]
  lb = EC.lane_bounds(fam, inp.P, inp.T, stat)
  flags, bflags, _ = MODES[case.mode]
  skipna, twin = bool(flags & FLAG_SKIPNA), bool(bflags & TWIN_MASK)
  bad, tnan = point_selections(inp)
  everything = np.ones_like(inp.valid)
  nlt = lanes_total(case.mode)
  want = np.empty((ncell, nlt, nbin))
  bound = np.zeros_like(want)
  nterms = np.zeros_like(want)
  scale = np.zeros_like(want)
  exact = np.zeros(want.shape, bool)
  layout_nan = np.zeros(nlt, bool)
  pow2 = M & (M - 1) == 0

  # every point's word -> its index among the distinct words of its bk, the order that groups the points by word
  groups = []
  for bk in range(nBk):
    uniq, inv = np.unique(inp.words[bk].reshape(-1), return_inverse=True)
    order = np.argsort(inv, kind='stable')
    starts = np.searchsorted(inv[order], np.arange(uniq.size))
    groups.append((member_of(uniq, nbin).astype(np.float64), inv.reshape(-1), order, starts))

  def sums(cell, sel, lane):
    """-> (want[nbin] or all NaN, sum w lb, sum |w v|, N) of `lane` (None: the count lane) over the points `sel` of the cell."""
    memf, inv, order, starts = groups[cell % nBk]
    s = sel[cell].reshape(-1)
    w = inp.W[cell % nBk].reshape(-1)
    nw = memf.shape[0]
    n = np.bincount(inv, weights=s.astype(np.float64), minlength=nw) @ memf
    if lane is None:
      term = np.where(s, w, 0.0)
      b = np.zeros(nbin)
    else:
      v = stat[cell, :, :, lane].reshape(-1)
      if not np.isfinite(v[s]).all():
        return np.full(nbin, np.nan), None, None, n
      term = np.where(s, v, 0.0).astype(LD) * w.astype(LD)
      b = np.bincount(inv, weights=np.where(s, lb[cell, :, :, lane].reshape(-1) * w, 0.0), minlength=nw) @ memf
    per_word = np.add.reduceat(np.asarray(term, LD)[order], starts)
    tot = (per_word[:, None] * memf.astype(LD)).sum(axis=0)
    a = np.bincount(inv, weights=np.abs(np.asarray(term, np.float64)), minlength=nw) @ memf
    return np.asarray(tot, np.float64), b, a, n

  def six(cell, sel_t, sel_m, at, count_at=None):
    """Lanes at .. at + 4 (and the count lane(s)) of one selection pair: the target lanes over sel_t, spread / variance over sel_m."""
    parts = {}
    for l in range(5):
      parts[l] = sums(cell, sel_m if l in (1, 2) else sel_t, l)
    v2t = parts[2] if sel_m is sel_t else sums(cell, sel_t, 2)  # (lane 3 is formed from the variance sum over the TARGET selection)
    for l in range(5):
      w_, b, a, n = parts[l]
      want[cell, at + l] = w_
      nterms[cell, at + l] = n
      if b is None:
        continue
      scale[cell, at + l] = a
      bound[cell, at + l] = b + (n + 4) * U * a
      if l == 0 and case.values == 'dyadic' and pow2 and case.dyadic_weights:
        exact[cell, at + l] = True
    if parts[4][1] is not None and v2t[1] is not None and parts[3][1] is not None:
      b4 = parts[4][1] + (parts[4][3] + 4) * U * parts[4][2]
      b2 = v2t[1] + (v2t[3] + 4) * U * v2t[2]
      bound[cell, at + 3] = b4 + b2 / M + 4 * U * (parts[4][2] + v2t[2] / M)
      scale[cell, at + 3] = parts[4][2] + v2t[2] / M
    return parts

  def count(cell, sel, at):
    w_, _, a, n = sums(cell, sel, None)
    want[cell, at] = w_
    nterms[cell, at] = n
    scale[cell, at] = a
    bound[cell, at] = (n + 4) * U * a
    exact[cell, at] = case.dyadic_weights

  with np.errstate(all='ignore'):
    for cell in range(ncell):
      if not skipna:
        six(cell, inp.valid, inp.valid, 0)
        count(cell, inp.valid, 5)
        if twin:
          six(cell, everything, everything, 6)
          count(cell, everything, 11)
      else:
        ok_m = inp.valid & ~bad
        ok_t = ok_m & ~tnan
        six(cell, ok_t, ok_m, 0)
        for l in range(5):
          count(cell, ok_m if (l in (1, 2) and not twin) else ok_t, 5 + l)
        if twin:
          all_m = ~bad
          six(cell, all_m & ~tnan, all_m, 10)
          for l in range(5):
            count(cell, all_m, 15 + l)
  if skipna and twin:
    layout_nan[[1, 2, 10, 13, 14]] = True
    want[:, layout_nan] = np.nan
    bound[:, layout_nan] = 0.0
    exact[:, layout_nan] = False
  bound[exact] = 0.0
  bound[np.isnan(want)] = 0.0
  shape = (case.nA, case.nBk, nlt, nbin)
  return Expected(want=want.reshape(shape), bound=bound.reshape(shape), exact=exact.reshape(shape), layout_nan=layout_nan, nterms=nterms.reshape(shape),
                  scale=scale.reshape(shape))


def special_effects(mode, kind, place):
  """include/wbx.h in words, for one special point (SPECIAL_KINDS x SPECIAL_PLACES) of a cell -> dict(nan = the output lanes that are
  NaN in every bin of the cell, drops = the count lanes that lose the point's weight in the bins it is in).  A NaN target makes skill,
  unbiased MSE and MSE of the mean NaN, a NaN / infinite member all five; a point the mask hides is in no sum of the masked lanes,
  but with twin output it is in every sum of the unmasked ones."""
  flags, bflags, mkind = MODES[mode]
  skipna, twin = bool(flags & FLAG_SKIPNA), bool(bflags & TWIN_MASK)
  lanes = {0, 3, 4} if kind == 'nan_target' else {0, 1, 2, 3, 4}
  hidden = mkind is not None and place == 'masked_out'
  nan, drops = set(), set()
  if not skipna:
    if not hidden:
      nan |= lanes
    if twin:
      nan |= {6 + l for l in lanes}
  elif not twin:
    if not hidden:
      drops |= {5 + l for l in lanes}
  else:  # the first ten count the points every target statistic is valid at, the second ten those with valid members
    if not hidden:
      drops |= {5, 6, 7, 8, 9}
    if kind != 'nan_target':
      drops |= {15, 16, 17, 18, 19}
  return dict(nan=nan, drops=drops)


@functools.lru_cache(maxsize=None)
def prepared(case):
  """-> (inputs, Expected), computed once per session and left unchanged."""
  inp = build(case)
  return inp, expected(inp)


# ---------------------------------------------------------------------------------------------------------------------
# the lane bookkeeping of ens_atoms_patch restated


def flush_profile(inp):
  """The two accumulator sets per lane and flush_all of ens_atoms_patch, patch by patch -> dict(mid = flushes before the patch's
  last row was taken in, retouched = flushes (the last one included) that add into a table row written by an earlier flush of the patch, twin_rows = patches
  that write a twin row, max_atoms = the most atom ids one lane meets down its column)."""
  case, g = inp.case, inp.geometry
  flags, bflags, kind = MODES[case.mode]
  skipna, twin_out = bool(flags & FLAG_SKIPNA), bool(bflags & TWIN_MASK)
  _, tnan = point_selections(inp)
  NONE = -1
  out = dict(mid=0, retouched=0, twin_rows=0, max_atoms=0)
  for cell in range(case.ncell):
    bk = cell % case.nBk
    for rs in range(g.nrs):
      r0, r1 = g.split_br[rs] * case.D, g.split_br[rs + 1] * case.D
      for xt in range(g.nxt):
        xs = slice(64 * xt, 64 * xt + g.live(xt))
        _, ids = np.unique(inp.words[bk, r0:r1, xs], return_inverse=True)
        ids = ids.reshape(r1 - r0, -1).astype(np.int64)
        v = inp.valid[cell, r0:r1, xs]
        if kind is not None:
          ids = np.where(v, ids, ids + 128 if twin_out else NONE)
        if skipna:
          ids = np.where(tnan[cell, r0:r1, xs] & (ids != NONE), ids | 128, ids)
        out['max_atoms'] = max(out['max_atoms'], max(np.unique(col[col != NONE]).size for col in ids.T))
        c0 = np.full(ids.shape[1], NONE)
        c1 = c0.copy()
        touched = set()

        def flush():
          rows = set(c0[c0 != NONE].tolist()) | set(c1[c1 != NONE].tolist())
          again = bool(rows & touched)
          touched.update(rows)
          return again

        for row in ids:
          ok = row != NONE
          miss = ok & (row != c0) & (row != c1)
          if miss.any():
            place = miss
            if (miss & (c0 != NONE) & (c1 != NONE)).any():
              out['mid'] += 1
              out['retouched'] += flush()
              c0[:], c1[:] = NONE, NONE
              place = ok
            first = place & (c0 == NONE)
            c1 = np.where(place & ~first, row, c1)
            c0 = np.where(first, row, c0)
        out['retouched'] += flush()  # (the flush behind the patch's last row)
        out['twin_rows'] += any(r >= 128 for r in touched)
  return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases


def _rot(seq, k):
  return seq[k % len(seq)]


def _shape(geom):
  """The frame of a named geometry: Case fields."""
  return {
      'one-patch': dict(nA=2, nBr=3, nx=64),
      'ragged-3-tiles': dict(nA=2, nBr=5, nx=130),
      'strided-x': dict(nA=2, nBr=5, nx=64, p_xs=2),
      'target-without-x': dict(nA=2, nBr=5, nx=130, t_xs=0),
      'two-level-2-groups': dict(nA=1, nBr=130, nx=512),
      'two-level-2-groups-ragged': dict(nA=1, nBr=130, nx=521),
      'tapered': dict(nA=1, nBr=70, D=4, nx=64),
      'depth-2-untapered': dict(nA=2, nBr=9, D=2, nx=96, d_outer=True),
      'nBk-3': dict(nA=2, nBk=3, nBr=6, nx=130),
      'nj-1': dict(nA=2, nBk=2, nBr=40, nx=96, w_on_x=False, bins='row-stripes'),
      'nbin-64': dict(nA=2, nBr=7, nx=130, bins='bits-64', nbin=64),
      'nbin-1': dict(nA=2, nBr=7, nx=64, bins='bit-0', nbin=1),
  }[geom]


def _nbin(pattern):
  return {'boxes': 6, 'row-stripes': 4, 'checker': 4, 'exactly-32-words': 5, '33-words': 6}[pattern]


def _case(name, geom, mode, m, k, **over):
  """A case of the rotation: `k` deals the values, the member layout, the weights and `fair`."""
  f = dict(name=name, geom=geom, mode=mode, M=m, fair=EC.fair_of(m, k), values=_rot(VALUES, k), layout=_rot(LAYOUTS, k // 3),
           wl=_rot(WEIGHTS, k // 2), seed=k)
  f.update(_shape(geom))
  f.update(over)
  if not f.get('w_on_x', True) and f['wl'] == 'x':
    f['wl'] = 'row'
  if 'bins' in f and 'nbin' not in f:
    f['nbin'] = _nbin(f['bins'])
  return Case(**f)


def matrix_cases(mode, bucket):
  """The two launches of a (mode, bucket) pair: one on the ragged route (four-wave blocks), one on whole lines (lone non-temporal
  waves).  The bucket's member counts alternate over the modes and the routes, the bin patterns, weights, value families and member
  layouts rotate; the small buckets take the two-level geometry (72 and 81 patches per cell), the large ones the tapered one."""
  mi, bi = MODE_NAMES.index(mode), BUCKET_NAMES.index(bucket)
  ms = BUCKETS[bucket]
  out = []
  for r, route in enumerate(('ragged', 'whole')):
    m = _rot(ms, mi + r)
    k = 7 * mi + 2 * bi + r
    if route == 'ragged':
      geom = 'two-level-2-groups-ragged' if bucket == 'm4' else 'ragged-3-tiles'
    else:
      geom = 'two-level-2-groups' if bi < 3 else 'tapered'
    over = dict(bins=_rot(PATTERNS, mi + bi + 2 * r))
    if geom == 'tapered' and m <= 33:
      over['nA'] = 2
    out.append(_case(f'{mode}-{bucket}-{route}-{geom}-{over["bins"]}-M{m}', geom, mode, m, k, **over))
  return out


def geometry_cases():
  """Every named geometry once more on its own, the modes and member counts dealt round robin (nj-1 takes no mask)."""
  names = ('one-patch', 'ragged-3-tiles', 'strided-x', 'target-without-x', 'two-level-2-groups', 'two-level-2-groups-ragged', 'tapered',
           'depth-2-untapered', 'nBk-3', 'nj-1', 'nbin-64', 'nbin-1')
  small = (8, 17, 5, 50, 4, 9, 33, 51, 16, 2, 64, 32)
  out = []
  for i, geom in enumerate(names):
    mode = _rot(MODE_NAMES, 3 * i + 1)
    if geom == 'nj-1':
      mode = 'skipna'
    over = {} if 'bins' in _shape(geom) else dict(bins=_rot(PATTERNS, i))
    out.append(_case(f'geom-{geom}-{mode}-M{small[i]}', geom, mode, small[i], 100 + i, **over))
  # the per-point id row (cell, r) against (bk, br): a per-point mask under depth rows, tapered and not, and under nBk = 3
  out.append(_case('geom-tapered-masked-pt-twin-M8', 'tapered', 'masked-pt-twin', 8, 120, bins='row-stripes', nA=2))
  out.append(_case('geom-depth-2-untapered-masked-pt-M5', 'depth-2-untapered', 'masked-pt', 5, 121, bins='checker'))
  out.append(_case('geom-nBk-3-skipna-masked-pt-twin-M17', 'nBk-3', 'skipna-masked-pt-twin', 17, 122, bins='boxes'))
  out.append(_case('geom-nBk-3-masked-w-twin-M50', 'nBk-3', 'masked-w-twin', 50, 123, bins='row-stripes'))
  out.append(_case('geom-nj-1-plain-M9', 'nj-1', 'plain', 9, 124, bins='row-stripes'))
  return out


def word_cases():
  """Exactly ATOM_MAX = 32 distinct words in a patch, in every mode: the last count that must still work."""
  ms = (64, 2, 51, 9, 33, 50, 5, 16, 32, 17)
  return [_case(f'words-32-{mode}-M{ms[i]}', 'ragged-3-tiles' if i % 2 else 'one-patch', mode, ms[i], 200 + i, bins='exactly-32-words',
                nBr=(5 if i % 2 else 12), nA=2) for i, mode in enumerate(MODE_NAMES)]


def overflow_cases():
  """33 words in every patch of bk = 1, at most 32 in those of bk = 0 (two routes)."""
  return [_case('words-33-plain-M8', 'one-patch', 'plain', 8, 220, bins='33-words', nBk=2, nBr=20, nx=128),
          _case('words-33-masked-pt-twin-M51', 'one-patch', 'masked-pt-twin', 51, 221, bins='33-words', nBk=2, nBr=20, nx=128, p_xs=2)]


def special_cases():
  """One special point per cell (a NaN member, a +inf member, a NaN target x a valid point, a masked-out point, a point in no bin,
  the last live x of the ragged tail) in every mode; cells 12 and 13 stay clean."""
  ms = (5, 50, 8, 33, 16, 51, 2, 17, 64, 9)
  return [_case(f'special-{mode}-M{ms[i]}', 'ragged-3-tiles', mode, ms[i], 300 + i, bins=_rot(PATTERNS, i), nA=7, nBk=2, special=True)
          for i, mode in enumerate(MODE_NAMES)]


def accumulate_cases():
  """One case per output mode (6 / 12 / 10 / 20 lanes), without NaN outputs but the documented ones."""
  return [_case(f'acc-{mode}-M{m}', 'ragged-3-tiles', mode, m, 400 + i, bins=_rot(PATTERNS, i))
          for i, (mode, m) in enumerate((('plain', 8), ('masked-w-twin', 51), ('skipna-masked-pt', 17), ('skipna-masked-pt-twin', 4)))]


def all_matrix_cases():
  return [c for mode in MODE_NAMES for b in BUCKET_NAMES for c in matrix_cases(mode, b)]


def all_cases():
  return all_matrix_cases() + geometry_cases() + word_cases() + overflow_cases() + special_cases() + accumulate_cases()


def by_name(name):
  return next(c for c in all_cases() if c.name == name)
