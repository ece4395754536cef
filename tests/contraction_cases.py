"""Inputs, the float64 restatement, the error bounds and the route restatement for stage 2, the weights x bin-mask contraction of
the stage-1 partials (wbx_contract, wbx_contract_bits: csrc/wbx_s2.hip, csrc/wbx_s2_patch.hip, csrc/wbx_patch.hpp), plain NumPy.

Restatement (include/wbx.h), in float64 on float64 inputs:
    partial[nA][nBk][nBr][nchunk][nlane][nj]      W[nBk][nBr][nj][nbin]
    sum_j = 1: out[a, b, l, n]    = sum_{r, c, j} partial[a, b, r, c, l, j] * W[b, r, j, n]
    sum_j = 0: out[a, b, l, j, n] = sum_{r, c}    partial[a, b, r, c, l, j] * W[b, r, j, n]
    bits form: W = wt[..., None] * member, bit n of bits[b, r, j] = member[b, r, j, n]
`restate` forms it as one matrix product per bk (sum_j) or np.einsum (keep j); test_contraction_cases.py holds both against a
triple loop.  An output that is exactly zero is +0.

Value classes.
  exact     partial holds integers in [-2^20, 2^20], wt = k / 8 with k in [4, 12].  Every product is a multiple of 1/8 below 1.5 * 2^20
            and every sum of up to 2^17 of them, in any order and with the chunks added first or not, a multiple of 1/8 below 2^38:
            exact in float64.  The kernels must equal the restatement BIT FOR BIT on every route.  `make_case` asserts the magnitudes.
  rounded   partial ~ N(0, 1) * 10^U(-3, 3), wt in [0.5, 1.5).  With N = nBr * nchunk * (nj if sum_j else 1) terms and
            S = sum |partial| * |W| over the same terms, ANY float64 evaluation order -- the chunks of a point added before the
            multiplication by wt (the bits routes), rounded products or fma, waves, LDS, patch and split folds -- is within
                E = (N + nchunk + 3) * 2^-53 * S * 1.01
            of the exact sum: N - 1 additions and one rounding per product make N u S to first order, the chunk pre-sum at most
            nchunk u S more, 3 u S covers the poison term's +0 and the final folds' roundings, 1.01 the second-order terms
            (N u < 2^-36).  The restatement is such an evaluation itself and carries the same bound, so the tests allow 2 E between
            the kernel and the restatement (the reference is the plain float64 restatement, not an exactly summed one).  Derived,
            never fitted.
  non-finite  a rounded case with ONE NaN, +inf or -inf partial.  The bits routes (s2_bits_kernel, s2_patch_kernel) add
            (partial * wt) * 0 to every bin: NaN in EVERY bin of the output row (a, b, l[, j]) the element belongs to -- bins without
            members and patches with an empty union included --, every other row untouched.  The dense route multiplies by W as it
            is: a NaN partial gives NaN in every bin of its row (NaN * 0), an infinite one +-inf in the bins the point belongs to
            (the weights are positive) and NaN in the others.  `nonfinite_case` builds both from the finite restatement; at
            least 75 % of the expected outputs stay finite (asserted).

Routes (`route`): a restatement of the dispatch in wbx_contract / wbx_contract_bits (csrc/wbx_s2.hip), s2_patch_eligible and the
K table of launch_s2_patch (csrc/wbx_s2_patch.hip) and patch_geometry with D = 1 (csrc/wbx_patch.hpp).  The case lists below are
the smallest shapes that reach each branch; test_contraction_cases.py asserts the route of each."""
import dataclasses
import functools

import numpy as np

U = 2.0 ** -53
SENTINEL = -77.25
BG = 8                                  # csrc/wbx_s2.hip: `constexpr int BG = 8` (bins per register group of the dense kernels)
DENSE_SPLIT_BLOCKS = 2048               # wbx_contract: `want = (2048 + grid - 1) / grid`
DENSE_SPLIT_MAX_GRID = 1024             # wbx_contract: `grid < 1024`
DENSE_SPLIT_MIN_TERMS = 1 << 16         # wbx_contract: `nrc * p.nj >= ((int64_t)1 << 16)`
DENSE_LONG_NJ = 64                      # wbx_contract / s2_reduce_kernel: `p.nj >= 64` (long rows; keep-j kernel from here on)
BITS_BLOCKS = 4096                      # wbx_contract_bits: `want = (4096 + nrow - 1) / nrow`
BITS_THREADS = 256                      # wbx_contract_bits: `nsplit = (p.nj + 255) / 256` blocks of 256 j (sum_j = 0)
PATCH_LANES = (1, 2, 3, 4, 5, 6, 7, 10, 12)  # s2_patch_eligible: `case 1: case 2: ... case 10: case 12:`
PATCH_MIN_DEFAULT = 1 << 20             # s2_patch_eligible: `(int64_t)1 << 20` elements without WBX_S2_PATCH_MIN
PATCH_TARGETS = (8192, 16384)           # patch_geometry: `target = nx % 32 == 0 ? 8192 : 16384`
PATCH_OFF = 1 << 40


def patch_k(nl: int) -> int:
  """launch_s2_patch: `K = NL <= 1 ? 32 : (NL <= 2 ? 24 : (NL <= 3 ? 16 : (NL <= 4 ? 12 : (NL <= 5 ? 8 : (NL <= 6 ? 7 : (NL <= 7 ? 5 : 2))))))`."""
  for top, k in ((1, 32), (2, 24), (3, 16), (4, 12), (5, 8), (6, 7), (7, 5)):
    if nl <= top:
      return k
  return 2


@dataclasses.dataclass(frozen=True)
class Plan:
  """wbx_s2_plan, field for field."""
  nA: int
  nBk: int
  nBr: int
  nchunk: int
  nlane: int
  nj: int
  nbin: int
  sum_j: int = 1

  @property
  def nrow(self):
    return self.nA * self.nBk * self.nlane

  @property
  def partial_shape(self):
    return (self.nA, self.nBk, self.nBr, self.nchunk, self.nlane, self.nj)

  @property
  def out_shape(self):
    head = (self.nA, self.nBk, self.nlane)
    return head + ((self.nbin,) if self.sum_j else (self.nj, self.nbin))

  @property
  def nterms(self):
    return self.nBr * self.nchunk * (self.nj if self.sum_j else 1)

  def fields(self):
    return (self.nA, self.nBk, self.nBr, self.nchunk, self.nlane, self.nj, self.nbin, self.sum_j)


@dataclasses.dataclass(frozen=True)
class Route:
  name: str     # 'reduce/short' | 'reduce/long' | 'reduce/long+split' | 'reduce/fixed_j' | 'keepj' | 'bits<NB>/sum_j' | 'bits<NB>/keep_j' | 'patch<NL,K>'
  info: dict    # the numbers of the launch, see `route`

  def __getattr__(self, key):
    try:
      return self.info[key]
    except KeyError:
      raise AttributeError(key) from None


def _ceil(a, b):
  return -(-a // b)


def patch_geometry(plan: Plan):
  """patch_geometry(g, cells = nA * nBk, nBk, nBr, nj, D = 1, nx = nj) -> (nxt, nrs, rows_per_split)."""
  cells, rows = plan.nA * plan.nBk, plan.nBr
  nxt = _ceil(plan.nj, 64)
  target = PATCH_TARGETS[0] if plan.nj % 32 == 0 else PATCH_TARGETS[1]
  want = _ceil(target, cells * nxt)
  want = max(1, min(want, _ceil(rows, 64)))
  rps = _ceil(rows, want)
  return nxt, _ceil(rows, rps), rps


def split_rows(nBr, rps):
  return [min(rps, nBr - r) for r in range(0, nBr, rps)]


def patch_unions(plan: Plan, bits):
  """uni[bk][rs][xt]: the OR of the membership words of the patch's live points."""
  nxt, nrs, rps = patch_geometry(plan)
  uni = np.zeros((plan.nBk, nrs, nxt), np.uint64)
  for rs in range(nrs):
    for xt in range(nxt):
      block = bits[:, rs * rps:(rs + 1) * rps, xt * 64:(xt + 1) * 64]
      uni[:, rs, xt] = np.bitwise_or.reduce(block.reshape(plan.nBk, -1), axis=1)
  return uni


def popcount(words):
  return np.array([bin(int(w)).count('1') for w in np.asarray(words).ravel()]).reshape(np.shape(words))


def route(plan: Plan, form: str, patch_min: int = PATCH_MIN_DEFAULT, bits=None) -> Route:
  """The kernel a call takes and its launch numbers.  form: 'dense' (wbx_contract) | 'bits' (wbx_contract_bits with
  WBX_S2_PATCH_MIN = patch_min).  `bits` (the membership words) adds the unions' numbers to a patch route."""
  p = plan
  assert p.nrow * (1 if p.sum_j else p.nj) * p.nbin > 0 and p.nterms > 0, 'an empty contraction launches nothing'
  if form == 'dense':
    if p.sum_j or p.nj < DENSE_LONG_NJ:
      fixed_j = not p.sum_j
      grid = p.nrow * (p.nj if fixed_j else 1)
      ncontr = p.nBr * p.nchunk * (1 if fixed_j else p.nj)
      threads = 256 if ncontr >= 256 else (128 if ncontr >= 128 else 64)
      info = dict(threads=threads, grid=grid, groups=_ceil(p.nbin, BG))
      if fixed_j:
        return Route('reduce/fixed_j', info)
      if p.nj < DENSE_LONG_NJ:
        return Route('reduce/short', info)
      nrc = p.nBr * p.nchunk
      if grid < DENSE_SPLIT_MAX_GRID and nrc * p.nj >= DENSE_SPLIT_MIN_TERMS:
        nsplit = min(_ceil(DENSE_SPLIT_BLOCKS, grid), nrc)
        if nsplit > 1:  # (nsplit == 1 goes through the scratch buffer but adds no finish launch)
          per = _ceil(nrc, nsplit)
          empty = sum(1 for s in range(nsplit) if s * per >= nrc)
          return Route('reduce/long+split', dict(info, nsplit=nsplit, per=per, empty_splits=empty))
      return Route('reduce/long', info)
    threads = 256 if p.nj >= 256 else (128 if p.nj >= 128 else 64)
    return Route('keepj', dict(threads=threads, njtile=_ceil(p.nj, threads)))
  assert form == 'bits' and 1 <= p.nbin <= 64
  nb = 16 if p.nbin <= 16 else (32 if p.nbin <= 32 else 64)
  eligible = bool(p.sum_j) and p.nj >= 64 and p.nlane in PATCH_LANES and int(np.prod(p.partial_shape, dtype=np.int64)) >= patch_min
  if eligible:
    nxt, nrs, rps = patch_geometry(p)
    k = patch_k(p.nlane)
    info = dict(NL=p.nlane, K=k, nxt=nxt, nrs=nrs, rows_per_split=rps, rows=split_rows(p.nBr, rps), tail_lanes=p.nj - 64 * (nxt - 1))
    if bits is not None:
      uni = patch_unions(p, bits)
      pc = popcount(uni)
      info.update(sweeps=max(1, _ceil(int(pc.max()), k)), largest_union=int(pc.max()), empty_unions=int((uni == 0).sum()),
                  high_only_unions=int(((uni != 0) & ((uni & np.uint64(0xFFFFFFFF)) == 0)).sum()), unions=uni)
    return Route(f'patch<{p.nlane},{k}>', info)
  if p.sum_j:
    want = max(1, min(_ceil(BITS_BLOCKS, p.nrow), p.nBr))
    rpb = _ceil(p.nBr, want)
    return Route(f'bits<{nb}>/sum_j', dict(NB=nb, rows_per_block=rpb, nsplit=_ceil(p.nBr, rpb), rows=split_rows(p.nBr, rpb)))
  return Route(f'bits<{nb}>/keep_j', dict(NB=nb, njtile=_ceil(p.nj, BITS_THREADS)))


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement


def pack_bits(member):
  bits = np.zeros(member.shape[:-1], np.uint64)
  for n in range(member.shape[-1]):
    bits |= member[..., n].astype(np.uint64) << np.uint64(n)
  return bits


def restate(partial, w, sum_j):
  """The formula of include/wbx.h on finite float64 inputs.  sum_j: per bk one product of [(a, l)] x [(r, c, j)] with
  [(r, c, j)] x [n] -- W repeated along the chunks, the chunks NOT added first --; keep j: np.einsum.  `+ 0.0` makes a zero +0."""
  nA, nBk, nBr, nchunk, nlane, nj = partial.shape
  nbin = w.shape[-1]
  assert w.shape == (nBk, nBr, nj, nbin) and partial.dtype == np.float64 and w.dtype == np.float64
  if not sum_j:
    return np.einsum('abrclj,brjn->abljn', partial, w) + 0.0
  out = np.empty((nA, nBk, nlane, nbin))
  for b in range(nBk):
    x = partial[:, b].transpose(0, 3, 1, 2, 4).reshape(nA * nlane, nBr * nchunk * nj)      # [(a, l)][(r, c, j)]
    wr = np.broadcast_to(w[b][:, None], (nBr, nchunk, nj, nbin)).reshape(nBr * nchunk * nj, nbin)
    out[:, b] = (x @ wr).reshape(nA, nlane, nbin)
  return out + 0.0


def brute_force(partial, w, sum_j):
  """The same as loops over every index, term by term in index order."""
  nA, nBk, nBr, nchunk, nlane, nj = partial.shape
  nbin = w.shape[-1]
  out = np.zeros((nA, nBk, nlane, nbin) if sum_j else (nA, nBk, nlane, nj, nbin))
  for a in range(nA):
    for b in range(nBk):
      for l in range(nlane):
        for j in range(nj):
          for n in range(nbin):
            s = 0.0
            for r in range(nBr):
              for c in range(nchunk):
                s += partial[a, b, r, c, l, j] * w[b, r, j, n]
            if sum_j:
              out[a, b, l, n] += s
            else:
              out[a, b, l, j, n] = s
  return out


# ------------------------------------------------------------------------------------------------------------------------------
# membership patterns


def member_dense(rng, plan: Plan, geom=None):
  """Every point in a random third of the bins; bin 0 holds EVERY point, bin 1 none (nbin >= 3), the top bit (and bit 31) some:
  the union of every patch is every bin but the empty one -- more than any K where nbin >= 34."""
  p = plan
  m = rng.random((p.nBk, p.nBr, p.nj, p.nbin)) < 0.3
  m[..., 0] = True
  if p.nbin >= 3:
    m[..., 1] = False
  m[:, ::2, ::3, p.nbin - 1] = True
  if p.nbin > 32:
    m[:, 1::2, 1::3, 31] = True
  return m


def member_tiles(rng, plan: Plan, geom=None):
  """Membership that is constant over a 64-wide x tile: bin (nbin - 1 - 5 * tile - 3 * bk) % nbin on two rows of three (row 0 among them), a second bin
  32 further on every fourth row, the other points in no bin: no patch sees more than 2 bins (K >= 2: one sweep for every NL)."""
  p = plan
  m = np.zeros((p.nBk, p.nBr, p.nj, p.nbin), bool)
  r = np.arange(p.nBr)[:, None]
  for b in range(p.nBk):
    for xt in range(_ceil(p.nj, 64)):
      first = (p.nbin - 1 - 5 * xt - 3 * b) % p.nbin
      m[b, :, xt * 64:(xt + 1) * 64, first] |= (r % 3 != 1)
      m[b, :, xt * 64:(xt + 1) * 64, (first + 32) % p.nbin] |= (r % 4 == 1)
  return m


def member_boxes(rng, plan: Plan, geom=None):
  """Region-like boxes in (row, j), one per bin and bk, a tenth of the points taken out of every bin; bin 1 empty (nbin >= 3); the
  top bit and bit 31 set on lattices of points.  Then, patch by patch of the geometry `geom` = (nxt, nrs, rows_per_split) (the
  patch route's, or any for the other routes):
    bk 0: the last x tile has no member in ANY row split (nxt >= 2); x tile 0 has none in row split 0 ONLY (nrs >= 2); x tile 0 of
          the last row split holds bins >= 32 only (nbin > 32);
    bk 1: x tile 0 has no member in any row split (nxt >= 2); the last x tile has none in the last row split only (nrs >= 2)."""
  p = plan
  nxt, nrs, rps = geom if geom is not None else patch_geometry(p)
  m = np.zeros((p.nBk, p.nBr, p.nj, p.nbin), bool)
  for b in range(p.nBk):
    for n in range(p.nbin):
      r0, j0 = int(rng.integers(0, p.nBr)), int(rng.integers(0, p.nj))
      r1 = r0 + 1 + int(rng.integers(0, max(1, p.nBr // 2) + 1))
      j1 = j0 + 1 + int(rng.integers(0, max(1, p.nj // 2) + 1))
      m[b, r0:r1, j0:j1, n] = True
      m[b, p.nBr - 1 - r0 // 2:, :max(1, j0 // 2), n] = True  # and a corner, so that the last rows of the last split are in use
  m &= rng.random((p.nBk, p.nBr, p.nj, 1)) > 0.1
  if p.nbin >= 3:
    m[..., 1] = False
  m[:, ::2, ::3, p.nbin - 1] = True
  if p.nbin > 32:
    m[:, 1::2, 1::3, 31] = True
  last = slice((nrs - 1) * rps, p.nBr)
  if p.nbin > 32:
    m[0, last, 0:64, :32] = False
    m[0, last, 0:64:2, p.nbin - 1] = True
    m[0, last, 1:64:4, 32] = True
  if p.nBk > 1:
    if nxt >= 2:
      m[1, :, 0:64] = False
    if nrs >= 2:
      m[1, last, (nxt - 1) * 64:] = False
  if nxt >= 2:
    m[0, :, (nxt - 1) * 64:] = False
  if nrs >= 2:
    m[0, 0:rps, 0:64] = False
  m[:, p.nBr // 2, p.nj // 3] = False  # however small the case, a point in no bin
  return m


PATTERNS = {'boxes': member_boxes, 'dense': member_dense, 'tiles': member_tiles}


# ------------------------------------------------------------------------------------------------------------------------------
# cases


@dataclasses.dataclass
class Case:
  plan: Plan
  kind: str             # 'exact' | 'rounded'
  pattern: str
  partial: np.ndarray   # float64 [nA][nBk][nBr][nchunk][nlane][nj]
  wt: np.ndarray        # float64 [nBk][nBr][nj]
  member: np.ndarray    # bool    [nBk][nBr][nj][nbin]

  @functools.cached_property
  def bits(self):
    return pack_bits(self.member)

  @functools.cached_property
  def w(self):
    return self.wt[..., None] * self.member

  @functools.cached_property
  def want(self):
    return restate(self.partial, self.w, self.plan.sum_j)

  @functools.cached_property
  def bound(self):
    """E of the module docstring per output (0 in the exact class): the tests allow 2 E."""
    if self.kind == 'exact':
      return np.zeros(self.plan.out_shape)
    s = restate(np.abs(self.partial), self.w, self.plan.sum_j)
    return (self.plan.nterms + self.plan.nchunk + 3) * U * s * 1.01


def _seed(plan, kind, pattern, seed):
  return [seed, {'exact': 1, 'rounded': 2}[kind], sorted(PATTERNS).index(pattern)] + list(plan.fields())


def make_case(plan: Plan, kind: str, pattern: str = 'boxes', seed: int = 0, geom=None) -> Case:
  rng = np.random.default_rng(_seed(plan, kind, pattern, seed))
  member = PATTERNS[pattern](rng, plan, geom)
  if kind == 'exact':
    partial = rng.integers(-2 ** 20, 2 ** 20 + 1, size=plan.partial_shape).astype(np.float64)
    wt = rng.integers(4, 13, size=(plan.nBk, plan.nBr, plan.nj)) / 8.0
    assert plan.nBr * plan.nchunk * plan.nj <= 2 ** 17, 'more terms than the exact class allows'
    assert np.abs(partial).max() <= 2 ** 20 and wt.min() >= 0.5 and wt.max() <= 1.5 and (wt * 8 == np.rint(wt * 8)).all()
  else:
    assert kind == 'rounded'
    partial = rng.normal(size=plan.partial_shape) * 10.0 ** rng.uniform(-3, 3, size=plan.partial_shape)
    wt = rng.random((plan.nBk, plan.nBr, plan.nj)) * 1.0 + 0.5
  return Case(plan, kind, pattern, partial, wt, member)


def check(got, case: Case, what: str) -> float:
  """Every output against the restatement: bit for bit (exact) or within 2 E (rounded).  -> the largest error / (2 E)."""
  want = case.want
  assert got.shape == want.shape, what
  assert not (got == SENTINEL).any(), f'{what}: {int((got == SENTINEL).sum())} outputs were never written'
  if case.kind == 'exact':
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert not len(bad), f'{what}: {len(bad)} of {got.size} outputs differ from the exact sums, the first at {tuple(bad[0])}: ' \
                         f'{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}'
    return 0.0
  assert np.isfinite(got).all(), f'{what}: non-finite outputs from finite inputs'
  err, allow = np.abs(got - want), 2.0 * case.bound
  bad = np.argwhere(err > allow)
  assert not len(bad), f'{what}: {len(bad)} of {got.size} outputs beyond the bound, the first at {tuple(bad[0])}: ' \
                       f'|{got[tuple(bad[0])]!r} - {want[tuple(bad[0])]!r}| = {err[tuple(bad[0])]:.3e} > {allow[tuple(bad[0])]:.3e}'
  nz = allow > 0
  return float((err[nz] / allow[nz]).max()) if nz.any() else 0.0


# ---- non-finite partials


def nonfinite_sites(plan: Plan, member, rows, b):
  """(label, (r, c, j)) of the places a non-finite partial of bk `b` is put at in turn, for a route whose row blocks / row splits
  are `rows` (lengths): the first row of a split, the last row of an odd-length and of an even-length split, a tail lane of the
  last x tile, a chunk other than 0, a point that belongs to no bin.  A place the shape does not have is left out."""
  p = plan
  starts = np.concatenate([[0], np.cumsum(rows)])
  sites = [('first row of a split', (int(starts[min(1, len(rows) - 1)]), 0, min(3, p.nj - 1)))]
  for parity, label in ((1, 'last row of an odd-length split'), (0, 'last row of an even-length split')):
    hit = [i for i, n in enumerate(rows) if n % 2 == parity]
    if hit:
      sites.append((label, (int(starts[hit[-1] + 1]) - 1, 0, min(5, p.nj - 1))))
  if p.nj % 64:
    sites.append(('tail lane of the last x tile', (p.nBr // 2, 0, p.nj - 1)))
  if p.nchunk > 1:
    sites.append(('a chunk other than 0', (p.nBr - 1, p.nchunk - 1, p.nj // 2)))
  r, j = no_bin_point(member, b)
  sites.append(('a point that belongs to no bin', (r, 0, j)))
  return sites


def no_bin_point(member, b):
  """(r, j) of a point of bk `b` that belongs to no bin: the last one whose row has members in the same 64-wide x tile (a point
  in no bin inside a patch that has bins), else the last one."""
  free = np.argwhere(~member[b].any(axis=-1))
  assert len(free), 'the pattern leaves no point without a bin'
  for r, j in free[::-1]:
    if member[b, r, j // 64 * 64:j // 64 * 64 + 64].any():
      return int(r), int(j)
  return int(free[-1][0]), int(free[-1][1])


def nonfinite_case(base: Case, value: float, site, row):
  """`base` (rounded) with `value` (NaN or +-inf) at partial[a, b, r, c, l, j], row = (a, b, l), site = (r, c, j).
  -> (partial, expected on the bits routes, expected on the dense route)."""
  assert base.kind == 'rounded'
  p = base.plan
  (a, b, l), (r, c, j) = row, site
  partial = base.partial.copy()
  partial[a, b, r, c, l, j] = 0.0
  finite = restate(partial, base.w, p.sum_j)
  partial[a, b, r, c, l, j] = value
  where = (a, b, l) if p.sum_j else (a, b, l, j)
  on_bits, on_dense = finite.copy(), finite.copy()
  on_bits[where] = np.nan
  if np.isnan(value):
    on_dense[where] = np.nan
  else:
    on_dense[where] = np.where(base.member[b, r, j], value, np.nan)  # wt > 0: +-inf keeps its sign in the point's bins
  for want in (on_bits, on_dense):
    share = float(np.isfinite(want).mean())
    assert share >= 0.75, ('finite share of the expected outputs', share, p)
  return partial, on_bits, on_dense


def check_nonfinite(got, want, base: Case, what: str):
  """NaN exactly where expected, +-inf exactly where expected with its sign, every other output within 2 E of the finite
  restatement (the bound of the base case: one term fewer)."""
  assert got.shape == want.shape and not (got == SENTINEL).any(), what
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{what}: NaN placement')
  inf = np.isinf(want)
  np.testing.assert_array_equal(np.isinf(got), inf, err_msg=f'{what}: inf placement')
  np.testing.assert_array_equal(got[inf], want[inf], err_msg=f'{what}: sign of the infinities')
  fin = np.isfinite(want)
  assert (np.abs(got[fin] - want[fin]) <= 2.0 * base.bound[fin]).all(), f'{what}: an untouched row moved'


# ---- the case lists: the smallest shapes that reach each branch ------------------------------------------------------------------

# dense, sum_j = 1.  (name, plan, route name, expected numbers)
DENSE_SUM_J = [
    ('short nj=1 64 threads nbin=1', Plan(2, 2, 9, 3, 2, 1, 1), 'reduce/short', dict(threads=64, groups=1)),
    ('short nj=5 128 threads nbin=8', Plan(2, 2, 13, 2, 3, 5, 8), 'reduce/short', dict(threads=128, groups=1)),
    ('short nj=63 256 threads nbin=9', Plan(2, 2, 5, 1, 2, 63, 9), 'reduce/short', dict(threads=256, groups=2)),
    ('short nj=5 64 threads nbin=34', Plan(1, 2, 6, 2, 3, 5, 34), 'reduce/short', dict(threads=64, groups=5)),
    ('long nj=64 nbin=9', Plan(2, 2, 7, 2, 3, 64, 9), 'reduce/long', dict(threads=256, groups=2)),
    ('long nj=257 nbin=34', Plan(2, 1, 3, 2, 2, 257, 34), 'reduce/long', dict(threads=256, groups=5)),
    ('long nj=64 one row nbin=1', Plan(1, 2, 1, 1, 1, 64, 1), 'reduce/long', dict(threads=64, groups=1)),
    ('long nj=65 one row nbin=8', Plan(1, 1, 1, 1, 2, 65, 8), 'reduce/long', dict(threads=64, groups=1)),
    ('long nj=129 one row nbin=8', Plan(1, 1, 1, 1, 2, 129, 8), 'reduce/long', dict(threads=128, groups=1)),
]
# 60 output rows over a 32 MB partial: 35 blocks of 2 (row, chunk) pairs per output, 12 of them empty; and one output row: 46 of 1
DENSE_SPLIT_BIG = ('split 60 outputs', Plan(5, 2, 23, 2, 6, 1440, 3), 'reduce/long+split', dict(nsplit=35, per=2, empty_splits=12))
DENSE_SPLIT_ONE = ('split one output', Plan(1, 1, 23, 2, 1, 1440, 3), 'reduce/long+split', dict(nsplit=46, per=1, empty_splits=0))
# four outputs over 1100 (row, chunk) pairs of 64 points: 512 blocks of ceil(1100 / 512) = 3 pairs, the last one ragged, 145 empty
DENSE_SPLIT_SMALL = ('split 4 outputs', Plan(1, 1, 550, 2, 4, 64, 9), 'reduce/long+split', dict(nsplit=512, per=3, empty_splits=145))
# dense, sum_j = 0
DENSE_KEEP_J = [
    ('fixed_j nj=1', Plan(2, 2, 150, 2, 3, 1, 9, 0), 'reduce/fixed_j', dict(threads=256)),
    ('fixed_j nj=7', Plan(2, 2, 33, 4, 2, 7, 34, 0), 'reduce/fixed_j', dict(threads=128)),
    ('fixed_j nj=63', Plan(1, 2, 9, 3, 2, 63, 8, 0), 'reduce/fixed_j', dict(threads=64)),
    ('keepj nj=64', Plan(2, 2, 9, 3, 2, 64, 9, 0), 'keepj', dict(threads=64, njtile=1)),
    ('keepj nj=65', Plan(2, 2, 5, 1, 3, 65, 34, 0), 'keepj', dict(threads=64, njtile=2)),
    ('keepj nj=129', Plan(1, 2, 7, 2, 2, 129, 1, 0), 'keepj', dict(threads=128, njtile=2)),
    ('keepj nj=257', Plan(2, 1, 4, 3, 2, 257, 8, 0), 'keepj', dict(threads=256, njtile=2)),
    ('keepj nj=600', Plan(1, 2, 3, 2, 2, 600, 9, 0), 'keepj', dict(threads=256, njtile=3)),
]
# bits, sum_j = 1, the patch kernel off (WBX_S2_PATCH_MIN huge) or not eligible
BITS_SUM_J = [
    ('nbin=1 nj=1 nlane=1', Plan(2, 2, 9, 3, 1, 1, 1), 'bits<16>/sum_j', dict(rows_per_block=1, nsplit=9)),
    ('nbin=16 nj=3 nlane=8', Plan(2, 2, 11, 2, 8, 3, 16), 'bits<16>/sum_j', dict(rows_per_block=1, nsplit=11)),
    ('nbin=17 nj=64 nlane=9', Plan(2, 2, 10, 1, 9, 64, 17), 'bits<32>/sum_j', dict(rows_per_block=1, nsplit=10)),
    ('nbin=32 nj=300 nlane=13', Plan(1, 2, 5, 2, 13, 300, 32), 'bits<32>/sum_j', dict(rows_per_block=1, nsplit=5)),
    ('nbin=33 nj=3 nlane=1', Plan(3, 2, 8, 3, 1, 3, 33), 'bits<64>/sum_j', dict(rows_per_block=1, nsplit=8)),
    ('nbin=64 nj=64 nlane=8', Plan(2, 2, 6, 2, 8, 64, 64), 'bits<64>/sum_j', dict(rows_per_block=1, nsplit=6)),
    ('nbin=64 nj=300 nlane=3', Plan(2, 2, 9, 1, 3, 300, 64), 'bits<64>/sum_j', dict(rows_per_block=1, nsplit=9)),
    ('1500 rows of 7: blocks of 3, 3, 1', Plan(50, 2, 7, 2, 15, 1, 17), 'bits<32>/sum_j', dict(rows_per_block=3, nsplit=3, rows=[3, 3, 1])),
    ('4100 rows of 7: one block each', Plan(82, 2, 7, 1, 25, 3, 33), 'bits<64>/sum_j', dict(rows_per_block=7, nsplit=1, rows=[7])),
]
# bits, sum_j = 0
BITS_KEEP_J = [
    ('nj=1 nbin=5', Plan(2, 2, 9, 3, 2, 1, 5, 0), 'bits<16>/keep_j', dict(njtile=1)),
    ('nj=255 nbin=33', Plan(1, 2, 5, 1, 2, 255, 33, 0), 'bits<64>/keep_j', dict(njtile=1)),
    ('nj=256 nbin=64', Plan(1, 2, 4, 3, 1, 256, 64, 0), 'bits<64>/keep_j', dict(njtile=1)),
    ('nj=257 nbin=5', Plan(2, 1, 6, 1, 2, 257, 5, 0), 'bits<16>/keep_j', dict(njtile=2)),
    ('nj=600 nbin=33', Plan(1, 2, 3, 3, 1, 600, 33, 0), 'bits<64>/keep_j', dict(njtile=3)),
    ('nj=257 nbin=17', Plan(1, 1, 3, 1, 3, 257, 17, 0), 'bits<32>/keep_j', dict(njtile=2)),
]
# the patch kernel (WBX_S2_PATCH_MIN = 0): (nBr, nj) with six (a, bk) cells -> (nxt, rows of the row splits, live lanes of the last tile)
PATCH_CELLS = (3, 2)
PATCH_GEOMETRIES = [
    ((1, 65), 2, [1], 1),
    ((2, 127), 2, [2], 63),
    ((37, 64), 1, [37], 64),
    ((65, 65), 2, [33, 32], 1),
    ((67, 130), 3, [34, 33], 2),
    ((130, 64), 1, [44, 44, 42], 64),
    ((193, 70), 2, [49, 49, 49, 46], 6),
]
PATCH_NBINS = (1, 34, 64)
PATCH_NCHUNKS = (1, 3)
PATCH_PATTERNS = ('boxes', 'dense', 'tiles')


def patch_rotation(nl: int):
  """The launches of lane count `nl`: every geometry once, the chunk count, nbin and the pattern rotating so that every (nBr, nj),
  every nbin, both chunk counts and every pattern occur with every lane count while the combinations differ from lane count to
  lane count (a geometry meets nchunk = 1, the two-rows-in-flight loop, under every other lane count).  -> [(Plan, pattern)]"""
  i = PATCH_LANES.index(nl)
  out = []
  for g, ((nbr, nj), _, _, _) in enumerate(PATCH_GEOMETRIES):
    nchunk = PATCH_NCHUNKS[(g + i) % 2]
    nbin = PATCH_NBINS[(g + i) % 3]
    pattern = PATCH_PATTERNS[(g + g // 3 + i) % 3]
    out.append((Plan(*PATCH_CELLS, nbr, nchunk, nl, nj, nbin), pattern))
  return out


def all_listed():
  """[(form, patch_min, name, plan, route name, numbers)] of every list above, the patch rotation of every lane count included."""
  rows = []
  for name, plan, rname, nums in DENSE_SUM_J + [DENSE_SPLIT_BIG, DENSE_SPLIT_ONE, DENSE_SPLIT_SMALL] + DENSE_KEEP_J:
    rows.append(('dense', PATCH_OFF, name, plan, rname, nums))
  for name, plan, rname, nums in BITS_SUM_J + BITS_KEEP_J:
    rows.append(('bits', PATCH_OFF, name, plan, rname, nums))
  for nl in PATCH_LANES:
    for plan, pattern in patch_rotation(nl):
      geo = next(g for g in PATCH_GEOMETRIES if g[0] == (plan.nBr, plan.nj))
      rows.append(('bits', 0, f'patch NL={nl} {pattern}', plan, f'patch<{nl},{patch_k(nl)}>', dict(nxt=geo[1], rows=geo[2], tail_lanes=geo[3])))
  return rows
