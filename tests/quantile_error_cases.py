"""Inputs and the float64 restatement for the errors of ensemble quantiles (wbx_ens_quantile_error_partial), plain NumPy.

Restatement (include/wbx.h): per point with members x_m (m < M), target t and quantile levels q_j
    Q_j = np.quantile(x, q_j) over the members AS THEY ARE (NumPy's `linear` method, float64 results; NaN where a member is NaN),
    e_j = Q_j - float64(t)
    Error = e_j,  AbsoluteError = |e_j|,  SquaredError = e_j * e_j;   value lane stat * Q + j.
A stage-1 partial is the float64 sum of a lane's values over its points: masked points add exactly 0, under skipna a NaN value is
counted out of its own lane (one count lane per value lane), under a mask alone one count lane holds the valid points.
np.quantile of float32 members is NOT np.quantile of the members cast to float64: NumPy subtracts the two neighbours in the members'
type before the float64 weight joins, so d = B - A is rounded to float32 (tests/test_quantile_errors.py shows both facts).  The
host route hands NumPy the members as they are, and so does this restatement; for float64 members the two are the same thing.

How a test may compare (`expected` gives a partial and its bound):
  * x kept: a lane owns an x and adds the rows of its chunk in order, 0.0 + v_0 + v_1 ...: `expected` adds them in that order, so the
    partial is compared bit for bit.
  * exactly summable inputs (`exact=True`: members and targets are small integers, levels are multiples of 1/8, so every value is a
    multiple of 1/64 below 2^12): any order of adding gives the same float64, bit for bit.
  * otherwise (x summed over general values) the kernel adds in its own fixed order.  `expected` then gives the correctly rounded
    sum (math.fsum) and `bound` = n 2^-53 sum|v|, n the number of addends: the first-order bound of ANY order of adding n float64
    numbers, (n - 1) u sum|v| with u = 2^-53, plus the u |S| the reference itself is rounded by.  It comes from the case's own values.
  Non-finite partials (a NaN poisons, +-inf members) are compared as they are: NaN where NaN, the same infinity where infinite.

`model` is the kernel's arithmetic step by step (sort in the input type, the host's (k, g), the difference of the neighbours in the
input type, the two-branch lerp in float64, the NaN flag) with the mistakes a kernel could make switchable: tests/test_quantile_errors.py shows that the restatement equals the model
bit for bit and tells every mutant from it on at least one case."""
import fractions
import math

import numpy as np

FLAG_MASKED, FLAG_SKIPNA = 1, 2
ERR, ABS, SQ = 0, 1, 2
STATS = 3
MAX_QUANTILES = 16
MAX_MEMBERS = 64
SIZES = (4, 8, 16, 32, 50, 51, 64)  # the generated sorting networks (csrc/wbx_sortnet3_gen.hpp)
MEMBERS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 50, 51, 52, 64)  # every network size, both sides of every padding step
MUTANTS = ('fma', 'no_upper_branch', 'unclamped', 'no_nan_flag', 'transposed', 'float32', 'widened_difference')


def padded(m: int) -> int:
  """The network size an ensemble of m members is padded to (csrc/wbx_ens_park.hpp: ivl_padded)."""
  return next(s for s in SIZES if m <= s)


def bound(q, m: int):
  """(k, g): h = q (m - 1), k = floor(h), g = h - k, in float64 (engine.ivl_bound)."""
  h = float(q) * (int(m) - 1)
  k = math.floor(h)
  return int(k), h - k


def around_half(m: int):
  """Two levels of m >= 2 members whose weights g lie just under and just over 0.5 (the two branches of the lerp)."""
  mid = (m - 1) // 2
  q = (mid + 0.5) / (m - 1)
  lo = hi = q
  while not bound(lo, m)[1] < 0.5:
    lo = np.nextafter(lo, 0.0)
  while not (bound(hi, m)[1] >= 0.5 and bound(hi, m)[1] != 0.5):
    hi = np.nextafter(hi, 1.0)
  assert bound(lo, m)[0] == bound(hi, m)[0] == mid and 0.49 < bound(lo, m)[1] < 0.5 < bound(hi, m)[1] < 0.51, (m, lo, hi)
  return float(lo), float(hi)


def levels(nq: int, m: int, exact=False):
  """nq quantile levels for m members.  General: out of 0, 1 (the upper rank clamps), 0.5, 0.1, 0.9, 1/3, the two around g = 0.5 and
  more deciles; unsorted, with a duplicate at 16.  Exact: multiples of 1/8."""
  if exact:
    pool = [0.5, 0.0, 1.0, 0.125, 0.875, 0.25, 0.75, 0.375, 0.625, 0.5, 1.0, 0.0, 0.125, 0.625, 0.75, 0.25]
    return np.array(pool[:nq], np.float64)
  under, over = around_half(m) if m >= 2 else (0.49, 0.51)
  if nq == 1:
    return np.array([0.5])
  if nq == 2:
    return np.array([0.9, 0.1])
  if nq == 3:
    return np.array([1.0, 1.0 / 3.0, 0.0])
  pool = [0.0, 1.0, 0.5, 0.1, 0.9, 1.0 / 3.0, under, over, 1.0, 0.2, 0.8, 0.3, 0.7, 0.4, 0.6, 0.05]
  return np.array(pool[:nq], np.float64)


def quantile_values(p, q):
  """p[M, frame...] -> float64 [Q, frame...]: NumPy's own quantiles of the members as they are (see the module docstring)."""
  with np.errstate(all='ignore'):
    return np.quantile(np.asarray(p), np.asarray(q, np.float64), axis=0).astype(np.float64)


def points(p, t, q):
  """The three statistics per point in float64 [frame..., 3 Q], lane stat * Q + j."""
  with np.errstate(all='ignore'):
    e = np.moveaxis(quantile_values(p, q), 0, -1) - np.asarray(t).astype(np.float64)[..., None]
    return np.concatenate([e, np.abs(e), e * e], axis=-1)


def _fma(a, b, c):
  """round(a * b + c) with ONE rounding, elementwise in float64 (exact rational arithmetic; non-finite operands as IEEE has them)."""
  a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
  with np.errstate(all='ignore'):
    out = np.array(a * b + c, np.float64)
  for i in np.ndindex(out.shape):
    if np.isfinite(a[i]) and np.isfinite(b[i]) and np.isfinite(c[i]):
      out[i] = float(fractions.Fraction(float(a[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(c[i])))
  return out


def model(p, t, q, mutant=None):
  """What the kernel computes per point, [frame..., 3 Q], step by step; `mutant`: one of MUTANTS, a mistake it could make."""
  assert mutant is None or mutant in MUTANTS
  p = np.asarray(p)
  m = p.shape[0]
  nan = np.isnan(p).any(axis=0)
  # the network's min / max drop a NaN: the slot holds the other operand, and the padding's +inf fills in at the end
  xs = np.sort(np.where(np.isnan(p), np.inf, p), axis=0)
  work = np.float32 if mutant == 'float32' else np.float64
  widen_first = mutant == 'widened_difference'  # (what ivl_quantile does: exact for float64 members, another number for float32)
  t = np.asarray(t).astype(np.float64)
  out = []
  with np.errstate(all='ignore'):
    for level in np.asarray(q, np.float64):
      k, g = bound(level, m)
      k1 = k + 1 if mutant == 'unclamped' else min(k + 1, m - 1)
      lo = xs[k]
      hi = xs[k1] if k1 < m else np.full_like(lo, np.inf)  # (past the members: the padding)
      d = (hi.astype(np.float64) - lo.astype(np.float64) if widen_first else hi - lo).astype(work)  # (else in the members' type)
      a, b = lo.astype(work), hi.astype(work)
      gw = work(g)
      if mutant == 'fma':
        low, high = _fma(d, gw, a), _fma(-d, work(1.0) - gw, b)
      else:
        low, high = a + d * gw, b - d * (work(1.0) - gw)
      val = (low if (g < 0.5 or mutant == 'no_upper_branch') else high).astype(np.float64)
      if mutant != 'no_nan_flag':
        val = np.where(nan, np.nan, val)
      out.append(val - t)
    e = np.stack(out, axis=-1)
    if mutant == 'transposed':  # lane j * 3 + stat
      return np.stack([e, np.abs(e), e * e], axis=-1).reshape(e.shape[:-1] + (-1,))
    return np.concatenate([e, np.abs(e), e * e], axis=-1)


def same_bits(a, b) -> bool:
  """Bit for bit, every NaN taken for every other and -0.0 for 0.0 (a sum that starts at 0.0 has no negative zero)."""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return a.shape == b.shape and bool(np.array_equal(np.isnan(a), np.isnan(b))) and bool(np.array_equal(a, b, equal_nan=True))


def expected(p, t, q, valid, flags, depth_chunk, x_kept):
  """p[M, lead, row, x], t[lead, row, x], valid[row, x] or None -> (want, bound) of what stage 1 writes, each
  [lead][chunk][lane][j]: the 3 Q value lanes, then the count lanes (one shared under a mask alone, one per value lane under skipna).
  `want`: x kept -- the rows added in order; x summed -- the correctly rounded sum.  `bound`: see the module docstring (0 for the
  count lanes and for x kept)."""
  v = points(p, t, q)                                        # [lead, row, x, 3 Q]
  nlead, nrow, nx, nl = v.shape
  ok = np.ones(v.shape, bool)
  if valid is not None and flags & FLAG_MASKED:
    ok = ok & np.asarray(valid, bool)[None, :, :, None]
  take = ok & ~np.isnan(v) if flags & FLAG_SKIPNA else ok
  with np.errstate(all='ignore'):
    vals = np.where(take, v, 0.0)
  nchunk = -(-nrow // depth_chunk)
  nj = nx if x_kept else 1
  want = np.zeros((nlead, nchunk, nl, nj))
  tol = np.zeros_like(want)
  counts = np.zeros_like(want)
  shared = np.zeros((nlead, nchunk, 1, nj))
  for c in range(nchunk):
    rows = slice(c * depth_chunk, min((c + 1) * depth_chunk, nrow))
    if x_kept:
      with np.errstate(all='ignore'):
        for r in range(rows.start, rows.stop):
          want[:, c] += np.moveaxis(vals[:, r], -1, 1)        # [lead, lane, x]: 0.0 + v_0 + v_1 ...
      counts[:, c] = np.moveaxis(take[:, rows].sum(axis=1), -1, 1)
      shared[:, c, 0] = ok[:, rows, :, 0].sum(axis=1)
      continue
    counts[:, c, :, 0] = take[:, rows].sum(axis=(1, 2))
    shared[:, c, 0, 0] = ok[:, rows, :, 0].sum(axis=(1, 2))
    for lead in range(nlead):
      for lane in range(nl):
        a = vals[lead, rows, :, lane].reshape(-1)
        if np.isfinite(a).all():
          want[lead, c, lane, 0] = math.fsum(a)
          tol[lead, c, lane, 0] = a.size * 2.0 ** -53 * math.fsum(np.abs(a))
        else:
          with np.errstate(all='ignore'):
            want[lead, c, lane, 0] = a.sum()                  # NaN, or the infinity every order of adding gives
  if flags & FLAG_SKIPNA:
    return np.concatenate([want, counts], axis=2), np.concatenate([tol, np.zeros_like(counts)], axis=2)
  if flags & FLAG_MASKED:
    return np.concatenate([want, shared], axis=2), np.concatenate([tol, np.zeros_like(shared)], axis=2)
  return want, tol


def case(seed, m, nlead, nrow, nx, dtype, flags, exact=False, clean=False):
  """-> p[M, lead, row, x] (C order), t[lead, row, x], mask[row, x].  General values: normal numbers of a few units with ties among the
  members; exact: integers in -8..8.  Unless `clean`, lead 0 carries the edges where the frame has room -- a NaN member, a NaN
  target, a +inf member, a -inf member (at q = 0 / q = 1 with g == 0 that is inf * 0), all members +inf -- in row 0 and the last row,
  so the other leads (and the middle chunk rows) stay finite; under a mask one partial (lead-independent rows x 0) is masked out
  whole where x is kept, and the mask hides one of the NaNs."""
  rng = np.random.default_rng(seed)
  if exact:
    p = rng.integers(-8, 9, (m, nlead, nrow, nx)).astype(dtype)
    t = rng.integers(-8, 9, (nlead, nrow, nx)).astype(dtype)
  else:
    p = (rng.standard_normal((m, nlead, nrow, nx)) * 3.0 + 1.0).astype(dtype)
    t = (rng.standard_normal((nlead, nrow, nx)) * 3.0 + 1.0).astype(dtype)
    if m >= 2:
      p[m - 1] = np.where(rng.random((nlead, nrow, nx)) < 0.3, p[0], p[m - 1])  # ties
  mask = rng.random((nrow, nx)) < 0.7
  mask[:, 0] = False  # x = 0: masked out in every row (an all-masked partial where x is kept; all of it where nx == 1)
  if not clean:
    last = nrow - 1
    spots = [(0, min(1, nx - 1)), (0, min(2, nx - 1)), (last, min(3, nx - 1)), (last, min(4, nx - 1)), (last, nx - 1), (0, nx // 2)]
    p[rng.integers(0, m), 0, spots[0][0], spots[0][1]] = np.nan
    t[0, spots[1][0], spots[1][1]] = np.nan
    p[0, 0, spots[2][0], spots[2][1]] = np.inf
    p[m - 1, 0, spots[3][0], spots[3][1]] = -np.inf
    p[:, 0, spots[4][0], spots[4][1]] = np.inf
    if nx > 8:
      p[0, 0, spots[5][0], spots[5][1]] = np.nan
      mask[spots[5][0], spots[5][1]] = False    # a NaN the mask hides
      mask[spots[0][0], spots[0][1]] = True     # and one it does not
      mask[spots[2][0], spots[2][1]] = True
  return p, t, mask


def member_view(p, member_axis):
  """p[M, lead, row, x] stored with the member axis at `member_axis` (0: outermost; 3: innermost, member stride 1 and x stride M), as a
  view with the members first."""
  if member_axis == 0:
    return np.ascontiguousarray(p)
  return np.moveaxis(np.ascontiguousarray(np.moveaxis(p, 0, member_axis)), member_axis, 0)


def row_fastest(a):
  """a[..., row, x] stored with the ROW axis fastest (a latitude-fastest frame: x is strided), as a view in the same axis order."""
  return np.swapaxes(np.ascontiguousarray(np.swapaxes(a, -1, -2)), -1, -2)


def host_float32_bounds(p, t, q):
  """What the host route may differ by per point where it works in float32 throughout (torch.quantile keeps the input dtype; the
  kernel forms the quantile in float64): p[M, frame...], t[frame...] float32 -> float64 [frame..., 3 Q] laid out as `points`, a bound
  on |difference| of (e_j, |e_j|, e_j^2), from that route's rounding count and the point's own magnitudes.  With u = 2^-24,
  X = max|member|, R = max member - min member (no two neighbours are further apart), M members and e_j the restatement's error:
    the level is rounded to float32 and so is its product with M - 1: |dh| <= 2 u (M - 1), and the quantile is piecewise linear in
    h with slopes of at most R                                                                   -> 2 (M - 1) u R
    d = B - A is rounded in both routes alike; its product with the weight is rounded (<= u R), and so is the sum, a number between
    A and B (<= u X)                                                                             -> u (R + X)
  so the quantile differs by at most DQ = u (2 (M - 1) R + R + X); e = Q - t is rounded (<= u (|e_j| + DQ)), hence
  |de| <= D = DQ + u (|e_j| + DQ), the same for |e|; e^2: |2 e de| + de^2 + the rounding of the square
  <= 2 |e_j| D + D^2 + u (|e_j| + D)^2.  Second-order terms of u are kept: the bound is not first-order only.  NaN where e_j is."""
  u = 2.0 ** -24
  p64 = np.asarray(p, np.float64)
  m = p64.shape[0]
  with np.errstate(all='ignore'):
    x = np.abs(p64).max(axis=0)[..., None]
    r = (p64.max(axis=0) - p64.min(axis=0))[..., None]
    e = np.abs(points(p, t, q)[..., :len(q)])
    dq = u * (2.0 * (m - 1) * r + r + x)
    d = dq + u * (e + dq)
    return np.concatenate([d, d, 2.0 * e * d + d * d + u * (e + d) ** 2], axis=-1)
