"""Inputs, the float64 restatement, an exact evaluation and per-point error bounds for the Wasserstein-1 distance between two
ensembles (wbx_ens_wasserstein_partial), plain NumPy.

Restatement (include/wbx.h): per point with the sorted members p_(0) <= ... <= p_(M-1) and t_(0) <= ... <= t_(N-1)
    W1 = ( sum over pieces of c |p_(i) - t_(j)| ) / (M N)
over the M + N - gcd(M, N) pieces between consecutive breakpoints of {i / M} u {j / N}: c = min((i + 1) N, (j + 1) M) - max(i N, j M),
i advances when (i + 1) N <= (j + 1) M, j when (j + 1) M <= (i + 1) N.  In float64 on the float64-widened inputs, here with every
operation rounded on its own (the kernel fuses the product and the addition), the sum in the order of the walk, one division at the
end.  A NaN member on either side makes the point NaN;
so do two or more +inf among the pooled M + N members, and two or more -inf; anything else is what the arithmetic gives.

Exact evaluation: on a dyadic grid sum c |p - t| is exact in float64, so the kernel's per-point value must equal
float(S) / float(M N), S the sum in fractions.Fraction, bit for bit.

Bounds, derived from the kernel's documented arithmetic and never from what it gives.  Both the kernel and the restatement sum at
most M + N non-negative terms with at most three roundings each (the difference, the product, the addition) and divide once:
relative (M + N + 4) 2^-53 a side, whatever the launch dtype (everything after the exact sort is float64):
    bound of the point = 2 (M + N + 4) 2^-53 W1
A partial of n points: the sum of its points' bounds + (n + 2) 2^-53 sum |value|.  Where the expectation is NaN or +inf the output
must be the same at the same place; count lanes are bit-equal.

Values, a class per point: a dyadic grid in [-8, 8] (multiples of 1/8), tight clusters 280 + k 2^-10, every member of both sides
equal (exactly 0), ties between the two ensembles, duplicated members, +-0.0 among the members, subnormal float32 members
(multiples of 2^-149).  NaN-making points (NAN_KINDS): a NaN member in p, one in t, two +inf in p, +inf in p and +inf in t, two -inf
in t.  Single infinities (INF_KINDS, the value is +inf) are put by the tests that keep every dim only."""
import fractions
import math

import numpy as np

from contingency_cases import expected_partials  # the chunking of [lead, row, x, lane] into [lead][chunk][lane][j]
import energy_cases as GC

FLAG_MASKED, FLAG_SKIPNA = 1, 2
NLANE = 1
MAX_MEMBERS = 64
NETWORK_SIZES = (4, 8, 16, 32, 50, 51, 64)  # the generated sorting networks a side is padded to (csrc/wbx_ens_wasserstein.hip)
MEMBER_AXES = ('outer', 'middle', 'inner')
NAN_KINDS = ('nan_p', 'nan_t', 'two_pinf_p', 'pinf_p_pinf_t', 'two_ninf_t')
INF_KINDS = ('pinf_p', 'ninf_t', 'ninf_p_pinf_t', 'ninf_p_pinf_p')
check, unit = GC.check, GC.unit


def padded(m: int) -> int:
  return next(s for s in NETWORK_SIZES if m <= s)


def pieces(m: int, n: int):
  """The walk: [(i, j, c)] in order, c in units of 1 / (m n)."""
  out, i, j = [], 0, 0
  while i < m and j < n:
    out.append((i, j, min((i + 1) * n, (j + 1) * m) - max(i * n, j * m)))
    ai, aj = (i + 1) * n <= (j + 1) * m, (j + 1) * m <= (i + 1) * n
    i, j = i + ai, j + aj
  return out


def nan_rule(p, t):
  """p[M, frame...], t[N, frame...] -> bool[frame...]: the points the non-finite rule makes NaN."""
  both = np.concatenate([np.asarray(p, np.float64), np.asarray(t, np.float64)], axis=0)
  return np.isnan(both).any(axis=0) | ((both == np.inf).sum(axis=0) >= 2) | ((both == -np.inf).sum(axis=0) >= 2)


def wasserstein_points(p, t):
  """p[M, frame...], t[N, frame...] -> (W1[frame...], bound[frame...]) in float64; the bound is meaningless where W1 is not
  finite."""
  x = np.sort(np.asarray(p).astype(np.float64), axis=0)
  y = np.sort(np.asarray(t).astype(np.float64), axis=0)
  m, n = x.shape[0], y.shape[0]
  total = np.zeros(x.shape[1:])
  with np.errstate(all='ignore'):
    for i, j, c in pieces(m, n):
      total = total + float(c) * np.abs(x[i] - y[j])
    w1 = total / float(m * n)
  w1 = np.where(nan_rule(p, t), np.nan, w1)
  bound = np.where(np.isfinite(w1), 2.0 * (m + n + 4) * 2.0 ** -53 * np.abs(w1), 0.0)
  return w1, bound


def exact_points(p, t):
  """The same on finite inputs, S = sum c |p_(i) - t_(j)| in exact rational arithmetic: float(S) / float(M N), point by point."""
  x = np.sort(np.asarray(p).astype(np.float64), axis=0)
  y = np.sort(np.asarray(t).astype(np.float64), axis=0)
  m, n = x.shape[0], y.shape[0]
  walk = pieces(m, n)
  xf, yf = x.reshape(m, -1), y.reshape(n, -1)
  out = np.empty(xf.shape[1])
  for q in range(xf.shape[1]):
    px, ty = [fractions.Fraction(float(v)) for v in xf[:, q]], [fractions.Fraction(float(v)) for v in yf[:, q]]
    s = sum((c * abs(px[i] - ty[j]) for i, j, c in walk), fractions.Fraction(0))
    f = float(s)
    assert fractions.Fraction(f) == s, 'the sum must be exact in float64 for this comparison to be fair'
    out[q] = f / float(m * n)
  return out.reshape(x.shape[1:])


def expected(p, t, valid, flags, depth_chunk, x_kept):
  """-> (want[lead][chunk][lane][j], bound of the same shape (0 on count lanes; meaningless where want is not finite), stat[lead, row, x])."""
  stat, pbound = wasserstein_points(p, t)
  mode = flags & (FLAG_MASKED | FLAG_SKIPNA)
  want = expected_partials(stat[..., None], valid, mode, depth_chunk, x_kept)
  mag = np.where(np.isfinite(stat), np.abs(stat), 0.0)[..., None]
  summed = expected_partials(mag, valid, mode, depth_chunk, x_kept)[:, :, :NLANE]
  own = expected_partials(pbound[..., None], valid, mode, depth_chunk, x_kept)[:, :, :NLANE]
  k = min(depth_chunk, stat.shape[1]) * (1 if x_kept else stat.shape[2])
  bound = np.zeros(want.shape)
  bound[:, :, :NLANE] = own + (k + 2) * 2.0 ** -53 * summed
  return want, bound, stat


def arrange(a, member='outer'):
  """A view of a[members, lead, row, x] with the same values stored otherwise: the member axis outermost in memory, in the middle
  (between lead and row) or innermost (stride 1)."""
  order = {'outer': (0, 1, 2, 3), 'middle': (1, 0, 2, 3), 'inner': (1, 2, 3, 0)}[member]
  v = np.ascontiguousarray(np.transpose(a, order)).transpose(np.argsort(order))
  assert v.shape == a.shape
  return v


def put(p, t, rng, at, kind):
  """Make the point `at` = (lead, row, x) one of NAN_KINDS / INF_KINDS (ensembles of one member take the nearest kind that fits)."""
  m, n = p.shape[0], t.shape[0]
  a, b = int(rng.integers(0, m)), int(rng.integers(0, n))
  if kind == 'nan_p':
    p[(a,) + at] = np.nan
  elif kind == 'nan_t':
    t[(b,) + at] = np.nan
  elif kind == 'two_pinf_p' and m > 1:
    p[(a,) + at] = p[((a + 1) % m,) + at] = np.inf
  elif kind in ('pinf_p_pinf_t', 'two_pinf_p'):
    p[(a,) + at] = t[(b,) + at] = np.inf
  elif kind == 'two_ninf_t' and n > 1:
    t[(b,) + at] = t[((b + 1) % n,) + at] = -np.inf
  elif kind == 'two_ninf_t':
    p[(a,) + at] = t[(b,) + at] = -np.inf
  elif kind == 'pinf_p':
    p[(a,) + at] = np.inf
  elif kind == 'ninf_t':
    t[(b,) + at] = -np.inf
  elif kind == 'ninf_p_pinf_t':
    p[(a,) + at], t[(b,) + at] = -np.inf, np.inf
  elif kind == 'ninf_p_pinf_p' and m > 1:
    p[(a,) + at], p[((a + 1) % m,) + at] = -np.inf, np.inf
  elif kind == 'ninf_p_pinf_p':
    p[(a,) + at] = -np.inf
  else:
    raise ValueError(kind)


def values(seed, m, n, shape, dtype):
  """-> p[M, shape...], t[N, shape...] (C order), finite: the value classes, one per point."""
  rng = np.random.default_rng(seed)
  p = (rng.integers(-64, 65, size=(m,) + shape) / 8.0).astype(dtype)
  t = (rng.integers(-64, 65, size=(n,) + shape) / 8.0).astype(dtype)
  kind = rng.integers(0, 10, size=shape)  # 0..3 the dyadic grid, then one class each
  tight = kind == 4
  p[:, tight] = (280.0 + rng.integers(0, 1024, size=(m, int(tight.sum()))) * 2.0 ** -10).astype(dtype)
  t[:, tight] = (280.0 + rng.integers(0, 1024, size=(n, int(tight.sum()))) * 2.0 ** -10).astype(dtype)
  same = kind == 5  # every member of both sides equal: exactly 0
  p[:, same] = p[0][same][None]
  t[:, same] = p[0][same][None]
  ties = kind == 6  # members of t that are members of p
  for j in range(0, n, 2):
    t[j][ties] = p[j % m][ties]
  dup = kind == 7  # duplicated members on both sides
  for i in range(1, m, 2):
    p[i][dup] = p[i - 1][dup]
  for j in range(1, n, 3):
    t[j][dup] = t[j - 1][dup]
  zeros = kind == 8  # +-0.0 among the members
  p[0][zeros] = -0.0
  t[0][zeros] = 0.0
  if m > 1:
    p[1][zeros] = 0.0
  if n > 1:
    t[1][zeros] = -0.0
  sub = kind == 9  # subnormal float32 members (ordinary small numbers in float64)
  p[:, sub] = (rng.integers(-4096, 4097, size=(m, int(sub.sum()))) * 2.0 ** -149).astype(dtype)
  t[:, sub] = (rng.integers(-4096, 4097, size=(n, int(sub.sum()))) * 2.0 ** -149).astype(dtype)
  return p, t


def wasserstein_case(seed, m, n, nlead, nrow, nx, dtype, flags, depth_chunk, x_kept):
  """-> p[M, lead, row, x], t[N, lead, row, x] (C order), mask[row, x], want, bound, stat (`expected` of them).

  NaN-making points (NAN_KINDS in turn), placed as tests/energy_cases.py places its non-finite points: under skipna anywhere;
  otherwise into at most min(3, npartial // 5) distinct partials (one point each); under a mask three more under masked-out points,
  where they must leave no trace.  Asserted here, on the restatement's output: no point is infinite; without skipna at least 80 % of
  the expected partials are finite; under skipna some point is NaN and no partial is."""
  rng = np.random.default_rng(seed + 7919)
  shape = (nlead, nrow, nx)
  p, t = values(seed, m, n, shape, dtype)
  mask = rng.random((nrow, nx)) > 0.3
  npoint = int(np.prod(shape))
  if flags & FLAG_SKIPNA:
    for i in range(max(5, npoint // 25)):
      at = tuple(int(rng.integers(0, s)) for s in shape)
      put(p, t, rng, at, NAN_KINDS[i % 5])
      if i < 5:
        mask[at[1], at[2]] = True  # (at least five of them count)
  else:
    nchunk = -(-nrow // depth_chunk)
    npartial = nlead * nchunk * (nx if x_kept else 1)
    allowed = min(3, npartial // 5)
    picks = rng.choice(npartial, size=allowed, replace=False) if allowed else []  # distinct partials
    taken = set()
    for i, q in enumerate(picks):
      q = int(q)
      x = q % nx if x_kept else int(rng.integers(0, nx))
      q = q // nx if x_kept else q
      lead, chunk = q // nchunk, q % nchunk
      row = min(chunk * depth_chunk + int(rng.integers(0, depth_chunk)), nrow - 1)
      put(p, t, rng, (lead, row, x), NAN_KINDS[(seed + i) % 5])
      mask[row, x] = True  # a NaN point that counts
      taken.add((row, x))
    if flags & FLAG_MASKED:  # ... and those the mask hides (the mask has no lead axis: hidden for every lead)
      free = [(r, x) for r in range(nrow) for x in range(nx) if (r, x) not in taken]
      for i in range(min(3, len(free))):
        row, x = free[int(rng.integers(0, len(free)))]
        mask[row, x] = False
        put(p, t, rng, (int(rng.integers(0, nlead)), row, x), NAN_KINDS[(seed + i + 1) % 5])
  want, bound, stat = expected(p, t, mask, flags, depth_chunk, x_kept)
  assert not np.isinf(stat).any()
  if flags & FLAG_SKIPNA:
    assert np.isnan(stat).any() and not np.isnan(want).any(), (seed, m, n)
  else:
    share = float(np.isfinite(want[:, :, 0]).mean())
    assert share >= 0.8, (seed, m, n, nx, 'finite share of the partials', share)
  return p, t, mask, want, bound, stat


def piece_count(m: int, n: int) -> int:
  return m + n - math.gcd(m, n)
