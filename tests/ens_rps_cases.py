"""Inputs and the integer restatement for the ranked probability score of an ensemble (wbx_ens_rps_partial), plain NumPy.

Restatement (include/wbx.h): per point with members x_m, target y, prediction thresholds a_k and target thresholds b_k
    c_k = #{m : float64(x_m) <= a_k},  o_k = [float64(y) <= b_k]         (< instead of <= when not right-inclusive)
    fair:    n_k = (M - 1) (c_k - o_k M)^2 - c_k (M - c_k),  D = M^2 (M - 1)
    unfair:  n_k = (c_k - o_k M)^2,                          D = M^2
    RPS = (sum_k n_k) / D, NaN where a member or the target is NaN.
A stage-1 partial is float64(S) / float64(D) with S the int64 sum of sum_k n_k over its points: tests compare bit for bit.

Inputs sit on a dyadic grid (multiples of 1/8: ties with the thresholds are real ties) with the edges sprinkled in: values equal
to a threshold, float32(0.1) and both neighbours against the threshold 0.1, +-inf, +-0.0, points whose members are all -inf (at
or below every threshold: c = M) and points whose members are all +inf."""
import numpy as np

from contingency_cases import expected_partials  # the chunking of [lead, row, x, lane] into [lead][chunk][lane][j]

FLAG_MASKED, FLAG_SKIPNA, FLAG_FAIR = 1, 2, 4
F32_TENTH = np.float32(0.1)  # > 0.1 in float64
F32_BELOW_TENTH = np.nextafter(F32_TENTH, np.float32(-np.inf))
F32_ABOVE_TENTH = np.nextafter(F32_TENTH, np.float32(np.inf))

# (prediction thresholds a, target thresholds b) by K
_A16 = np.array([0.25, -0.25, 1.0, np.inf, 0.1, 0.0, 0.25, -1.5, 1.75, -np.inf, 1e40, -1e40, 0.5, -0.0, 0.125, -1.0])
THRESHOLDS = {
    1: (np.array([0.0]), np.array([0.0])),
    3: (np.array([0.1, 0.0, 0.1]), np.array([0.1, 0.0, 0.1])),                                        # unsorted, a duplicate
    5: (np.array([-1.0, -0.25, 0.1, 0.5, 1.0]), np.array([-0.75, -0.25, 0.125, 0.5, 1.25])),          # a_k != b_k
    16: (_A16, _A16[::-1].copy()),  # +-inf, +-1e40 (beyond the float32 range), 0.1, 0.0 and -0.0 (one threshold), ties with the grid
}


def thresholds(nthr: int):
  a, b = THRESHOLDS[nthr]
  return a.copy(), b.copy()


def denominator(m: int, fair: bool) -> float:
  return float(m * m * (m - 1)) if fair else float(m * m)


def counts(p, a, right):
  """p[M, frame...] -> c[frame..., K] int64: members at or below (below) every prediction threshold, compared in float64."""
  x = np.asarray(p).astype(np.float64)[..., None]
  with np.errstate(invalid='ignore'):
    below = (x <= np.asarray(a, np.float64)) if right else (x < np.asarray(a, np.float64))
  return below.sum(axis=0).astype(np.int64)


def numerators(p, t, a, b, fair, right):
  """p[M, frame...], t[frame...] -> sum_k n_k per point as int64 (meaningless where nan_points says NaN)."""
  m = int(np.asarray(p).shape[0])
  c = counts(p, a, right)
  y = np.asarray(t).astype(np.float64)[..., None]
  with np.errstate(invalid='ignore'):
    o = ((y <= np.asarray(b, np.float64)) if right else (y < np.asarray(b, np.float64))).astype(np.int64)
  e = c - o * m
  n = (m - 1) * e * e - c * (m - c) if fair else e * e
  return n.sum(axis=-1)


def nan_points(p, t):
  return np.isnan(np.asarray(p)).any(axis=0) | np.isnan(np.asarray(t))


def rps_points(p, t, a, b, fair, right):
  """The per-point score in float64, NaN where a member or the target is NaN."""
  out = numerators(p, t, a, b, fair, right).astype(np.float64) / denominator(np.asarray(p).shape[0], fair)
  out[nan_points(p, t)] = np.nan
  return out


def point_bound(stat):
  """What a per-point value of rps_points can be off by: its one division (sum_k n_k is an exact integer), 2^-53 relatively; 0
  where the value is NaN.  The kernel divides once per partial, after an exact integer sum: it has no per-point error at all."""
  return np.where(np.isfinite(stat), 2.0 ** -53 * np.abs(stat), 0.0)


def term_magnitudes(p, t, a, b, fair, right):
  """Per point, sum_k of the absolute values of the terms whose difference is the score: (c_k / M - o_k)^2 and, when fair,
  c_k (M - c_k) / (M^2 (M - 1)).  A route that forms the score from these in floating point, as the host route does, is accurate
  relative to this sum and not to the score, which may be their exact cancellation (0 where no rounding at all would be allowed)."""
  m = int(np.asarray(p).shape[0])
  c = counts(p, a, right).astype(np.float64)
  y = np.asarray(t).astype(np.float64)[..., None]
  with np.errstate(invalid='ignore'):
    o = ((y <= np.asarray(b, np.float64)) if right else (y < np.asarray(b, np.float64))).astype(np.float64)
  terms = (c / m - o) ** 2
  if fair:
    terms = terms + c * (m - c) / float(m * m * (m - 1))
  return terms.sum(axis=-1)


def expected(p, t, a, b, fair, right, valid, flags, depth_chunk, x_kept):
  """-> (what stage 1 writes, [lead][chunk][lane][j]: the value lane, then the count lane under a mask and / or skipna; the
  statistic of every point as integers held in float64, NaN where it is NaN)."""
  stat = numerators(p, t, a, b, fair, right).astype(np.float64)  # |sum_k n_k| < 2^31: exact, and so are sums of < 2^22 of them
  stat[nan_points(p, t)] = np.nan
  want = expected_partials(stat[..., None], valid, flags & (FLAG_MASKED | FLAG_SKIPNA), depth_chunk, x_kept)
  want[:, :, 0] = want[:, :, 0] / denominator(np.asarray(p).shape[0], fair)  # float64(S) / float64(D)
  return want, stat


def ens_rps_case(seed, m, nlead, nrow, nx, dtype, flags, depth_chunk, x_kept, a, member_innermost=False):
  """-> p[M, lead, row, x] (`member_innermost`: a view of an array stored [lead][row][x][M]: member stride 1, x stride M),
  t[lead, row, x], mask[row, x].

  NaNs (one member only, the target only, both): under skipna anywhere; otherwise a NaN under a valid point poisons its whole
  partial, so such NaNs go into at most 20 % of the partials (one point each, none where that share is less than one partial);
  under a mask three more sit under masked-out points, where they must leave no trace."""
  rng = np.random.default_rng(seed)
  shape = (nlead, nrow, nx)
  n = int(np.prod(shape))
  p = (rng.integers(-16, 17, size=(m,) + shape) / 8.0).astype(dtype)
  t = (rng.integers(-16, 17, size=shape) / 8.0).astype(dtype)
  edges = [F32_TENTH, F32_BELOW_TENTH, F32_ABOVE_TENTH, np.inf, -np.inf, -0.0, 0.0] + [v for v in np.asarray(a) if np.isfinite(v) and abs(v) < 1e30]
  if np.dtype(dtype) == np.float64:
    edges += [0.1, np.nextafter(0.1, np.inf), np.nextafter(0.1, -np.inf)]
  for arr in (p, t):
    flat = arr.reshape(-1)
    for v in edges:
      flat[rng.integers(0, flat.size, size=max(1, flat.size // 40))] = v
  pf = p.reshape(m, n)
  for v in (-np.inf, np.inf):  # every member at or below every threshold (c = M); no member below any finite one
    pf[:, rng.integers(0, n, size=max(1, n // 30))] = v
  mask = rng.random((nrow, nx)) > 0.3
  nan_kinds = [(True, False), (False, True), (True, True)]  # (one member of p, t)

  def put_nan(lead, row, x, kind):
    if kind[0]:
      p[int(rng.integers(0, m)), lead, row, x] = np.nan
    if kind[1]:
      t[lead, row, x] = np.nan

  if flags & FLAG_SKIPNA:
    for i in range(max(3, n // 25)):
      lead, row, x = (int(rng.integers(0, s)) for s in shape)
      put_nan(lead, row, x, nan_kinds[i % 3])
      if i < 3:
        mask[row, x] = True  # (at least three of them count)
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
      put_nan(lead, row, x, nan_kinds[(seed + i) % 3])
      mask[row, x] = True  # a NaN under a VALID point
      taken.add((row, x))
    if flags & FLAG_MASKED:  # ... and NaNs the mask hides (the mask has no lead axis: hidden for every lead)
      free = [(r, x) for r in range(nrow) for x in range(nx) if (r, x) not in taken]
      for i in range(min(3, len(free))):
        row, x = free[int(rng.integers(0, len(free)))]
        mask[row, x] = False
        put_nan(int(rng.integers(0, nlead)), row, x, nan_kinds[i % 3])
  if member_innermost:
    p = np.moveaxis(np.ascontiguousarray(np.moveaxis(p, 0, -1)), -1, 0)
  return p, t, mask
