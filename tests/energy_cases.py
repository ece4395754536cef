"""Inputs, the float64 restatement and per-point error bounds for the energy score of an ensemble (wbx_ens_energy_partial), plain
NumPy.

Restatement (include/wbx.h): per point with members x_m in R^L (m < M) and target y in R^L
    lane 0 (skill)  = (sum_m ||x_m - y||) / M
    lane 1 (spread) = (sum_{m != m'} ||x_m - x_m'||) / D,   D = M (M - 1) when fair, M^2 otherwise
in float64 on the float64-widened inputs, NaN and inf as IEEE arithmetic gives them (a member is never paired with itself).

Bounds, derived from the kernel's documented arithmetic and never from what it gives.  u = 2^-24 for a float32 launch, 2^-53 for a
float64 one.  A norm: every difference is rounded once (relative u each, so relative 2 u on its square and on the sum of squares),
the sum of squares takes at most L fma roundings (relative L u on a sum of non-negative terms), the root is correctly rounded
(halves the relative error of its argument, adds u): (2 u + L u) / 2 + u <= (L / 2 + 4) u.  Every term of both lanes is a
non-negative norm, so the same relative bound holds for the lanes' sums; the float64 part -- at most M (M - 1) / 2 additions, a
doubling, a division -- adds (M^2 + 4) 2^-53.  A partial of N points: the sum of its points' bounds + (N + 2) 2^-53 sum |value|.
Where the expectation is +-inf or NaN the output must be of the same class at the same place, per lane; count lanes are bit-equal.

Values: dyadic grids in [-8, 8] (multiples of 1/8: no square overflows or underflows in float32), tight clusters 280 + k 2^-10
(exactly representable in float32, whose spacing there is 2^-15), points whose members all equal the target (both lanes exactly 0),
and the non-finite points: an inf member, two +inf members, a NaN member, a NaN target only."""
import numpy as np

from contingency_cases import expected_partials  # the chunking of [lead, row, x, lane] into [lead][chunk][lane][j]

FLAG_MASKED, FLAG_SKIPNA, FLAG_FAIR = 1, 2, 4
NLANE = 2
LDS_CHUNK = 16  # elements of the norm run the kernel stages at a time
MEMBER_AXES = ('outer', 'inner')
NORM_AXES = ('outer', 'middle', 'inner', 'tdiff')
NONFINITE = ('inf_member', 'two_inf', 'nan_member', 'nan_target')


def unit(dtype) -> float:
  return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def relative_bound(m: int, l: int, dtype) -> float:
  return (l / 2.0 + 4.0) * unit(dtype) + (m * m + 4.0) * 2.0 ** -53


def host_relative_bound(m: int, l: int, dtype) -> float:
  """The host route's (labelled-array arithmetic in the input type): the same norms, (L / 2 + 4) u, then added in the input type too
  -- M terms for the skill (M u more), M - 1 passes of M terms and the M - 1 pass sums for the spread (2 M u more)."""
  return (l / 2.0 + 4.0 + 2.0 * m) * unit(dtype)


def energy_points(p, t, fair):
  """p[M, frame..., L], t[frame..., L] -> stat[frame..., 2] in float64."""
  x = np.asarray(p).astype(np.float64)
  y = np.asarray(t).astype(np.float64)
  m = x.shape[0]
  with np.errstate(all='ignore'):
    skill = np.sqrt(((x - y[None]) ** 2).sum(axis=-1)).sum(axis=0) / m
    pairs = np.zeros(y.shape[:-1])
    for i in range(m - 1):  # every unordered pair once; the ordered sum is twice that
      pairs = pairs + np.sqrt(((x[i + 1:] - x[i][None]) ** 2).sum(axis=-1)).sum(axis=0)
    spread = 2.0 * pairs / (m * (m - 1) if fair else m * m)
  return np.stack([skill, spread], axis=-1)


def expected(p, t, fair, valid, flags, depth_chunk, x_kept):
  """-> (want[lead][chunk][lane][j], bound of the same shape (0 on count lanes; meaningless where want is not finite), stat)."""
  stat = energy_points(p, t, fair)
  mode = flags & (FLAG_MASKED | FLAG_SKIPNA)
  want = expected_partials(stat, valid, mode, depth_chunk, x_kept)
  m, l = p.shape[0], p.shape[-1]
  mag = np.where(np.isfinite(stat), np.abs(stat), 0.0)
  summed = expected_partials(mag, valid, mode, depth_chunk, x_kept)[:, :, :NLANE]
  n = min(depth_chunk, stat.shape[1]) * (1 if x_kept else stat.shape[2])
  bound = np.zeros(want.shape)
  bound[:, :, :NLANE] = (relative_bound(m, l, p.dtype) + (n + 2) * 2.0 ** -53) * summed
  return want, bound, stat


def check(got, want, bound, tag):
  """Every lane of every partial: the class where the expectation is not finite, the bound where it is."""
  assert got.shape == want.shape, (tag, got.shape, want.shape)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{tag}: NaN positions')
  inf = np.isinf(want)
  np.testing.assert_array_equal(got[inf], want[inf], err_msg=f'{tag}: infinities')
  fin = np.isfinite(want)
  err = np.abs(got[fin] - want[fin])
  worst = float((err - bound[fin]).max()) if err.size else 0.0
  assert (err <= bound[fin]).all(), (tag, 'worst excess over the bound', worst, 'largest error', float(err.max()), 'largest bound',
                                     float(bound[fin].max()))
  return float(err.max()) if err.size else 0.0


def arrange(p, t, member='outer', norm='inner'):
  """Views of p[M, lead, row, x, l], t[lead, row, x, l] with the same values stored otherwise.  member: the member axis outermost
  in memory or innermost (stride 1).  norm: the norm axis outermost, in the middle (between lead and row), innermost (stride 1) in
  both inputs, or ('tdiff') innermost in p and outermost in t.  With member = 'inner' the norm axis of p is the next one out."""
  order = {'outer': (4, 1, 2, 3), 'middle': (1, 4, 2, 3), 'inner': (1, 2, 3, 4), 'tdiff': (1, 2, 3, 4)}[norm]
  porder = ((0,) + order) if member == 'outer' else (order + (0,))
  pv = np.ascontiguousarray(np.transpose(p, porder)).transpose(np.argsort(porder))
  torder = tuple(a - 1 for a in ({'tdiff': (4, 1, 2, 3)}.get(norm, order)))
  tv = np.ascontiguousarray(np.transpose(t, torder)).transpose(np.argsort(torder))
  assert pv.shape == p.shape and tv.shape == t.shape
  return pv, tv


def _put(p, t, rng, lead, row, x, kind):
  m, l = p.shape[0], p.shape[-1]
  e = int(rng.integers(0, l))
  if kind == 'inf_member':
    p[int(rng.integers(0, m)), lead, row, x, e] = np.inf if rng.random() < 0.5 else -np.inf
  elif kind == 'two_inf':
    a, b = rng.choice(m, size=2, replace=False)
    p[a, lead, row, x, e] = p[b, lead, row, x, e] = np.inf
  elif kind == 'nan_member':
    p[int(rng.integers(0, m)), lead, row, x, e] = np.nan
  else:
    t[lead, row, x, e] = np.nan


def energy_case(seed, m, l, nlead, nrow, nx, dtype, flags, depth_chunk, x_kept):
  """-> p[M, lead, row, x, l], t[lead, row, x, l] (C order), mask[row, x].

  Non-finite points (NONFINITE in turn): under skipna anywhere; otherwise into at most min(3, npartial // 5) distinct partials (one
  point each), so that at least 80 % of the expected partials are finite; under a mask three more sit under masked-out points,
  where they must leave no trace."""
  rng = np.random.default_rng(seed)
  shape = (nlead, nrow, nx)
  n = int(np.prod(shape))
  p = (rng.integers(-64, 65, size=(m,) + shape + (l,)) / 8.0).astype(dtype)
  t = (rng.integers(-64, 65, size=shape + (l,)) / 8.0).astype(dtype)
  kind = rng.integers(0, 8, size=shape)  # 0..4 the dyadic grid, 5..6 a tight cluster, 7 all members equal to the target
  tight = kind >= 5
  p[:, tight] = (280.0 + rng.integers(0, 1024, size=(m, int(tight.sum()), l)) * 2.0 ** -10).astype(dtype)
  t[tight] = (280.0 + rng.integers(0, 1024, size=(int(tight.sum()), l)) * 2.0 ** -10).astype(dtype)
  same = kind == 7
  p[:, same] = t[same][None]
  mask = rng.random((nrow, nx)) > 0.3
  if flags & FLAG_SKIPNA:
    for i in range(max(4, n // 25)):
      lead, row, x = (int(rng.integers(0, s)) for s in shape)
      _put(p, t, rng, lead, row, x, NONFINITE[i % 4])
      if i < 4:
        mask[row, x] = True  # (at least four of them count)
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
      _put(p, t, rng, lead, row, x, NONFINITE[(seed + i) % 4])
      mask[row, x] = True  # a non-finite point that counts
      taken.add((row, x))
    if flags & FLAG_MASKED:  # ... and those the mask hides (the mask has no lead axis: hidden for every lead)
      free = [(r, x) for r in range(nrow) for x in range(nx) if (r, x) not in taken]
      for i in range(min(3, len(free))):
        row, x = free[int(rng.integers(0, len(free)))]
        mask[row, x] = False
        _put(p, t, rng, int(rng.integers(0, nlead)), row, x, NONFINITE[(seed + i + 1) % 4])
  return p, t, mask
