"""Seeded inputs for the indicator (rank histogram / error exceedance) and two-ensemble tests
(tests/test_gpu_indicators.py, tests/test_indicators_edges.py).  A plain helper module, not a fixture file: pure NumPy.

Values sit on a dyadic grid (multiples of 0.25 of modest size), so `p - t` is exact in float32 and in float64 alike and a
tie -- a member equal to the target, an absolute error equal to a threshold -- is a tie on both sides of a comparison
whatever the input dtype.  With members on [-3, 3], targets on [-2, 2] and thresholds k * 0.25 about 7 % of all |p_m - t|
equal a threshold and about 4 % of the members equal the target: the strict `>` and `<` of the kernels are exercised
at every point.

In the plain mode (no mask, no skipna) one NaN statistic makes a whole output NaN, so the NaN targets and all-NaN points
go only into rows the caller names (`poison_rows`); everything else a plain-mode output sees is finite."""
import numpy as np


def gridded(rng, shape, lo, hi, step=0.25, dtype=np.float32):
  """Values k * step, k uniform on [lo / step, hi / step]: exact in float32 for |value| < 2^22 * step."""
  k = rng.integers(int(round(lo / step)), int(round(hi / step)) + 1, size=shape)
  return (k * step).astype(dtype)


def sprinkle(rng, a, nan=0.0, pinf=0.0, ninf=0.0, negzero=0.0):
  """`a` (in place) with NaN, +inf, -inf and -0.0 at the given shares of its elements; returns `a`."""
  u = rng.random(a.shape)
  edge = 0.0
  for share, value in ((nan, np.nan), (pinf, np.inf), (ninf, -np.inf), (negzero, -0.0)):
    a[(u >= edge) & (u < edge + share)] = value
    edge += share
  return a


def thresholds(ncat, nan_at=None, step=0.25):
  """float64[ncat]: multiples of `step` from 0 up, with (where they fit) one negative value, one +inf and one NaN among
  them.  Order is not monotone on purpose: the kernel must not assume it."""
  thr = np.arange(ncat, dtype=np.float64) * step
  if ncat >= 3:
    thr[1] = -step          # every finite error exceeds it, an error of exactly 0 too
    thr[ncat - 1] = np.inf  # nothing exceeds it
  if ncat >= 2:
    thr[ncat // 2 if nan_at is None else nan_at] = np.nan
  return thr


# the named special points, in the order place_special_points puts them along a row
SPECIAL = ('all_members_nan', 'one_valid_member', 'inf_minus_inf', 'nan_target')


def place_special_points(p, t, member_axis, row, first=0, step=1):
  """Writes the named special points into row `row` of the LAST-BUT-ONE axis of t (t is [..., row, x]; p is t with a member axis
  at `member_axis`) at x = first, first + step, ...: every leading index gets them.  Returns {name: x}.
    all_members_nan    every member NaN: exceedance NaN (0 / 0 members), rank 0
    one_valid_member   every member but the last NaN
    inf_minus_inf      t = +inf and member 0 = +inf: inf - inf is NaN (counted out of the member mean), inf < inf is false
    nan_target         t NaN: every |p - t| NaN, rank 0"""
  pm = np.moveaxis(p, member_axis, -1)  # [..., row, x, member] view
  where = {}
  for i, name in enumerate(SPECIAL):
    x = first + i * step
    if x >= t.shape[-1]:
      break
    where[name] = x
    if name == 'all_members_nan':
      pm[..., row, x, :] = np.nan
    elif name == 'one_valid_member':
      pm[..., row, x, :-1] = np.nan
      pm[..., row, x, -1] = 1.25
    elif name == 'inf_minus_inf':
      t[..., row, x] = np.inf
      pm[..., row, x, 0] = np.inf
    else:
      t[..., row, x] = np.nan
  return where


def indicator_case(seed, m, nlead, nrow, nx, dtype=np.float32, poison_rows=(), exposed_rows=None, nan=0.02, inf=0.01,
                   layout='member_outside', t_range=(-2, 2)):
  """One (predictions, targets, mask) triple.

  layout 'member_outside': p is [lead, member, row, x]; 'ifs': p is [member, lead, row, x] (a member's planes are not adjacent).
  Returned p is always indexed [lead, member, row, x] -- for 'ifs' a transposed VIEW of the contiguous [member, lead, row, x] base.
  t is [lead, row, x] on `t_range`, mask (bool) is [row, x], False on ~30 % of the points.
  NaN / infinite / -0.0 members are sprinkled everywhere (the member mean skips them; they never make an output NaN by
  themselves as long as a point keeps one finite member -- with m <= 2 they would, so the sprinkle is left out there);
  the special points (all members NaN, NaN target, inf - inf ...) go into `poison_rows` only.
  The mask at the points whose statistic is NaN: on `exposed_rows` (default: every poisoned row) True at the NaN target of
  the first, third ... such row and False at the others'; on the other poisoned rows False at every such point."""
  rng = np.random.default_rng(seed)
  shape = (m, nlead, nrow, nx) if layout == 'ifs' else (nlead, m, nrow, nx)
  base = gridded(rng, shape, -3, 3, dtype=dtype)
  if m > 2:
    sprinkle(rng, base, nan=nan, pinf=inf / 2, ninf=inf / 2, negzero=0.01)
  p = np.transpose(base, (1, 0, 2, 3)) if layout == 'ifs' else base
  t = gridded(rng, (nlead, nrow, nx), t_range[0], t_range[1], dtype=dtype)
  sprinkle(rng, t, negzero=0.01)
  mask = rng.random((nrow, nx)) > 0.3
  exposed = set(poison_rows if exposed_rows is None else exposed_rows)
  for i, row in enumerate(poison_rows):
    where = place_special_points(p, t, 1, row)
    if row in exposed:
      if 'nan_target' in where:
        mask[row, where['nan_target']] = i % 2 == 0
    else:
      for name in ('all_members_nan', 'nan_target') + (('inf_minus_inf',) if m == 1 else ()):
        if name in where:
          mask[row, where[name]] = False
  return p, t, mask
