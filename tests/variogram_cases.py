"""Inputs, the float64 restatement and per-point error bounds for the variogram score of an ensemble (wbx_ens_variogram_partial),
plain NumPy.

Restatement (include/wbx.h): per point with members x_m in R^L (m < M) and target y in R^L
    VS = sum_{i, j in [0, L)} ( |y_i - y_j|^p - (1 / M) sum_m |x_i^m - x_j^m|^p )^2
over ordered pairs, the diagonal included: 2 * (sum over i < j) where every one of the (M + 1) L inputs is finite, NaN where any is
NaN or infinite (the diagonal |v - v|^p).  In float64 on the float64-widened inputs.

Bounds, derived from the kernel's documented arithmetic and never from what it gives.  u = 2^-24 for a float32 launch, 2^-53 for a
float64 one.  Per pair, with ty = |y_i - y_j|^p, tx = mean_m |x_i^m - x_j^m|^p and e = ty - tx of the restatement: a term |d|^p is
formed in the input type with relative error c u -- c = 1.5 for p = 0.5 (the difference rounded once, halved by a correctly rounded
root, which adds one), 1 for p = 1 (the difference rounded once), 3 for p = 2 (the difference rounded once, squared, the product
rounded once) --; the float64 member sum of M non-negative terms, its division and the subtraction add (M + 2) 2^-53 tx and
2^-53 (ty + tx):
    delta = c u (ty + tx) + (M + 2) 2^-53 tx + 2^-53 (ty + tx)
    bound of the pair  = 2 |e| delta + delta^2
    bound of the point = 2 * (sum over i < j) + (L^2 + 4) 2^-53 VS        (the squares, the pair sum in any order, the doubling)
A partial of n points: the sum of its points' bounds + (n + 2) 2^-53 sum |value|.  Where the expectation is NaN the output must be
NaN at the same place; count lanes are bit-equal.

Values: the classes of tests/energy_cases.py -- dyadic grids in [-8, 8], tight clusters 280 + k 2^-10, points whose members all
equal the target (the score is exactly 0), and the non-finite points (an inf member, two +inf members, a NaN member, a NaN target),
every one of which must give NaN here.

Staging boundaries of the kernel (csrc/wbx_ens_variogram.hip), restated: a tile holds tile_points(L) adjacent x -- what ITEMS_TOTAL
(point, pair) items and TGT_ELEMS target elements hold, PMAX at most --; the members of a tile are staged member_chunk(M, L) at a
time -- what STAGE_ELEMS elements hold."""
import numpy as np

from contingency_cases import expected_partials  # the chunking of [lead, row, x, lane] into [lead][chunk][lane][j]
import energy_cases as GC

FLAG_MASKED, FLAG_SKIPNA = 1, 2
NLANE = 1
POWERS = {0.5: 0, 1.0: 1, 2.0: 2}          # p -> the entry's code
ROUNDINGS = {0.5: 1.5, 1.0: 1.0, 2.0: 3.0}  # p -> c
MAX_MEMBERS = MAX_RUN = 64
PMAX, ITEMS_TOTAL, STAGE_ELEMS, TGT_ELEMS = 64, 2048, 6144, 512
MEMBER_AXES, RUN_AXES, NONFINITE = GC.MEMBER_AXES, GC.NORM_AXES, GC.NONFINITE
arrange, check, unit = GC.arrange, GC.check, GC.unit


def tile_points(l: int) -> int:
  npair = l * (l - 1) // 2
  return max(1, min(PMAX, ITEMS_TOTAL // npair if npair else PMAX, TGT_ELEMS // l))


def member_chunk(m: int, l: int) -> int:
  return min(m, STAGE_ELEMS // (tile_points(l) * l))


def variogram_points(p, t, power, dtype=None):
  """p[M, frame..., L], t[frame..., L] -> (VS[frame...], bound[frame...]) in float64; the bound (for a launch in `dtype`, the
  inputs' by default) is meaningless where VS is NaN."""
  u = unit(p.dtype if dtype is None else dtype)
  c = ROUNDINGS[float(power)]
  x = np.asarray(p).astype(np.float64)
  y = np.asarray(t).astype(np.float64)
  m, l = x.shape[0], x.shape[-1]
  total = np.zeros(y.shape[:-1])
  err = np.zeros(y.shape[:-1])
  with np.errstate(all='ignore'):
    for i in range(l - 1):  # the pairs (i, j > i)
      ty = np.abs(y[..., i + 1:] - y[..., i:i + 1]) ** power
      tx = (np.abs(x[..., i + 1:] - x[..., i:i + 1]) ** power).sum(axis=0) / m
      e = ty - tx
      delta = c * u * (ty + tx) + (m + 2) * 2.0 ** -53 * tx + 2.0 ** -53 * (ty + tx)
      total = total + (e * e).sum(axis=-1)
      err = err + (2.0 * np.abs(e) * delta + delta * delta).sum(axis=-1)
    vs = 2.0 * total
    bound = 2.0 * err + (l * l + 4) * 2.0 ** -53 * vs
  finite = np.isfinite(x).all(axis=(0, -1)) & np.isfinite(y).all(axis=-1)
  return np.where(finite, vs, np.nan), np.where(finite, bound, 0.0)


def expected(p, t, power, valid, flags, depth_chunk, x_kept):
  """-> (want[lead][chunk][lane][j], bound of the same shape (0 on count lanes; meaningless where want is NaN), stat[lead, row, x])."""
  stat, pbound = variogram_points(p, t, power)
  mode = flags & (FLAG_MASKED | FLAG_SKIPNA)
  want = expected_partials(stat[..., None], valid, mode, depth_chunk, x_kept)
  mag = np.where(np.isfinite(stat), np.abs(stat), 0.0)[..., None]
  summed = expected_partials(mag, valid, mode, depth_chunk, x_kept)[:, :, :NLANE]
  own = expected_partials(pbound[..., None], valid, mode, depth_chunk, x_kept)[:, :, :NLANE]
  n = min(depth_chunk, stat.shape[1]) * (1 if x_kept else stat.shape[2])
  bound = np.zeros(want.shape)
  bound[:, :, :NLANE] = own + (n + 2) * 2.0 ** -53 * summed
  return want, bound, stat


def variogram_case(seed, m, l, nlead, nrow, nx, dtype, flags, depth_chunk, x_kept, power):
  """-> p[M, lead, row, x, l], t[lead, row, x, l] (C order), mask[row, x], want, bound, stat (`expected` of them).

  The values and the placing of the non-finite points are energy_cases.energy_case's: under skipna anywhere; otherwise into at most
  min(3, npartial // 5) distinct partials (one point each); under a mask three more under masked-out points, where they must leave
  no trace.  (One member: the case of two, its first member.)  Asserted here, on the restatement's output: without skipna at
  least 80 % of the expected partials are finite; under skipna some point is NaN and no partial is."""
  p, t, mask = GC.energy_case(seed, max(m, 2), l, nlead, nrow, nx, dtype, flags, depth_chunk, x_kept)
  p = np.ascontiguousarray(p[:m])
  want, bound, stat = expected(p, t, power, mask, flags, depth_chunk, x_kept)
  assert not np.isinf(stat).any()
  if flags & FLAG_SKIPNA:
    assert np.isnan(stat).any() and not np.isnan(want).any(), (seed, m, l)
  else:
    share = float(np.isfinite(want[:, :, 0]).mean())
    assert share >= 0.8, (seed, m, l, nx, 'finite share of the partials', share)
  return p, t, mask, want, bound, stat
