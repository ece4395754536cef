"""Inputs and the integer restatement for the Brier-type errors of event probabilities (wbx_ens_brier_partial), plain NumPy.

Restatement (include/wbx.h): per point with members x_m (m < M), target y, thresholds a_k and the denominator D (M: the member
mean; M + 1: Weibull's plotting position; 1 for a deterministic pair, M = 1)
    c_k = #{m : float64(x_m) > a_k},  o_k = [float64(y) > a_k],  e_k = c_k - o_k D                  (integers)
    Error = e_k / D,  AbsoluteError = |e_k| / D,  SquaredError = e_k^2 / D^2,  NaN where a member or the target is NaN.
A stage-1 partial is float64(S) / float64(D) (float64(D * D) for the squared error) with S the integer sum of the numerators over
its points: tests compare bit for bit.  The numerators are held as int64 and summed as integers (|e_k^2| <= 257^2, a test's partial
has fewer than 2^20 points: nowhere near 2^53); value lane stat * K + k, stat in (Error, AbsoluteError, SquaredError).

Inputs are those of tests/ens_rps_cases.py: a dyadic grid (multiples of 1/8: ties with the thresholds are real ties) with the edges
sprinkled in -- values equal to a threshold, float32(0.1) and both neighbours against the threshold 0.1, +-inf, +-0.0, points whose
members are all -inf and points whose members are all +inf -- and NaNs placed by mode."""
import numpy as np

from ens_rps_cases import ens_rps_case, nan_points  # pylint: disable=unused-import

FLAG_MASKED, FLAG_SKIPNA = 1, 2
ERR, ABS, SQ = 0, 1, 2
STATS = 3

# +-inf, +-1e40 (beyond the float32 range), 0.1 (no float32), 0.0 and -0.0 (one threshold), a NaN (never exceeded), a duplicate
# (0.25), unsorted, ties with the grid
_A16 = np.array([0.25, -0.25, 1.0, np.inf, 0.1, 0.0, 0.25, -1.5, 1.75, -np.inf, 1e40, -1e40, 0.5, -0.0, np.nan, -1.0])
THRESHOLDS = {
    1: np.array([0.0]),
    2: np.array([0.1, -0.0]),
    4: np.array([0.1, 0.0, 0.1, -1e40]),                    # unsorted, a duplicate, beyond the float32 range
    5: np.array([-1.0, np.nan, 0.1, 0.5, 1.0]),
    8: _A16[:8].copy(),
    9: _A16[7:].copy(),
    16: _A16,
}


def thresholds(nthr: int):
  return THRESHOLDS[nthr].copy()


def counts(p, a):
  """p[M, frame...] -> c[frame..., K] int64: members over every threshold, compared in float64 (a NaN on either side: not over)."""
  x = np.asarray(p).astype(np.float64)[..., None]
  with np.errstate(invalid='ignore'):
    return (x > np.asarray(a, np.float64)).sum(axis=0).astype(np.int64)


def observed(t, a):
  y = np.asarray(t).astype(np.float64)[..., None]
  with np.errstate(invalid='ignore'):
    return (y > np.asarray(a, np.float64)).astype(np.int64)


def numerators(p, t, a, denom):
  """p[M, frame...], t[frame...] -> int64 [frame..., 3 * K], lane stat * K + k: e_k, |e_k|, e_k^2 (meaningless where nan_points
  says NaN)."""
  e = counts(p, a) - observed(t, a) * int(denom)
  return np.concatenate([e, np.abs(e), e * e], axis=-1)


def points(p, t, a, denom):
  """The three statistics per point and threshold in float64 [frame..., 3 * K], NaN where a member or the target is NaN."""
  k = len(a)
  out = numerators(p, t, a, denom).astype(np.float64)
  out[..., :2 * k] /= np.float64(denom)
  out[..., 2 * k:] /= np.float64(denom * denom)
  out[nan_points(p, t)] = np.nan
  return out


def expected(p, t, a, denom, valid, flags, depth_chunk, x_kept):
  """p[M, lead, row, x], t[lead, row, x], valid[row, x] or None -> what stage 1 writes, [lead][chunk][lane][j]: the 3 K value lanes,
  then the count lanes (one shared under a mask alone, one per value lane under skipna)."""
  k = len(a)
  num = numerators(p, t, a, denom)                       # int64 [lead, row, x, 3 K]
  bad = nan_points(p, t)[..., None]
  ok = np.ones(num.shape, bool)
  if valid is not None and flags & FLAG_MASKED:
    ok = ok & np.asarray(valid, bool)[None, :, :, None]
  poison = ok & bad                                       # a NaN under a valid point
  good = ok & ~bad
  nlead, nrow, nx, nl = num.shape
  nchunk = -(-nrow // depth_chunk)

  def chunked(a4):  # [lead, row, x, lane] -> integer sums [lead, chunk, lane, j]
    pad = np.pad(a4, ((0, 0), (0, nchunk * depth_chunk - nrow), (0, 0), (0, 0))).reshape(nlead, nchunk, depth_chunk, nx, a4.shape[-1])
    s = pad.sum(axis=2) if x_kept else pad.sum(axis=(2, 3))[:, :, None, :]
    return np.moveaxis(s, -1, 2)
  s = chunked(np.where(good, num, 0))                     # int64: S
  div = np.concatenate([np.full(2 * k, np.float64(denom)), np.full(k, np.float64(denom * denom))])[None, None, :, None]
  values = s.astype(np.float64) / div                     # one correctly rounded quotient per partial
  if flags & FLAG_SKIPNA:
    return np.ascontiguousarray(np.concatenate([values, chunked(good.astype(np.int64)).astype(np.float64)], axis=2))
  values = np.where(chunked(poison.astype(np.int64)) > 0, np.nan, values)
  if flags & FLAG_MASKED:
    return np.ascontiguousarray(np.concatenate([values, chunked(ok[..., :1].astype(np.int64)).astype(np.float64)], axis=2))
  return np.ascontiguousarray(values)


def brier_case(seed, m, nlead, nrow, nx, dtype, flags, depth_chunk, x_kept, a, member_axis=0):
  """-> p[M, lead, row, x] (`member_axis`: where the member axis is STORED -- 0: outermost, [M][lead][row][x]; 1: in the middle,
  [lead][M][row][x]; 3: innermost, [lead][row][x][M], member stride 1 and x stride M -- p is a view with the members first
  whichever it is), t[lead, row, x], mask[row, x]; the NaNs as ens_rps_cases.ens_rps_case places them."""
  p, t, mask = ens_rps_case(seed, m, nlead, nrow, nx, dtype, flags, depth_chunk, x_kept, [v for v in np.asarray(a) if not np.isnan(v)])
  return member_view(p, member_axis), t, mask


def member_view(p, member_axis):
  if member_axis == 0:
    return np.ascontiguousarray(p)
  return np.moveaxis(np.ascontiguousarray(np.moveaxis(p, 0, member_axis)), member_axis, 0)
