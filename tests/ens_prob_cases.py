"""Inputs and the integer restatement for the contingency tables of ensemble event probabilities
(wbx_ens_prob_contingency_partial), plain NumPy.

Restatement (include/wbx.h): per point with members x_m, target y and event thresholds a_k
    c_k = #{m : float64(x_m) > a_k} in 0..M,   o_k = [float64(y) > a_k]      (strict; a NaN threshold compares false)
    P_kj = lo_j <= c_k <= hi_j                                              (slot j as a run of member counts; lo > hi: empty)
the four cells TP / FP / FN / TN as 0 / 1 in lane cell * (K * J) + k * J + j, NaN in all 4 * K * J lanes where a member or the
target is NaN.  Every partial is then a sum of 0 / 1 of fewer than 2^53 terms: tests compare bit for bit.

The slot table restated: the member mean of M float32 indicators with c ones is fl32(c / M) (the sum is exact), and
    ContinuousToBinary(tau):   slot j holds c  <=>  float64(fl32(c / M)) > tau_j                (false for a NaN tau)
    ContinuousToBins(edges):   slot j holds c  <=>  [p <= e_{j+1}] != [p <= e_j], p = float64(fl32(c / M))
                               (for increasing edges: e_j < p <= e_{j+1})
and a slot is the run (min c, max c) of the counts it holds, (1, 0) where it holds none, None where they are not one run.

Inputs are those of tests/ens_rps_cases.py: a dyadic grid with the edges sprinkled in (values equal to a threshold, float32(0.1)
and both neighbours against the threshold 0.1, +-inf, +-0.0, all members -inf / +inf), NaNs placed so that at least three quarters
of the partials of a plain or masked case stay finite."""
import numpy as np

from contingency_cases import THR16, expected_partials
from ens_rps_cases import ens_rps_case

FLAG_MASKED, FLAG_SKIPNA = 1, 2
CELLS = 4

# event thresholds by K: 0.0 against -0.0; unsorted with a NaN (every good point: c = 0, o = 0) and 0.1, which float32 cannot hold;
# ties with the grid; THR16: a duplicate, NaN, +-inf, +-1e40 (beyond the float32 range), -0.0 (the same threshold as 0.0)
EVENT_THRESHOLDS = {
    1: np.array([0.0]),
    3: np.array([0.1, np.nan, 0.0]),
    4: np.array([0.25, -0.25, 0.1, 0.0]),
    16: THR16,
}


def event_thresholds(nthr: int) -> np.ndarray:
  return EVENT_THRESHOLDS[nthr].copy()


def slot_runs(nslot: int, m: int) -> np.ndarray:
  """int32 [nslot, 2] of (lo, hi) runs for M = m members, the same shapes at every M: every count, an empty slot (lo > hi), c = 0
  alone, c = M alone, runs that reach beyond 0..M on either side, an upper set (what a probability threshold gives), inner runs."""
  h = m // 2
  every = [(0, m), (1, 0), (0, 0), (m, m), (-5, h), (h + 1, m + 7), (1, m), (h, h), (m + 1, m + 3), (-3, -1),
           (min(1, m), max(m - 1, 0)), (0, h), (h, m), (2, 1), (m // 3, 2 * m // 3), (m - m // 4, m)]
  pick = {1: [4], 4: [0, 1, 4, 5], 5: [6, 1, 2, 3, 7], 16: list(range(16))}[nslot]
  return np.array([every[i] for i in pick], np.int32).reshape(nslot, 2)


def counts(p, thr):
  """p[M, frame...] -> c[frame..., K] int64: members over every event threshold, compared in float64."""
  x = np.asarray(p).astype(np.float64)[..., None]
  with np.errstate(invalid='ignore'):
    return (x > np.asarray(thr, np.float64)).sum(axis=0).astype(np.int64)


def observed(t, thr):
  """t[frame...] -> o[frame..., K] bool."""
  with np.errstate(invalid='ignore'):
    return np.asarray(t).astype(np.float64)[..., None] > np.asarray(thr, np.float64)


def nan_points(p, t):
  return np.isnan(np.asarray(p)).any(axis=0) | np.isnan(np.asarray(t))


def member_fraction(m: int) -> np.ndarray:
  """fl32(c / M) for c = 0..M as float64: the member mean of float32 indicators with c ones."""
  return (np.arange(m + 1, dtype=np.float32) / np.float32(m)).astype(np.float64)


def hits_thresholds(m: int, tau) -> np.ndarray:
  """hit[c, j]: c members over the event threshold exceed probability threshold tau_j."""
  with np.errstate(invalid='ignore'):
    return member_fraction(m)[:, None] > np.asarray(tau, np.float64)[None, :]


def hits_bins(m: int, edges) -> np.ndarray:
  """hit[c, j]: c members over the event threshold fall into bin j of the len(edges) - 1 bins."""
  e = np.asarray(edges, np.float64)
  below = member_fraction(m)[:, None] <= e[None, :]
  return below[:, 1:] != below[:, :-1]


def runs_of(hit):
  """hit[c, j] -> int32 [J, 2] of (lo, hi), (1, 0) for a slot that holds no count; None where a slot is not one run."""
  out = np.empty((hit.shape[1], 2), np.int32)
  for j in range(hit.shape[1]):
    c = np.flatnonzero(hit[:, j])
    if c.size == 0:
      out[j] = (1, 0)
    elif c[-1] - c[0] + 1 != c.size:
      return None
    else:
      out[j] = (c[0], c[-1])
  return out


def cells(p, t, thr, slots):
  """p[M, frame...], t[frame...] -> stat[frame..., 4 * K * J] float64, lane cell * (K * J) + k * J + j, NaN where a member or the
  target is NaN."""
  slots = np.asarray(slots, np.int64).reshape(-1, 2)
  c = counts(p, thr)[..., None]  # [frame, K, 1]
  P = (slots[:, 0] <= c) & (c <= slots[:, 1])  # [frame, K, J]
  O = np.broadcast_to(observed(t, thr)[..., None], P.shape)
  flat = lambda a: a.reshape(a.shape[:-2] + (-1,))
  stat = np.concatenate([flat(x).astype(np.float64) for x in (P & O, P & ~O, ~P & O, ~P & ~O)], axis=-1)
  stat[nan_points(p, t)] = np.nan
  return stat


def expected(p, t, thr, slots, valid, flags, depth_chunk, x_kept):
  """-> what stage 1 writes for p[M, lead, row, x], t[lead, row, x], valid[row, x]: [lead][chunk][lane][j], the value lanes, then the
  count lanes (one shared under a mask alone, one per value lane under skipna)."""
  return expected_partials(cells(p, t, thr, slots), valid, flags & (FLAG_MASKED | FLAG_SKIPNA), depth_chunk, x_kept)


def ens_prob_case(seed, m, nlead, nrow, nx, dtype, flags, depth_chunk, x_kept, thr, member_innermost=False):
  """-> p[M, lead, row, x], t[lead, row, x], mask[row, x] (tests/ens_rps_cases.ens_rps_case: NaN points under skipna anywhere;
  otherwise in at most a fifth of the partials, and under a mask three more beneath mask = 0, where they must leave no trace)."""
  return ens_rps_case(seed, m, nlead, nrow, nx, dtype, flags, depth_chunk, x_kept, thr, member_innermost=member_innermost)
