"""The FSS terms of THRESHOLDED continuous fields restated in NumPy (include/wbx.h: wbx_fss_threshold_partial), the case lists that
tests/test_fss_thresholds.py, tests/test_gpu_fss_thresholds.py and tests/test_gpu_fss_thresholds_api.py share.

The restatement is tests/fss_cases.py applied to the binarised fields: for threshold a_k the float32 field (float64(x) > a_k) with NaN
kept -- `(x > thr).where(~isnan)` as float32, what wrappers.binarize_thresholds hands the statistic -- goes through
fss_cases.point_values and fss_cases.partials, and the lanes of threshold k land at 3 k + l, the count lanes behind all value lanes
(none; one shared; one per value lane at 3 K + 3 k + l).  Window sums of 0 / 1 fields are exact in any order, so the restated point
values ARE the kernel's; only the float64 sums over x and depth round.

`mutant` restates it wrongly in one of four ways, each of which a case here must see (tests/test_fss_thresholds.py):
  'ge'          >= instead of >                         -- seen by points exactly equal to a threshold
  'nearest'     the threshold rounded to nearest into the input type, compared there -- seen by float32(0.1) under the threshold 0.1
  'nan_zero'    NaN counted as "not exceeded" (0)       -- seen by the NaN share
  'shared_nan'  one NaN count for both inputs           -- seen wherever only one of p, t has a NaN in a window
"""
import numpy as np

import fss_cases as FC

KB = 2  # thresholds one launch of the entry carries (csrc/wbx_fss_thresholds.hip: FSS_KB)
THR_MAX = 16
NAN_INF = 5  # the list that holds a NaN and an infinite threshold
SHAPES, WIDE, sizes_for, LANES = FC.SHAPES, FC.WIDE, FC.sizes_for, FC.LANES

# K = 1, KB, KB + 1 and 16, a list with a NaN and an infinite threshold (an odd number: the last launch of its call carries one), and
# K = 7; 0.1 is no float32, 0.5 and 0.25 are
THRESHOLD_LISTS = {
    1: [0.5],
    KB: [0.25, 0.1],
    KB + 1: [0.75, 0.1, 0.5],
    NAN_INF: [0.1, float('nan'), 0.5, float('inf'), -0.25],
    7: [0.9, 0.1, 0.5, 0.3, 0.7, 0.2, 0.6],
    THR_MAX: [0.1, 0.5] + [round(0.05 + 0.06 * i, 3) for i in range(THR_MAX - 3)] + [float('-inf')],
}
assert all(len(v) == k for k, v in THRESHOLD_LISTS.items())


def continuous_fields(shape, dtype, seed, thresholds, nan_share=0.06):
  """Smooth blobs plus noise in about [-0.3, 1.3]; points exactly equal to every finite threshold (as the input type holds it: for
  float32 inputs and the threshold 0.1 that is float32(0.1), which exceeds 0.1), `nan_share` NaN and a few +-inf."""
  rng = np.random.default_rng(seed)
  nlat, nlon = shape[-2:]
  y, x = np.arange(nlat)[:, None] / max(nlat, 1), np.arange(nlon)[None, :] / max(nlon, 1)
  lead = shape[:-2]
  phase = rng.random(lead + (1, 1)) * 6.28
  blobs = 0.5 + 0.35 * np.sin(6.28 * (2 * x + y) + phase) * np.cos(6.28 * (x - 1.5 * y) - phase)
  out = []
  for shift in (0.0, 0.07):
    f = (blobs + shift + 0.2 * rng.normal(size=shape)).astype(dtype)
    flat = f.reshape(-1)
    finite = [v for v in thresholds if np.isfinite(v)]
    for v in finite:  # ties: about 3 % of the points per threshold
      flat[rng.random(flat.size) < 0.03] = dtype(v)
    flat[rng.random(flat.size) < nan_share] = np.nan
    flat[rng.random(flat.size) < 0.004] = np.inf
    flat[rng.random(flat.size) < 0.004] = -np.inf
    out.append(f)
  return out[0], out[1]


def binarized(x, thr, mutant=None):
  """float32 (x > thr) with NaN kept, the comparison in float64."""
  x = np.asarray(x)
  with np.errstate(invalid='ignore'):
    if mutant == 'ge':
      over = x.astype(np.float64) >= np.float64(thr)
    elif mutant == 'nearest':
      over = x > x.dtype.type(thr)
    else:
      over = x.astype(np.float64) > np.float64(thr)
  b = over.astype(np.float32)
  if mutant != 'nan_zero':
    b[np.isnan(x)] = np.nan
  return b


def binarized_pair(p, t, thr, mutant=None):
  pb, tb = binarized(p, thr, mutant), binarized(t, thr, mutant)
  if mutant == 'shared_nan':
    either = np.isnan(pb) | np.isnan(tb)
    pb, tb = np.where(either, np.float32(np.nan), pb), np.where(either, np.float32(np.nan), tb)
  return pb, tb


def point_values(p, t, thresholds, n, wrap, mutant=None):
  """float64 [K, 3, ...]: the three lanes of every point and threshold."""
  return np.stack([FC.point_values(*binarized_pair(p, t, thr, mutant), n, wrap) for thr in thresholds])


def lanes_total(flags, nthr):
  nv = LANES * nthr
  return 2 * nv if flags & 2 else (nv + 1 if flags & 1 else nv)


def partials(values, mask, flags, depth_chunk, x_kept):
  """values [K, 3, key, depth, lat, lon] -> (want, mag, nterm): want[key][lat][chunk][lanes_total][nj] in the entry's lane order, mag
  and nterm per VALUE lane (3 k + l) as fss_cases.partials gives them."""
  nthr = values.shape[0]
  nv = LANES * nthr
  want = mag = nterm = None
  for k in range(nthr):
    w, m, nt = FC.partials(values[k], mask, flags, depth_chunk, x_kept)
    if want is None:
      want = np.zeros(w.shape[:3] + (lanes_total(flags, nthr),) + w.shape[4:])
      mag = np.zeros(w.shape[:3] + (nv,) + w.shape[4:])
      nterm = np.zeros_like(mag)
    want[:, :, :, LANES * k:LANES * (k + 1)] = w[:, :, :, :LANES]
    mag[:, :, :, LANES * k:LANES * (k + 1)] = m
    nterm[:, :, :, LANES * k:LANES * (k + 1)] = nt
    if flags & 2:
      want[:, :, :, nv + LANES * k:nv + LANES * (k + 1)] = w[:, :, :, LANES:]
    elif flags & 1:
      want[:, :, :, nv] = w[:, :, :, LANES]  # one shared lane: the same for every threshold
  return want, mag, nterm


def slice_of(got, flags, nthr, k):
  """The lanes of threshold k of a partial of the entry as wbx_fss_partial lays them out: [..., lanes_total(flags), nj]."""
  nv = LANES * nthr
  parts = [got[:, :, :, LANES * k:LANES * (k + 1)]]
  if flags & 2:
    parts.append(got[:, :, :, nv + LANES * k:nv + LANES * (k + 1)])
  elif flags & 1:
    parts.append(got[:, :, :, nv:nv + 1])
  return np.concatenate(parts, axis=3)
