"""Inputs and the float64 restatement for the thresholded contingency tables (wbx_contingency_partial), plain NumPy.

Restatement (include/wbx.h): per point and threshold k, P = float64(p) > thr_k, O = float64(t) > thr_k (strict; a NaN threshold
compares false), the four cells TP / FP / FN / TN as 0 / 1 in lane cell * K + k, NaN in all 4 * K lanes where p or t is NaN.
Every partial is then a sum of 0 / 1 of fewer than 2^53 terms: tests compare bit for bit.

Inputs sit on a dyadic grid (multiples of 1/8: ties with the thresholds are real ties) with the edges sprinkled in: values equal
to a threshold, float32(0.1) and its lower neighbour against the threshold 0.1, +-inf and -0.0 against 0.0."""
import numpy as np

FLAG_MASKED, FLAG_SKIPNA = 1, 2
CELLS = 4
F32_TENTH = np.float32(0.1)  # > 0.1 in float64: exceeds the threshold 0.1; its lower neighbour does not
F32_BELOW_TENTH = np.nextafter(F32_TENTH, np.float32(-np.inf))

# unsorted, a duplicate (0.25), ties with the grid (0.25, -0.25, 1.0, 0.5, 0.125, 0.0), NaN (every good point is TN), +inf (never
# exceeded), -inf (exceeded by all but -inf), +-1e40 (beyond the float32 range), -0.0 (the same threshold as 0.0)
THR16 = np.array([0.25, -0.25, np.nan, 1.0, np.inf, 0.1, 0.0, 0.25, -1.5, 1.75, -np.inf, 1e40, -1e40, 0.5, -0.0, 0.125])
THR3 = np.array([0.1, 0.0, 0.1])  # unsorted, a duplicate
THR1 = np.array([0.0])


def thresholds(nthr: int) -> np.ndarray:
  if nthr == 1:
    return THR1.copy()
  if nthr == 3:
    return THR3.copy()
  reps = -(-nthr // THR16.size)
  return np.tile(THR16, reps)[:nthr].copy()


def contingency_stat(p: np.ndarray, t: np.ndarray, thr: np.ndarray) -> np.ndarray:
  """p, t broadcastable to one frame -> stat[frame..., 4 * K] float64, lane cell * K + k, NaN where p or t is NaN."""
  p, t = np.broadcast_arrays(np.asarray(p), np.asarray(t))
  thr = np.asarray(thr, np.float64)
  with np.errstate(invalid='ignore'):
    P = p.astype(np.float64)[..., None] > thr
    O = t.astype(np.float64)[..., None] > thr
  cells = [P & O, P & ~O, ~P & O, ~P & ~O]
  stat = np.concatenate([c.astype(np.float64) for c in cells], axis=-1)
  stat[np.isnan(p) | np.isnan(t)] = np.nan
  return stat


def expected_partials(stat, valid, flags, depth_chunk, x_kept):
  """stat[lead, row, x, lane] (NaN where the statistic is NaN), valid[row, x] or None -> what stage 1 writes,
  [lead][chunk][lane][j]: the value lanes, then the count lanes (one shared under a mask alone, one per lane under skipna)."""
  ok = np.ones(stat.shape, bool) if valid is None or not (flags & FLAG_MASKED) else np.broadcast_to(valid[None, :, :, None], stat.shape)
  if flags & FLAG_SKIPNA:
    ok = ok & ~np.isnan(stat)
    lanes = np.concatenate([np.where(ok, stat, 0.0), ok.astype(np.float64)], axis=-1)
  elif flags & FLAG_MASKED:
    lanes = np.concatenate([np.where(ok, stat, 0.0), ok[..., :1].astype(np.float64)], axis=-1)
  else:
    lanes = stat
  nlead, nrow, nx, nl = lanes.shape
  nchunk = -(-nrow // depth_chunk)
  a = np.pad(lanes, ((0, 0), (0, nchunk * depth_chunk - nrow), (0, 0), (0, 0))).reshape(nlead, nchunk, depth_chunk, nx, nl)
  out = a.sum(axis=2) if x_kept else a.sum(axis=(2, 3))[:, :, None, :]  # [lead, chunk, j, lane]
  return np.ascontiguousarray(np.moveaxis(out, -1, 2))


def contingency_case(seed, nlead, nrow, nx, dtype, flags, depth_chunk, x_kept, transposed=False):
  """-> p[lead, row, x], t[lead, row, x] (`transposed`: views of arrays stored [lead][x][row], x stride = nrow), mask[row, x].

  NaNs (p only, t only, both): under skipna anywhere; otherwise a NaN under a valid point poisons its whole partial, so such
  NaNs go into at most 20 % of the partials (one point each, none where that share is less than one partial); under a mask three
  more sit under masked-out points, where they must leave no trace."""
  rng = np.random.default_rng(seed)
  shape = (nlead, nrow, nx)
  n = int(np.prod(shape))
  p = (rng.integers(-16, 17, size=shape) / 8.0).astype(dtype)
  t = (rng.integers(-16, 17, size=shape) / 8.0).astype(dtype)
  edges = [F32_TENTH, F32_BELOW_TENTH, 0.25, np.inf, -np.inf, -0.0, 0.0, 1.0, -0.25]
  if np.dtype(dtype) == np.float64:
    edges += [0.1, np.nextafter(0.1, np.inf), np.nextafter(0.1, -np.inf)]
  for arr in (p, t):
    flat = arr.reshape(-1)
    for v in edges:
      flat[rng.integers(0, n, size=max(1, n // 40))] = v
  mask = rng.random((nrow, nx)) > 0.3
  nan_kinds = [(True, False), (False, True), (True, True)]  # (p, t)

  def put_nan(lead, row, x, kind):
    if kind[0]:
      p[lead, row, x] = np.nan
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
    # distinct partials: (lead, chunk[, x]) drawn without replacement
    picks = rng.choice(npartial, size=allowed, replace=False) if allowed else []
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
        # (the other leads' points at (row, x) are hidden as well, whatever they hold)
  if transposed:
    p = np.ascontiguousarray(np.swapaxes(p, 1, 2)).swapaxes(1, 2)
    t = np.ascontiguousarray(np.swapaxes(t, 1, 2)).swapaxes(1, 2)
  return p, t, mask
