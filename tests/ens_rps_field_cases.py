"""Inputs and the integer restatement for the ranked probability score of an ensemble at threshold FIELDS
(wbx_ens_rps_field_partial), plain NumPy.

Restatement (include/wbx.h): the one of ens_rps_cases with the thresholds a[frame..., K], b[frame..., K] read at the point -- its
`numerators` broadcasts them as they are -- compared as NumPy's promoted comparison compares (everything widened to float64, which is
exact for float32), and a point is NaN where a member, the target or any of its K prediction or target thresholds is NaN.

A threshold field is stored once (`FieldCase.root`) and addressed through element strides: a leading `side` axis (1: both sides
read the same thresholds, t_off = 0; 2: the target's thresholds follow the prediction's, t_off = that axis' stride), the bin axis
outermost [side, K, day, row, x] or innermost [side, day, row, x, K], NDAY = 3 days of which the two leads gather DAYS = (2, 0), and
axes the field does not vary along stored with one element and addressed with stride 0.

Data sits on the dyadic grid of ens_rps_case; the threshold fields sit on the same grid, so ties are real ties, with the edges
sprinkled in: 0.1 in the field's type (against float32(0.1) and both neighbours in float32 data, 0.1 and both neighbours in float64
data), +-inf, +-1e40 (float64 fields: beyond the float32 range), -0.0.  NaNs come in six kinds -- one member, the target, both, a
prediction threshold, a target threshold, both -- placed so that without skipna at most 20 % of the partials hold a NaN point of any
kind (a NaN under a valid point poisons its whole partial); under a mask three more NaN thresholds sit under masked-out points,
where they must leave no trace; day 1, which no lead gathers, holds NaN thresholds throughout where the field varies by day."""
import dataclasses

import numpy as np

import ens_rps_cases as EC

FLAG_MASKED, FLAG_SKIPNA, FLAG_FAIR = EC.FLAG_MASKED, EC.FLAG_SKIPNA, EC.FLAG_FAIR
NDAY = 3
DAYS = (2, 0)  # the day of the source each lead gathers
VARIES = ('all', 'x', 'none')  # the field varies over (day, row, x) / over x only / not at all


def numerators(p, t, a, b, fair, right):
  """p[M, frame...], t[frame...], a / b[frame..., K] -> sum_k n_k per point as int64."""
  return EC.numerators(p, t, np.asarray(a, np.float64), np.asarray(b, np.float64), fair, right)


def nan_points(p, t, a, b):
  return EC.nan_points(p, t) | np.isnan(np.asarray(a)).any(axis=-1) | np.isnan(np.asarray(b)).any(axis=-1)


def expected(p, t, a, b, fair, right, valid, flags, depth_chunk, x_kept):
  """-> (what stage 1 writes, [lead][chunk][lane][j], as ens_rps_cases.expected; the statistic of every point, NaN where it is NaN)."""
  stat = numerators(p, t, a, b, fair, right).astype(np.float64)
  stat[nan_points(p, t, a, b)] = np.nan
  want = EC.expected_partials(stat[..., None], valid, flags & (FLAG_MASKED | FLAG_SKIPNA), depth_chunk, x_kept)
  want[:, :, 0] = want[:, :, 0] / EC.denominator(np.asarray(p).shape[0], fair)
  return want, stat


@dataclasses.dataclass
class FieldCase:
  p: np.ndarray       # [M, lead, row, x]
  t: np.ndarray       # [lead, row, x]
  mask: np.ndarray    # [row, x]
  root: np.ndarray    # the stored thresholds, C-contiguous
  view: np.ndarray    # root as [side, K stored, day, row, x] (one element along what the field does not vary over)
  nthr: int           # thresholds the score uses: the first nthr of the stored ones
  varies: str
  bin_innermost: bool

  def _stride(self, axis):
    return 0 if self.view.shape[axis] == 1 else self.view.strides[axis] // self.view.itemsize

  @property
  def t_off(self):
    return self._stride(0)

  @property
  def thr_stride(self):
    return self.view.strides[1] // self.view.itemsize  # (not 0 for one stored threshold: the ABI refuses 0 only for nthr > 1)

  @property
  def day_stride(self):
    return self._stride(2)

  @property
  def row_stride(self):
    return self._stride(3)

  @property
  def x_stride(self):
    return self._stride(4)

  def selected(self, side, days=DAYS, nthr=None):
    """The thresholds every point of the frame reads on `side` (0: prediction, 1: target): [lead, row, x, K] in the field's type."""
    nlead, nrow, nx = self.t.shape
    v = self.view[min(side, self.view.shape[0] - 1), :self.nthr if nthr is None else nthr]
    v = v[:, [d if v.shape[1] > 1 else 0 for d in days]]  # [K, lead, row?, x?]
    return np.ascontiguousarray(np.moveaxis(np.broadcast_to(v, (v.shape[0], nlead, nrow, nx)), 0, -1))


def field_case(seed, m, nthr, nlead, nrow, nx, dtype, thr_dtype, flags, depth_chunk, x_kept, varies='all', bin_innermost=False,
               stacked=False, member_innermost=False, extra_bins=0):
  """-> FieldCase.  `extra_bins`: thresholds stored behind the nthr-th that the score must not read into its sums."""
  assert nlead == len(DAYS) and varies in VARIES
  rng = np.random.default_rng(seed)
  p, t, mask = EC.ens_rps_case(seed, m, nlead, nrow, nx, dtype, 0, depth_chunk, x_kept, np.array([0.1, 0.0, 0.25, -0.5, 1.0]))
  p[np.isnan(p)], t[np.isnan(t)] = 0.375, -0.625  # (the NaNs are placed below, together with the thresholds')
  nside, kst = (2 if stacked else 1), nthr + extra_bins
  logical = (nside, kst) + {'all': (NDAY, nrow, nx), 'x': (1, 1, nx), 'none': (1, 1, 1)}[varies]
  vals = (rng.integers(-16, 17, size=logical) / 8.0).astype(thr_dtype)
  flat = vals.reshape(-1)
  edges = [0.1, np.inf, -np.inf, -0.0, 0.0, 0.25, -0.5, 1.0] + ([1e40, -1e40] if np.dtype(thr_dtype) == np.float64 else [])
  for v in edges:
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 24))] = v
  if bin_innermost:  # stored [side, day, row, x, K]
    root = np.ascontiguousarray(np.moveaxis(vals, 1, -1))
    view = np.moveaxis(root, -1, 1)
  else:
    root = np.ascontiguousarray(vals)
    view = root
  case = FieldCase(p, t, mask, root, view, nthr, varies, bin_innermost)
  if varies == 'all':
    view[:, :, 1] = np.nan  # the day no lead gathers
  nchunk = -(-nrow // depth_chunk)
  npartial = nlead * nchunk * (nx if x_kept else 1)

  def partials_of(lead, row, x, kind):
    """The partials a NaN of `kind` at the point poisons: a threshold NaN reaches every point that reads that element."""
    leads = [lead] if kind < 3 or varies == 'all' else range(nlead)
    rows = [row] if kind < 3 or varies == 'all' else range(nrow)
    return {(l, r // depth_chunk, x if x_kept else 0) for l in leads for r in rows}

  def put_nan(lead, row, x, kind):
    """kind 0..5: one member, the target, both, a prediction threshold, a target threshold, one of each."""
    if kind in (0, 2):
      p[int(rng.integers(0, m)), lead, row, x] = np.nan
    if kind in (1, 2):
      t[lead, row, x] = np.nan
    at = (DAYS[lead], row, x) if varies == 'all' else (0, 0, x)
    if kind in (3, 5):
      view[(0, int(rng.integers(0, nthr))) + at] = np.nan
    if kind in (4, 5):
      view[(nside - 1, int(rng.integers(0, nthr))) + at] = np.nan  # (one field for both sides: the target reads it too)

  kinds = list(range(6)) if varies != 'none' else [0, 1, 2]  # a NaN in a field that does not vary makes every point NaN
  if flags & FLAG_SKIPNA:
    n = nlead * nrow * nx
    ncolumn = 0
    for i in range(max(6, n // 25)):
      lead, row, x = (int(rng.integers(0, s)) for s in (nlead, nrow, nx))
      kind = kinds[i % len(kinds)]
      if kind >= 3 and varies == 'x':
        ncolumn += 1
        if ncolumn > 2:
          kind -= 3  # (a column of the field is a whole column of NaN points: two of them at most)
      put_nan(lead, row, x, kind)
      if i < 6:
        mask[row, x] = True
  else:
    poisoned, taken = set(), set()
    for i in range(12):
      lead, row, x = (int(rng.integers(0, s)) for s in (nlead, nrow, nx))
      kind = kinds[(seed + i) % len(kinds)]
      hit = partials_of(lead, row, x, kind)
      if 5 * len(poisoned | hit) > npartial:
        continue
      poisoned |= hit
      put_nan(lead, row, x, kind)
      if kind >= 3 and varies == 'x':
        mask[:, x] = True
        taken |= {(r, x) for r in range(nrow)}
      else:
        mask[row, x] = True  # a NaN under a VALID point
        taken.add((row, x))
    if flags & FLAG_MASKED and varies != 'none':  # NaN thresholds the mask hides (the mask has no lead axis)
      free = sorted({x for x in range(nx)} - {x for _, x in taken}) if varies == 'x' else \
          [(r, x) for r in range(nrow) for x in range(nx) if (r, x) not in taken]
      for i in range(min(3, len(free))):
        pick = free[int(rng.integers(0, len(free)))]
        if varies == 'x':
          mask[:, pick] = False
          put_nan(0, 0, pick, 3 + i % 3)
        else:
          mask[pick] = False
          put_nan(int(rng.integers(0, nlead)), pick[0], pick[1], 3 + i % 3)
  if member_innermost:
    case.p = np.moveaxis(np.ascontiguousarray(np.moveaxis(p, 0, -1)), -1, 0)
  return case


def round_to_float32(v, right):
  """float64 thresholds as the kernel compares them with float32 data: rounded toward -inf for <=, toward +inf for < (NaN stays)."""
  v = np.asarray(v, np.float64)
  with np.errstate(over='ignore', invalid='ignore'):
    f = v.astype(np.float32)
    wrong = (f.astype(np.float64) > v) if right else (f.astype(np.float64) < v)
    return np.where(wrong, np.nextafter(f, np.float32(-np.inf if right else np.inf)), f)
