"""Inputs and the float64 / integer restatement for the thresholded contingency tables at threshold FIELDS
(wbx_contingency_field_partial), plain NumPy.

Restatement (include/wbx.h): per point and threshold k, P = p > thr_k(point), O = t > thr_k(point) as NumPy's promoted comparison
decides (`np.result_type` of the data and the field, then `>`: strict; a NaN threshold compares false), the four cells TP / FP / FN /
TN as 0 / 1 in lane cell * K + k, NaN in all 4 * K lanes where p or t is NaN.  Every partial is a sum of 0 / 1: tests compare bit
for bit (tests/contingency_cases.py has the partials).

The frame is (lead, row, x).  Data sit on a dyadic grid (multiples of 1/8) with tests/contingency_cases.py's edges sprinkled in; the
field sits on the same grid -- ties with the data are real ties -- with NaN, +-inf, -0.0 and 0.0 sprinkled in, and for a float64 field
0.1 and the float64 just above float32(0.1): thresholds strictly between two neighbouring float32 values, one on either side of the
data value float32(0.1).  Fixed points (lead 1, x 0) make sure the edges meet: row 2 the rounding (p = float32(0.1), t its lower
neighbour, thresholds 0.1 in slot 0 and the one just above in the last slot), row 3 the tie (p = t = threshold = 0.25: strict `>`);
(lead 1, row 4, x nx - 1) is a good point under a NaN threshold.
NaN data are placed so that no test passes on all-NaN partials: p at (lead 0, row 0, x nx - 1), t at (lead 0, row 1, x nx - 1) -- one
depth chunk when depth_chunk = 2 --, and under a mask one NaN at the masked-out point (lead 0, row 4, x nx // 2)."""
import dataclasses

import numpy as np

import contingency_cases as CC

FLAG_MASKED, FLAG_SKIPNA = CC.FLAG_MASKED, CC.FLAG_SKIPNA
VARIES = ('row_x', 'x', 'row', 'lead_row_x')  # what the field varies over, beside its threshold axis
F64_ABOVE_F32_TENTH = np.nextafter(np.float64(CC.F32_TENTH), np.inf)  # between float32(0.1) and its upper neighbour


def promoted_gt(x: np.ndarray, thr: np.ndarray) -> np.ndarray:
  """x[frame] > thr[frame, K] as NumPy promotes the two dtypes -- literally: float32 against float32 in float32, else float64."""
  rt = np.result_type(x.dtype, thr.dtype)
  with np.errstate(invalid='ignore'):
    return x.astype(rt)[..., None] > thr.astype(rt)


def field_stat(p, t, thr, gt=promoted_gt, nan_thr_is_nan=False) -> np.ndarray:
  """p[frame], t[frame], thr[frame, K] -> stat[frame, 4 * K] float64, lane cell * K + k, NaN where p or t is NaN.  `gt` and
  `nan_thr_is_nan` are for the mutants of tests/test_contingency_field.py."""
  P, O = gt(p, thr), gt(t, thr)
  cells = [P & O, P & ~O, ~P & O, ~P & ~O]
  stat = np.concatenate([c.astype(np.float64) for c in cells], axis=-1)
  stat[np.isnan(p) | np.isnan(t)] = np.nan
  if nan_thr_is_nan:
    stat[np.tile(np.isnan(thr), CC.CELLS)] = np.nan
  return stat


@dataclasses.dataclass
class FieldCase:
  p: np.ndarray      # [lead, row, x]
  t: np.ndarray
  mask: np.ndarray   # [row, x] bool
  root: np.ndarray   # the field as it is stored (contiguous)
  strides: dict      # element strides of 'thr', 'lead', 'row', 'x' in `root` (0 where the field does not vary)
  size: int          # thresholds along the field's threshold axis

  def thresholds(self, first=0, nthr=None, ignore=()) -> np.ndarray:
    """[lead, row, x, nthr]: the thresholds of every point through the strides, `ignore`: strides a mutant leaves out."""
    nthr = self.size - first if nthr is None else nthr
    s = {k: (0 if k in ignore else v) for k, v in self.strides.items()}
    nlead, nrow, nx = self.p.shape
    at = (np.arange(nlead)[:, None, None, None] * s['lead'] + np.arange(nrow)[None, :, None, None] * s['row']
          + np.arange(nx)[None, None, :, None] * s['x'] + (first + np.arange(nthr))[None, None, None, :] * s['thr'])
    return self.root.reshape(-1)[at]


def expected(case: FieldCase, flags, depth_chunk, x_kept, first=0, nthr=None, **mutant):
  """[lead][chunk][lane][j] of a launch of thresholds first .. first + nthr - 1, and the per-point statistic."""
  ignore = mutant.pop('ignore', ())
  stat = field_stat(case.p, case.t, case.thresholds(first, nthr, ignore), **mutant)
  return CC.expected_partials(stat, case.mask, flags, depth_chunk, x_kept), stat


def field_case(seed, size, nlead, nrow, nx, dtype, thr_dtype, flags, varies='row_x', inner=False, pad=0, transposed=False) -> FieldCase:
  """`inner`: the threshold axis innermost (else outermost); `pad`: unused elements behind every row of the field (its row and
  threshold strides are then no multiples of 4); `transposed`: p, t stored [lead][x][row]."""
  assert varies in VARIES and nrow >= 5
  rng = np.random.default_rng(seed)
  shape = (nlead, nrow, nx)
  n = int(np.prod(shape))
  p = (rng.integers(-16, 17, size=shape) / 8.0).astype(dtype)
  t = (rng.integers(-16, 17, size=shape) / 8.0).astype(dtype)
  edges = [CC.F32_TENTH, CC.F32_BELOW_TENTH, 0.25, np.inf, -np.inf, -0.0, 0.0, 1.0, -0.25]
  for arr in (p, t):
    flat = arr.reshape(-1)
    for v in edges:
      flat[rng.integers(0, n, size=max(1, n // 40))] = v
  mask = rng.random((nrow, nx)) > 0.3
  # the field: [size, lead?, row?, x? (+ pad)], singleton where it does not vary
  fl, fr, fx = varies == 'lead_row_x', varies in ('row_x', 'row', 'lead_row_x'), varies in ('row_x', 'x', 'lead_row_x')
  fshape = (size, nlead if fl else 1, nrow if fr else 1, (nx + pad) if fx else 1)
  field = (rng.integers(-16, 17, size=fshape) / 8.0).astype(thr_dtype)
  fedges = [np.nan, np.inf, -np.inf, -0.0, 0.0, 0.25, CC.F32_TENTH]
  if np.dtype(thr_dtype) == np.float64:
    fedges += [0.1, F64_ABOVE_F32_TENTH, 1e40, -1e40]
  flat = field.reshape(-1)
  for v in fedges:
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 20))] = v
  # the fixed points, lead 1, x 0
  at = lambda lead, row: (lead if fl else 0, row if fr else 0, 0)
  tenth = 0.1 if np.dtype(thr_dtype) == np.float64 else CC.F32_TENTH  # (a float32 field: a tie with the data instead)
  field[(0,) + at(1, 2)] = tenth
  field[(size - 1,) + at(1, 2)] = F64_ABOVE_F32_TENTH if np.dtype(thr_dtype) == np.float64 and size > 1 else tenth
  p[1, 2, 0], t[1, 2, 0] = CC.F32_TENTH, CC.F32_BELOW_TENTH
  if fr or size > 1:  # (one threshold that does not vary over the rows stays the rounding edge)
    field[(size // 2,) + at(1, 3)] = 0.25
  p[1, 3, 0] = t[1, 3, 0] = 0.25
  if fr or (fx and nx > 1):  # a NaN threshold under a good point, (lead 1, row 4, x nx - 1)
    field[(size // 2, 1 if fl else 0, 4 if fr else 0, nx - 1 if fx else 0)] = np.nan
    p[1, 4, nx - 1], t[1, 4, nx - 1] = 0.5, -0.5
    mask[4, nx - 1] = True
  mask[2, 0] = mask[3, 0] = True
  # NaN data
  p[0, 0, nx - 1], t[0, 1, nx - 1] = np.nan, np.nan
  mask[0, nx - 1] = mask[1, nx - 1] = True
  if flags & FLAG_MASKED:
    mask[4, nx // 2] = False
    p[0, 4, nx // 2] = np.nan
  if transposed:
    p = np.ascontiguousarray(np.swapaxes(p, 1, 2)).swapaxes(1, 2)
    t = np.ascontiguousarray(np.swapaxes(t, 1, 2)).swapaxes(1, 2)
  root = np.ascontiguousarray(np.moveaxis(field, 0, -1)) if inner else field
  es = [s // root.itemsize for s in root.strides]
  es = es[-1:] + es[:-1] if inner else es  # -> (thr, lead, row, x)
  strides = {'thr': es[0], 'lead': es[1] if fl else 0, 'row': es[2] if fr else 0, 'x': es[3] if fx else 0}
  return FieldCase(p, t, mask, root, strides, size)


def assert_not_all_nan(want, flags, what=''):
  """At least half of the plain and masked partials are finite; under skipna every output is."""
  if flags & FLAG_SKIPNA:
    assert np.isfinite(want).all(), what
  else:
    share = float(np.isfinite(want).mean())
    assert share >= 0.5, (what, 'finite share', share)
    assert np.isnan(want).any(), (what, 'no poisoned partial')


def _self_check():
  for flags in (0, FLAG_MASKED, FLAG_SKIPNA, FLAG_MASKED | FLAG_SKIPNA):
    for varies in VARIES:
      for depth_chunk in (5, 2):
        for x_kept in (False, True):
          for nx in (1, 65):
            case = field_case(3, 3, 2, 5, nx, np.float32, np.float64, flags, varies)
            want, _ = expected(case, flags, depth_chunk, x_kept)
            assert_not_all_nan(want, flags, (flags, varies, depth_chunk, x_kept, nx))


_self_check()
