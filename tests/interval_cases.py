"""The interval statistics (Covered, Confident, JaccardDistant) restated in float64 NumPy, as include/wbx.h states them for
wbx_ens_interval_partial, with the (k, g) table, the padded network size and the case generator of the tests.

The restatement is exact by construction: members are sorted in their own type, converted to float64 (exact), and every later
operation is ONE IEEE float64 operation of NumPy, in the order the header gives.  The kernel does the same operations, so every
indicator -- and every stage-1 partial, a sum of at most 2^53 zeros and ones -- is compared bit for bit, without a tolerance."""
import fractions

import numpy as np

SIZES = (4, 8, 16, 32, 50, 51, 64)  # the generated sorting networks (csrc/wbx_sortnet3_gen.hpp)
COVERED, CONFIDENT, JACCARD = 1, 2, 4  # WBX_IVL_*
BITS = (COVERED, CONFIDENT, JACCARD)
LEVELS = (0.0, 0.1, 0.2, 0.5, 0.7, 0.9, 1.0)  # the quantile labels of the test climatologies
MEMBER_AXES = ('outer', 'inner')  # where the member axis of p is stored


def padded(m: int) -> int:
  """The network size an ensemble of m members is padded to."""
  return next(s for s in SIZES if m <= s)


def bound(q, m: int):
  """(k, g): h = q (m - 1), k = floor(h), g = h - k, in float64."""
  h = np.float64(q) * np.float64(m - 1)
  k = np.floor(h)
  return int(k), float(h - k)


def bound_table(levels, m: int):
  return [bound(q, m) for q in levels]


def quantile_sorted(xs, k: int, g: float):
  """NumPy's `linear` quantile from the float64 members xs[M, ...] sorted along axis 0, in NumPy's order of operations."""
  m = xs.shape[0]
  with np.errstate(all='ignore'):
    a, b = xs[k], xs[min(k + 1, m - 1)]
    d = b - a
    return a + d * np.float64(g) if g < 0.5 else b - d * (np.float64(1.0) - np.float64(g))


def ens_quantile(p, q):
  """The quantile level q of the members p[M, ...] (any float type): sorted in their own type, float64 from there; NaN where a
  member is NaN."""
  nan = np.isnan(p).any(axis=0)
  xs = np.sort(p, axis=0).astype(np.float64)  # (NaN sorts last; such points are overwritten below)
  out = np.array(quantile_sorted(xs, *bound(q, p.shape[0])), np.float64)
  out[nan] = np.nan
  return out


def covered(p, t, levels):
  lo, hi = ens_quantile(p, levels[0]), ens_quantile(p, levels[1])
  t = np.asarray(t, np.float64)
  with np.errstate(all='ignore'):
    return (lo <= t) & (t <= hi)


def confident(p, c_lo, c_hi, levels, threshold):
  lo, hi = ens_quantile(p, levels[0]), ens_quantile(p, levels[1])
  with np.errstate(all='ignore'):
    return (hi - lo) < np.float64(threshold) * (np.asarray(c_hi, np.float64) - np.asarray(c_lo, np.float64))


def jaccard_distant(p, c_lo, c_hi, levels, threshold):
  a_lo, a_hi = ens_quantile(p, levels[0]), ens_quantile(p, levels[1])
  b_lo, b_hi = np.asarray(c_lo, np.float64), np.asarray(c_hi, np.float64)
  with np.errstate(all='ignore'):
    overlap = np.clip(np.minimum(a_hi, b_hi) - np.maximum(a_lo, b_lo), 0.0, None)  # (minimum, maximum and clip keep a NaN)
    union = (a_hi - a_lo) + (b_hi - b_lo) - overlap
    index = np.where(union > 0, overlap / union, 1.0)
    return (1.0 - index) > np.float64(threshold)


def indicators(p, t, c, lanes: int, params):
  """The requested indicators in value-lane order as float64 zeros and ones.  c[len(LEVELS), ...]: the climatology at LEVELS;
  params: {bit: (levels, threshold)}."""
  out = []
  pick = lambda q: c[LEVELS.index(q)]
  if lanes & COVERED:
    out.append(covered(p, t, params[COVERED][0]))
  if lanes & CONFIDENT:
    lv, thr = params[CONFIDENT]
    out.append(confident(p, pick(lv[0]), pick(lv[1]), lv, thr))
  if lanes & JACCARD:
    lv, thr = params[JACCARD]
    out.append(jaccard_distant(p, pick(lv[0]), pick(lv[1]), lv, thr))
  return [np.broadcast_to(v, p.shape[1:]).astype(np.float64) for v in out]


def partials(vals, mask, flags: int, depth_chunk: int, x_kept: bool):
  """partial[key][chunk][lanes_total][nj] of the indicator fields vals[lane][key, depth, x] under the library's count-lane
  convention (flags: 1 masked, 2 skipna); mask[depth, x] or None.  Sums of zeros and ones: exact in any order."""
  nkey, ndepth, nx = vals[0].shape
  valid = np.ones((nkey, ndepth, nx), bool) if not (flags & 1) else np.broadcast_to(np.asarray(mask) != 0, (nkey, ndepth, nx))
  lanes = [np.where(valid, v, 0.0) for v in vals]
  if flags & 2:
    lanes += [valid.astype(np.float64)] * len(vals)
  elif flags & 1:
    lanes += [valid.astype(np.float64)]
  nchunk = -(-ndepth // depth_chunk)
  out = np.zeros((nkey, nchunk, len(lanes), nx if x_kept else 1))
  for c in range(nchunk):
    rows = slice(c * depth_chunk, min((c + 1) * depth_chunk, ndepth))
    for l, v in enumerate(lanes):
      out[:, c, l, :] = v[:, rows].sum(axis=1) if x_kept else v[:, rows].sum(axis=(1, 2))[:, None]
  return out


def arrange(p, where: str):
  """p[M, ...] stored with the member axis outermost or innermost: a transposed view of a contiguous array."""
  if where == 'outer':
    return np.ascontiguousarray(p)
  return np.moveaxis(np.ascontiguousarray(np.moveaxis(p, 0, -1)), -1, 0)


def values(seed: int, m: int, shape, dtype):
  """Members p[M, *shape], targets t[*shape] and a climatology c[len(LEVELS), *shape] on the grid of eighths around 280, so that
  ties among the members and targets exactly on a bound are common, and the two spreads are of one size, so that every indicator
  takes both values."""
  rng = np.random.default_rng(seed)
  p = (280.0 + rng.integers(-40, 41, size=(m,) + tuple(shape)) / 8.0).astype(dtype)
  t = (280.0 + rng.integers(-40, 41, size=tuple(shape)) / 8.0).astype(dtype)
  centre = 280.0 + rng.integers(-24, 25, size=tuple(shape)) / 8.0
  half = rng.integers(0, 96, size=tuple(shape)) / 8.0
  c = np.stack([centre + (2.0 * q - 1.0) * half for q in LEVELS]).astype(dtype)
  return p, t, c


EDGE_KINDS = ('target_on_low', 'target_on_high', 'nan_member', 'nan_target', 'nan_clim', 'pos_inf_member', 'neg_inf_member',
              'two_pos_inf', 'equal_members_point_clim', 'equal_members', 'integers')


def put_edge(p, t, c, at, kind: str, params, rng):
  """Rewrites the point `at` of (p, t, c) into the edge case `kind`."""
  m = p.shape[0]
  col = (slice(None),) + tuple(at)
  lv = params.get(COVERED, params.get(CONFIDENT, params.get(JACCARD)))[0]
  if kind in ('target_on_low', 'target_on_high'):  # exactly on the restated bound (representable: it is rounded to the type first)
    q = ens_quantile(p[col][:, None], lv[kind == 'target_on_high'])[0]
    t[at] = q  # (float32: lands on the bound only where the bound is a float32; both outcomes are the restatement's)
  elif kind == 'nan_member':
    p[(int(rng.integers(m)),) + tuple(at)] = np.nan
  elif kind == 'nan_target':
    t[at] = np.nan
  elif kind == 'nan_clim':
    c[(int(rng.integers(len(LEVELS))),) + tuple(at)] = np.nan
    c[(LEVELS.index(lv[0]),) + tuple(at)] = np.nan
  elif kind == 'pos_inf_member':  # the largest member: at the wanted rank or next to it for the upper levels
    p[(int(rng.integers(m)),) + tuple(at)] = np.inf
  elif kind == 'neg_inf_member':
    p[(int(rng.integers(m)),) + tuple(at)] = -np.inf
  elif kind == 'two_pos_inf':  # d = inf - inf
    p[(0,) + tuple(at)] = np.inf
    p[(m - 1,) + tuple(at)] = np.inf
  elif kind == 'equal_members_point_clim':  # union 0: index = 1
    p[col] = p[(0,) + tuple(at)]
    c[col] = p[(0,) + tuple(at)]
  elif kind == 'equal_members':
    p[col] = p[(0,) + tuple(at)]
  elif kind == 'integers':
    p[col] = rng.integers(270, 290, size=m).astype(p.dtype)
    t[at] = rng.integers(270, 290)


def interval_case(seed: int, m: int, nkey: int, ndepth: int, nx: int, dtype, lanes: int, params, flags: int, depth_chunk: int,
                  x_kept: bool, edges: bool = True):
  """-> p[M, key, depth, x], t[key, depth, x], c[level, key, depth, x], mask[depth, x] and the stage-1 partial the entry must
  give.  With `edges`, one point per edge kind (as far as the frame holds them) is rewritten first."""
  rng = np.random.default_rng(seed)
  p, t, c = values(seed, m, (nkey, ndepth, nx), dtype)
  if edges:
    n = nkey * ndepth * nx
    spots = rng.choice(n, size=min(len(EDGE_KINDS), n), replace=False)
    for s, kind in zip(spots, EDGE_KINDS):
      put_edge(p, t, c, tuple(int(v) for v in np.unravel_index(s, (nkey, ndepth, nx))), kind, params, rng)
  mask = (rng.random((ndepth, nx)) < 0.7).astype(np.uint8)
  want = partials(indicators(p, t, c, lanes, params), mask, flags, depth_chunk, x_kept)
  return p, t, c, mask, want


# ---- a fused multiply-add would flip the indicator ------------------------------------------------------------------------------
def fma_quantile(xs, k: int, g: float) -> float:
  """The quantile of the sorted float64 members xs[M] as a kernel that contracts A + d g (or B - d (1 - g)) into ONE fused
  multiply-add would form it: d and 1 - g rounded as before, the product and the sum rounded once, exactly (fractions.Fraction)."""
  F = fractions.Fraction
  a, b = float(xs[k]), float(xs[min(k + 1, len(xs) - 1)])
  d = b - a
  if g < 0.5:
    return float(F(a) + F(d) * F(g))
  return float(F(b) - F(d) * F(1.0 - g))


def fma_flip_point(m: int, q: float, dtype, seed: int = 0):
  """-> (members[M], target, level pair, Covered as stated, Covered under contraction): a point whose lower bound at level q is
  rounded differently by a fused multiply-add, with the target on the bound that makes Covered differ."""
  rng = np.random.default_rng(seed)
  k, g = bound(q, m)
  for _ in range(10000):
    x = (rng.random(m) * 10.0).astype(dtype)  # (A and d of one magnitude: the product's rounding shows in the sum)
    xs = np.sort(x).astype(np.float64)
    plain, fused = float(quantile_sorted(xs, k, g)), fma_quantile(xs, k, g)
    target = min(plain, fused)  # the smaller of the two as the target: lo <= t holds for exactly one of them ...
    if plain != fused and np.dtype(dtype).type(target) == target and target <= xs[-1]:  # ... if the type holds it
      return x, np.dtype(dtype).type(target), (q, 1.0), bool(plain <= target), bool(fused <= target)
  raise AssertionError('no such point')


# ---- inputs of the public-API tests ---------------------------------------------------------------------------------------------
API_DIMS = ('init_time', 'lead_time', 'latitude', 'longitude')
API_SHAPE = (2, 3, 6, 9)
API_LAT = np.linspace(-75, 75, API_SHAPE[2])
API_LON = np.arange(API_SHAPE[3]) * (360.0 / API_SHAPE[3])
API_INIT = np.array(['2020-01-01T00', '2020-01-02T00'], dtype='datetime64[ns]')
API_LEAD = (np.arange(API_SHAPE[1]) * 12).astype('timedelta64[h]').astype('timedelta64[ns]')
API_DAYS, API_HOURS = np.arange(1, 9), np.array([0, 12])


def api_arrays(dtype, m: int, seed: int = 11, nans: bool = False):
  """p[number, init, lead, lat, lon], t[init, lead, lat, lon], the climatology clim[dayofyear, hour, quantile, lat, lon] at LEVELS,
  the same climatology aligned with the valid times c[level, init, lead, lat, lon], and a validity mask[lat, lon]."""
  rng = np.random.default_rng(seed + 1)
  p, t, _ = values(seed, m, API_SHAPE, dtype)
  _, _, clim = values(seed + 2, 1, (len(API_DAYS), len(API_HOURS)) + API_SHAPE[2:], dtype)  # [level, day, hour, lat, lon]
  if nans:
    p[rng.random(p.shape) < 0.01] = np.nan
    t[rng.random(t.shape) < 0.02] = np.nan
    clim[rng.random(clim.shape) < 0.01] = np.nan
  valid = API_INIT[:, None] + API_LEAD[None, :]
  day = (valid.astype('datetime64[D]') - valid.astype('datetime64[Y]').astype('datetime64[D]')).astype(int) + 1
  hour = (valid - valid.astype('datetime64[D]')).astype('timedelta64[h]').astype(int)
  c = clim[:, np.searchsorted(API_DAYS, day), np.searchsorted(API_HOURS, hour)]  # [level, init, lead, lat, lon]
  mask = rng.random(API_SHAPE[2:]) > 0.3
  return p, t, np.ascontiguousarray(np.moveaxis(clim, 0, 2)), c, mask


def api_inputs(dtype, m: int, seed: int = 11, nans: bool = False, mask: bool = False, device: bool = False, member_last: bool = False):
  """-> ({'v': predictions}, {'v': targets}, climatology Dataset, (p, t, c, mask) as NumPy arrays).  `mask`: a `mask` coordinate on
  predictions and targets; `device`: torch tensors in HBM."""
  from weatherbenchx_amd import xarray_lite as xr  # pylint: disable=g-import-not-at-top
  p, t, clim, c, valid = api_arrays(np.dtype(dtype).type, m, seed, nans)
  if device:
    import torch  # pylint: disable=g-import-not-at-top
    load = lambda a: torch.as_tensor(np.array(a)).cuda()
  else:
    load = np.array
  cs = {'init_time': API_INIT, 'lead_time': API_LEAD, 'latitude': API_LAT, 'longitude': API_LON}
  if mask:
    cs['mask'] = (('latitude', 'longitude'), valid.copy())
  pa, pdims = (np.moveaxis(p, 0, -1), API_DIMS + ('number',)) if member_last else (p, ('number',) + API_DIMS)
  pred = {'v': xr.DataArray(load(np.ascontiguousarray(pa)), dims=pdims, coords=dict(cs, number=np.arange(m)), name='v')}
  targ = {'v': xr.DataArray(load(t), dims=API_DIMS, coords=cs, name='v')}
  climatology = xr.Dataset({'v': xr.DataArray(
      load(clim), dims=('dayofyear', 'hour', 'quantile', 'latitude', 'longitude'),
      coords={'dayofyear': API_DAYS, 'hour': API_HOURS, 'quantile': np.array(LEVELS), 'latitude': API_LAT, 'longitude': API_LON})})
  return pred, targ, climatology, (p, t, c, valid)
