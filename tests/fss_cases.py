"""The three terms of the fractions skill score restated per point in NumPy, the partials of a plan in float64, the case lists and
the derived bounds that tests/test_fss.py, tests/test_gpu_fss.py and tests/test_gpu_fss_api.py share (include/wbx.h: wbx_fss_partial).

Per point (y, x), n odd and greater than 1, h = (n - 1) / 2:
    S = the sum of the n x n window (longitude cyclic), NaN members taken as 0;  H = the number of NaN members
    F = float32(float64(S) / float64(n * n)), NaN where H > 0, 0 at border points (y < h, y >= nlat - h, and x < h or x >= nlon - h
        unless wrap_longitude) whatever the window holds
    lanes, in float32 arithmetic: (Pf - Tf)^2, Pf^2, Tf^2
n == 1: F is the input, in the input's type, no border, the squares in that type.
The window sums are formed in extended precision (np.longdouble: 64 mantissa bits) by 2 n shifted additions, so they are EXACT for
0 / 1 and small-integer fields and correct to 2^-63 relative otherwise; the latitude shifts wrap, which touches border rows only.

Bounds (u = 2^-53, v = 2^-24).
  Sums.  A float64 sum of N terms in any order lies within N u sum |v_i| of the exact sum to first order (N (N - 1) u <= 1 here).
  Fractions on inputs whose window sums are not exact (Gaussian fields), M = max |x|, B <= 64 rows in a band: the header's
      |dS| <= u n M (n (n + 2 B) + 84 nlon + 8),    dq = |dS| / n^2 + 2 u |S| / n^2   (the kernel's quotient and this file's)
  Two float64 numbers dq apart round to float32 numbers at most e = dq + 2 v |F| + 2^-149 apart (half an ulp each, an ulp is at
  most 2 v |F|).  With |Pf' - Pf| <= ep and |Tf' - Tf| <= et:
      lane 1:  |Pf'^2 - Pf^2| <= (2 |Pf| + ep) ep, and each float32 product is within v of its exact value:
               b1 = (2 |Pf| + ep) ep + 2 v (Pf^2 + (2 |Pf| + ep) ep) + 2^-149;  lane 2 likewise
      lane 0:  d = fl(Pf - Tf): |d' - d| <= ed = ep + et + 2 v (|d| + ep + et), then the square as above with (|d|, ed).
  The test sums these per partial and adds the summation bound."""
import numpy as np

U = 2.0 ** -53
V = 2.0 ** -24
LANES = 3
MAX_BAND_ROWS = 64

# (nlat, nlon): the smallest that reach every path of the kernel -- one column per thread and one band (9 x 11, 12 x 16); a lane
# that owns two columns, nlon no multiple of 64 (5 x 300); more rows than two bands of the smallest band the library picks, the last
# band ragged (43 x 24: six bands of 8 rows at n = 3 and 5, the last of three rows; one band at n = 23); and every instantiation
# fss_kernel<T, NC> as built: NC = 1 (11, 16, 24 columns), 2 (300), 4 (5 x 600: three columns owned, the fourth beyond the circle), 6
# (5 x 1440, the 0.25 degree circle) and 8 (9 x 2048, the longest circle)
SHAPES = ((9, 11), (12, 16), (5, 300), (43, 24), (5, 600), (5, 1440), (9, 2048))
WIDE = 600  # from this many longitudes on the GPU tests take one key and two fields


def sizes_for(nlat, nlon):
  """n in {1, 3, 5, the largest odd n <= min(nlat, nlon)}."""
  top = min(nlat, nlon)
  top -= 1 - top % 2
  return sorted({1, 3, 5, top} & set(range(1, top + 1)))


def window_sums(x, n):
  """(S as longdouble, H as int64) over the last two axes, both cyclic."""
  x = np.asarray(x)
  nan = np.isnan(x)
  z = np.where(nan, 0, x).astype(np.longdouble)
  c = nan.astype(np.int64)
  h = (n - 1) // 2
  for axis in (-2, -1):
    z = sum(np.roll(z, s, axis=axis) for s in range(-h, h + 1))
    c = sum(np.roll(c, s, axis=axis) for s in range(-h, h + 1))
  return z, c


def border(shape, n, wrap):
  nlat, nlon = shape[-2:]
  h = (n - 1) // 2
  y, x = np.arange(nlat)[:, None], np.arange(nlon)[None, :]
  b = (y < h) | (y >= nlat - h)
  if not wrap:
    b = b | (x < h) | (x >= nlon - h)
  return np.broadcast_to(b, shape[-2:])


def fractions(x, n, wrap):
  """The neighbourhood fraction of every point: the input itself for n == 1, else float32."""
  x = np.asarray(x)
  if n == 1:
    return x
  s, c = window_sums(x, n)
  f = (s.astype(np.float64) / np.float64(n * n)).astype(np.float32)
  f = np.where(c > 0, np.float32(np.nan), f)
  return np.where(border(x.shape, n, wrap), np.float32(0), f).astype(np.float32)


def point_values(p, t, n, wrap):
  """float64 [3, ...]: the three lanes of every point, formed in float32 (n > 1) or the input type (n == 1)."""
  pf, tf = fractions(p, n, wrap), fractions(t, n, wrap)
  with np.errstate(invalid='ignore', over='ignore'):
    d = pf - tf
    return np.stack([d * d, pf * pf, tf * tf]).astype(np.float64)


def point_bounds(p, t, n, wrap):
  """float64 [3, ...]: how far the kernel's lanes of a point may lie from point_values on inputs whose sums are not exact."""
  p, t = np.asarray(p), np.asarray(t)
  if n == 1:
    return np.zeros((LANES,) + p.shape)
  nlon = p.shape[-1]
  es, fs = [], []
  for x in (p, t):
    m = float(np.nanmax(np.abs(x))) if np.isfinite(x).any() else 0.0
    s, _ = window_sums(x, n)
    ds = U * n * m * (n * (n + 2 * MAX_BAND_ROWS) + 84 * nlon + 8)
    dq = ds / (n * n) + 2 * U * np.abs(s.astype(np.float64)) / (n * n)
    f = np.abs(np.nan_to_num(fractions(x, n, wrap).astype(np.float64)))
    es.append(np.where(border(x.shape, n, wrap), 0.0, dq + 2 * V * f + 2.0 ** -149))
    fs.append(f)
  square = lambda a, e: (2 * a + e) * e + 2 * V * (a * a + (2 * a + e) * e) + 2.0 ** -149
  (ep, et), (fp, ft) = es, fs
  d = np.abs(np.nan_to_num(fractions(p, n, wrap).astype(np.float64) - fractions(t, n, wrap).astype(np.float64)))
  ed = ep + et + 2 * V * (d + ep + et)
  out = np.stack([square(d, ed), square(fp, ep), square(ft, et)])
  return np.where(np.stack([ep + et, ep, et]) == 0, 0.0, out)


def lanes_total(flags):
  return 2 * LANES if flags & 2 else (LANES + 1 if flags & 1 else LANES)


def partials(values, mask, flags, depth_chunk, x_kept, bounds=None):
  """values [3, key, depth, lat, lon] (point_values), mask broadcastable to [key, depth, lat, lon] (nonzero = valid) ->
  (want, mag, nterm[, slack]): want[key][lat][chunk][lanes_total][nj] the partials summed in extended precision and rounded once,
  mag = sum |v| and nterm = the number of terms per VALUE-lane partial, slack = the sum of `bounds` over the same points."""
  _, nkey, ndepth, nlat, nlon = values.shape
  masked, skipna = bool(flags & 1), bool(flags & 2)
  valid = np.broadcast_to(np.asarray(mask) != 0, values.shape[1:]) if masked else np.ones(values.shape[1:], bool)
  nchunk = -(-ndepth // depth_chunk)
  nj = nlon if x_kept else 1
  want = np.zeros((nkey, nlat, nchunk, lanes_total(flags), nj))
  mag = np.zeros((nkey, nlat, nchunk, LANES, nj))
  nterm = np.zeros((nkey, nlat, nchunk, LANES, nj))
  slack = np.zeros((nkey, nlat, nchunk, LANES, nj))
  red = (lambda a: a.sum(axis=1)) if x_kept else (lambda a: a.sum(axis=(1, 3))[..., None])  # [key, depth, lat, lon] -> [key, lat, nj]
  for c in range(nchunk):
    sl = slice(c * depth_chunk, min((c + 1) * depth_chunk, ndepth))
    ok = valid[:, sl]
    for l in range(LANES):
      v = np.where(ok, values[l][:, sl], 0.0)  # a masked-out point contributes exactly 0 whatever it holds
      use = ok
      if skipna:
        use = ok & ~np.isnan(v)
        v = np.where(np.isnan(v), 0.0, v)
        want[:, :, c, LANES + l] = red(use.astype(np.float64))
      with np.errstate(invalid='ignore'):
        want[:, :, c, l] = red(v.astype(np.longdouble)).astype(np.float64)
      mag[:, :, c, l] = red(np.abs(np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)))
      nterm[:, :, c, l] = red(np.ones_like(v))
      if bounds is not None:
        slack[:, :, c, l] = red(np.where(use, bounds[l][:, sl], 0.0))
    if masked and not skipna:
      want[:, :, c, LANES] = red(ok.astype(np.float64))
  return (want, mag, nterm) if bounds is None else (want, mag, nterm, slack)


def same_numbers(a, b):
  """Bit for bit, every NaN counting as the same number."""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return a.shape == b.shape and bool(np.array_equal(np.where(np.isnan(a), 0, a).view(np.uint64), np.where(np.isnan(b), 0, b).view(np.uint64))
                                     and np.array_equal(np.isnan(a), np.isnan(b)))


def indicator_fields(shape, dtype, seed, nan_share=0.0):
  """0 / 1 fields with smooth blobs (what FSS gets), `nan_share` of the points NaN."""
  rng = np.random.default_rng(seed)
  base = rng.random(shape)
  p = (base + 0.25 * rng.normal(size=shape) > 0.6).astype(dtype)
  t = (base > 0.6).astype(dtype)
  if nan_share:
    p[rng.random(shape) < nan_share] = np.nan
    t[rng.random(shape) < nan_share] = np.nan
  return p, t


def integer_fields(shape, dtype, seed):
  rng = np.random.default_rng(seed)
  return rng.integers(-3, 6, size=shape).astype(dtype), rng.integers(-3, 6, size=shape).astype(dtype)


def gaussian_fields(shape, dtype, seed):
  rng = np.random.default_rng(seed)
  return (rng.normal(size=shape) * 3).astype(dtype), (rng.normal(size=shape) * 3 + 0.5).astype(dtype)


def mean_bound_from_ulps(pf, tf):
  """How far the mean of a term may move when every float32 fraction moves by at most one ulp (2 v |F|, v = 2^-24): the lanes'
  bounds above with ep = 2 v |Pf|, et = 2 v |Tf|, as a relative bound on the three means -> (b0, b1, b2) absolute."""
  d = np.abs(np.nan_to_num(np.asarray(pf, np.float64) - np.asarray(tf, np.float64)))
  pf, tf = np.abs(np.nan_to_num(np.asarray(pf, np.float64))), np.abs(np.nan_to_num(np.asarray(tf, np.float64)))
  ep, et = 2 * V * pf + 2.0 ** -149, 2 * V * tf + 2.0 ** -149
  square = lambda a, e: (2 * a + e) * e + 2 * V * (a * a + (2 * a + e) * e) + 2.0 ** -149
  ed = ep + et + 2 * V * (d + ep + et)
  return square(d, ed), square(pf, ep), square(tf, et)
