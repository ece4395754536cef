"""Seeded inputs, per-point expectations and per-point error bounds for the five ensemble lanes (CRPS skill, CRPS spread,
ensemble variance, unbiased ensemble-mean MSE, ensemble-mean squared error): tests/test_gpu_ensemble_points.py and
tests/test_ensemble_points_edges.py.  A plain helper module, not a fixture file: pure NumPy.

Expectation: oracle/wbx_oracle.py on the float64-widened inputs, then the conventions include/wbx.h documents and nothing else
(`expected_lanes`).  Bounds: derived from the arithmetic of each kernel family (`lane_bounds`), never from what a kernel gives:

  u = 2^-24, eps = 2^-52;  s = the shift the kernel documents;  e_i = x_i - s;  A = mean |e_i|;  Q = sum e_i^2 / (M - 1)

  family     arithmetic                                       s
  sorted64   fp64 sums over the sorted registers (stats64)    the target if finite, else the smallest member
  pair       stats64 with fp32 rows of |x_i - x_j|            the target if finite, else the first member in memory
  generic    EnsOpGeneric (M > 64, float64): fp64 pair form   the first member in memory, whatever the target is
  chain32    fp32 chains of <= 8 terms (stats32, M = 50 / 51  the sorted median x_(M/2)
             on ens_pipe_kernel / ens_atoms_kernel)

  lane 0   fp64: (M + 4) eps relative                         chain32: 9 u relative
  lane 1   sorted64: absolute 2 (M + 4) eps A (rank weights <= M - 1); generic: (M + 4) eps relative (non-negative terms);
           pair: (M + 1) u relative (fp32 rows of <= M - 1 non-negative terms);  chain32: 9 u relative
  lane 2   fp64: absolute (M + 6) eps Q                       chain32: absolute 9 u Q
  lane 4   d = error of the mean error: fp64 (M + 4) eps A, chain32 9 u A; the generic operator forms the mean error as
           fl(fl(x_0 - t) + mean e): x_0 - t is rounded once (eps / 2 |x_0 - t|) and the sum once (eps / 2 (|x_0 - t| + A)), so
           there d = (M + 4) eps A + 2 eps |x_0 - t|;  bound 2 sqrt(lane 4) d + d^2
  lane 3   lane-4 bound + lane-2 bound / M
A tile of the chain32 kernels that took the wave-uniform fp64 escape satisfies the (tighter) generic row; the chain32 row is
applied to it all the same -- a test cannot see which way a wave went.  A partial of N points: the sum of its points' bounds
+ (N + 2) eps sum |value| (for x-weighted partials every term times its weight).  Count lanes are bit-equal."""
import numpy as np

from oracle import wbx_oracle as O
import indicator_cases as IC

U, EPS = 2.0 ** -24, 2.0 ** -52
NLANE = 5
PD, SD, MEMBER = ('lead_time', 'number', 'row', 'x'), ('lead_time', 'row', 'x'), 'number'
# both sides of every register-bucket edge (4 | 8 | 16 | 32 | 64), the two exact sizes with a neighbour on each side, two generic
M_F32 = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 49, 50, 51, 52, 64, 65, 100)
M_F64 = (8, 51)
M_BINNED = (2, 4, 5, 16, 17, 50, 51, 64)
M_SKIPNA_ENS_EDGES = (4, 5, 8, 9, 16, 17, 32, 49, 52, 64)
SORT, PAIRWISE = 0, 1
PIPELINED = ('pipe', 'flat', 'binned')  # the routes whose M = 50 / 51 instantiations run stats32


def family(route, m, dtype, algo=SORT):
  """The arithmetic a route runs for (M, dtype, algo).  route: 'map', 'xk', 'xr', 'xf1', 'masked', 'pipe', 'flat', 'binned'."""
  if np.dtype(dtype) == np.float64 or m > 64:
    return 'generic'
  if algo == PAIRWISE:
    return 'pair'
  return 'chain32' if route in PIPELINED and m in (50, 51) else 'sorted64'


def fair_of(m, i=0):
  """`fair` per case, so that both values occur for every M."""
  return bool((m + i) & 1)


def _members_last(p):
  """p[lead, member, row, x] -> float64 [lead, row, x, member] (the members in memory order)."""
  return np.moveaxis(np.asarray(p, np.float64), 1, -1)


def _ieee_restatement(x, t, fair, shift_is_target):
  """The documented formulas on e = x - s in float64, for the NaN / inf pattern of the families that have no poison rule:
  s = the target if it is finite and `shift_is_target`, else the first member in memory.  [..., member], [...] -> [..., 5]."""
  m = x.shape[-1]
  with np.errstate(all='ignore'):
    x0 = x[..., 0]
    s = np.where(np.isfinite(t), t, x0) if shift_is_target else x0
    e = x - s[..., None]
    se, sq = e.sum(axis=-1), (e * e).sum(axis=-1)
    sabs = np.abs(x - t[..., None]).sum(axis=-1)
    pair = np.zeros(t.shape)
    for i in range(1, m):
      pair = pair + np.abs(x[..., i:i + 1] - x[..., :i]).sum(axis=-1)
    mean_e = se / m
    mean_d = (s - t) + mean_e
    var = (sq - se * mean_e) / (m - 1.0)
    return np.stack([sabs / m, 2.0 * pair / (m * (m - float(fair))), var, mean_d * mean_d - var / m, mean_d * mean_d], axis=-1)


def expected_lanes(fam, p, t, fair):
  """p[lead, member, row, x], t[lead, row, x] (float32 or float64) -> float64 [lead, row, x, 5]: the oracle on the widened
  inputs, then the conventions of include/wbx.h:
    * float32 rank form, M <= 64 ('sorted64', 'chain32'): a NaN or infinite member makes all five lanes NaN;
    * 'pair', 'generic': plain IEEE arithmetic of the documented formulas where a member is not finite;
    * a NaN / infinite target leaves spread and variance finite (they never look at it);
    * M = 1: variance and unbiased MSE NaN, the fair spread NaN, the unfair spread 0."""
  p64, t64 = np.asarray(p, np.float64), np.asarray(t, np.float64)
  m = p64.shape[1]
  with np.errstate(all='ignore'):
    # The oracle sees the members ABOUT THE TARGET, (x - t, 0), wherever the target is finite: all five lanes are invariant under
    # a common shift, x - t costs eps / 2 relative to each |x_i - t| (1 / (2 M + 8) of the fp64 bounds), and the oracle's own
    # rounding of mean(x) - t is then eps A instead of eps |mean x| -- on a target that cancels against the ensemble mean the
    # latter is as large as the bounds it is the reference for.
    tfin = np.isfinite(t64)
    ps, ts = np.where(tfin[:, None], p64 - t64[:, None], p64), np.where(tfin, 0.0, t64)
    skill = O.crps_skill(ps, PD, ts, SD, MEMBER)[0]
    # (the pair form of the oracle: a sum of non-negative terms, no cancellation of its own; the two forms are one number)
    spread = O.crps_spread(ps, PD, MEMBER, fair=fair, use_sort=False)[0] if m >= 2 else np.full(t64.shape, np.nan if fair else 0.0)
    var = O.ensemble_variance(ps, PD, MEMBER)[0] if m >= 2 else np.full(t64.shape, np.nan)
    uemse = O.unbiased_ensemble_mean_squared_error(ps, PD, ts, SD, MEMBER)[0]
    emse = O.ensemble_mean_squared_error(ps, PD, ts, SD, MEMBER)[0]
  out = np.stack([skill, spread, var, uemse, emse], axis=-1)
  x = _members_last(p64)
  bad = ~np.isfinite(x).all(axis=-1)
  if fam in ('sorted64', 'chain32'):
    out[bad] = np.nan
  elif bad.any():
    # (what stays finite at such a point is a sum that no member enters: the spread of a single member, 0)
    out[bad] = _ieee_restatement(x[bad], t64[bad], fair, fam == 'pair')
  return out


def lane_bounds(fam, p, t, stat):
  """Per-point absolute error bounds [lead, row, x, 5] (float64) of `stat` = expected_lanes(...) for the family (the table in
  the module docstring); NaN where the expected value is not finite."""
  x, t64 = _members_last(p), np.asarray(t, np.float64)
  m = x.shape[-1]
  with np.errstate(all='ignore'):
    if fam == 'chain32':
      s = np.sort(x, axis=-1)[..., m // 2]
    elif fam == 'generic':
      s = x[..., 0]
    else:
      s = np.where(np.isfinite(t64), t64, x.min(axis=-1) if fam == 'sorted64' else x[..., 0])
    e = x - s[..., None]
    a = np.abs(e).mean(axis=-1)
    q = (e * e).sum(axis=-1) / (m - 1.0) if m > 1 else np.zeros(t64.shape)
    r = 9 * U if fam == 'chain32' else (m + 4) * EPS
    b = np.empty(stat.shape)
    b[..., 0] = r * np.abs(stat[..., 0])
    if fam == 'sorted64':
      b[..., 1] = 2 * (m + 4) * EPS * a
    else:
      b[..., 1] = {'pair': (m + 1) * U, 'generic': (m + 4) * EPS, 'chain32': 9 * U}[fam] * np.abs(stat[..., 1])
    b[..., 2] = (9 * U if fam == 'chain32' else (m + 6) * EPS) * q
    d = r * a
    if fam == 'generic':  # mean error = fl(fl(x_0 - t) + mean e): one rounding of x_0 - t, one of the sum (<= eps / 2 (|x_0 - t| + A))
      d = d + 2 * EPS * np.abs(s - t64)
    b[..., 4] = 2 * np.sqrt(stat[..., 4]) * d + d * d
    b[..., 3] = b[..., 4] + b[..., 2] / m
  b[~np.isfinite(stat)] = np.nan
  return b


# ---- the fp32 chain sums of EnsOpF32::stats32 restated in NumPy (the header's error model; this project's own arithmetic) ------
def _fma32(a, b, c):
  # (a float32 product is exact in float64; the sum is rounded once to float64 and once to float32)
  return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def stats32_emulated(p, t, fair):
  """p[lead, member, row, x], t[lead, row, x] float32 with finite members, M = 50 / 51 -> [lead, row, x, 5]: the sorted
  members centred on the median, K = 8 interleaved fp32 chains per sum, chains added in pairs in fp32, the rest in fp64;
  the points outside compute<FAST32>'s thresholds through the fp64 formulas (the wave-uniform escape, per point here)."""
  xm = np.sort(np.moveaxis(np.asarray(p, np.float32), 1, -1), axis=-1)
  t = np.asarray(t, np.float32)
  mp = xm.shape[-1]
  k8, npair = 8, mp // 2
  c = xm[..., mp // 2]
  zero = np.zeros(t.shape, np.float32)
  se, sq, sa, dt = ([zero.copy() for _ in range(k8)] for _ in range(4))
  with np.errstate(all='ignore'):
    for i in range(npair):
      j, k = mp - 1 - i, i % k8
      ei, ej = xm[..., i] - c, xm[..., j] - c
      se[k] = se[k] + (ei + ej)
      sq[k] = _fma32(ej, ej, _fma32(ei, ei, sq[k]))
      sa[k] = (sa[k] + np.abs(xm[..., i] - t)) + np.abs(xm[..., j] - t)
      dt[k] = _fma32(np.full(t.shape, mp - 1 - 2 * i, np.float32), xm[..., j] - xm[..., i], dt[k])
    if mp & 1:
      sa[npair % k8] = sa[npair % k8] + np.abs(c - t)
    fold = lambda v: ((v[0] + v[4]).astype(np.float64) + (v[1] + v[5]).astype(np.float64)) + ((v[2] + v[6]).astype(np.float64) + (v[3] + v[7]).astype(np.float64))
    dse, dsq, dsa, ddt = fold(se), fold(sq), fold(sa), fold(dt)
    dm = float(mp)
    mean_e = dse * (1.0 / dm)
    mean_d = (c.astype(np.float64) - t.astype(np.float64)) + mean_e
    var = (dsq - dse * mean_e) * (1.0 / (dm - 1.0))
    out = np.stack([dsa * (1.0 / dm), ddt * (2.0 / (dm * (dm - float(fair)))), var, mean_d * mean_d - var * (1.0 / dm), mean_d * mean_d], axis=-1)
    rng_ = xm[..., -1] - xm[..., 0]
    big = np.fmax(np.maximum(np.abs(xm[..., 0]), np.abs(xm[..., -1])), np.abs(t))  # (fmaxf: a NaN target drops out, no escape)
    fast = ((rng_ == 0) | ((rng_ >= np.float32(2.0 ** -50)) & (rng_ <= np.float32(2.0 ** 60)))) & (big <= np.float32(2.0 ** 100))
  if not fast.all():
    x64 = np.moveaxis(np.asarray(p, np.float64), 1, -1)
    out[~fast] = _ieee_restatement(x64[~fast], t.astype(np.float64)[~fast], fair, False)
  return out


# ---- dense cases ---------------------------------------------------------------------------------------------------------------
# (a +inf target is held per point by the one-live-point cases: a dense skipna partial would sum it to +inf)
SPECIAL = ('nan_member', 'nan_target', 'pinf_member', 'ninf_member')


def place_special_points(p, t, row, first=0, step=1, names=SPECIAL):
  """The named special points in row `row` of every lead at x = first, first + step, ... (as far as the row is long) -> {name: x}.
  p is indexed [lead, member, row, x]."""
  m = p.shape[1]
  where = {}
  for i, name in enumerate(names):
    x = first + i * step
    if x >= t.shape[-1]:
      break
    where[name] = x
    if name == 'nan_member':
      p[:, m // 2, row, x] = np.nan
    elif name == 'pinf_member':
      p[:, m - 1, row, x] = np.inf   # (never the first member in memory: see include/wbx.h on the generic operator)
    elif name == 'ninf_member':
      p[:, m - 1, row, x] = -np.inf
    else:
      assert name == 'nan_target', name
      t[:, row, x] = np.nan
  return where


def dense_case(seed, m, nlead, nrow, nx, values='dyadic', dtype=np.float32, layout='member_outside', poison_rows=(), exposed_rows=None,
               inf_members=True):
  """-> (p, t, mask): p indexed [lead, member, row, x] ('ifs': a transposed view of a contiguous [member, lead, row, x] base),
  t[lead, row, x], mask[row, x] (False on ~30 % of the points).  Every point is live.
    'dyadic'   indicator_cases.gridded: ties are real ties, every sum is exact
    'anomaly'  members and targets ~ N(0, 1); on ~10 % of the points the members are +-10^U(-6, 6): the data on which the fp32
               chains round
    'cancel'   'anomaly' with the target within 1e-4 of the ensemble mean: lanes 3 and 4 cancel
  The special points (SPECIAL; without the infinite members where `inf_members` is off: on the families without the poison
  rule they give +-inf, which skipna does not count out) go into `poison_rows`; the mask hides them except on `exposed_rows`
  (default: all of them)."""
  rng = np.random.default_rng(seed)
  shape = (m, nlead, nrow, nx) if layout == 'ifs' else (nlead, m, nrow, nx)
  if values == 'dyadic':
    base = IC.gridded(rng, shape, -3, 3, dtype=dtype)
    IC.sprinkle(rng, base, negzero=0.01)
    t = IC.gridded(rng, (nlead, nrow, nx), -2, 2, dtype=dtype)
  else:
    base = rng.normal(size=shape)
    wide = rng.random((nlead, nrow, nx)) < 0.1
    mixed = np.sign(rng.normal(size=shape)) * 10.0 ** rng.uniform(-6, 6, size=shape)
    sel = np.broadcast_to(wide[None] if layout == 'ifs' else wide[:, None], shape)
    base = np.where(sel, mixed, base).astype(dtype)
    t = rng.normal(size=(nlead, nrow, nx)).astype(dtype)
  p = np.transpose(base, (1, 0, 2, 3)) if layout == 'ifs' else base
  if values == 'cancel':
    t = (p.astype(np.float64).mean(axis=1) + rng.uniform(-1e-4, 1e-4, size=t.shape)).astype(dtype)
  mask = rng.random((nrow, nx)) > 0.3
  exposed = set(poison_rows if exposed_rows is None else exposed_rows)
  for row in poison_rows:
    where = place_special_points(p, t, row, names=SPECIAL if inf_members else SPECIAL[:2])
    for x in where.values():
      mask[row, x] = row in exposed
  return p, t, mask


# ---- one live point per partial --------------------------------------------------------------------------------------------------
def live_points(m, seed=0):
  """[(name, members float32[M], target float32)]: the points that are put, one per partial, among points whose members all
  equal their target (all five lanes exactly 0 on every route)."""
  rng = np.random.default_rng(1000 + 7 * m + seed)
  f = np.float32
  ramp = np.linspace(0.0, 1.0, m).astype(f) if m > 1 else np.zeros(1, f)
  ordinary = rng.normal(size=m).astype(f)
  pts = [('ordinary', ordinary, f(rng.normal())),
         ('range0', np.full(m, 1.25, f), f(-0.5)),
         ('ties', (rng.integers(-2, 3, size=m) * 0.5).astype(f), f(0.5)),
         ('zeros', np.where(np.arange(m) % 2 == 0, f(-0.0), f(0.0)).astype(f), f(0.25)),
         ('subnormal', (rng.integers(-100, 100, size=m) * 2.0 ** -149).astype(f), f(3 * 2.0 ** -149)),
         ('sorted', np.sort(ordinary), f(0.1)),
         ('reversed', np.sort(ordinary)[::-1].copy(), f(0.1)),
         ('nan_target', ordinary.copy(), f(np.nan)),
         ('pinf_target', ordinary.copy(), f(np.inf)),
         # the escape thresholds of compute<FAST32>, each just inside and just outside
         ('range_2^-50', ramp * f(2.0 ** -50), f(2.0 ** -52)),
         ('range_2^-51', ramp * f(2.0 ** -51), f(2.0 ** -52)),
         ('range_2^60', ramp * f(2.0 ** 60), f(2.0 ** 58)),
         ('range_2^61', ramp * f(2.0 ** 61), f(2.0 ** 58)),
         ('big_2^100', np.full(m, 2.0 ** 100, f), f(2.0 ** 99)),
         ('big_2^101', np.full(m, 2.0 ** 101, f), f(2.0 ** 99))]
  if m > 1:
    for name, idx, v in (('nan_member', (m // 2,), np.nan), ('pinf_member', (m - 1,), np.inf), ('ninf_member', (m - 1,), -np.inf),
                         ('two_pinf_members', (m - 1, m // 2), np.inf)):
      x = ordinary.copy()
      x[list(idx)] = v
      pts.append((name, x, f(0.3)))
  return pts


def one_live_case(m, nlead, nrow, nx, depth_chunk, kinds, shift=0, layout='member_outside', dtype=np.float32, positions=None):
  """-> (p, t, live): every point has all members equal to its finite target, except one point in every SECOND partial (partials
  counted [lead][chunk]; where x is kept the live point's x column is its partial): live = [(lead, row, x, name)].  The kinds are
  dealt round-robin; the place inside the partial walks `positions` = [(row in chunk: 0 first / -1 last, x)] starting at `shift`:
  lane 0, lane 63, the last (ragged) tile, the first and the last row of a chunk."""
  rng = np.random.default_rng(31 * m + nx + shift)
  t = IC.gridded(rng, (nlead, nrow, nx), -2, 2, dtype=np.float32).astype(dtype)
  shape = (m, nlead, nrow, nx) if layout == 'ifs' else (nlead, m, nrow, nx)
  base = np.empty(shape, dtype)
  p = np.transpose(base, (1, 0, 2, 3)) if layout == 'ifs' else base
  p[...] = t[:, None]
  if positions is None:
    positions = [(0, 0), (-1, min(63, nx - 1)), (-1, nx - 1), (0, nx - 1), (-1, 0), (0, min(64, nx - 1))]
  nchunk = -(-nrow // depth_chunk)
  live, k = [], 0
  for q in range(0, nlead * nchunk, 2):
    lead, chunk = divmod(q, nchunk)
    r0, r1 = chunk * depth_chunk, min((chunk + 1) * depth_chunk, nrow)
    where, x = positions[(k + shift) % len(positions)]
    row = r0 if where == 0 else r1 - 1
    name, members, target = kinds[k % len(kinds)]
    p[lead, :, row, x] = members.astype(dtype)
    t[lead, row, x] = target
    live.append((lead, row, x, name))
    k += 1
  return p, t, live


def finite_share(want, lanes=None):
  w = want if lanes is None else want[:, :, lanes]
  return float(np.isfinite(w).mean())
