"""Randomised checks of the fused ensemble score families -- energy score ('enrg'), variogram score ('vgrm'), Wasserstein distance
('wass'), ensemble RPS at number thresholds ('erps') -- through the public API against the float64 restatements of the case modules:
random dim orders, the member dim anywhere, targets in another order (or lacking a dim), random reduce sets, vector weights,
boolean bins, NaNs, masks and skipna.  What is under test is the code between the public statistic and the kernel: the gates of
metrics/multivariate.py, the groups of lazy.py, lazy.payload_layout, engine.norm_run and the operands built from them, and the plan
that puts the frame onto (key, depth, x).

Expectation: the payloads transposed to the case modules' canonical order (p[M, frame..., L], t[frame..., L]), their per-point
values and per-point bounds, aggregated by oracle.wbx_oracle.aggregate under the same weights, bins, mask and skipna.

Tolerance on 'hip' (tests/test_gpu_variogram_api.py derives it): per output cell sum w (b_f + 2 b_64) over the cell's points --
b_f the case module's bound of the fused route in the payload's dtype, b_64 the same formula in float64, doubled --, plus
(N + 4) 2^-52 sum w |value| for the float64 summations, N the points per cell; NaN and +-inf of the same class at the same cells;
sum_weights at rtol 1e-12.  A case that `eligible` says keeps the host route (energy scores only) is held to the same bound with the
host route's own b_f, energy_cases.host_relative_bound: it adds the M norms in the payload's dtype, which the kernel does in float64.

The 'emulated' half never runs these kernels (tests/fake_device.py has no context of the library's): it takes the host route, on
float64 copies of the payloads, and checks this file's own bookkeeping on the CPU at 1e-12 of the cell's sum w |value| -- for the
RPS of sum w (the terms whose difference the value is: ens_rps_cases.term_magnitudes), since the host route forms the fair score as
a difference in floating point and a cell whose value is exactly 0 would allow it no rounding at all.  (The float64 host route
agrees with the restatements to a few 1e-15 on such frames; the float32 one is off by up to 1.2e-6 for the variogram score, which
is why this half does not use it.)

The route is asserted: `eligible` restates the documented gates of _fused_energy, _fused_variogram, _fused_wasserstein and
EnsembleRankedProbabilityScore._fused_per_variable, and on 'hip' a statistic is a lazy one of its family's kind, with a logged
launch, exactly when `eligible`.  test_most_seeds_are_eligible keeps the generator from drifting towards the host route.

More seeds for a soak run: WBX_FUZZ_SCALE=10 python -m pytest tests/test_fuzz_scores.py [-m gpu]"""
import os
import types

import numpy as np
import pytest

import energy_cases as GC
import ens_rps_cases as RC
import variogram_cases as VC
import wasserstein_cases as WC
from oracle import wbx_oracle as O
from test_fuzz import RandomBins
from test_fuzz import VectorWeighting
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import probabilistic

FUZZ_SCALE = int(os.environ.get('WBX_FUZZ_SCALE', '1'))
N_API, N_DEVICE = 40 * FUZZ_SCALE, 24 * FUZZ_SCALE
ELIGIBLE_FLOOR = 0.8

E = 'number'
FRAME_DIMS = ['init_time', 'lead_time', 'level', 'latitude', 'longitude']
FAMILIES = ('energy', 'variogram', 'wasserstein', 'rps')
KIND = {'energy': 'enrg', 'variogram': 'vgrm', 'wasserstein': 'wass', 'rps': 'erps'}
SEED_BASE = {'energy': 61000, 'variogram': 63000, 'wasserstein': 65000, 'rps': 67000}
# the smallest sizes that straddle the kernels' internal tilings, as the raw tests of each kernel list them
MEMBERS = {'energy': [2, 3, 5, 17, 51, 64], 'variogram': [1, 2, 5, 17, 64], 'wasserstein': [1, 2, 5, 8, 9, 50, 51, 64], 'rps': [2, 3, 9, 51]}
RUNS = {'energy': [1, 2, 5, 17, 37], 'variogram': [1, 2, 5, 17, 64]}
LAST_DIM = [1, 4, 63, 64, 65, 130]
MODES = ['plain', 'nan_plain', 'masked', 'skipna']
# elements of the larger payload: what keeps a case (float64 restatement and host route included) well under a second
MAX_ELEMENTS = 600_000


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def _glue(order, a, b, rng):
  """`order` with `b` moved next to `a`, on either side."""
  order = [d for d in order if d != b]
  order.insert(order.index(a) + int(rng.integers(0, 2)), b)
  return order


def draw_case(family, seed):
  """The frame, parameters and payloads of one seed (NumPy, C order, in the seed's dtype)."""
  rng = np.random.default_rng(SEED_BASE[family] + seed)
  c = types.SimpleNamespace(family=family, seed=seed)
  ndim = int(rng.integers(2, 5))
  two = family == 'energy' and rng.random() < 0.3  # the norm over two frame dims
  # two norm dims are one run of an input only where it stores them next to each other: most such seeds are made so, in both inputs
  glue = two and rng.random() < 0.7
  if two:
    ndim = max(ndim, 3)
  dims = [str(d) for d in rng.permutation(FRAME_DIMS)[:ndim]]
  c.norm = ()
  if family in RUNS:
    # (two norm dims: neither is the last stored one, which stays a dim of the points)
    c.norm = tuple(str(d) for d in rng.permutation(dims[:-1] if two else dims)[:2 if two else 1])
  if glue:
    dims = _glue(dims, c.norm[0], c.norm[1], rng)
  sizes = {d: int(rng.integers(1, 6)) for d in dims}
  sizes[dims[-1]] = int(rng.choice(LAST_DIM))
  if c.norm:
    sizes[c.norm[0]] = int(rng.choice(RUNS[family]))
  c.m = int(rng.choice(MEMBERS[family]))
  c.n = int(rng.choice(MEMBERS[family])) if family == 'wasserstein' else None
  c.stat_dims = tuple(d for d in dims if d not in c.norm)
  # shrink the small dims -- never the member counts, the run or the last stored dim -- until the case is quick
  elements = lambda: max(c.m, c.n or 0) * int(np.prod([sizes[d] for d in dims], dtype=np.int64))
  small = [d for d in dims[:-1] if d not in c.norm[:1]]
  while elements() > MAX_ELEMENTS and any(sizes[d] > 1 for d in small):
    d = max(small, key=lambda d: sizes[d])
    sizes[d] -= 1
  # the predictions: the member dim anywhere (glued norm dims stay neighbours)
  places = [i for i in range(ndim + 1) if not (glue and 0 < i < ndim and {dims[i - 1], dims[i]} == set(c.norm))]
  c.pdims = list(dims)
  c.pdims.insert(int(rng.choice(places)), E)
  # the targets: another order; energy, variogram, RPS: sometimes without one of the dims that are no norm dim
  tdims = [str(d) for d in rng.permutation(dims)]
  if glue:
    tdims = _glue(tdims, c.norm[0], c.norm[1], rng)
  if family != 'wasserstein' and rng.random() < 0.25:
    tdims.remove(str(rng.choice(c.stat_dims)))
  if family == 'wasserstein':
    tdims.insert(int(rng.integers(0, ndim + 1)), E)
  c.tdims = tdims
  c.sizes = sizes
  psizes, tsizes = dict(sizes, **{E: c.m}), dict(sizes, **{E: c.n})
  c.dtype = np.float32 if rng.random() < 0.7 else np.float64
  # even seeds: multiples of 1/8 in [-8, 8] (ties between members, targets and thresholds); else N(0, 3), a quarter of all seeds at 280
  offset = 280.0 if seed % 4 == 1 else 0.0
  if seed % 2 == 0:
    values = lambda shape: rng.integers(-64, 65, size=shape) / 8.0
  else:
    values = lambda shape: rng.normal(size=shape) * 3.0 + offset
  pv = values([psizes[d] for d in c.pdims]).astype(c.dtype)
  tv = values([tsizes[d] for d in c.tdims]).astype(c.dtype)
  # family parameters
  if family == 'energy':
    c.fair = bool(rng.random() < 0.5)
  elif family == 'variogram':
    c.power = float(rng.choice([0.5, 1.0, 2.0]))
  elif family == 'rps':
    k = int(rng.choice([1, 4, 5, 16]))
    if seed % 2 == 0:
      thr = np.sort(rng.choice(np.arange(-48, 49), size=k, replace=False)) / 8.0  # on the values' grid: real ties
    else:
      thr = np.sort(rng.normal(size=k) * 3.0 + offset)
    assert np.all(np.diff(thr) > 0)
    c.thresholds = [float(v) for v in thr]
    c.fair, c.right = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
  # the aggregation: a reduce set over the statistic's dims, sometimes empty, sometimes without the last stored dim (x is kept)
  if rng.random() < 0.1:
    c.reduce = []
  else:
    c.reduce = [d for d in c.stat_dims if rng.random() < 0.7]
    if rng.random() < 0.3 and dims[-1] in c.reduce:
      c.reduce.remove(dims[-1])
  c.weights = [(d, rng.random(sizes[d]) + 0.5) for d in dims if rng.random() < 0.3]
  c.bins = None
  if rng.random() < 0.5:
    bd = [str(d) for d in rng.permutation(c.stat_dims)[:int(rng.integers(1, min(2, len(c.stat_dims)) + 1))]]
    c.bins = (bd, rng.random([int(rng.choice([2, 7]))] + [sizes[d] for d in bd]) > 0.4)
  draw_mode(c, rng, pv, tv, [d for d in c.tdims if d != E and d not in c.norm])  # never along the member dim or a norm dim
  c.pv, c.tv = pv, tv
  return c


def draw_mode(c, rng, pv, tv, own):
  """Draws c.mode and c.mask and puts the mode's NaNs into the payloads: one NaN each ('nan_plain'), a sprinkle ('skipna'), a mask
  over some of the targets' dims `own` with a NaN target under a masked-out point ('masked')."""
  c.mode = str(rng.choice(MODES))
  c.mask = None
  spot = lambda a: tuple(int(rng.integers(0, s)) for s in a.shape)
  if c.mode == 'nan_plain':
    tv[spot(tv)] = np.nan
    pv[spot(pv)] = np.nan
  elif c.mode == 'skipna':
    tv[rng.random(tv.shape) < 0.02] = np.nan
    pv[rng.random(pv.shape) < 0.01] = np.nan
  elif c.mode == 'masked':
    if not own:
      c.mode = 'plain'  # (targets of norm dims only: nothing to put a mask on)
    else:
      mdims = [d for d in own if rng.random() < 0.6] or own[:1]
      mask = rng.random([c.sizes[d] for d in mdims]) > 0.25
      c.mask = (tuple(mdims), mask)
      hidden = np.argwhere(~mask)
      if hidden.size:  # a NaN target under a masked-out point: it must leave no trace
        at = dict(zip(mdims, hidden[int(rng.integers(0, len(hidden)))]))
        tv[tuple(int(at[d]) if d in at else int(rng.integers(0, tv.shape[i])) for i, d in enumerate(c.tdims))] = np.nan


# ---- the gates, restated from their docstrings ----------------------------------------------------------------------------------------
def _one_run(stored, norm, sizes):
  """The norm dims are one strided run of an input stored densely in the order `stored`: without the dims of size 1, they are
  neighbours."""
  live = [d for d in stored if sizes[d] != 1]
  at = [live.index(d) for d in norm if d in live]
  return not at or max(at) - min(at) == len(at) - 1


def eligible(c, p_stored=None, t_stored=None):
  """Whether the statistics of the case are fused, from the documented gates alone.  `p_stored` / `t_stored`: the order the inputs
  are stored in (outermost first) where that is not their dim order -- dense device-resident views keep their strides."""
  p_stored, t_stored = p_stored or c.pdims, t_stored or c.tdims
  psizes, tsizes = dict(c.sizes, **{E: c.m}), dict(c.sizes, **{E: c.n})
  frame = set(c.pdims) - {E}
  mask_dims = set(c.mask[0]) if c.mask else set()
  if E in mask_dims:
    return False
  if c.family == 'wasserstein':
    return (1 <= c.m <= _hip.WASS_MAX_MEMBERS and 1 <= c.n <= _hip.WASS_MAX_MEMBERS and E in c.tdims and bool(frame)
            and frame == set(c.tdims) - {E})
  if E in c.tdims or not set(c.tdims) <= set(c.pdims):
    return False
  if c.family == 'rps':
    return c.m <= _hip.ERPS_MAX_MEMBERS and (c.m >= 2 or not c.fair) and 1 <= len(c.thresholds) <= _hip.ERPS_MAX_THRESHOLDS
  if mask_dims & set(c.norm) or not frame - set(c.norm) or any(d not in c.tdims for d in c.norm):
    return False
  if c.family == 'energy':
    if not 2 <= c.m <= _hip.ENRG_MAX_MEMBERS:
      return False
  else:
    run = int(np.prod([c.sizes[d] for d in c.norm]))
    if not (1 <= c.m <= _hip.VGRAM_MAX_MEMBERS and 1 <= run <= _hip.VGRAM_MAX_RUN and c.power in _hip.VGRAM_POWERS):
      return False
  if not (_one_run(p_stored, c.norm, psizes) and _one_run(t_stored, c.norm, tsizes)):
    return False
  # ... and the same run in both: element i of one is element i of the other only where both store the norm dims in one order
  walk = lambda stored: [d for d in stored if d in c.norm and c.sizes[d] != 1]
  return walk(p_stored) == walk(t_stored)


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def _canonical(c, pv, tv):
  """The payloads in the case modules' order: p[M, points..., L], t[points..., L] (Wasserstein: t[N, points...]; RPS: no L)."""
  full = c.stat_dims + c.norm
  shape = [c.sizes[d] for d in full]
  p = np.transpose(pv, [c.pdims.index(d) for d in (E,) + full])
  if c.family == 'wasserstein':
    return p, np.transpose(tv, [c.tdims.index(d) for d in (E,) + full])
  t = np.broadcast_to(O.expand_to(tv, tuple(c.tdims), full), shape)
  if c.norm:
    points = shape[:len(c.stat_dims)]
    p, t = p.reshape([c.m] + points + [-1]), t.reshape(points + [-1])
  return p, t


def expected_points(c, pv, tv, fused=True):
  """{statistic: (per-point values, b_f, b_64, carries the targets' mask, what the float64 host route is accurate relative to: the
  per-point |value| except for the RPS)} over c.stat_dims, from the case modules."""
  p, t = _canonical(c, pv, tv)
  if c.family == 'energy':
    stat = GC.energy_points(p, t, c.fair)
    l = p.shape[-1]
    mag = np.where(np.isfinite(stat), np.abs(stat), 0.0)
    b_f = (GC.relative_bound if fused else GC.host_relative_bound)(c.m, l, pv.dtype) * mag
    b_64 = GC.relative_bound(c.m, l, np.float64) * mag
    # the spread is a statistic of the predictions alone: the targets' mask does not reach it (tests/test_fuzz.py, the CRPS spread)
    return {'skill': (stat[..., 0], b_f[..., 0], b_64[..., 0], True, mag[..., 0]),
            'spread': (stat[..., 1], b_f[..., 1], b_64[..., 1], False, mag[..., 1])}
  if c.family == 'variogram':
    stat, b_f = VC.variogram_points(p, t, c.power, pv.dtype)
    return {'vs': (stat, b_f, VC.variogram_points(p, t, c.power, np.float64)[1], True, np.abs(stat))}
  if c.family == 'wasserstein':
    stat, bound = WC.wasserstein_points(p, t)  # (everything after the exact sort is float64, whatever the launch dtype)
    return {'w1': (stat, bound, bound, True, np.abs(stat))}
  stat = RC.rps_points(p, t, c.thresholds, c.thresholds, c.fair, c.right)
  # the fair score is a difference of like-sized terms, which the host route forms in floating point: on the CPU half its 1e-12 is
  # of the terms, not of the difference (as for the unbiased ensemble-mean squared error in tests/test_fuzz.py)
  terms = RC.term_magnitudes(p, t, c.thresholds, c.thresholds, c.fair, c.right)
  return {'rps': (stat, np.zeros(stat.shape), RC.point_bound(stat), True, terms)}


def statistics(c):
  dim = list(c.norm) if len(c.norm) > 1 else (c.norm[0] if c.norm else None)
  if c.family == 'energy':  # both in one evaluation: they share a group
    return {'skill': probabilistic.EnergyScoreSkill(dim, E), 'spread': probabilistic.EnergyScoreSpread(dim, E, fair=c.fair)}
  if c.family == 'variogram':
    return {'vs': probabilistic.VariogramScore(dim, E, c.power)}
  if c.family == 'wasserstein':
    return {'w1': probabilistic.WassersteinDistance(E)}
  return {'rps': probabilistic.EnsembleRankedProbabilityScore(c.thresholds, c.thresholds, 'bin', 'fuzz', ensemble_dim=E, fair=c.fair,
                                                              right_inclusive=c.right)}


def aggregator(c):
  weights = [VectorWeighting(d, v) for d, v in c.weights]
  bins = [RandomBins('bin0', c.bins[0], c.bins[1])] if c.bins else None
  return aggregation.Aggregator(reduce_dims=c.reduce, weigh_by=weights or None, bin_by=bins, masked=c.mode == 'masked',
                                skipna=c.mode == 'skipna')


def _is_fused(c, stat):
  return isinstance(stat, lazy.LazyStatistic) and stat._group.kind == KIND[c.family]  # pylint: disable=protected-access


def evaluate(c, p_data, t_data, on_device):
  """-> (state, every statistic is fused / none is, the family's launches logged (None off the device))."""
  p = xr.DataArray(p_data, dims=c.pdims)
  t = xr.DataArray(t_data, dims=c.tdims)
  if c.mask:
    t.coords['mask'] = xr.DataArray(c.mask[1], dims=c.mask[0])
  computed = {k: s.compute({'v': p}, {'v': t}) for k, s in statistics(c).items()}
  fused = {_is_fused(c, per_var['v']) for per_var in computed.values()}
  assert len(fused) == 1, (c.family, c.seed, 'some statistics of one group are fused and some are not')
  state = aggregator(c).aggregate_statistics(computed)
  launches = [e for e in engine.S1_EVENT_LOG if e['kind'] == KIND[c.family]] if on_device else None
  return state, fused.pop(), launches


def check_against_the_restatement(c, state, pv, tv, emulated, fused=True):
  """Every statistic's sums and weights against the aggregated per-point values -> the worst error / bound.  `fused`: the route the
  sums came by (asserted by the caller), whose bound b_f is."""
  # weights on dims the statistic does not have (the norm dims) are 1 (VectorWeighting)
  ow = [(v, (d,)) for d, v in c.weights if d in c.stat_dims]
  ob = [('bin0', c.bins[1], ('bin0',) + tuple(c.bins[0]))] if c.bins else []
  worst = 0.0
  for name, (stat, b_f, b_64, masked, host_mag) in expected_points(c, pv, tv, fused).items():
    mkw = dict(mask=c.mask[1], mask_dims=c.mask[0]) if (c.mode == 'masked' and masked) else {}
    agg = lambda a, **kw: O.aggregate(a, c.stat_dims, c.reduce, weights=ow, bin_masks=ob, **mkw, **kw)
    got_s, got_w = state.sum_weighted_statistics[name].get('v'), state.sum_weights[name].get('v')
    worst = max(worst, check_cells((c.family, c.seed, name), got_s, got_w, agg, stat, b_f, b_64, host_mag, c.reduce, c.sizes,
                                   c.mode == 'skipna', emulated))
  return worst


def check_cells(tag, got_s, got_w, agg, stat, b_f, b_64, host_mag, reduce, sizes, skipna, emulated, host_own=None):
  """One statistic's sums and weights against its per-point values `stat` aggregated by `agg` (O.aggregate under the case's weights,
  bins and mask; the dims of `stat` may include lane dims: ordinary dims there) -> the worst error / bound.  `host_own`: a per-point
  bound that the emulated half grants on top of its 1e-12 (arithmetic that the host route does in float32 whatever the payload)."""
  n = int(np.prod([sizes[d] for d in reduce]))
  sws, sw, out_dims = agg(stat, skipna=skipna)
  finite = np.isfinite(stat)
  own = agg(np.where(finite, b_f + 2.0 * b_64, 0.0))[0]
  mag = agg(np.where(finite, np.abs(stat), 0.0))[0]
  bound = 1e-12 * agg(np.where(finite, host_mag, 0.0))[0] if emulated else own + (n + 4) * 2.0 ** -52 * mag
  if emulated and host_own is not None:
    bound = bound + agg(np.where(finite, host_own, 0.0))[0]
  assert got_s is not None and set(got_s.dims) == set(out_dims), (tag, got_s if got_s is None else got_s.dims, out_dims)
  got = np.asarray(got_s.transpose(*out_dims).values, np.float64)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(sws), err_msg=f'{tag}: NaN cells')
  inf = np.isinf(sws)
  np.testing.assert_array_equal(got[inf], sws[inf], err_msg=f'{tag}: infinite cells')
  fin = np.isfinite(sws)
  err = np.abs(got[fin] - sws[fin])
  with np.errstate(all='ignore'):
    ratio = float(np.where(err > 0, err / bound[fin], 0.0).max()) if err.size else 0.0
  assert (err <= bound[fin]).all(), (tag, 'worst error / bound', ratio, 'largest error', float(err.max()))
  np.testing.assert_allclose(np.asarray(got_w.transpose(*out_dims).values), sw, rtol=1e-12, atol=0, err_msg=f'{tag}: weights')
  return ratio


def run_host_arrays(c, backend, monkeypatch):
  if backend == 'emulated':
    # float64 copies of the same numbers: the host route in float64, whatever dtype the seed drew
    pv, tv = c.pv.astype(np.float64), c.tv.astype(np.float64)
    state, fused, _ = evaluate(c, pv, tv, on_device=False)
    assert not fused, (c.family, c.seed, 'a fused statistic without a device')
  else:
    pv, tv = c.pv, c.tv
    monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
    state, fused, launches = evaluate(c, pv, tv, on_device=True)
    want = eligible(c)
    assert fused == want, (c.family, c.seed, 'fused' if fused else 'host route', 'eligible' if want else 'not eligible', c.pdims, c.tdims, c.norm)
    assert bool(launches) == want, (c.family, c.seed, launches)
  worst = check_against_the_restatement(c, state, pv, tv, backend == 'emulated', fused)
  print(f'fuzz_scores {c.family} {backend} seed {c.seed} route {"fused" if fused else "host"} worst_error_over_bound {worst:.3g}')


# ---- 1. random frames through the public API --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(N_API))
def test_random_energy_score_frames(backend, monkeypatch, seed):
  """EnergyScoreSkill + EnergyScoreSpread (fair or not) in one evaluation: 2-64 members, a norm run of 1-37 elements along one frame
  dim -- on 30 % of the seeds along two, which are one strided run of an input or not."""
  run_host_arrays(draw_case('energy', seed), backend, monkeypatch)


@pytest.mark.parametrize('seed', range(N_API))
def test_random_variogram_score_frames(backend, monkeypatch, seed):
  """VariogramScore at p = 0.5, 1, 2: 1-64 members, 1-64 elements along its dim, stored anywhere."""
  run_host_arrays(draw_case('variogram', seed), backend, monkeypatch)


@pytest.mark.parametrize('seed', range(N_API))
def test_random_wasserstein_distance_frames(backend, monkeypatch, seed):
  """WassersteinDistance: 1-64 members a side, each side with its own count and its own place for the member dim."""
  run_host_arrays(draw_case('wasserstein', seed), backend, monkeypatch)


@pytest.mark.parametrize('seed', range(N_API))
def test_random_ensemble_rps_frames(backend, monkeypatch, seed):
  """EnsembleRankedProbabilityScore at 1-16 strictly increasing number thresholds that cut through the values, fair or not, either
  inclusiveness, 2-51 members."""
  run_host_arrays(draw_case('rps', seed), backend, monkeypatch)


# ---- 2. the floor on how often the route is the fused one ---------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
def test_most_seeds_are_eligible(family):
  """A condition on the generator, no measurement: at least 80 % of a family's seeds must be frames the gates let through, or
  the tests above quietly turn into tests of the host route."""
  share = float(np.mean([eligible(draw_case(family, seed)) for seed in range(N_API)]))
  assert share >= ELIGIBLE_FLOOR, (family, share)


# ---- 3. device-resident payloads with the strides they come with ----------------------------------------------------------------------------
def _physical_orders(c, seed, families=FAMILIES, base=69000):
  """-> (the order the predictions are stored in, the targets', whether the views start one element into their allocations, the
  frame dim along which they are every other element of an allocation twice as long, or None).  `families`: the families the
  caller rotates over with the seed; `base`: its own stream of random numbers."""
  rng = np.random.default_rng(base + seed)
  p_stored = [str(d) for d in rng.permutation(c.pdims)]
  t_stored = [str(d) for d in rng.permutation(c.tdims)]
  turn = seed // len(families)  # (the family rotates with the seed: a third and a quarter of every family's seeds)
  offset = turn % 3 == 0
  sliced = str(rng.choice([d for d in c.pdims if d != E])) if turn % 4 == seed % len(families) % 4 else None
  return p_stored, t_stored, offset, sliced


def _device_view(values, dims, stored, offset, sliced):
  """`values` (axes named `dims`) as a view with those axes of a device tensor stored in the order `stored`."""
  import torch  # pylint: disable=g-import-not-at-top
  physical = np.ascontiguousarray(np.transpose(values, [dims.index(d) for d in stored]))
  shape = list(physical.shape)
  index = [slice(None)] * len(shape)
  if sliced in stored:
    shape[stored.index(sliced)] *= 2
    index[stored.index(sliced)] = slice(None, None, 2)
  count = int(np.prod(shape))
  # (the allocation is filled with NaN: an element of it that is not the view's and reaches a sum shows)
  buf = torch.full((count + int(offset),), float('nan'), dtype=torch.from_numpy(physical).dtype, device='cuda')
  view = buf[int(offset):].view(shape)[tuple(index)]
  view.copy_(torch.from_numpy(physical))
  torch.cuda.synchronize()
  assert tuple(view.shape) == physical.shape
  return view.permute([stored.index(d) for d in dims])


@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(N_DEVICE))
def test_device_resident_views_keep_their_strides(monkeypatch, seed):
  """The frames of the tests above as torch views of device memory stored in a random order of their own: the member, norm and x
  strides are whatever the view has (lazy.payload_layout reads them from the tensor).  A third start one element into their
  allocation; a quarter are every other element along one frame dim of an allocation twice as long -- not dense: the engine may
  fuse or copy, only the values are asserted."""
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  engine.clear_caches()
  family = FAMILIES[seed % len(FAMILIES)]
  c = draw_case(family, seed)
  p_stored, t_stored, offset, sliced = _physical_orders(c, seed)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  p_view = _device_view(c.pv, c.pdims, p_stored, offset, sliced)
  t_view = _device_view(c.tv, c.tdims, t_stored, offset, sliced)
  np.testing.assert_array_equal(p_view.cpu().numpy(), c.pv)
  state, fused, launches = evaluate(c, p_view, t_view, on_device=True)
  if sliced is None:
    want = eligible(c, p_stored, t_stored)
    assert fused == want, (family, seed, 'fused' if fused else 'host route', 'eligible' if want else 'not eligible', p_stored, t_stored, c.norm)
    assert bool(launches) == want, (family, seed, launches)
  worst = check_against_the_restatement(c, state, c.pv, c.tv, emulated=False, fused=fused)
  engine.clear_caches()
  print(f'fuzz_scores {family} device seed {seed} route {"fused" if fused else "host"}{"" if sliced is None else " (not dense)"} '
        f'worst_error_over_bound {worst:.3g}')


# ---- pinned frames: what the random frames above have found, kept whatever becomes of the generator -------------------------------------
def _pinned_energy_case(pdims, tdims, sizes, m, norm, reduce):
  """An energy score case that is written out: float32 multiples of 1/8, fair, no weights, bins, NaNs or mask."""
  rng = np.random.default_rng(71000)
  c = types.SimpleNamespace(family='energy', seed='pinned', pdims=list(pdims), tdims=list(tdims), sizes=dict(sizes), m=m, n=None, norm=tuple(norm),
                            dtype=np.float32, fair=True, reduce=list(reduce), weights=[], bins=None, mode='plain', mask=None)
  c.stat_dims = tuple(d for d in pdims if d != E and d not in norm)
  psizes = dict(sizes, **{E: m})
  c.pv = (rng.integers(-64, 65, size=[psizes[d] for d in pdims]) / 8.0).astype(np.float32)
  c.tv = (rng.integers(-64, 65, size=[sizes[d] for d in tdims]) / 8.0).astype(np.float32)
  return c


# energy seeds 1 and 17: either input stores its two norm dims as one strided run, but in the other order.  The launch paired
# element i of the predictions' run with element i of the targets', another element of the vector: the skill was off by 3.3 (seed 1)
# and 0.38 (seed 17), 37000 and 860 times the bound; the spread, of the predictions alone, was right.  Such frames keep the host route.
PINNED_ENERGY = {
    'seed 1: (init_time, level) against (level, init_time)': (
        dict(pdims=(E, 'init_time', 'level', 'latitude'), tdims=('level', 'init_time'), sizes={'init_time': 17, 'level': 2, 'latitude': 4}, m=5,
             norm=('init_time', 'level'), reduce=['latitude']), False),
    'seed 17: (latitude, lead_time) against (lead_time, latitude), members innermost': (
        dict(pdims=('latitude', 'lead_time', 'init_time', E), tdims=('lead_time', 'latitude', 'init_time'),
             sizes={'latitude': 17, 'lead_time': 5, 'init_time': 4}, m=64, norm=('latitude', 'lead_time'), reduce=['init_time']), False),
    # their neighbours that are the same run in both inputs, and fused: the norm dims named in either order
    'seed 1 with the targets in the order of the predictions': (
        dict(pdims=(E, 'init_time', 'level', 'latitude'), tdims=('init_time', 'level'), sizes={'init_time': 17, 'level': 2, 'latitude': 4}, m=5,
             norm=('level', 'init_time'), reduce=['latitude']), True),
    'seed 17 with the targets in the order of the predictions': (
        dict(pdims=('latitude', 'lead_time', 'init_time', E), tdims=('init_time', 'latitude', 'lead_time'),
             sizes={'latitude': 17, 'lead_time': 5, 'init_time': 4}, m=64, norm=('latitude', 'lead_time'), reduce=['init_time']), True),
    # a dim of one element is walked by nobody: it cannot put two runs out of order
    'a second norm dim of one element, stored on the other side': (
        dict(pdims=(E, 'init_time', 'level', 'latitude'), tdims=('level', 'init_time'), sizes={'init_time': 17, 'level': 1, 'latitude': 4}, m=5,
             norm=('init_time', 'level'), reduce=['latitude']), True),
}


@pytest.mark.parametrize('which', list(PINNED_ENERGY))
def test_pinned_energy_frames(backend, monkeypatch, which):
  spec, fused = PINNED_ENERGY[which]
  c = _pinned_energy_case(**spec)
  assert eligible(c) == fused, which
  run_host_arrays(c, backend, monkeypatch)


def test_norm_run_order_tells_runs_that_pair_other_elements_apart():
  from weatherbenchx_amd import planner  # pylint: disable=g-import-not-at-top
  sizes = {'a': 17, 'b': 2, 'c': 1}
  ab = planner.InputLayout(strides={'a': 2, 'b': 1, 'c': 1}, itemsize=4)
  ba = planner.InputLayout(strides={'a': 1, 'b': 17, 'c': 34}, itemsize=4)
  assert engine.norm_run(ab, ('a', 'b'), sizes) == (34, 1) == engine.norm_run(ba, ('a', 'b'), sizes)  # one run each ...
  assert engine.norm_run_order(ab, ('a', 'b'), sizes) == ('b', 'a') == engine.norm_run_order(ab, ('b', 'a'), sizes)
  assert engine.norm_run_order(ba, ('a', 'b'), sizes) == ('a', 'b')                                   # ... walked otherwise
  assert engine.norm_run_order(ab, ('a', 'c'), sizes) == ('a',) == engine.norm_run_order(ba, ('c', 'a'), sizes)
