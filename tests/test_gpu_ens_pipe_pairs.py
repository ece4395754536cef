"""ens_pipe_kernel's paired blocks: in a launch whose every (key, chunk) is ONE row of 64 q + 32 points, the rows IN FRONT OF THE
LAST TWO ROUNDS of resident waves go two to a block -- row A's last 32 points and row B's first 32 share the junction tile,
row B then runs from its point 32 -- and every (key, chunk) must get the very bits the one-index block writes
(csrc/wbx_ens_impl.hpp: launch_ens_pipe decides; the rule is restated in `_npair`).  A plan with ONE (key, chunk) is never
paired, so a row launched alone is the reference for "the one-index block": partials are compared with it through view(int64).

Launches long enough to pair (more than 2 x 12 x CUs rows: 6144 on an MI355X) are built without the memory: `lead_time` is
a broadcast (stride 0) dim over a unit of FIVE distinct rows, the (key, chunk) index is lead * 5 + row, so pair j holds rows
(2 j % 5, (2 j + 1) % 5) -- every row is an A and a B somewhere, next to each of its neighbours, also across the key
boundary -- and every lead's partials equal the five rows launched alone.

  * bit identity on ordinary data, M = 51 / 50 (fp32 chains) and 4 (fp64 sums of a padded bucket), nx = 96, 32 (the junction is
    the whole row), 1440 and strided x; the short launches of the same shapes (2, 3, 5 keys: not paired) likewise;
  * NaN / infinite members, a NaN target and a point outside the fp32 thresholds (the fp64 escape, decided per HALF of the
    junction tile) at a row's last point (junction lane 31 where the row is an A, the last lane of the block where it is a B)
    and at its first (junction lane 32 where it is a B): that row is held against the float64 oracle, every other row stays
    bit-identical to its stand-alone launch;
  * launches the rule leaves alone (nx = 64, nx = 100, two rows per chunk, FLAT planes) against the oracle at the bounds of
    tests/ensemble_cases.py, and the launch the engine logs: grid = nkey * nchunk, block = 64;
  * all five lanes of every row at nx = 96, M = 51 against the oracle at the per-point bounds, paired."""
import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import probabilistic
from oracle import wbx_oracle as O
import ensemble_cases as EC
import test_gpu_ensemble_points as EP

pytestmark = pytest.mark.gpu
NL = EC.NLANE
UNIT = 5  # distinct rows of a long launch (odd: every row meets both places of a pair)


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def _tail(ctx):
  """The rows that keep a block each: two rounds of the resident waves, 3 per SIMD, 4 SIMDs per CU (launch_ens_pipe)."""
  return 2 * int(ctx.device_name().rsplit('cus=', 1)[1]) * 4 * 3


def _npair(ctx, plan):
  """launch_ens_pipe's rule, restated (the plan already runs the 'pipe' route): how many blocks own two (key, chunk) indices."""
  one_row = (plan.ndepth == 1 and plan.nchunk == 1) or (plan.depth_chunk == 1 and plan.nchunk == plan.ndepth)
  total = plan.nkey * plan.nchunk
  if plan.x_weights is not None or not one_row or plan.nx % 64 != 32 or total <= _tail(ctx):
    return 0
  return (total - _tail(ctx)) // 2


def _launch(ctx, p, t, fair, dc=1):
  """-> (plan, got[lead][chunk][lane]) of one wbx_ens_partial launch with one-wave blocks on the pipelined sweep."""
  plan, dplan, mstride = EP._plans(ctx, p, t, False, dc, EP._flags('plain', fair), block=64)  # pylint: disable=protected-access
  assert EP._route(plan, p.shape[1], np.float32, EC.SORT) == 'pipe', plan  # pylint: disable=protected-access
  got = EP._run_partial(ctx, p, t, None, plan, dplan, mstride, EC.SORT, sentinel=-77.0)  # pylint: disable=protected-access
  assert got.shape == (p.shape[0], plan.nchunk, NL, 1)
  return plan, got[..., 0]


def _alone(ctx, p, t, lead, row, fair):
  """Row (lead, row) as a plan of its own: one (key, chunk), the one-index block -> its five lanes."""
  ps, ts = p[lead:lead + 1, :, row:row + 1].copy(), t[lead:lead + 1, row:row + 1].copy()
  plan, got = _launch(ctx, ps, ts, fair)
  assert plan.nkey * plan.nchunk == 1 and _npair(ctx, plan) == 0
  return got[0, 0]


def _bits(a):
  return np.ascontiguousarray(a, np.float64).view(np.int64)


def _against_oracle(got, plan, p, t, fair, what):
  fam = EC.family('pipe', p.shape[1], np.float32)
  stat = EC.expected_lanes(fam, p, t, fair)
  return EP._check_partials(got[..., None], plan, stat, EC.lane_bounds(fam, p, t, stat), None, what)  # pylint: disable=protected-access


def _strided(a, xs):
  return a if xs == 1 else a[..., ::xs]


def _long_launch(ctx, p, t, fair):
  """p[1, member, UNIT, x], t[1, UNIT, x] repeated along a stride-0 lead dim until the launch is the tail and 64 units more
  -> (plan, got[lead][row][lane], pairs).  Asserts that the launch pairs and that every row is an A and a B of some pair."""
  assert p.shape[0] == 1 and p.shape[2] == UNIT
  nlead = -(-_tail(ctx) // UNIT) + 64
  pb, tb = np.broadcast_to(p, (nlead,) + p.shape[1:]), np.broadcast_to(t, (nlead,) + t.shape[1:])
  plan, got = _launch(ctx, pb, tb, fair)
  npair = _npair(ctx, plan)
  assert plan.nkey * plan.nchunk == nlead * UNIT and npair >= 32 * UNIT
  assert (got != -77.0).all()
  for row in range(UNIT):
    places = {i % 2 for i in range(2 * npair) if i % UNIT == row}
    assert places == {0, 1}, (row, places)
  return plan, got, npair


def _unit_case(seed, m, nx, layout='member_outside', xs=1):
  p, t, _ = EC.dense_case(seed, m, 1, UNIT, nx * xs, values='anomaly', layout=layout)
  return _strided(p, xs), _strided(t, xs)


# (nx, member layout, x stride)
LONG_CASES = [(96, 'member_outside', 1), (96, 'ifs', 1), (32, 'member_outside', 1), (1440, 'ifs', 1), (96, 'member_outside', 2)]


@pytest.mark.parametrize('nx,layout,xs', LONG_CASES, ids=[f'nx{c[0]}-{c[1]}-xs{c[2]}' for c in LONG_CASES])
@pytest.mark.parametrize('m', [51, 50, 4])
def test_paired_rows_are_bit_identical_to_rows_launched_alone(ctx, m, nx, layout, xs):
  """Every partial of the long launch -- rows in pairs in front, one per block in the tail -- equals, bit for bit, its row
  launched alone; the five rows launched alone hold the oracle's bounds."""
  fair = EC.fair_of(m, nx)
  p, t = _unit_case(7 * m + nx, m, nx, layout, xs)
  plan, got, _ = _long_launch(ctx, p, t, fair)
  assert plan.xstride[0] == xs
  alone = np.stack([_alone(ctx, p, t, 0, row, fair) for row in range(UNIT)])
  assert np.isfinite(alone).all()
  same = _bits(got) == _bits(alone)[None]
  assert same.all(), (f'M={m} nx={nx} xs={xs}', 'first (lead, row, lane) that differs', tuple(np.argwhere(~same)[0]))
  plan1, got1 = _launch(ctx, p, t, fair)
  assert (_bits(got1[0]) == _bits(alone)).all()
  _against_oracle(got1, plan1, p, t, fair, f'M={m} nx={nx} xs={xs}')


# (nx, leads = keys, rows = chunks of one row, layout)
SHORT_CASES = [(96, 2, 1, 'member_outside'), (96, 3, 1, 'ifs'), (96, 5, 1, 'member_outside'), (96, 2, 3, 'ifs'), (32, 5, 1, 'member_outside'),
               (1440, 4, 1, 'ifs')]


@pytest.mark.parametrize('nx,nlead,nrow,layout', SHORT_CASES, ids=[f'nx{c[0]}-{c[1]}keys-{c[2]}rows' for c in SHORT_CASES])
@pytest.mark.parametrize('m', [51, 50, 4])
def test_short_launches_of_the_same_shapes_match_rows_launched_alone(ctx, m, nx, nlead, nrow, layout):
  """Two, three and five keys of one row, two keys of three rows: shorter than the tail, so every row keeps a block of its own --
  and writes what it writes alone."""
  fair = EC.fair_of(m, nx)
  p, t, _ = EC.dense_case(7 * m + nx + nlead, m, nlead, nrow, nx, values='anomaly', layout=layout)
  plan, got = _launch(ctx, p, t, fair)
  assert _npair(ctx, plan) == 0 and plan.nkey * plan.nchunk == nlead * nrow
  assert np.isfinite(got).all()
  for lead in range(nlead):
    for row in range(nrow):
      want = _alone(ctx, p, t, lead, row, fair)
      assert (_bits(got[lead, row]) == _bits(want)).all(), (m, nx, lead, row, got[lead, row], want)
  _against_oracle(got, plan, p, t, fair, f'short M={m} nx={nx} keys={nlead} rows={nrow}')


EDGE_KINDS = ('nan_member', 'pinf_member', 'big_2^101', 'range_2^-51', 'nan_target')


@pytest.mark.parametrize('where', ['last-point', 'first-point'])
@pytest.mark.parametrize('m', [51, 50])
def test_a_special_point_at_the_junction_stays_in_its_own_row(ctx, m, where):
  """The special point sits in row 2 of the unit of five rows of 96, at the row's last point -- lane 31 of the junction tile in
  the pairs whose A is row 2, lane 63 of the block's last tile in the pairs whose B it is -- or at its first point: lane 32 of
  the junction where row 2 is a B.  A NaN / infinite member turns its own row's five lanes NaN; a point outside the fp32
  thresholds sends its half of the junction tile (its whole tile elsewhere) through the fp64 operator: every variant of that
  row is held against the oracle at its bounds; a NaN target reaches the lanes that look at the target.  Every OTHER row -- its
  neighbour in the same block above all -- is bit-identical to its stand-alone launch in every block of the launch."""
  kinds = {k[0]: k for k in EC.live_points(m)}
  nx, row = 96, 2
  x = nx - 1 if where == 'last-point' else 0
  for i, kind in enumerate(EDGE_KINDS):
    fair = EC.fair_of(m, i)
    p, t = _unit_case(11 * m + i, m, nx)
    p[0, :, row, x], t[0, row, x] = kinds[kind][1], kinds[kind][2]
    plan, got, _ = _long_launch(ctx, p, t, fair)
    what = f'M={m} {kind} at the {where} of row {row}'
    others = [r for r in range(UNIT) if r != row]
    alone = np.stack([_alone(ctx, p, t, 0, r, fair) for r in range(UNIT)])
    assert np.isfinite(alone[others]).all(), what
    same = _bits(got[:, others]) == _bits(alone[others])[None]
    assert same.all(), (what, 'first (lead, row, lane) that differs', tuple(np.argwhere(~same)[0]))
    # the row that holds the point: every variant the launch wrote (as an A, as a B, alone in the tail) against the oracle
    plan1, _ = _launch(ctx, p, t, fair)
    variants = np.unique(_bits(got[:, row]), axis=0).view(np.float64)
    assert 1 <= len(variants) <= 3, (what, variants)
    for v in variants:
      unit = alone.copy()
      unit[row] = v
      _against_oracle(unit[None], plan1, p, t, fair, what)
      if kind in ('nan_member', 'pinf_member'):
        assert np.isnan(v).all(), what
      elif kind == 'nan_target':
        assert np.isnan(v[[0, 3, 4]]).all() and np.isfinite(v[[1, 2]]).all(), what
      else:
        assert np.isfinite(v).all(), what


def test_launches_the_pair_rule_leaves_alone(ctx):
  """nx = 64 and nx = 100 (no half tile of 32), two rows per chunk (dchunk = 2) at nx = 96, and the FLAT flavour over planes of
  three rows of 96: none is paired, all against the oracle at the bounds of ensemble_cases.  (The strided paired launch is held
  by the bit-identity cases.)"""
  m = 51
  fam = EC.family('pipe', m, np.float32)
  for i, (nx, nrow, dc) in enumerate(((64, 3, 1), (100, 3, 1), (96, 4, 2))):
    fair = EC.fair_of(m, i)
    p, t, _ = EC.dense_case(900 + i, m, 3, nrow, nx, values='anomaly', layout='ifs' if i & 1 else 'member_outside')
    plan, got = _launch(ctx, p, t, fair, dc=dc)
    assert _npair(ctx, plan) == 0 and plan.depth_chunk == dc
    _against_oracle(got, plan, p, t, fair, f'unpaired nx={nx} rows/chunk={dc}')
  # the same three geometries long enough to pair if the rule let them: every partial equals the unit's
  for i, (nx, dc) in enumerate(((64, 1), (100, 1), (96, 2))):
    nrow = UNIT * dc
    p, t, _ = EC.dense_case(920 + i, m, 1, nrow, nx, values='anomaly')
    nlead = -(-_tail(ctx) // UNIT) + 64
    plan, got = _launch(ctx, np.broadcast_to(p, (nlead,) + p.shape[1:]), np.broadcast_to(t, (nlead,) + t.shape[1:]), True, dc=dc)
    assert _npair(ctx, plan) == 0 and plan.nkey * plan.nchunk == nlead * UNIT > _tail(ctx)
    plan1, got1 = _launch(ctx, p, t, True, dc=dc)
    assert (_bits(got) == _bits(got1)).all(), (nx, dc)
    _against_oracle(got1, plan1, p, t, True, f'long unpaired nx={nx} rows/chunk={dc}')
  nx, nrow, R = 96, 6, 3
  p, t, _ = EC.dense_case(950, m, 2, nrow, nx, values='anomaly')
  w = EP._flat_weights(nx, m)  # pylint: disable=protected-access
  plan, dplan, mstride = EP._plans(ctx, p, t, False, 2, EP._flags('plain', True), block=64, flat=(R, w))  # pylint: disable=protected-access
  assert EP._route(plan, m, np.float32, EC.SORT) == 'flat' and _npair(ctx, plan) == 0  # pylint: disable=protected-access
  got = EP._run_partial(ctx, p, t, None, plan, dplan, mstride, EC.SORT, sentinel=-77.0)  # pylint: disable=protected-access
  stat = EC.expected_lanes(fam, p, t, True)
  EP._check_partials(got, plan, stat, EC.lane_bounds(fam, p, t, stat), None, 'flat nx=96 R=3', weights=w)  # pylint: disable=protected-access


@pytest.mark.parametrize('nlon', [96, 64, 100])
def test_the_engine_logs_the_plan_grid_and_one_wave_blocks(ctx, nlon):
  """Through the Aggregator (reduce longitude only: one partial per latitude row), five rows of `nlon` points, M = 51: the
  logged launch is the plan's -- grid = nkey * nchunk = 5, block = 64 -- whatever the library does with the rows, and every
  row's mean of three lanes matches the float64 oracle to 1e-6 (the fp32 chains' 9 x 2^-24 per point)."""
  nlat, m = UNIT, 51
  rng = np.random.default_rng(nlon)
  tv = (rng.normal(size=(nlat, nlon)) + 280).astype(np.float32)
  pv = (tv[None] + rng.normal(size=(m, nlat, nlon))).astype(np.float32)
  tv = (tv + rng.normal(size=(nlat, nlon))).astype(np.float32)
  coords = {'latitude': np.linspace(-60, 60, nlat), 'longitude': np.arange(nlon) * (360.0 / nlon)}
  pd, td = ('number', 'latitude', 'longitude'), ('latitude', 'longitude')
  stats = {'CRPSSkill': probabilistic.CRPSSkill(), 'CRPSSpread': probabilistic.CRPSSpread(use_sort=True),
           'EnsembleVariance': probabilistic.EnsembleVariance()}
  agg = aggregation.Aggregator(reduce_dims=['longitude'])
  engine.S1_EVENT_LOG = []
  try:
    state = agg.aggregate_statistics(metrics_base.compute_unique_statistics_for_all_metrics(
        stats, {'v': xr.DataArray(pv, dims=pd, coords=coords)}, {'v': xr.DataArray(tv, dims=td, coords=coords)}))
    means = state.mean_statistics()
    log = [e for e in engine.S1_EVENT_LOG if e['kind'] == 'ens']
  finally:
    engine.S1_EVENT_LOG = None
  assert len(log) == 1 and log[0]['grid'] == nlat and log[0]['block'] == 64, log
  want = {'CRPSSkill': O.crps_skill(pv, pd, tv, td, 'number')[0], 'CRPSSpread': O.crps_spread(pv, pd, 'number', fair=True, use_sort=True)[0],
          'EnsembleVariance': O.ensemble_variance(pv, pd, 'number')[0]}
  for name, lane in want.items():
    got = np.asarray(means[stats[name].unique_name]['v'].values)
    np.testing.assert_allclose(got, lane.mean(axis=-1), rtol=1e-6, err_msg=f'nlon={nlon} {name}')


def test_every_lane_of_every_row_against_the_oracle(ctx):
  """nx = 96, M = 51 on the three kinds of dense data, in a launch that pairs: every distinct partial[key][chunk][lane] the launch
  wrote within the sum of its points' bounds (include/wbx.h; the fp32 chains: 9 x 2^-24 per point)."""
  m = 51
  for j, vals in enumerate(EP.VALUES):
    fair = EC.fair_of(m, j)
    p, t, _ = EC.dense_case(400 + j, m, 1, UNIT, 96, values=vals, layout='ifs' if j & 1 else 'member_outside')
    plan, got, _ = _long_launch(ctx, p, t, fair)
    plan1, _ = _launch(ctx, p, t, fair)
    for unit in np.unique(_bits(got), axis=0).view(np.float64):
      want = _against_oracle(unit[None], plan1, p, t, fair, f'paired nx=96 {vals} fair={fair}')
      assert np.isfinite(want).all()
