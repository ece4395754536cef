"""CPU side of tests/test_gpu_ensemble_points.py: everything in that file that is not a kernel is held here without a GPU.

  * The test bodies of the GPU file run unchanged on the NumPy interpreter of the plans (tests/fake_device.py, the `emulated`
    backend) in place of the launches: every case the GPU file runs -- every route, member count, mode and live point -- passes
    its finite-share and exact-zero conditions on the expectation alone, and the expectation (ensemble_cases.expected_lanes,
    from oracle/wbx_oracle.py) agrees with an independent float64 restatement of the plan to the fp64 row of the bounds.  A
    mistake in the expectation or in a bound's plumbing shows here.  (At points with a NaN / infinite member the interpreter is
    GIVEN the conventions of include/wbx.h by `_emulated_lanes`, in the expectation's own words: there these runs hold the
    plumbing, and test_documented_conventions_of_the_expectation holds the conventions.)
  * The fp32 chain sums of stats32 restated in NumPy (ensemble_cases.stats32_emulated: the error model of include/wbx.h) stay
    inside the chain32 bounds on every dense float32 case of the pipelined routes and on 3 x 10^4 points per data family: the
    largest error / bound per lane is asserted <= 1 and printed, so whoever tightens a bound sees the margin.
  * The special points sit where the GPU file's docstrings say and the live-point list covers the escape thresholds from both
    sides."""
import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
import ensemble_cases as EC
import fake_device
import test_gpu_ensemble_points as GP

NL = EC.NLANE


class _Dev:
  def __init__(self, arr):
    self.ptr = arr


def _emulated_lanes(plan, p, t, algo):
  """fake_device._ens_lanes on the plan's own offset tables, with the two conventions of include/wbx.h the interpreter does not
  carry: the generic operator (M > 64, float64) IS the pair form, and in the float32 rank form for M <= 64 an infinite member
  poisons all five lanes like a NaN member does."""
  m = p.shape[1]
  _, mstride = GP.GI._layout(p, GP.GI.PD)  # pylint: disable=protected-access
  fam = EC.family('map', m, p.dtype, algo)
  devs = [_Dev(GP.GI._root(p).reshape(-1)), _Dev(GP.GI._root(t).reshape(-1))]  # pylint: disable=protected-access
  with np.errstate(all='ignore'):
    lanes = fake_device._ens_lanes(plan, devs, (m, mstride, EC.PAIRWISE if fam == 'generic' else algo), plan.flags)  # pylint: disable=protected-access
  lanes = np.stack(lanes, axis=-1)  # [key, depth, x, lane]
  x = np.moveaxis(np.asarray(p, np.float64), 1, -1)
  bad = ~np.isfinite(x).all(axis=-1)
  if fam == 'sorted64':
    lanes[bad.reshape(lanes.shape[:-1])] = np.nan
  elif bad.any():
    # the interpreter's pair matrix has a diagonal (|inf - inf| = NaN); the kernels sum the pairs i > j: an infinite spread
    with np.errstate(all='ignore'):
      pair = sum(np.abs(x[bad][:, i:i + 1] - x[bad][:, :i]).sum(axis=-1) for i in range(1, m)) if m > 1 else np.zeros(int(bad.sum()))
      lanes[bad.reshape(lanes.shape[:-1]), 1] = 2.0 * pair / (m * (m - (1.0 if plan.flags & _hip.FLAG_FAIR else 0.0)))
  return lanes


def _emulated_partial(ctx, p, t, mask, plan, dplan, mstride, algo, sentinel=None):
  lanes = _emulated_lanes(plan, p, t, algo)
  return GP.GI._expected_partials(plan, lanes * (1.0 if plan.x_weights is None else plan.x_weights[None, None, :, None]), mask, plan.flags)  # pylint: disable=protected-access


def _emulated_map(ctx, p, t, plan, dplan, mstride, algo):
  return _emulated_lanes(plan, p, t, algo)


def _emulated_binned(ctx, plan, dplan, p, t, m, mstride, wrow, bits, nbin, sentinel):
  nlead = p.shape[0]
  if not 2 <= m <= 64:
    return -1, np.full((nlead, 6, nbin), sentinel)
  lanes = _emulated_lanes(plan, p, t, EC.SORT).reshape(nlead, p.shape[2], p.shape[3], NL)
  member = ((bits[0][:, None] >> np.arange(nbin, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.float64)
  out = np.empty((nlead, 6, nbin))
  with np.errstate(invalid='ignore'):
    out[:, :NL] = np.einsum('ayxl,y,xb->alb', lanes, wrow, member)
  out[:, 5] = np.einsum('y,xb->b', wrow, member)
  return 0, out


class _Lib:
  def wbx_last_error(self):
    return b'wbx_ens_binned handles 2..64 members'


class _Ctx(fake_device.FakeCtx):
  lib = _Lib()


@pytest.fixture
def emu(monkeypatch):
  """The GPU file's launches replaced by the interpreter; plans are built by the planner exactly as on the GPU."""
  monkeypatch.setattr(engine, '_PlanOnDevice', lambda ctx, plan: None)
  monkeypatch.setattr(GP, '_run_partial', _emulated_partial)
  monkeypatch.setattr(GP, '_run_map', _emulated_map)
  monkeypatch.setattr(GP, '_launch_binned', _emulated_binned)
  return _Ctx()


# ---- the GPU file's own test bodies on the interpreter: shares, exact zeros, expectation == restatement -----------------------
@pytest.mark.parametrize('m,dtype', GP.M_CASES, ids=GP.M_IDS)
def test_map_x_kept_and_x_summed_cases_on_the_interpreter(emu, m, dtype):
  GP.test_map_every_point_every_lane(emu, m, dtype)
  GP.test_x_kept_every_partial(emu, m, dtype)
  GP.test_x_summed_wide_blocks_every_partial(emu, m, dtype)


@pytest.mark.parametrize('m', GP.M_REG)
def test_pair_form_and_pipelined_cases_on_the_interpreter(emu, m):
  GP.test_pair_form_every_partial(emu, m)
  GP.test_pipelined_sweep_every_partial(emu, m)


@pytest.mark.parametrize('m,dtype', GP.M_CASES, ids=GP.M_IDS)
def test_flat_weighted_cases_on_the_interpreter(emu, m, dtype):
  GP.test_flat_weighted_sweeps_every_partial(emu, m, dtype, 64, 'flat')
  GP.test_flat_weighted_sweeps_every_partial(emu, m, dtype, 128, 'xf1')


@pytest.mark.parametrize('mode', ['masked', 'skipna', 'masked+skipna'])
@pytest.mark.parametrize('m,dtype', GP.M_CASES, ids=GP.M_IDS)
def test_wrapper_cases_on_the_interpreter(emu, m, dtype, mode):
  for x_kept in (True, False):
    GP.test_masked_and_skipna_wrappers_every_partial(emu, m, dtype, mode, x_kept)


@pytest.mark.parametrize('m', GP.M_LIVE)
def test_one_live_point_cases_on_the_interpreter(emu, m):
  GP.test_pipelined_sweep_one_live_point_per_partial(emu, m)
  GP.test_flat_weighted_sweeps_one_live_point_per_partial(emu, m, 64, 'flat')
  GP.test_flat_weighted_sweeps_one_live_point_per_partial(emu, m, 128, 'xf1')
  GP.test_block_kernels_one_live_point_per_partial(emu, m, np.float32)
  if m in (50, 51):
    GP.test_escape_and_ordinary_point_in_one_tile(emu, m, 'pipe')
    GP.test_escape_and_ordinary_point_in_one_tile(emu, m, 'flat')


def test_generic_one_live_point_cases_on_the_interpreter(emu):
  GP.test_block_kernels_one_live_point_per_partial(emu, 65, np.float32)
  GP.test_block_kernels_one_live_point_per_partial(emu, 8, np.float64)


@pytest.mark.parametrize('m', EC.M_BINNED)
def test_binned_cases_on_the_interpreter(emu, m):
  GP.test_binned_dense_every_bin(emu, m)
  GP.test_binned_one_live_point_per_bin(emu, m)
  if m == 2:
    GP.test_binned_refuses_more_members_than_the_registers_hold(emu)
  if m in (50, 51):
    GP.test_binned_escape_and_ordinary_point_in_one_tile(emu, m)


# ---- the header's error model: stats32 restated, against the chain32 bounds --------------------------------------------------------
# (the chains are <= 8 terms of random rounding, so the largest error over many points sits well inside the worst case 9 u: what
#  is asserted is error <= bound at every point; the largest ratio per lane is returned and printed)
def _worst_ratio(p, t, fair):
  stat = EC.expected_lanes('chain32', p, t, fair)
  bound = EC.lane_bounds('chain32', p, t, stat)
  emu32 = EC.stats32_emulated(p, t, fair)
  fin = np.isfinite(stat)
  np.testing.assert_array_equal(np.isfinite(emu32), fin)
  err = np.abs(emu32 - stat)
  assert (err[fin] <= bound[fin]).all(), float(np.nanmax(np.where(fin & (bound > 0), err / np.where(bound > 0, bound, 1), 0)))
  with np.errstate(invalid='ignore', divide='ignore'):
    ratio = np.where(fin & (bound > 0), err / bound, 0.0)
  return ratio.reshape(-1, NL).max(axis=0)


def _finite_members(p, t):
  """The points stats32 is defined on: finite members (the others are poisoned before the sums)."""
  ok = np.isfinite(np.asarray(p, np.float64)).all(axis=1)
  p = np.where(ok[:, None], p, 0.0).astype(np.float32)
  return p, np.where(ok, t, 0.0).astype(np.float32)


@pytest.mark.parametrize('m', [50, 51])
def test_stats32_restated_holds_the_chain32_bounds_on_every_dense_case(m):
  """Every dense float32 case the pipelined routes run at M = 50 / 51 (ens_pipe_kernel, its FLAT flavour, ens_atoms_kernel): the
  NumPy restatement of the fp32 chains is inside the bounds the GPU file holds the kernels to."""
  worst = np.zeros(NL)
  for _, _, _, fair, fam, p, t, _ in GP._dense_inputs('pipe', m, np.float32, 'plain', False):  # pylint: disable=protected-access
    assert fam == 'chain32'
    worst = np.maximum(worst, _worst_ratio(*_finite_members(p, t), fair))
  for _, _, fair, fam, p, t, _, _ in GP._flat_inputs('flat', m, np.float32):  # pylint: disable=protected-access
    worst = np.maximum(worst, _worst_ratio(*_finite_members(p, t), fair))
  for _, _, _, fair, fam, p, t, _ in GP._binned_inputs(m):  # pylint: disable=protected-access
    worst = np.maximum(worst, _worst_ratio(*_finite_members(p, t), fair))
  print(f'stats32 restated, M={m}: largest error / bound per lane', np.round(worst, 3))
  assert (worst <= 1.0).all() and worst[0] > 0.05  # (inside the bound, and the data does make the chains round)


@pytest.mark.parametrize('values', ['anomaly', 'cancel'])
@pytest.mark.parametrize('m', [50, 51])
def test_stats32_restated_on_many_points_rounds_and_stays_inside(m, values):
  """3 x 10^4 points per family: on N(0, 1) anomalies and mixed magnitudes the chains of lanes 0 and 1 do round (the data of
  test_fp32_chain_sums_where_they_are_weakest, at offsets 280 and 5.5e4, adds them exactly) and stay inside 9 u."""
  p, t, _ = EC.dense_case(m, m, 2, 60, 250, values=values)
  worst = _worst_ratio(p, t, EC.fair_of(m))
  print(f'stats32 restated, M={m} {values}: largest error / bound per lane', np.round(worst, 3))
  assert (worst <= 1.0).all()
  assert worst[0] > 0.1 and worst[1] > 0.1, worst


# ---- the cases are what they say ----------------------------------------------------------------------------------------------------
def test_live_points_cover_the_escape_thresholds_from_both_sides():
  """compute<FAST32>: range == 0 or 2^-50 <= range <= 2^60, and the largest magnitude (target included) <= 2^100."""
  for m in (50, 51):
    kinds = {k[0]: k for k in EC.live_points(m)}
    rng_of = lambda k: float(np.float32(kinds[k][1].max()) - np.float32(kinds[k][1].min()))
    big_of = lambda k: float(max(np.abs(kinds[k][1]).max(), abs(kinds[k][2])))
    assert rng_of('range_2^-50') == 2.0 ** -50 and rng_of('range_2^-51') == 2.0 ** -51
    assert rng_of('range_2^60') == 2.0 ** 60 and rng_of('range_2^61') == 2.0 ** 61
    assert rng_of('big_2^100') == 0 and big_of('big_2^100') == 2.0 ** 100 and big_of('big_2^101') == 2.0 ** 101
    assert rng_of('range0') == 0 and kinds['range0'][1][0] != kinds['range0'][2]
    sub = np.abs(kinds['subnormal'][1])
    assert (sub[sub > 0] < np.finfo(np.float32).tiny).all() and (sub > 0).any()
    assert np.signbit(kinds['zeros'][1]).any() and not np.signbit(kinds['zeros'][1]).all()
    assert len(np.unique(kinds['ties'][1])) < m
    assert (np.diff(kinds['sorted'][1]) >= 0).all() and (np.diff(kinds['reversed'][1]) <= 0).all()
    assert np.isnan(kinds['nan_member'][1]).sum() == 1 and np.isposinf(kinds['pinf_member'][1]).sum() == 1
    assert np.isneginf(kinds['ninf_member'][1]).sum() == 1 and np.isposinf(kinds['two_pinf_members'][1]).sum() == 2
    assert np.isnan(kinds['nan_target'][2]) and np.isposinf(kinds['pinf_target'][2])


def test_documented_conventions_of_the_expectation():
  """include/wbx.h, line by line: the poison rule of the float32 rank form, plain IEEE on the other families, a NaN / infinite
  target leaves spread and variance finite, M = 1."""
  kinds = {k[0]: k for k in EC.live_points(8)}
  def lanes(fam, name, fair=True):
    k = kinds[name]
    return EC.expected_lanes(fam, k[1][None, :, None, None], np.array(k[2], np.float32).reshape(1, 1, 1), fair)[0, 0, 0]
  for name in ('nan_member', 'pinf_member', 'ninf_member', 'two_pinf_members'):
    assert np.isnan(lanes('sorted64', name)).all() and np.isnan(lanes('chain32', name)).all()
  assert np.isnan(lanes('pair', 'nan_member')).all() and np.isnan(lanes('generic', 'nan_member')).all()
  for fam in ('pair', 'generic'):
    v = lanes(fam, 'pinf_member')
    assert v[0] == np.inf and v[1] == np.inf and np.isnan(v[2]) and np.isnan(v[3]) and v[4] == np.inf
    v = lanes(fam, 'two_pinf_members')
    assert v[0] == np.inf and np.isnan(v[1:4]).all() and v[4] == np.inf
  for fam in ('sorted64', 'pair', 'generic', 'chain32'):
    v = lanes(fam, 'nan_target')
    assert np.isnan(v[[0, 3, 4]]).all() and np.isfinite(v[[1, 2]]).all()
    v = lanes(fam, 'pinf_target')
    assert (v[[0, 3, 4]] == np.inf).all() and np.isfinite(v[[1, 2]]).all()
  one = EC.live_points(1)[0]
  for fair in (True, False):
    v = EC.expected_lanes('sorted64', one[1][None, :, None, None], np.array(one[2], np.float32).reshape(1, 1, 1), fair)[0, 0, 0]
    assert np.isnan(v[2]) and np.isnan(v[3]) and np.isfinite(v[[0, 4]]).all()
    assert np.isnan(v[1]) if fair else v[1] == 0.0


def test_fair_is_on_and_off_for_every_member_count():
  for m in EC.M_F32 + EC.M_F64:
    assert {EC.fair_of(m, i) for i in range(4)} == {True, False}
