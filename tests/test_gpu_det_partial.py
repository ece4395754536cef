"""wbx_det_partial and wbx_det_map through the raw C ABI: EVERY output of every case of tests/det_partial_cases.py against its
float64 restatement -- NaN positions first, infinities equal, then bit for bit (the exact class) or |got - want| <= bound, the bound
computed per output from the inputs (2 (N + 3) 2^-53 sum |term| x 1.01 against a plain float64 evaluation, derived there).  The cases,
the route each one is aimed at, the conditions that keep a failure from hiding and the mutants that show what the cases can see are
checked on the CPU by tests/test_det_partial_cases.py.

Every launch prefills `out` with a sentinel and keeps GUARD sentinels behind the partial's end: the guard must be intact, no
sentinel may survive inside after a successful launch, and a refused call leaves every one of them.

Where two routes serve the same data the exact class gives the same bits on all of them: s1_xr with vec 1 / vec 4 / the mask row in
LDS, s1_xk against plane mode, the flat sweep against s1_xk followed by a host sum with the same weights."""
import ctypes as C

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
import det_partial_cases as DC

pytestmark = pytest.mark.gpu
SENTINEL = -7.7e77
GUARD = 64
ERR_INVALID = -1
WORST = {}  # route -> (largest |got - want| / bound, case)


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def _vp(v):
  return None if v is None else C.c_void_p(int(v))


def _bits(a):
  return (np.asarray(a) + 0.0).view(np.uint64)


class _Job:
  """The device side of one case: the plan with its tables, the inputs."""

  def __init__(self, ctx, inp):
    self.ctx, self.inp, self.case, self.plan = ctx, inp, inp.case, inp.plan
    self.dplan = self.device_plan(inp.plan)
    self.bufs = {name: ctx.upload(flat) for name, flat in inp.flat.items()}

  def device_plan(self, plan):
    return engine._PlanOnDevice(self.ctx, plan)  # pylint: disable=protected-access

  def run(self, plan=None, dtype=None, shift=(), lane=None):
    """-> (rc, the outputs, the guard behind them); `plan`: another plan over the same inputs."""
    case = self.case
    dplan = self.dplan if plan is None else self.device_plan(plan)
    plan = self.plan if plan is None else plan
    is_map = case.kernel == 'map'
    shape = (plan.nkey, plan.ndepth, plan.nx) if is_map else plan.partial_shape(DC.lanes_total(case.func, plan.flags))
    n = int(np.prod(shape))
    out = self.ctx.upload(np.full(n + GUARD, SENTINEL))
    ptr = {name: self.bufs[name].ptr + dict(shift).get(name, 0) if name in self.bufs else None for name in DC.NAMES}
    dt = (_hip.F32 if case.dtype == 'float32' else _hip.F64) if dtype is None else dtype
    if is_map:
      rc = self.ctx.lib.wbx_det_map(self.ctx.handle, C.byref(dplan.struct), case.func, dt, case.lane if lane is None else lane, _vp(ptr['p']),
                                    _vp(ptr['t']), _vp(ptr['c']), _vp(out.ptr))
    else:
      rc = self.ctx.lib.wbx_det_partial(self.ctx.handle, C.byref(dplan.struct), case.func, dt, _vp(ptr['p']), _vp(ptr['t']), _vp(ptr['c']),
                                        _vp(ptr['mask']), _vp(out.ptr))
    full = self.ctx.download(out.ptr, (n + GUARD,))
    return rc, full[:n].reshape(shape), full[n:]


def _compare(got, exp, case):
  want, bound = exp.want, exp.bound
  assert got.shape == want.shape, (case.name, got.shape, want.shape)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{case.name}: NaN positions')
  inf = np.isinf(want)
  np.testing.assert_array_equal(got[inf], want[inf], err_msg=f'{case.name}: infinities')
  if case.klass == 'exact':
    assert np.array_equal(_bits(got), _bits(want)), (case.name, 'exact class, bit for bit', np.argwhere(got != want)[:4].tolist())
    return 0.0
  fin = np.isfinite(want)
  err = np.abs(got[fin] - want[fin])
  with np.errstate(all='ignore'):
    ratio = np.where(err == 0, 0.0, err / bound[fin])
  worst = float(ratio.max()) if ratio.size else 0.0
  print(f'{case.name}: largest |got - want| / bound = {worst:.3f} (N <= {exp.terms})')
  if worst >= WORST.get(case.kernel, (-1.0, ''))[0]:
    WORST[case.kernel] = (worst, case.name)
  bad = err > bound[fin]
  assert not bad.any(), (case.name, 'outputs beyond the bound', int(bad.sum()), np.argwhere(fin)[bad][:4].tolist(), worst)
  return worst


def _check(ctx, case):
  inp, exp = DC.prepared(case)
  job = _Job(ctx, inp)
  rc, got, guard = job.run()
  _hip.check(rc, case.name)
  assert (guard == SENTINEL).all(), (case.name, 'written behind the end of the partial')
  assert not (got == SENTINEL).any(), (case.name, 'outputs left unwritten', int((got == SENTINEL).sum()))
  _compare(got, exp, case)
  return job, got


def _ids(cases):
  return dict(argvalues=cases, ids=[c.name for c in cases])


def _pair_ids(pairs):
  return dict(argvalues=pairs, ids=[a.name for a, _ in pairs])


# ---- s1_xr
@pytest.mark.parametrize('case', **_ids(DC.xr_matrix_cases()))
def test_xr_every_dtype_family_and_mask_mode(ctx, case):
  _check(ctx, case)


def test_xr_vec1_and_vec4_give_the_same_bits_on_the_exact_class(ctx):
  cases = {c.name: c for c in DC.xr_matrix_cases() + DC.xr_address_cases()}
  n = 0
  for name, case in cases.items():
    if name.endswith('vec1-int') and name.replace('vec1', 'vec4') in cases:
      _, one = _check(ctx, case)
      _, four = _check(ctx, cases[name.replace('vec1', 'vec4')])
      assert np.array_equal(_bits(one), _bits(four)), name
      n += 1
  assert n >= 24 + 6


@pytest.mark.parametrize('case', **_ids(DC.xr_shape_cases()))
def test_xr_row_widths_row_batches_and_chunks(ctx, case):
  _check(ctx, case)


@pytest.mark.parametrize('case', **_ids(DC.xr_address_cases()))
def test_xr_addressing(ctx, case):
  _check(ctx, case)


@pytest.mark.parametrize('case', **_ids(DC.xr_mrow_cases()))
def test_xr_mask_row_in_lds_and_where_it_is_not(ctx, case):
  _check(ctx, case)


@pytest.mark.parametrize('pair', **_pair_ids(DC.xr_mrow_pair() + DC.xr_mrow_twins()))
def test_xr_mask_row_in_lds_agrees_with_the_plain_route(ctx, pair):
  on, off = pair
  _, a = _check(ctx, on)
  _, b = _check(ctx, off)
  if on.klass == 'exact':
    assert np.array_equal(_bits(a), _bits(b)), (on.name, off.name)
  else:
    tol = DC.prepared(on)[1].bound + DC.prepared(off)[1].bound
    assert (np.abs(a - b) <= tol).all(), (on.name, off.name)


# ---- s1_xk
@pytest.mark.parametrize('case', **_ids(DC.xk_cases()))
def test_xk_every_output(ctx, case):
  _check(ctx, case)


# ---- s1_xp
@pytest.mark.parametrize('case', **_ids(DC.xp_cases()))
def test_xp_every_output(ctx, case):
  _check(ctx, case)


@pytest.mark.parametrize('pair', **_pair_ids(DC.xp_route_twins()))
def test_xp_and_xk_agree_on_the_same_data(ctx, pair):
  plane, rows = pair
  _, a = _check(ctx, plane)
  _, b = _check(ctx, rows)
  np.testing.assert_array_equal(DC.prepared(plane)[1].want, DC.prepared(rows)[1].want)
  if plane.klass == 'exact':
    assert np.array_equal(_bits(a), _bits(b)), plane.name
  else:
    assert (np.abs(a - b) <= 2 * DC.prepared(plane)[1].bound).all(), plane.name


# ---- s1_xf
@pytest.mark.parametrize('case', **_ids(DC.xf_cases()))
def test_xf_every_output(ctx, case):
  _check(ctx, case)


@pytest.mark.parametrize('pair', **_pair_ids(DC.xf_route_twins()))
def test_xf_agrees_with_xk_and_a_host_sum_with_the_same_weights(ctx, pair):
  flat, rows = pair
  assert flat.klass == 'exact'
  _, a = _check(ctx, flat)
  _, b = _check(ctx, rows)
  w = DC.prepared(flat)[0].xw
  host = (b * w[None, None, None, :]).sum(axis=3, keepdims=True)  # exact: multiples of 1/8 far below 2^53
  assert np.array_equal(_bits(a), _bits(host)), flat.name


# ---- s1_map
@pytest.mark.parametrize('case', **_ids(DC.map_cases()))
def test_map_every_lane(ctx, case):
  _check(ctx, case)


# ---- non-finite values
@pytest.mark.parametrize('case', **_ids(DC.nonfinite_cases()))
def test_non_finite_points_land_where_the_restatement_puts_them(ctx, case):
  _check(ctx, case)


# ---- empty extents
@pytest.mark.parametrize('case', **_ids(DC.empty_cases()))
def test_empty_extents_give_zeros_of_the_right_length(ctx, case):
  inp, exp = DC.prepared(case)
  plan = inp.plan
  n = C.c_int64(-1)
  job = _Job(ctx, inp)
  _hip.check(ctx.lib.wbx_s1_partial_len(C.byref(job.dplan.struct), DC.NLANES[case.func], C.byref(n)), 'wbx_s1_partial_len')
  assert n.value == exp.want.size == plan.nkey * plan.nchunk * DC.lanes_total(case.func, case.flags) * plan.nj
  rc, got, guard = job.run()
  _hip.check(rc, case.name)
  assert (got == 0).all() and (guard == SENTINEL).all(), case.name


# ---- refusals
@pytest.mark.parametrize('ref', DC.refusals(), ids=lambda r: r.name)
def test_one_broken_requirement_is_refused_in_the_entrys_words_and_out_is_untouched(ctx, ref):
  base = DC.REFUSAL_BASES[ref.base]
  inp, exp = DC.prepared(base)
  job = _Job(ctx, inp)
  rc, got, guard = job.run(plan=DC.refused_plan(inp.plan, ref), dtype=ref.dtype, shift=ref.shift, lane=ref.lane)
  message = ctx.lib.wbx_last_error().decode()
  assert rc == ERR_INVALID and DC.REFUSED[ref.why] in message, (ref.name, rc, message)
  assert (got == SENTINEL).all() and (guard == SENTINEL).all(), ref.name
  rc, got, guard = job.run()  # and the same call as it stands is accepted
  _hip.check(rc, base.name)
  assert (guard == SENTINEL).all() and not (got == SENTINEL).any()
  _compare(got, exp, base)


def test_zz_largest_ratio_to_the_bound_per_route():
  """(runs last: prints what the comparisons above have seen)"""
  for kernel in ('xr', 'xk', 'xp', 'xf', 'map'):
    worst, name = WORST.get(kernel, (float('nan'), 'not run'))
    print(f'largest |got - want| / bound on {kernel}: {worst:.3f} ({name})')
    assert not worst >= 1.0, (kernel, worst, name)
