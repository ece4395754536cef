"""The cases of tests/det_partial_cases.py on the CPU: the restatement against oracle/wbx_oracle.py and tests/fake_device.py, the
route of every case against what its list claims, the conditions that keep a failure from hiding (exact magnitudes, the finite
share, the NaN share, the size cap), and the mutants -- wrong readings of the plan that the cases of a route must be able to see."""
import collections

import numpy as np
import pytest

from oracle import wbx_oracle as O
import det_partial_cases as DC
import fake_device

ALL = DC.all_cases()
BY_KERNEL = collections.defaultdict(list)
for _c in ALL:
  BY_KERNEL[_c.kernel].append(_c)


def test_names_are_unique_and_every_list_is_small():
  names = [c.name for c in ALL]
  assert len(names) == len(set(names))
  assert DC.MAX_POINTS == 300_000
  for c in ALL:
    assert c.npoint <= DC.MAX_POINTS, c.name
  assert sum(c.npoint for c in ALL) < 4_000_000


def test_the_six_lane_formulas_are_those_of_the_oracle_and_of_the_fake_device():
  rng = np.random.default_rng(3)
  p, t, c = ((5.5e4 + 300 * rng.normal(size=(4, 5, 6))).astype(np.float32) for _ in range(3))
  p[0, 0, 0], t[1, 1, 1], c[2, 2, 2] = np.nan, np.inf, -np.inf
  with np.errstate(all='ignore'):
    want = [O.error(p, t), O.absolute_error(p, t), O.squared_error(p, t), O.squared_prediction_anomaly(p, c), O.squared_target_anomaly(t, c),
            O.anomaly_covariance(p, t, c)]
    for func, n in ((DC.DET6, 6), (DC.DET3, 3)):
      got = DC.stat(func, p, t, c)
      fake = fake_device._det_lanes(func, [p, t, c])  # pylint: disable=protected-access
      assert len(got) == n
      for l in range(n):
        np.testing.assert_array_equal(got[l], want[l])
        np.testing.assert_array_equal(got[l], fake[l])
    np.testing.assert_array_equal(DC.stat(DC.PASS1, p)[0], p.astype(np.float64))


@pytest.mark.parametrize('kernel', ['xr', 'xk', 'xp', 'xf', 'map', 'none'])
def test_addresses_are_those_of_the_fake_device(kernel):
  for case in BY_KERNEL[kernel]:
    inp, _ = DC.prepared(case)
    for i, name in enumerate(DC.NAMES):
      if name in inp.flat:
        np.testing.assert_array_equal(DC.addresses(inp.plan, i), fake_device._offsets(inp.plan, i), err_msg=case.name)  # pylint: disable=protected-access


def _fake_partial(inp):
  case, plan = inp.case, inp.plan
  devs = [fake_device._Buf(inp.flat[n]) if n in inp.flat else None for n in DC.NAMES]  # pylint: disable=protected-access
  nl = DC.lanes_total(case.func, case.flags)
  return fake_device._run_s1(None, 'det', None, plan, devs, None, nl, func=case.func).ptr.reshape(plan.partial_shape(nl))  # pylint: disable=protected-access


@pytest.mark.parametrize('kernel', ['xr', 'xk', 'xp', 'xf', 'none'])
def test_restatement_against_the_fake_device(kernel):
  """Bit for bit on the exact class, within the bound on the others (the fake device sums with np.sum)."""
  for case in BY_KERNEL[kernel]:
    inp, exp = DC.prepared(case)
    got = _fake_partial(inp)
    if case.klass == 'exact':
      np.testing.assert_array_equal(got, exp.want, err_msg=case.name)
    assert not DC.differs(got, exp), case.name


def test_restatement_against_the_oracles_aggregate():
  """oracle.aggregate on the lanes the oracle computes from the points the plan addresses: one chunk, the exact class."""
  n = 0
  for case in ALL:
    if case.klass != 'exact' or case.kernel in ('map', 'none') or case.plan_nchunk != 1:
      continue
    inp, exp = DC.prepared(case)
    plan = inp.plan
    v = [inp.flat[nm][inp.idx[nm]] for nm in DC.NAMES[:DC.NINPUTS[case.func]]]
    with np.errstate(all='ignore'):
      lanes = {DC.PASS1: lambda p: [O.f64(p)], DC.DET3: lambda p, t: [O.error(p, t), O.absolute_error(p, t), O.squared_error(p, t)],
               DC.DET6: lambda p, t, c: [O.error(p, t), O.absolute_error(p, t), O.squared_error(p, t), O.squared_prediction_anomaly(p, c),
                                         O.squared_target_anomaly(t, c), O.anomaly_covariance(p, t, c)]}[case.func](*v)
    mask = (inp.flat['mask'][inp.idx['mask']] != 0) if case.flags & DC.FLAG_MASKED else None
    if mask is not None:  # aggregation.py:339-352 works on the statistic; the library zeroes the inputs: the same wherever the statistic is finite
      lanes = [np.where(mask, l, 0.0) for l in lanes]
    weights = [(inp.xw, ('x',))] if case.weights else []
    nl = len(lanes)
    for l, lane in enumerate(lanes):
      sws, sw, _ = O.aggregate(lane, ('k', 'd', 'x'), ('d',) if plan.x_kept else ('d', 'x'), weights=weights, mask=mask, mask_dims=('k', 'd', 'x'),
                               skipna=bool(case.flags & DC.FLAG_SKIPNA))
      np.testing.assert_array_equal(exp.want[:, 0, l, :].reshape(sws.shape), sws, err_msg=f'{case.name} lane {l}')
      if case.flags & DC.FLAG_SKIPNA:
        np.testing.assert_array_equal(exp.want[:, 0, nl + l, :].reshape(sw.shape), sw, err_msg=f'{case.name} count lane {l}')
      elif case.flags & DC.FLAG_MASKED:
        np.testing.assert_array_equal(exp.want[:, 0, nl, :].reshape(sw.shape), sw, err_msg=f'{case.name} count lane')
    n += 1
  assert n >= 40


def test_map_restatement_is_the_lane_of_the_point():
  for case in BY_KERNEL['map']:
    inp, exp = DC.prepared(case)
    v = [inp.flat[nm][inp.idx[nm]] for nm in DC.NAMES[:DC.NINPUTS[case.func]]]
    with np.errstate(all='ignore'):
      np.testing.assert_array_equal(exp.want, fake_device._det_lanes(case.func, v)[case.lane], err_msg=case.name)  # pylint: disable=protected-access
    assert exp.want.shape == (case.nkey, case.D, case.nx)


# ---------------------------------------------------------------------------------------------------------------------
# routes


@pytest.mark.parametrize('kernel', ['xr', 'xk', 'xp', 'xf', 'map', 'none'])
def test_every_case_takes_the_route_its_list_claims(kernel):
  assert BY_KERNEL[kernel]
  for case in BY_KERNEL[kernel]:
    inp, _ = DC.prepared(case)
    r = DC.route_of(inp)
    assert r['refused'] is None, (case.name, r)
    assert r['kernel'] == case.kernel and r['mrow'] == case.mrow, (case.name, r)
    if kernel in ('xr', 'xk'):
      assert r['V'] == case.vec and r['threads'] == case.bt, (case.name, r)
    if kernel == 'xr':
      assert r['grid'] == case.nkey * case.plan_nchunk


def test_the_branches_the_lists_name_are_reached():
  route = lambda name: DC.route_of(DC.prepared({c.name: c for c in ALL}[name])[0])
  # the mask row in LDS: on at 8192, off at 8196, off for one row, off with a depth_off[3], off under skipna
  for (on, off) in DC.xr_mrow_pair():
    assert DC.route_of(DC.prepared(on)[0])['mrow'] and not DC.route_of(DC.prepared(off)[0])['mrow']
    assert on.nx == DC.MROW_MAX and off.nx == DC.MROW_MAX + 4
  assert not route('xr-mrow-off-one-row-int')['mrow'] and not route('xr-mrow-off-zero-table-int')['mrow'] and not route('xr-mrow-off-skipna-int')['mrow']
  for on, off in DC.xr_mrow_twins():
    assert on.mrow and not off.mrow
  # x tiles of s1_xk
  assert route('xk-two-tiles-vec1-int')['grid'] == 3 * 2 * 2 and route('xk-two-tiles-vec4-int')['grid'] == 3 * 2 * 2
  assert route('xk-block-256-int')['grid'] == 3 * 2
  # plane mode: the second float4 of a thread, the LDS attribute branch, the block
  assert route('xp-64-R5-second-float4-int')['second_vec'] and route('xp-65-R8-D19-plain-int')['second_vec']
  assert not route('xp-65-R5-D10-plain-int')['second_vec'] and not route('xp-64-R3-D7-plain-int')['second_vec']
  for mode in ('plain', 'masked'):
    r = route(f'xp-det6-721-R8-{mode}-int')
    assert r['lds_attr'] and r['threads'] == 768 and DC.PLANE_LDS_ATTR < r['lds'] <= DC.PLANE_LDS_MAX, r
  assert not route('xp-det6-masked-int')['lds_attr']
  assert {route(f'xp-{nx}-R2-D{d}-plain-int')['threads'] for nx, d in ((64, 5), (721, 4), (1024, 3))} == {64, 768, 1024}
  # every lead 0..3 in every input and in the mask, inputs out of phase with each other
  inp, _ = DC.prepared({c.name: c for c in ALL}['xp-65-R5-D10-masked-int'])
  leads = np.stack([inp.plan.key_off[i] % 4 for i in (0, 1, 3)])
  assert all(set(row.tolist()) == {0, 1, 2, 3} for row in leads) and (leads[0] != leads[1]).all() and (leads[0] != leads[2]).all()
  # the flat sweep: a chunk boundary inside a plane, two planes in a chunk, fewer float4s than threads, more than one trip
  r = DC.prepared({c.name: c for c in ALL}['xf-nx-721-R8-chunk4-plain-int'])[0].plan
  assert r.depth_chunk < r.plane_rows and r.nx > r.block_threads
  r = DC.prepared({c.name: c for c in ALL}['xf-nx-7-R4-chunk8-plain-int'])[0].plan
  assert r.depth_chunk == 2 * r.plane_rows and r.nx < r.block_threads
  assert {c.nx for c in BY_KERNEL['xf']} >= {1, 2, 3, 7, 67, 721} and {c.bt for c in BY_KERNEL['xf']} == {64, 128, 256}
  for c in BY_KERNEL['xf']:
    if c.nx > 1:
      assert len(set(DC.prepared(c)[0].xw.tolist())) > 1, c.name  # weights that differ per latitude


def test_the_matrix_covers_every_instantiation():
  seen = {(c.dtype, c.func, c.flags, c.vec) for c in DC.xr_matrix_cases()}
  assert len(seen) == 2 * 3 * 4 * 2
  assert {c.bt for c in BY_KERNEL['xr']} == {64, 128, 256}
  assert {(c.flags, c.dtype) for c in BY_KERNEL['xk']} >= {(f, d) for f in DC.MODES.values() for d in ('float32', 'float64')}
  assert {c.nx % 4 for c in BY_KERNEL['xk'] if c.vec == 4} == {0, 1, 2, 3}
  assert {(c.dtype, c.func, c.lane) for c in BY_KERNEL['map']} >= {(d, f, l) for d in ('float32', 'float64') for f in DC.NLANES
                                                                     for l in range(DC.NLANES[f])}


@pytest.mark.parametrize('ref', DC.refusals(), ids=lambda r: r.name)
def test_a_refusal_breaks_one_requirement_of_an_accepted_call(ref):
  base = DC.REFUSAL_BASES[ref.base]
  inp, _ = DC.prepared(base)
  lane = base.lane if base.kernel == 'map' else None
  ok = DC.route(inp.plan, base.func, DC.F32, map_lane=lane)
  assert ok['refused'] is None and ok['kernel'] == base.kernel, ok
  r = DC.route(DC.refused_plan(inp.plan, ref), base.func, ref.dtype, map_lane=ref.lane if ref.lane is not None else lane,
               misaligned=tuple(n for n, _ in ref.shift))
  assert r['refused'] == DC.REFUSED[ref.why], (ref.name, r)


# ---------------------------------------------------------------------------------------------------------------------
# the conditions of the value classes


def test_the_exact_class_does_not_depend_on_the_order_of_its_terms():
  rng = np.random.default_rng(5)
  for case in ALL:
    if case.klass != 'exact' or case.kernel in ('map', 'none'):
      continue
    inp, exp = DC.prepared(case)
    assert (exp.bound == 0).all()
    assert (exp.want * 8 == np.round(exp.want * 8)).all() and np.abs(exp.want).max() < 2.0 ** 28, case.name
    if case.npoint > 40_000:
      continue
    lanes, _ = DC.point_lanes(inp)
    terms = lanes[0] * (1.0 if inp.xw is None else inp.xw[None, None, :])
    d0, d1 = inp.plan.chunk_rows(0)
    blk = terms[0, d0:d1].reshape(-1) if not inp.plan.x_kept else terms[0, d0:d1, 0]
    assert float(np.sum(rng.permutation(blk))) == exp.want[0, 0, 0, 0], case.name


def test_non_finite_cases_keep_three_quarters_of_the_outputs_finite_and_poison_only_their_own_partial():
  k0 = DC.TARGET_KEY
  for case in DC.nonfinite_cases():
    inp, exp = DC.prepared(case)
    want = exp.want
    assert np.isfinite(want).mean() >= 0.75, (case.name, np.isfinite(want).mean())
    bad = ~np.isfinite(want)
    if case.kernel == 'map':
      assert bad.sum() == 1 and bad[k0, 0, case.nx // 3]
      continue
    nl = DC.NLANES[case.func]
    if case.special == 'hidden':
      assert not bad.any(), case.name  # what the mask hides changes nothing
      continue
    assert not bad[:, :, nl:].any(), (case.name, 'a count lane is never poisoned')
    if not case.flags & DC.FLAG_SKIPNA:
      assert bad[k0, 0].any(), case.name
      rest = bad.copy()
      rest[k0, 0] = False
      assert not rest.any(), (case.name, 'another partial is poisoned')
      if inp.plan.x_kept:
        assert not np.delete(bad[k0, 0], case.nx // 3, axis=-1).any(), (case.name, 'another x is poisoned')
      if case.special == 'nan':
        assert np.isnan(want[k0, 0, :nl, case.nx // 3 if inp.plan.x_kept else 0]).sum() == 5  # every lane that reads p
      if case.special == 'inf_pair':
        assert np.isnan(want[k0, 0, 0]).any() and np.isposinf(want[k0, 0, 1]).any()


def test_skipna_cases_keep_a_counted_point_in_every_output_but_one():
  for case in DC.nonfinite_cases():
    if not case.flags & DC.FLAG_SKIPNA:
      continue
    inp, exp = DC.prepared(case)
    nl = DC.NLANES[case.func]
    nan_point = np.zeros((case.nkey, case.D, case.nx), bool)
    for n in ('p', 't', 'c'):
      nan_point |= np.isnan(inp.flat[n][inp.idx[n]])
    assert nan_point.mean() <= 0.25, (case.name, nan_point.mean())
    counts = exp.want[:, :, nl:]
    j = case.nx // 3 if inp.plan.x_kept else 0
    if case.special == 'all_nan':
      for l in (0, 1, 2, 3, 5):  # the lanes that read p: sum 0, count 0
        assert exp.want[DC.TARGET_KEY, 0, l, j] == 0 and counts[DC.TARGET_KEY, 0, l, j] == 0, (case.name, l)
      assert counts[DC.TARGET_KEY, 0, 4, j] > 0
      counts = counts.copy()
      counts[DC.TARGET_KEY, 0, :, j] = 1
    assert (counts > 0).all(), (case.name, int((counts == 0).sum()))
    if case.special == 'c_nan':  # a NaN climatology alone drops lanes 3-5 and keeps 0-2
      inp2 = DC.build(case)
      inp2.flat['c'][inp2.idx['c'][DC.TARGET_KEY, 0, case.nx // 3]] = 5.5e4
      d = DC.expected(inp2).want[DC.TARGET_KEY, 0, nl:, j] - counts[DC.TARGET_KEY, 0, :, j]
      assert d.tolist() == [0, 0, 0, 1, 1, 1], (case.name, d)


# ---------------------------------------------------------------------------------------------------------------------
# mutants


MUTANT_CASES = [(k, m) for k, ms in DC.MUTANTS.items() for m in ms]


@pytest.mark.parametrize('kernel,mutant', MUTANT_CASES, ids=[f'{k}-{m}' for k, m in MUTANT_CASES])
def test_a_wrong_reading_of_the_plan_leaves_the_restatement_on_some_case_of_its_route(kernel, mutant):
  """Each mutant is the error one of the index computations of the route's kernel would make: the last row of a chunk dropped; the
  rows past the first 64-row batch of every wave dropped (s1_xr); the ragged last lane of a vec-4 row dropped (s1_xk's nvalid < V);
  a plane lead off by one element / one mask byte (s1_xp); the flat sweep's weight index one latitude on, or not wrapped at the row
  end (s1_xf's m and the pad); the skipna count lanes all taken from lane 0's validity; the mask not applied to the climatology; row
  and column of the gather table swapped."""
  caught = []
  for case in BY_KERNEL[kernel]:
    if case.klass == 'nonfinite' or case.npoint > 40_000:
      continue
    inp, exp = DC.prepared(case)
    got = (DC.expected_map if kernel == 'map' else DC.expected)(inp, mutant).want
    if DC.differs(got, exp):
      caught.append(case.name)
  print(f'{kernel} / {mutant}: seen by {len(caught)} cases, e.g. {caught[:3]}')
  assert caught, (kernel, mutant)
  assert any(n.endswith('-int') for n in caught) and any(n.endswith('-rnd') for n in caught), (kernel, mutant, caught[:5])


def test_the_named_cases_see_their_mutants():
  """The case that is there for an index computation sees the mutant of it."""
  cases = {c.name: c for c in ALL}
  for name, mutant in (('xr-rows-65-int', 'first_batch_only'), ('xr-rows-257-four-waves-int', 'first_batch_only'),
                       ('xr-rows-130-two-waves-int', 'first_batch_only'), ('xk-masked-float32-vec4-nx69-int', 'drop_tail_lane'), ('xk-rows-3-ragged-lane-int', 'drop_tail_lane'),
                       ('xp-65-straddle-int', 'lead_data'), ('xp-65-straddle-int', 'lead_mask'), ('xf-nx-2-R4-chunk8-masked-int', 'weight_next_latitude'),
                       ('xf-nx-7-R4-chunk8-plain-int', 'weight_wrap'), ('xf-nx-721-R8-chunk4-masked-int', 'weight_wrap'),
                       ('xr-det6-skipna-float32-vec4-int', 'count_from_lane0'), ('xk-masked-float32-vec4-nx70-int', 'mask_not_on_c')):
    inp, exp = DC.prepared(cases[name])
    assert DC.differs(DC.expected(inp, mutant).want, exp), (name, mutant)
  for name in ('xr-rows-64-int', 'xr-rows-63-int'):  # ... and the shapes below the batch do not
    inp, exp = DC.prepared(cases[name])
    assert not DC.differs(DC.expected(inp, 'first_batch_only').want, exp)
