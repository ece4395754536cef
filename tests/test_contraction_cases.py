"""tests/contraction_cases.py without a GPU: the restatement against loops, the exactness of the exact class, the routes the case
lists are aimed at (restated from csrc/wbx_s2.hip, csrc/wbx_s2_patch.hip and csrc/wbx_patch.hpp) and the builders' own asserts."""
import numpy as np
import pytest

import contraction_cases as CC
from contraction_cases import Plan


@pytest.mark.parametrize('sum_j', [1, 0])
def test_the_restatement_is_the_loop_over_every_index(sum_j):
  for kind in ('exact', 'rounded'):
    case = CC.make_case(Plan(2, 2, 3, 2, 2, 5, 4, sum_j), kind, 'dense')
    loops = CC.brute_force(case.partial, case.w, sum_j)
    einsum = np.einsum('abrclj,brjn->abln' if sum_j else 'abrclj,brjn->abljn', case.partial, case.w)
    assert case.want.shape == case.plan.out_shape
    if kind == 'exact':
      assert case.want.tobytes() == loops.tobytes() == (einsum + 0.0).tobytes()
    else:
      assert (np.abs(case.want - loops) <= 2 * case.bound).all() and (np.abs(case.want - einsum) <= 2 * case.bound).all()
      assert (case.bound[..., 0] > 0).all() and (case.bound[..., 1] == 0).all()  # bin 1 is empty: its outputs are exactly 0
      assert (case.bound <= 1e-12 * np.abs(case.partial).max() * case.plan.nterms).all()


def test_bits_and_dense_operands_describe_the_same_w():
  case = CC.make_case(Plan(1, 2, 5, 1, 1, 70, 64), 'exact', 'boxes')
  for n in (0, 31, 32, 63):
    np.testing.assert_array_equal((case.bits >> np.uint64(n)) & np.uint64(1), case.member[..., n])
  np.testing.assert_array_equal(case.w != 0, case.member)
  assert case.bits.dtype == np.uint64 and (case.bits >> np.uint64(63)).any()


def test_the_exact_class_does_not_depend_on_the_order_of_its_terms():
  rng = np.random.default_rng(0)
  for name, plan, _, _ in (CC.DENSE_SPLIT_ONE, CC.DENSE_SUM_J[4]):
    case = CC.make_case(plan, 'exact', 'dense')
    terms = (case.partial[0, 0, :, :, 0, :, None] * case.w[0, :, None]).reshape(-1, plan.nbin)  # [(r, c, j)][n]
    assert len(terms) == plan.nterms
    straight = np.zeros(plan.nbin)
    for t in terms:
      straight += t
    shuffled = np.zeros(plan.nbin)
    for t in terms[rng.permutation(len(terms))]:
      shuffled += t
    chunks_first = (case.partial[0, 0, :, :, 0].sum(axis=1)[..., None] * case.w[0]).reshape(-1, plan.nbin).sum(axis=0)
    assert straight.tobytes() == shuffled.tobytes() == (chunks_first + 0.0).tobytes() == case.want[0, 0, 0].tobytes(), name
    assert (terms * 8 == np.rint(terms * 8)).all() and np.abs(terms).sum(axis=0).max() < 2.0 ** 42


def test_more_terms_than_the_exact_class_allows_are_refused():
  with pytest.raises(AssertionError, match='more terms'):
    CC.make_case(Plan(1, 1, 2, 1, 1, 2 ** 16 + 1, 1), 'exact', 'dense')


def test_every_listed_case_takes_the_route_it_is_aimed_at():
  seen = set()
  threads = {'reduce': set(), 'keepj': set()}
  for form, patch_min, name, plan, rname, nums in CC.all_listed():
    r = CC.route(plan, form, patch_min)
    assert r.name == rname, (name, plan, r)
    for key, value in nums.items():
      assert r.info[key] == value, (name, plan, key, r.info[key], value)
    seen.add(r.name)
    if form == 'dense':
      threads[r.name.split('/')[0]].add(r.threads)
  want = {'reduce/short', 'reduce/long', 'reduce/long+split', 'reduce/fixed_j', 'keepj'}
  want |= {f'bits<{nb}>/{kind}' for nb in (16, 32, 64) for kind in ('sum_j', 'keep_j')}
  want |= {f'patch<{nl},{k}>' for nl, k in zip(CC.PATCH_LANES, (32, 24, 16, 12, 8, 7, 5, 2, 2))}
  assert seen == want
  assert threads == {'reduce': {64, 128, 256}, 'keepj': {64, 128, 256}}
  # the three thread counts of each of s2_reduce_kernel's three loops
  for rname in ('reduce/short', 'reduce/long', 'reduce/fixed_j'):
    assert {CC.route(p, 'dense').threads for _, p, n, _ in CC.DENSE_SUM_J + CC.DENSE_KEEP_J if n == rname} == {64, 128, 256}, rname


def test_the_geometries_named_in_the_lists():
  assert CC.route(CC.DENSE_SPLIT_BIG[1], 'dense').info == dict(threads=256, grid=60, groups=1, nsplit=35, per=2, empty_splits=12)
  assert CC.route(CC.DENSE_SPLIT_ONE[1], 'dense').info == dict(threads=256, grid=1, groups=1, nsplit=46, per=1, empty_splits=0)
  assert int(np.prod(CC.DENSE_SPLIT_BIG[1].partial_shape)) * 8 == 31795200  # the 32 MB partial
  assert CC.route(CC.DENSE_SPLIT_SMALL[1], 'dense').info == dict(threads=256, grid=4, groups=2, nsplit=512, per=3, empty_splits=145)
  assert 1100 % 3 == 2 and 1100 // 512 == 2  # a ragged last block; the rounded-down share would drop rows
  r = CC.route(Plan(50, 2, 7, 2, 15, 1, 17), 'bits', CC.PATCH_OFF)
  assert (r.rows_per_block, r.nsplit, r.rows) == (3, 3, [3, 3, 1])
  got = {(g[0]): CC.route(Plan(3, 2, g[0][0], 1, 4, g[0][1], 34), 'bits', 0) for g in CC.PATCH_GEOMETRIES}
  assert [r.rows for r in got.values()] == [[1], [2], [37], [33, 32], [34, 33], [44, 44, 42], [49, 49, 49, 46]]
  assert {r.nrs for r in got.values()} == {1, 2, 3, 4}
  assert [r.nxt for r in got.values()] == [2, 2, 1, 2, 3, 1, 2]


def test_what_decides_between_the_patch_kernel_and_the_block_kernel():
  big = Plan(3, 2, 29, 1, 4, 1440, 34)
  assert int(np.prod(big.partial_shape)) < CC.PATCH_MIN_DEFAULT
  assert CC.route(big, 'bits').name == 'bits<64>/sum_j' and CC.route(big, 'bits', 0).name == 'patch<4,12>'
  assert CC.route(Plan(3, 2, 37, 1, 4, 1440, 34, 0), 'bits', 0).name == 'bits<64>/keep_j'
  assert CC.route(Plan(3, 2, 37, 1, 4, 63, 34), 'bits', 0).name == 'bits<64>/sum_j'
  for nl in (8, 9, 11, 13, 14):
    assert CC.route(Plan(3, 2, 37, 1, nl, 64, 34), 'bits', 0).name == 'bits<64>/sum_j'
  assert CC.route(Plan(5, 2, 23, 2, 6, 1440, 3), 'bits').name == 'patch<6,7>'  # 4 M elements: past the default threshold


def test_the_patterns_hold_what_the_patch_kernel_has_to_meet():
  """Over the patch launches of all lane counts: patches with an empty union in every row split and in one only, a union in the
  high 32 bits only, bits 31 and 63, an empty bin, a bin of every point, points in no bin, one sweep and several."""
  seen = {'sweeps1': set(), 'sweeps>1': set(), 'empty': set(), 'high': set()}
  for nl in CC.PATCH_LANES:
    for plan, pattern in CC.patch_rotation(nl):
      case = CC.make_case(plan, 'exact', pattern)
      r = CC.route(plan, 'bits', 0, case.bits)
      assert r.sweeps >= -(-r.largest_union // r.K) and r.unions.shape == (plan.nBk, r.nrs, r.nxt)
      if pattern == 'tiles':
        assert r.largest_union <= 2 <= r.K and r.sweeps == 1
      if pattern == 'dense' and plan.nbin >= 34:
        assert r.largest_union == plan.nbin - 1 > r.K and r.sweeps > 1
        assert case.member[..., 0].all() and not case.member[..., 1].any()
      if pattern == 'boxes':
        assert not case.member.any(axis=-1).all(), 'some points belong to no bin'
        if r.nxt >= 2:
          assert (r.unions[0, :, -1] == 0).all() and (r.unions[1, :, 0] == 0).all()
        if r.nrs >= 2:
          assert r.unions[0, 0, 0] == 0 and (r.unions[0, 1:, 0] != 0).all()
          assert r.unions[1, -1, -1] == 0 and (r.unions[1, :-1, -1] != 0).any()
        if plan.nbin >= 3:
          assert not case.member[..., 1].any()
        if plan.nbin > 32:
          assert r.high_only_unions >= 1 and r.unions[0, -1, 0] >> np.uint64(32) and not r.unions[0, -1, 0] & np.uint64(0xFFFFFFFF)
      if plan.nbin == 64:
        assert case.member[..., 63].any() and (case.member[..., 31].any() or plan.nBr == 1)
      seen['sweeps1' if r.sweeps == 1 else 'sweeps>1'].add(nl)
      if r.empty_unions:
        seen['empty'].add(nl)
      if r.high_only_unions:
        seen['high'].add(nl)
  assert all(v == set(CC.PATCH_LANES) for v in seen.values()), seen


def test_every_axis_value_occurs_with_every_lane_count():
  for nl in CC.PATCH_LANES:
    rot = CC.patch_rotation(nl)
    assert {(p.nBr, p.nj) for p, _ in rot} == {g[0] for g in CC.PATCH_GEOMETRIES}
    assert {p.nbin for p, _ in rot} == set(CC.PATCH_NBINS) and {p.nchunk for p, _ in rot} == set(CC.PATCH_NCHUNKS)
    assert {pat for _, pat in rot} == set(CC.PATCH_PATTERNS)
    assert all((p.nA, p.nBk, p.nlane, p.sum_j) == (3, 2, nl, 1) for p, _ in rot)
  # the two-rows-in-flight loop (nchunk = 1) meets every geometry, and nlane 2, 4 and 12 meet three chunks
  assert {(p.nBr, p.nj) for nl in CC.PATCH_LANES for p, _ in CC.patch_rotation(nl) if p.nchunk == 1} == {g[0] for g in CC.PATCH_GEOMETRIES}


def test_non_finite_cases_keep_three_quarters_of_the_outputs_finite():
  plan = Plan(3, 2, 65, 3, 2, 65, 34)
  base = CC.make_case(plan, 'rounded', 'boxes')
  r = CC.route(plan, 'bits', 0, base.bits)
  sites = CC.nonfinite_sites(plan, base.member, r.rows, 0)
  assert [label for label, _ in sites] == ['first row of a split', 'last row of an odd-length split', 'last row of an even-length split',
                                           'tail lane of the last x tile', 'a chunk other than 0', 'a point that belongs to no bin']
  assert [s[0] for _, s in sites[:3]] == [33, 32, 64] and sites[3][1][2] == 64 and sites[4][1][1] == 2
  assert not base.member[0][sites[5][1][0], sites[5][1][2]].any()
  assert r.unions[0, 0, 1] == 0 and sites[3][1][2] // 64 == 1  # the tail-lane site of bk 0 lies in a patch with an empty union
  for value in (np.nan, np.inf, -np.inf):
    for _, site in sites:
      partial, on_bits, on_dense = CC.nonfinite_case(base, value, site, (1, 0, 1))
      with np.errstate(invalid='ignore'):
        literal = np.einsum('abrclj,brjn->abln', partial, base.w)
      np.testing.assert_array_equal(np.isnan(literal), np.isnan(on_dense))
      np.testing.assert_array_equal(literal[np.isinf(literal)], on_dense[np.isinf(on_dense)])
      assert np.isnan(on_bits[1, 0, 1]).all() and np.isfinite(np.delete(on_bits.reshape(12, 34), 5, axis=0)).all()
      assert np.isfinite(on_bits).mean() >= 0.75
  with pytest.raises(AssertionError, match='finite share'):
    CC.nonfinite_case(CC.make_case(Plan(1, 1, 4, 1, 2, 3, 2), 'rounded', 'dense'), np.nan, (0, 0, 0), (0, 0, 0))


def test_non_finite_expectations_when_j_is_kept():
  plan = Plan(2, 2, 5, 2, 2, 9, 5, 0)
  base = CC.make_case(plan, 'rounded', 'boxes')
  r, j = CC.no_bin_point(base.member, 1)
  partial, on_bits, on_dense = CC.nonfinite_case(base, -np.inf, (r, 1, j), (0, 1, 1))
  assert np.isnan(on_bits[0, 1, 1, j]).all() and np.isnan(on_bits).sum() == 5 and np.isnan(on_dense[0, 1, 1, j]).all()
  with np.errstate(invalid='ignore'):
    literal = np.einsum('abrclj,brjn->abljn', partial, base.w)
  np.testing.assert_array_equal(np.isnan(literal), np.isnan(on_dense))
