"""Stage 2 through the raw C ABI: EVERY output of wbx_contract and wbx_contract_bits against the float64 restatement of
tests/contraction_cases.py on every route -- s2_reduce_kernel (short rows, long rows, fixed j, split + finish), s2_keepj_kernel,
s2_bits_kernel<16 | 32 | 64> (j summed over row blocks, j kept), s2_patch_kernel<NL, K> + det_binned_finish for the nine lane
counts.  Bit for bit in the exact class, within twice the derived bound E in the rounded class, NaN / inf placement as include/wbx.h
documents it in the non-finite class.  Every output buffer is prefilled with a sentinel, every launch is made twice and the two
results must be bit-equal (the summation order is fixed by the launch geometry).  The cases, their routes and the membership
patterns are those of contraction_cases.py; test_contraction_cases.py holds the routes against the dispatch."""
import ctypes as C

import numpy as np
import pytest

from weatherbenchx_amd import _hip
import contraction_cases as CC
from contraction_cases import Plan

pytestmark = pytest.mark.gpu
KINDS = ('exact', 'rounded')
PATTERNS = CC.PATCH_PATTERNS
VALUES = (np.nan, np.inf, -np.inf)


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def _ptr(buf):
  return None if buf is None else C.c_void_p(buf.ptr)


class _Operands:
  """The device copies of a case's operands; the dense W only where a dense launch asks for it."""

  def __init__(self, ctx, case, partial=None):
    self.ctx, self.case = ctx, case
    self.partial = ctx.upload(case.partial if partial is None else partial)
    self.wt, self.bits = ctx.upload(case.wt), ctx.upload(case.bits)
    self._w = None

  @property
  def w(self):
    if self._w is None:
      self._w = self.ctx.upload(self.case.w)
    return self._w


def _call(ctx, form, plan, partial, second, third, out):
  struct = _hip.S2PlanStruct(*plan.fields())
  if form == 'dense':
    return ctx.lib.wbx_contract(ctx.handle, C.byref(struct), _ptr(partial), _ptr(second), _ptr(out))
  return ctx.lib.wbx_contract_bits(ctx.handle, C.byref(struct), _ptr(partial), _ptr(second), _ptr(third), _ptr(out))


def _launch(ctx, monkeypatch, form, ops, patch_min=CC.PATCH_OFF):
  """Two launches into sentinel-filled buffers -> the first result; the second must repeat its bits."""
  plan = ops.case.plan
  monkeypatch.setenv('WBX_S2_PATCH_MIN', str(patch_min))
  outs = []
  for _ in range(2):
    out = ctx.upload(np.full(plan.out_shape, CC.SENTINEL))
    second, third = (ops.w, None) if form == 'dense' else (ops.wt, ops.bits)
    _hip.check(_call(ctx, form, plan, ops.partial, second, third, out), f'{form} {plan}')
    outs.append(ctx.download(out.ptr, plan.out_shape, np.float64))
  assert outs[0].tobytes() == outs[1].tobytes(), f'{form} {plan}: two launches of one case differ'
  return outs[0]


def _both_kinds(ctx, monkeypatch, form, name, plan, rname, patch_min, pattern, geom=None):
  """The exact and the rounded case of one plan through one route."""
  for kind in KINDS:
    case = CC.make_case(plan, kind, pattern, geom=geom)
    r = CC.route(plan, form, patch_min, case.bits)
    assert r.name == rname, (name, r)
    what = f'{name}: {rname} {pattern} {kind} {plan}'
    ratio = CC.check(_launch(ctx, monkeypatch, form, _Operands(ctx, case), patch_min), case, what)
    print(f'{what}: largest error / allowed {ratio:.3f}')


def _ids(rows):
  return [r[0].replace(' ', '-') for r in rows]


@pytest.mark.parametrize('row', CC.DENSE_SUM_J + [CC.DENSE_SPLIT_ONE, CC.DENSE_SPLIT_SMALL], ids=_ids(CC.DENSE_SUM_J + [CC.DENSE_SPLIT_ONE, CC.DENSE_SPLIT_SMALL]))
def test_dense_rows_summed_over_j(ctx, monkeypatch, row):
  """s2_reduce_kernel with j contracted: rows shorter than a wave, long rows walked by the lanes, one output over 46 one-row blocks,
  four outputs over 512 blocks of 3 (row, chunk) pairs with a ragged last one and 145 empty ones."""
  name, plan, rname, _ = row
  i = (CC.DENSE_SUM_J + [CC.DENSE_SPLIT_ONE, CC.DENSE_SPLIT_SMALL]).index(row)
  _both_kinds(ctx, monkeypatch, 'dense', name, plan, rname, CC.PATCH_OFF, PATTERNS[i % 3])


def test_dense_split_of_sixty_outputs_over_a_32_mb_partial(ctx, monkeypatch):
  """35 blocks of 2 (row, chunk) pairs per output, the last 12 of them without a pair: they must write zeros for the finish."""
  name, plan, rname, _ = CC.DENSE_SPLIT_BIG
  _both_kinds(ctx, monkeypatch, 'dense', name, plan, rname, CC.PATCH_OFF, 'boxes')


@pytest.mark.parametrize('row', CC.DENSE_KEEP_J, ids=_ids(CC.DENSE_KEEP_J))
def test_dense_rows_with_j_kept(ctx, monkeypatch, row):
  """A block per j below 64 points (s2_reduce_kernel, fixed j), a thread per j from 64 on (s2_keepj_kernel), ragged last tiles."""
  name, plan, rname, _ = row
  _both_kinds(ctx, monkeypatch, 'dense', name, plan, rname, CC.PATCH_OFF, PATTERNS[CC.DENSE_KEEP_J.index(row) % 3])


@pytest.mark.parametrize('row', CC.BITS_SUM_J, ids=_ids(CC.BITS_SUM_J))
def test_bit_masks_summed_over_j_by_row_blocks(ctx, monkeypatch, row):
  """s2_bits_kernel + s2_bits_finish_kernel with the patch kernel switched off or not eligible: the three instantiations at their
  first and last bin counts, lane counts the patch kernel does not have, row blocks of 3, 3 and 1 rows, one block per output."""
  name, plan, rname, _ = row
  _both_kinds(ctx, monkeypatch, 'bits', name, plan, rname, CC.PATCH_OFF, PATTERNS[CC.BITS_SUM_J.index(row) % 3])


@pytest.mark.parametrize('row', CC.BITS_KEEP_J, ids=_ids(CC.BITS_KEEP_J))
def test_bit_masks_with_j_kept(ctx, monkeypatch, row):
  """s2_bits_kernel with one j per thread in blocks of 256 j."""
  name, plan, rname, _ = row
  _both_kinds(ctx, monkeypatch, 'bits', name, plan, rname, 0, PATTERNS[(CC.BITS_KEEP_J.index(row) + 1) % 3])


@pytest.mark.parametrize('nl', CC.PATCH_LANES)
def test_patch_kernel_of_every_lane_count(ctx, monkeypatch, nl):
  """s2_patch_kernel<NL, K> + det_binned_finish over the seven (rows, points) geometries -- one row, two rows, one split, two to
  four splits with ragged last ones, tiles with 1, 2, 6 and 63 live lanes -- with nchunk, nbin and the membership pattern rotating."""
  for plan, pattern in CC.patch_rotation(nl):
    _both_kinds(ctx, monkeypatch, 'bits', f'patch NL={nl}', plan, f'patch<{nl},{CC.patch_k(nl)}>', 0, pattern)


CROSS = [Plan(3, 2, 65, 1, 4, 65, 64), Plan(3, 2, 67, 3, 2, 130, 34), Plan(2, 2, 130, 1, 12, 64, 64), Plan(3, 2, 1, 1, 7, 65, 34),
         Plan(3, 2, 2, 3, 10, 127, 1), Plan(1, 1, 23, 2, 1, 1440, 33)]


@pytest.mark.parametrize('plan', CROSS, ids=[f'nBr{p.nBr}-nchunk{p.nchunk}-nlane{p.nlane}-nj{p.nj}-nbin{p.nbin}' for p in CROSS])
def test_the_three_routes_of_one_case_give_the_same_bits(ctx, monkeypatch, plan):
  """An exact case through the dense W, the bit masks by row blocks and the patch kernel: each equals the restatement bit for bit, so
  all three are bit-identical; the same with j kept (two routes)."""
  for pattern in ('boxes', 'dense'):
    case = CC.make_case(plan, 'exact', pattern)
    ops = _Operands(ctx, case)
    names = [CC.route(plan, 'dense').name.split('/')[0], CC.route(plan, 'bits', CC.PATCH_OFF).name.split('<')[0], CC.route(plan, 'bits', 0).name.split('<')[0]]
    assert names == ['reduce', 'bits', 'patch']
    got = [_launch(ctx, monkeypatch, 'dense', ops), _launch(ctx, monkeypatch, 'bits', ops, CC.PATCH_OFF), _launch(ctx, monkeypatch, 'bits', ops, 0)]
    for g, name in zip(got, ('dense', 'bits by row blocks', 'patch')):
      CC.check(g, case, f'{name} {pattern} {plan}')
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()
    kept = Plan(*plan.fields()[:7], 0)
    case = CC.Case(kept, 'exact', pattern, case.partial, case.wt, case.member)
    ops = _Operands(ctx, case)
    got = [_launch(ctx, monkeypatch, 'dense', ops), _launch(ctx, monkeypatch, 'bits', ops, 0)]
    for g, name in zip(got, ('dense', 'bits')):
      CC.check(g, case, f'{name} with j kept {pattern} {plan}')
    assert got[0].tobytes() == got[1].tobytes()


# ---- non-finite partials


def _walk_sites(ctx, monkeypatch, plan, forms, pattern='boxes', shift=0):
  """One non-finite partial at each site in turn, NaN, +inf and -inf rotating, bk and the lane rotating with the site; `forms` =
  [(form, patch_min)].  -> the labels of the sites walked."""
  base = CC.make_case(plan, 'rounded', pattern)
  labels = []
  for form, patch_min in forms:
    r = CC.route(plan, form, patch_min, base.bits)
    rows = r.info.get('rows', [plan.nBr])
    for b in range(plan.nBk):
      for i, (label, site) in enumerate(CC.nonfinite_sites(plan, base.member, rows, b)):
        value = VALUES[(i + b + shift) % 3]
        row = (plan.nA - 1, b, (i + shift) % plan.nlane)
        partial, on_bits, on_dense = CC.nonfinite_case(base, value, site, row)
        got = _launch(ctx, monkeypatch, form, _Operands(ctx, base, partial), patch_min)
        what = f'{r.name} {value} at {label} {site} of row {row}, {plan}'
        CC.check_nonfinite(got, on_dense if form == 'dense' else on_bits, base, what)
        labels.append(label)
  return set(labels)


ALL_SITES = {'first row of a split', 'last row of an odd-length split', 'last row of an even-length split', 'tail lane of the last x tile',
             'a chunk other than 0', 'a point that belongs to no bin'}


@pytest.mark.parametrize('nl', CC.PATCH_LANES)
def test_a_non_finite_partial_under_the_patch_kernel_poisons_its_row_and_nothing_else(ctx, monkeypatch, nl):
  """NaN and +-inf alike: NaN in every bin of the row -- also from a patch whose union is empty (bk 0: the tail tile, bk 1: tile 0),
  from a point in no bin and into bins without members.  Splits of 33 + 32 rows with three chunks, and of 34 + 33 rows with one
  (two rows in flight: the last row of an odd split is fetched alone)."""
  i = CC.PATCH_LANES.index(nl)
  seen = _walk_sites(ctx, monkeypatch, Plan(3, 2, 65, 3, nl, 65, 34), [('bits', 0)], shift=i)
  seen |= _walk_sites(ctx, monkeypatch, Plan(3, 2, 67, 1, nl, 130, 64), [('bits', 0)], shift=i + 1)
  assert seen == ALL_SITES


def test_a_non_finite_partial_in_a_one_row_patch(ctx, monkeypatch):
  for nl, nchunk in ((1, 1), (4, 3), (12, 1)):
    seen = _walk_sites(ctx, monkeypatch, Plan(3, 2, 1, nchunk, nl, 65, 34), [('bits', 0)], shift=nl)
    assert 'tail lane of the last x tile' in seen and 'a point that belongs to no bin' in seen


def test_a_non_finite_partial_under_the_block_kernels_poisons_its_row_and_nothing_else(ctx, monkeypatch):
  """s2_bits_kernel: row blocks of 3, 3 and 1 rows; long rows in one-row blocks (64 bins: the high word); j kept: only that j."""
  for plan in (Plan(50, 2, 7, 2, 15, 1, 17), Plan(2, 2, 6, 2, 8, 70, 64), Plan(1, 2, 5, 3, 2, 257, 33, 0), Plan(2, 2, 9, 1, 3, 300, 5)):
    seen = _walk_sites(ctx, monkeypatch, plan, [('bits', CC.PATCH_OFF)])
    assert 'a point that belongs to no bin' in seen and 'first row of a split' in seen


def test_the_dense_route_keeps_an_infinity_in_the_bins_of_its_point(ctx, monkeypatch):
  """wbx_contract multiplies by W as it is: NaN * 0 = NaN in every bin of the row; +-inf * w = +-inf in the point's bins, NaN in
  the others -- on every dense route."""
  plans = (Plan(2, 2, 13, 2, 3, 5, 8), Plan(2, 2, 7, 2, 3, 70, 9), Plan(1, 1, 23, 2, 4, 1440, 3), Plan(2, 2, 33, 4, 2, 7, 34, 0),
           Plan(2, 2, 5, 2, 3, 65, 34, 0))
  names = set()
  for plan in plans:
    names.add(CC.route(plan, 'dense').name)
    _walk_sites(ctx, monkeypatch, plan, [('dense', CC.PATCH_OFF)])
  assert names == {'reduce/short', 'reduce/long', 'reduce/long+split', 'reduce/fixed_j', 'keepj'}


# ---- one scratch buffer per context


def test_stale_scratch_of_a_larger_launch_does_not_show_in_a_smaller_one(ctx, monkeypatch):
  """s2_scratch only grows: after a route that needs a large one (tmp | poison | atom tables of a four-split patch launch with
  12 lanes and 64 bins; the split buffer of the dense route), a different route on a small case and the same route on a smaller
  case read only what they wrote themselves."""
  order = [
      ('bits', 0, Plan(3, 2, 193, 3, 12, 70, 64), 'dense'),                # the largest patch scratch of the file
      ('bits', CC.PATCH_OFF, Plan(2, 2, 11, 2, 8, 3, 16), 'boxes'),         # another route, small
      ('bits', 0, Plan(3, 2, 1, 1, 12, 65, 34), 'boxes'),                  # the same route, one row, patches with an empty union
      ('bits', 0, Plan(1, 1, 2, 1, 12, 127, 1), 'tiles'),
      ('dense', CC.PATCH_OFF, Plan(1, 1, 23, 2, 1, 1440, 3), 'boxes'),      # 46 splits
      ('bits', 0, Plan(3, 2, 65, 1, 2, 65, 64), 'boxes'),
      ('dense', CC.PATCH_OFF, Plan(1, 1, 23, 1, 1, 2880, 2), 'dense'),      # the same route, 23 splits
      ('bits', CC.PATCH_OFF, Plan(50, 2, 7, 2, 15, 1, 17), 'dense'),        # row blocks of 3, 3, 1 through the scratch
      ('bits', CC.PATCH_OFF, Plan(2, 2, 9, 3, 1, 1, 1), 'boxes'),
  ]
  for kind in KINDS:
    for form, patch_min, plan, pattern in order:
      case = CC.make_case(plan, kind, pattern)
      got = _launch(ctx, monkeypatch, form, _Operands(ctx, case), patch_min)
      CC.check(got, case, f'{CC.route(plan, form, patch_min).name} {kind} {plan}')
  # and with a NaN left behind in tmp_poison by the larger launch
  plan = Plan(3, 2, 193, 3, 12, 70, 64)
  base = CC.make_case(plan, 'rounded', 'boxes')
  partial = base.partial.copy()
  partial[:, :, 100, 1, :, 5] = np.nan
  monkeypatch.setenv('WBX_S2_PATCH_MIN', '0')
  out = ctx.alloc(int(np.prod(plan.out_shape)) * 8)
  big = _Operands(ctx, base, partial)
  _hip.check(_call(ctx, 'bits', plan, big.partial, big.wt, big.bits, out), 'poisoned launch')
  assert np.isnan(ctx.download(out.ptr, plan.out_shape, np.float64)).all()
  for small in (Plan(3, 2, 65, 1, 12, 65, 34), Plan(3, 2, 1, 1, 12, 65, 64), Plan(3, 2, 130, 3, 2, 64, 34)):
    case = CC.make_case(small, 'exact', 'boxes')
    CC.check(_launch(ctx, monkeypatch, 'bits', _Operands(ctx, case), 0), case, f'after a poisoned launch: {small}')


# ---- entry checks


def _entry(ctx, form, plan, operands=True, out=True):
  """-> (rc, message, out as downloaded) of a call with 8-byte dummies for operands that are never read."""
  n = max(1, int(np.prod(plan.out_shape)) if min(plan.fields()[:7]) >= 0 else 1)
  buf = ctx.upload(np.full(n, CC.SENTINEL))
  dummy = ctx.upload(np.zeros(max(1, int(np.prod(plan.partial_shape)))))
  ops = (dummy, dummy, dummy) if operands else (None, None, None)
  rc = _call(ctx, form, plan, ops[0], ops[1], ops[2], buf if out else None)
  return rc, ctx.lib.wbx_last_error(), ctx.download(buf.ptr, (n,), np.float64)


def test_bin_counts_the_bit_mask_form_does_not_have_are_refused(ctx):
  for nbin in (0, 65, -1):
    rc, message, out = _entry(ctx, 'bits', Plan(1, 1, 2, 1, 1, 4, nbin))
    assert rc == -1 and b'handles 1..64 bins' in message and (out == CC.SENTINEL).all(), nbin
  for nbin in (1, 64):
    rc, _, out = _entry(ctx, 'bits', Plan(1, 1, 2, 1, 1, 4, nbin))
    assert rc == 0 and (out == 0.0).all()  # zero partials, no members


@pytest.mark.parametrize('form', ['dense', 'bits'])
def test_nothing_to_contract_gives_zeros_and_nothing_to_write_leaves_the_output(ctx, form):
  for sum_j in (1, 0):
    for plan in (Plan(2, 2, 0, 3, 2, 5, 3, sum_j), Plan(2, 2, 4, 0, 2, 5, 3, sum_j)):
      rc, _, out = _entry(ctx, form, plan, operands=False)  # operands may be NULL: nothing is read
      assert rc == 0 and (out == 0.0).all() and not np.signbit(out).any(), plan
  rc, _, out = _entry(ctx, form, Plan(2, 2, 4, 3, 2, 0, 3, 1), operands=False)  # j summed over no points
  assert rc == 0 and (out == 0.0).all()
  for plan in (Plan(0, 2, 4, 3, 2, 5, 3), Plan(2, 0, 4, 3, 2, 5, 3), Plan(2, 2, 4, 3, 0, 5, 3), Plan(2, 2, 4, 3, 2, 0, 3, 0)):
    rc, _, out = _entry(ctx, form, plan, operands=False, out=False)
    assert rc == 0, plan
    rc, _, out = _entry(ctx, form, plan)
    assert rc == 0 and (out == CC.SENTINEL).all(), plan
  if form == 'dense':
    rc, _, out = _entry(ctx, form, Plan(2, 2, 4, 3, 2, 5, 0))
    assert rc == 0 and (out == CC.SENTINEL).all()


@pytest.mark.parametrize('form', ['dense', 'bits'])
def test_null_pointers_and_negative_extents_are_refused(ctx, form):
  plan = Plan(2, 2, 4, 3, 2, 5, 3)
  rc, message, out = _entry(ctx, form, plan, operands=False)
  assert rc == -1 and (b'partial/W is NULL' if form == 'dense' else b'partial/wt/bits is NULL') in message and (out == CC.SENTINEL).all()
  rc, message, _ = _entry(ctx, form, plan, out=False)
  assert rc == -1 and b'out is NULL' in message
  rc, message, out = _entry(ctx, form, Plan(2, 2, -4, 3, 2, 5, 3))
  assert rc == -1 and b'negative extent' in message and (out == CC.SENTINEL).all()
  dummy = ctx.upload(np.zeros(1))
  struct = _hip.S2PlanStruct(*plan.fields())
  if form == 'dense':
    rc = ctx.lib.wbx_contract(ctx.handle, None, _ptr(dummy), _ptr(dummy), _ptr(dummy))
  else:
    rc = ctx.lib.wbx_contract_bits(None, C.byref(struct), _ptr(dummy), _ptr(dummy), _ptr(dummy), _ptr(dummy))
  assert rc == -1 and b'ctx/plan is NULL' in ctx.lib.wbx_last_error()
