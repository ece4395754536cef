"""CPU side of tests/test_gpu_ens_binned.py: everything in that file that is not a kernel is held here without a GPU.

  * The rotation of member counts, modes, routes, bin patterns, geometries, weights, layouts and value families reaches what the GPU
    file's docstring says: every (register bucket, MODE, route) instantiation of ens_atoms_kernel, and every member count under every
    MODE on both routes.
  * The case generator's own conditions, for EVERY case: the addressing handed to the kernel reads the intended elements (by the
    case's strides and by the plan's tables), no patch holds more than 32 words unless the case says so, every geometry has the
    property it is named for by the restated rules of wbx_patch.hpp, a case without a planted special point has >= 90 % of its outputs
    finite and not zero (a kernel that writes zeros cannot pass), the bounds are finite and small against the outputs, and one point
    dropped from a bin moves its count lane by more than the bound.
  * The lane bookkeeping restated (ens_binned_cases.flush_profile): the row stripes do make every wave flush mid-patch and add into
    table rows it has written before, the twin modes do write twin rows, the checker does not flush.
  * The expectation against an independent restatement of the aggregation through oracle.wbx_oracle.aggregate, and the special
    points' effects (which lanes turn NaN, which counts drop by the point's weight) against the rule in words.
  * The GPU file's test bodies on the plan interpreter (tests/fake_device.py: _run_ens_binned) in place of the launches: flags, lane
    layouts, strides and weights.  The interpreter knows no patches: a patch never overflows there, and the 33-word rule is given to
    it in the expectation's own words.
  * Mutations of the interpreter, each of which must make a GPU test body fail: the twin half dropped, the per-point mask read at the
    row of (bk, br) instead of (cell, r), lane 3 formed with 1 / (M - 1), the points of the last record of every level-2 group dropped,
    the points whose word is the 32nd of its patch dropped; and the restated split table without its shaved first split no longer
    tiles the Br rows."""
import types

import numpy as np
import pytest

from oracle import wbx_oracle as O
from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
import ens_binned_cases as BC
import ensemble_cases as EC
import fake_device
import test_gpu_ens_binned as GB

ALL = BC.all_cases()
IDS = [c.name for c in ALL]


# ---- the rotation -----------------------------------------------------------------------------------------------------------------
def test_the_rotation_reaches_every_instantiation_and_every_member_count():
  cases = BC.all_matrix_cases()
  reached = {(BC.bucket_of(c.M), BC.kernel_mode(c.mode), c.ragged) for c in cases}
  want = {(b, mode, ragged) for b in BC.BUCKET_NAMES for mode in (0, 1, 2) for ragged in (False, True)}
  assert reached == want and len(want) == 42, sorted(want - reached)
  per_m = {(c.M, BC.kernel_mode(c.mode), c.ragged) for c in cases}
  assert per_m == {(m, mode, ragged) for m in BC.MEMBER_COUNTS for mode in (0, 1, 2) for ragged in (False, True)}
  assert set(BC.MEMBER_COUNTS) == {m for ms in BC.BUCKETS.values() for m in ms}
  for mode in BC.MODE_NAMES:
    mine = [c for c in cases if c.mode == mode]
    assert {c.bins for c in mine} == set(BC.PATTERNS), mode
    assert {c.geom for c in mine} >= {'ragged-3-tiles', 'two-level-2-groups', 'two-level-2-groups-ragged', 'tapered'}, mode
    assert {c.wl for c in mine} == set(BC.WEIGHTS), mode
    assert {c.values for c in mine} == set(BC.VALUES) and {c.layout for c in mine} == set(BC.LAYOUTS), mode
    assert {c.fair for c in mine} == {True, False}, mode
  assert {c.mode for c in BC.word_cases()} == {c.mode for c in BC.special_cases()} == set(BC.MODE_NAMES)
  assert {BC.lanes_total(c.mode) for c in BC.accumulate_cases()} == {6, 12, 10, 20}
  assert len({c.name for c in ALL}) == len(ALL)


def test_fair_layouts_and_values_of_the_named_geometries():
  geoms = {c.geom for c in BC.geometry_cases()}
  assert geoms == {'one-patch', 'ragged-3-tiles', 'strided-x', 'target-without-x', 'two-level-2-groups', 'two-level-2-groups-ragged', 'tapered',
                   'depth-2-untapered', 'nBk-3', 'nj-1', 'nbin-64', 'nbin-1'}
  for c in BC.geometry_cases() + BC.all_matrix_cases():
    BC.geometry_property(c)


def test_the_split_table_without_its_shaved_first_split_does_not_tile_the_rows(monkeypatch):
  """patch_taper restated: 70 Br rows in eight segments of 9 and 8; the mutation `skip the first-split shave` gives 72."""
  assert BC.patch_taper(70, 4) == tuple(np.cumsum([0] + [4, 2, 2, 1] * 6 + [3, 2, 2, 1] * 2).tolist())
  assert BC.patch_taper(64, 4)[-1] == 64 and BC.patch_taper(63, 4) is None and BC.patch_taper(70, 3) is None
  sizes = np.diff(BC.patch_taper(70, 4)).reshape(8, 4)
  assert (sizes.sum(axis=1) == [9] * 6 + [8] * 2).all()


# ---- every case: addressing, words, outputs, bounds ---------------------------------------------------------------------------------
class _Dev:
  def __init__(self, arr, layout=None):
    self.ptr, self.layout = arr, layout


def _devs(inp):
  devs = []
  for name in ('p', 't', 'c', 'mask'):
    if name in inp.store:
      flat, st = inp.store[name]
      devs.append(_Dev(flat, planner.InputLayout(strides=dict(st), itemsize=flat.itemsize, base_alignment=256)))
    else:
      devs.append(None)
  return devs


@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_the_case_is_what_it_says(case):
  inp, exp = BC.prepared(case)
  g = inp.geometry
  # addressing: by the strides of the case, and by the tables the planner hands the kernel
  np.testing.assert_array_equal(BC.read_back(inp, 'p'), inp.P)
  np.testing.assert_array_equal(BC.read_back(inp, 't'), inp.T)
  if 'mask' in inp.store:
    np.testing.assert_array_equal(BC.read_back(inp, 'mask') != 0, inp.valid)
  plan = BC.plan_for(inp)
  for i, name in enumerate(('p', 't', 'c', 'mask')):
    if name in inp.store:
      flat, st = inp.store[name]
      got = flat[fake_device._offsets(plan, i)].reshape(case.ncell, case.R, case.nx)  # pylint: disable=protected-access
      want = {'p': inp.P[:, 0], 't': inp.T, 'mask': inp.valid}[name]
      np.testing.assert_array_equal(got != 0 if name == 'mask' else got, want, err_msg=name)
      assert plan.xstride[i] == st['x']
  assert plan.flags == case.plan_flags and case.ragged == ((plan.nx * plan.xstride[0] * 4) % 128 != 0 or plan.xstride[0] != 1)
  # words
  words = g.words(inp.bits)
  if case.bins == '33-words':
    assert (words[0] <= BC.ATOM_MAX).all() and (words[1:] == BC.ATOM_MAX + 1).all()
  else:
    assert words.max() <= BC.ATOM_MAX, words.max()
  if case.bins == 'exactly-32-words':
    assert words.max() == BC.ATOM_MAX
  if case.bins == 'boxes':
    n = BC.member_of(inp.bits, case.nbin).sum(axis=-1)
    assert (n == 0).any() and (n >= 2).any(), 'boxes: points in no bin and points in several'
  if case.nbin == 64:
    assert (inp.bits >> np.uint64(63)).any()
  assert case.bins == '33-words' or BC.member_of(inp.bits, case.nbin).any(axis=(1, 2)).all(), 'no bin is empty in any bk'
  # outputs and bounds
  assert exp.want.shape == (case.nA, case.nBk, BC.lanes_total(case.mode), case.nbin)
  assert not np.isinf(exp.want).any() and np.isfinite(exp.bound).all() and (exp.bound >= 0).all()
  live = exp.want[:, :, ~exp.layout_nan]
  if not case.special and case.bins != '33-words':
    assert np.isfinite(live).all()
    assert (live != 0).mean() >= 0.9, ('outputs that are finite and not zero', float((live != 0).mean()))
  if BC.MODES[case.mode][0] & BC.FLAG_SKIPNA:
    bad, tnan = BC.point_selections(inp)
    assert np.isfinite(live).all() and bad.any() and tnan.any(), 'under skipna every output is finite, and there are NaNs to skip'
  fin = np.isfinite(exp.want) & ~exp.exact & (exp.scale > 0)
  if case.values == 'cancel':  # (the target cancels against the ensemble mean: lanes 3 and 4 are small against their own bound by design)
    block = np.arange(exp.want.shape[2]) % (10 if BC.MODES[case.mode][0] & BC.FLAG_SKIPNA else 6)
    fin = fin & ~np.isin(block, (3, 4))[None, None, :, None]
  # (the fp64 buckets: a few thousand terms x 2^-53; the fp32 chains: 9 x 2^-24 of the lanes' own scale)
  assert (exp.bound[fin] <= (2e-5 if case.M in (50, 51) else 1e-10) * exp.scale[fin]).all(), float((exp.bound[fin] / exp.scale[fin]).max())
  # one point dropped from a bin, or counted twice, moves the bin's count lane by more than its bound
  counts = [5, 11] if exp.want.shape[2] in (6, 12) else list(range(5, 10)) + list(range(15, 20))
  counts = [l for l in counts if l < exp.want.shape[2]]
  wmin = float(inp.W.min())
  assert (exp.bound[:, :, counts] < 0.5 * wmin).all()


def test_the_lane_bookkeeping_the_patterns_are_made_for():
  """flush_all mid-patch, adds into touched table rows, twin rows -- and their absence where the pattern leaves two atoms per lane."""
  prof = lambda name: BC.flush_profile(BC.prepared(GB._named(name))[0])  # pylint: disable=protected-access
  stripes = prof('plain-m16-whole-two-level-2-groups')
  assert GB._named('plain-m16-whole-two-level-2-groups').bins == 'row-stripes'  # pylint: disable=protected-access
  assert stripes['mid'] > 0 and stripes['retouched'] > 0 and stripes['max_atoms'] == 3 and stripes['twin_rows'] == 0, stripes
  tapered = prof('geom-tapered-masked-pt-twin')  # row stripes under a twin mask: six ids down a lane, twin rows in every patch
  assert tapered['mid'] > 0 and tapered['retouched'] > 0 and tapered['max_atoms'] >= 5 and tapered['twin_rows'] > 0, tapered
  checker = [c for c in BC.all_matrix_cases() if c.mode == 'plain' and c.bins == 'checker']
  for c in checker:
    p = BC.flush_profile(BC.prepared(c)[0])
    assert p['mid'] == 0 and p['max_atoms'] == 2, (c.name, p)
  w32 = prof('words-32-plain')
  assert w32['mid'] > 0 and w32['retouched'] > 0, w32
  skip = prof('skipna-m8-ragged-ragged-3-tiles')  # NaN targets go to their atom's twin
  assert skip['twin_rows'] > 0, skip
  for mode in BC.MODE_NAMES:
    total = dict(mid=0, retouched=0, twin_rows=0)
    for c in BC.all_matrix_cases():
      if c.mode == mode and c.geom in ('ragged-3-tiles', 'tapered'):
        p = BC.flush_profile(BC.prepared(c)[0])
        total = {k: total[k] + p[k] for k in total}
    assert total['mid'] > 0 and total['retouched'] > 0 and (total['twin_rows'] > 0) == (mode not in ('plain', 'masked-w', 'masked-pt')), (mode, total)


# ---- the expectation against the oracle's aggregation -------------------------------------------------------------------------------
def _aggregate(inp, stat_l, valid, skipna):
  """oracle.wbx_oracle.aggregate over runs of at most 4096 points of a cell (the einsum adds in float64 in an order of its own: its
  rounding grows with the number of terms), the runs added in extended precision."""
  case = inp.case
  dims = ('a', 'bk', 'r', 'x')
  shape = (case.nA, case.nBk, case.R, case.nx)
  member = BC.member_of(inp.words, case.nbin)
  stat_l = stat_l.reshape(shape)
  valid = None if valid is None else valid.reshape(shape)
  step = max(1, 4096 // case.nx)
  sws = sw = None
  for r0 in range(0, case.R, step):
    rs = slice(r0, r0 + step)
    a, b, od = O.aggregate(stat_l[:, :, rs], dims, ['r', 'x'], weights=[(inp.W[:, rs], ('bk', 'r', 'x'))],
                           bin_masks=[('bin', member[:, rs], ('bk', 'r', 'x', 'bin'))], mask=None if valid is None else valid[:, :, rs], mask_dims=dims,
                           skipna=skipna)
    assert od == ('a', 'bk', 'bin')
    sws = a.astype(BC.LD) if sws is None else sws + a
    sw = b.astype(BC.LD) if sw is None else sw + b
  return sws.astype(np.float64), sw.astype(np.float64)


@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_expectation_against_the_oracles_aggregate(case):
  """The aggregation restated through oracle.wbx_oracle.aggregate (as tests/test_ens_binned.py::_check_lanes does): NaN at the same
  places, and the finite outputs equal to 1e-13 relative -- relative to sum |w lane|, the scale of the float64 einsum's own rounding:
  lane 3 takes both signs point by point, so its sum can cancel (one such output sits at 1.1e-13 of its own magnitude and at 1e-15 of
  the scale); for a lane without cancellation the scale IS the output's magnitude."""
  inp, exp = BC.prepared(case)
  fam = EC.family('binned', case.M, np.float32)
  stat = EC.expected_lanes(fam, inp.P, inp.T, case.fair)
  flags, bflags, kind = BC.MODES[case.mode]
  skipna, twin = bool(flags & BC.FLAG_SKIPNA), bool(bflags & BC.TWIN_MASK)
  valid = None if kind is None else inp.valid
  got = np.full(exp.want.shape, np.nan)
  for l in range(5):
    sws, sw = _aggregate(inp, stat[..., l], valid, skipna)
    sws_all, sw_all = _aggregate(inp, stat[..., l], None, skipna) if twin else (None, None)
    if not skipna:
      got[:, :, l], got[:, :, 5] = sws, sw
      if twin:
        got[:, :, 6 + l], got[:, :, 11] = sws_all, sw_all
    elif not twin:
      got[:, :, l], got[:, :, 5 + l] = sws, sw
    else:
      if l in (0, 3, 4):
        got[:, :, l] = sws
        if l == 0:
          got[:, :, 5:10] = sw[:, :, None]
      else:
        got[:, :, 10 + l] = sws_all
        if l == 1:
          got[:, :, 15:20] = sw_all[:, :, None]
  if case.bins == '33-words':
    got, want, scale = got[:, :1], exp.want[:, :1], exp.scale[:, :1]
  else:
    want, scale = exp.want, exp.scale
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
  fin = np.isfinite(want)
  assert (np.abs(got - want)[fin] <= 1e-13 * np.maximum(scale, np.abs(want))[fin]).all(), float((np.abs(got - want)[fin] / np.maximum(scale, np.abs(want))[fin]).max())


@pytest.mark.parametrize('case', BC.special_cases(), ids=lambda c: c.name)
def test_special_points_do_to_the_expectation_what_the_header_says(case):
  """Which lanes of which cell are NaN, and, under skipna, which count lanes lose exactly the point's weight in the bins it is in."""
  inp, exp = BC.prepared(case)
  flags, bflags, kind = BC.MODES[case.mode]
  want = exp.want.reshape(case.ncell, -1, case.nbin)
  member = BC.member_of(inp.words, case.nbin).astype(np.float64)  # [nBk, R, nx, nbin]
  assert len(inp.special) == 12 and {(k, p) for k, p, _, _ in inp.special.values()} == {(k, p) for k in BC.SPECIAL_KINDS for p in BC.SPECIAL_PLACES}
  for cell, (name, place, r, x) in inp.special.items():
    bk = cell % case.nBk
    eff = BC.special_effects(case.mode, name, place)
    nan = np.isnan(want[cell])
    assert (nan.any(axis=1) == nan.all(axis=1)).all()
    assert set(np.nonzero(nan.all(axis=1) & ~exp.layout_nan)[0].tolist()) == eff['nan'], (cell, name, place)
    assert inp.valid[cell, r, x] == (not (place == 'masked_out' and kind is not None))
    assert (inp.words[bk, r, x] == 0) == (place == 'no_bin') and (place != 'tail' or x == case.nx - 1)
    if flags & BC.FLAG_SKIPNA:
      for lane in range(5, want.shape[1]):
        if exp.layout_nan[lane - 5]:
          pass  # (the count lane of a NaN lane repeats a live one: held below all the same)
        if 10 <= lane < 15:
          continue
        base = inp.valid[cell] if lane < 10 else np.ones_like(inp.valid[cell])
        full = np.einsum('rx,rxb->b', np.where(base, inp.W[bk], 0.0), member[bk])
        lost = inp.W[bk, r, x] * member[bk, r, x] if lane in eff['drops'] else 0.0
        np.testing.assert_allclose(want[cell, lane], full - lost, rtol=1e-12, err_msg=str((cell, name, place, lane)))
  assert np.isfinite(want[12:][:, ~exp.layout_nan]).all()


# ---- the GPU file's test bodies on the plan interpreter ------------------------------------------------------------------------------
def _poisoned_ens_lanes(orig):
  """fake_device._ens_lanes with the convention of include/wbx.h the interpreter does not carry: in the float32 rank form an
  infinite member poisons all five lanes like a NaN member does."""
  def lanes(plan, devs, ens, flags):
    m, mstride, _ = ens
    off = fake_device._offsets(plan, 0)  # pylint: disable=protected-access
    bad = ~np.isfinite(np.stack([devs[0].ptr[off + k * mstride] for k in range(m)], axis=-1)).all(axis=-1)
    return [np.where(bad, np.nan, l) for l in orig(plan, devs, ens, flags)]
  return lanes


def _emulated_launch(ctx, job, atoms=None, extra=0, init=GB.SENTINEL, empty=False):
  case, inp = job.case, job.inp
  init = np.array(np.broadcast_to(np.asarray(init, np.float64), job.shape))
  accumulate = bool(extra & _hip.BINNED_ACCUMULATE)
  if empty:
    return 0, (init if accumulate else np.zeros(job.shape))
  bits = ctx.bits_of(inp) if ctx.bits_of is not None else inp.bits
  flag = case.w_flags & (_hip.BINNED_WT_X_ONLY | _hip.BINNED_WT_ROW_ONLY)
  fac = inp.wt if inp.wt is not None else np.ones((case.nBk, case.nBr))
  w_buf = types.SimpleNamespace(shape=(case.nBk, case.nBr, case.nj, case.nbin), factored=(flag, _Dev(fac)), bufs=[None, _Dev(bits)])
  out, shape = fake_device._run_ens_binned(ctx, None, job.plan, _devs(inp), _hip.F32, (case.M, inp.mstride, _hip.ENS_SORT), w_buf, (case.w_flags | extra, None))  # pylint: disable=protected-access
  assert shape == job.shape[:3] + (1, case.nbin)
  res = out[:, :, :, 0, :]
  over = inp.geometry.words(inp.bits).reshape(case.nBk, -1).max(axis=1) > BC.ATOM_MAX
  res[:, over] = np.nan  # (the documented return of a patch with more than 32 words; the interpreter has no patches)
  with np.errstate(invalid='ignore'):
    return 0, (init + res if accumulate else res)


def _emulated_tables(ctx, job):
  return None, int((job.inp.geometry.words(job.inp.bits) > BC.ATOM_MAX).sum())


@pytest.fixture
def emu(monkeypatch):
  """The GPU file's launches replaced by the interpreter; plans are built by the planner exactly as on the GPU."""
  monkeypatch.setattr(engine, '_PlanOnDevice', lambda ctx, plan: None)
  monkeypatch.setattr(fake_device, '_ens_lanes', _poisoned_ens_lanes(fake_device._ens_lanes))  # pylint: disable=protected-access
  monkeypatch.setattr(GB, '_launch', _emulated_launch)
  monkeypatch.setattr(GB, '_tables', _emulated_tables)
  monkeypatch.setattr(GB, '_atoms_size', lambda ctx, job: job.inp.geometry.atoms_bytes)
  monkeypatch.setattr(GB, 'WORST', {})
  ctx = fake_device.FakeCtx()
  ctx.bits_of = None
  return ctx


@pytest.mark.parametrize('bucket', BC.BUCKET_NAMES)
@pytest.mark.parametrize('mode', BC.MODE_NAMES)
def test_mode_and_bucket_cases_on_the_interpreter(emu, mode, bucket):
  GB.test_every_output_of_every_mode_and_bucket_on_both_routes(emu, mode, bucket)


def test_the_other_cases_on_the_interpreter(emu):
  for case in BC.geometry_cases():
    GB.test_named_geometries(emu, case)
  for case in BC.word_cases():
    GB.test_exactly_32_words_in_a_patch(emu, case)
  for case in BC.overflow_cases():
    GB.test_33_words_turn_the_cells_of_their_bk_nan_and_no_other(emu, case)
  for case in BC.special_cases():
    GB.test_special_points_reach_the_lanes_of_their_cell_and_nothing_else(emu, case)
  for prefix in GB.PREPARED:
    GB.test_prepared_tables_give_the_same_bits_as_atoms_null(emu, prefix)
  for case in BC.accumulate_cases():
    GB.test_accumulate_adds_into_out_and_an_empty_reduction_leaves_it(emu, case)
  GB.test_a_launch_of_another_geometry_leaves_the_context_as_it_found_it(emu, 'plain-m16-whole-two-level-2-groups', 'words-33-plain')


# ---- mutations of the interpreter: each must make a GPU test body fail --------------------------------------------------------------
def _twin_half_dropped(monkeypatch):
  """`drop the twin half in the level-1 sum`: the second six / ten repeat the masked sums."""
  orig = fake_device._run_ens_binned  # pylint: disable=protected-access
  def run(ctx, dplan, plan, devs, dtype_code, ens_args, w_buf, route):
    out, shape = orig(ctx, dplan, plan, devs, dtype_code, ens_args, w_buf, route)
    if route[0] & _hip.BINNED_TWIN_MASK and not plan.flags & _hip.FLAG_SKIPNA:
      out[:, :, 6:] = out[:, :, :6]
    elif route[0] & _hip.BINNED_TWIN_MASK:
      keep = np.isnan(out[:, :, 10:])
      out[:, :, 10:] = np.where(keep, np.nan, np.where(np.isnan(out[:, :, :10]), out[:, :, 5:6], out[:, :, :10]))
    return out, shape
  monkeypatch.setattr(fake_device, '_run_ens_binned', run)


def _mask_row_of_bk_br(monkeypatch):
  """`br_a instead of r_a for the per-point id row`: the mask byte of (a = 0, d = 0) for every (a, d)."""
  orig = fake_device._offsets  # pylint: disable=protected-access
  def offsets(plan, i):
    off = orig(plan, i)
    if i == 3:
      nA = plan.n(plan.a_dims)
      o5 = off.reshape(nA, -1, plan.ndepth, plan.nx)
      off = np.broadcast_to(o5[:1, :, :1, :], o5.shape).reshape(off.shape)
    return off
  monkeypatch.setattr(fake_device, '_offsets', offsets)


def _lane3_with_m_minus_1(monkeypatch):
  orig = fake_device._ens_lanes  # pylint: disable=protected-access
  def lanes(plan, devs, ens, flags):
    out = orig(plan, devs, ens, flags)
    m = ens[0]
    out[3] = out[4] - out[2] / (m - 1)
    return out
  monkeypatch.setattr(fake_device, '_ens_lanes', lanes)


def _patches_of(inp, pick):
  """bits with the points of the patches pick(rs, xt) in no bin."""
  g, bits = inp.geometry, inp.bits.copy()
  for rs in range(g.nrs):
    for xt in range(g.nxt):
      if pick(rs * g.nxt + xt):
        bits[:, g.split_br[rs]:g.split_br[rs + 1], (slice(64 * xt, 64 * xt + 64) if g.nj > 1 else slice(0, 1))] = 0
  return bits


def _last_level2_record_dropped(inp):
  """`sum qn - 1 records at level 2`: the last level-1 group of every level-2 group adds nothing."""
  g = inp.geometry
  def pick(patch):
    g1 = patch // BC.G1
    q0 = g1 // BC.G2 * BC.G2
    return g1 == min(q0 + BC.G2, g.ng1) - 1
  return _patches_of(inp, pick)


def _id_31_is_none(inp):
  """`treat id 31 as NONE`: the points whose word is the 32nd of its patch's list (in the order binned_atoms_kernel meets them: row by
  row, lane by lane) are in no sum."""
  g, bits = inp.geometry, inp.bits.copy()
  for bk in range(g.nBk):
    for rs in range(g.nrs):
      for xt in range(g.nxt):
        xs = slice(64 * xt, 64 * xt + g.live(xt)) if g.nj > 1 else slice(0, 1)
        tile = bits[bk, g.split_br[rs]:g.split_br[rs + 1], xs]
        seen = list(dict.fromkeys(tile.reshape(-1).tolist()))
        if len(seen) >= 32:
          tile[tile == seen[31]] = 0
  return bits


MUTATIONS = {
    'twin-half-dropped': (_twin_half_dropped, None, [('matrix', 'masked-w-twin', 'm8'), ('matrix', 'skipna-masked-pt-twin', 'm50')]),
    'mask-row-of-bk-br': (_mask_row_of_bk_br, None, [('matrix', 'masked-pt', 'm51'), ('matrix', 'skipna-masked-pt', 'm64')]),
    'lane-3-with-m-minus-1': (_lane3_with_m_minus_1, None, [('matrix', 'plain', 'm64'), ('matrix', 'skipna', 'm16')]),
    'last-level-2-record-dropped': (None, _last_level2_record_dropped, [('matrix', 'plain', 'm16'), ('matrix', 'skipna-masked-w-twin', 'm4')]),
    'id-31-is-none': (None, _id_31_is_none, [('words', 0), ('words', 7)]),
}


@pytest.mark.parametrize('name', list(MUTATIONS))
def test_a_mutated_interpreter_fails_the_gpu_test_bodies(emu, monkeypatch, name):
  patch, bits_of, targets = MUTATIONS[name]
  for target in targets:  # the unmutated interpreter passes them ...
    _run_target(emu, target)
  if patch is not None:
    patch(monkeypatch)
  emu.bits_of = bits_of
  for target in targets:  # ... the mutated one fails every one of them
    with pytest.raises(AssertionError):
      _run_target(emu, target)


def _run_target(emu, target):
  if target[0] == 'matrix':
    GB.test_every_output_of_every_mode_and_bucket_on_both_routes(emu, target[1], target[2])
  else:
    GB.test_exactly_32_words_in_a_patch(emu, BC.word_cases()[target[1]])
