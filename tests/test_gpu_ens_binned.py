"""wbx_ens_binned (ens_atoms_kernel) through the raw C ABI: EVERY output out[a][bk][lane][bin] of every case of
tests/ens_binned_cases.py against its float64 expectation -- NaN at the same positions, no infinity anywhere, the outputs the cases
mark exact bit for bit, every other one within the bound computed per output from the inputs (sum w lane_bounds + (N + 4) 2^-53 sum
|w lane|, derived there).  The output buffer is pre-filled with a sentinel; the largest |error| / bound of every case is printed.
The cases themselves, the geometry each one is named for and the expectation are held on the CPU by tests/test_ens_binned_cases.py,
which also runs the test bodies of this file on the plan interpreter; here every launch also holds wbx_ens_binned_atoms_size
against the restated patch geometry, so a drift between the restatement and the library fails instead of un-aiming the cases.

(a) output mode (6 / 12 / 10 / 20 lanes: plain, a mask on the W dims or per point, twin output, skipna) x register bucket (4, 8, 16, 32,
64, and the fp32-chain instantiations 50 and 51), each pair on the ragged route (four-wave blocks) and on whole lines (lone
non-temporal waves), over overlapping boxes, row stripes (a flush every third row) and a checker, row / x / NULL weights, two member
layouts and three value families; (b) the named geometries: one patch, three tiles with a ragged tail, strided members, a target
without x, two level-2 groups, the tapered split table with its shaved first split, depth rows, nBk = 3, W without x, 64 bins and
one; (c) exactly 32 words in a patch; (d) 33 words in the patches of one bk: the documented NaN cells, the others untouched by it;
(e) NaN / infinite members and NaN targets at a valid point, a masked-out point, a point in no bin and the last live x; (f) prepared
atom tables against atoms = NULL; (g) a launch of another geometry between two launches of one case; (h) WBX_BINNED_ACCUMULATE and
an empty reduction."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
import ens_binned_cases as BC
import test_gpu_round4 as R4

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
WORST = {}  # mode -> (largest |error| / bound, case): what profiles/ens_binned_tests_timing.txt records


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


# ---- plumbing (tests/test_ens_binned_cases.py replaces _atoms_size, _tables and _launch by the plan interpreter) --------------
def _job(ctx, case):
  """The device side of one case: plan, inputs, weights, membership words."""
  inp, exp = BC.prepared(case)
  plan = BC.plan_for(inp)
  job = types.SimpleNamespace(case=case, inp=inp, exp=exp, plan=plan, dplan=engine._PlanOnDevice(ctx, plan), bufs=None,  # pylint: disable=protected-access
                              shape=(case.nA, case.nBk, BC.lanes_total(case.mode), case.nbin))
  return job


def _upload(ctx, job):
  if job.bufs is None:
    inp = job.inp
    job.bufs = {name: ctx.upload(inp.store[name][0]) for name in inp.store}
    job.bufs['wt'] = None if inp.wt is None else ctx.upload(inp.wt)
    job.bufs['bits'] = ctx.upload(inp.bits)
    job.bufs.setdefault('mask', None)
  return job.bufs


def _atoms_size(ctx, job):
  n = C.c_int64(-1)
  case = job.case
  _hip.check(ctx.lib.wbx_ens_binned_atoms_size(C.byref(job.dplan.struct), case.nA, case.nBk, case.nBr, case.w_flags, C.byref(n)), 'wbx_ens_binned_atoms_size')
  return int(n.value)


def _tables(ctx, job):
  """-> (the prepared atom tables, the number of patches wbx_ens_binned_atoms reports as overflowing)"""
  case, bufs = job.case, _upload(ctx, job)
  tables = ctx.alloc(_atoms_size(ctx, job))
  overflow = C.c_int64(-1)
  _hip.check(ctx.lib.wbx_ens_binned_atoms(ctx.handle, C.byref(job.dplan.struct), case.nA, case.nBk, case.nBr, case.w_flags, C.c_void_p(bufs['bits'].ptr),
                                          C.c_void_p(tables.ptr), C.byref(overflow)), 'wbx_ens_binned_atoms')
  return tables, int(overflow.value)


def _launch(ctx, job, atoms=None, extra=0, init=SENTINEL, empty=False):
  """One wbx_ens_binned launch -> (rc, out[nA][nBk][lanes][nbin]); `out` starts as `init` (a value or an array); `empty`: the plan
  says ndepth = 0."""
  case, bufs = job.case, _upload(ctx, job)
  out = ctx.upload(np.ascontiguousarray(np.broadcast_to(np.asarray(init, np.float64), job.shape)))
  plan, dplan = job.plan, job.dplan
  if empty:
    plan = dataclasses.replace(job.plan, ndepth=0)
    dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  rc = R4._raw_call(ctx, plan, dplan, case.M, job.inp.mstride, bufs['p'], bufs['t'], bufs['mask'], bufs['wt'], bufs['bits'], case.nA, case.nBk,  # pylint: disable=protected-access
                    case.nBr, case.w_flags | extra, case.nbin, atoms, out)
  return rc, ctx.download(out.ptr, job.shape, np.float64)


def _same_bits(a, b):
  return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _compare(got, exp, case, what='', only=None):
  """Every output (`only`: a boolean [nA][nBk] choice of cells) by class, bit for bit or within its bound -> largest error / bound."""
  what = f'{case.name} {what}'.strip()
  want, bound, exact = exp.want, exp.bound, exp.exact
  if only is not None:
    got, want, bound, exact = got[only], want[only], bound[only], exact[only]
  assert not np.isinf(got).any(), (what, 'an infinite output', np.argwhere(np.isinf(got))[:4].tolist())
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{what}: NaN positions')
  fin = ~np.isnan(want)
  np.testing.assert_array_equal(got[fin & exact], want[fin & exact], err_msg=f'{what}: count lanes and dyadic sums, bit for bit')
  rest = fin & ~exact
  err = np.abs(got[rest] - want[rest])
  with np.errstate(all='ignore'):
    ratio = np.where(err == 0, 0.0, err / bound[rest])
  worst = float(ratio.max()) if ratio.size else 0.0
  print(f'{what}: largest |got - want| / bound = {worst:.3f}')
  if worst > WORST.get(case.mode, (-1.0, ''))[0]:
    WORST[case.mode] = (worst, case.name)
  bad = err > bound[rest]
  assert not bad.any(), (what, 'outputs beyond the bound', int(bad.sum()), 'first [a, bk, lane, bin]', np.argwhere(rest)[bad][:4].tolist(),
                         'got', got[rest][bad][:4].tolist(), 'want', want[rest][bad][:4].tolist(), 'bound', bound[rest][bad][:4].tolist(), worst)
  return worst


def _check(ctx, case, atoms=None):
  job = _job(ctx, case)
  assert _atoms_size(ctx, job) == job.inp.geometry.atoms_bytes, (case.name, 'wbx_ens_binned_atoms_size against the restated geometry')
  rc, got = _launch(ctx, job, atoms=atoms)
  _hip.check(rc, case.name)
  _compare(got, job.exp, case)
  return job, got


# ---- (a)
@pytest.mark.parametrize('bucket', BC.BUCKET_NAMES)
@pytest.mark.parametrize('mode', BC.MODE_NAMES)
def test_every_output_of_every_mode_and_bucket_on_both_routes(ctx, mode, bucket):
  cases = BC.matrix_cases(mode, bucket)
  assert [c.ragged for c in cases] == [True, False] and all(BC.bucket_of(c.M) == bucket and c.mode == mode for c in cases)
  for case in cases:
    _check(ctx, case)


# ---- (b)
@pytest.mark.parametrize('case', BC.geometry_cases(), ids=lambda c: c.name)
def test_named_geometries(ctx, case):
  BC.geometry_property(case)
  _check(ctx, case)


# ---- (c)
@pytest.mark.parametrize('case', BC.word_cases(), ids=lambda c: c.name)
def test_exactly_32_words_in_a_patch(ctx, case):
  job, direct = _check(ctx, case)
  assert job.inp.geometry.words(job.inp.bits).max() == BC.ATOM_MAX
  tables, overflow = _tables(ctx, job)
  assert overflow == 0
  rc, got = _launch(ctx, job, atoms=tables)
  _hip.check(rc, case.name)
  assert _same_bits(got, direct)


# ---- (d)
@pytest.mark.parametrize('case', BC.overflow_cases(), ids=lambda c: c.name)
def test_33_words_turn_the_cells_of_their_bk_nan_and_no_other(ctx, case):
  """The documented return for bins that are no boxes: wbx_ens_binned_atoms counts the patches, the cells of bk = 1 come back NaN in
  every lane and bin (prepared tables or not), the cells of bk = 0 stay within their bounds."""
  job = _job(ctx, case)
  words = job.inp.geometry.words(job.inp.bits)
  assert (words[0] <= BC.ATOM_MAX).all() and (words[1] == BC.ATOM_MAX + 1).all()
  tables, overflow = _tables(ctx, job)
  assert overflow == words[1].size > 0
  keep = np.zeros((case.nA, case.nBk), bool)
  keep[:, 0] = True
  for atoms in (tables, None):
    rc, got = _launch(ctx, job, atoms=atoms)
    _hip.check(rc, case.name)
    assert np.isnan(got[:, 1]).all()
    _compare(got, job.exp, case, 'bk = 0', only=keep)
    assert np.isfinite(job.exp.want[keep][:, ~job.exp.layout_nan]).all()


# ---- (e)
@pytest.mark.parametrize('case', BC.special_cases(), ids=lambda c: c.name)
def test_special_points_reach_the_lanes_of_their_cell_and_nothing_else(ctx, case):
  """Every output against the expectation (under skipna that is where the counts drop: the count lanes are held like every other
  output, and tests/test_ens_binned_cases.py holds the expectation's counts to the documented rule), and in words: which lanes of
  which cell are NaN -- in every bin or in none -- by ens_binned_cases.special_effects.  With twin output a NaN member under a
  masked-out point leaves lanes 0-5 finite and turns the value lanes of the second six NaN."""
  job, got = _check(ctx, case)
  layout = job.exp.layout_nan
  flat = got.reshape(case.ncell, -1, case.nbin)
  assert np.isfinite(flat[12:][:, ~layout]).all(), 'the cells without a special point'
  for cell, (name, place, _, _) in job.inp.special.items():
    nan = np.isnan(flat[cell]).all(axis=1)  # a NaN lane is NaN in every bin ...
    assert (np.isnan(flat[cell]).any(axis=1) == nan).all(), (cell, name, place)  # ... or in none
    assert set(np.nonzero(nan & ~layout)[0].tolist()) == BC.special_effects(case.mode, name, place)['nan'], (cell, name, place, np.nonzero(nan)[0])


# ---- (f)
PREPARED = ['plain-m16-whole-two-level-2-groups', 'masked-w-twin-m4-ragged-two-level-2-groups-ragged', 'masked-pt-m51-whole-tapered',
            'skipna-masked-pt-twin-m32-whole-tapered', 'skipna-m8-ragged-ragged-3-tiles', 'geom-nj-1-plain', 'geom-nBk-3-masked-w-twin']


def _named(prefix):
  (case,) = [c for c in BC.all_cases() if c.name.startswith(prefix + '-')]
  return case


@pytest.mark.parametrize('prefix', PREPARED)
def test_prepared_tables_give_the_same_bits_as_atoms_null(ctx, prefix):
  case = _named(prefix)
  job, direct = _check(ctx, case)
  tables, overflow = _tables(ctx, job)
  assert overflow == 0
  rc, got = _launch(ctx, job, atoms=tables)
  _hip.check(rc, case.name)
  assert _same_bits(got, direct), np.argwhere(got != direct)[:4]


# ---- (g)
@pytest.mark.parametrize('first,between', [('plain-m16-whole-two-level-2-groups', 'masked-pt-twin-m64-whole-tapered'),
                                           ('skipna-masked-w-twin-m50-ragged-ragged-3-tiles', 'words-33-plain'),
                                           ('geom-nBk-3-skipna-masked-pt-twin', 'plain-m4-ragged-two-level-2-groups-ragged')])
def test_a_launch_of_another_geometry_leaves_the_context_as_it_found_it(ctx, first, between):
  """The counters of the in-kernel sums are left zero by every launch (an overflowing one included), and the scratch of one geometry
  holds nothing the next launch reads: first and third launch bit-identical."""
  a, b = _named(first), _named(between)
  ja, one = _check(ctx, a)
  jb = _job(ctx, b)
  rc, mid = _launch(ctx, jb)
  _hip.check(rc, b.name)
  if b.bins != '33-words':
    _compare(mid, jb.exp, b)
  rc, three = _launch(ctx, ja)
  _hip.check(rc, a.name)
  assert _same_bits(one, three), np.argwhere(one != three)[:4]


# ---- (h)
@pytest.mark.parametrize('case', BC.accumulate_cases(), ids=lambda c: c.name)
def test_accumulate_adds_into_out_and_an_empty_reduction_leaves_it(ctx, case):
  job, res = _check(ctx, case)
  nan = np.isnan(res)
  assert (nan == np.broadcast_to(job.exp.layout_nan[None, None, :, None], res.shape)).all()
  seed = np.random.default_rng(5).integers(-64, 65, size=job.shape) / 16.0  # dyadic: what comes back is seed + result, rounded once
  rc, got = _launch(ctx, job, extra=_hip.BINNED_ACCUMULATE, init=seed)
  _hip.check(rc, case.name)
  want = seed + res
  assert (np.isnan(got) == nan).all() and _same_bits(got[~nan], want[~nan]), np.argwhere((got != want) & ~nan)[:4]
  rc, got = _launch(ctx, job, extra=_hip.BINNED_ACCUMULATE, init=seed, empty=True)
  _hip.check(rc, 'ndepth = 0, accumulate')
  assert _same_bits(got, seed)
  rc, got = _launch(ctx, job, init=seed, empty=True)
  _hip.check(rc, 'ndepth = 0')
  assert (got == 0).all()  # no rows: the sums are zero
