"""wbx_det_binned through the raw C ABI: EVERY output out[a][bk][lane][bin] against the float64 restatement of
tests/det_binned_cases.py -- NaN positions must match, then |got - want| <= bound, the bound computed per output from the inputs
((N + 4) 2^-53 sum |w val|, derived there); the integer-valued flavour of every case is compared bit for bit.  The cases, the
route each one is aimed at and the conditions that keep a failure from hiding are checked on the CPU by
tests/test_det_binned_cases.py; here every launch also holds wbx_binned_atoms_size against the restated patch geometry, so a
drift between the restatement and the library fails instead of un-aiming the cases.

(a) FUNC x flags x weight layout x dtype; (b) ragged rows and four-wave blocks; (c) one to four 64-row batches per patch and the
prefetch pipeline's main loop and tail; (d) rows that are not evenly spaced, a gathered climatology; (e) patches that overflow to
the slot kernel, mixed ownership, several sweeps of the slots; (f) nbin 1 / 33 / 64, bit 63, the high half alone, W that does not
depend on x; (g) the MERGED mask byte against the per-point mask, bit-identical; (h) prepared atom tables and the address-keyed
record of overflow-free tables; (i) the all-slot route of a reversed-x view; (j) non-finite statistics; (k) ACCUMULATE and empty
reductions; (l) the refusals."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
import det_binned_cases as DC

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
ERR_INVALID = -1


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


def _vp(v):
  return None if v is None else C.c_void_p(int(v))


class _Job:
  """The device side of one case: plan, inputs, weights, membership words."""

  def __init__(self, ctx, inp):
    self.ctx, self.inp, self.case = ctx, inp, inp.case
    case = inp.case
    self.plan = DC.plan_for(inp)
    self.dplan = engine._PlanOnDevice(ctx, self.plan)  # pylint: disable=protected-access
    self.bufs, self.ptrs = {}, {}
    for name in ('p', 't', 'c', 'mask'):
      self.ptrs[name] = None
      if name in inp.store:
        flat, _, base = inp.store[name]
        self.bufs[name] = ctx.upload(flat)
        self.ptrs[name] = self.bufs[name].ptr + base * flat.itemsize  # (a reversed view starts at the last element of its row)
    self.wt, self.bits = ctx.upload(inp.wt), ctx.upload(inp.bits)
    self.shape = (case.nA, case.nBk, DC.lanes_total(case.func, case.flags), case.nbin)
    self.w_flags = ((_hip.BINNED_W_ON_X if case.w_on_x else 0) | {'dense': 0, 'x': _hip.BINNED_WT_X_ONLY, 'row': _hip.BINNED_WT_ROW_ONLY}[case.wl]
                    | (_hip.BINNED_MASK_ON_W if case.merged else 0))
    self.geometry = DC.geometry(case.nA, case.nBk, case.nBr, case.nj, case.D, case.nx)

  def atoms_size(self):
    n = C.c_int64(-1)
    _hip.check(self.ctx.lib.wbx_binned_atoms_size(C.byref(self.dplan.struct), self.case.nA, self.case.nBk, self.case.nBr, self.w_flags, C.byref(n)),
               'wbx_binned_atoms_size')
    return int(n.value)

  def fill_tables(self, tables):
    assert tables.nbytes >= self.geometry.atoms_bytes == self.atoms_size()
    _hip.check(self.ctx.lib.wbx_binned_atoms(self.ctx.handle, C.byref(self.dplan.struct), self.case.nA, self.case.nBk, self.case.nBr, self.w_flags,
                                             _vp(self.bits.ptr), _vp(tables.ptr)), 'wbx_binned_atoms')

  def run(self, extra=0, seed=None, sentinel=None, struct=None, **over):
    """-> (rc, out[nA][nBk][lanes][nbin]); `over` replaces arguments of the call by name."""
    case = self.case
    if seed is not None:
      out = self.ctx.upload(seed)
    elif sentinel is not None:
      out = self.ctx.upload(np.full(self.shape, sentinel))
    else:
      out = self.ctx.alloc(int(np.prod(self.shape)) * 8)
    a = dict(func=case.func, dtype=_hip.F32 if case.dtype == 'float32' else _hip.F64, p=self.ptrs['p'], t=self.ptrs['t'], c=self.ptrs['c'],
             mask=self.ptrs['mask'], wt=self.wt.ptr, bits=self.bits.ptr, nA=case.nA, nBk=case.nBk, nBr=case.nBr, w_on_x=self.w_flags | extra,
             nbin=case.nbin, atoms=None)
    assert set(over) <= set(a), over
    a.update(over)
    rc = self.ctx.lib.wbx_det_binned(self.ctx.handle, C.byref(self.dplan.struct if struct is None else struct), a['func'], a['dtype'], _vp(a['p']),
                                     _vp(a['t']), _vp(a['c']), _vp(a['mask']), _vp(a['wt']), _vp(a['bits']), a['nA'], a['nBk'], a['nBr'],
                                     a['w_on_x'], a['nbin'], _vp(a['atoms']), _vp(out.ptr))
    return rc, self.ctx.download(out.ptr, self.shape, np.float64)


def _compare(got, exp, case, what=''):
  what = f'{case.name} {what}'
  want, bound = np.broadcast_to(exp.want, got.shape), np.broadcast_to(exp.bound, got.shape)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f'{what}: NaN positions')
  if case.integer:
    np.testing.assert_array_equal(got, want, err_msg=f'{what}: integer-valued, bit for bit')
    return 0.0
  fin = ~np.isnan(want)
  err = np.abs(got[fin] - want[fin])
  with np.errstate(all='ignore'):
    ratio = np.where(err == 0, 0.0, err / bound[fin])
  worst = float(ratio.max()) if ratio.size else 0.0
  print(f'{what}: largest |got - want| / bound = {worst:.3f}')
  bad = err > bound[fin]
  assert not bad.any(), (what, 'outputs beyond the bound', int(bad.sum()), np.argwhere(~np.isnan(want))[bad][:4].tolist(), worst)
  return worst


def _check(ctx, case, reverse=False):
  inp, exp = DC.prepared_reversed(case) if reverse else DC.prepared(case)
  job = _Job(ctx, inp)
  assert job.atoms_size() == job.geometry.atoms_bytes, (inp.case.name, 'wbx_binned_atoms_size against the restated geometry')
  rc, got = job.run()
  _hip.check(rc, inp.case.name)
  _compare(got, exp, inp.case)
  return job, got, exp


# ---- (a)
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('mode', list(DC.MODES))
@pytest.mark.parametrize('fname', list(DC.FUNCS))
def test_mode_matrix_every_output(ctx, fname, mode, dtype):
  cases = [c for c in DC.matrix_cases() if c.func == DC.FUNCS[fname] and c.flags == DC.MODES[mode] and c.dtype == dtype]
  assert len(cases) == 6  # three weight layouts, random and integer-valued
  for case in cases:
    _check(ctx, case)


# ---- (b) - (f)
@pytest.mark.parametrize('case', DC.ragged_cases(), ids=lambda c: c.name)
def test_ragged_rows_and_block_shape(ctx, case):
  _check(ctx, case)


@pytest.mark.parametrize('case', DC.batch_cases(), ids=lambda c: c.name)
def test_row_batches_and_the_prefetch_pipeline(ctx, case):
  _check(ctx, case)


@pytest.mark.parametrize('case', DC.uneven_cases(), ids=lambda c: c.name)
def test_unevenly_spaced_rows_and_their_even_twin(ctx, case):
  _check(ctx, case)


@pytest.mark.parametrize('case', DC.overflow_cases(), ids=lambda c: c.name)
def test_overflow_patches_and_mixed_ownership(ctx, case):
  _check(ctx, case)


@pytest.mark.parametrize('case', DC.word_cases(), ids=lambda c: c.name)
def test_bin_word_edges(ctx, case):
  _check(ctx, case)


# ---- (g)
@pytest.mark.parametrize('case', DC.merged_cases(), ids=lambda c: c.name)
def test_merged_mask_byte_is_bit_identical_to_the_per_point_mask(ctx, case):
  job, plain, _ = _check(ctx, case)  # the (br, x) mask handed over like any per-point mask
  rc, merged = job.run(extra=_hip.BINNED_MASK_ON_W)
  _hip.check(rc, case.name)
  assert np.array_equal(plain.view(np.uint64), merged.view(np.uint64)), np.argwhere(plain != merged)[:4]


# ---- (h)
def test_prepared_tables_and_the_record_of_overflow_free_ones(ctx):
  clean, over = DC.prepared_table_cases()
  jc, direct_c, _ = _check(ctx, clean)
  jo, direct_o, exp_o = _check(ctx, over)
  assert jc.geometry == jo.geometry
  tables = ctx.alloc(jc.geometry.atoms_bytes)
  jc.fill_tables(tables)  # no patch overflows: no slot-kernel launch behind these tables
  rc, got = jc.run(atoms=tables.ptr)
  _hip.check(rc, 'prepared, clean')
  assert np.array_equal(got.view(np.uint64), direct_c.view(np.uint64))
  jo.fill_tables(tables)  # the SAME buffer, now with overflowing patches: the record kept by address must go
  rc, got = jo.run(atoms=tables.ptr)
  _hip.check(rc, 'prepared, overflowing')
  _compare(got, exp_o, over, 'through refilled tables')
  assert np.array_equal(got.view(np.uint64), direct_o.view(np.uint64))
  jc.fill_tables(tables)  # ... and back
  rc, got = jc.run(atoms=tables.ptr)
  _hip.check(rc, 'prepared, clean again')
  assert np.array_equal(got.view(np.uint64), direct_c.view(np.uint64))


# ---- (i)
@pytest.mark.parametrize('case', DC.forward_cases_for_reversal(), ids=lambda c: c.name)
def test_reversed_x_view_takes_the_slot_kernel_everywhere(ctx, case):
  """check_plan does not refuse a negative xstride; launch_binned_k then leaves every patch to the slot kernel (the only route that
  memsets tmp).  Pinned as it is: same sums as the forward view of the same data, in another order."""
  _, fwd, exp = _check(ctx, case)
  _, rev, rexp = _check(ctx, case, reverse=True)
  np.testing.assert_array_equal(np.isnan(fwd), np.isnan(rev))
  if case.integer:
    np.testing.assert_array_equal(fwd, rev)
  else:
    fin = ~np.isnan(fwd)
    assert (np.abs(fwd - rev)[fin] <= (np.broadcast_to(exp.bound, fwd.shape) + np.broadcast_to(rexp.bound, fwd.shape))[fin]).all()


# ---- (j)
@pytest.mark.parametrize('case', DC.special_cases(), ids=lambda c: c.name)
def test_one_nan_poisons_its_lane_in_its_cell_and_nothing_else(ctx, case):
  _, got, _ = _check(ctx, case)
  nan = np.isnan(got)
  if case.special == 'masked_out':
    assert not nan.any()
  else:
    assert nan[DC.NAN_CELL].any()
    nan[DC.NAN_CELL] = False
    assert not nan.any()


@pytest.mark.parametrize('case', DC.inf_cases(), ids=lambda c: c.name)
def test_an_infinite_statistic_is_nan_in_every_bin(ctx, case):
  """include/wbx.h: a lane that meets an infinite statistic under a valid point is NaN in EVERY bin of its cell (the reference's
  xr.dot keeps +-inf in the bins the point is in: DC.expected(inf_poisons=False), tests/test_det_binned_cases.py)."""
  _, got, _ = _check(ctx, case)
  cell = got[DC.NAN_CELL]
  for l in (0, 1, 2, 3, 5):
    assert np.isnan(cell[l]).all(), l
  assert np.isfinite(cell[4]).all() and np.isfinite(cell[6:]).all()  # (t - c)^2 and the count do not see p
  assert not np.isinf(got).any()


# ---- (k)
def _accumulates(job, what):
  rng = np.random.default_rng(11)
  seed = rng.normal(size=job.shape)
  rc, res = job.run()
  _hip.check(rc, what)
  assert not np.isnan(res).any(), what
  rc, got = job.run(extra=_hip.BINNED_ACCUMULATE, seed=seed)
  _hip.check(rc, what)
  assert np.array_equal((seed + res).view(np.uint64), got.view(np.uint64)), (what, np.argwhere((seed + res) != got)[:4])


def test_accumulate_adds_into_out_on_every_route(ctx):
  _accumulates(_Job(ctx, DC.prepared(DC.by_name('a-det6-masked-dense-float32-rnd'))[0]), 'atom route')
  _accumulates(_Job(ctx, DC.prepared(DC.by_name('b-97-float32-rnd'))[0]), 'atom route, four-wave blocks')
  _accumulates(_Job(ctx, DC.prepared(DC.by_name('e-half-float32-rnd'))[0]), 'mixed route')
  _accumulates(_Job(ctx, DC.prepared_reversed(DC.by_name('i-det6-masked-rnd'))[0]), 'all-slot route')


def test_empty_reductions(ctx):
  job = _Job(ctx, DC.prepared(DC.by_name('a-det6-masked-dense-float32-rnd'))[0])
  for empty in (dict(nx=0), dict(ndepth=0)):
    dplan = engine._PlanOnDevice(ctx, dataclasses.replace(job.plan, **empty))  # pylint: disable=protected-access
    rc, got = job.run(sentinel=SENTINEL, struct=dplan.struct)
    _hip.check(rc, str(empty))
    assert (got == 0).all(), empty  # no rows: the sums are zero
    rc, got = job.run(extra=_hip.BINNED_ACCUMULATE, sentinel=SENTINEL, struct=dplan.struct)
    _hip.check(rc, str(empty))
    assert (got == SENTINEL).all(), empty  # ... and an accumulator stays as it is
  dplan = engine._PlanOnDevice(ctx, dataclasses.replace(job.plan, nkey=0))  # pylint: disable=protected-access
  rc, got = job.run(sentinel=SENTINEL, struct=dplan.struct, nA=0)
  _hip.check(rc, 'nA = 0')
  assert (got == SENTINEL).all()


# ---- (l)
def test_refusals(ctx):
  job = _Job(ctx, DC.prepared(DC.by_name('a-det6-masked-dense-float32-rnd'))[0])
  w = job.w_flags
  refused = {
      'nbin = 0': dict(nbin=0), 'nbin = 65': dict(nbin=65), 'nA nBk nBr != nkey': dict(nBr=job.case.nBr + 1),
      'X_ONLY | ROW_ONLY': dict(w_on_x=w | _hip.BINNED_WT_X_ONLY | _hip.BINNED_WT_ROW_ONLY), 'TWIN_MASK': dict(w_on_x=w | _hip.BINNED_TWIN_MASK),
      'an unknown bit': dict(w_on_x=w | 64), 'NULL wt': dict(wt=None), 'NULL bits': dict(bits=None), 'MASKED with a NULL mask': dict(mask=None),
      'DET6 with NULL c': dict(c=None), 'an unknown dtype': dict(dtype=7), 'an unknown func': dict(func=9)}
  for what, over in refused.items():
    rc, got = job.run(sentinel=SENTINEL, **over)
    assert rc == ERR_INVALID, (what, rc)
    with pytest.raises(_hip.WbxError):
      _hip.check(rc, what)
    assert (got == SENTINEL).all(), what
  rc, got = job.run(sentinel=SENTINEL)  # and the same job as it stands is accepted
  _hip.check(rc, 'accepted')
  assert not (got == SENTINEL).any()
