"""The float64 restatement behind tests/test_gpu_det_binned.py, checked without a GPU: against the project's float64 oracle
(oracle.wbx_oracle.aggregate) and against the binned emulation of tests/fake_device.py, and for EVERY case of the GPU matrix the
conditions that keep a GPU failure from hiding -- where the NaNs are, that one dropped or doubled point exceeds the bound, that the
addressing handed to the kernel reads the intended elements, and that the case takes the route it is aimed at (which kernel owns
which patch, the EVEN / !EVEN sweep, the 64-row batches, non-temporal lone waves against four-wave blocks)."""
import types

import numpy as np
import pytest

from oracle import wbx_oracle as O
import det_binned_cases as DC
import fake_device

FORWARD = DC.all_forward_cases()
REVERSED = DC.forward_cases_for_reversal()
IDS = [c.name for c in FORWARD]


def _get(case, reverse=False):
  return DC.prepared_reversed(case) if reverse else DC.prepared(case)


def _three():
  """plain, masked, skipna: DET6, dense weights, float32, random data, of the mode matrix."""
  names = {f'a-det6-{m}-dense-float32-rnd' for m in ('plain', 'masked', 'skipna')}
  out = [c for c in FORWARD if c.name in names]
  assert len(out) == 3
  return out


@pytest.mark.parametrize('case', _three(), ids=lambda c: c.name)
def test_restatement_agrees_with_the_oracle(case):
  inp, exp = _get(case)
  lanes = DC.stat(case.func, inp.p, inp.t, inp.c)
  member = np.broadcast_to(DC.member_of(inp.bits, case.nbin), (case.nBk, case.nBr, case.nx, case.nbin))
  mask = None if inp.mask is None else np.broadcast_to(inp.mask != 0, inp.p.shape)
  nl = len(lanes)
  for l, v in enumerate(lanes):
    sws, sw, od = O.aggregate(v, DC.DIMS, ['br', 'd', 'x'], weights=[(inp.W, ('bk', 'br', 'x'))],
                              bin_masks=[('bin', member, ('bk', 'br', 'x', 'bin'))], mask=mask, mask_dims=DC.DIMS,
                              skipna=bool(case.flags & DC.FLAG_SKIPNA))
    assert od == ('a', 'bk', 'bin')
    pairs = [(exp.want[:, :, l], exp.bound[:, :, l], sws)]
    if case.flags & DC.FLAG_SKIPNA:
      pairs.append((exp.want[:, :, nl + l], exp.bound[:, :, nl + l], sw))
    elif case.flags & DC.FLAG_MASKED:
      pairs.append((exp.want[:, :, nl], exp.bound[:, :, nl], sw))
    for want, bound, got in pairs:
      np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
      fin = np.isfinite(want)
      # (the einsum's own sum errs by the same bound, and its three-factor products by one more rounding per term)
      assert (np.abs(got - want)[fin] <= 2 * bound[fin]).all(), (case.name, l, float(np.nanmax(np.abs(got - want) / bound)))
  if case.flags == 0:
    assert np.isnan(exp.want).any() and not np.isnan(exp.want[0]).any()  # c alone: lanes 3-5 of one cell


@pytest.mark.parametrize('case', _three(), ids=lambda c: c.name)
def test_restatement_agrees_with_the_emulated_device(case):
  inp, exp = _get(case)
  plan = DC.plan_for(inp)
  devs = [types.SimpleNamespace(ptr=inp.store[n][0]) if n in inp.store else None for n in ('p', 't', 'c', 'mask')]
  w_buf = types.SimpleNamespace(shape=(case.nBk, case.nBr, case.nj, case.nbin), factored=None,
                                bufs=[types.SimpleNamespace(ptr=inp.W), types.SimpleNamespace(ptr=inp.bits)])
  nlt = DC.lanes_total(case.func, case.flags)
  out, shape = fake_device._run_binned(None, None, plan, devs, None, nlt, case.func, w_buf)  # pylint: disable=protected-access
  assert shape == (case.nA, case.nBk, nlt, 1, case.nbin)
  got = out[:, :, :, 0, :]
  np.testing.assert_array_equal(np.isnan(got), np.isnan(exp.want))
  fin = np.isfinite(exp.want)
  assert (np.abs(got - exp.want)[fin] <= 2 * exp.bound[fin]).all()


def _conditions(case, inp, exp):
  nl = DC.NLANES[case.func]
  values = exp.want[:, :, :nl]
  assert exp.want.shape == (case.nA_stored, case.nBk, DC.lanes_total(case.func, case.flags), case.nbin)
  if case.flags & DC.FLAG_SKIPNA:
    assert np.isfinite(exp.want).all(), 'under skipna every output is finite'
    assert exp.nan_stat, 'under skipna the statistic does contain NaNs'
  else:
    share = float(np.isfinite(values).mean())
    assert share >= 0.8, ('finite share of the value outputs', share)
  assert (exp.bound >= 0).all() and np.isfinite(exp.bound).all()
  # one point dropped or doubled in any bin moves lane 1 (|e|) and every count lane by more than the bound
  watch = ([1] if case.func != DC.PASS1 else []) + list(range(nl, exp.want.shape[2]))
  for l in watch:
    fin = np.isfinite(exp.want[:, :, l])
    assert (exp.minterm[:, :, l][fin] > 2 * exp.bound[:, :, l][fin]).all(), ('lane', l, 'smallest term against twice the bound')
  if case.integer:
    fin = np.isfinite(exp.want)
    assert (exp.want[fin] == np.rint(exp.want[fin])).all() and (np.abs(exp.want[fin]) < 2.0 ** 53).all()
  if not case.integer and case.wl == 'dense' and not case.special:
    assert np.unique(inp.wt).size == inp.wt.size, 'weights distinct point by point'
  if case.func != DC.PASS1:
    with np.errstate(invalid='ignore'):
      d = np.abs(inp.p.astype(np.float64) - inp.t.astype(np.float64))
    assert (d[np.isfinite(d)] >= 0.25).all()


def _addressing(case, inp):
  """What the plan's tables address is what the restatement summed."""
  shape = (case.nA, case.nBk, case.nBr, case.D, case.nx)
  for name in inp.store:
    logical = np.broadcast_to(getattr(inp, name), shape)
    np.testing.assert_array_equal(DC.read_back(inp, name), logical, err_msg=name)
  plan = DC.plan_for(inp)
  for i, name in enumerate(('p', 't', 'c', 'mask')):
    if name in inp.store:
      base = inp.store[name][2]
      off = fake_device._offsets(plan, i)[:, :, 0].reshape(shape[:4]) + base  # pylint: disable=protected-access
      np.testing.assert_array_equal(off, DC.row_offsets(inp, name), err_msg=name)
      assert plan.xstride[i] == inp.store[name][1]['x']


def _route(case, inp):
  r = DC.route(inp)
  assert r['owner'] == case.owner, (r['owner'], r['words'].max())
  assert r['nt'] == case.nt
  assert r['atoms'] == (not case.reversed_x)
  if case.batches is not None:
    assert r['batches'] == case.batches, r['batches']
  if case.even is True:
    assert r['even'] <= {True}, r['even']
  elif case.even is False:
    assert r['even'] == {False}, r['even']
  g = r['geometry']
  assert g.atoms_bytes % 8 == 0 and g.nxt == -(-case.nx // 64)
  if case.lonely:
    r0, x0 = case.nBr - 2, 5
    rs = (r0 * case.D) // g.rows_per_split
    rbeg, rend = g.rows(rs)
    patch = inp.bits[:, rbeg // case.D:(rend - 1) // case.D + 1, :64]
    for bk in range(case.nBk):
      assert (patch[bk] == inp.bits[bk, r0, x0]).sum() == 1 and inp.mask[0, bk, r0, 0, x0] == 0
  if case.special == 'empty_patch':
    tile = 1 if case.reversed_x else 0  # the tile whose patches are in no bin and hold the NaN
    assert (inp.bits[:, :, tile * 64:tile * 64 + 64] == 0).all() and (r['words'][:, :, tile] == 1).all()
    assert np.isnan(inp.p[DC.NAN_CELL][:, :, tile * 64:tile * 64 + 64]).sum() == 1


@pytest.mark.parametrize('case', FORWARD, ids=IDS)
def test_every_case_of_the_gpu_matrix(case):
  inp, exp = _get(case)
  _conditions(case, inp, exp)
  _addressing(case, inp)
  _route(case, inp)


@pytest.mark.parametrize('case', REVERSED, ids=[c.name for c in REVERSED])
def test_every_reversed_view(case):
  fwd, fexp = _get(case)
  inp, exp = _get(case, reverse=True)
  assert inp.case.reversed_x and inp.case.owner == 'slot'
  # the same stored data, and the same sums
  for name in fwd.store:
    assert fwd.store[name][0] is not inp.store[name][0]
    np.testing.assert_array_equal(fwd.store[name][0], inp.store[name][0])
    assert inp.store[name][1]['x'] == -1 and inp.store[name][2] == case.nx - 1
  np.testing.assert_array_equal(exp.want, fexp.want)
  _conditions(inp.case, inp, exp)
  _addressing(inp.case, inp)
  _route(inp.case, inp)


def test_special_values_poison_one_cell_only():
  for case in DC.special_cases() + DC.inf_cases():
    _, exp = _get(case)
    nan = np.isnan(exp.want)
    a0, b0 = DC.NAN_CELL
    if case.special == 'masked_out':
      assert not nan.any(), case.name
      continue
    assert nan[a0, b0].any(), case.name
    nan[a0, b0] = False
    assert not nan.any(), case.name
    nl = DC.NLANES[case.func]
    cell = np.isnan(exp.want[a0, b0])
    assert (cell.all(axis=1) | ~cell.any(axis=1)).all(), 'a poisoned lane is NaN in every bin'
    poisoned = cell.all(axis=1)
    if case.special == 'c_only':
      assert poisoned.tolist() == [False] * 3 + [True] * 3 + [False], case.name
    else:  # a NaN or an infinity in p: (t - c)^2 does not see it, and the count of valid points stays a number
      assert poisoned[:nl].tolist() == [l != 4 for l in range(nl)] and not poisoned[nl:].any(), case.name


def test_an_infinite_term_in_plain_float64():
  """What the reference's xr.dot gives for an infinite statistic: +-inf in the bins the point is in, NaN in the others.  The library
  gives NaN in every bin (include/wbx.h); both restatements are kept, and they differ exactly in the member bins."""
  for case in DC.inf_cases():
    inp, exp = _get(case)
    ieee = DC.expected(inp, inf_poisons=False)
    a0, b0 = DC.NAN_CELL
    r0, x0 = case.nBr // 2, case.nx // 3
    mem = DC.member_of(inp.bits[b0, r0, x0], case.nbin)
    assert mem.any() and not mem.all()
    for l in (0, 1, 2, 3, 5):
      assert np.isinf(ieee.want[a0, b0, l][mem]).all() and np.isnan(ieee.want[a0, b0, l][~mem]).all()
      assert np.isnan(exp.want[a0, b0, l]).all()
    np.testing.assert_array_equal(ieee.want[a0, b0, 4], exp.want[a0, b0, 4])
    others = np.ones(exp.want.shape[:2], bool)
    others[a0, b0] = False
    np.testing.assert_array_equal(ieee.want[others], exp.want[others])


def test_geometry_of_known_launches():
  # 156 cells of 721 x 1440 longitude-fastest: 8192 / (156 * 23) -> 3 splits of 241 rows; latitude-fastest rows (721 % 32 != 0)
  # take the larger target: 16384 / (156 * 12) -> 9 splits of 160 rows (the figures wbx_patch.hpp quotes)
  g = DC.geometry(156, 1, 721, 1440, 1, 1440)
  assert (g.nxt, g.nrs, g.rows_per_split) == (23, 3, 241)
  g = DC.geometry(156, 1, 1440, 721, 1, 721)
  assert (g.nxt, g.nrs, g.rows_per_split) == (12, 9, 160)
  g = DC.geometry(4096, 1, 200, 64, 1, 64)
  assert g.batches() == ((64, 36), (64, 36))
  g = DC.geometry(2, 2, 30, 96, 3, 96)
  assert g.rows_per_split % 3 == 0 and g.batches() == ((45,), (45,))
  bits = np.zeros((2, 30, 96), np.uint64)
  bits[1, 17, 70] = 5
  assert g.words(bits).tolist() == [[[1, 1], [1, 1]], [[1, 1], [1, 2]]]
