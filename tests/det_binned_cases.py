"""Inputs, the float64 restatement, the error bounds and the route predicates for the fused binned deterministic reduction
(wbx_det_binned: binned_atoms_kernel, aid_merge_kernel, det_atoms_kernel, det_binned_kernel, det_binned_finish), plain NumPy.

Frame.  Dims (a, bk, br, d, x): `a` kept, `bk` kept and W-dependent, `br` reduced and W-dependent, `d` reduced only, `x` reduced
and summed (W-dependent unless the case says `w_on_x = False`).  out[nA][nBk][lanes_total][nbin], count lanes as in include/wbx.h
(none / one shared under a mask alone / one per value lane under skipna).

Restatement (`expected`): the statistic lanes of DET3 / DET6 / PASS1 in float64 from the widened inputs, in the kernel's order of
operations (e = p - t, pa = p - c, ta = t - c); every term is the ROUNDED product lane * W and every sum is math.fsum, so the
restatement's own error is one rounding.  NaN rule of aggregation.py:272-277: a NaN term under a valid point turns every bin of that
lane in that (a, bk) cell NaN, whatever the point's membership or weight (NaN * 0 = NaN); under a mask alone a masked-out point
contributes exactly 0; under skipna a NaN statistic is counted out lane by lane.  An INFINITE term: the plain float64 sum of
term * member(0 / 1) gives +-inf in the bins the point is in and NaN in the others (`inf_poisons=False`); the library adds
sum * 0 of every atom / slot to every bin, so the lane is NaN in EVERY bin (`inf_poisons=True`, what include/wbx.h documents).

Bound (`Expected.bound`, per output): (N + 4) * 2^-53 * sum |w_i * val_i|, N = the valid points of the cell inside the bin.
Derived, not measured: any order of N fp64 additions errs by at most (N - 1) u sum |term|; the atom kernel's fma(val, w, acc) and the
slot kernel's rounded val * w differ from the restatement's rounded product by at most one u per term; the rest covers the final
rounding and the wave / LDS / patch folds.  Count lanes take the same bound.  The integer-valued flavour (small-integer p, t, c,
unit weights) makes every lane an integer below 2^53: those cases are compared bit for bit, whatever the order of the sums.

Routes (`geometry`, `route`): a restatement of patch_geometry (wbx_patch.hpp) and of what launch_binned_k / det_atoms_kernel decide
from it -- which patches the atom kernel owns (<= 32 distinct membership words) and which overflow to the slot kernel, whether the
rows of every 64-row batch are evenly spaced in every operand (the EVEN sweep) or not, the batches of a patch, and non-temporal
lone waves against four-wave blocks (rows of whole 128-byte lines or not).  `Geometry.atoms_bytes` restates atoms_carve; the GPU test
holds it against wbx_binned_atoms_size, so a drift between this file and the library fails loudly."""
import dataclasses
import functools
import math
import types

import numpy as np

DET3, DET6, PASS1 = 0, 1, 2
FLAG_MASKED, FLAG_SKIPNA = 1, 2
NLANES = {DET3: 3, DET6: 6, PASS1: 1}
NINPUTS = {DET3: 2, DET6: 3, PASS1: 1}
DIMS = ('a', 'bk', 'br', 'd', 'x')
ATOM_MAX = 32
U = 2.0 ** -53
MODES = {'plain': 0, 'masked': FLAG_MASKED, 'skipna': FLAG_SKIPNA, 'masked+skipna': FLAG_MASKED | FLAG_SKIPNA}
FUNCS = {'det3': DET3, 'det6': DET6, 'pass1': PASS1}
NAN_CELL = (1, 0)  # the (a, bk) cell the chosen non-finite values go into


def lanes_total(func, flags):
  nl = NLANES[func]
  return 2 * nl if flags & FLAG_SKIPNA else (nl + 1 if flags & FLAG_MASKED else nl)


@dataclasses.dataclass(frozen=True)
class Case:
  """One launch.  The last four fields name the route the case is aimed at; test_det_binned_cases.py holds them against `route`."""
  name: str
  func: int = DET3
  flags: int = 0
  wl: str = 'dense'        # weights: 'dense' wt[nBk][nBr][nj] | 'x' wt[nBk][nx] (WT_X_ONLY) | 'row' wt[nBk][nBr] (WT_ROW_ONLY)
  dtype: str = 'float32'
  nA: int = 2
  nBk: int = 2
  nBr: int = 37
  D: int = 1
  nx: int = 96
  a_bcast: bool = False    # one stored frame, stride 0 along a in every input
  bins: tuple = ('boxes', 34, 0)
  w_on_x: bool = True      # False: W depends on (bk, br) only -- bits[nBk][nBr], wt[nBk][nBr]
  integer: bool = False    # small-integer data and unit weights: every output is an exact integer
  special: str = ''        # one chosen non-finite value in NAN_CELL, see `build`
  d_outer: bool = False    # p, t, mask stored [a][d][bk][br][x]: consecutive rows of a batch are not evenly spaced
  gather: bool = False     # c comes through gather_key / gather_depth / gather_tab with a table that wraps
  mask_on_w: bool = False  # the mask depends on (bk, br, x) only
  merged: bool = False     # ... and the launch says so (WBX_BINNED_MASK_ON_W)
  reversed_x: bool = False  # the kernel walks x backwards: xstride = -1, pointers at the last element of the row
  lonely: bool = False     # one masked-out point is the only one of its atom in its patch
  seed: int = 0
  owner: str = 'atom'      # 'atom': every patch <= 32 words | 'slot': every patch to the slot kernel | 'mixed'
  even: object = True      # every batch of more than two rows evenly spaced / none of them / None: not claimed
  batches: object = None   # the 64-row batches of every row split, e.g. ((64, 36), (64, 36)); None: not claimed
  nt: bool = True          # rows are whole 128-byte lines (non-temporal lone waves) or not (four-wave blocks)

  @property
  def nj(self):
    return self.nx if self.w_on_x else 1

  @property
  def nbin(self):
    return self.bins[1] + (self.bins[2] if self.bins[0] == 'boxes' else 0)

  @property
  def nA_stored(self):
    return 1 if self.a_bcast else self.nA


# ---------------------------------------------------------------------------------------------------------------------
# geometry


@dataclasses.dataclass(frozen=True)
class Geometry:
  nBk: int
  nBr: int
  nj: int
  D: int
  nx: int
  nxt: int
  nrs: int
  rows_per_split: int

  @property
  def npatch(self):
    return self.nrs * self.nxt

  @property
  def atoms_bytes(self):
    """atoms_carve: uni | words | nwords | aid, each padded to 8 bytes."""
    n = self.nBk * self.npatch
    return (n + n * ATOM_MAX + (n + 1) // 2 + (self.nBk * self.nBr * self.nj + 7) // 8) * 8

  def rows(self, rs):
    rbeg = rs * self.rows_per_split
    return rbeg, min(rbeg + self.rows_per_split, self.nBr * self.D)

  def batches(self):
    """The row counts of the 64-row batches of every row split."""
    out = []
    for rs in range(self.nrs):
      rbeg, rend = self.rows(rs)
      out.append(tuple(min(64, rend - rb) for rb in range(rbeg, rend, 64)))
    return tuple(out)

  def words(self, bits):
    """bits[nBk][nBr][nj] -> the number of distinct membership words of every patch, [nBk][nrs][nxt] (live x only)."""
    bits = np.asarray(bits, np.uint64).reshape(self.nBk, self.nBr, self.nj)
    out = np.zeros((self.nBk, self.nrs, self.nxt), np.int64)
    for rs in range(self.nrs):
      rbeg, rend = self.rows(rs)
      br0, br1 = rbeg // self.D, (rend - 1) // self.D
      for xt in range(self.nxt):
        xs = slice(xt * 64, min(xt * 64 + 64, self.nx)) if self.nj > 1 else slice(0, 1)
        for bk in range(self.nBk):
          out[bk, rs, xt] = np.unique(bits[bk, br0:br1 + 1, xs]).size
    return out


def geometry(nA, nBk, nBr, nj, D, nx):
  """patch_geometry of wbx_patch.hpp (rows_hint = 0)."""
  cells = nA * nBk
  rows = nBr * D
  nxt = (nx + 63) // 64
  target = 8192 if nx % 32 == 0 else 16384
  want = (target + cells * nxt - 1) // (cells * nxt)
  want = max(1, min(want, (rows + 63) // 64))
  rps = (rows + want - 1) // want
  rps = (rps + D - 1) // D * D
  nrs = (rows + rps - 1) // rps
  return Geometry(nBk=nBk, nBr=nBr, nj=nj, D=D, nx=nx, nxt=nxt, nrs=nrs, rows_per_split=rps)


# ---------------------------------------------------------------------------------------------------------------------
# bins


def _layers_boxes(nBk, nBr, nj, nbin):
  """Box-shaped bins: region boxes that tile the (br, x) plane, two hemispheres and 'global', each split by a land / sea checker
  (an odd nbin: the last bin is 'global' unsplit); nbin = 1: one box.  -> bool [nBk][nBr][nj][nbin]"""
  br = np.arange(nBr)[None, :, None]
  xj = np.arange(nj)[None, None, :]
  bk = np.arange(nBk)[:, None, None]
  brs = (br + 3 * bk) % nBr  # (every bk has its own map)
  shape = (nBk, nBr, nj)
  if nbin == 1:
    box = (brs >= nBr // 4) & (xj * 3 >= nj) | (xj == 0) & (brs == 0)
    return np.broadcast_to(box, shape)[..., None].copy()
  base = nbin // 2
  lay = []
  nbox = max(base - 3, 0)
  if nbox:
    gr = 2 if nj > 1 else nbox
    gc = -(-nbox // gr) if nj > 1 else 1
    idx = (brs * gr // nBr) * gc + xj * gc // max(nj, 1)
    idx = np.minimum(idx, nbox - 1)
    lay += [np.broadcast_to(idx == b, shape) for b in range(nbox)]
  if base >= 3:
    lay += [np.broadcast_to(brs * 2 < nBr, shape), np.broadcast_to(brs * 2 >= nBr, shape)]
  while len(lay) < base:
    lay.append(np.ones(shape, bool))
  land = np.broadcast_to(((br // 5) + (xj // 9) + bk) % 2 == 0, shape)
  out = [l & land for l in lay] + [l & ~land for l in lay]
  if nbin % 2:
    out.append(np.ones(shape, bool))
  return np.stack(out, axis=-1)


def make_bits(case, rng):
  """-> bits[nBk][nBr][nj] uint64"""
  nBk, nBr, nj = case.nBk, case.nBr, case.nj
  kind, nbin = case.bins[0], case.bins[1]
  shape = (nBk, nBr, nj)
  shift = 0
  if kind == 'boxes':
    layers, shift = _layers_boxes(nBk, nBr, nj, nbin), case.bins[2]
  elif kind == 'xbands':  # nbin - 1 bands along x and 'global' on the last bit
    band = np.arange(nj) * (nbin - 1) // nj
    layers = np.zeros(shape + (nbin,), bool)
    layers[..., nbin - 1] = True
    for b in range(nbin - 1):
      layers[:, :, band == b, b] = True
  elif kind == 'single63':  # 64 bins, every one empty but the last: a box on bit 63
    layers = np.zeros(shape + (64,), bool)
    layers[:, nBr // 4:, nj // 3:, 63] = True
  elif kind in ('half', 'random', 'halfx'):
    # row bands + one global bin, with membership drawn point by point in the first half of the rows ('half'), of x
    # ('halfx') or everywhere ('random')
    bands = (np.arange(nBr)[:, None] * nbin // nBr == np.arange(nbin)[None, :]) | (np.arange(nbin)[None, :] == 0)
    layers = np.broadcast_to(bands[None, :, None, :], shape + (nbin,)).copy()
    noise = rng.random(shape + (nbin,)) < 0.5
    if kind == 'half':
      layers[:, :nBr // 2] = noise[:, :nBr // 2]
    elif kind == 'halfx':
      layers[:, :, :64] = noise[:, :, :64]
    else:
      layers = noise
  elif kind == 'right':  # boxes beyond the first x tile only: its patches are in no bin at all (and after mirroring a row of
    # 97 points, the patches of the second tile)
    layers = _layers_boxes(nBk, nBr, nj, nbin).copy()
    layers[:, :, :64] = False
  else:
    raise ValueError(kind)
  bits = np.zeros(shape, np.uint64)
  for b in range(layers.shape[-1]):
    bits |= layers[..., b].astype(np.uint64) << np.uint64(b + shift)
  return bits


def member_of(bits, nbin):
  """bits[...] -> bool [..., nbin]"""
  return ((np.asarray(bits, np.uint64)[..., None] >> np.arange(nbin, dtype=np.uint64)) & np.uint64(1)).astype(bool)


# ---------------------------------------------------------------------------------------------------------------------
# inputs


def _store(logical, order, a_bcast, reversed_x):
  """logical[a, bk, br, d, x] -> (flat storage, element strides by dim, element offset of the first element)."""
  perm = [DIMS.index(d) for d in order]
  st = np.ascontiguousarray(np.transpose(logical[..., ::-1] if reversed_x else logical, perm))
  strides = {d: s // st.itemsize for d, s in zip(order, st.strides)}
  base = 0
  if reversed_x:
    strides['x'], base = -1, logical.shape[-1] - 1
  for d, n in zip(DIMS, logical.shape):
    if n == 1 and d != 'x':
      strides[d] = 0
  if a_bcast:
    strides['a'] = 0
  return st.reshape(-1), strides, base


def build(case):
  """-> namespace: p, t, c, mask (logical [nA_stored or 1, nBk, nBr, D or 1, nx] as the kernel indexes them; None where unused),
  W[nBk][nBr][nx] (the weight of every point), wt (as handed to the kernel), bits[nBk][nBr][nj], store[name] = (flat array,
  strides, base offset) and gather = None or (table[nA][D] of element offsets into c's storage)."""
  assert not case.reversed_x, 'a reversed view is made by reverse_view() from its forward case'
  rng = np.random.default_rng(1000 + case.seed)
  dt = np.dtype(case.dtype)
  nAs, nBk, nBr, D, nx, nj = case.nA_stored, case.nBk, case.nBr, case.D, case.nx, case.nj
  shape = (nAs, nBk, nBr, D, nx)
  func, flags = case.func, case.flags
  if case.integer:
    t = rng.integers(-6, 7, size=shape).astype(dt)
    e = rng.integers(1, 5, size=shape) * rng.choice([-1, 1], size=shape)
    p = (t + e).astype(dt)
    cdev = rng.integers(1, 4, size=shape) + np.abs(e)
  else:
    t = (rng.normal(size=shape) * 2).astype(dt)
    e = (0.3 + 1.7 * rng.random(shape)) * rng.choice([-1.0, 1.0], size=shape)
    p = (t.astype(np.float64) + e).astype(dt)  # |p - t| >= 0.25 after the rounding to float32
    cdev = 0.3 + rng.random(shape) + np.abs(e)
  nslice = 3
  table = None
  if case.gather:  # c[a, .., d, ..] = slice (2 + a + d) mod 3 of a climatology stored [slice][bk][br][x]: it wraps, so it is not monotone
    cstore = (rng.integers(-9, 10, size=(nslice, nBk, nBr, nx)) + (0 if case.integer else 0.37)).astype(dt)
    sl = (2 + np.arange(case.nA)[:, None] + np.arange(D)[None, :]) % nslice
    table = sl.astype(np.int64) * (nBk * nBr * nx)
    c = np.moveaxis(cstore[sl[:nAs]], 1, 3)  # [a, d, bk, br, x] -> [a, bk, br, d, x]
    c = np.ascontiguousarray(c)
    assert not case.a_bcast
  else:
    c = (t.astype(np.float64) - np.sign(e) * cdev).astype(dt)  # distinct from both: |t - c| >= 0.3, |p - c| >= 0.6

  # weights in [0.5, 1.5], distinct point by point (a point credited to the wrong row or x shows)
  def distinct(n):
    return 0.5 + (rng.permutation(n) + rng.random(n) * 0.5) / n

  if case.integer:
    wt = np.ones((nBk, nBr, nj) if case.wl == 'dense' else ((nBk, nx) if case.wl == 'x' else (nBk, nBr)))
  elif case.wl == 'dense':
    wt = distinct(nBk * nBr * nj).reshape(nBk, nBr, nj)
  elif case.wl == 'x':
    wt = distinct(nBk * nx).reshape(nBk, nx)
  else:
    wt = distinct(nBk * nBr).reshape(nBk, nBr)
  assert case.w_on_x or case.wl == 'dense'
  bits = make_bits(case, rng)

  mask = None
  if flags & FLAG_MASKED:
    mshape = (1, nBk, nBr, 1, nx) if case.mask_on_w else shape
    mask = (rng.random(mshape) > 0.25).astype(np.uint8)
  else:
    assert not (case.mask_on_w or case.merged or case.lonely)

  full = lambda m: np.broadcast_to(m, shape)
  # ---- NaNs
  if flags & FLAG_SKIPNA:  # a 3 % share, in p, t and c independently: a NaN in c alone leaves lanes 0-2 and their counts whole
    for arr in (p, t) if case.gather else (p, t, c):
      arr[rng.random(shape) < 0.03] = np.nan
    if case.gather:
      cstore[rng.random(cstore.shape) < 0.03] = np.nan
      c = np.ascontiguousarray(np.moveaxis(cstore[sl[:nAs]], 1, 3))
  elif flags & FLAG_MASKED:  # NaNs the mask hides: they must leave no trace
    hide = (rng.random(shape) < 0.12) & (full(mask) == 0)
    p[hide] = np.nan
  elif func == DET6 and not case.a_bcast and case.nA * nBk >= 4 and not case.gather and not case.special:
    c[NAN_CELL[0], NAN_CELL[1], nBr // 2, 0, nx // 3] = np.nan  # c alone: lanes 3-5 of one cell are NaN in every bin
  # ---- one chosen non-finite value (in NAN_CELL; the other cells stay clean)
  sp = case.special
  if sp:
    assert case.nA * nBk >= 6 and not case.a_bcast and not (flags & FLAG_SKIPNA)
    a0, b0 = NAN_CELL
    r0, x0 = nBr // 2, (nx - 1 if sp == 'last_live' else nx // 3)
    xj0 = x0 if nj > 1 else 0
    if mask is not None:
      mask[a0 if not case.mask_on_w else 0, b0, r0, 0, x0] = 0 if sp == 'masked_out' else 1
    if sp == 'zero_weight':
      assert case.wl == 'dense'
      wt[b0, r0, xj0] = 0.0
    if sp == 'no_bin':
      bits[b0, r0, xj0] = 0
    if sp == 'c_only':
      c[a0, b0, r0, 0, x0] = np.nan
    elif sp == 'inf':
      p[a0, b0, r0, 0, x0] = np.inf
    elif sp == 'empty_patch':  # (bins 'right': the patches of x < 64 are in no bin)
      assert nj > 64 and (bits[:, :, :64] == 0).all()
      p[a0, b0, r0, 0, 0] = np.nan
    else:
      p[a0, b0, r0, 0, x0] = np.nan
  if case.lonely:  # a word of its own under a masked-out point
    r0, x0 = nBr - 2, 5
    bits[:, r0, x0] ^= np.uint64(1) << np.uint64(case.nbin - 1)
    bits[:, r0, x0] ^= np.uint64(2)
    mask[:, :, r0, :, x0] = 0

  if case.wl == 'dense':
    W = np.broadcast_to(wt, (nBk, nBr, nx)) if nj > 1 else np.broadcast_to(wt.reshape(nBk, nBr, 1), (nBk, nBr, nx))
  elif case.wl == 'x':
    W = np.broadcast_to(wt[:, None, :], (nBk, nBr, nx))
  else:
    W = np.broadcast_to(wt[:, :, None], (nBk, nBr, nx))

  order = ('a', 'd', 'bk', 'br', 'x') if case.d_outer else DIMS
  store = {'p': _store(p, order, case.a_bcast, case.reversed_x)}
  if func != PASS1:
    store['t'] = _store(t, order, case.a_bcast, case.reversed_x)
  if func == DET6:
    if case.gather:
      assert not case.reversed_x
      store['c'] = (cstore.reshape(-1), {'a': 0, 'bk': nBr * nx, 'br': nx, 'd': 0, 'x': 1}, 0)
    else:
      store['c'] = _store(c, order, case.a_bcast, case.reversed_x)
  if mask is not None:
    store['mask'] = _store(mask, order, case.a_bcast or case.mask_on_w, case.reversed_x)
  return types.SimpleNamespace(case=case, p=p, t=t if func != PASS1 else None, c=c if func == DET6 else None, mask=mask, W=np.ascontiguousarray(W),
                               wt=np.ascontiguousarray(wt), bits=np.ascontiguousarray(bits), store=store, gather=table)


def reverse_view(inp):
  """The same stored data, weights and bins as `inp` (a forward case) read through xstride = -1 from the last element of every
  row: the kernel's x is the mirror image, so wt / bits / mask are handed over mirrored and every point keeps its own."""
  case = dataclasses.replace(inp.case, reversed_x=True, owner='slot', even=None, name=inp.case.name + '-reversed')
  flip = lambda v: None if v is None else np.ascontiguousarray(v[..., ::-1])
  order = DIMS
  assert not case.d_outer and not case.gather and case.w_on_x
  out = types.SimpleNamespace(case=case, p=flip(inp.p), t=flip(inp.t), c=flip(inp.c), mask=flip(inp.mask), W=flip(inp.W),
                              wt=flip(inp.wt) if case.wl != 'row' else inp.wt, bits=flip(inp.bits), gather=None, store={})
  for name in inp.store:
    out.store[name] = _store(getattr(out, name), order, case.a_bcast or (name == 'mask' and case.mask_on_w), True)
  return out


def row_offsets(inp, name):
  """Element offset of the first element (kernel x = 0) of every row of input `name`: [nA][nBk][nBr][D], the gather included."""
  case = inp.case
  _, st, base = inp.store[name]
  off = np.full((case.nA, case.nBk, case.nBr, case.D), base, np.int64)
  for ax, d in enumerate(DIMS[:4]):
    sh = [1, 1, 1, 1]
    sh[ax] = -1
    off = off + (np.arange(off.shape[ax], dtype=np.int64) * st.get(d, 0)).reshape(sh)
  if name == 'c' and inp.gather is not None:
    off = off + inp.gather[:, None, None, :]
  return off


def read_back(inp, name):
  """What the kernel's addressing reads of input `name`: [nA][nBk][nBr][D][nx] -- must equal the logical array."""
  flat, st, _ = inp.store[name]
  idx = row_offsets(inp, name)[..., None] + np.arange(inp.case.nx, dtype=np.int64) * st['x']
  assert idx.min() >= 0 and idx.max() < flat.size, (name, idx.min(), idx.max(), flat.size)
  return flat[idx]


# ---------------------------------------------------------------------------------------------------------------------
# restatement


def stat(func, p, t=None, c=None):
  """The value lanes of `func` in float64 from the widened inputs, in the kernel's order of operations: a list of arrays."""
  with np.errstate(all='ignore'):
    p = np.asarray(p).astype(np.float64)
    if func == PASS1:
      return [p]
    t = np.asarray(t).astype(np.float64)
    e = p - t
    lanes = [e, np.abs(e), e * e]
    if func == DET6:
      c = np.asarray(c).astype(np.float64)
      pa, ta = p - c, t - c
      lanes += [pa * pa, ta * ta, pa * ta]
    return lanes


@dataclasses.dataclass
class Expected:
  want: np.ndarray     # [nA_stored][nBk][lanes_total][nbin]
  bound: np.ndarray    # same shape
  minterm: np.ndarray  # same shape: the smallest |w * val| among the terms of the output (inf where there is none)
  nan_stat: bool       # a value lane holds a NaN somewhere


def expected(inp, inf_poisons=True):
  """The float64 restatement of the launch `inp` describes -> Expected, [nA_stored][nBk][lanes_total][nbin]: a frame that is
  broadcast along a (stride 0) is computed once, and the comparison broadcasts it over the launch's nA."""
  case = inp.case
  func, flags, nbin = case.func, case.flags, case.nbin
  nAs, nBk, nBr, D, nx = case.nA_stored, case.nBk, case.nBr, case.D, case.nx
  shape = (nAs, nBk, nBr, D, nx)
  vals = stat(func, inp.p, inp.t, inp.c)
  nan_stat = any(np.isnan(v).any() for v in vals)
  valid = np.ones(shape, bool) if not (flags & FLAG_MASKED) else np.broadcast_to(inp.mask != 0, shape)
  if flags & FLAG_SKIPNA:
    oks = [valid & ~np.isnan(v) for v in vals]
    lanes = [np.where(ok, v, 0.0) for ok, v in zip(oks, vals)] + [ok.astype(np.float64) for ok in oks]
  elif flags & FLAG_MASKED:
    lanes = [np.where(valid, v, 0.0) for v in vals] + [valid.astype(np.float64)]
  else:
    lanes = vals
  nlt = len(lanes)
  assert nlt == lanes_total(func, flags)
  member = member_of(inp.bits, nbin)  # [nBk, nBr, nj, nbin]
  member = np.broadcast_to(member[:, :, None, :, :], (nBk, nBr, D, nx, nbin)).reshape(nBk, nBr * D * nx, nbin)
  Wp = np.broadcast_to(inp.W[:, :, None, :], (nBk, nBr, D, nx))
  want = np.empty((nAs, nBk, nlt, nbin))
  bound = np.empty_like(want)
  minterm = np.empty_like(want)
  with np.errstate(all='ignore'):
    for a in range(nAs):
      for bk in range(nBk):
        mem = member[bk]
        memf = mem.astype(np.float64)
        nvalid = valid[a, bk].reshape(-1).astype(np.float64) @ memf  # [nbin]
        for l in range(nlt):
          terms = (lanes[l][a, bk] * Wp[bk]).reshape(-1)  # the rounded products
          absd = np.abs(terms)
          finite = np.isfinite(terms)
          absf = np.where(finite, absd, 0.0)
          bound[a, bk, l] = (nvalid + 4) * U * (absf @ memf) * (1 + 1e-12)  # (the sum of |terms| itself is rounded)
          live = valid[a, bk].reshape(-1) & (absd > 0)
          big = np.where(live, absd, np.inf)
          minterm[a, bk, l] = np.where(mem, big[:, None], np.inf).min(axis=0) if terms.size else np.inf
          if np.isnan(terms).any() or (inf_poisons and not finite.all()):
            want[a, bk, l] = np.nan
            continue
          if case.integer:  # every partial sum is an integer below 2^53: exact in any order
            want[a, bk, l] = terms @ memf if finite.all() else [float(np.sum(terms * memf[:, b])) for b in range(nbin)]
            continue
          tl = terms
          for b in range(nbin):
            sel = mem[:, b]
            if finite.all():
              want[a, bk, l, b] = math.fsum(tl[sel].tolist())
            else:  # an infinite term: NaN where it meets a 0 membership, +-inf where it is a member
              want[a, bk, l, b] = float(np.sum(tl * memf[:, b]))
  return Expected(want=want, bound=bound, minterm=minterm, nan_stat=nan_stat)


@functools.lru_cache(maxsize=None)
def prepared(case):
  """-> (inputs, Expected) of a forward case, computed once per session and left unchanged."""
  inp = build(case)
  return inp, expected(inp)


@functools.lru_cache(maxsize=None)
def prepared_reversed(case):
  inp = reverse_view(prepared(case)[0])
  return inp, expected(inp)


def plan_for(inp, flags=None):
  """The stage-1 plan of the launch: build_s1_plan(dims, sizes, layouts, reduce_dims=(br, d, x), wdep_dims={bk, br[, x]},
  force_x_dim=x, allow_vec4=False)."""
  from weatherbenchx_amd import planner  # pylint: disable=g-import-not-at-top
  case = inp.case
  sizes = dict(zip(DIMS, (case.nA, case.nBk, case.nBr, case.D, case.nx)))
  layouts = []
  for name in ('p', 't', 'c', 'mask'):
    if name in inp.store:
      flat, st, _ = inp.store[name]
      layouts.append(planner.InputLayout(strides=dict(st), itemsize=flat.itemsize, base_alignment=256))
    else:
      layouts.append(None)
  gather = planner.GatherSpec(dims=('a', 'd'), table=inp.gather) if inp.gather is not None else None
  wdep = {'bk', 'br', 'x'} if case.w_on_x else {'bk', 'br'}
  plan = planner.build_s1_plan(DIMS, sizes, layouts, reduce_dims=('br', 'd', 'x'), wdep_dims=wdep, gather=gather,
                               flags=case.flags if flags is None else flags, allow_vec4=False, force_x_dim='x')
  assert plan.a_dims == ('a',) and plan.bk_dims == ('bk',) and plan.br_dims == ('br',) and plan.depth_dims == ('d',), plan
  assert plan.nkey == case.nA * case.nBk * case.nBr and plan.ndepth == case.D and plan.nx == case.nx and plan.plane_rows == 0, plan
  return plan


# ---------------------------------------------------------------------------------------------------------------------
# routes


def route(inp):
  """What launch_binned_k and det_atoms_kernel decide for the launch: dict(atoms, nt, words[nBk][nrs][nxt], owner, batches, even)
  -- `even`: the set of the EVEN predicate's values over every (cell, row split, batch of more than two rows)."""
  case = inp.case
  g = geometry(case.nA, case.nBk, case.nBr, case.nj, case.D, case.nx)
  itemsize = np.dtype(case.dtype).itemsize
  xstrides = [inp.store[n][1]['x'] for n in inp.store]
  atoms = all(0 <= s and (case.nx - 1) * s < (1 << 31) // 8 for s in xstrides)
  words = g.words(inp.bits)
  over = words > ATOM_MAX
  owner = 'slot' if (not atoms or over.all()) else ('mixed' if over.any() else 'atom')
  # EVEN: within a batch, consecutive rows are the same distance apart in every operand the kernel reads, and in the
  # (bk, br) row index of wt / bits / the atom ids
  offs = [row_offsets(inp, n).reshape(case.nA, case.nBk, case.nBr * case.D) for n in inp.store]
  wrow = np.broadcast_to((np.arange(case.nBk)[:, None] * case.nBr + np.arange(case.nBr)[None, :]).repeat(case.D, axis=1) * case.nj,
                         (case.nA, case.nBk, case.nBr * case.D))
  even = set()
  for rs in range(g.nrs):
    rbeg, rend = g.rows(rs)
    for rb in range(rbeg, rend, 64):
      re_ = min(rb + 64, rend)
      if re_ - rb <= 2:
        continue
      ok = np.ones((case.nA, case.nBk), bool)
      for o in offs + [wrow]:
        dd = np.diff(o[:, :, rb:re_], axis=2)
        ok &= (dd == dd[:, :, :1]).all(axis=2)
      even |= set(ok.reshape(-1).tolist())
  return dict(atoms=atoms, nt=(case.nx * itemsize) % 128 == 0, words=words, owner=owner, batches=g.batches(), even=even, geometry=g)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU matrix (tests/test_gpu_det_binned.py runs every one; tests/test_det_binned_cases.py checks every one on the CPU)


def _name(*parts):
  return '-'.join(str(p) for p in parts)


def matrix_cases():
  """(a) FUNC x flags x weight layout x dtype x {random, integer-valued} at nA = 2, nBk = 2, nBr = 37, D = 1, nx = 96 (whole
  128-byte lines in both dtypes), 34 box-shaped bins: every patch <= 32 words."""
  out = []
  seed = 0
  for fname, func in FUNCS.items():
    for mode, flags in MODES.items():
      for wl in ('dense', 'x', 'row'):
        for dtype in ('float32', 'float64'):
          for integer in (False, True):
            seed += 1
            out.append(Case(name=_name('a', fname, mode, wl, dtype, 'int' if integer else 'rnd'), func=func, flags=flags, wl=wl, dtype=dtype,
                            integer=integer, seed=seed, batches=((37,),)))
  return out


def ragged_cases():
  """(b) ragged rows and the block shape: float32 DET6 masked at nx = 1, 63, 64, 65, 97, 130; float64 at 80 (whole lines) and 97."""
  out = []
  for nx, dtype in ((1, 'float32'), (63, 'float32'), (64, 'float32'), (65, 'float32'), (97, 'float32'), (130, 'float32'),
                    (80, 'float64'), (97, 'float64')):
    nt = (nx * np.dtype(dtype).itemsize) % 128 == 0
    for integer in (False, True):
      out.append(Case(name=_name('b', nx, dtype, 'int' if integer else 'rnd'), func=DET6, flags=FLAG_MASKED, dtype=dtype, nx=nx, nt=nt,
                      integer=integer, seed=200 + nx, batches=((37,),)))
  for wl in ('x', 'row'):  # (four-wave blocks with factored weights)
    out.append(Case(name=_name('b', 97, 'float32', wl), func=DET3, flags=FLAG_SKIPNA, wl=wl, nx=97, nt=False, seed=298, batches=((37,),)))
  return out


def batch_cases():
  """(c) row batches and the prefetch pipeline: D = 1, nx = 64, nBk = 1, one stored frame broadcast along a."""
  out = []
  for nBr in (1, 2, 5, 6, 9, 63, 64):
    out.append(Case(name=_name('c', nBr), func=DET6, flags=FLAG_MASKED, nA=2, nBk=1, nBr=nBr, nx=64, a_bcast=True, bins=('boxes', 34, 0),
                    seed=300 + nBr, batches=((nBr,),)))
  # (65 rows at nA = 2 are cut into two splits of 33 and 32: one patch of 64 + 1 rows needs cells * nxt >= 8192)
  out.append(Case(name='c-65', func=DET3, flags=FLAG_MASKED, nA=8192, nBk=1, nBr=65, nx=64, a_bcast=True, seed=365, batches=((64, 1),)))
  out.append(Case(name='c-200-two-batches', func=DET6, flags=FLAG_MASKED, nA=4096, nBk=1, nBr=200, nx=64, a_bcast=True, seed=366,
                  batches=((64, 36), (64, 36))))
  out.append(Case(name='c-200-four-batches', func=DET3, flags=0, nA=8192, nBk=1, nBr=200, nx=64, a_bcast=True, seed=367,
                  batches=((64, 64, 64, 8),)))
  out.append(Case(name='c-200-four-batches-int', func=DET6, flags=FLAG_SKIPNA, nA=8192, nBk=1, nBr=200, nx=64, a_bcast=True, seed=368,
                  integer=True, batches=((64, 64, 64, 8),)))
  return out


def uneven_cases():
  """(d) rows that are not evenly spaced inside a batch: D = 3, nBr = 30 stored [a][d][bk][br][x], the climatology of DET6 gathered
  through a table that wraps; the same frame with D = 1 as the EVEN twin."""
  out = []
  for dtype in ('float32', 'float64'):
    for mode in ('plain', 'masked', 'skipna'):
      for integer in (False, True):
        tag = _name(dtype, mode, 'int' if integer else 'rnd')
        out.append(Case(name=_name('d-uneven', tag), func=DET6, flags=MODES[mode], dtype=dtype, nBr=30, D=3, nx=96, d_outer=True, gather=True,
                        integer=integer, seed=400, even=False, batches=((45,), (45,))))
        out.append(Case(name=_name('d-even', tag), func=DET6, flags=MODES[mode], dtype=dtype, nBr=30, D=1, nx=96, d_outer=True, gather=True,
                        integer=integer, seed=400, even=True, batches=((30,),)))
  return out


def overflow_cases():
  """(e) patches with more than 32 words: 40 bins random in the first half of the rows ('half': mixed ownership), everywhere
  ('random': every patch to the slot kernel; the union of a patch has 40 bins, so the slot kernel takes more than one sweep:
  K = 3 at DET6 skipna, K = 32 at PASS1 plain), in the first x tile ('halfx')."""
  out = []
  for dtype in ('float32', 'float64'):
    for integer in (False, True):
      tag = _name(dtype, 'int' if integer else 'rnd')
      out.append(Case(name=_name('e-half', tag), func=DET6, flags=FLAG_MASKED, dtype=dtype, nA=2, nBk=2, nBr=150, nx=90, bins=('half', 40), integer=integer,
                      seed=500, owner='mixed', nt=False, batches=((50,), (50,), (50,))))
  for integer in (False, True):
    tag = 'int' if integer else 'rnd'
    out.append(Case(name=_name('e-random-det6-skipna', tag), func=DET6, flags=FLAG_SKIPNA, nBr=37, nx=90, bins=('random', 40), integer=integer, seed=501,
                    owner='slot', nt=False, batches=((37,),)))
    out.append(Case(name=_name('e-random-pass1', tag), func=PASS1, flags=0, nBr=37, nx=96, bins=('random', 40), integer=integer, seed=502,
                    owner='slot', batches=((37,),)))
    out.append(Case(name=_name('e-halfx-det3', tag), func=DET3, flags=FLAG_MASKED | FLAG_SKIPNA, nBr=30, nx=130, bins=('halfx', 40), integer=integer,
                    seed=503, owner='mixed', nt=False, batches=((30,),)))
  return out


def word_cases():
  """(f) the edges of the membership word and of det_binned_finish (ng = 256 / nbin)."""
  out = []
  for integer in (False, True):
    tag = 'int' if integer else 'rnd'
    out.append(Case(name=_name('f-nbin1', tag), func=DET6, flags=FLAG_MASKED, bins=('boxes', 1, 0), integer=integer, seed=601, batches=((37,),)))
    out.append(Case(name=_name('f-nbin33', tag), func=DET3, flags=FLAG_SKIPNA, bins=('boxes', 33, 0), integer=integer, seed=602, batches=((37,),)))
    out.append(Case(name=_name('f-nbin64', tag), func=DET6, flags=0, nx=130, bins=('xbands', 64), integer=integer, seed=603, nt=False, batches=((37,),)))
    out.append(Case(name=_name('f-bit63-only', tag), func=DET3, flags=FLAG_MASKED, bins=('single63', 64), integer=integer, seed=604, batches=((37,),)))
    out.append(Case(name=_name('f-high-half', tag), func=DET6, flags=FLAG_MASKED, bins=('boxes', 32, 32), integer=integer, seed=605, batches=((37,),)))
    out.append(Case(name=_name('f-high-half-plain', tag), func=DET3, flags=0, bins=('boxes', 32, 32), integer=integer, seed=606, batches=((37,),)))
    out.append(Case(name=_name('f-nj1', tag), func=DET6, flags=FLAG_MASKED, nx=130, w_on_x=False, bins=('boxes', 34, 0), integer=integer, seed=607, nt=False,
                    batches=((37,),)))
    out.append(Case(name=_name('f-nj1-float64', tag), func=DET3, flags=FLAG_SKIPNA, dtype='float64', nx=130, w_on_x=False, bins=('boxes', 34, 0),
                    integer=integer, seed=608, nt=False, batches=((37,),)))
  return out


def merged_cases():
  """(g) a (br, x) mask: every pair runs once with WBX_BINNED_MASK_ON_W and once without, bit-identical."""
  out = []
  for wl in ('dense', 'x', 'row'):
    out.append(Case(name=_name('g', wl), func=DET6, flags=FLAG_MASKED, wl=wl, mask_on_w=True, lonely=True, seed=700, batches=((37,),)))
  out.append(Case(name='g-ragged', func=DET3, flags=FLAG_MASKED, nx=97, mask_on_w=True, lonely=True, seed=701, nt=False, batches=((37,),)))
  out.append(Case(name='g-float64', func=DET6, flags=FLAG_MASKED, dtype='float64', mask_on_w=True, lonely=True, seed=702, batches=((37,),)))
  out.append(Case(name='g-overflow', func=DET6, flags=FLAG_MASKED, nBr=150, nx=90, bins=('half', 40), mask_on_w=True, lonely=True, seed=703,
                  owner='mixed', nt=False, batches=((50,), (50,), (50,))))
  return out


def special_cases():
  """(j) one non-finite value in the cell NAN_CELL of six."""
  out = []
  kw = dict(nA=3, nBk=2, nBr=37, nx=97, nt=False, batches=((37,),))
  out.append(Case(name='j-zero-weight', func=DET3, flags=0, special='zero_weight', seed=801, **kw))
  out.append(Case(name='j-zero-weight-masked', func=DET6, flags=FLAG_MASKED, special='zero_weight', seed=802, **kw))
  out.append(Case(name='j-masked-out', func=DET6, flags=FLAG_MASKED, special='masked_out', seed=803, **kw))
  out.append(Case(name='j-no-bin', func=DET3, flags=0, special='no_bin', seed=804, **kw))
  out.append(Case(name='j-no-bin-masked', func=DET3, flags=FLAG_MASKED, special='no_bin', seed=805, **kw))
  out.append(Case(name='j-last-live-lane', func=DET6, flags=0, special='last_live', seed=806, **kw))
  out.append(Case(name='j-c-only', func=DET6, flags=FLAG_MASKED, special='c_only', seed=807, **kw))
  out.append(Case(name='j-empty-patch', func=DET3, flags=0, special='empty_patch', bins=('right', 34), seed=808, **kw))
  out.append(Case(name='j-slot-owned', func=DET3, flags=FLAG_MASKED, special='no_bin', bins=('random', 40), seed=809, owner='slot', **kw))
  return out


def inf_cases():
  kw = dict(nA=3, nBk=2, nBr=37, nx=97, nt=False, batches=((37,),), special='inf')
  return [Case(name='j-inf-atom', func=DET6, flags=0, seed=811, **kw),
          Case(name='j-inf-slot', func=DET6, flags=FLAG_MASKED, bins=('random', 40), seed=812, owner='slot', **kw)]


def forward_cases_for_reversal():
  """(i) the forward views whose mirror images (reverse_view) take the all-slot route."""
  out = []
  for fname in ('det3', 'det6'):
    for mode in ('plain', 'masked'):
      for integer in (False, True):
        out.append(Case(name=_name('i', fname, mode, 'int' if integer else 'rnd'), func=FUNCS[fname], flags=MODES[mode], nx=97, nt=False, integer=integer,
                        seed=900, batches=((37,),)))
  for wl in ('x', 'row'):  # (the slot kernel's factored-weight flavours with every patch theirs)
    for integer in (False, True):
      out.append(Case(name=_name('i-det6-skipna', wl, 'int' if integer else 'rnd'), func=DET6, flags=FLAG_SKIPNA, wl=wl, nx=97, nt=False, integer=integer,
                      seed=902, batches=((37,),)))
  out.append(Case(name='i-empty-patch', func=DET3, flags=0, nA=3, nBk=2, nx=97, nt=False, special='empty_patch', bins=('right', 34), seed=901,
                  batches=((37,),)))
  return out


def prepared_table_cases():
  """(h) two sets of bins on ONE geometry (the atom tables of both have the same size and can share a device buffer): boxes, free of
  overflow, and 'half', whose first two row splits overflow."""
  kw = dict(func=DET6, flags=FLAG_MASKED, nA=2, nBk=2, nBr=150, nx=90, nt=False, batches=((50,), (50,), (50,)))
  return [Case(name='h-clean', bins=('boxes', 34, 0), seed=1001, **kw), Case(name='h-overflowing', bins=('half', 40), seed=1002, owner='mixed', **kw)]


def all_forward_cases():
  return (matrix_cases() + ragged_cases() + batch_cases() + uneven_cases() + overflow_cases() + word_cases() + merged_cases() + special_cases()
          + inf_cases() + forward_cases_for_reversal() + prepared_table_cases())


def by_name(name):
  (case,) = [c for c in all_forward_cases() if c.name == name]
  return case
