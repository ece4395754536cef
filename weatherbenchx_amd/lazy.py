"""Deferred per-point statistics: how an unfused plugin API is lowered to fused kernels.

The reference contract is "Statistic.compute returns a full-resolution array, the Aggregator reduces it"
(weatherbenchX/metrics/base.py:135-158, weatherbenchX/aggregation.py:337-366).  Materialising that
array on the GPU would double HBM traffic, so the built-in statistics return a `LazyStatistic`: a
DataArray (dims, coords, mask coordinate all present) whose payload is only computed -- by the HIP map
kernel -- if somebody actually reads `.data`/`.values`.  Statistics built from the same
(predictions, targets[, climatology]) arrays share one `FusedGroup`; the Aggregator asks the group for
all lanes at once, which is one stage-1 launch that reads every input exactly once.
"""
from __future__ import annotations

import collections
import os
import weakref
from typing import Sequence

import numpy as np

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import planner
from weatherbenchx_amd import replay
from weatherbenchx_amd import xarray_lite as xr

DET_LANE = {'Error': 0, 'AbsoluteError': 1, 'SquaredError': 2, 'SquaredPredictionAnomaly': 3,
            'SquaredTargetAnomaly': 4, 'AnomalyCovariance': 5}
ENS_LANE = {'CRPSSkill': 0, 'CRPSSpread': 1, 'EnsembleVariance': 2, 'UnbiasedEnsembleMeanSquaredError': 3,
            'EnsembleMeanSquaredError': 4}


# Indicator launches keep one column of counters per lane and thread in LDS (csrc/wbx_cat.hip): 64 threads x 8 bytes per
# exceedance lane (fp64 fractions), x 4 bytes per rank lane (uint32 counts), 64 KB per launch.
CAT_LDS_BYTES = 64 * 1024


def cat_lanes_per_launch(func: int, masked: bool, skipna: bool) -> int:
  """Value lanes (categories) ONE wbx_cat_partial / wbx_cat_exceed_field launch holds: skipna adds a count lane per value
  lane, a mask alone one shared count lane.  Exceedance: 128 / 127 / 64 thresholds; rank histogram: 256 / 255 / 128 ranks."""
  lanes = CAT_LDS_BYTES // (64 * (4 if func == _hip.CAT_RANK else 8))
  return lanes // 2 if skipna else (lanes - 1 if masked else lanes)


# False (WBX_FUSED_CONTINGENCY=0): thresholded contingency tables (categorical.TruePositives .. behind wrappers.ContinuousToBinary)
# are materialised and reduced on the host route as before wbx_contingency_partial existed (A/B timing and tests).
FUSED_CONTINGENCY = os.environ.get('WBX_FUSED_CONTINGENCY', '1') != '0'
# False (WBX_FUSED_CONTINGENCY_FIELD=0): the same tables at a threshold FIELD (ContinuousToBinary('both', DataArray / Dataset, dim):
# per-gridpoint thresholds such as a climatological percentile) are binarised and reduced on the host route as before
# wbx_contingency_field_partial existed (A/B timing and tests).  WBX_FUSED_CONTINGENCY=0 switches the whole family off, fields included.
FUSED_CONTINGENCY_FIELD = os.environ.get('WBX_FUSED_CONTINGENCY_FIELD', '1') != '0'
# False (WBX_FUSED_ENS_RPS=0): probabilistic.EnsembleRankedProbabilityScore builds the [K, M, frame] indicator arrays of its two
# ContinuousToCDF transforms on the host and reduces them as before wbx_ens_rps_partial existed (A/B timing and tests).
FUSED_ENS_RPS = os.environ.get('WBX_FUSED_ENS_RPS', '1') != '0'
# False (WBX_FUSED_ENS_RPS_FIELD=0): EnsembleRankedProbabilityScore at threshold FIELDS (DataArray / Dataset thresholds such as
# climatological terciles) selects the chunk's thresholds, builds the indicator arrays on the host and reduces them as before
# wbx_ens_rps_field_partial existed (A/B timing and tests).  WBX_FUSED_ENS_RPS is about plain lists of thresholds only.
FUSED_ENS_RPS_FIELD = os.environ.get('WBX_FUSED_ENS_RPS_FIELD', '1') != '0'
# False (WBX_FUSED_ENERGY=0): EnergyScoreSkill / EnergyScoreSpread (EnergyScore, TiledEnergyScore) are labelled-array arithmetic on
# the host -- one whole-array pass per cyclic member offset -- and reduced as before wbx_ens_energy_partial existed (A/B timing, tests).
FUSED_ENERGY = os.environ.get('WBX_FUSED_ENERGY', '1') != '0'
ENERGY_LANE = {'EnergyScoreSkill': 0, 'EnergyScoreSpread': 1}
# False (WBX_FUSED_VARIOGRAM=0): VariogramScore (TiledVariogramScore) is labelled-array arithmetic on the host -- one whole-array pass
# per cyclic offset along its dim -- and reduced as before wbx_ens_variogram_partial existed (A/B timing, tests).
FUSED_VARIOGRAM = os.environ.get('WBX_FUSED_VARIOGRAM', '1') != '0'
# False (WBX_FUSED_WASSERSTEIN=0): WassersteinDistance is a pooled float64 sort and two cumulative sums on the host, reduced as before
# wbx_ens_wasserstein_partial existed (A/B timing, tests).
FUSED_WASSERSTEIN = os.environ.get('WBX_FUSED_WASSERSTEIN', '1') != '0'
# False (WBX_FUSED_INTERVALS=0): Covered, Confident and JaccardDistant (Opportunism) take two host quantile fields each, an aligned
# copy of the climatology and a Boolean array per statistic, reduced as before wbx_ens_interval_partial existed (A/B timing, tests).
FUSED_INTERVALS = os.environ.get('WBX_FUSED_INTERVALS', '1') != '0'
# False (WBX_FUSED_ENS_PROB=0): contingency tables of ensemble event probabilities (TruePositives .. behind ContinuousToBinary('both')
# -> EnsembleMean('predictions') -> ContinuousToBinary / ContinuousToBins('predictions'): RelativeEconomicValue, Reliability) build
# the [K, M, frame] and [K, J, frame] indicator arrays on the host and reduce them as before wbx_ens_prob_contingency_partial existed
# (A/B timing, tests).
FUSED_ENS_PROB = os.environ.get('WBX_FUSED_ENS_PROB', '1') != '0'
# False (WBX_FUSED_SEEPS=0): SEEPS builds an aligned copy of the wet thresholds, six float64 indicator arrays, their six products with
# broadcast coefficient fields and a Boolean mask per chunk and variable, reduced as before wbx_seeps_partial existed (A/B timing,
# tests).
FUSED_SEEPS = os.environ.get('WBX_FUSED_SEEPS', '1') != '0'
# False (WBX_FUSED_FSS=0): SquaredFractionsError, SquaredPredictionFraction and SquaredTargetFraction (FSS) each form their
# neighbourhood means as whole-array float64 running sums per size and hand three float32 fields to the reduction, as before
# wbx_fss_partial existed (A/B timing, tests).
FUSED_FSS = os.environ.get('WBX_FUSED_FSS', '1') != '0'
FSS_TERM = {'SquaredFractionsError': 0, 'SquaredPredictionFraction': 1, 'SquaredTargetFraction': 2}  # value lanes (wbx.h)
FSS_SIZE_DIM = 'neighborhood_size'
# reductions of fused FSS statistics that the stencil's plan could not serve and that took the host route instead, with the plan's
# reasons (tests and tools read these, like replay.STATS)
FSS_STATS = {'plan_declined': 0, 'reasons': []}
# False (WBX_FUSED_FSS_THRESHOLDS=0): the FSS terms behind ContinuousToBinary('both', thresholds, dim) binarise both inputs on the host
# route (two [frame, K] float32 indicator arrays per variable) before the statistic sees them, as before wbx_fss_threshold_partial
# existed (A/B timing, tests).  Only effective while FUSED_FSS is on.
FUSED_FSS_THRESHOLDS = os.environ.get('WBX_FUSED_FSS_THRESHOLDS', '1') != '0'
# False (WBX_FUSED_BRIER=0): Error, AbsoluteError and SquaredError behind ContinuousToBinary('both') [-> EnsembleMean /
# WeibullEnsembleToProbabilistic('predictions')] (the Brier score and its kin) build the [K, M, frame] indicator arrays on the host
# and reduce them as before wbx_ens_brier_partial existed (A/B timing, tests).
FUSED_BRIER = os.environ.get('WBX_FUSED_BRIER', '1') != '0'
BRIER_STAT = {'Error': 0, 'AbsoluteError': 1, 'SquaredError': 2}  # lane blocks (wbx.h)
# False (WBX_FUSED_ENS_QUANTILES=0): Error, AbsoluteError and SquaredError behind EnsembleQuantiles('predictions') build the float64
# [Q, frame] quantile array on the host (np.quantile / torch.quantile) and reduce the statistic of it as before
# wbx_ens_quantile_error_partial existed (A/B timing, tests).
FUSED_ENS_QUANTILES = os.environ.get('WBX_FUSED_ENS_QUANTILES', '1') != '0'
CONT_CELL = {'TruePositives': 0, 'FalsePositives': 1, 'FalseNegatives': 2, 'TrueNegatives': 3}  # lane blocks (wbx.h)

_frame_memo: list = [None]  # (weakref p, weakref t, mutations, frame without drop_dims): the last (p, t) frame that was computed


def _stat_frame(arrays: Sequence[xr.DataArray], drop_dims=()):
  """dims / sizes / coords of the broadcast of `arrays` (what `a - b` would carry), without computing it."""
  if len(arrays) == 2:
    # `_aligned(p, t)` checks the frame of a pair and the FusedGroup built right after asks for it again (minus the member
    # dim): one walk over the coordinates serves both
    memo = _frame_memo[0]
    a, b = arrays
    muts = (a.__dict__.get('_mutations', 0), b.__dict__.get('_mutations', 0))
    if memo is not None and memo[0]() is a and memo[1]() is b and memo[2] == muts:
      dims, sizes, coords = memo[3]
    elif drop_dims:
      return _stat_frame_walk(arrays, drop_dims)  # (nobody has looked at the whole frame of this pair: it may not even exist)
    else:
      dims, sizes, coords = _stat_frame_walk(arrays)
      _frame_memo[0] = (weakref.ref(a), weakref.ref(b), muts, (dims, sizes, coords))
    if not drop_dims:
      return dims, dict(sizes), dict(coords)
    drop = set(drop_dims)
    if drop & set(dims):
      # a dropped dim changes which coordinates collide: walk again with it (the member dim is on p only: not the case here)
      if any(d in b.dims for d in drop) or any(d in a.dims and d in b.dims for d in drop):
        return _stat_frame_walk(arrays, drop_dims)
    return (tuple(d for d in dims if d not in drop), {d: n for d, n in sizes.items() if d not in drop},
            {k: v for k, v in coords.items() if not (set(v[0]) & drop)})
  return _stat_frame_walk(arrays, drop_dims)


def _stat_frame_walk(arrays: Sequence[xr.DataArray], drop_dims=()):
  dims, sizes = [], {}
  for a in arrays:
    for d, n in a.sizes.items():
      if d in drop_dims:
        continue
      if d not in dims:
        dims.append(d)
        sizes[d] = n
      elif sizes[d] != n:
        if all(d in x._coords for x in arrays if d in x.dims):  # pylint: disable=protected-access
          raise _NeedsAlignment(d)  # labeled dims of different length: inner join like xarray arithmetic
        raise ValueError(f'cannot broadcast: size mismatch along {d!r} ({sizes[d]} vs {n})')
  coords = {}
  dropped = set()
  for a in arrays:
    for k, (cd, cv) in a._coords.items():  # pylint: disable=protected-access
      if set(cd) & set(drop_dims) or k in dropped:
        continue
      if k in coords:
        d0, v0 = coords[k]
        if d0 != cd or not xr._values_equal(v0, cv):  # pylint: disable=protected-access
          if k in dims:
            raise _NeedsAlignment(k)
          del coords[k]
          dropped.add(k)
      else:
        coords[k] = (cd, cv)
  return tuple(dims), sizes, coords


class _NeedsAlignment(Exception):
  pass


class ClimatologyRef(xr.LazyPickleMixin, xr.DataArray):
  """The climatology aligned with valid_time (metrics/base.py:382-403) -- as an index table, not a copy.

  Built-in statistics only read `.source` / `.positions` and let the stage-1 kernel gather whole climatology fields
  in place.  For user-defined `PerVariableStatisticWithClimatology` plugins it still IS the aligned DataArray the
  reference would hand over: touching `.data` / doing arithmetic materialises the gather (on the device for torch
  payloads)."""

  origin = None    # (host climatology, its positions) when `source` is a slab pool (climatology_cache.SlabCache.ref)
  activate = None  # slab pool: the launch streams wait for the slabs still on their way (called before the launches)

  def __init__(self, source: xr.DataArray, over_dims: tuple, positions: dict):
    self.source = source          # dims e.g. (dayofyear, hour, level, latitude, longitude)
    self.over_dims = tuple(over_dims)    # statistic dims the selection varies over, e.g. (init_time, lead_time)
    self.positions = positions    # climatology dim -> int positions, shape = sizes of over_dims
    self._data = None
    self._dims = self.aligned_dims()
    self.name = source.name
    self.attrs = dict(source.attrs)
    self._coords = {k: v for k, v in source._coords.items() if not set(v[0]) & set(positions)}  # pylint: disable=protected-access

  def aligned_dims(self):
    return self.over_dims + tuple(d for d in self.source.dims if d not in self.positions)

  @property
  def shape(self):
    first = np.asarray(next(iter(self.positions.values()))) if self.positions else np.zeros(())  # (no positions: the source as it is)
    return tuple(first.shape) + tuple(self.source.sizes[d] for d in self.source.dims if d not in self.positions)

  @property
  def dtype(self):
    return self.source.dtype

  @property
  def data(self):
    if self._data is None:
      self._data = self.aligned_view().data
    return self._data

  def aligned_view(self) -> xr.DataArray:
    """The aligned climatology as a plain labeled array (a gather of whole fields)."""
    # (behind a slab pool: gathered from the HOST climatology the pool caches -- what a user-defined statistic is handed is
    #  the reference's `climatology.sel(...).compute()`, metrics/base.py:396-403)
    src, positions = self.origin if self.origin is not None else (self.source, self.positions)
    if not positions:  # nothing is selected (a threshold field without a time dim): the source itself
      return xr.DataArray(src.data, dims=src.dims, coords=dict(src._coords), _raw_coords=True)  # pylint: disable=protected-access
    order = [src.dims.index(d) for d in positions] + [i for i, d in enumerate(src.dims) if d not in positions]
    data = xr._transpose(src.data, order)  # pylint: disable=protected-access
    gather = tuple(np.asarray(positions[d]).reshape(-1) for d in positions)
    if xr._is_torch(data):  # pylint: disable=protected-access
      import torch  # pylint: disable=g-import-not-at-top
      gather = tuple(torch.as_tensor(g, device=data.device) for g in gather)
    g = data[gather]
    shape = tuple(np.asarray(next(iter(positions.values()))).shape)
    g = g.reshape(shape + tuple(xr._shape(g)[1:]))  # pylint: disable=protected-access
    coords = {k: v for k, v in src._coords.items() if not set(v[0]) & set(positions)}  # pylint: disable=protected-access
    return xr.DataArray(g, dims=self.aligned_dims(), coords=coords, _raw_coords=True)


def _reduce_in_blocks(subs, reduce_one, join):
  """reduce_one(sub) -> (values, counts, out_dims) for every block of `subs`, one launch each, joined on the host right away."""
  values, counts, out_dims = [], [], None
  with engine.synchronous_results():
    for sub in subs:
      v, c, out_dims = reduce_one(sub)
      values.append(np.array(v, dtype=np.float64))  # (own memory: the next launch reuses the result buffers)
      counts.append(np.array(c, dtype=np.float64))
  return join(values), join(counts), out_dims


def _reduce_threshold_blocks(launch, thr, ngroup: int, block: int, **extra):
  """Statistics whose lanes are `ngroup` groups of one lane per threshold, lane g * K + k (the 4 cells of a contingency table, the 3
  Brier-type statistics): one launch -- `cat` = {'thresholds', **extra} -- for up to `block` thresholds; more are cut into blocks --
  thresholds are independent of one another --, one launch each, joined on the host group by group: the result is
  (ngroup * K,) + out_dims whatever the number of launches.  ONE launch is handed on as it is: nothing is joined, so the result may
  still be pending (deferred read-back, chunk records)."""
  thr = np.asarray(thr, np.float64)
  nthr = int(thr.size)
  if nthr <= block:
    return launch(dict(extra, thresholds=thr))
  # (group, k of the block) + out_dims; the sizes are spelled out: an out dim of length 0 leaves nothing to infer them from
  groups = lambda a: a.reshape((ngroup, a.shape[0] // ngroup) + a.shape[1:])
  return _reduce_in_blocks([dict(extra, thresholds=np.ascontiguousarray(thr[k0:k0 + block])) for k0 in range(0, nthr, block)], launch,
                           lambda parts: np.concatenate([groups(a) for a in parts], axis=1).reshape(
                               (ngroup * nthr,) + parts[0].shape[1:]))


def _reduce_position_blocks(launch, size: int, ngroup: int, block: int, **extra):
  """_reduce_threshold_blocks for thresholds that lie along a dim of input 2 (a threshold field): a block is named by its POSITIONS
  along that dim, one launch -- `cat` = {'thr_first', 'nthr', 'size', **extra} -- per block of at most `block` of the `size`
  thresholds, each block advancing 'thr_first'; the same lanes g * K + k, joined in the same way, ONE launch handed on as it is."""
  if size <= block:
    return launch(dict(extra, thr_first=0, nthr=size, size=size))
  groups = lambda a: a.reshape((ngroup, a.shape[0] // ngroup) + a.shape[1:])
  return _reduce_in_blocks([dict(extra, thr_first=k0, nthr=min(block, size - k0), size=size) for k0 in range(0, size, block)], launch,
                           lambda parts: np.concatenate([groups(a) for a in parts], axis=1).reshape(
                               (ngroup * size,) + parts[0].shape[1:]))


def _group_known(p, t, kind: str, pred=lambda key: True) -> bool:
  """A group of kind `kind` of these very objects exists (`pred`: of the rest of its key): an earlier statistic has checked
  their frames."""
  table = p.__dict__.get('_wbx_groups')
  return bool(table) and any(k[0] == kind and k[1] == id(t) and k[2] == t.__dict__.get('_mutations', 0) and pred(k)
                             and v[0]() is t and v[1]() is not None for k, v in table.items())


class FusedGroup:
  """All fused statistics over one (predictions, targets[, climatology]) triple.  What differs between kinds -- input 2, how `reduce`
  runs, where per-point values come from -- is a row of `_LAZY_KINDS` below."""

  def __init__(self, kind: str, p: xr.DataArray, t: xr.DataArray, ens=None, cat=None):
    self.kind = kind
    self.p, self.t = p, t
    self.ens = ens  # {'member_dim', 'M'}; kind 'enrg': + {'fair' (None: no spread statistic has said yet), 'norm_dims', 'norm_sizes'};
    # kind 'vgrm': + {'fair': False, 'norm_dims' (the score's one dim), 'norm_sizes', 'power'}; kinds 'ens2', 'wass': + {'N'}
    self.cat = cat  # indicator statistics: {'func', 'ncat', 'thresholds', 'member_dim', 'M'}; kind 'ivl': {'lanes', 'params',
    # 'quantile_dim'} (engine._ivl_operands), growing as statistics join; kind 'seeps': {'dry_threshold', 'table', 'place_dims',
    # 'device_tables', 'host', 'mask_da'} (seeps_statistic); kind 'fss': {'sizes', 'scalar', 'wrap_longitude', 'masks' (one DataArray
    # per size, or None), 'thresholds' (float64 ndarray, or None: binary inputs), 'threshold_dim', 'coord'} (fss_statistic); kind 'brier': {'thresholds', 'values', 'coord', 'threshold_dim', 'denom'} (brier_statistic) or {'quantiles': True, 'thresholds': the levels, 'values', 'coord', 'threshold_dim'} (quantile_error_statistic);
    # kind 'erpsf': {'bin_dim', 'nthr', 'side_dim', 'right_inclusive', 'host'} (ens_rps_field_statistic);
    # kind 'cont' at a threshold field: {'threshold_dim', 'size' (thresholds along it), 'coord' (its labels, or None)}
    # (contingency_field_statistic)
    self.clim: ClimatologyRef | None = None
    self._clim_key = None
    drop = (ens['member_dim'],) if ens else ((cat['member_dim'],) if cat and cat.get('member_dim') else ())
    if ens:  # a point is one index of the frame without the member dim and the dims the norm / the pairs run over ('enrg', 'vgrm')
      drop += tuple(ens.get('norm_dims', ()))
    self.dims, self.sizes, self.coords = _stat_frame([p, t], drop_dims=drop)
    self.cache: dict = {}

  def attach_climatology(self, ref: ClimatologyRef, key, own_dims=()) -> bool:
    """`own_dims`: dims of the climatology that the kernel addresses itself (the quantile dim of the interval statistics)."""
    if self.clim is None:
      # frame check: aligned climatology dims must already be statistic dims (it only broadcasts)
      for d in ref.aligned_dims():
        if d not in self.dims and d not in own_dims:
          return False
      for d in ref.source.dims:
        if d in self.dims and d in ref.source._coords and d in self.coords:  # pylint: disable=protected-access
          if not xr._values_equal(ref.source._coords[d][1], self.coords[d][1]):  # pylint: disable=protected-access
            return False
      self.clim, self._clim_key = ref, key
      return True
    return self._clim_key == key

  @property
  def mask(self) -> xr.DataArray | None:
    if self.cat and self.cat.get('mask_da') is not None:  # ('seeps': the places whose dry fraction is in range)
      return self.cat['mask_da']
    if 'mask' in self.coords:
      cd, cv = self.coords['mask']
      # a mask that was built in HBM (data.add_nan_mask_to_data on device payloads) is consumed there
      return xr.DataArray(cv if xr._is_torch(cv) else np.asarray(cv), dims=cd)  # pylint: disable=protected-access
    return None

  # -- execution ---------------------------------------------------------------------------------
  def inputs_and_func(self):
    third = _LAZY_KINDS[self.kind].third
    inputs = [self.p, self.t]
    if third == 'required' or (third == 'optional' and self.clim is not None):
      inputs.append(self.clim.source)
    if self.kind != 'det':
      return inputs, 0
    return inputs, (_hip.DET6 if self.clim is not None else _hip.DET3)  # (the climatology brings the anomaly lanes with it)

  def _ens(self, ens_params):
    """The group's `ens` under the settings a statistic of kind 'ens' brings along (algo, fair, skipna)."""
    return dict(self.ens, **ens_params) if ens_params else self.ens

  def reduce(self, reduce_dims, w_da, bin_dims, *, use_mask: bool, skipna: bool, ens_params=None, extra_reduce=()):
    how = _LAZY_KINDS[self.kind].reduce
    inputs, func = self.inputs_and_func()
    mask = self.mask if use_mask else None
    reduce_dims = tuple(reduce_dims) + tuple(extra_reduce)
    if how in (_GATHER, _GATHER_IN_PLACE):
      return _reduce_with_gather(self.kind, inputs, self.dims, self.sizes, reduce_dims, w_da, bin_dims, func=func, mask=mask,
                                 skipna=skipna, clim=self.clim, ens=self._ens(ens_params), cat=self.cat, may_align=how == _GATHER)
    if how == _PER_SIZE:
      return self._reduce_fss(inputs, reduce_dims, w_da, bin_dims, use_mask, skipna)
    # (the fair / inclusive settings of an 'erps' / 'enrg' group and the power of a 'vgrm' group are its own)
    if self.clim is not None:  # ('cont' at a field: blocks of thresholds of the field, which is input 2 of every launch)
      launch = lambda cat: _reduce_with_gather(self.kind, inputs, self.dims, self.sizes, reduce_dims, w_da, bin_dims, func=func,
                                               mask=mask, skipna=skipna, clim=self.clim, ens=self.ens, cat=cat, may_align=False)
    else:
      launch = lambda cat: engine.reduce_statistics(self.kind, inputs, self.dims, self.sizes, reduce_dims, w_da, bin_dims, mask=mask,
                                                    skipna=skipna, ens=self.ens, cat=cat)
    return launch(self.cat) if how == _PLAIN else how(self, launch, mask, skipna)

  def _reduce_cat(self, launch, mask, skipna):
    """Indicator statistics: one launch where the categories fit its LDS columns (cat_lanes_per_launch), else -- thresholds
    are independent of one another -- one launch per block of categories that fits, the results joined along the category
    axis.  The ranks of a histogram are not independent (a point adds to ONE of its M + 1 bins, whichever): no split."""
    cat = self.cat
    ncat, func = int(cat['ncat']), int(cat['func'])
    block = cat_lanes_per_launch(func, mask is not None, skipna)
    if ncat > block and func == _hip.CAT_RANK:
      how = 'with skipna' if skipna else ('under a mask' if mask is not None else 'without mask and skipna')
      raise ValueError(f'RankHistogram: {ncat - 1} members need {ncat} rank lanes, but one launch holds {block} {how} '
                       f'(at most {block - 1} members); the ranks of a histogram cannot be split over launches')
    if ncat <= block:
      return launch(cat)
    return _reduce_in_blocks(self._cat_blocks(block), launch, lambda parts: np.concatenate(parts, axis=0))

  def _reduce_fss(self, inputs, reduce_dims, w_da, bin_dims, use_mask, skipna):
    """The three terms of the fractions skill score: one launch per neighbourhood size (wbx_fss_partial; the shared count lane of a
    mask does not allow several sizes in one), each under the mask of the statistic for ITS size, joined on the host term by term:
    the result is (3 * K,) + out_dims with lane term * K + k.  A scalar size is one launch and nothing is joined.
    Thresholded continuous inputs (cat['thresholds']): one entry call (wbx_fss_threshold_partial) per size and block of at most
    _hip.FSS_THR_MAX thresholds, the mask of a size serving all of them; a call's lanes 3 j + term are joined on the host into
    (3 * K * J,) + out_dims with lane term * (K * J) + k * J + j, J the number of thresholds.  ONE call (one size, one block) is
    handed on as it is, lanes 3 j + term (LazyFSS.lanes_interleaved tells the Aggregator): nothing is joined, so the result may
    still be pending (deferred read-back, chunk records)."""
    cat = self.cat
    sizes, masks = list(cat['sizes']), cat['masks']
    thr = cat.get('thresholds')

    def launch(k, thresholds=None):
      sub = {'n': int(sizes[k]), 'wrap_longitude': bool(cat['wrap_longitude'])}
      if thresholds is not None:
        sub['thresholds'] = thresholds
      return engine.reduce_statistics('fss', inputs, self.dims, self.sizes, reduce_dims, w_da, bin_dims,
                                      mask=masks[k] if (use_mask and masks is not None) else None, skipna=skipna, cat=sub)
    nl = _hip.FSS_LANES
    if thr is not None:
      nthr, block = int(thr.size), _hip.FSS_THR_MAX
      cuts = [(k, j0, min(j0 + block, nthr)) for k in range(len(sizes)) for j0 in range(0, nthr, block)]
      blocks = {j0: np.ascontiguousarray(thr[j0:j1]) for _, j0, j1 in cuts}  # (one table per block: uploaded once per contents)
      if len(cuts) == 1:
        return launch(0, blocks[0])

      def join(parts):
        out = np.empty((nl, len(sizes), nthr) + parts[0].shape[1:], np.float64)
        for (k, j0, j1), a in zip(cuts, parts):  # (the sizes are spelled out: an out dim of length 0 leaves nothing to infer them from)
          out[:, k, j0:j1] = np.moveaxis(a.reshape((j1 - j0, nl) + a.shape[1:]), 1, 0)
        return out.reshape((nl * len(sizes) * nthr,) + parts[0].shape[1:])
      return _reduce_in_blocks(cuts, lambda cut: launch(cut[0], blocks[cut[1]]), join)
    if len(sizes) == 1:
      return launch(0)
    return _reduce_in_blocks(range(len(sizes)), launch,
                             lambda parts: np.stack(parts, axis=1).reshape((nl * len(parts),) + parts[0].shape[1:]))

  def _reduce_epc(self, launch):
    """Contingency tables of ensemble event probabilities: one launch for up to _hip.EPC_MAX_PAIRS (event threshold k, probability
    slot j) pairs; more are cut into blocks -- pairs are independent of one another --, along j first and, where the thresholds
    alone are more than a launch holds, along k too, one launch each, joined on the host cell by cell: the result is (4 * K * J,) +
    out_dims with lane cell * (K * J) + k * J + j whatever the number of launches."""
    thr = np.asarray(self.cat['thresholds'], np.float64).reshape(-1)
    slots = np.asarray(self.cat['slots'], np.int32).reshape(-1, 2)
    nthr, nslot, block = int(thr.size), int(slots.shape[0]), _hip.EPC_MAX_PAIRS
    if nthr * nslot <= block:
      return launch({'thresholds': thr, 'slots': slots})
    bk = min(nthr, block)
    bj = max(1, block // bk)
    cuts = [(k0, min(k0 + bk, nthr), j0, min(j0 + bj, nslot)) for k0 in range(0, nthr, bk) for j0 in range(0, nslot, bj)]
    subs = [{'thresholds': np.ascontiguousarray(thr[k0:k1]), 'slots': np.ascontiguousarray(slots[j0:j1])} for k0, k1, j0, j1 in cuts]

    def join(parts):
      out = np.empty((_hip.EPC_CELLS, nthr, nslot) + parts[0].shape[1:], np.float64)
      for (k0, k1, j0, j1), a in zip(cuts, parts):  # (the sizes are spelled out: an out dim of length 0 leaves nothing to infer them from)
        out[:, k0:k1, j0:j1] = a.reshape((_hip.EPC_CELLS, k1 - k0, j1 - j0) + a.shape[1:])
      return out.reshape((_hip.EPC_CELLS * nthr * nslot,) + parts[0].shape[1:])
    return _reduce_in_blocks(subs, launch, join)

  def _cat_blocks(self, block: int):
    """self.cat cut into runs of at most `block` categories (kept: a block's threshold table / field is uploaded once)."""
    memo = self.__dict__.setdefault('_cat_block_memo', {})
    if block not in memo:
      cat, subs = self.cat, []
      for k0 in range(0, int(cat['ncat']), block):
        k1 = min(k0 + block, int(cat['ncat']))
        sub = dict(cat, ncat=k1 - k0)
        if cat.get('thr_field') is not None:
          field, cdim = cat['thr_field'], cat['cat_dim']
          ax = field.dims.index(cdim)
          vals = np.ascontiguousarray(np.take(np.asarray(field.values, np.float64), np.arange(k0, k1), axis=ax))
          sub['thr_field'] = xr.DataArray(vals, dims=field.dims, coords={d: field.coords[d].values for d in field.dims
                                                                         if d != cdim and d in field.coords})
        else:
          sub['thresholds'] = np.ascontiguousarray(cat['thresholds'][k0:k1])
        subs.append(sub)
      memo[block] = subs
    return memo[block]

  def materialise(self, lane: int, ens_params=None) -> np.ndarray:
    row = _LAZY_KINDS[self.kind]
    if row.host is not None:
      # the per-point values are the host route's, bit for bit, in whatever array type it gives (a tensor for torch payloads):
      # whoever reads them sees what it saw before the fused reduction existed
      return row.host(self, lane)(self.p, self.t).transpose(*self.dims).data
    if row.points is not None:  # stage 1 with every dim kept IS the per-point statistic ('ivl': `lane` among the lanes launched)
      with engine.synchronous_results():
        values, _, out_dims = self.reduce((), None, (), use_mask=False, skipna=False)
      arr = np.asarray(values, np.float64)[lane]
      return row.points(self, np.ascontiguousarray(np.transpose(arr, [out_dims.index(d) for d in self.dims])))
    inputs, func = self.inputs_and_func()
    gather, inputs = _gather_spec(self.clim, inputs, self.dims, self.kind)
    return engine.materialise(self.kind, inputs, self.dims, self.sizes, lane, func=func, gather=gather, ens=self._ens(ens_params))


def gather_from_ref(clim: ClimatologyRef, dtype_code: int) -> planner.GatherSpec:
  """Element-offset gather table of an aligned climatology from its device layout (the climatology itself is uploaded once and
  cached on its DataArray)."""
  ctx = _hip.default_context()
  if clim.origin is not None and str(clim.source.dtype) != ('float32' if dtype_code == _hip.F32 else 'float64'):
    raise ValueError(f'the slab-cached climatology is {clim.source.dtype} but the statistic is evaluated in '
                     f"{'float32' if dtype_code == _hip.F32 else 'float64'}: cast the climatology (or the fields) to one dtype")
  if clim.activate is not None:
    clim.activate()  # slab pool: the launch streams wait for slabs that are still on the copy stream (asked for a chunk ahead)
  dev = engine._to_device(ctx, clim.source, dtype_code)  # pylint: disable=protected-access
  table = np.zeros(tuple(np.asarray(next(iter(clim.positions.values()))).shape), dtype=np.int64)
  for d, pos in clim.positions.items():
    table = table + np.asarray(pos, dtype=np.int64) * dev.layout.stride(d)
  return planner.GatherSpec(dims=tuple(clim.over_dims), table=table)


def _gather_dtype(kind, inputs) -> int:
  """The dtype input 2 goes to the device in: the inputs' common one, or its own (engine._KINDS: 'erpsf', the threshold field)."""
  if engine._KINDS[kind].own_dtype2:  # pylint: disable=protected-access
    return engine.own_dtype(inputs[2])
  return engine._common_dtype([i.data for i in inputs])  # pylint: disable=protected-access


def _gather_spec(clim: ClimatologyRef | None, inputs, dims, kind):
  """Element-offset gather table for the climatology input, from its device layout."""
  if clim is None or not clim.positions:  # (no positions: a threshold field without a time dim, nothing to gather)
    return None, inputs
  return gather_from_ref(clim, _gather_dtype(kind, inputs)), inputs


def _regather(p_new, g):
  """replay.ChunkRecord: the plan variant of a recorded launch for the chunk whose predictions are `p_new` -- the climatology
  positions of ITS time labels (metrics/base.py: `_climatology_ref`, cached per label set), the gather table from them, the
  cached plan with that table swapped in."""
  from weatherbenchx_amd.metrics import base as metrics_base  # pylint: disable=g-import-not-at-top
  try:
    ref = metrics_base.PerVariableStatisticWithClimatology._climatology_ref(p_new, g['source'])  # pylint: disable=protected-access
    if tuple(ref.over_dims) != tuple(g['over_dims']):
      return None
    return g['replan'](gather_from_ref(ref, g['dtype_code']))
  except (ValueError, KeyError):
    return None


def _regather_bins(p_new, g):
  """_regather for a threshold field (kind 'erpsf'): the positions are wrappers.bin_threshold_positions of the new chunk."""
  from weatherbenchx_amd.metrics import base as metrics_base  # pylint: disable=g-import-not-at-top
  from weatherbenchx_amd.metrics import wrappers  # pylint: disable=g-import-not-at-top
  try:
    over_dims, positions = wrappers.bin_threshold_positions(g['source'], p_new)
    if tuple(over_dims) != tuple(g['over_dims']):
      return None
    ref = metrics_base._aligned_ref(g['source'], over_dims, positions)  # pylint: disable=protected-access
    return g['replan'](gather_from_ref(ref, g['dtype_code']))
  except (ValueError, KeyError):
    return None


def _reduce_with_gather(kind, inputs, dims, sizes, reduce_dims, w_da, bin_dims, *, func, mask, skipna, clim, ens, cat=None,
                        may_align=True):
  """`may_align` False: a gather along the innermost dim is the caller's error (kind 'seeps': its score table is addressed by the
  climatology's own places, which an aligned copy does not have)."""
  gather, inputs = _gather_spec(clim, inputs, dims, kind)
  rec = replay.active() if clim is not None else None
  if rec is not None:  # a chunk that is being recorded: what its gather plans have to be rebuilt from for the next chunk
    rec.gather_context = {'source': clim.origin[0] if clim.origin is not None else clim.source, 'p': inputs[0], 'over_dims': tuple(clim.over_dims),
                          'dtype_code': _gather_dtype(kind, inputs), 'regather': _LAZY_KINDS[kind].regather}
  try:
    return engine.reduce_statistics(kind, inputs, dims, sizes, reduce_dims, w_da, bin_dims, func=func, mask=mask,
                                    skipna=skipna, gather=gather, ens=ens, cat=cat)
  except ValueError as e:
    if clim is None or 'innermost' not in str(e) or not may_align:
      raise
    # the selection runs along the contiguous dim: align the climatology first, then fuse as usual
    aligned = clim.aligned_view()
    inputs = list(inputs[:2]) + [aligned]
    return engine.reduce_statistics(kind, inputs, dims, sizes, reduce_dims, w_da, bin_dims, func=func, mask=mask,
                                    skipna=skipna, gather=None, ens=ens, cat=cat)
  finally:
    if rec is not None:
      rec.gather_context = None


def _like_payload(arr, *das):
  """`arr` as a tensor on the device of the first of `das` whose payload is one -- the array type the host route gives --, else as
  it is."""
  for da in das:
    if xr._is_torch(da.data):  # pylint: disable=protected-access
      import torch  # pylint: disable=g-import-not-at-top
      return torch.as_tensor(arr, device=da.data.device)
  return arr


def _rebuilt(build):
  """host(group, lane) of a row below: the host route of the `multivariate` statistic that `build(multivariate, group, lane)` makes
  from what the group holds."""
  def host(g, lane):
    from weatherbenchx_amd.metrics import multivariate  # pylint: disable=g-import-not-at-top
    return build(multivariate, g, lane).host_per_variable
  return host


# What FusedGroup does per kind, beside engine._KINDS (the same keys).  Rows are looked up by `group.kind` when needed: nothing
# callable is kept on a group or a statistic, which are pickled.
#   third:    input 2, the source of `group.clim` (a climatology, the wet thresholds, a threshold field): None, 'optional' ('det': it
#             also chooses DET6 over DET3) or 'required'
#   reduce:   _GATHER: one launch through _reduce_with_gather, input 2 gathered in place like ACC's climatology ('ivl': one launch for
#             every lane asked for so far) and aligned first where the selection runs along the innermost dim;  _GATHER_IN_PLACE:
#             the same, never aligned ('seeps': its score table is addressed by the climatology's own places);  _PER_SIZE: one
#             launch per neighbourhood size under that size's mask (FusedGroup._reduce_fss);  _PLAIN: one launch;  or
#             blocks(group, launch, mask, skipna): one launch(cat) per block of what a launch holds, joined on the host
#   host:     host(group, lane) -> (p, t) -> the host route's per-point values, what `.values` of a statistic gives;  else
#   points:   points(group, arr) -> the per-point values from `arr`, lane `lane` of stage 1 with every dim kept, float64 over the
#             group's dims, in the array type the host route gives;  neither: engine.materialise
#   regather: of a recorded chunk's gather context (replay.ChunkRecord), how input 2 is gathered for the next chunk
_GATHER, _GATHER_IN_PLACE, _PER_SIZE, _PLAIN = 'gather', 'gather in place', 'per size', 'plain'
_LazyKind = collections.namedtuple('_LazyKind', 'third reduce host points regather', defaults=(None, _PLAIN, None, None, _regather))
_host_of_cat = lambda g, lane: g.cat['host']  # (categorical.SEEPS._one; EnsembleRankedProbabilityScore.host_per_variable)
_LAZY_KINDS = {
    'det': _LazyKind('optional', _GATHER),
    'ens': _LazyKind(None, _GATHER),
    'ens2': _LazyKind(points=lambda g, arr: arr),
    'cat': _LazyKind(reduce=FusedGroup._reduce_cat),  # pylint: disable=protected-access
    # (second arm, a threshold FIELD -- `group.clim`, input 2 of every launch --: blocks of positions along the field's threshold dim)
    'cont': _LazyKind('optional', lambda g, launch, mask, skipna:
                      _reduce_position_blocks(launch, int(g.cat['size']), _hip.CONT_CELLS, _hip.CONT_MAX_THRESHOLDS,
                                              threshold_dim=g.cat['threshold_dim'])
                      if g.clim is not None else
                      _reduce_threshold_blocks(launch, g.cat['thresholds'], _hip.CONT_CELLS, _hip.CONT_MAX_THRESHOLDS)),
    'erps': _LazyKind(host=_rebuilt(lambda mv, g, lane: mv.EnsembleRankedProbabilityScore(  # (the indicator arrays of the two
        # ContinuousToCDF transforms and labelled-array arithmetic on them)
        g.cat['p_values'], g.cat['t_values'], g.cat['bin_dim'], '', ensemble_dim=g.ens['member_dim'], skipna_ensemble=False,
        fair=g.ens['fair'], enforce_monotonicity=False, right_inclusive=g.cat['right_inclusive']))),
    'erpsf': _LazyKind('required', _GATHER, host=_host_of_cat, regather=_regather_bins),
    'epc': _LazyKind(reduce=lambda g, launch, mask, skipna: g._reduce_epc(launch)),  # pylint: disable=protected-access
    'brier': _LazyKind(reduce=lambda g, launch, mask, skipna:  # (quantile levels, not event thresholds: the row's second arm)
                       _reduce_threshold_blocks(launch, g.cat['thresholds'], _hip.QERR_STATS, _hip.QERR_MAX_QUANTILES, quantiles=True)
                       if g.cat.get('quantiles') else
                       _reduce_threshold_blocks(launch, g.cat['thresholds'], _hip.BRIER_STATS, _hip.BRIER_MAX_THRESHOLDS,
                                                denom=int(g.cat['denom']))),
    'enrg': _LazyKind(host=_rebuilt(lambda mv, g, lane:
                                    mv.EnergyScoreSkill(dim=list(g.ens['norm_dims']), ensemble_dim=g.ens['member_dim'])
                                    if lane == ENERGY_LANE['EnergyScoreSkill'] else
                                    mv.EnergyScoreSpread(dim=list(g.ens['norm_dims']), ensemble_dim=g.ens['member_dim'],
                                                         fair=g.ens['fair'] is not False))),
    'vgrm': _LazyKind(host=_rebuilt(lambda mv, g, lane: mv.VariogramScore(dim=g.ens['norm_dims'][0], ensemble_dim=g.ens['member_dim'],
                                                                          p=g.ens['power']))),
    'wass': _LazyKind(points=lambda g, arr: _like_payload(arr, g.p, g.t)),
    'ivl': _LazyKind('optional', _GATHER, points=lambda g, arr: _like_payload(arr != 0, g.p)),  # (Boolean statistics)
    'seeps': _LazyKind('required', _GATHER_IN_PLACE, host=_host_of_cat),
    'fss': _LazyKind(reduce=_PER_SIZE),
}


def _group_for(kind: str, p: xr.DataArray, t: xr.DataArray, ens=None, clim_key=None, cat=None) -> FusedGroup:
  """The FusedGroup shared by every statistic built from these very (p, t) objects."""
  # (the table holds the group WEAKLY: the group holds p, and a strong p -> table -> group -> p cycle kept a chunk's result
  # buffers -- views of pooled page-locked / device memory cached on the group -- away from their pools until the cyclic
  # collector happened to run; a chunk loop then allocated fresh memory job after job: 2.5 instead of 1.0 ms per chunk)
  table = p.__dict__.setdefault('_wbx_groups', {})
  key = (kind, id(t), t.__dict__.get('_mutations', 0), ens['member_dim'] if ens else None, clim_key)
  hit = table.get(key)
  if hit is not None and hit[0]() is t:
    grp = hit[1]()
    if grp is not None:
      return grp
  grp = FusedGroup(kind, p, t, ens=ens, cat=cat)
  if len(table) > 8:  # entries of groups that have died
    for k in [k for k, v in table.items() if v[1]() is None]:
      del table[k]
  table[key] = (weakref.ref(t), weakref.ref(grp))
  return grp


class LazyStatistic(xr.LazyPickleMixin, xr.DataArray):
  """A per-point statistic that is a DataArray in every respect, evaluated on demand by a HIP kernel."""

  def __init__(self, group: FusedGroup, lane: int, name=None, ens_params=None, mean_dims=(), coord_names=None):
    # deliberately no super().__init__: the payload does not exist yet
    self._data = None
    self._dims = tuple(d for d in group.dims if d not in mean_dims)
    self.name = name
    self.attrs = {}
    dset = set(self._dims)
    # coord_names: statistics of the predictions alone (EnsembleVariance, CRPSSpread) carry the predictions' coordinates
    # only -- in particular not the targets' `mask` (probabilistic.py:250-273: `predictions.var(...)`)
    self._coords = {k: v for k, v in group.coords.items()
                    if set(v[0]) <= dset and (coord_names is None or k in coord_names)}
    self._group = group
    self._lane = lane
    self._ens_params = ens_params
    self._mean_dims = tuple(mean_dims)
    self._coord_names = coord_names

  @property
  def is_lazy(self) -> bool:
    return self._data is None

  @property
  def data(self):
    if self._data is None:
      arr = self._group.materialise(self._lane, self._ens_params)
      if self._mean_dims:
        axes = tuple(self._group.dims.index(d) for d in self._mean_dims)
        arr = arr.mean(axis=axes)
      self._data = arr
    return self._data

  @property
  def shape(self):
    return tuple(self._group.sizes[d] for d in self._dims)

  @property
  def dtype(self):
    return np.dtype(np.float64)

  def mean(self, dim=None, skipna=None, **kw):
    """Mean over a dim that nothing else depends on stays lazy (EnsembleAveragedStatistic,
    probabilistic.py:35-69): it becomes one more reduced dim of the fused launch."""
    dims = (dim,) if isinstance(dim, str) else tuple(dim or ())
    # only an explicit skipna=False stays lazy: the default (None) drops NaNs like DataArray.mean / xarray do
    if (self.is_lazy and dims and skipna is False and all(d in self._dims for d in dims)
        and self._group.kind == 'det'):
      return LazyStatistic(self._group, self._lane, name=self.name, ens_params=self._ens_params,
                           mean_dims=self._mean_dims + dims, coord_names=self._coord_names)
    return super().mean(dim, skipna=skipna, **kw)


class LazyEnsembleMean(xr.LazyPickleMixin, xr.DataArray):
  """`predictions.mean(ensemble_dim)` (wrappers.py:116-148) that remembers where it came from, so
  SquaredError of it is served by the ensemble kernel's lane 4 without a second pass over the members."""

  def __init__(self, source: xr.DataArray, ensemble_dim: str):
    self._data = None
    self._dims = tuple(d for d in source.dims if d != ensemble_dim)
    self.name = source.name
    self.attrs = dict(source.attrs)
    dset = set(self._dims)
    self._coords = {k: v for k, v in source._coords.items() if set(v[0]) <= dset}  # pylint: disable=protected-access
    self._source = source
    self._ensemble_dim = ensemble_dim

  @property
  def is_lazy(self) -> bool:
    return self._data is None

  @property
  def data(self):
    if self._data is None:
      self._data = xr.DataArray.mean(self._source, self._ensemble_dim, skipna=False).data
    return self._data

  @property
  def shape(self):
    return tuple(self._source.sizes[d] for d in self._dims)

  @property
  def dtype(self):
    return self._source.dtype


# ---- constructors used by the metric classes ---------------------------------------------------------
def _aligned(p: xr.DataArray, t: xr.DataArray):
  try:
    _stat_frame([p, t])
    return p, t
  except _NeedsAlignment:
    return xr.align(p, t, join='inner')


def det_statistic(stat_name: str, p, t, climatology_ref: ClimatologyRef | None = None, clim_key=None) -> xr.DataArray:
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if isinstance(p, LazyEnsembleMean) and p.is_lazy and stat_name == 'SquaredError':
    return ens_statistic('EnsembleMeanSquaredError', p._source, t, p._ensemble_dim)  # pylint: disable=protected-access
  if not _group_known(p, t, 'det'):
    p, t = _aligned(p, t)
  # one group per (p, t): Error/AbsoluteError/SquaredError and the anomaly statistics of the FIRST
  # climatology share a launch; a second, different climatology gets its own group.
  grp = _group_for('det', p, t)
  if climatology_ref is not None and not grp.attach_climatology(climatology_ref, clim_key):
    grp = _group_for('det', p, t, clim_key=clim_key)
    if not grp.attach_climatology(climatology_ref, clim_key):
      raise ValueError('climatology does not broadcast against predictions/targets '
                       f'(climatology dims {climatology_ref.aligned_dims()}, statistic dims {grp.dims})')
  return LazyStatistic(grp, DET_LANE[stat_name], name=p.name)


def _same_mask(p: xr.DataArray, t: xr.DataArray) -> bool:
  pm, tm = p._coords.get('mask'), t._coords.get('mask')  # pylint: disable=protected-access
  if tm is None:
    return True
  return pm is not None and pm[0] == tm[0] and xr._values_equal(pm[1], tm[1])  # pylint: disable=protected-access


# True: CRPSSpread(use_sort=False) launches the register-tiled O(M^2) pair kernel (EnsOpF32<..., PAIRWISE>) instead of the
# rank-form kernel.  A measurement switch (bench.py's `pairwise_form`, tools/kbench.py): the results agree to ~1e-7.
PAIR_FORM_KERNEL = False


def ens_statistic(stat_name: str, p, t, ensemble_dim: str, *, use_sort=False, fair=True,
                  skipna_ensemble=False, member_only=False) -> xr.DataArray:
  """`member_only`: the statistic looks at `p` alone (EnsembleVariance, CRPSSpread); `t` is only the kernel's companion
  operand.  Its frame and coordinates are then those of `p` -- the reference computes it from the predictions, so a
  `mask` coordinate or an extra dim of the targets must not leak into it (Aggregator(masked=True) leaves such a statistic
  unmasked, aggregation.py:339-352).  While `t` has the frame of `p` the (p, t) launch of the other lanes is shared."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if ensemble_dim not in p.dims:
    raise ValueError(f'Dimension {ensemble_dim} not found in {p.dims}')
  if ensemble_dim in t.dims:
    raise ValueError(f'targets must not carry {ensemble_dim!r} here (select a member or use target_members())')
  coord_names = None
  if member_only:
    if not (set(t.dims) <= set(p.dims) and _same_mask(p, t)):
      t = first_member(p, ensemble_dim)  # a companion with exactly the predictions' frame
    coord_names = frozenset(p._coords)  # pylint: disable=protected-access
  if not _group_known(p, t, 'ens', lambda k: k[3] == ensemble_dim):
    p, t = _aligned(p, t)
  m = p.sizes[ensemble_dim]
  grp = _group_for('ens', p, t, ens={'member_dim': ensemble_dim, 'M': m})
  # use_sort=False (the reference's default, probabilistic.py:644) asks for the O(M^2) pair form of the SAME number -- the
  # reference's own CRPSSpread.unique_name leaves use_sort out (probabilistic.py:189-192), i.e. it treats the two forms as
  # one statistic.  On this hardware the rank form is the cheaper way to that number (51 members: 0.31 against 0.51 ms per
  # 1.73 GB) and all five lanes of a (p, t) pair come out of ONE launch, so both settings run the rank-form kernel; the
  # register-tiled pair kernel stays reachable through PAIR_FORM_KERNEL for measurements.
  # skipna_ensemble needs per-point member counts: the generic pair-form kernel (WBX_FLAG_SKIPNA_ENS).
  pair = bool(skipna_ensemble) or (not use_sort and PAIR_FORM_KERNEL)
  params = {'algo': _hip.ENS_PAIRWISE if pair else _hip.ENS_SORT, 'fair': bool(fair), 'skipna': bool(skipna_ensemble)}
  return LazyStatistic(grp, ENS_LANE[stat_name], name=p.name, ens_params=params, coord_names=coord_names)


class LazyCategorical(xr.LazyPickleMixin, xr.DataArray):
  """An indicator statistic (ErrorExceedance, EnsembleErrorExceedance, RankHistogram): the frame of (p, t) plus ONE new
  trailing dimension of categories.  The Aggregator reduces all categories in one launch (wbx_cat_partial) -- or, past what a
  launch's LDS columns hold, in one launch per block of thresholds (FusedGroup._reduce_cat); reading `.data` evaluates the
  same kernel without reducing anything.

  `split` = (dims, shape, coords): the kernel's category axis stands for these trailing dims -- none (a threshold field that
  adds no dimension: one category, squeezed out) or several (a field that adds two or more: stacked for the kernel)."""

  def __init__(self, group: FusedGroup, cat_dim: str, cat_coord, name=None, split=None):
    self._data = None
    self._split = None if split is None else (tuple(split[0]), tuple(int(n) for n in split[1]), dict(split[2]))
    self._dims = tuple(group.dims) + ((cat_dim,) if split is None else self._split[0])
    self.name = name
    self.attrs = {}
    self._coords = dict(group.coords)
    if cat_coord is not None and split is None:
      self._coords[cat_dim] = ((cat_dim,), np.asarray(cat_coord))
    if split is not None:
      for d, c in self._split[2].items():
        self._coords[d] = ((d,), np.asarray(c))
    self._group = group
    self._cat_dim = cat_dim

  @property
  def is_lazy(self) -> bool:
    return self._data is None

  @property
  def ncat(self) -> int:
    return int(self._group.cat['ncat'])

  @property
  def cat_dims(self) -> tuple:
    """The statistic's dims that the kernel's category axis stands for."""
    return (self._cat_dim,) if self._split is None else self._split[0]

  def split_categories(self, a: np.ndarray, axis: int) -> np.ndarray:
    """`a` with its category axis replaced by the dims it stands for -- always a view (an axis is split or dropped)."""
    if self._split is None:
      return a
    v = a.reshape(a.shape[:axis] + self._split[1] + a.shape[axis + 1:])
    if a.size and not np.may_share_memory(v, a):
      raise RuntimeError('internal: category split copied a pending result')
    return v

  @property
  def data(self):
    if self._data is None:
      grp = self._group
      with engine.synchronous_results():
        values, _, out_dims = grp.reduce((), None, (), use_mask=False, skipna=False)
      arr = np.moveaxis(np.asarray(values, np.float64), 0, -1)
      arr = np.transpose(arr, [out_dims.index(d) for d in grp.dims] + [len(out_dims)])
      self._data = self.split_categories(np.ascontiguousarray(arr), arr.ndim - 1)
    return self._data

  @property
  def shape(self):
    return tuple(self._group.sizes[d] for d in self._group.dims) + ((self.ncat,) if self._split is None else self._split[1])

  @property
  def dtype(self):
    return np.dtype(np.float64)


class LazyContingency(xr.LazyPickleMixin, xr.DataArray):
  """One cell (TruePositives / FalsePositives / FalseNegatives / TrueNegatives) of the contingency table of (p > thr, t > thr)
  along a new trailing `threshold_dim`: what `_Indicator` of the `ContinuousToBinary`-transformed inputs is.  The four cells of
  one (p, t) pair and threshold list share a FusedGroup of kind 'cont', so the Aggregator gets all of them from one launch
  (wbx_contingency_partial).  Reading `.data` materialises this cell on the host exactly as the unfused route does -- float32
  indicator arithmetic on the binarised inputs -- and needs no device."""

  def __init__(self, group: FusedGroup, cell: int, threshold_dim: str, name=None):
    self._data = None
    self._dims = tuple(group.dims) + (threshold_dim,)
    self.name = name
    self.attrs = {}
    self._coords = dict(group.coords)
    self._coords[threshold_dim] = ((threshold_dim,), np.asarray(group.cat['coord']))
    self._group = group
    self._cell = int(cell)
    self._threshold_dim = threshold_dim

  @property
  def is_lazy(self) -> bool:
    return self._data is None

  @property
  def nthr(self) -> int:
    return int(np.asarray(self._group.cat['thresholds']).size)

  # what the Aggregator's route for the four cells asks (shared with LazyEnsProbContingency)
  @property
  def lane_dims(self) -> tuple:
    return (self._threshold_dim,)

  @property
  def lane_shape(self) -> tuple:
    return (self.nthr,)

  @staticmethod
  def launchable() -> bool:
    return FUSED_CONTINGENCY and engine.contingency_available(_hip.default_context())

  def frame(self) -> xr.DataArray:
    """The statistic's frame without the threshold dim -- dims, sizes, coordinates (the mask among them), a payload of zeros that
    takes no memory: what coordinate-only weightings and binnings are asked for their W with (one object per group)."""
    grp = self._group
    if getattr(grp, 'frame_proxy', None) is None:
      zeros = np.broadcast_to(np.zeros((), np.float32), tuple(grp.sizes[d] for d in grp.dims))
      grp.frame_proxy = xr.DataArray._assemble(zeros, tuple(grp.dims), dict(grp.coords), name=self.name)  # pylint: disable=protected-access
    return grp.frame_proxy

  @property
  def data(self):
    if self._data is None:
      from weatherbenchx_amd.metrics import categorical, wrappers  # pylint: disable=g-import-not-at-top
      grp = self._group
      values = list(grp.cat['values'])
      pb = wrappers.binarize_thresholds(grp.p, values, self._threshold_dim)
      tb = wrappers.binarize_thresholds(grp.t, values, self._threshold_dim)
      predicted, observed = ((True, True), (True, False), (False, True), (False, False))[self._cell]
      out = categorical._indicator(pb, tb, predicted, observed)  # pylint: disable=protected-access
      self._data = out.transpose(*self._dims).data
    return self._data

  @property
  def shape(self):
    return tuple(self._group.sizes[d] for d in self._group.dims) + (self.nthr,)

  @property
  def dtype(self):
    return np.dtype(np.float32)


class LazyContingencyField(LazyContingency):
  """LazyContingency at a threshold FIELD: the thresholds of `ContinuousToBinary('both', DataArray / Dataset, dim)` vary with the
  point (the local climatological 95th percentile, a per-station warning level).  The four cells of one (p, t, field) share a
  FusedGroup of kind 'cont' whose `clim` is the field, so the Aggregator gets all of them from one launch per block of
  _hip.CONT_MAX_THRESHOLDS thresholds (wbx_contingency_field_partial).  Reading `.data` is the unfused route on the host, as for
  lists.  The threshold dim is labelled where the field labels it."""

  def __init__(self, group: FusedGroup, cell: int, threshold_dim: str, name=None):
    self._data = None
    self._dims = tuple(group.dims) + (threshold_dim,)
    self.name = name
    self.attrs = {}
    self._coords = dict(group.coords)
    if group.cat['coord'] is not None:
      self._coords[threshold_dim] = ((threshold_dim,), np.asarray(group.cat['coord']))
    self._group = group
    self._cell = int(cell)
    self._threshold_dim = threshold_dim

  @property
  def nthr(self) -> int:
    return int(self._group.cat['size'])

  @staticmethod
  def launchable() -> bool:
    return (FUSED_CONTINGENCY and FUSED_CONTINGENCY_FIELD
            and engine.contingency_field_available(_hip.default_context()))

  @property
  def data(self):
    if self._data is None:
      from weatherbenchx_amd.metrics import categorical, wrappers  # pylint: disable=g-import-not-at-top
      grp = self._group
      field = grp.clim.aligned_view() if grp.clim.positions else grp.clim.source
      pb = wrappers.binarize_thresholds(grp.p, field, self._threshold_dim)
      tb = wrappers.binarize_thresholds(grp.t, field, self._threshold_dim)
      predicted, observed = ((True, True), (True, False), (False, True), (False, False))[self._cell]
      out = categorical._indicator(pb, tb, predicted, observed)  # pylint: disable=protected-access
      self._data = out.transpose(*self._dims).data
    return self._data


class LazyBrier(xr.LazyPickleMixin, xr.DataArray):
  """Error, AbsoluteError or SquaredError of (the fraction of members over a threshold, or the indicator of a deterministic
  prediction) against (the target is over that threshold) along a new trailing `threshold_dim`: what these statistics are behind
  ContinuousToBinary('both') [-> EnsembleMean / WeibullEnsembleToProbabilistic('predictions')].  The three statistics of one (p, t)
  pair, threshold list, member dim and denominator share a FusedGroup of kind 'brier', so the Aggregator gets all of them from one
  launch (wbx_ens_brier_partial).  Reading `.data` runs the transforms and the statistic as labelled-array arithmetic on the host,
  the unfused route's float32 indicator arithmetic, and needs no device."""

  def __init__(self, group: FusedGroup, stat: int, name=None):
    cat = group.cat
    self._data = None
    self._threshold_dim = cat['threshold_dim']
    self._dims = tuple(group.dims) + (self._threshold_dim,)
    self.name = name
    self.attrs = {}
    self._coords = dict(group.coords)
    self._coords[self._threshold_dim] = ((self._threshold_dim,), np.asarray(cat['coord']))
    self._group = group
    self._cell = int(stat)

  @property
  def is_lazy(self) -> bool:
    return self._data is None

  # what the Aggregator's route for lane blocks asks (shared with LazyContingency)
  @property
  def lane_dims(self) -> tuple:
    return (self._threshold_dim,)

  @property
  def lane_shape(self) -> tuple:
    return (int(np.asarray(self._group.cat['thresholds']).size),)

  @staticmethod
  def launchable() -> bool:
    try:
      return FUSED_BRIER and engine.brier_available(_hip.default_context())
    except _hip.WbxUnavailableError:
      return False

  frame = LazyContingency.frame

  @property
  def data(self):
    if self._data is None:
      from weatherbenchx_amd.metrics import wrappers  # pylint: disable=g-import-not-at-top
      grp, cat = self._group, self._group.cat
      pb = wrappers.binarize_thresholds(grp.p, list(cat['values']), self._threshold_dim)
      tb = wrappers.binarize_thresholds(grp.t, list(cat['values']), self._threshold_dim)
      if grp.ens is not None:  # the member mean, or Weibull's plotting position (wrappers.WeibullEnsembleToProbabilistic)
        e, m = grp.ens['member_dim'], int(grp.ens['M'])
        pb = pb.mean(e, skipna=False) if cat['denom'] == m else pb.sum(e, skipna=False) / (m + 1)
      d = pb - tb
      out = (d, abs(d), d ** 2)[self._cell]
      self._data = out.transpose(*self._dims).data
    return self._data

  @property
  def shape(self):
    return tuple(self._group.sizes[d] for d in self._group.dims) + self.lane_shape

  @property
  def dtype(self):
    return np.dtype(np.float32)


def brier_statistic(stat: str, p, t, ensemble_dim, threshold_dim: str, thresholds, denom: int) -> xr.DataArray:
  """`stat` ('Error', 'AbsoluteError', 'SquaredError') of the event probabilities of `p` against the events of `t` as a LazyBrier.
  `ensemble_dim`: the member dim of `p`, or None for a deterministic pair (`denom` = 1); `thresholds`: the plain sequence of real
  numbers the ContinuousToBinary was built with; `denom`: M (the member mean) or M + 1 (Weibull's plotting position).  The (p, t)
  objects, the thresholds' bytes, the member dim and `denom` key the group, so the three statistics of a pair meet in one group."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if ensemble_dim is not None and (ensemble_dim not in p.dims or ensemble_dim in t.dims):
    raise ValueError(f'{ensemble_dim!r} must be a dim of the predictions and not of the targets')
  if threshold_dim in p.dims or threshold_dim in t.dims:
    raise ValueError(f'{threshold_dim!r} is already a dimension of the inputs')
  values = list(thresholds)
  thr = np.asarray(values, np.float64).reshape(-1)
  ckey = ('brier', threshold_dim, thr.tobytes(), int(denom))
  if not _group_known(p, t, 'brier', lambda k: k[3] == ensemble_dim and k[4] == ckey):
    p, t = _aligned(p, t)
  ens = {'member_dim': ensemble_dim, 'M': p.sizes[ensemble_dim], 'fair': False} if ensemble_dim is not None else None
  cat = {'thresholds': thr, 'values': values, 'coord': np.asarray(values), 'threshold_dim': threshold_dim, 'denom': int(denom)}
  grp = _group_for('brier', p, t, ens=ens, clim_key=ckey, cat=cat)
  return LazyBrier(grp, BRIER_STAT[stat], name=p.name)


class LazyQuantileError(LazyBrier):
  """Error, AbsoluteError or SquaredError of (the quantiles of the members of `p`) against `t` along a new LEADING `quantile_dim`:
  what these statistics are behind EnsembleQuantiles('predictions', quantiles).  The three statistics of one (p, t) pair, list of
  levels, member dim and quantile dim share a FusedGroup of kind 'brier' whose `cat` has 'quantiles' set, so the Aggregator gets all of
  them from one launch (wbx_ens_quantile_error_partial), through the lane-block route of LazyBrier.  Reading `.data` runs the
  transform and the statistic as labelled-array arithmetic on the host and needs no device."""

  def __init__(self, group: FusedGroup, stat: int, name=None):
    super().__init__(group, stat, name=name)
    self._dims = (self._threshold_dim,) + tuple(group.dims)  # (the host route's order: transform_fn puts the new dim first)
    self._coords[self._threshold_dim] = ((self._threshold_dim,), np.asarray(group.cat['coord'], np.float64))

  @property
  def result_dims(self) -> tuple:
    return self._dims

  @staticmethod
  def launchable() -> bool:
    try:
      return FUSED_ENS_QUANTILES and engine.ens_quantile_available(_hip.default_context())
    except _hip.WbxUnavailableError:
      return False

  @property
  def data(self):
    if self._data is None:
      from weatherbenchx_amd.metrics import wrappers  # pylint: disable=g-import-not-at-top
      grp, cat = self._group, self._group.cat
      pq = wrappers.EnsembleQuantiles('predictions', list(cat['values']), self._threshold_dim, grp.ens['member_dim']).transform_fn(grp.p)
      d = pq - grp.t
      out = (d, abs(d), d ** 2)[self._cell]
      self._data = out.transpose(*self._dims).data
    return self._data

  @property
  def shape(self):
    return self.lane_shape + tuple(self._group.sizes[d] for d in self._group.dims)

  @property
  def dtype(self):  # NumPy's quantiles are float64 whatever the members are; torch.quantile stays in the input dtype
    p = self._group.p
    return np.dtype(str(p.dtype)) if xr._is_torch(p.data) else np.dtype(np.float64)  # pylint: disable=protected-access


def quantile_error_statistic(stat: str, p, t, ensemble_dim: str, quantile_dim: str, quantiles) -> xr.DataArray:
  """`stat` ('Error', 'AbsoluteError', 'SquaredError') of the `quantiles` (levels in [0, 1]) of the members of `p` against `t` as a
  LazyQuantileError with the host route's dims, (quantile_dim,) + frame, and its float64 quantile coordinate.  The (p, t) objects, the
  levels' bytes, the member dim and the quantile dim key the group, so the three statistics of a pair meet in one group."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if ensemble_dim not in p.dims or ensemble_dim in t.dims:
    raise ValueError(f'{ensemble_dim!r} must be a dim of the predictions and not of the targets')
  if quantile_dim in p.dims or quantile_dim in t.dims or quantile_dim == ensemble_dim:
    raise ValueError(f'{quantile_dim!r} is already a dimension of the inputs')
  values = [float(q) for q in quantiles]
  levels = np.asarray(values, np.float64).reshape(-1)
  if not levels.size or not np.all((levels >= 0.0) & (levels <= 1.0)):
    raise ValueError('Quantiles must be in the range [0, 1]')
  ckey = ('qerr', quantile_dim, levels.tobytes())
  if not _group_known(p, t, 'brier', lambda k: k[3] == ensemble_dim and k[4] == ckey):
    p, t = _aligned(p, t)
  ens = {'member_dim': ensemble_dim, 'M': p.sizes[ensemble_dim], 'fair': False}
  cat = {'quantiles': True, 'thresholds': levels, 'values': values, 'coord': levels, 'threshold_dim': quantile_dim}
  grp = _group_for('brier', p, t, ens=ens, clim_key=ckey, cat=cat)
  return LazyQuantileError(grp, BRIER_STAT[stat], name=p.name)


class LazyFSS(xr.LazyPickleMixin, xr.DataArray):
  """One term of the fractions skill score -- SquaredFractionsError, SquaredPredictionFraction or SquaredTargetFraction -- of (p, t)
  at a neighbourhood size, or at several along a leading `neighborhood_size` dim.  The three terms of one (p, t, sizes, wrap,
  combine_mask) share a FusedGroup of kind 'fss', so the Aggregator gets all of them from one launch per size (wbx_fss_partial).
  Reading `.data` gives the host route's array (torch stays torch) and needs no device.
  With thresholds in the group (fss_statistic(thresholds=...)) p and t are CONTINUOUS fields and the statistic is what the term is
  behind ContinuousToBinary('both', thresholds, threshold_dim): the threshold dim, with its coordinate, sits where
  binarize_thresholds followed by neighborhood_averaging puts it -- after the other non-spatial dims, before latitude and longitude --
  and the launches are wbx_fss_threshold_partial's, one per size and block of thresholds."""

  def __init__(self, group: FusedGroup, term: int, host, mask=None, name=None):
    cat = group.cat
    self._data = None
    rest = tuple(d for d in group.dims if d not in ('latitude', 'longitude'))
    lead = () if cat['scalar'] else (FSS_SIZE_DIM,)
    self._threshold_dim = cat.get('threshold_dim') if cat.get('thresholds') is not None else None
    if self._threshold_dim is not None:
      rest += (self._threshold_dim,)
    self._dims = lead + rest + ('latitude', 'longitude')  # the host route's order: the spatial dims end up last
    self.name = name
    self.attrs = {}
    self._coords = {k: v for k, v in group.coords.items() if k != 'mask'}
    if not cat['scalar']:
      self._coords[FSS_SIZE_DIM] = ((FSS_SIZE_DIM,), np.asarray(list(cat['sizes'])))
    if self._threshold_dim is not None:
      self._coords[self._threshold_dim] = ((self._threshold_dim,), np.asarray(cat['coord']))
    if mask is not None:  # what _FractionStatistic._compute_per_variable attaches
      self._coords['mask'] = (tuple(mask.dims), np.asarray(mask.values, dtype=bool))
    self._group = group
    self._cell = int(term)
    self._host = host

  @property
  def is_lazy(self) -> bool:
    return self._data is None

  # what the Aggregator's route for lane blocks asks (shared with LazyContingency)
  @property
  def lane_dims(self) -> tuple:
    lead = () if self._group.cat['scalar'] else (FSS_SIZE_DIM,)
    return lead + ((self._threshold_dim,) if self._threshold_dim is not None else ())

  @property
  def lane_shape(self) -> tuple:
    lead = () if self._group.cat['scalar'] else (len(self._group.cat['sizes']),)
    return lead + ((int(self._group.cat['thresholds'].size),) if self._threshold_dim is not None else ())

  @property
  def threshold_dim(self):
    """The threshold dim of a thresholded statistic, else None."""
    return self._threshold_dim

  @property
  def lanes_interleaved(self) -> bool:
    """Whether the group's reduction comes as lanes 3 j + term (one call of wbx_fss_threshold_partial, handed on unjoined) instead
    of term * K + k (FusedGroup._reduce_fss)."""
    cat = self._group.cat
    return self._threshold_dim is not None and len(cat['sizes']) == 1 and int(cat['thresholds'].size) <= _hip.FSS_THR_MAX

  @property
  def result_dims(self) -> tuple:
    return self._dims

  def launchable(self) -> bool:
    try:
      ctx = _hip.default_context()
      if self._threshold_dim is not None:
        return FUSED_FSS and FUSED_FSS_THRESHOLDS and engine.fss_available(ctx) and engine.fss_thresholds_available(ctx)
      return FUSED_FSS and engine.fss_available(ctx)
    except _hip.WbxUnavailableError:
      return False

  frame = LazyContingency.frame

  @property
  def data(self):
    if self._data is None:
      self._data = self._host().transpose(*self._dims).data
    return self._data

  @property
  def shape(self):
    sizes = dict(self._group.sizes, **{FSS_SIZE_DIM: len(self._group.cat['sizes'])})
    if self._threshold_dim is not None:
      sizes[self._threshold_dim] = int(self._group.cat['thresholds'].size)
    return tuple(sizes[d] for d in self._dims)

  @property
  def dtype(self):
    wide = (self._threshold_dim is None and str(self._group.p.dtype) == 'float64'
            and 1 in [int(n) for n in self._group.cat['sizes']])  # (binarised fields are float32 whatever the inputs are)
    return np.dtype(np.float64 if wide else np.float32)


def fss_statistic(term: int, p, t, sizes, wrap_longitude: bool, mask, *, combine_mask: bool = False, host=None, name=None,
                  thresholds=None, threshold_dim=None) -> xr.DataArray:
  """Term `term` (FSS_TERM) of the fractions skill score of (p, t) as a LazyFSS.  `sizes`: one odd neighbourhood size or a sequence
  of them (a leading `neighborhood_size` dim); `mask`: what spatial.get_fss_mask returns for these sizes (a Boolean DataArray, the
  size dim leading where there are several) or None -- the mask of the STATISTIC, the kernel does not erode masks; `host()`: the host
  route's DataArray, which whoever reads the per-point values gets.  `thresholds` (the plain sequence of real numbers a
  ContinuousToBinary was built with) and `threshold_dim`: p and t are continuous fields and the term is that of (p > thr, t > thr)
  along `threshold_dim`; the mask has no threshold dim and serves every threshold.  One group per (p, t, sizes, wrap, combine_mask,
  thresholds): the three terms of one FSS meet in it."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  scalar = not isinstance(sizes, (list, tuple, np.ndarray))
  size_list = [int(sizes)] if scalar else [int(n) for n in sizes]
  thr = coord = None
  if thresholds is not None:
    if threshold_dim is None or threshold_dim in p.dims or threshold_dim in t.dims:
      raise ValueError(f'{threshold_dim!r} must be a new dimension of the inputs')
    coord = np.asarray(list(thresholds))
    thr = np.asarray(list(thresholds), np.float64).reshape(-1)
  ckey = ('fss', tuple(size_list), scalar, bool(wrap_longitude), bool(combine_mask), threshold_dim if thr is not None else None,
          thr.tobytes() if thr is not None else None)
  grp = _group_for('fss', p, t, clim_key=ckey, cat={'sizes': size_list, 'scalar': scalar, 'wrap_longitude': bool(wrap_longitude),
                                                     'masks': None, 'thresholds': thr, 'threshold_dim': threshold_dim, 'coord': coord})
  if mask is not None and grp.cat['masks'] is None:  # one DataArray per size: its device copy is cached on the object
    vals = np.asarray(mask.values, dtype=bool)
    mdims = tuple(mask.dims)
    if scalar:
      grp.cat['masks'] = [xr.DataArray(np.ascontiguousarray(vals), dims=mdims)]
    else:
      vals = np.moveaxis(vals, mdims.index(FSS_SIZE_DIM), 0)
      rest = tuple(d for d in mdims if d != FSS_SIZE_DIM)
      grp.cat['masks'] = [xr.DataArray(np.ascontiguousarray(vals[k]), dims=rest) for k in range(len(size_list))]
  return LazyFSS(grp, term, host, mask=mask, name=p.name if name is None else name)



def contingency_statistic(cell: int, p, t, threshold_dim: str, thresholds) -> xr.DataArray:
  """Cell `cell` (0..3: TP, FP, FN, TN) of the 2x2 table of (p > thr_k, t > thr_k) as a LazyContingency.  `thresholds`: the
  plain sequence of real numbers a ContinuousToBinary was built with; the (p, t) objects, the thresholds' bytes and the dim key
  the group, so the four cells of a pair meet in one group."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if threshold_dim in p.dims or threshold_dim in t.dims:
    raise ValueError(f'{threshold_dim!r} is already a dimension of the inputs')
  values = list(thresholds)
  thr = np.asarray(values, np.float64).reshape(-1)
  ckey = ('cont', threshold_dim, thr.tobytes())
  if not _group_known(p, t, 'cont', lambda k: k[4] == ckey):
    p, t = _aligned(p, t)
  cat = {'thresholds': thr, 'values': values, 'coord': np.asarray(values), 'threshold_dim': threshold_dim}
  grp = _group_for('cont', p, t, clim_key=ckey, cat=cat)
  return LazyContingency(grp, cell, threshold_dim, name=p.name)


def contingency_field_statistic(cell: int, p, t, threshold_dim: str, ref: ClimatologyRef, *, clim_key=None) -> xr.DataArray:
  """Cell `cell` (0..3: TP, FP, FN, TN) of the 2x2 table of (p > thr_k, t > thr_k) at the threshold field behind `ref` (its source
  carries `threshold_dim`; the kernel addresses that dim itself) as a LazyContingencyField on a FusedGroup of kind 'cont'
  (wbx_contingency_field_partial).  The (p, t) objects, the field (`clim_key`: its identity and state) and the dim key the group, so
  the four cells of a (p, t, field) meet in one group and one launch per block of thresholds.  Raises ValueError where the field
  does not broadcast against the frame: the caller keeps the host route."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if threshold_dim in p.dims or threshold_dim in t.dims:
    raise ValueError(f'{threshold_dim!r} is already a dimension of the inputs')
  source = ref.source
  if threshold_dim not in source.dims:
    raise ValueError(f'the threshold field has dims {source.dims}')
  ckey = ('contf', clim_key, threshold_dim)
  if not _group_known(p, t, 'cont', lambda k: k[4] == ckey):
    p, t = _aligned(p, t)
  if source.sizes[threshold_dim] > 1 and payload_layout(source).stride(threshold_dim) == 0:
    raise ValueError(f'the threshold dim {threshold_dim!r} of the field is a broadcast view (stride 0)')  # (engine._contf_operands)
  coord = np.asarray(source.coords[threshold_dim].values) if threshold_dim in source.coords else None
  cat = {'threshold_dim': threshold_dim, 'size': int(source.sizes[threshold_dim]), 'coord': coord}
  grp = _group_for('cont', p, t, clim_key=ckey, cat=cat)
  if not grp.attach_climatology(ref, ckey, own_dims=(threshold_dim,)):
    raise ValueError(f'threshold field dims {ref.aligned_dims()} do not broadcast against the statistic dims {grp.dims}')
  return LazyContingencyField(grp, cell, threshold_dim, name=p.name)


EPC_COUNT_DIM = '__member_count__'  # the dim of the column of counts c = 0..M that the slot table is derived from


def ens_prob_slot_table(mean_transform, inner_transform, m: int, ensemble_dim: str, slot_dim: str, like=None):
  """Which member counts c = 0..M put a point into probability slot j, read off the host route itself: `mean_transform`
  (wrappers.EnsembleMean) and then `inner_transform` (ContinuousToBinary / ContinuousToBins on the predictions) applied to a column
  [M, M + 1] of float32 members with c ones among them, and `!= 0` of what comes out (what categorical._indicator reads).  ->
  (slots int32 [J, 2] of runs lo <= c <= hi, lo > hi: an empty slot; the coordinates {name: (dims, values)} the inner transform puts
  on `slot_dim`), or None where a slot's counts are not one contiguous run or the result is not ('count', slot_dim).  `like`: a
  payload (NumPy array or tensor) whose kind and device the column takes."""
  # (kept per contents: the four cells of every variable and chunk ask for the same table)
  values = getattr(inner_transform, '_threshold_value', getattr(inner_transform, '_bin_values', None))
  torch_like = like is not None and xr._is_torch(like)  # pylint: disable=protected-access
  key = None
  if isinstance(values, (list, tuple, np.ndarray)):
    try:
      key = (type(inner_transform).__name__, slot_dim, str(np.asarray(values).dtype), np.asarray(values, np.float64).tobytes(), bool(getattr(inner_transform, '_enforce_monotonicity', False)),
             int(m), ensemble_dim, bool(getattr(mean_transform, '_skipna', False)), str(like.device) if torch_like else None)
    except (TypeError, ValueError):
      key = None
  if key is not None and key in _slot_tables:
    slots, coords = _slot_tables[key]
    return slots.copy(), dict(coords)
  out = _derive_slot_table(mean_transform, inner_transform, m, ensemble_dim, slot_dim, like if torch_like else None)
  if key is not None and out is not None:
    if len(_slot_tables) > 64:
      _slot_tables.clear()
    _slot_tables[key] = (out[0].copy(), dict(out[1]))
  return out


_slot_tables: dict = {}


def _derive_slot_table(mean_transform, inner_transform, m, ensemble_dim, slot_dim, like):
  col = (np.arange(m)[:, None] < np.arange(m + 1)[None, :]).astype(np.float32)
  if like is not None and xr._is_torch(like):  # pylint: disable=protected-access
    import torch  # pylint: disable=g-import-not-at-top
    col = torch.as_tensor(col, device=like.device)
  da = xr.DataArray(col, dims=(ensemble_dim, EPC_COUNT_DIM))
  out = xr.as_dataarray(inner_transform.transform_fn(mean_transform.transform_fn(da)))
  if set(out.dims) != {EPC_COUNT_DIM, slot_dim}:
    return None
  hit = (out != 0).transpose(EPC_COUNT_DIM, slot_dim).values
  hit = np.asarray(hit.cpu() if xr._is_torch(hit) else hit, bool)  # pylint: disable=protected-access
  slots = np.empty((hit.shape[1], 2), np.int32)
  for j in range(hit.shape[1]):
    c = np.flatnonzero(hit[:, j])
    if c.size == 0:
      slots[j] = (1, 0)
    elif int(c[-1]) - int(c[0]) + 1 != c.size:  # (no bin between two edges and no threshold gives this: for transforms to come)
      return None
    else:
      slots[j] = (c[0], c[-1])
  coords = {k: (tuple(v[0]), np.asarray(v[1])) for k, v in out._coords.items() if set(v[0]) == {slot_dim}}  # pylint: disable=protected-access
  return slots, coords


class LazyEnsProbContingency(xr.LazyPickleMixin, xr.DataArray):
  """One cell (TruePositives / FalsePositives / FalseNegatives / TrueNegatives) of the contingency tables of an ensemble's event
  probabilities along two new trailing dims, (event_dim, slot_dim): what `_Indicator` is behind ContinuousToBinary('both', event
  thresholds) -> EnsembleMean('predictions') -> ContinuousToBinary / ContinuousToBins('predictions').  The four cells of one (p, t)
  pair, threshold list and inner transform share a FusedGroup of kind 'epc', so the Aggregator gets all of them from one launch per
  block of pairs (wbx_ens_prob_contingency_partial).  Reading `.data` runs the three transforms and the float32 indicator arithmetic
  on the host exactly as the unfused route does, and needs no device."""

  def __init__(self, group: FusedGroup, cell: int, name=None):
    cat = group.cat
    self._data = None
    self._event_dim, self._slot_dim = cat['event_dim'], cat['slot_dim']
    self._dims = tuple(group.dims) + (self._event_dim, self._slot_dim)
    self.name = name
    self.attrs = {}
    self._coords = dict(group.coords)
    self._coords[self._event_dim] = ((self._event_dim,), np.asarray(cat['event_coord']))
    self._coords.update(cat['slot_coords'])
    self._group = group
    self._cell = int(cell)

  @property
  def is_lazy(self) -> bool:
    return self._data is None

  @property
  def lane_dims(self) -> tuple:
    return (self._event_dim, self._slot_dim)

  @property
  def lane_shape(self) -> tuple:
    cat = self._group.cat
    return (int(np.asarray(cat['thresholds']).size), int(np.asarray(cat['slots']).shape[0]))

  @staticmethod
  def launchable() -> bool:
    return FUSED_ENS_PROB and engine.ens_prob_available(_hip.default_context())

  frame = LazyContingency.frame

  @property
  def data(self):
    if self._data is None:
      from weatherbenchx_amd.metrics import categorical  # pylint: disable=g-import-not-at-top
      grp = self._group
      outer, mean, inner = grp.cat['transforms']
      pb = inner.transform_fn(mean.transform_fn(outer.transform_fn(grp.p)))
      tb = outer.transform_fn(grp.t)
      predicted, observed = ((True, True), (True, False), (False, True), (False, False))[self._cell]
      out = categorical._indicator(pb, tb, predicted, observed)  # pylint: disable=protected-access
      self._data = out.transpose(*self._dims).data
    return self._data

  @property
  def shape(self):
    return tuple(self._group.sizes[d] for d in self._group.dims) + self.lane_shape

  @property
  def dtype(self):
    return np.dtype(np.float32)


def ens_prob_contingency_statistic(cell: int, p, t, ensemble_dim: str, event_dim: str, event_values, slot_dim: str, slot_coords, slots,
                                   transforms, inner_key=None) -> xr.DataArray:
  """Cell `cell` (0..3: TP, FP, FN, TN) of the tables of (the member count over event threshold k lies in slot j, t > threshold k) as
  a LazyEnsProbContingency.  `event_values`: the plain sequence of real numbers the outer ContinuousToBinary was built with;
  `slots`, `slot_coords`: ens_prob_slot_table of the inner transform; `transforms`: (outer, mean, inner), what `.data` runs.  The
  (p, t) objects, the member dim, the bytes of the event thresholds and the inner transform (`inner_key` and its table) key the
  group, so the four cells of a pair meet in one group."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if ensemble_dim not in p.dims or ensemble_dim in t.dims:
    raise ValueError(f'{ensemble_dim!r} must be a dim of the predictions and not of the targets')
  for d in (event_dim, slot_dim):
    if d in p.dims or d in t.dims:
      raise ValueError(f'{d!r} is already a dimension of the inputs')
  values = list(event_values)
  thr = np.asarray(values, np.float64).reshape(-1)
  slots = np.ascontiguousarray(slots, np.int32).reshape(-1, 2)
  ckey = ('epc', event_dim, thr.tobytes(), slot_dim, inner_key, slots.tobytes())
  if not _group_known(p, t, 'epc', lambda k: k[3] == ensemble_dim and k[4] == ckey):
    p, t = _aligned(p, t)
  ens = {'member_dim': ensemble_dim, 'M': p.sizes[ensemble_dim], 'fair': False}
  cat = {'thresholds': thr, 'slots': slots, 'event_dim': event_dim, 'slot_dim': slot_dim, 'event_coord': np.asarray(values),
         'slot_coords': dict(slot_coords), 'transforms': tuple(transforms)}
  grp = _group_for('epc', p, t, ens=ens, clim_key=ckey, cat=cat)
  return LazyEnsProbContingency(grp, cell, name=p.name)


def ens_rps_statistic(p, t, ensemble_dim: str, p_thr, t_thr, fair: bool, right_inclusive: bool, bin_dim: str = 'bin') -> xr.DataArray:
  """EnsembleRankedProbabilityScore of the ensemble `p` against the scalar-valued `t` as a LazyStatistic (lane 0) on a FusedGroup of
  kind 'erps'.  `p_thr` / `t_thr`: plain sequences of as many real numbers, prediction and target thresholds.  The (p, t) objects,
  the bytes of both tables, `fair` and `right_inclusive` key the group; its frame drops the member dim.  `bin_dim` only names
  the threshold dim of the host route behind `.data`, which sums it away."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if ensemble_dim not in p.dims:
    raise ValueError(f'Dimension {ensemble_dim} not found in {p.dims}')
  if ensemble_dim in t.dims:
    raise ValueError(f'targets must not carry {ensemble_dim!r} here')
  p_values, t_values = list(p_thr), list(t_thr)
  pa, tb = np.asarray(p_values, np.float64).reshape(-1), np.asarray(t_values, np.float64).reshape(-1)
  if pa.size != tb.size:
    raise ValueError(f'{pa.size} prediction thresholds against {tb.size} target thresholds')
  ckey = ('erps', pa.tobytes(), tb.tobytes(), bool(fair), bool(right_inclusive), bin_dim)
  if not _group_known(p, t, 'erps', lambda k: k[3] == ensemble_dim):
    p, t = _aligned(p, t)
  ens = {'member_dim': ensemble_dim, 'M': p.sizes[ensemble_dim], 'fair': bool(fair)}
  cat = {'p_thresholds': pa, 't_thresholds': tb, 'right_inclusive': bool(right_inclusive), 'p_values': p_values,
         't_values': t_values, 'bin_dim': bin_dim}
  grp = _group_for('erps', p, t, ens=ens, clim_key=ckey, cat=cat)
  return LazyStatistic(grp, 0, name=p.name)


ERPSF_SIDE_DIM = 'wbx_rps_side'  # the leading axis of two stacked threshold fields: prediction thresholds, target thresholds


def ens_rps_field_statistic(p, t, ensemble_dim: str, ref: ClimatologyRef, *, bin_dim: str, stacked: bool, fair: bool,
                            right_inclusive: bool, host, clim_key=None) -> xr.DataArray:
  """EnsembleRankedProbabilityScore of the ensemble `p` against the scalar-valued `t` at the threshold field behind `ref` (its
  source carries `bin_dim` and, where `stacked`, a leading ERPSF_SIDE_DIM of length 2: prediction thresholds, then target
  thresholds) as a LazyStatistic (lane 0) on a FusedGroup of kind 'erpsf' (wbx_ens_rps_field_partial).  The field is gathered in place
  through `ref`'s positions (wrappers.bin_threshold_positions); the kernel addresses `bin_dim` and the side dim itself.  `host`:
  (p, t) -> the host route's per-point values, what `.data` gives.  Raises ValueError where the field does not broadcast against the
  frame: the caller keeps the host route."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if ensemble_dim not in p.dims or ensemble_dim in t.dims:
    raise ValueError(f'{ensemble_dim!r} must be a dim of the predictions and not of the targets')
  source = ref.source
  if bin_dim not in source.dims or stacked != (ERPSF_SIDE_DIM in source.dims):
    raise ValueError(f'the threshold field has dims {source.dims}')
  ckey = ('erpsf', clim_key, bin_dim, bool(stacked), bool(fair), bool(right_inclusive))
  if not _group_known(p, t, 'erpsf', lambda k: k[3] == ensemble_dim):
    p, t = _aligned(p, t)
  ens = {'member_dim': ensemble_dim, 'M': p.sizes[ensemble_dim], 'fair': bool(fair)}
  cat = {'bin_dim': bin_dim, 'nthr': int(source.sizes[bin_dim]), 'side_dim': ERPSF_SIDE_DIM if stacked else None,
         'right_inclusive': bool(right_inclusive), 'host': host}
  grp = _group_for('erpsf', p, t, ens=ens, clim_key=ckey, cat=cat)
  if not grp.attach_climatology(ref, ckey, own_dims=(bin_dim, ERPSF_SIDE_DIM)):
    raise ValueError(f'threshold field dims {ref.aligned_dims()} do not broadcast against the statistic dims {grp.dims}')
  return LazyStatistic(grp, 0, name=p.name)


def payload_layout(da: xr.DataArray) -> planner.InputLayout:
  """Element strides of `da` as a launch will see it: a device-resident tensor as it is stored, anything else as the C-ordered
  copy that is uploaded."""
  data = da.data
  if xr._is_torch(data) and data.is_cuda:  # pylint: disable=protected-access
    return planner.layout_of(data, da.dims)
  strides, step = {}, 1
  for d in reversed(da.dims):
    strides[d] = step
    step *= int(da.sizes[d])
  return planner.InputLayout(strides=strides, itemsize=4)


def energy_statistic(lane: int, p, t, ensemble_dim: str, norm_dims, fair) -> xr.DataArray:
  """EnergyScoreSkill (lane 0) / EnergyScoreSpread (lane 1) of the ensemble `p` against `t`, the norm over `norm_dims`, as a
  LazyStatistic on a FusedGroup of kind 'enrg' (wbx_ens_energy_partial).  The (p, t) objects, the member dim, the norm dims and
  `fair` key the group, so the skill and the spread of one pair share one launch; `fair` is None for the skill, which does not
  depend on it and joins whichever group of the pair there is.  The group's frame drops the member dim and the norm dims; the
  spread carries the predictions' coordinates only (the host route computes it from the predictions alone)."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  norm_dims = tuple(norm_dims)
  if ensemble_dim not in p.dims or ensemble_dim in t.dims:
    raise ValueError(f'{ensemble_dim!r} must be a dim of the predictions and not of the targets')
  for d in norm_dims:
    if d not in p.dims or d not in t.dims:
      raise ValueError(f'norm dim {d!r} must be a dim of both inputs')
  ens = {'member_dim': ensemble_dim, 'M': p.sizes[ensemble_dim], 'fair': None if fair is None else bool(fair), 'norm_dims': norm_dims,
         'norm_sizes': {d: int(p.sizes[d]) for d in norm_dims}}
  grp = _group_for('enrg', p, t, ens=ens, clim_key=('enrg', norm_dims))
  have = grp.ens['fair']
  if fair is not None and have is not None and have != bool(fair):  # a second spread of the pair with the other divisor
    grp = _group_for('enrg', p, t, ens=ens, clim_key=('enrg', norm_dims, bool(fair)))
  elif fair is not None and have is None:
    if grp.cache and not fair:  # (sums of a launch that took the default divisor)
      grp.cache.clear()
    grp.ens['fair'] = bool(fair)
  coord_names = frozenset(p._coords) if lane == ENERGY_LANE['EnergyScoreSpread'] else None  # pylint: disable=protected-access
  return LazyStatistic(grp, lane, name=p.name, coord_names=coord_names)


def variogram_statistic(p, t, ensemble_dim: str, dim: str, power) -> xr.DataArray:
  """VariogramScore of the ensemble `p` against `t`, the pairs along `dim`, as a LazyStatistic on a FusedGroup of kind 'vgrm'
  (wbx_ens_variogram_partial).  The (p, t) objects, the member dim, `dim` and the power key the group: the statistic's unique name
  does not tell two powers apart, the groups do.  The group's frame drops the member dim and `dim`."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if ensemble_dim not in p.dims or ensemble_dim in t.dims:
    raise ValueError(f'{ensemble_dim!r} must be a dim of the predictions and not of the targets')
  if dim not in p.dims or dim not in t.dims:
    raise ValueError(f'dim {dim!r} must be a dim of both inputs')
  power = float(power)
  ens = {'member_dim': ensemble_dim, 'M': p.sizes[ensemble_dim], 'fair': False, 'norm_dims': (dim,), 'norm_sizes': {dim: int(p.sizes[dim])},
         'power': power}
  grp = _group_for('vgrm', p, t, ens=ens, clim_key=('vgrm', dim, power))
  return LazyStatistic(grp, 0, name=p.name)


def wasserstein_statistic(p, t, ensemble_dim: str) -> xr.DataArray:
  """WassersteinDistance between the ensembles `p` and `t`, each with its own size along `ensemble_dim`, as a LazyStatistic on a
  FusedGroup of kind 'wass' (wbx_ens_wasserstein_partial), lane 0.  The (p, t) objects and the member dim key the group; its frame
  drops the member dim.  Frames or labels that differ raise _NeedsAlignment: the caller keeps the host route, which broadcasts."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  for da in (p, t):
    if ensemble_dim not in da.dims:
      raise ValueError(f'Dimension {ensemble_dim} not found in {da.dims}')
  ens = {'member_dim': ensemble_dim, 'M': p.sizes[ensemble_dim], 'N': t.sizes[ensemble_dim], 'fair': False}
  grp = _group_for('wass', p, t, ens=ens, clim_key=('wass',))
  return LazyStatistic(grp, 0, name=p.name)


class LazyInterval(LazyStatistic):
  """Covered / Confident / JaccardDistant as a Boolean statistic on a FusedGroup of kind 'ivl'.  Its value lane is its place among
  the lanes the group launches, which grows while statistics join: it is looked up when asked for, not fixed here."""

  @property
  def _lane(self) -> int:
    return bin(int(self._group.cat['lanes']) & (self._bit - 1)).count('1')

  @_lane.setter
  def _lane(self, bit: int):
    self._bit = int(bit)

  @property
  def dtype(self):
    return np.dtype(bool)


IVL_QUANTILE_DIM = 'quantile'  # the climatology's dim of quantile levels (categorical.py: `climatology.sel(quantile=...)`)
IVL_MAX_GROUPS = 4  # groups of one (p, t, member dim): a statistic whose parameters differ from its kind's in a group opens the next


def interval_statistic(p, t, clim_ref: ClimatologyRef | None, ensemble_dim: str, which: str, bounds, threshold=None,
                       clim_key=None) -> xr.DataArray:
  """`which` in ('Covered', 'Confident', 'JaccardDistant') of the ensemble `p` -- against `t` (Covered) or the climatology behind
  `clim_ref` (the other two) -- as a LazyInterval on a FusedGroup of kind 'ivl' (wbx_ens_interval_partial).  `bounds`: the two
  quantile levels; `threshold`: confidence_threshold / the Jaccard threshold.  The (p, t) objects, the member dim and the
  climatology key the group, so the three statistics of one Opportunism meet in one group whatever their levels and thresholds,
  and its first reduction launches every lane that has joined by then.  The two levels of a lane become positions along the
  climatology's quantile dim (element offsets once its device layout is known); the climatology itself is gathered in place.
  Raises ValueError / _NeedsAlignment where the launch cannot take the inputs as they stand: the caller keeps the host route."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if ensemble_dim not in p.dims or ensemble_dim in t.dims:
    raise ValueError(f'{ensemble_dim!r} must be a dim of the predictions and not of the targets')
  bit = engine.IVL_BITS[which]
  lane = {'bounds': (float(bounds[0]), float(bounds[1])), 'threshold': None, 'q_index': None}
  if bit != _hip.IVL_COVERED:
    if clim_ref is None or IVL_QUANTILE_DIM not in clim_ref.source.dims:
      raise ValueError(f'{which} needs a climatology with a {IVL_QUANTILE_DIM!r} dim')
    try:
      lane['q_index'] = tuple(int(j) for j in clim_ref.source._index_positions(IVL_QUANTILE_DIM, list(lane['bounds'])))  # pylint: disable=protected-access
    except KeyError as e:
      raise ValueError(str(e)) from e
    lane['threshold'] = float(threshold)
  ens = {'member_dim': ensemble_dim, 'M': p.sizes[ensemble_dim], 'fair': False}
  for n in range(IVL_MAX_GROUPS):
    grp = _group_for('ivl', p, t, ens=ens, clim_key=('ivl', n),
                     cat={'lanes': 0, 'params': {}, 'quantile_dim': IVL_QUANTILE_DIM})
    if bit != _hip.IVL_COVERED and not grp.attach_climatology(clim_ref, clim_key, own_dims=(IVL_QUANTILE_DIM,)):
      if grp.clim is None:  # (not another climatology: this one does not fit the frame)
        raise ValueError(f'climatology dims {clim_ref.aligned_dims()} do not broadcast against the statistic dims {grp.dims}')
      continue
    have = grp.cat['params'].get(bit)
    if have is None:
      if grp.cache:  # sums of a launch without this lane: the value lanes move
        grp.cache.clear()
      grp.cat['params'][bit] = lane
      grp.cat['lanes'] |= bit
    elif have != lane:
      continue
    # Confident and JaccardDistant never look at the targets: the predictions' and the climatology's coordinates only
    names = None if bit == _hip.IVL_COVERED else frozenset(p._coords) | frozenset(clim_ref._coords)  # pylint: disable=protected-access
    return LazyInterval(grp, bit, name=p.name, coord_names=names)
  raise ValueError(f'more than {IVL_MAX_GROUPS} interval groups of one (predictions, targets) pair')


def seeps_statistic(p, t, clim_ref: ClimatologyRef, *, table, place_dims, dry_threshold: float, device_tables: dict, mask, extra_coords,
                    host, clim_key=None, name=None, mask_da=None) -> xr.DataArray:
  """SEEPS of (p, t) as a LazyStatistic on a FusedGroup of kind 'seeps' (wbx_seeps_partial).  `clim_ref`: the wet thresholds aligned
  with p's valid times (gathered in place); `table`: categorical.seeps_score_table of the places' dry fractions over `place_dims`;
  `device_tables`: the dict its device copies are kept in (the statistic's, one upload per variable, device and layout); `mask`:
  (dims, Boolean values), the host route's `mask` coordinate -- the group reduces under it (`mask_da`: the same as a DataArray that
  outlives the chunk and carries its device copy); `extra_coords`: the coordinates the host
  route's selection of the wet thresholds adds; `host(p, t)`: the host route, which whoever reads the per-point values gets.  One
  group per (p, t, `clim_key`).  Raises ValueError where the wet thresholds do not broadcast against the frame of (p, t)."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  cat = {'dry_threshold': float(dry_threshold), 'table': table, 'place_dims': tuple(place_dims), 'device_tables': device_tables,
         'host': host, 'mask_da': mask_da}
  grp = _group_for('seeps', p, t, clim_key=('seeps', clim_key), cat=cat)
  if not grp.attach_climatology(clim_ref, clim_key):
    raise ValueError(f'wet-threshold dims {clim_ref.aligned_dims()} do not broadcast against the statistic dims {grp.dims}')
  for k, v in extra_coords.items():
    grp.coords.setdefault(k, v)
  grp.coords['mask'] = (tuple(mask[0]), mask[1])
  return LazyStatistic(grp, 0, name=p.name if name is None else name)


ENS2_LANE = {'CRPSSkill': 0, 'UnbiasedEnsembleMeanSquaredError': 1}


def ens2_statistic(stat_name: str, p, t, ensemble_dim: str, *, skipna_ensemble: bool) -> xr.DataArray:
  """Statistics of an ensemble of predictions against an ensemble of TARGETS with per-point member counts on both sides
  (wbx_ens2_partial): both lanes of a (p, t) pair come out of one launch."""
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  for da in (p, t):
    if ensemble_dim not in da.dims:
      raise ValueError(f'Dimension {ensemble_dim} not found in {da.dims}')
  try:  # frames without the member axes (the two ensembles have their own sizes and member labels)
    _stat_frame([p.isel({ensemble_dim: 0}, drop=True), t.isel({ensemble_dim: 0}, drop=True)])
  except _NeedsAlignment:
    p0, t0 = xr.align(p.isel({ensemble_dim: 0}, drop=True), t.isel({ensemble_dim: 0}, drop=True), join='inner')
    p = p.sel({d: p0[d].values for d in p0.dims if d in p0.coords})
    t = t.sel({d: t0[d].values for d in t0.dims if d in t0.coords})
  ens = {'member_dim': ensemble_dim, 'M': p.sizes[ensemble_dim], 'N': t.sizes[ensemble_dim], 'skipna': bool(skipna_ensemble)}
  grp = _group_for('ens2', p, t, ens=ens, clim_key=('ens2', bool(skipna_ensemble)))
  return LazyStatistic(grp, ENS2_LANE[stat_name], name=p.name)


def cat_statistic(func: int, p, t, cat_dim: str, cat_coord, *, thresholds=None, ensemble_dim=None, threshold_field=None,
                  split=None) -> xr.DataArray:
  p, t = xr.as_dataarray(p), xr.as_dataarray(t)
  if ensemble_dim is not None:
    if ensemble_dim not in p.dims:
      raise ValueError(f'Dimension {ensemble_dim} not found in {p.dims}')
    if ensemble_dim in t.dims:
      raise ValueError(f'targets must not carry {ensemble_dim!r} here')
  p, t = _aligned(p, t)
  if cat_dim in p.dims or cat_dim in t.dims:
    raise ValueError(f'{cat_dim!r} is already a dimension of the inputs')
  thr = None if thresholds is None else np.asarray(thresholds, np.float64).reshape(-1)
  if threshold_field is not None:
    # thresholds that depend on the statistic's dims (wbx_cat_exceed_field): a float64 DataArray over (some of) the frame's dims
    # + `cat_dim`, consumed in place through its strides
    threshold_field = xr.as_dataarray(threshold_field)
    extra = [d for d in threshold_field.dims if d != cat_dim and d not in p.dims and d not in t.dims]
    if extra or cat_dim not in threshold_field.dims:
      raise ValueError(f'thresholds over {threshold_field.dims} do not broadcast against the statistic (extra dims {extra})')
    for d in threshold_field.dims:  # same labels on the shared dims (the reference's comparison aligns on them)
      ref = p if d in p.dims else t
      if d != cat_dim and d in threshold_field.coords and d in ref.coords and not xr._values_equal(threshold_field.coords[d].values, ref.coords[d].values):  # pylint: disable=protected-access
        raise ValueError(f'thresholds and inputs carry different {d!r} coordinates: select the common labels first')
    if not xr._is_float(threshold_field.data) or str(threshold_field.dtype) != 'float64':  # pylint: disable=protected-access
      threshold_field = threshold_field.astype(np.float64)
    thr = None
  ncat = (p.sizes[ensemble_dim] + 1) if func == _hip.CAT_RANK else (int(thr.size) if thr is not None else threshold_field.sizes[cat_dim])
  cat = {'func': int(func), 'ncat': ncat, 'thresholds': thr, 'member_dim': ensemble_dim,
         'M': p.sizes[ensemble_dim] if ensemble_dim else 1, 'thr_field': threshold_field, 'cat_dim': cat_dim}
  key = ('cat', int(func), cat_dim, None if thr is None else thr.tobytes(), None if threshold_field is None else id(threshold_field))
  grp = _group_for('cat', p, t, ens=None, clim_key=(key, ensemble_dim), cat=cat)
  return LazyCategorical(grp, cat_dim, cat_coord, name=p.name, split=split)


def first_member(p: xr.DataArray, ensemble_dim: str) -> xr.DataArray:
  """Member 0 of `p` as a (cached) view: the companion operand of statistics that only look at the predictions.  (Not
  `target_members(p)[0]`: that builds a view of EVERY member -- 51 of them, 1.2 ms of host time per chunk on the public
  probabilistic configuration with a mask.)"""
  cache = p.__dict__.setdefault('_wbx_member0', {})
  if ensemble_dim not in cache:
    # (the general isel walks every axis and every coordinate: ~40 us per chunk of the masked public configuration; a view of
    #  member 0 needs one slice and the coordinates that do not live on the member dim)
    ax = p.dims.index(ensemble_dim)
    data = p.data[(slice(None),) * ax + (0,)]
    coords = {k: v for k, v in p._coords.items() if ensemble_dim not in v[0]}  # pylint: disable=protected-access
    cache[ensemble_dim] = xr.DataArray._assemble(data, p.dims[:ax] + p.dims[ax + 1:], coords, name=p.name, attrs=p.attrs)  # pylint: disable=protected-access
  return cache[ensemble_dim]


def target_members(t: xr.DataArray, ensemble_dim: str):
  """The members of an ensemble-valued target as separate (cached) views: statistics that are linear in the target
  member index are evaluated per member and averaged (LinearCombination)."""
  cache = t.__dict__.setdefault('_wbx_members', {})
  if ensemble_dim not in cache:
    cache[ensemble_dim] = [t.isel({ensemble_dim: j}, drop=True) for j in range(t.sizes[ensemble_dim])]
  return cache[ensemble_dim]


class LinearCombination(xr.LazyPickleMixin, xr.DataArray):
  """scale * sum(coeff_i * term_i) of lazy statistics on the same frame.  The weighted reduction is linear, so the
  Aggregator reduces every term with its own fused launch and combines the accumulators (WindVectorSquaredError =
  SE(u) + SE(v), deterministic.py:174-219; CRPSSkill / UnbiasedEnsembleMeanSquaredError against an ensemble of
  targets, probabilistic.py:134-145, 320-336)."""

  def __init__(self, terms, scale: float = 1.0, name=None, coeffs=None):
    first = terms[0]
    self._coeffs = [1.0] * len(terms) if coeffs is None else [float(c) for c in coeffs]
    if len(self._coeffs) != len(terms):
      raise ValueError('one coefficient per term')
    self._data = None
    self._dims = first.dims
    self.name = name
    self.attrs = {}
    self._coords = dict(first._coords)  # pylint: disable=protected-access
    self._terms = list(terms)
    self._scale = float(scale)

  @property
  def is_lazy(self):
    return self._data is None

  @property
  def data(self):
    if self._data is None:
      total = self._terms[0].data * self._coeffs[0] if self._coeffs[0] != 1.0 else self._terms[0].data
      for t, c in zip(self._terms[1:], self._coeffs[1:]):
        total = total + (t.data * c if c != 1.0 else t.data)
      self._data = total * self._scale if self._scale != 1.0 else total
    return self._data

  @property
  def shape(self):
    return self._terms[0].shape

  @property
  def dtype(self):
    return np.dtype(np.float64)
