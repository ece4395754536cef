"""Multivariate and distribution scores of ensembles, and the relative economic value of probability forecasts (counterpart of
weatherbenchX/metrics/probabilistic.py:339-603, 785-833, 1006-1303, 1346-1527).

None of these is on the path SURVEY section 8 names and none has a kernel of its own: the per-point values are labelled-array
arithmetic on whatever holds the payload (NumPy on the host, torch where a chunk is resident in HBM), and their weighted, binned,
masked means are the Aggregator's reduction -- the same kernels as every other statistic.  `metrics.probabilistic` hands these
names on, so `probabilistic.EnergyScore` etc. resolve as in the reference.

Four exceptions, all in how the Aggregator gets its sums -- the per-point values anybody reads are still this arithmetic:
EnsembleRankedProbabilityScore at one plain list of thresholds is reduced by a kernel of its own, wbx_ens_rps_partial
(lazy.ens_rps_statistic), and at threshold fields (a DataArray / Dataset such as climatological terciles) by
wbx_ens_rps_field_partial (rps_field_route, lazy.ens_rps_field_statistic); EnergyScoreSkill and EnergyScoreSpread of one (predictions, targets) pair -- EnergyScore,
TiledEnergyScore -- by one launch of wbx_ens_energy_partial (lazy.energy_statistic); VariogramScore -- TiledVariogramScore -- at
p = 0.5, 1 or 2 by one launch of wbx_ens_variogram_partial (lazy.variogram_statistic); WassersteinDistance between ensembles of at
most 64 members a side by one launch of wbx_ens_wasserstein_partial (lazy.wasserstein_statistic).
"""
from __future__ import annotations

from typing import Mapping

import numpy as np

from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base
from weatherbenchx_amd.metrics import categorical
from weatherbenchx_amd.metrics import deterministic
from weatherbenchx_amd.metrics import wrappers
from weatherbenchx_amd.metrics.probabilistic import ENSEMBLE_DIM
from weatherbenchx_amd.metrics.probabilistic import UnbiasedEnsembleMeanSquaredError


def _dims_tuple(dim) -> tuple:
  return (dim,) if isinstance(dim, str) else tuple(dim)


def _norm_over(da: xr.DataArray, dims: tuple) -> xr.DataArray:
  """Euclidean norm over `dims`; a NaN anywhere in the vector makes its norm NaN."""
  return (da * da).sum(dims, skipna=False)._unary(np.sqrt, 'sqrt')  # pylint: disable=protected-access


class EnsembleRankedProbabilityScore(base.PerVariableStatistic):
  """RPS of an ensemble against bin thresholds: the squared error between the prediction's and the target's empirical CDF at
  every threshold, summed over `bin_dim`.  `fair=True` uses the unbiased ensemble-mean squared error per threshold (debiasing
  in the ensemble size, for whichever side is an ensemble); otherwise the squared error of the ensemble-mean CDFs
  (probabilistic.py:339-477)."""

  def __init__(self, prediction_bin_thresholds, target_bin_thresholds, bin_dim: str, unique_name_suffix: str,
               ensemble_dim: str = ENSEMBLE_DIM, skipna_ensemble: bool = False, fair: bool = True,
               enforce_monotonicity: bool = True, right_inclusive: bool = True):
    self._ensemble_dim = ensemble_dim
    self._skipna_ensemble = skipna_ensemble
    self._fair = fair
    self._bin_dim = bin_dim
    self._unique_name_suffix = unique_name_suffix
    self._thresholds = (prediction_bin_thresholds, target_bin_thresholds)
    self._enforce_monotonicity = enforce_monotonicity
    self._right_inclusive = right_inclusive
    cdf = {which: wrappers.ContinuousToCDF(which=which, threshold_values=values, threshold_dim=bin_dim,
                                           unique_name_suffix=unique_name_suffix, enforce_monotonicity=enforce_monotonicity,
                                           right_inclusive=right_inclusive)
           for which, values in (('predictions', prediction_bin_thresholds), ('targets', target_bin_thresholds))}
    if fair:
      per_threshold = UnbiasedEnsembleMeanSquaredError(ensemble_dim=ensemble_dim, skipna_ensemble=skipna_ensemble)
    else:
      # (targets without the ensemble dim are left as they are; an ensemble of targets is averaged too)
      per_threshold = wrappers.WrappedStatistic(
          deterministic.SquaredError(),
          wrappers.EnsembleMean(which='both', ensemble_dim=ensemble_dim, skipna=skipna_ensemble,
                                skip_if_ensemble_dim_missing=True))
    self._per_threshold = wrappers.WrappedStatistic(wrappers.WrappedStatistic(per_threshold, cdf['targets']), cdf['predictions'])

  @property
  def unique_name(self) -> str:
    return (f'RankedProbabilityScore_{self._ensemble_dim}_skipna_ensemble_{self._skipna_ensemble}_fair_{self._fair}_'
            f'{self._unique_name_suffix}')

  def _compute_per_variable(self, predictions, targets):
    fused = self._fused_per_variable(predictions, targets)
    return fused if fused is not None else self.host_per_variable(predictions, targets)

  def host_per_variable(self, predictions, targets):
    """The score from the indicator arrays of the two ContinuousToCDF transforms, on the host."""
    squared = self._per_threshold.compute({'_': predictions}, {'_': targets})['_']
    return xr.as_dataarray(squared).sum(self._bin_dim, skipna=self._skipna_ensemble)

  def _fused_per_variable(self, predictions, targets):
    """The score as a lazy statistic that the Aggregator reduces with one launch of wbx_ens_rps_partial (lazy.ens_rps_statistic),
    or None when the combination is not the plain one: numbers for thresholds, an ensemble of predictions against scalar-valued
    targets, no per-point member counts.  Thresholds that are fields (DataArray / Dataset) go to _fused_field_per_variable.
    Reading the statistic's values still computes them on the host."""
    if any(isinstance(v, (xr.DataArray, xr.Dataset)) for v in self._thresholds):
      return self._fused_field_per_variable(predictions, targets)
    if not lazy.FUSED_ENS_RPS or self._skipna_ensemble:
      return None
    pa, tb = (wrappers.plain_thresholds(v) for v in self._thresholds)
    if pa is None or tb is None or len(pa) != len(tb) or len(pa) > _hip.ERPS_MAX_THRESHOLDS:
      return None
    fa, fb = np.asarray(pa, np.float64), np.asarray(tb, np.float64)
    if np.isnan(fa).any() or np.isnan(fb).any():
      return None
    if not np.array_equal(np.asarray(pa), np.asarray(tb)):
      return None  # (two lists label the threshold dim differently: the host route joins them on the labels they share)
    p, t = xr.as_dataarray(predictions), xr.as_dataarray(targets)
    e = self._ensemble_dim
    if e not in p.dims or e in t.dims or self._bin_dim in p.dims or self._bin_dim in t.dims or not set(t.dims) <= set(p.dims):
      return None
    if str(p.dtype) not in ('float32', 'float64') or str(t.dtype) not in ('float32', 'float64'):
      return None
    m = p.sizes[e]
    if m > _hip.ERPS_MAX_MEMBERS or (self._fair and m < 2):
      return None
    if self._enforce_monotonicity and not (np.all(np.diff(fa) > 0) and np.all(np.diff(fb) > 0)):
      return None  # (the host route raises)
    try:
      ctx = _hip.default_context()
    except _hip.WbxUnavailableError:  # no device or no library: nothing to launch on (the host route says so where it needs one)
      return None
    if not engine.ens_rps_available(ctx):
      return None
    return lazy.ens_rps_statistic(p, t, e, pa, tb, self._fair, self._right_inclusive, bin_dim=self._bin_dim)

  def _fused_field_per_variable(self, predictions, targets):
    """The score at threshold fields as a lazy statistic that the Aggregator reduces with one launch of wbx_ens_rps_field_partial
    (lazy.ens_rps_field_statistic), the fields gathered in place, or None where rps_field_route, the monotonicity that is asked
    for, or the frame keep the host route."""
    if not lazy.FUSED_ENS_RPS_FIELD:
      return None
    p, t = xr.as_dataarray(predictions), xr.as_dataarray(targets)
    try:
      fields = [v[da.name] if isinstance(v, xr.Dataset) else v for v, da in zip(self._thresholds, (p, t))]
    except KeyError:
      return None  # (the host route raises)
    fields = [xr.as_dataarray(f) if isinstance(f, xr.DataArray) else f for f in fields]
    route, how = rps_field_route(p, t, fields[0], fields[1], ensemble_dim=self._ensemble_dim, bin_dim=self._bin_dim,
                                 skipna_ensemble=self._skipna_ensemble, fair=self._fair)
    if route != 'fused':
      return None
    if self._enforce_monotonicity and not all(_strictly_increasing(f, self._bin_dim) for f in fields[:2 if how['stacked'] else 1]):
      return None  # (the host route raises or not by the chunk's own selection)
    try:
      ctx = _hip.default_context()
    except _hip.WbxUnavailableError:  # no device or no library: nothing to launch on (the host route says so where it needs one)
      return None
    if not engine.ens_rps_field_available(ctx):
      return None
    # A host-resident field behind a slab pool (a memory map, a very large array, climatology_cache.cached()) is gathered slab by
    # slab like any climatology -- where there are slabs to select and one field serves both sides.  Without a time dim the pool has
    # nothing to select along, and stacking two such fields would read them whole: both keep the host route.
    from weatherbenchx_amd import climatology_cache  # pylint: disable=g-import-not-at-top
    pooled = any(climatology_cache.cache_for(f) is not None for f in fields[:2 if how['stacked'] else 1])
    if pooled and (how['stacked'] or not how['positions']):
      return None
    source = _stacked_fields(self.__dict__.setdefault('_field_stacks', {}), *fields) if how['stacked'] else fields[0]
    try:
      ref = base._aligned_ref(source, how['over_dims'], how['positions'])  # pylint: disable=protected-access
      return lazy.ens_rps_field_statistic(p, t, self._ensemble_dim, ref, bin_dim=self._bin_dim, stacked=how['stacked'], fair=self._fair,
                                          right_inclusive=self._right_inclusive, host=self.host_per_variable,
                                          clim_key=(id(source), source.__dict__.get('_mutations', 0)))
    except (ValueError, lazy._NeedsAlignment):  # pylint: disable=protected-access  (a frame the field does not broadcast against, a
      return None  # slab pool built for another selection)


def rps_field_route(predictions, targets, p_field, t_field, *, ensemble_dim: str, bin_dim: str, skipna_ensemble: bool, fair: bool):
  """Where EnsembleRankedProbabilityScore at the threshold fields `p_field` / `t_field` (the variable's DataArrays) goes, decided
  from labels, dims and dtypes alone (no device, no look at the values): ('fused', {'over_dims', 'positions', 'stacked'}) -- one
  launch of wbx_ens_rps_field_partial, the fields gathered in place through `positions` (wrappers.bin_threshold_positions), `stacked`:
  two different fields that are stacked along a new leading axis -- or ('host', the reason)."""
  host = lambda why: ('host', why)
  if skipna_ensemble:
    return host('skipna_ensemble')
  if not isinstance(p_field, xr.DataArray) or not isinstance(t_field, xr.DataArray):
    return host('a side whose thresholds are not a field')
  p, t = xr.as_dataarray(predictions), xr.as_dataarray(targets)
  e = ensemble_dim
  if e not in p.dims or e in t.dims:
    return host('the member dim must be a dim of the predictions and not of the targets')
  if bin_dim in p.dims or bin_dim in t.dims or not set(t.dims) <= set(p.dims):
    return host('the frames of predictions and targets')
  floats = ('float32', 'float64')
  if any(str(a.dtype).replace('torch.', '') not in floats for a in (p, t, p_field, t_field)):
    return host('dtypes other than float32 / float64')
  m = p.sizes[e]
  if m > _hip.ERPS_MAX_MEMBERS or (fair and m < 2):
    return host(f'{m} members')
  for f in (p_field, t_field):
    if bin_dim not in f.dims or e in f.dims:
      return host(f'a threshold field with dims {f.dims}')
  k = p_field.sizes[bin_dim]
  if not 1 <= k <= _hip.ERPS_MAX_THRESHOLDS or t_field.sizes[bin_dim] != k:
    return host(f'{k} against {t_field.sizes[bin_dim]} thresholds')
  labelled = [bin_dim in f.coords for f in (p_field, t_field)]
  if labelled[0] != labelled[1] or (labelled[0] and not np.array_equal(np.asarray(p_field.coords[bin_dim].values),
                                                                          np.asarray(t_field.coords[bin_dim].values))):
    return host('bin labels that differ between the sides')  # (the host route joins them on the labels they share)
  try:
    over_p, pos_p = wrappers.bin_threshold_positions(p_field, p)
    over_t, pos_t = wrappers.bin_threshold_positions(t_field, t)
  except (KeyError, ValueError) as err:
    return host(f'a selection that raises ({err})')  # (labels that are not found: the host route raises)
  if over_p != over_t or set(pos_p) != set(pos_t) or any(not np.array_equal(pos_p[d], pos_t[d]) for d in pos_p):
    return host('the two sides select different thresholds')
  if p_field is t_field:
    return 'fused', {'over_dims': over_p, 'positions': pos_p, 'stacked': False}
  if p_field.dims != t_field.dims or p_field.shape != t_field.shape or str(p_field.dtype) != str(t_field.dtype):
    return host('threshold fields that differ in dims, shape or dtype')
  if set(p_field.coords) != set(t_field.coords) or any(
      tuple(p_field.coords[c].dims) != tuple(t_field.coords[c].dims)
      or not xr._values_equal(p_field._coords[c][1], t_field._coords[c][1]) for c in p_field.coords):  # pylint: disable=protected-access
    return host('threshold fields that differ in coordinates')
  # (one array behind two labelled objects -- the same variable of two Datasets -- is still one field)
  return 'fused', {'over_dims': over_p, 'positions': pos_p, 'stacked': p_field.data is not t_field.data}


def _strictly_increasing(field: xr.DataArray, bin_dim: str) -> bool:
  """The whole field is free of NaN and strictly increasing along `bin_dim` (then every selection of it is), looked at once per
  field object and state."""
  memo = field.__dict__.setdefault('_wbx_rps_monotone', {})
  key = (bin_dim, field.__dict__.get('_mutations', 0))
  if key not in memo:
    memo.clear()
    values = np.moveaxis(np.asarray(field.values), field.dims.index(bin_dim), 0)
    memo[key] = bool(not np.isnan(values).any() and (values.shape[0] < 2 or np.all(values[1:] > values[:-1])))
  return memo[key]


def _stacked_fields(cache: dict, p_field: xr.DataArray, t_field: xr.DataArray) -> xr.DataArray:
  """[prediction thresholds, target thresholds] along a new leading axis (on the device for device payloads), built once per pair
  of field objects and their states (`cache`: the statistic's, like SEEPS's device tables)."""
  key = (id(p_field), id(t_field))
  state = (p_field.__dict__.get('_mutations', 0), t_field.__dict__.get('_mutations', 0))
  hit = cache.get(key)
  if hit is None or hit[0] is not p_field or hit[1] is not t_field or hit[2] != state:
    a, b = p_field.data, t_field.data
    if xr._is_torch(a) or xr._is_torch(b):  # pylint: disable=protected-access
      import torch  # pylint: disable=g-import-not-at-top
      a = a if xr._is_torch(a) else torch.as_tensor(np.asarray(a), device=b.device)  # pylint: disable=protected-access
      b = b if xr._is_torch(b) else torch.as_tensor(np.asarray(b), device=a.device)  # pylint: disable=protected-access
      data = torch.stack([a, b.to(a.device)])
    else:
      data = np.stack([np.asarray(a), np.asarray(b)])
    both = xr.DataArray(data, dims=(lazy.ERPSF_SIDE_DIM,) + tuple(p_field.dims), coords=dict(p_field._coords), _raw_coords=True,  # pylint: disable=protected-access
                        name=p_field.name)
    if len(cache) > 16:
      cache.clear()
    hit = cache[key] = (p_field, t_field, state, both)
  return hit[3]


def _fused_energy(lane: int, predictions, targets, dim, ensemble_dim: str, fair):
  """The skill (lane 0) or spread (lane 1) of the energy score as a lazy statistic that the Aggregator reduces with
  wbx_ens_energy_partial (lazy.energy_statistic), or None where the host route has to do it: the switch is off, no device, other
  dtypes than float32 / float64, no member dim in the predictions or one in the targets, a norm dim that one input lacks, norm dims
  that are not one strided run of an input as a launch sees it or that the two inputs store in different orders (element i of one
  run would not be element i of the other), targets with a dim of their own, nothing left of the frame, a `mask` coordinate along a
  norm or member dim, or an ensemble size the kernel does not take."""
  if not lazy.FUSED_ENERGY:
    return None
  p, t = xr.as_dataarray(predictions), xr.as_dataarray(targets)
  e, norm = ensemble_dim, _dims_tuple(dim)
  if e not in p.dims or e in t.dims or e in norm or not norm or len(set(norm)) != len(norm):
    return None
  if any(d not in p.dims or d not in t.dims or p.sizes[d] != t.sizes[d] for d in norm):
    return None
  if str(p.dtype) not in ('float32', 'float64') or str(t.dtype) not in ('float32', 'float64'):
    return None
  if not set(t.dims) <= set(p.dims) or not set(p.dims) - {e} - set(norm):
    return None
  if not 2 <= p.sizes[e] <= _hip.ENRG_MAX_MEMBERS:
    return None
  for da in (p, t):
    if 'mask' in da.coords and set(da.coords['mask'].dims) & ({e} | set(norm)):
      return None
    if engine.norm_run(lazy.payload_layout(da), norm, da.sizes) is None:
      return None
  if len({engine.norm_run_order(lazy.payload_layout(da), norm, da.sizes) for da in (p, t)}) != 1:
    return None
  try:
    ctx = _hip.default_context()
  except _hip.WbxUnavailableError:  # no device or no library: nothing to launch on
    return None
  if not engine.ens_energy_available(ctx):
    return None
  try:
    return lazy.energy_statistic(lane, p, t, e, norm, fair)
  except lazy._NeedsAlignment:  # pylint: disable=protected-access  (labels that differ: the host route joins them)
    return None


class EnergyScoreSkill(base.PerVariableStatistic):
  """mean_m ||X_m - Y|| with the norm over `dim` (probabilistic.py:480-503)."""

  def __init__(self, dim, ensemble_dim: str = 'sample'):
    self._dim = dim
    self._ensemble_dim = ensemble_dim

  @property
  def unique_name(self):
    return f'EnergyScore_Skill_dim={self._dim}_ensemble_dim={self._ensemble_dim}'

  def _compute_per_variable(self, predictions, targets):
    fused = _fused_energy(lazy.ENERGY_LANE['EnergyScoreSkill'], predictions, targets, self._dim, self._ensemble_dim, None)
    return fused if fused is not None else self.host_per_variable(predictions, targets)

  def host_per_variable(self, predictions, targets):
    """The score as labelled-array arithmetic on whatever holds the payload."""
    return _norm_over(predictions - targets, _dims_tuple(self._dim)).mean(self._ensemble_dim, skipna=False)


class EnergyScoreSpread(base.PerVariableStatistic):
  """sum_{m, m'} ||X_m - X_m'|| / (M (M - 1))  (M**2 when not fair), the norm over `dim` (probabilistic.py:506-551).

  The M x M table of the reference is never formed: one pass per offset k = 1 .. M - 1 pairs every member with the one k
  places on (cyclically), which visits each ordered pair (m, m' != m) once; the diagonal contributes nothing."""

  def __init__(self, dim, ensemble_dim: str = 'sample', fair: bool = True):
    self._dim = dim
    self._ensemble_dim = ensemble_dim
    self._fair = fair

  @property
  def unique_name(self):
    return f'EnergyScore_Spread_dim={self._dim}_ensemble_dim={self._ensemble_dim}_fair={self._fair}'

  def _compute_per_variable(self, predictions, targets):
    fused = _fused_energy(lazy.ENERGY_LANE['EnergyScoreSpread'], predictions, targets, self._dim, self._ensemble_dim, self._fair)
    return fused if fused is not None else self.host_per_variable(predictions, targets)

  def host_per_variable(self, predictions, targets):
    """The score as labelled-array arithmetic on whatever holds the payload: one pass per cyclic member offset."""
    del targets
    e = self._ensemble_dim
    m = predictions.sizes[e]
    plain = predictions.drop_vars([e]) if e in predictions.coords else predictions
    total = None
    for k in range(1, m):
      rolled = plain.isel({e: np.roll(np.arange(m), -k)})
      part = _norm_over(plain - rolled, _dims_tuple(self._dim)).sum(e, skipna=False)
      total = part if total is None else total + part
    if total is None:  # one member: no pairs; 0 / 0 for the fair estimate, like the reference's empty sum over the divider
      total = _norm_over(plain - plain, _dims_tuple(self._dim)).sum(e, skipna=False)
    with np.errstate(all='ignore'):
      return total / float(m * (m - 1) if self._fair else m * m)


def _fused_variogram(predictions, targets, dim, ensemble_dim: str, power):
  """The variogram score as a lazy statistic that the Aggregator reduces with wbx_ens_variogram_partial (lazy.variogram_statistic),
  or None where the host route has to do it: the conditions of _fused_energy -- the switch is off, no device, other dtypes than
  float32 / float64, no member dim in the predictions or one in the targets, a `dim` that one input lacks or that has two sizes,
  a `dim` that is not one strided run of an input as a launch sees it, targets with a dim of their own, nothing left of the frame,
  a `mask` coordinate along `dim` or the member dim, labels that differ -- and a power other than 0.5, 1 or 2, more than
  _hip.VGRAM_MAX_RUN elements along `dim` or more than _hip.VGRAM_MAX_MEMBERS members."""
  if not lazy.FUSED_VARIOGRAM:
    return None
  try:
    if not isinstance(dim, str) or float(power) not in _hip.VGRAM_POWERS:
      return None
  except (TypeError, ValueError):
    return None
  p, t = xr.as_dataarray(predictions), xr.as_dataarray(targets)
  e = ensemble_dim
  if e not in p.dims or e in t.dims or e == dim:
    return None
  if dim not in p.dims or dim not in t.dims or p.sizes[dim] != t.sizes[dim]:
    return None
  if str(p.dtype) not in ('float32', 'float64') or str(t.dtype) not in ('float32', 'float64'):
    return None
  if not set(t.dims) <= set(p.dims) or not set(p.dims) - {e, dim}:
    return None
  if not 1 <= p.sizes[e] <= _hip.VGRAM_MAX_MEMBERS or not 1 <= p.sizes[dim] <= _hip.VGRAM_MAX_RUN:
    return None
  for da in (p, t):
    if 'mask' in da.coords and set(da.coords['mask'].dims) & {e, dim}:
      return None
    if engine.norm_run(lazy.payload_layout(da), (dim,), da.sizes) is None:
      return None
  try:
    ctx = _hip.default_context()
  except _hip.WbxUnavailableError:  # no device or no library: nothing to launch on
    return None
  if not engine.ens_variogram_available(ctx):
    return None
  try:
    return lazy.variogram_statistic(p, t, e, dim, power)
  except lazy._NeedsAlignment:  # pylint: disable=protected-access  (labels that differ: the host route joins them)
    return None


class VariogramScore(base.PerVariableStatistic):
  """sum_{i, j} (|y_i - y_j|**p - mean_m |x_i^m - x_j^m|**p)**2 over all pairs along `dim` (Scheuerer & Hamill 2015;
  probabilistic.py:554-603).  Same pairing by cyclic offsets as EnergyScoreSpread: [N, N] tables are never formed."""

  def __init__(self, dim: str, ensemble_dim: str, p: float = 0.5):
    self._dim = dim
    self._ensemble_dim = ensemble_dim
    self._p = p

  @property
  def unique_name(self):
    return f'VariogramScore_dim={self._dim}_ensemble_dim={self._ensemble_dim}'

  def _compute_per_variable(self, predictions, targets):
    fused = _fused_variogram(predictions, targets, self._dim, self._ensemble_dim, self._p)
    return fused if fused is not None else self.host_per_variable(predictions, targets)

  def host_per_variable(self, predictions, targets):
    """The score as labelled-array arithmetic on whatever holds the payload: one pass per cyclic offset along `dim`."""
    d, n = self._dim, predictions.sizes[self._dim]
    strip = lambda a: a.drop_vars([d]) if d in a.coords else a
    x, y = strip(predictions), strip(targets)
    total = None
    for k in range(n):  # (k = 0 is the diagonal: zero unless NaN, which it must hand on)
      order = np.roll(np.arange(n), -k)
      ty = abs(y - y.isel({d: order})) ** self._p
      tx = (abs(x - x.isel({d: order})) ** self._p).mean(self._ensemble_dim, skipna=False)
      part = ((ty - tx) ** 2).sum(d, skipna=False)
      total = part if total is None else total + part
    return total


def _fused_wasserstein(predictions, targets, ensemble_dim: str):
  """The Wasserstein distance as a lazy statistic that the Aggregator reduces with wbx_ens_wasserstein_partial
  (lazy.wasserstein_statistic), or None where the host route has to do it: the switch is off, no device or library, or no such
  symbol in it, a dtype other than float32 / float64 or two different dtypes, an ensemble of fewer than 1 or more than
  _hip.WASS_MAX_MEMBERS members on either side, a `mask` coordinate along the member dim, nothing left of the frame without the
  member dim, and frames or labels the launch cannot take as they stand where the host route broadcasts: a dim that one input
  lacks, sizes or labels that differ, a coordinate the two inputs disagree about.  No shape class is kept from the kernel for
  speed: it won at every shape that was measured."""
  if not lazy.FUSED_WASSERSTEIN:
    return None
  p, t = xr.as_dataarray(predictions), xr.as_dataarray(targets)
  e = ensemble_dim
  if str(p.dtype) not in ('float32', 'float64') or str(t.dtype) != str(p.dtype):
    return None
  if not 1 <= p.sizes[e] <= _hip.WASS_MAX_MEMBERS or not 1 <= t.sizes[e] <= _hip.WASS_MAX_MEMBERS:
    return None
  frame = tuple(d for d in p.dims if d != e)
  if not frame or set(frame) != set(t.dims) - {e}:
    return None
  for da in (p, t):
    if 'mask' in da.coords and e in da.coords['mask'].dims:
      return None
  try:
    ctx = _hip.default_context()
  except _hip.WbxUnavailableError:  # no device or no library: nothing to launch on
    return None
  if not engine.ens_wasserstein_available(ctx):
    return None
  try:
    stat = lazy.wasserstein_statistic(p, t, e)
  except (lazy._NeedsAlignment, ValueError):  # pylint: disable=protected-access  (the host route broadcasts, or says what is wrong)
    return None
  # the host route hands on every coordinate of either input that lies in the frame, the predictions' first; a group drops what
  # the two disagree about
  want = {k for da in (p, t) for k, (cd, _) in da._coords.items() if k != e and set(cd) <= set(frame)}  # pylint: disable=protected-access
  if stat.dims != frame or set(stat._coords) != want:  # pylint: disable=protected-access
    return None
  return stat


class WassersteinDistance(base.PerVariableStatistic):
  """1-Wasserstein (earth mover's) distance between the prediction ensemble and the target ensemble at every point; the two
  ensembles may differ in size (probabilistic.py:785-833, there through scipy.stats.wasserstein_distance point by point).

  Here for all points at once: W1 = integral |F_p - F_t|.  The pooled members are sorted, the two empirical CDFs are running
  counts of where each sorted value came from, and the integral is the sum over the gaps between consecutive pooled values."""

  def __init__(self, ensemble_dim: str = ENSEMBLE_DIM):
    self._ensemble_dim = ensemble_dim

  @property
  def unique_name(self) -> str:
    return f'WassersteinDistance_{self._ensemble_dim}'

  def _compute_per_variable(self, predictions, targets):
    e = self._ensemble_dim
    if e not in predictions.dims:
      raise ValueError(f'Ensemble dimension {e!r} not found in predictions: {predictions}')
    if e not in targets.dims:
      raise ValueError(f'Ensemble dimension {e!r} not found in targets: {targets}')
    fused = _fused_wasserstein(predictions, targets, e)
    return fused if fused is not None else self.host_per_variable(predictions, targets)

  def host_per_variable(self, predictions, targets):
    """The distance as array arithmetic on whatever holds the payload: a stable float64 sort of the pooled members, two
    cumulative sums and the gaps between them."""
    e = self._ensemble_dim
    strip = lambda a: a.drop_vars([e]) if e in a.coords else a
    p, t = xr.broadcast(strip(predictions).rename({e: '_p'}), strip(targets).rename({e: '_t'}))
    frame = tuple(d for d in p.dims if d not in ('_p', '_t'))
    p = p.isel(_t=0).transpose(*frame, '_p')
    t = t.isel(_p=0).transpose(*frame, '_t')
    m, n = p.sizes['_p'], t.sizes['_t']
    pd, td = p.data, t.data
    if xr._is_torch(pd) or xr._is_torch(td):  # pylint: disable=protected-access
      import torch  # pylint: disable=g-import-not-at-top
      dev = pd.device if xr._is_torch(pd) else td.device  # pylint: disable=protected-access
      pd, td = (torch.as_tensor(a, device=dev).to(torch.float64) for a in (pd, td))
      pooled, order = torch.sort(torch.cat([pd, td], dim=-1), dim=-1, stable=True)
      from_p = (order < m).to(torch.float64)
      gap = torch.abs(torch.cumsum(from_p, -1) / m - torch.cumsum(1.0 - from_p, -1) / n)[..., :-1]
      dist = (gap * (pooled[..., 1:] - pooled[..., :-1])).sum(-1)
    else:
      both = np.concatenate([np.asarray(pd, dtype=np.float64), np.asarray(td, dtype=np.float64)], axis=-1)
      order = np.argsort(both, axis=-1, kind='stable')
      pooled = np.take_along_axis(both, order, axis=-1)
      from_p = (order < m).astype(np.float64)
      gap = np.abs(np.cumsum(from_p, -1) / m - np.cumsum(1.0 - from_p, -1) / n)[..., :-1]
      dist = (gap * np.diff(pooled, axis=-1)).sum(-1)
    coords = {k: v for k, v in p._coords.items() if set(v[0]) <= set(frame)}  # pylint: disable=protected-access
    return xr.DataArray._assemble(dist, frame, coords, name=predictions.name)  # pylint: disable=protected-access


class EnergyScore(base.PerVariableMetric):
  """E||X - Y|| - 0.5 E||X - X'|| with the norm over `dim` (Gneiting & Raftery; probabilistic.py:1346-1406)."""

  def __init__(self, dim, ensemble_dim: str = ENSEMBLE_DIM, fair: bool = True):
    self._dim = dim
    self._ensemble_dim = ensemble_dim
    self._fair = fair

  @property
  def statistics(self) -> Mapping[str, base.Statistic]:
    return {'EnergyScoreSkill': EnergyScoreSkill(dim=self._dim, ensemble_dim=self._ensemble_dim),
            'EnergyScoreSpread': EnergyScoreSpread(dim=self._dim, ensemble_dim=self._ensemble_dim, fair=self._fair)}

  def _values_from_mean_statistics_per_variable(self, statistic_values):
    return statistic_values['EnergyScoreSkill'] - 0.5 * statistic_values['EnergyScoreSpread']


def _tile(window_size: int, window_dim: str, wrap_longitude: bool):
  return wrappers.Tile(which='both', window_size=window_size, window_dim=window_dim, wrap_longitude=wrap_longitude)


class TiledEnergyScore(base.PerVariableMetric):
  """EnergyScore of every window_size x window_size patch of the grid (rows without a full window at the top and bottom are
  dropped, longitude optionally wraps): probabilistic.py:1409-1467."""

  _WINDOW_DIM = 'window'

  def __init__(self, window_size: int = 3, ensemble_dim: str = ENSEMBLE_DIM, fair: bool = True, wrap_longitude: bool = True):
    self._window_size = window_size
    self._ensemble_dim = ensemble_dim
    self._fair = fair
    self._wrap_longitude = wrap_longitude

  @property
  def statistics(self) -> Mapping[str, base.Statistic]:
    tile = _tile(self._window_size, self._WINDOW_DIM, self._wrap_longitude)
    return {
        'TiledEnergyScore_Skill': wrappers.WrappedStatistic(
            EnergyScoreSkill(dim=self._WINDOW_DIM, ensemble_dim=self._ensemble_dim), tile),
        'TiledEnergyScore_Spread': wrappers.WrappedStatistic(
            EnergyScoreSpread(dim=self._WINDOW_DIM, ensemble_dim=self._ensemble_dim, fair=self._fair), tile),
    }

  def _values_from_mean_statistics_per_variable(self, statistic_values):
    return statistic_values['TiledEnergyScore_Skill'] - 0.5 * statistic_values['TiledEnergyScore_Spread']


class TiledVariogramScore(base.PerVariableMetric):
  """VariogramScore of every window_size x window_size patch: the pairs stay among correlated neighbours
  (probabilistic.py:1470-1527)."""

  _WINDOW_DIM = 'window'

  def __init__(self, window_size: int = 3, ensemble_dim: str = ENSEMBLE_DIM, p: float = 0.5, wrap_longitude: bool = True):
    self._window_size = window_size
    self._ensemble_dim = ensemble_dim
    self._p = p
    self._wrap_longitude = wrap_longitude

  @property
  def statistics(self) -> Mapping[str, base.Statistic]:
    tile = _tile(self._window_size, self._WINDOW_DIM, self._wrap_longitude)
    return {'TiledVariogramScore': wrappers.WrappedStatistic(
        VariogramScore(dim=self._WINDOW_DIM, ensemble_dim=self._ensemble_dim, p=self._p), tile)}

  def _values_from_mean_statistics_per_variable(self, statistic_values):
    return statistic_values['TiledVariogramScore']


# ---- relative economic value (probabilistic.py:1006-1303) ---------------------------------------------------------------------------
def _select_optimal_thresholds(values: xr.DataArray, optimal_thresholds: xr.DataArray, method: str | None = None) -> xr.DataArray:
  """`values` at, for every cost/loss ratio (and every other dim the two share, e.g. lead_time), the probability threshold chosen
  for it: `values.sel(threshold=optimal_thresholds, method=method)` without the `threshold` coordinate
  (probabilistic.py:1006-1059).  method None = exact labels (KeyError otherwise), 'nearest' = the closest available one."""
  values, optimal_thresholds = xr.as_dataarray(values), xr.as_dataarray(optimal_thresholds)
  available = np.asarray(values.coords['threshold'].values, dtype=np.float64)
  wanted = np.asarray(optimal_thresholds.values, dtype=np.float64)
  position = np.abs(wanted[..., None] - available).argmin(axis=-1)
  if method is None:
    missing = available[position] != wanted
    if missing.any():
      raise KeyError(f'thresholds {np.unique(wanted[missing])[:5]} not among the available {available}')
  elif method != 'nearest':
    raise ValueError(f'unsupported selection method {method!r}')
  index = xr.DataArray(position, dims=optimal_thresholds.dims,
                       coords={d: optimal_thresholds.coords[d] for d in optimal_thresholds.dims if d in optimal_thresholds.coords})
  plain = values.drop_vars(['threshold'])
  table, index = xr.broadcast(plain, index)              # both [..., threshold, ..., cost_loss_ratio] in one dim order
  axis = table.dims.index('threshold')
  picked = np.take_along_axis(np.asarray(table.values), np.take(np.asarray(index.values), [0], axis=axis), axis=axis)
  out_dims = tuple(d for d in table.dims if d != 'threshold')
  coords = {k: v for k, v in table._coords.items() if 'threshold' not in v[0]}  # pylint: disable=protected-access
  return xr.DataArray._assemble(np.squeeze(picked, axis=axis), out_dims, coords, name=values.name)  # pylint: disable=protected-access


class RelativeEconomicValue(base.Metric):
  """Relative economic value of probability forecasts of a binary event for users with cost/loss ratio C/L who act when the
  forecast probability exceeds a threshold: (E_climate - E_forecast) / (E_climate - E_perfect) with expenses per unit loss
  E_forecast = C/L (TP + FP) + FN,  E_perfect = C/L (TP + FN),  E_climate = min(C/L, TP + FN).

  Predictions are probabilities in [0, 1], targets binary.  The contingency table is accumulated for every probability
  threshold -- by default the N thresholds between the N + 1 possible values of an N-member ensemble, (k + 0.5) / N -- plus the
  two constant decisions (threshold 0: always act; 1: never).  Without `optimal_thresholds` the result has dims
  (threshold, cost_loss_ratio); with them, one threshold is picked per cost/loss ratio (and per any other shared dim) and
  `threshold` is gone.  Default cost/loss ratios: 50 values from 0.005 towards 1 on a log scale.  probabilistic.py:1062-1303."""

  def __init__(self, *, ensemble_size: int | None = None, probability_thresholds: np.ndarray | None = None,
               cost_loss_ratios: np.ndarray | None = None, optimal_thresholds=None,
               optimal_thresholds_select_nearest: bool = False, statistic_suffix: str | None = None):
    if ensemble_size is None and probability_thresholds is None:
      raise ValueError('Either ensemble_size or probability_thresholds must be specified.')
    if probability_thresholds is not None and ensemble_size is not None:
      raise ValueError('Only one of ensemble_size or probability_thresholds must be specified.')
    if probability_thresholds is not None and statistic_suffix is None:
      raise ValueError('If probability_thresholds is specified, statistic_suffix must be specified.')
    ratios = np.geomspace(0.005, 1, 51)[:-1] if cost_loss_ratios is None else np.asarray(cost_loss_ratios)
    self._cost_loss_ratio = xr.DataArray(ratios, dims=['cost_loss_ratio'], coords={'cost_loss_ratio': ratios})
    if probability_thresholds is None:
      self._thresholds = (np.arange(ensemble_size) + 0.5) / ensemble_size
      if statistic_suffix is None:
        statistic_suffix = 'all_thresholds_for_ensemble_size'
    else:
      self._thresholds = np.asarray(probability_thresholds)
    if not (np.all(self._thresholds >= 0.0) and np.all(self._thresholds <= 1.0)):
      raise ValueError(f'Probability thresholds must be in [0, 1], got {self._thresholds=}.')
    self._unique_name_suffix = statistic_suffix or ''
    if optimal_thresholds is not None:
      for var in (optimal_thresholds.values() if isinstance(optimal_thresholds, Mapping) else [optimal_thresholds]):
        var = xr.as_dataarray(var)
        if 'cost_loss_ratio' not in var.dims:
          raise ValueError('optimal_thresholds must have "cost_loss_ratio" dimensions.')
        if ('cost_loss_ratio' not in var.coords
            or not np.array_equal(np.asarray(var.coords['cost_loss_ratio'].values), ratios)):
          raise ValueError('optimal_thresholds must have cost_loss_ratio coordinates with the same values as the '
                           'cost_loss_ratios argument.')
    self._optimal_thresholds = optimal_thresholds
    self._optimal_thresholds_select_nearest = optimal_thresholds_select_nearest

  @property
  def statistics(self) -> Mapping[str, base.Statistic]:
    binarize = wrappers.ContinuousToBinary(which='predictions', threshold_value=self._thresholds, threshold_dim='threshold',
                                           unique_name_suffix=self._unique_name_suffix)
    return {name: wrappers.WrappedStatistic(getattr(categorical, name)(), binarize)
            for name in ('TruePositives', 'TrueNegatives', 'FalsePositives', 'FalseNegatives')}

  def _with_constant_decisions(self, tp, fp, fn):
    """Threshold 0 (always act: TP = base rate, FP = 1 - base rate, FN = 0) in front, threshold 1 (never act: FN = base rate) behind."""
    base_rate = tp.isel(threshold=0, drop=True) + fn.isel(threshold=0, drop=True)
    zero = base_rate * 0.0
    at = lambda x, threshold: x.expand_dims(threshold=[threshold])
    return (xr.concat([at(base_rate, 0.0), tp, at(zero, 1.0)], dim='threshold'),
            xr.concat([at(1.0 - base_rate, 0.0), fp, at(zero, 1.0)], dim='threshold'),
            xr.concat([at(zero, 0.0), fn, at(base_rate, 1.0)], dim='threshold'))

  def values_from_mean_statistics(self, statistic_values):
    names = list(self.statistics)
    common = set.intersection(*[set(statistic_values[s]) for s in names])
    return {var: self._values_from_mean_statistics_per_variable({s: statistic_values[s][var] for s in names}, var)
            for var in statistic_values[names[0]] if var in common}

  def _values_from_mean_statistics_per_variable(self, statistic_values, var_name):
    def ordered(da):  # the statistics carry `threshold` wherever the transform put it; the table below wants it first
      da = xr.as_dataarray(da)
      return da.transpose('threshold', *[d for d in da.dims if d != 'threshold'])
    tp, fp, fn = self._with_constant_decisions(*(ordered(statistic_values[s])
                                                 for s in ('TruePositives', 'FalsePositives', 'FalseNegatives')))
    if self._optimal_thresholds is not None:
      chosen = self._optimal_thresholds[var_name] if isinstance(self._optimal_thresholds, Mapping) else self._optimal_thresholds
      method = 'nearest' if self._optimal_thresholds_select_nearest else None
      tp, fp, fn = (_select_optimal_thresholds(x, chosen, method) for x in (tp, fp, fn))
    ratio = self._cost_loss_ratio
    forecast = ratio * (tp + fp) + fn
    perfect = ratio * (tp + fn)
    climate = np.minimum(ratio, tp + fn)
    return (climate - forecast) / (climate - perfect)
