"""The two tables that spell a fused statistic kind -- engine._KINDS (the launch) and lazy._LAZY_KINDS (what FusedGroup does) -- and
the gates next to them, without a device and without the library."""
import pickle

import numpy as np
import pytest

import energy_cases as GC
import ens_rps_cases as EC
import fake_device
import fss_cases as FC
import seeps_cases as SC
from weatherbenchx_amd import _hip
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import categorical
from weatherbenchx_amd.metrics import deterministic
from weatherbenchx_amd.metrics import probabilistic
from weatherbenchx_amd.metrics import spatial
from weatherbenchx_amd.metrics import wrappers

# gate -> the entry points it asks the library for
GATES = {
    'contingency_available': 'wbx_contingency_partial', 'ens_rps_available': 'wbx_ens_rps_partial',
    'ens_rps_field_available': 'wbx_ens_rps_field_partial', 'ens_energy_available': 'wbx_ens_energy_partial',
    'ens_variogram_available': 'wbx_ens_variogram_partial', 'ens_wasserstein_available': 'wbx_ens_wasserstein_partial',
    'ens_interval_available': 'wbx_ens_interval_partial', 'ens_prob_available': 'wbx_ens_prob_contingency_partial',
    'brier_available': 'wbx_ens_brier_partial', 'seeps_available': 'wbx_seeps_partial',
    'fss_thresholds_available': 'wbx_fss_threshold_partial', 'fss_available': 'wbx_fss_partial',
}
SWITCHES = ('FUSED_CONTINGENCY', 'FUSED_ENS_RPS', 'FUSED_ENS_RPS_FIELD', 'FUSED_ENERGY', 'FUSED_VARIOGRAM', 'FUSED_WASSERSTEIN',
            'FUSED_INTERVALS', 'FUSED_ENS_PROB', 'FUSED_SEEPS', 'FUSED_FSS', 'FUSED_FSS_THRESHOLDS', 'FUSED_BRIER')


def test_the_two_tables_have_the_same_keys():
  assert set(engine._KINDS) == set(lazy._LAZY_KINDS) and len(engine._KINDS) == 15  # pylint: disable=protected-access


class _Any:
  """The `cat` tuple of any kind: every field is an integer that also is a device buffer."""
  field = type('Field', (int,), {'ptr': 0})(1)

  def __init__(self, **none):
    self.__dict__.update(none)

  def __getattr__(self, name):
    return self.field


def test_every_entry_point_a_row_names_is_declared():
  """Both arms of 'cat' (thresholds in a table / in a field) and of 'fss' (binary / thresholded continuous fields) too."""
  named = {}
  for kind, row in engine._KINDS.items():  # pylint: disable=protected-access
    arms = [_Any()] + {'cat': [_Any(cstride=None)], 'fss': [_Any(thr=None)]}.get(kind, [])
    named[kind] = {row.call(['p', 't', 'c', 'm'], 'out', _hip.F32, _hip.DET3, (_Any.field,) * 3, cat)[0] for cat in arms}
    assert len(named[kind]) == len(arms), kind
  assert named['cat'] == {'wbx_cat_partial', 'wbx_cat_exceed_field'} and named['fss'] == {'wbx_fss_partial', 'wbx_fss_threshold_partial'}
  for kind, names in named.items():
    for name in names:
      assert name in _hip.EXPORTED_SYMBOLS and name in _hip.FN_IDS, (kind, name)
  assert set(GATES.values()) <= set().union(*named.values())  # (every gate guards an entry point of the table)


class _Ctx(_hip.Context):  # a context a gate may ask: nothing is launched on it
  def __init__(self, *symbols):  # pylint: disable=super-init-not-called
    self.lib = type('Lib', (), {s: staticmethod(lambda *a: 0) for s in symbols})()

  def __del__(self):
    pass


class _NoLib(_Ctx):
  lib = property(lambda self: (_ for _ in ()).throw(AttributeError('lib')), lambda self, value: None)


@pytest.mark.parametrize('gate', list(GATES))
def test_a_gate_opens_for_a_library_context_that_exports_its_entry_only(gate):
  available = getattr(engine, gate)
  assert available(_Ctx(GATES[gate])) is True
  assert available(object()) is False and available(fake_device.FakeCtx()) is False
  assert available(_Ctx()) is False and available(_Ctx(*(s for s in GATES.values() if s != GATES[gate]))) is False
  assert available(_NoLib()) is False


# ---- a statistic of every kind, built by the public classes on the smallest frames of the cases modules ---------------------------
M, THR = 4, [0.25, 0.5]
DIMS = ('time', 'latitude', 'longitude')


def _labelled(a, dims, **extra):
  cs = {'time': np.arange(a.shape[dims.index('time')]), 'latitude': np.linspace(-40, 40, a.shape[dims.index('latitude')]),
        'longitude': np.arange(a.shape[dims.index('longitude')]) * (360.0 / a.shape[dims.index('longitude')])}
  for d in dims:
    if d not in cs:
      cs[d] = np.arange(a.shape[dims.index(d)])
  return {'v': xr.DataArray(a, dims=dims, coords=dict(cs, **extra), name='v')}


def _ensemble_pair():
  p, t, _ = EC.ens_rps_case(1, M, 2, 3, 5, np.float32, 0, 3, False, THR)
  return _labelled(p, ('number',) + DIMS), _labelled(t, DIMS)


def _member(pred, k=0):
  return {'v': pred['v'].isel(number=k, drop=True)}


def _norm_pair():
  p, t, _ = GC.energy_case(2, M, 3, 2, 3, 5, np.float32, 0, 3, False)
  return _labelled(p, ('number',) + DIMS + ('level',)), _labelled(t, DIMS + ('level',))


def _binary(*chain):
  return [wrappers.ContinuousToBinary('both', THR, 'threshold')] + list(chain)


def _build_det():
  pred, targ = _ensemble_pair()
  return deterministic.RMSE(), _member(pred), targ


def _build_ens():
  return (probabilistic.CRPSEnsemble(use_sort=True),) + _ensemble_pair()


def _build_ens2():
  pred, _ = _ensemble_pair()
  return probabilistic.CRPSSkill(skipna_ensemble=True), pred, {'v': pred['v'].isel(number=slice(1, None))}


def _build_cat():
  return (probabilistic.EnsembleErrorExceedance(THR),) + _ensemble_pair()


def _build_cont():
  pred, targ = _ensemble_pair()
  return wrappers.WrappedMetric(categorical.CSI(), _binary()), _member(pred), targ


def _build_erps():
  return (probabilistic.EnsembleRankedProbabilityScore(THR, THR, 'bin', 's'),) + _ensemble_pair()


def _build_erpsf():
  pred, targ = _ensemble_pair()
  place = np.asarray(targ['v'].values)[0]
  place = np.where(np.isfinite(place), place, 0.0).astype(np.float32)
  field = xr.DataArray(np.stack([place, place + 0.25]), dims=('bin', 'latitude', 'longitude'),
                       coords={'bin': np.arange(2), 'latitude': targ['v'].coords['latitude'].values,
                               'longitude': targ['v'].coords['longitude'].values}, name='v')
  return probabilistic.EnsembleRankedProbabilityScore(xr.Dataset({'v': field}), xr.Dataset({'v': field}), 'bin', 's'), pred, targ


def _build_epc():
  return (wrappers.WrappedMetric(categorical.Reliability(), _binary(wrappers.EnsembleMean('predictions', 'number'))),) + _ensemble_pair()


def _build_brier():
  return (wrappers.WrappedMetric(deterministic.MSE(), _binary(wrappers.EnsembleMean('predictions', 'number'))),) + _ensemble_pair()


def _build_enrg():
  return (probabilistic.EnergyScore(dim='level', ensemble_dim='number', fair=True),) + _norm_pair()


def _build_vgrm():
  return (probabilistic.VariogramScore(dim='level', ensemble_dim='number', p=0.5),) + _norm_pair()


def _build_seeps():
  pred, targ, clim, _ = SC.labelled_case(np.float32, 11, shape=(2, 2, 3, 4))
  return categorical.SEEPS([SC.VAR], clim, SC.DRY_MM, SC.MIN_P1, SC.MAX_P1), pred, targ


def _build_fss():
  p, t = FC.indicator_fields((2,) + FC.SHAPES[0], np.float32, 3)
  return spatial.FSS([1, 3], wrap_longitude=True), _labelled(p, DIMS), _labelled(t, DIMS)


BUILDERS = {'det': _build_det, 'ens': _build_ens, 'ens2': _build_ens2, 'cat': _build_cat, 'cont': _build_cont, 'erps': _build_erps,
            'erpsf': _build_erpsf, 'epc': _build_epc, 'brier': _build_brier, 'enrg': _build_enrg, 'vgrm': _build_vgrm,
            'seeps': _build_seeps, 'fss': _build_fss}
# Pickling a lazy statistic materialises it (xarray_lite.LazyPickleMixin), and the per-point values of these kinds are stage 1 of
# their own entry points with every dim kept, which the plan interpreter of the CPU tests does not know: without a device their
# statistics cannot be pickled, before this table or after it.  tests/test_gpu_wasserstein_api.py and tests/test_gpu_intervals_api.py
# read their values on the device.
NEEDS_THE_DEVICE = ('wass', 'ivl')


def test_the_builders_and_the_exceptions_cover_the_table():
  assert set(BUILDERS) | set(NEEDS_THE_DEVICE) == set(lazy._LAZY_KINDS) and not set(BUILDERS) & set(NEEDS_THE_DEVICE)  # pylint: disable=protected-access


@pytest.fixture
def fused(monkeypatch):
  """The plan interpreter with every gate open: what a device context whose library exports every entry point gives."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  for gate in GATES:
    monkeypatch.setattr(engine, gate, lambda ctx: True)
  for switch in SWITCHES:
    monkeypatch.setattr(lazy, switch, True)
  yield
  engine.clear_caches()


@pytest.mark.parametrize('kind', list(BUILDERS))
def test_a_statistic_of_every_kind_pickles_to_its_values(fused, kind):
  what, pred, targ = BUILDERS[kind]()
  with np.errstate(all='ignore'):
    if hasattr(what, 'statistics'):
      stats = metrics_base.compute_unique_statistics_for_all_metrics({'m': what}, pred, targ)
    else:
      stats = {what.unique_name: what.compute(pred, targ)}
    mine = [s for per_var in stats.values() for s in per_var.values() if getattr(getattr(s, '_group', None), 'kind', None) == kind]
    assert mine, (kind, {k: type(v) for per_var in stats.values() for k, v in per_var.items()})
    for stat in mine:
      grp = stat._group  # pylint: disable=protected-access
      assert not [k for k, v in vars(grp).items() if callable(v)], kind  # (rows are looked up by `kind`, not kept)
      assert stat.is_lazy
      back = pickle.loads(pickle.dumps(stat))
      assert not stat.is_lazy and type(back) is xr.DataArray and back.dims == stat.dims and back.name == stat.name  # pylint: disable=unidiomatic-typecheck
      assert back.dtype == np.asarray(stat.values).dtype and set(back.coords) == set(stat.coords)
      np.testing.assert_array_equal(np.asarray(back.values), np.asarray(stat.values))
