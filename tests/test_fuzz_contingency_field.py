"""Randomised checks of the contingency tables at threshold fields (kind 'cont' with a field) through the public API against the restatement of
tests/contingency_field_cases.py: random dim orders of the inputs, targets in another order, a field over a random non-empty subset
of the frame's dims in a random order with its threshold dim anywhere, 1..20 thresholds, the four (data, field) dtype pairs, random
reduce sets, NaNs, masks and skipna.  What is under test is the code between the public statistic and the kernel: the gate of
categorical._Indicator, the group of lazy.py with the field as its `clim`, engine._contf_operands and the plan that puts the frame and the field onto
(key, depth, x).

Expectation: the per-point statistic of the restatement on the payloads transposed to one order, summed over the reduce dims in
NumPy under the same mask and skipna.  Nothing is weighted, so every sum is an integer count: bit for bit, NaN for NaN.  On 'hip'
the statistic is asserted to be a LazyContingencyField with a logged launch; the 'emulated' half takes the host route
(tests/fake_device.py has no context of the library's) and checks this file's own bookkeeping on the CPU, bit for bit as well.

More seeds for a soak run: WBX_FUZZ_SCALE=10 python -m pytest tests/test_fuzz_contingency_field.py [-m gpu]"""
import os

import numpy as np
import pytest

import contingency_field_cases as FC
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import categorical
from weatherbenchx_amd.metrics import wrappers

FUZZ_SCALE = int(os.environ.get('WBX_FUZZ_SCALE', '1'))
N_DEVICE, N_EMULATED = 24 * FUZZ_SCALE, 8 * FUZZ_SCALE
FRAME_DIMS = ['init_time', 'lead_time', 'level', 'latitude', 'longitude']
LAST_DIM = [1, 4, 63, 64, 65, 130, 256]
MODES = ['plain', 'nan_plain', 'masked', 'skipna']
THR = 'quantile'
CELLS = ('TruePositives', 'FalsePositives', 'FalseNegatives', 'TrueNegatives')


def draw_case(seed):
  rng = np.random.default_rng(91000 + seed)
  ndim = int(rng.integers(2, 5))
  dims = [str(d) for d in rng.choice(FRAME_DIMS, size=ndim, replace=False)]
  sizes = {d: int(rng.integers(1, 6)) for d in dims}
  sizes[dims[-1]] = int(rng.choice(LAST_DIM))
  dtype, thr_dtype = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)][seed % 4]
  k = int(rng.choice([1, 2, 3, 5, 16, 17, 20]))
  mode = MODES[int(rng.integers(0, len(MODES)))]
  shape = [sizes[d] for d in dims]
  grid = lambda shp: rng.integers(-16, 17, size=shp) / 8.0
  p, t = grid(shape).astype(dtype), grid(shape).astype(dtype)
  for arr in (p, t):
    flat = arr.reshape(-1)
    for v in (np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(0)), np.inf, -np.inf, -0.0):
      flat[rng.integers(0, flat.size, size=max(1, flat.size // 40))] = v
  if mode != 'plain':
    p.reshape(-1)[rng.integers(0, p.size, size=max(1, p.size // 50))] = np.nan
    t.reshape(-1)[rng.integers(0, t.size, size=max(1, t.size // 50))] = np.nan
  fdims = [d for d in dims if rng.random() < 0.6] or [dims[-1]]
  fdims = [str(d) for d in rng.permutation(fdims)]
  fdims.insert(int(rng.integers(0, len(fdims) + 1)), THR)
  field = grid([k if d == THR else sizes[d] for d in fdims]).astype(thr_dtype)
  flat = field.reshape(-1)
  edges = [np.nan, np.inf, -np.inf, 0.0, np.float32(0.1)] + ([0.1, FC.F64_ABOVE_F32_TENTH, 1e40] if thr_dtype == np.float64 else [])
  for v in edges:
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 25))] = v
  coords = {d: np.arange(sizes[d]) * 1.5 for d in dims}
  t_order = [str(d) for d in rng.permutation(dims)]
  mask = None
  tc = dict(coords)
  if mode == 'masked':
    mdims = [d for d in dims if rng.random() < 0.7] or [dims[-1]]
    mask = rng.random([sizes[d] for d in mdims]) > 0.3
    tc['mask'] = (tuple(mdims), mask)
  pred = xr.DataArray(p, dims=dims, coords=coords, name='v')
  targ = xr.DataArray(np.ascontiguousarray(np.transpose(t, [dims.index(d) for d in t_order])), dims=t_order, coords=tc, name='v')
  fld = xr.DataArray(field, dims=fdims, coords={d: coords[d] for d in fdims if d != THR})
  reduce_dims = [d for d in dims if rng.random() < 0.6]
  # the restatement on the canonical order: thr[frame..., K]
  f = np.moveaxis(field, fdims.index(THR), -1)
  rest = [d for d in fdims if d != THR]
  f = np.transpose(f, [rest.index(d) for d in dims if d in rest] + [len(rest)])
  f = f.reshape([sizes[d] if d in rest else 1 for d in dims] + [k])
  stat = FC.field_stat(p, t, np.broadcast_to(f, tuple(shape) + (k,)))  # [frame..., 4 K]
  valid = np.ones(shape, bool)
  if mask is not None:
    valid = np.broadcast_to(mask.reshape([sizes[d] if d in mdims else 1 for d in dims]), shape)
  return dict(pred=pred, targ=targ, field=fld, dims=dims, reduce_dims=reduce_dims, mode=mode, k=k, stat=stat, valid=valid)


def _expected(case, cell):
  stat, valid, k = case['stat'][..., cell * case['k']:(cell + 1) * case['k']], case['valid'][..., None], case['k']
  axes = tuple(case['dims'].index(d) for d in case['reduce_dims'])
  ok = np.broadcast_to(valid, stat.shape)
  if case['mode'] == 'skipna':
    ok = ok & ~np.isnan(stat)
  return np.where(ok, stat, 0.0).sum(axis=axes), ok.astype(np.float64).sum(axis=axes), [d for d in case['dims'] if d not in case['reduce_dims']] + [THR], k


def _check(case, fused_expected):
  binary = lambda: wrappers.ContinuousToBinary('both', case['field'], THR, unique_name_suffix='f')
  metrics = {'csi': wrappers.WrappedMetric(categorical.CSI(), [binary()]), 'ets': wrappers.WrappedMetric(categorical.ETS(), [binary()])}
  agg = aggregation.Aggregator(reduce_dims=case['reduce_dims'], masked=case['mode'] == 'masked', skipna=case['mode'] == 'skipna')
  with np.errstate(all='ignore'):
    stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, {'v': case['pred']}, {'v': case['targ']})
    kinds = {(type(s), getattr(getattr(s, '_group', None), 'kind', None)) for per_var in stats.values() for s in per_var.values()}
    assert kinds == ({(lazy.LazyContingencyField, 'cont')} if fused_expected else {(xr.DataArray, None)}), kinds
    state = agg.aggregate_statistics(stats)
  for cell, name in enumerate(CELLS):
    key = next(k for k in state.sum_weighted_statistics if k.startswith(name))
    want, count, order, _ = _expected(case, cell)
    got = state.sum_weighted_statistics[key]['v']
    np.testing.assert_array_equal(np.asarray(got.transpose(*order).values, np.float64), want, err_msg=f'{name} {case["mode"]} {case["dims"]}')
    np.testing.assert_array_equal(np.asarray(state.sum_weights[key]['v'].transpose(*order).values, np.float64), count, err_msg=f'{name} counts')


@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(N_DEVICE))
def test_random_frames_and_fields_on_the_device(monkeypatch, seed):
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  engine.clear_caches()
  monkeypatch.setattr(lazy, 'FUSED_CONTINGENCY_FIELD', True)
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', [])
  case = draw_case(seed)
  _check(case, True)
  launches = [e for e in engine.S1_EVENT_LOG if e['kind'] == 'cont']
  assert len(launches) == -(-case['k'] // _hip.CONT_MAX_THRESHOLDS), engine.S1_EVENT_LOG
  engine.clear_caches()


@pytest.mark.parametrize('seed', range(N_EMULATED))
def test_the_bookkeeping_on_the_host_route(monkeypatch, seed):
  import fake_device  # pylint: disable=g-import-not-at-top
  engine.clear_caches()
  fake_device.install(monkeypatch)
  _check(draw_case(seed), False)
  engine.clear_caches()


def test_the_generator_covers_the_modes_and_both_block_counts():
  cases = [draw_case(s) for s in range(N_DEVICE)]
  assert {c['mode'] for c in cases} == set(MODES)
  assert {c['k'] > _hip.CONT_MAX_THRESHOLDS for c in cases} == {False, True}
  assert any(not c['reduce_dims'] for c in cases) or any(len(c['reduce_dims']) == len(c['dims']) for c in cases)
  finite = [np.isfinite(_expected(c, 3)[0]).mean() for c in cases]
  assert np.mean(finite) > 0.5, finite
