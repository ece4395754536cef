"""Zonal spectra of RED rows against the float64 oracle on every route of the library.

The older spectrum tests feed white rows, where S_k ~ S'_max at every wavenumber and an fp32 transform's error looks small
next to S_k.  Real fields are red: the tail of a k^-3 or k^-5 spectrum sits 8 to 14 orders of magnitude below S'_max, and
the second term of the per-row bound (1e-6 sqrt(S'_max S_k)) is only tested by rows with S_k << S'_max.  The rows come from
tests/spectrum_rows.py (white, temperature-, geopotential- and zonal-wind-like, single tones at the wavenumbers the mean-shift
estimates sample in phase); the oracle is always numpy.fft in float64 of the float32 row.

  (a) per row, every route: the route's documented bound (test_spectra.bound_1440 for the in-house kernels,
      library_bound for rocFFT), S_0 to 1e-6;
  (b) area-weighted means over 200 rows (4 leads x 50 latitudes): relative error per band within BAND_TOL, which is about
      3x the MI355X measurement of profiles/spectrum_accuracy_red_rows.txt (tests/measure_spectrum_error.py);
  (c) tones: S_k0 and S_0 to 1e-6 of the oracle, every other bin within tone_bound;
  (e) S_0 of rows whose shifted mean F'_0 is small but not 0 to S0_RTOL: F_0 = F'_0 + n m is formed in fp64, not fp32;
  (d) S(2^j x) == 2^2j S(x) bit for bit on the in-house kernels (no magnitude-dependent shortcut).

Routes through the public API take the `backend` fixture (the emulated half checks the test logic on the CPU); the raw C ABI
entry points of the fused det + spectra sweep are gpu tests.  Only variables the library reads per call are set here
(WBX_SPECTRUM_TEAM, WBX_SPECTRUM_PATH); the kernels selected by latched variables are reached through their default routes."""
import ctypes as C

import numpy as np
import pytest

from oracle import wbx_oracle as O
import spectrum_rows as R
from test_spectra import bound_1440
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import spectra
from weatherbenchx_amd import weighting
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base

FAMS = tuple(R.FAMILIES)
NLEAD, NLAT = 4, 50  # 200 rows per family and mean
LAT = np.linspace(-80, 80, NLAT)
SCALES = (-24, -8, 8, 24)


def library_bound(want):
  """The rocFFT route (include/wbx.h): |dS_k| <= 2e-5 S_k + 4e-7 sqrt(S_max S_k), S_max with the mean (k = 0) included.  The
  rows are shifted by their means in front of the transform like on the in-house routes (shift_rows_kernel)."""
  return 2e-5 * want + 4e-7 * np.sqrt(want.max(axis=-1, keepdims=True) * want)


# route -> (row length, layout, environment, route family).  'generic': zspec_fused_kernel (every 2/3/5-smooth even length
# but 1440, and 1440 with the team size pinned); 'z14': the 1440-point one-wave kernels (zspec1440_kernel lon-fastest,
# zspec1440_latfast_kernel lat-fastest); 'library': batched rocFFT (forced, odd lengths, a lon-fastest field that starts at an
# odd element -- not 8-byte aligned; the same view latitude-fastest goes through the transposing one-wave kernel).
ROUTES = {}
for _n in (64, 240, 360, 720, 1024, 2048):
  for _l in ('lon', 'lat'):
    ROUTES[f'generic{_n}-{_l}'] = (_n, _l, {}, 'generic')
for _g in ('64', '128', '256'):
  for _l in ('lon', 'lat'):
    ROUTES[f'team{_g}-1440-{_l}'] = (1440, _l, {'WBX_SPECTRUM_TEAM': _g}, 'generic')
ROUTES['z14-lon'] = (1440, 'lon', {}, 'z14')
ROUTES['z14-lat'] = (1440, 'lat', {}, 'z14')
ROUTES['offset-1440-lat'] = (1440, 'lat', {'offset': True}, 'z14')
for _l in ('lon', 'lat'):
  ROUTES[f'rocfft-1440-{_l}'] = (1440, _l, {'WBX_SPECTRUM_PATH': 'rocfft'}, 'library')
  ROUTES[f'odd45-{_l}'] = (45, _l, {}, 'library')
  ROUTES[f'odd1215-{_l}'] = (1215, _l, {}, 'library')
ROUTES['offset-1440-lon'] = (1440, 'lon', {'offset': True}, 'library')
IN_HOUSE = [r for r, v in ROUTES.items() if v[3] != 'library']

# (b): max over the band of |mean dS_k| / mean S_k of the area-weighted mean over 200 rows, per (route family, row family);
# bands of spectrum_rows.BANDS (1-9, 10-99, 100-299, 300-599, 600-end; shorter rows check the bands they have).  About 3x the
# largest value the routes of the family gave on an MI355X (profiles/spectrum_accuracy_red_rows.txt), rounded up on a 1-2-5
# scale, never below 2x it.  'fused': the det + spectra sweep (wbx_det_spectrum / _folded / _slabs).
BAND_TOL = {
    'generic': {'white': (5e-7, 5e-7, 5e-7, 5e-7, 5e-7), 'temperature': (5e-7, 1e-5, 1e-4, 2e-4, 5e-4),
                'geopotential': (1e-6, 1e-3, 2e-2, 1e-1, 2e0), 'wind': (5e-7, 1e-5, 1e-4, 2e-4, 1e-3)},
    'z14': {'white': (2e-7, 2e-7, 5e-7, 5e-7, 5e-7), 'temperature': (5e-7, 5e-6, 5e-5, 2e-4, 5e-4),
            'geopotential': (5e-7, 5e-4, 1e-2, 2e-1, 1e0), 'wind': (2e-7, 1e-5, 5e-5, 1e-4, 5e-4)},
    'fused': {'white': (2e-7, 5e-7, 5e-7, 5e-7, 5e-7), 'temperature': (2e-7, 5e-6, 5e-5, 2e-4, 5e-4),
              'geopotential': (5e-7, 5e-4, 1e-2, 1e-1, 1e0), 'wind': (2e-7, 5e-6, 5e-5, 2e-4, 5e-4)},
    'library': {'white': (5e-7, 5e-7, 5e-7, 5e-7, 5e-7), 'temperature': (5e-7, 1e-5, 5e-5, 1e-4, 1e-3),
                'geopotential': (2e-6, 5e-4, 5e-2, 1e-1, 2e0), 'wind': (5e-7, 5e-6, 1e-4, 2e-4, 1e-4)},
}


def red_field(nlon, seed=1):
  """float32[family, lead, latitude, longitude]: 200 rows of every row family."""
  return np.stack([R.family_rows(f, NLEAD * NLAT, nlon, seed + 10 * i).reshape(NLEAD, NLAT, nlon) for i, f in enumerate(FAMS)])


def area_mean(per_row):
  """[family, lead, latitude, k] -> the area-weighted mean over (lead, latitude): [family, k]."""
  w = O.grid_area_weights(LAT)[None, None, :, None]
  return (per_row * w).sum(axis=(1, 2)) / (w * np.ones_like(per_row)).sum(axis=(1, 2))


def route_bound(family, want):
  return library_bound(want) if family == 'library' else bound_1440(want)


# A coefficient the row has (almost) none of -- the bins next to a tone, which the fp32 rounding of 280 + 10 cos(k0 x) can
# leave at exactly 0 in the oracle -- still carries the square of the transform's own error, ~(eps |F'|_max)^2, which the
# relative terms of the bounds do not cover: those bins are held to the bound plus TONE_FLOOR x S'_max (3x the largest need
# measured on the routes, rounded up on a 1-2-5 scale: profiles/spectrum_accuracy_red_rows.txt, "absolute term needed").  A
# butterfly constant off by 1e-6 leaks (1e-6 |F_k0|)^2 ~ 1e-12 S_k0 into them.
TONE_FLOOR = 2e-14


def tone_bound(family, want):
  return route_bound(family, want) + TONE_FLOOR * want[..., 1:].max(axis=-1, keepdims=True)


def _odd_offset(arr, backend):
  """The same values in a view that starts one element into its allocation (device memory on hip)."""
  if backend == 'hip':
    import torch  # pylint: disable=g-import-not-at-top
    buf = torch.empty(arr.size + 1, dtype=torch.float32, device='cuda')
    buf[1:] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).to('cuda')
    torch.cuda.synchronize()
    return buf[1:].view(arr.shape)
  buf = np.empty(arr.size + 1, np.float32)
  buf[1:] = arr.reshape(-1)
  return buf[1:].reshape(arr.shape)


def public_spectra(vals, layout, backend, offset=False, energy=False, mean=True):
  """Spectra of vals[..., lat, lon] (leading dims: family, lead_time) through ZonalPowerSpectrum / ZonalEnergySpectrum on a
  longitude- or latitude-fastest field -> (per-row spectra [..., lat, k], area-weighted mean over (lead_time, latitude)
  [family, k] or None)."""
  nlon = vals.shape[-1]
  lead = ('family', 'lead_time')[:vals.ndim - 2]
  dims = lead + (('latitude', 'longitude') if layout == 'lon' else ('longitude', 'latitude'))
  arr = vals if layout == 'lon' else np.ascontiguousarray(np.swapaxes(vals, -1, -2))
  data = _odd_offset(arr, backend) if offset else arr
  lat = LAT if vals.shape[-2] == NLAT else np.linspace(-60, 60, vals.shape[-2])
  f = xr.DataArray(data, dims=dims, coords={'latitude': lat, 'longitude': np.arange(nlon) * (360.0 / nlon)})
  metric = spectra.ZonalEnergySpectrum() if energy else spectra.ZonalPowerSpectrum()
  per_row = np.asarray(metric.compute({'v': f}, {'v': f})['v'].transpose(*lead, 'latitude', 'zonal_wavenumber').values)
  if not mean:
    return per_row, None
  agg = aggregation.Aggregator(reduce_dims=['lead_time', 'latitude'], weigh_by=[weighting.GridAreaWeighting()])
  stats = metrics_base.compute_unique_statistics_for_all_metrics({'s': metric}, {'v': f}, {'v': f})
  means = agg.aggregate_statistics(stats).metric_values({'s': metric})['s.v'].transpose('family', 'zonal_wavenumber').values
  return per_row, np.asarray(means)


def _ratio(got, want, bound):
  """|got - want| / bound; a coefficient that is exactly 0 in the oracle (the rounded input of a steep row can cancel at a
  tail wavenumber) has to be 0."""
  d = np.abs(got - want)
  return np.divide(d, bound, out=np.where(d == 0, 0.0, np.inf), where=bound > 0)


def check_per_row(got, want, family, what=''):
  """(a): the route's bound at every wavenumber of every row, S_0 to 1e-6."""
  ratio = _ratio(got, want, route_bound(family, want))
  worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
  assert float(ratio.max()) <= 1.0, f'{what}: |dS| / bound = {float(ratio.max()):.3g} at {worst}'
  np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=1e-6, err_msg=f'{what}: S_0')


def band_mean_errors(got_mean, want_mean, nlon):
  """{row family: [max over the band of |mean dS_k| / mean S_k for each band of the row length]} of [family, k] means."""
  return {fam: [float(np.max(np.abs(got_mean[i, sl] - want_mean[i, sl]) / want_mean[i, sl])) for _, sl in R.band_slices(nlon)]
          for i, fam in enumerate(FAMS)}


def check_band_means(got_mean, want_mean, family, nlon, what=''):
  """(b): |mean dS_k| / mean S_k per band within BAND_TOL[family][row family]."""
  fails = []
  labels = [label for label, _ in R.band_slices(nlon)]
  for fam, errs in band_mean_errors(got_mean, want_mean, nlon).items():
    for b, err in enumerate(errs):
      if not err <= BAND_TOL[family][fam][b]:
        fails.append(f'{fam} k {labels[b]}: {err:.2e} > {BAND_TOL[family][fam][b]:.0e}')
  assert not fails, f'{what}: ' + '; '.join(fails)


def _set_env(monkeypatch, env):
  for k, v in env.items():
    if k != 'offset':
      monkeypatch.setenv(k, v)


def check_tones(got, want, ks, family, what=''):
  """(c): S_k0 and S_0 to 1e-6 of the oracle, every other bin within the route's bound (tone_bound)."""
  idx = np.arange(len(ks))
  np.testing.assert_allclose(got[idx, ks], want[idx, ks], rtol=1e-6, err_msg=f'{what}: S_k0, k0 = {ks}')
  np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=1e-6, err_msg=f'{what}: S_0')
  rest = np.ones(want.shape, bool)
  rest[idx, ks] = False
  rest[:, 0] = False
  ratio = np.where(rest, _ratio(got, want, tone_bound(family, want)), 0.0)
  assert float(ratio.max()) <= 1.0, (what, float(ratio.max()), np.unravel_index(int(np.argmax(ratio)), ratio.shape))


@pytest.mark.parametrize('route', list(ROUTES))
def test_red_rows_per_row_bound_and_band_means(backend, monkeypatch, route):
  """(a) and (b) on 4 x 200 rows (white, temperature-, geopotential-, zonal-wind-like) of the route's length and layout."""
  nlon, layout, env, family = ROUTES[route]
  _set_env(monkeypatch, env)
  vals = red_field(nlon)
  per_row, means = public_spectra(vals, layout, backend, offset=env.get('offset', False))
  want = O.zonal_power_spectrum(vals)
  check_per_row(per_row, want, family, route)
  check_band_means(means, area_mean(want), family, nlon, route)


@pytest.mark.parametrize('route', list(ROUTES))
def test_tones(backend, monkeypatch, route):
  """(c) 280 + 10 cos(k0 x + phi) at the wavenumbers the mean-shift estimates sample in phase (1440 points: 1, 2, 4, 6, 12),
  around a quarter of the row and at its end (Nyquist: 2 A^2), and one tone over a red background: S_k0 and S_0 = mean^2 to
  1e-6 of the oracle, every other bin within the route's bound."""
  nlon, layout, env, family = ROUTES[route]
  _set_env(monkeypatch, env)
  rows, ks, amps = R.tone_rows(nlon, seed=nlon)
  got, _ = public_spectra(rows, layout, backend, offset=env.get('offset', False), mean=False)
  want = O.zonal_power_spectrum(rows)
  # (the generator: the oracle of the pure tones is A^2 / 2, 2 A^2 at Nyquist, and mean^2 -- up to the input's fp32 rounding)
  pure = np.arange(len(ks) - 1)
  np.testing.assert_allclose(want[pure, ks[pure]], [R.tone_power(nlon, k, a) for k, a in zip(ks[pure], amps[pure])], rtol=1e-5)
  np.testing.assert_allclose(want[pure, 0], R.TONE_MEAN ** 2, rtol=1e-6)
  check_tones(got, want, ks, family, route)


# (e): with F_0 = F'_0 + n m formed in fp64, S_0 of a row near 280 comes out within 5e-16 of the oracle on every route but
# one; the same sum rounded to fp32 first is off by up to ulp(n m) / (n m) ~ 6e-8.  The lon-fastest one-wave kernel
# (zspec1440_kernel) gives 8.6e-8 on these rows -- inside its documented 1e-6, but fp32-like: held to 3x that (the
# profile, "(e)") until its k = 0 term is traced; the latitude-fastest kernel shares z14_pair's restore and is held tight.
S0_RTOL = 2e-9
S0_RTOL_Z14_LON = 5e-7


def check_s0(got, want, what=''):
  """(e): S_0 to S0_RTOL (S0_RTOL_Z14_LON on the lon-fastest one-wave kernel)."""
  rtol = S0_RTOL_Z14_LON if what == 'z14-lon' else S0_RTOL
  np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=rtol, err_msg=f'{what}: S_0')


@pytest.mark.parametrize('route', list(ROUTES))
def test_mean_is_restored_in_fp64(backend, monkeypatch, route):
  """(e) Rows of means 280.xxx (n m not representable in fp32) with a wavenumber-6 wave of 0.5 and noise of 1e-3 on top, so
  that the shift estimate misses the mean and F'_0 is small but not 0: S_0 to S0_RTOL of the oracle."""
  nlon, layout, env, _ = ROUTES[route]
  _set_env(monkeypatch, env)
  rng = np.random.default_rng(nlon + 5)
  x = 2 * np.pi * np.arange(nlon) / nlon
  means = 280.0 + rng.random(8)
  rows = (means[:, None] + 0.5 * np.cos(6 * x + 2 * np.pi * rng.random((8, 1))) + 1e-3 * rng.standard_normal((8, nlon)))
  rows = rows.astype(np.float32)
  got, _ = public_spectra(rows, layout, backend, offset=env.get('offset', False), mean=False)
  check_s0(got, O.zonal_power_spectrum(rows), route)


@pytest.mark.parametrize('route', IN_HOUSE)
def test_power_of_two_scaling_is_exact(backend, monkeypatch, route):
  """(d) S(2^j x) == 2^2j S(x) bit for bit, j = -24, -8, 8, 24: power-of-two scaling is exact in fp32 and fp64, so any
  difference is a magnitude-dependent shortcut in the kernel."""
  nlon, layout, env, _ = ROUTES[route]
  _set_env(monkeypatch, env)
  vals = np.stack([R.family_rows(f, 2 * 6, nlon, 3 + i).reshape(2, 6, nlon) for i, f in enumerate(FAMS)])
  base, _ = public_spectra(vals, layout, backend, offset=env.get('offset', False), mean=False)
  for j in SCALES:
    got, _ = public_spectra(vals * np.float32(2.0 ** j), layout, backend, offset=env.get('offset', False), mean=False)
    np.testing.assert_array_equal(got, base * 4.0 ** j, err_msg=f'{route}: 2^{j}')


def test_energy_spectrum_of_red_rows(backend):
  """ZonalEnergySpectrum (S_k times the circle of latitude) on the 1440-point lon-fastest route: (a) and (b) with the scale."""
  vals = red_field(1440, seed=7)
  per_row, means = public_spectra(vals, 'lon', backend, energy=True)
  circ = 2 * np.pi * spectra.EARTH_RADIUS_M * np.cos(np.deg2rad(LAT))[None, None, :, None]
  want = O.zonal_power_spectrum(vals) * circ
  check_per_row(per_row, want, 'z14', 'energy')
  w = O.grid_area_weights(LAT)[None, None, :, None]
  want_mean = (want * w).sum(axis=(1, 2)) / (w * np.ones_like(want)).sum(axis=(1, 2))
  check_band_means(means, want_mean, 'z14', 1440, 'energy')


# ---- the fused det + spectra sweep ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['folded', 'partial', 'latfast'])
def test_fused_det_spectra_sweep_on_red_fields(backend, monkeypatch, variant):
  """The chunk loop with a deterministic pass (area-weighted RMSE, MAE per (lead, level)) and zonal spectra of predictions and
  targets over the same red fields: engine.FUSE_DET_SPECTRA with stage 2 folded in (wbx_det_spectrum_folded) and not
  (wbx_det_spectrum), and on latitude-fastest fields (FUSE_DET_SPECTRA_LATFAST, wbx_det_spectrum_slabs).  Levels = the four row
  families, 4 init times x 50 latitudes = 200 rows per mean: spectra within BAND_TOL['fused'], deterministic values at 1e-6."""
  from weatherbenchx_amd import pipeline  # pylint: disable=g-import-not-at-top
  from weatherbenchx_amd import time_chunks  # pylint: disable=g-import-not-at-top
  from weatherbenchx_amd.metrics import deterministic  # pylint: disable=g-import-not-at-top
  monkeypatch.setattr(engine, 'FUSE_DET_SPECTRA', True)
  monkeypatch.setattr(engine, 'FOLD_DET_SPECTRA', variant == 'folded')
  monkeypatch.setattr(engine, 'FUSE_DET_SPECTRA_LATFAST', variant == 'latfast')
  ninit, nlon = NLEAD, 1440
  # [init, lead = 1, level = family, lat, lon]
  pv = np.moveaxis(red_field(nlon, seed=21), 0, 1)[:, None]
  tv = np.moveaxis(red_field(nlon, seed=41), 0, 1)[:, None]
  lon = np.arange(nlon) * 0.25
  init_times = np.datetime64('2021-06-01T00', 'ns') + np.arange(ninit) * np.timedelta64(24, 'h')
  lead_time = np.array([6], dtype='timedelta64[h]').astype('timedelta64[ns]')
  level = np.arange(len(FAMS))
  lat_fastest = variant == 'latfast'
  dims = ('init_time', 'lead_time', 'level') + (('longitude', 'latitude') if lat_fastest else ('latitude', 'longitude'))
  store = [np.ascontiguousarray(np.swapaxes(a, -1, -2)) if lat_fastest else a for a in (pv, tv)]

  def load(inits, leads):
    i = [int(np.where(init_times == x)[0][0]) for x in inits]
    cs = {'init_time': inits, 'lead_time': leads, 'level': level, 'latitude': LAT, 'longitude': lon}
    return {'z': xr.DataArray(store[0][i], dims=dims, coords=cs)}, {'z': xr.DataArray(store[1][i], dims=dims, coords=cs)}
  det = {'rmse': deterministic.RMSE(), 'mae': deterministic.MAE()}
  spec = {'sp': spectra.ZonalPowerSpectrum('predictions'), 'st': spectra.ZonalPowerSpectrum('targets')}
  area = aggregation.Aggregator(reduce_dims=['init_time', 'latitude', 'longitude'], weigh_by=[weighting.GridAreaWeighting()])
  zonal = aggregation.Aggregator(reduce_dims=['init_time', 'latitude'], weigh_by=[weighting.GridAreaWeighting()])
  times = time_chunks.TimeChunks(init_times, lead_time, init_time_chunk_size=1)
  engine.S1_EVENT_LOG, engine.S1_EVENT_REPEAT = [], 1
  try:
    out = pipeline.evaluate_passes(times, [('det', load, det, area), ('spec', load, spec, zonal)])
    kinds = [e['kind'] for e in engine.S1_EVENT_LOG]
  finally:
    engine.S1_EVENT_LOG = None
  if backend == 'hip':  # the fused launch ran, once per chunk, and no spectrum launch of its own
    assert kinds.count('det_spectrum') == ninit and 'spectrum' not in kinds, kinds
  dv, sv = out['det'][None].metric_values(det), out['spec'][None].metric_values(spec)
  w = O.grid_area_weights(LAT)[None, None, None, :, None]
  p64, t64 = pv.astype(np.float64), tv.astype(np.float64)
  wsum = (w * np.ones_like(p64)).sum(axis=(0, 3, 4))
  np.testing.assert_allclose(dv['rmse.z'].transpose('lead_time', 'level').values,
                             np.sqrt(((p64 - t64) ** 2 * w).sum(axis=(0, 3, 4)) / wsum), rtol=1e-6)
  np.testing.assert_allclose(dv['mae.z'].transpose('lead_time', 'level').values,
                             (np.abs(p64 - t64) * w).sum(axis=(0, 3, 4)) / wsum, rtol=1e-6)
  for key, f in (('sp.z', pv), ('st.z', tv)):
    got = sv[key].transpose('lead_time', 'level', 'zonal_wavenumber').values[0]
    # [init, family, lat, k] -> area mean over (init, lat): the same reduction as area_mean with init in the lead's place
    check_band_means(got, area_mean(np.moveaxis(O.zonal_power_spectrum(f[:, 0]), 0, 1)), 'fused', nlon, f'{variant} {key}')


def _raw_sweep(ctx, entry, pv, tv, group, scale, ngroup):
  """One raw wbx_det_spectrum / wbx_det_spectrum_folded / wbx_det_spectrum_slabs call (DET3) on pv, tv float32
  [lead, level, lat, lon]: -> (per-key sums of e, |e|, e^2 [nkey, 3] (det_out for the folded entry, det_scale = 1), power_p,
  power_t [ngroup, 721])."""
  from weatherbenchx_amd import planner  # pylint: disable=g-import-not-at-top
  nlead, nlev, nlat, nlon = pv.shape
  slabs = entry == 'slabs'
  dims = ('init_time', 'lead_time', 'level') + (('longitude', 'latitude') if slabs else ('latitude', 'longitude'))
  arrs = [np.ascontiguousarray(np.swapaxes(a, -1, -2) if slabs else a)[None] for a in (pv, tv)]
  devs = [engine._to_device(ctx, xr.DataArray(a, dims=dims), _hip.F32) for a in arrs]  # pylint: disable=protected-access
  lays = [d.layout for d in devs] + [None, None]
  sizes = dict(zip(dims, arrs[0].shape))
  extra = {'force_x_dim': 'longitude', 'allow_vec4': False} if slabs else {}
  plan = planner.build_s1_plan(dims, sizes, lays, ['init_time', 'latitude', 'longitude'], wdep_dims=['latitude'], **extra)
  nrows, nk = nlead * nlev * nlat, nlon // 2 + 1
  assert plan.nkey == nrows and plan.ndepth == 1 and plan.nchunk == 1
  dplan = engine._device_plan(ctx, plan)  # pylint: disable=protected-access
  g_dev, s_dev = ctx.upload(np.ascontiguousarray(group, np.int32)), ctx.upload(np.ascontiguousarray(scale, np.float64))
  part = ctx.alloc(max(nrows, ngroup) * 3 * 8)
  pw_p, pw_t = ctx.alloc(ngroup * nk * 8), ctx.alloc(ngroup * nk * 8)
  ptr = lambda d: C.c_void_p(d.ptr)
  p, t = ptr(devs[0]), ptr(devs[1])
  if entry == 'plain':
    _hip.check(ctx.lib.wbx_det_spectrum(ctx.handle, C.byref(dplan.struct), _hip.DET3, _hip.F32, p, t, None, ptr(g_dev), ptr(s_dev),
                                        ngroup, ptr(part), ptr(pw_p), ptr(pw_t)), 'wbx_det_spectrum')
    nout = nrows
  elif entry == 'folded':
    d_dev = ctx.upload(np.ones(nrows))
    _hip.check(ctx.lib.wbx_det_spectrum_folded(ctx.handle, C.byref(dplan.struct), _hip.DET3, _hip.F32, p, t, None, ptr(g_dev),
                                               ptr(s_dev), ptr(d_dev), ngroup, ptr(part), ptr(pw_p), ptr(pw_t)),
               'wbx_det_spectrum_folded')
    nout = ngroup
  else:
    _hip.check(ctx.lib.wbx_det_spectrum_slabs(ctx.handle, C.byref(dplan.struct), _hip.DET3, _hip.F32, p, t, None, nlat, ptr(g_dev),
                                              ptr(s_dev), ngroup, ptr(part), ptr(pw_p), ptr(pw_t)), 'wbx_det_spectrum_slabs')
    nout = nrows
  ctx.synchronize()
  return (ctx.download(part.ptr, (nout, 3)).copy(), ctx.download(pw_p.ptr, (ngroup, nk)).copy(),
          ctx.download(pw_t.ptr, (ngroup, nk)).copy())


@pytest.mark.gpu
@pytest.mark.parametrize('entry', ['plain', 'folded', 'slabs'])
def test_det_spectrum_entry_points_on_red_rows(entry):
  """The raw entry points of the fused sweep on [family, lead, lat, 1440] red fields: one group per row -> (a) for both
  spectra and the per-row deterministic sums at the existing 1e-11; the families' area-weighted means -> (b) within
  BAND_TOL['fused']; (d) 2^j x bit for bit."""
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  ctx = _hip.default_context(0)
  pv, tv = red_field(1440, seed=61), red_field(1440, seed=81)
  nfam, nlead, nlat, nlon = pv.shape
  nrows = nfam * nlead * nlat
  rows = np.arange(nrows, dtype=np.int32)
  sums, sp, st = _raw_sweep(ctx, entry, pv, tv, rows, np.ones(nrows), nrows)
  p64, t64 = pv.astype(np.float64), tv.astype(np.float64)
  want_sums = [O.error(p64, t64), O.absolute_error(p64, t64), O.squared_error(p64, t64)]
  for lane, wv in enumerate(want_sums):
    np.testing.assert_allclose(sums[:, lane], wv.sum(axis=-1).reshape(-1), rtol=1e-11, atol=1e-6, err_msg=f'{entry} lane {lane}')
  want_p, want_t = O.zonal_power_spectrum(pv), O.zonal_power_spectrum(tv)
  check_per_row(sp, want_p.reshape(nrows, -1), 'z14', f'{entry} p')
  check_per_row(st, want_t.reshape(nrows, -1), 'z14', f'{entry} t')
  # the families' means: group = family, scale = area weight / sum of the family's weights
  w = np.broadcast_to(O.grid_area_weights(LAT), (nfam, nlead, nlat))
  scale = (w / w[0].sum()).reshape(-1)
  group = np.repeat(np.arange(nfam, dtype=np.int32), nlead * nlat)
  _, mp, mt = _raw_sweep(ctx, entry, pv, tv, group, scale, nfam)
  check_band_means(mp, area_mean(want_p), 'fused', nlon, f'{entry} p')
  check_band_means(mt, area_mean(want_t), 'fused', nlon, f'{entry} t')
  for j in SCALES:
    s = np.float32(2.0 ** j)
    _, gp, gt = _raw_sweep(ctx, entry, pv * s, tv * s, rows, np.ones(nrows), nrows)
    np.testing.assert_array_equal(gp, sp * 4.0 ** j, err_msg=f'{entry} p 2^{j}')
    np.testing.assert_array_equal(gt, st * 4.0 ** j, err_msg=f'{entry} t 2^{j}')
