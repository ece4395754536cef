"""Measured error of the zonal spectrum routes against the float64 numpy.fft oracle -- where the bounds and tolerances of
tests/test_spectra.py and tests/test_spectra_red.py come from.  A checker like the tests next to it (it calls the oracle), not
collected by pytest.  usage (GPU box): python tests/measure_spectrum_error.py [--white-only | --red-only]

Part 1, white rows (N(0, 1) and N(280, 1), 1440 points, both layouts): per row median / 99.9th percentile / maximum relative
error and the maximum of |dS_k| / sqrt(S_max S_k); relative error after the area-weighted mean over 200 rows.

Part 2, red rows and tones on every route (tests/spectrum_rows.py; profiles/spectrum_accuracy_red_rows.txt): runs the test
functions of tests/test_spectra_red.py on the device with their checks replaced by recorders, so the numbers are exactly
what the tests compare.  Per route and row family, per band of wavenumbers: the per-row median of |dS_k| / S_k, the maximum of
|mean dS_k| / mean S_k over 200 area-weighted rows, and both as multiples of the fp32 floor (tools/spectrum_fp32_floor.py:
a plain fp32 mixed-radix transform of the same rows, emulated on the CPU); the worst |dS_k| / bound per row, the tones' worst
relative error of S_k0 and S_0.  Last, per (route family, row family, band): the largest mean error of the family's routes
and 3x it rounded up on a 1-2-5 scale -- BAND_TOL of tests/test_spectra_red.py."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
  if _p not in sys.path:
    sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import pytest  # noqa: E402

from oracle import wbx_oracle as O  # noqa: E402
from weatherbenchx_amd import aggregation, engine, spectra, weighting  # noqa: E402
from weatherbenchx_amd import xarray_lite as xr  # noqa: E402
from weatherbenchx_amd.metrics import base as mb  # noqa: E402


def white_rows():
  for layout in ('lon_fastest', 'lat_fastest'):
    for mean in (0.0, 280.0):
      rng = np.random.default_rng(1)
      nlat, nlon = 50, 1440
      lat, lon = np.linspace(-80, 80, nlat), np.arange(nlon) * 0.25
      dims = ('lead_time', 'level', 'latitude', 'longitude') if layout == 'lon_fastest' else ('lead_time', 'level', 'longitude', 'latitude')
      shape = {'lead_time': 4, 'level': 3, 'latitude': nlat, 'longitude': nlon}
      vals = (rng.normal(size=[shape[d] for d in dims]) + mean).astype(np.float32)
      f = xr.DataArray(vals, dims=dims, coords={'latitude': lat, 'longitude': lon})
      lon_ax = dims.index('longitude')
      per_row = np.moveaxis(O.zonal_power_spectrum(vals, lon_axis=lon_ax), lon_ax, -1)
      rd = tuple(d for d in dims if d != 'longitude')
      stat = np.asarray(spectra.ZonalPowerSpectrum().compute({'v': f}, {'v': f})['v'].transpose(*rd, 'zonal_wavenumber').values)
      rel = np.abs(stat - per_row) / per_row
      relmax = np.abs(stat - per_row) / np.sqrt(per_row.max(-1, keepdims=True) * per_row)
      print(layout, mean, 'per-row: median rel', np.median(rel), 'p99.9 rel', np.quantile(rel, 0.999), 'max rel', rel.max(), 'max |d|/sqrt(Smax S)', relmax.max())
      metrics = {'spec': spectra.ZonalPowerSpectrum()}
      agg = aggregation.Aggregator(reduce_dims=['lead_time', 'latitude'], weigh_by=[weighting.GridAreaWeighting()])
      res = agg.aggregate_statistics(mb.compute_unique_statistics_for_all_metrics(metrics, {'v': f}, {'v': f})).metric_values(metrics)
      wv = O.expand_to(O.grid_area_weights(lat), ('latitude',), rd)[..., None]
      red = tuple(rd.index(d) for d in ('lead_time', 'latitude'))
      want = (per_row * wv).sum(axis=red) / (wv * np.ones_like(per_row)).sum(axis=red)
      got = res['spec.v'].transpose('level', 'zonal_wavenumber').values
      rel = np.abs(got - want) / want
      print('   aggregated over 200 rows: median rel', np.median(rel), 'max rel', rel.max())


def _up125(x):
  """The smallest 1, 2 or 5 x 10^n >= x."""
  e = math.floor(math.log10(x))
  for m in (1, 2, 5, 10):
    if m * 10.0 ** e >= x * (1 - 1e-12):
      return m * 10.0 ** e
  return 10.0 ** (e + 1)


def red_rows():
  import spectrum_fp32_floor as F  # pylint: disable=g-import-not-at-top
  import spectrum_rows as R  # pylint: disable=g-import-not-at-top
  import test_spectra_red as T  # pylint: disable=g-import-not-at-top
  fams = T.FAMS
  wrow = np.broadcast_to(O.grid_area_weights(T.LAT), (T.NLEAD, T.NLAT)).reshape(-1)
  floors = {}

  def floor(nlon, seed=1):
    """The fp32 floor of the very rows a test feeds: red_field(nlon, seed)."""
    if (nlon, seed) not in floors:
      vals = T.red_field(nlon, seed=seed)
      floors[nlon, seed] = {}
      for i, fam in enumerate(fams):
        rows = vals[i].reshape(-1, nlon)
        floors[nlon, seed][fam] = R.band_errors(F.spectrum_fp32(rows), O.zonal_power_spectrum(rows), wrow, nlon)
    return floors[nlon, seed]

  def seed_of(what):
    """The seed of red_field behind a check's label (the tests' own seeds)."""
    if what == 'energy':
      return 7
    if what.endswith('sp.z'):
      return 21
    if what.endswith('st.z'):
      return 41
    if what.endswith(' p'):
      return 61
    if what.endswith(' t'):
      return 81
    return 1

  cur = {}
  multiples = {}  # route family -> [(per-row median / floor, 200-row mean / floor)]
  needs = {'tone': 0.0, 's0': 0.0}
  records = []  # (route, route family, nlon, {fam: [(median, mean)]})

  def rec_per_row(got, want, family, what=''):
    ratio = T._ratio(got, want, T.route_bound(family, want))  # pylint: disable=protected-access
    s0 = float(np.max(np.abs(got[..., 0] - want[..., 0]) / want[..., 0]))
    ref = want if family == 'library' else want[..., 1:]
    # the absolute term (x S'_max, S_max on the library route) the bound would need to cover every coefficient
    extra = float(np.max((np.abs(got - want) - T.route_bound(family, want)) / ref.max(axis=-1, keepdims=True)))
    nlon = 2 * (want.shape[-1] - 1) + cur.get('odd', 0)
    g, w = got.reshape(len(fams), -1, want.shape[-1]), want.reshape(len(fams), -1, want.shape[-1])
    # (an exact zero of a steep row's rounded tail in the oracle -- 0 / 0 -- is left out of the median)
    med = {fam: [float(np.nanmedian(np.abs(g[i][:, sl] - w[i][:, sl]) / w[i][:, sl])) for _, sl in R.band_slices(nlon)]
           for i, fam in enumerate(fams)}
    cur.setdefault('per_row', []).append((what, float(ratio.max()), s0, med, extra))

  def rec_band(got_mean, want_mean, family, nlon, what=''):
    cur.setdefault('bands', []).append((what, family, nlon, T.band_mean_errors(got_mean, want_mean, nlon)))

  def rec_tones(got, want, ks, family, what=''):
    idx = np.arange(len(ks))
    rest = np.ones(want.shape, bool)
    rest[idx, ks] = False
    rest[:, 0] = False
    ratio = np.where(rest, T._ratio(got, want, T.tone_bound(family, want)), 0.0)  # pylint: disable=protected-access
    ref = want[..., 1:]
    extra = np.where(rest, (np.abs(got - want) - T.route_bound(family, want)) / ref.max(axis=-1, keepdims=True), 0.0)
    cur['tones'] = (float(np.max(np.abs(got[idx, ks] / want[idx, ks] - 1))), float(np.max(np.abs(got[:, 0] / want[:, 0] - 1))),
                    float(ratio.max()), max(float(extra.max()), 0.0))

  def rec_s0(got, want, what=''):
    cur['s0'] = float(np.max(np.abs(got[:, 0] / want[:, 0] - 1)))

  T.check_per_row, T.check_band_means, T.check_tones, T.check_s0 = rec_per_row, rec_band, rec_tones, rec_s0

  def run(fn, *args):
    engine.clear_caches()
    with pytest.MonkeyPatch.context() as mp:
      try:
        fn(*[mp if a is MP else a for a in args])
        return 'ok'
      except AssertionError as e:
        return 'FAILED ' + str(e).splitlines()[0][:200]
      finally:
        engine.clear_caches()
  MP = object()

  def show(route, family, nlon):
    labels = [label for label, _ in R.band_slices(nlon)]
    for what, worst, s0, med, extra in cur.get('per_row', []):
      print(f'  (a) {what}: max |dS_k| / bound {worst:.3f}   S_0 rel {s0:.1e}   absolute term needed {max(extra, 0):.1e} x S\'_max')
    for what, fam_route, n, errs in cur.get('bands', []):
      fl = floor(n, seed_of(what))
      meds = next((r[3] for r in cur.get('per_row', []) if r[0] == what), None)
      print(f'  (b) {what}  [{fam_route}]   band: per-row median | 200-row mean  (x fp32 floor)')
      for fam in fams:
        cells = []
        for b, lab in enumerate(labels if n == nlon else [l for l, _ in R.band_slices(n)]):
          fm, fmean = fl[fam][lab]
          # (the chunk-loop tests only see the means: no per-row median there)
          md = f'{meds[fam][b]:.1e}' if meds else '-'
          mdx = f'x{meds[fam][b] / fm:4.1f}' if meds else 'x   -'
          cells.append(f'{lab:>8s} {md} | {errs[fam][b]:.1e} ({mdx} | x{errs[fam][b] / fmean:4.1f})')
          multiples.setdefault(fam_route, []).append((meds[fam][b] / fm if meds else float('nan'), errs[fam][b] / fmean))
        print(f'      {fam:13s}' + '  '.join(cells))
      records.append((what, fam_route, n, errs))

  print('\nfp32 floor (tools/spectrum_fp32_floor.py) of the same rows, per-row median | 200-row area-weighted mean (max in band)')
  for nlon in sorted({v[0] for v in T.ROUTES.values()}):
    print(f'  {nlon} points')
    for fam, errs in floor(nlon).items():
      print(f'      {fam:13s}' + '  '.join(f'{b:>8s} {e[0]:.1e} | {e[1]:.1e}' for b, e in errs.items()))

  for route, (nlon, _, _, family) in T.ROUTES.items():
    cur.clear()
    cur['odd'] = nlon % 2
    st = run(T.test_red_rows_per_row_bound_and_band_means, 'hip', MP, route)
    print(f'\n{route}  ({family}, {nlon} points)  red rows: {st}')
    show(route, family, nlon)
    st = run(T.test_tones, 'hip', MP, route)
    t = cur.get('tones')
    print(f'  (c) tones: {st}' + (f'   max |S_k0 / oracle - 1| {t[0]:.1e}  S_0 {t[1]:.1e}  other bins max |dS| / tone_bound {t[2]:.3f} (absolute term needed {t[3]:.1e} x S\'_max)' if t else ''))
    if t:
      needs['tone'] = max(needs['tone'], t[3])
    st = run(T.test_mean_is_restored_in_fp64, 'hip', MP, route)
    needs['s0'] = max(needs['s0'], cur.get('s0', 0.0))
    print(f'  (e) S_0 of rows with a small F\'_0: {st}   max |S_0 / oracle - 1| {cur.get("s0", float("nan")):.1e}')
    if route in T.IN_HOUSE:
      print(f'  (d) 2^j scaling bit for bit: {run(T.test_power_of_two_scaling_is_exact, "hip", MP, route)}')
  cur.clear()
  print(f'\nenergy spectrum (z14, 1440 points): {run(T.test_energy_spectrum_of_red_rows, "hip")}')
  show('energy', 'z14', 1440)
  for variant in ('folded', 'partial', 'latfast'):
    cur.clear()
    print(f'\nfused det + spectra sweep through the chunk loop, {variant}: {run(T.test_fused_det_spectra_sweep_on_red_fields, "hip", MP, variant)}')
    show('fused', 'fused', 1440)
  for entry in ('plain', 'folded', 'slabs'):
    cur.clear()
    print(f'\nraw wbx_det_spectrum entry point, {entry}: {run(T.test_det_spectrum_entry_points_on_red_rows, entry)}')
    show('fused', 'fused', 1440)

  print('\n(b) per (route family, row family): largest 200-row mean error per band over the family\'s routes -> 3x, rounded up '
        'on a 1-2-5 scale')
  for family in ('generic', 'z14', 'fused', 'library'):
    for fam in fams:
      worst = [0.0] * len(R.BANDS)
      for _, fr, n, errs in records:
        if fr == family:
          for b, e in enumerate(errs[fam]):
            worst[b] = max(worst[b], e)
      print(f'  {family:8s} {fam:13s} measured ' + ' '.join(f'{w:.1e}' for w in worst) + '   tolerance ' +
            ' '.join(f'{_up125(3 * w):.0e}' if w > 0 else '-' for w in worst))
  print('\nerror as a multiple of the fp32 floor of the same rows, min - max over routes, row families and bands: per-row median | '
        '200-row mean')
  for family, ms in multiples.items():
    a, b = np.array([m[0] for m in ms]), np.array([m[1] for m in ms])
    print(f'  {family:8s} x{np.nanmin(a):.1f} - x{np.nanmax(a):.1f} | x{np.nanmin(b):.1f} - x{np.nanmax(b):.1f}')
  print(f"\n(c) largest absolute term the tones' side bins need: {needs['tone']:.1e} x S'_max -> TONE_FLOOR {_up125(3 * needs['tone']):.0e}")
  print(f"(e) largest S_0 error of the rows with a small F'_0: {needs['s0']:.1e} -> S0_RTOL {_up125(3 * needs['s0']):.0e}")


if __name__ == '__main__':
  if '--red-only' not in sys.argv:
    white_rows()
  if '--white-only' not in sys.argv:
    with np.errstate(divide='ignore', invalid='ignore'):
      red_rows()
