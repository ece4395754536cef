"""Deterministic zonal rows for the spectrum accuracy tests (tests/test_spectra_red.py, tests/measure_spectrum_error.py,
tools/spectrum_fp32_floor.py).  A plain helper module, not a fixture file.

White rows -- the only rows the older spectrum tests use -- have S_k ~ S'_max at every wavenumber, the one regime where an
fp32 transform's error looks small next to S_k.  Real fields are red (S_k ~ k^-3 for temperature and wind, steeper for
geopotential): the tail of the spectrum sits 8 to 14 orders of magnitude below S'_max = max_{k >= 1} S_k.  `red_rows` builds
such rows, `tone_rows` single waves at the wavenumbers the kernels' mean-shift estimates sample in phase.  Every row is
returned as float32: the oracle (oracle.wbx_oracle.zonal_power_spectrum) is always applied to the float32 row, so the input
rounding is on both sides."""
import numpy as np

# name -> (spectral slope, mean, standard deviation); S_k ~ k^-slope for k >= 1
FAMILIES = {
    'white': (0.0, 280.0, 10.0),
    'temperature': (3.0, 280.0, 10.0),     # k^-3, 280 +- 10 (K)
    'geopotential': (5.0, 5.4e4, 1.0e3),   # k^-5, 5.4e4 +- 1e3 (m^2 s^-2)
    'wind': (3.0, 5.0, 15.0),              # k^-3, 5 +- 15 (m/s): crosses zero, the shift by the mean is not exact
}
TONE_AMPLITUDE, TONE_MEAN = 10.0, 280.0
# bands of wavenumbers on a 1440-point row (clipped to the row's own wavenumbers on other lengths; the last band runs to
# the last wavenumber of the row)
BANDS = ((1, 9), (10, 99), (100, 299), (300, 599), (600, None))


def band_slices(nlon):
  """[(label, slice of wavenumbers)] of BANDS that exist on rows of `nlon` points."""
  nk = nlon // 2 + 1
  out = []
  for lo, hi in BANDS:
    hi = nk - 1 if hi is None else min(hi, nk - 1)
    if lo <= hi:
      out.append((f'{lo}-{hi}', slice(lo, hi + 1)))
  return out


def red_rows(nrows, nlon, slope, mean, sigma, seed):
  """float32[nrows, nlon]: float64 irfft of amplitudes k^(-slope / 2) (k >= 1) with random phases and a real Nyquist term
  (even nlon), each row rescaled to standard deviation `sigma`, plus `mean`, then rounded to float32."""
  rng = np.random.default_rng(seed)
  nk = nlon // 2 + 1
  k = np.arange(nk, dtype=np.float64)
  amp = np.zeros(nk)
  amp[1:] = k[1:] ** (-slope / 2.0)
  coef = amp * np.exp(2j * np.pi * rng.random((nrows, nk)))
  if nlon % 2 == 0:
    coef[:, -1] = amp[-1] * rng.choice([-1.0, 1.0], size=nrows)
  x = np.fft.irfft(coef, n=nlon, axis=-1)
  x *= sigma / x.std(axis=-1, keepdims=True)
  return (x + mean).astype(np.float32)


def family_rows(family, nrows, nlon, seed):
  slope, mean, sigma = FAMILIES[family]
  return red_rows(nrows, nlon, slope, mean, sigma, seed)


def tone_wavenumbers(nlon):
  """1, 2, 4, 6, 12 (the large scales the shift estimates sample in phase), nlon/4 - 1 .. nlon/4 + 1 and the last two
  wavenumbers -- on 1440 points: 1, 2, 4, 6, 12, 359, 360, 361, 719, 720."""
  h = nlon // 2
  ks = [1, 2, 4, 6, 12, h // 2 - 1, h // 2, h // 2 + 1, h - 1, h]
  return sorted({k for k in ks if 1 <= k <= h})


def tone_rows(nlon, seed, mixed_k=12):
  """-> (float32[nrows, nlon], k0[nrows], amplitude[nrows]).  TONE_MEAN + A cos(k0 x + phi), x = 2 pi j / nlon, A = 10, for
  every k0 of tone_wavenumbers (phi = 0 at the Nyquist wavenumber of an even row, random elsewhere), plus one row with the
  tone k0 = `mixed_k` over a temperature-like k^-3 background of standard deviation 1 (the last row)."""
  rng = np.random.default_rng(seed)
  x = 2 * np.pi * np.arange(nlon) / nlon
  ks = tone_wavenumbers(nlon)
  rows = []
  for k0 in ks:
    phi = 0.0 if 2 * k0 == nlon else 2 * np.pi * rng.random()
    rows.append(TONE_MEAN + TONE_AMPLITUDE * np.cos(k0 * x + phi))
  bg = red_rows(1, nlon, 3.0, 0.0, 1.0, seed + 1)[0].astype(np.float64)
  rows.append(TONE_MEAN + TONE_AMPLITUDE * np.cos(mixed_k * x + 2 * np.pi * rng.random()) + bg)
  return np.stack(rows).astype(np.float32), np.array(ks + [mixed_k]), np.full(len(ks) + 1, TONE_AMPLITUDE)


def tone_power(nlon, k0, amplitude):
  """What the oracle gives for A cos(k0 x + phi): A^2 / 2, and 2 A^2 at the Nyquist wavenumber (S_k doubles every k >= 1,
  Nyquist included: A (-1)^j has |F_{n/2}| = A)."""
  return 2 * amplitude ** 2 if 2 * k0 == nlon else amplitude ** 2 / 2


def band_errors(got, want, weights, nlon, got_mean=None):
  """Relative error of a set of per-row spectra, per band: {band: (median over the rows and wavenumbers of |dS_k| / S_k,
  max over the band of |mean dS_k| / mean S_k)} -- `got`, `want` [nrows, nk], the mean weighted by `weights` [nrows]
  (`got_mean` [nk]: the mean as the library aggregated it, instead of the mean of `got`)."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  w = np.asarray(weights, np.float64)[:, None]
  mw = (want * w).sum(0) / w.sum()
  mg = (got * w).sum(0) / w.sum() if got_mean is None else np.asarray(got_mean, np.float64)
  out = {}
  for label, sl in band_slices(nlon):
    with np.errstate(divide='ignore', invalid='ignore'):  # (an exact zero of a steep row's rounded tail: inf, not counted in the median's middle)
      out[label] = (float(np.median(np.abs(got[:, sl] - want[:, sl]) / want[:, sl])),
                    float(np.max(np.abs(mg[sl] - mw[sl]) / mw[sl])))
  return out
