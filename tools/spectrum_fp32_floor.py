"""The fp32 floor of a zonal spectrum: what a plain single-precision mixed-radix transform gets wrong on the rows of
tests/spectrum_rows.py, emulated on the CPU -- NumPy complex64 arithmetic (fp32 twiddles, fp32 butterflies), decimation in
time, the full complex transform of the real row (1440 = 12 * 12 * 10), every row shifted by its fp32 mean in front of the
transform and F_0 put back in fp64 -- against float64 numpy.fft of the same fp32 rows.  No GPU needed.

tests/measure_spectrum_error.py divides the HIP kernels' error by this floor; profiles/spectrum_accuracy_red_rows.txt holds
both.  usage: python tools/spectrum_fp32_floor.py [nlon ...]   (default 1440)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import spectrum_rows as R  # noqa: E402


def _radices(n):
  """Greedy factorisation into radices 12, 10, 8, 6, 5, 4, 3, 2 (1440 -> 12 * 12 * 10)."""
  out = []
  while n > 1:
    for r in (12, 10, 8, 6, 5, 4, 3, 2):
      if n % r == 0:
        out.append(r)
        n //= r
        break
    else:
      raise ValueError(f'{n} is not 2/3/5-smooth')
  return out


def _dft_matrix(r):
  j = np.arange(r)
  return np.exp(-2j * np.pi * np.outer(j, j) / r).astype(np.complex64)


def fft_c64(x, radices=None):
  """Complex transform along the last axis in complex64 arithmetic: X[k + m q] = sum_j W_r^(j q) (W_N^(j k) X_j[k]), X_j
  the transform of x[j::r] (m = N / r)."""
  n = x.shape[-1]
  radices = _radices(n) if radices is None else radices
  r = radices[0]
  if len(radices) == 1:
    return np.einsum('qj,...j->...q', _dft_matrix(r), x).astype(np.complex64)
  m = n // r
  sub = np.stack([fft_c64(x[..., j::r], radices[1:]) for j in range(r)], axis=-2)  # [..., j, k]
  tw = np.exp(-2j * np.pi * np.outer(np.arange(r), np.arange(m)) / n).astype(np.complex64)
  t = (sub * tw).astype(np.complex64)
  out = np.einsum('qj,...jk->...qk', _dft_matrix(r), t).astype(np.complex64)  # [..., q, k] -> index k + m q
  return out.reshape(x.shape[:-1] + (n,))


def spectrum_fp32(rows):
  """S_k of float32 rows through the emulated fp32 transform (the row shifted by its fp32 mean, F_0 restored in fp64)."""
  rows = np.asarray(rows, np.float32)
  n = rows.shape[-1]
  m = rows.mean(axis=-1, dtype=np.float32, keepdims=True)
  F = fft_c64((rows - m).astype(np.complex64))[..., :n // 2 + 1].astype(np.complex128) / n
  F[..., 0] += m[..., 0].astype(np.float64)
  S = F.real ** 2 + F.imag ** 2
  S[..., 1:] *= 2
  return S


def main():
  from oracle import wbx_oracle as O  # pylint: disable=g-import-not-at-top
  nlons = [int(a) for a in sys.argv[1:]] or [1440]
  for nlon in nlons:
    print(f'fp32 floor, {nlon}-point rows: relative error of S_k, per-row median | 200-row mean (max in band)')
    for fam in R.FAMILIES:
      rows = R.family_rows(fam, 200, nlon, seed=1)
      errs = R.band_errors(spectrum_fp32(rows), O.zonal_power_spectrum(rows), np.ones(200), nlon)
      print(f'  {fam:13s} ' + '  '.join(f'{b:>8s} {e[0]:.1e} | {e[1]:.1e}' for b, e in errs.items()))


if __name__ == '__main__':
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  main()
