"""Interval statistics of an ensemble (wbx_ens_interval_partial): kernel time against its floors, and Opportunism through the public
API end to end against the host route.

(a) f32[M, T, 721, 1440] predictions (M = 51 and 4 members; T = 13 valid times and a single field), targets of the frame and a
    climatology f32[4 days, 4 hours, 2 quantile levels, 721, 1440] gathered in place, all generated on the device.  The launches
    go through the group the statistics build (lazy.interval_statistic -> FusedGroup.reduce), each between a HIP event pair
    (engine.S1_EVENT_LOG), medians of REPS; Covered alone and all three lanes; the frame reduced over every dim (x summed) and over
    (valid_time, latitude) (x kept).  Next to each: the HBM floor, (M + 1) x 4 bytes per point for Covered alone and
    (M + 1 + 2) x 4 for the three lanes against a two-level climatology (four values, two addresses), / 8 TB/s; and the VALU floor
    of the sort: NINSTR of csrc/wbx_sortnet3_gen.hpp at the padded size + MEMBER_INSTRUCTIONS per loaded member (its NaN test and
    its LDS store or padding select) / (256 CUs x 64 lanes x the probed clock).
(b) Opportunism(True, True, True) of device-resident tensors of the same shapes through the public API: host wall time from
    compute_unique_statistics_for_all_metrics through Aggregator.aggregate_statistics up to a synchronise, the fused route against
    WBX_FUSED_INTERVALS=0 on the same payload in the same process.  The requirement: the fused route is not slower at any shape.
(c) the same metric on a small float64 payload on both routes: identical indicators, so the scores agree to the summation's rounding.

Usage: python tools/bench_intervals.py [--out profiles/intervals_kbench.txt] [--skip-kernel] [--skip-e2e]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from weatherbenchx_amd import _hip, aggregation, engine, lazy
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import categorical

SHAPES = ((51, 13), (51, 1), (4, 13), (4, 1))  # (members, valid times) of a 721 x 1440 grid
GRID = (721, 1440)
REPS = 10
HBM_TBS = 8.0
CUS, LANES = 256, 64
NETWORK = {4: 8, 8: 29, 16: 97, 32: 301, 50: 586, 51: 606, 64: 850}  # padded size -> NINSTR (csrc/wbx_sortnet3_gen.hpp)
MEMBER_INSTRUCTIONS = 2  # v_cmp_u_f32 and ds_write_b32
DIMS = ('valid_time', 'latitude', 'longitude')
LEVELS = (0.1, 0.9)


def padded(m):
  return next(s for s in sorted(NETWORK) if m <= s)


def _inputs(seed, m, nt, dtype, grid=GRID):
  import torch  # pylint: disable=g-import-not-at-top
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  shape = (nt,) + tuple(grid)
  p = torch.randn((m,) + shape, generator=g, device='cuda', dtype=dtype)
  t = torch.randn(shape, generator=g, device='cuda', dtype=dtype) * 0.7
  lo = torch.randn((4, 4, 1) + tuple(grid), generator=g, device='cuda', dtype=dtype) * 0.3 - 1.0
  clim = torch.cat([lo, lo + 0.5 + 2.5 * torch.rand(lo.shape, generator=g, device='cuda', dtype=dtype)], dim=2)
  coords = {'valid_time': np.datetime64('2020-01-01T00', 'ns') + np.arange(nt) * np.timedelta64(6, 'h'),
            'latitude': np.linspace(-90, 90, grid[0]), 'longitude': np.linspace(0, 360, grid[1], endpoint=False)}
  pred = {'v': xr.DataArray(p, dims=('number',) + DIMS, coords=coords, name='v')}
  targ = {'v': xr.DataArray(t, dims=DIMS, coords=coords, name='v')}
  climatology = xr.Dataset({'v': xr.DataArray(clim, dims=('dayofyear', 'hour', 'quantile', 'latitude', 'longitude'), coords={
      'dayofyear': np.arange(1, 5), 'hour': np.arange(4) * 6, 'quantile': np.array(LEVELS), 'latitude': coords['latitude'],
      'longitude': coords['longitude']})})
  torch.cuda.synchronize()
  return pred, targ, climatology


def kernel_times(ctx, lines, clock_mhz):
  import torch  # pylint: disable=g-import-not-at-top
  lines.append(f'(a) kernel time, {REPS} launches each between event pairs, medians; floors: unique bytes per point / {HBM_TBS:.0f} TB/s and '
               f'(NINSTR(M) + {MEMBER_INSTRUCTIONS} x M) vector instructions per point / ({CUS} CUs x {LANES} lanes x {clock_mhz:.0f} MHz)')
  lazy.FUSED_INTERVALS = True
  for m, nt in SHAPES:
    pred, targ, climatology = _inputs(1, m, nt, torch.float32)
    npoint = nt * GRID[0] * GRID[1]
    instr = NETWORK[padded(m)] + MEMBER_INSTRUCTIONS * m
    floor_valu = float(npoint) * instr / (CUS * LANES * clock_mhz * 1e6) * 1e3
    lines.append(f'  f32{[m, nt] + list(GRID)}: {instr} instructions per point, VALU floor {floor_valu:.3f} ms')
    for which, stats in (('Covered alone', {'c': categorical.Covered('number', LEVELS)}),
                         ('three lanes  ', categorical.Opportunism('number', climatology, True, True, True).statistics)):
      engine.clear_caches()
      lazy_stats = [s.compute(pred, targ)['v'] for s in stats.values()]
      grp = lazy_stats[0]._group  # pylint: disable=protected-access
      assert all(isinstance(s, lazy.LazyInterval) and s._group is grp for s in lazy_stats)  # pylint: disable=protected-access
      nbytes = (m + 1 + (2 if len(lazy_stats) > 1 else 0)) * npoint * 4
      floor_hbm = nbytes / (HBM_TBS * 1e12) * 1e3
      for what, reduce_dims in (('x summed', DIMS), ('x kept  ', DIMS[:2])):
        with engine.synchronous_results():
          grp.reduce(reduce_dims, None, (), use_mask=False, skipna=False)  # plans, uploads
          engine.S1_EVENT_LOG = log = []
          for _ in range(REPS):
            values, _, _ = grp.reduce(reduce_dims, None, (), use_mask=False, skipna=False)
          engine.S1_EVENT_LOG = None
        assert len(log) == REPS and all(e['kind'] == 'ivl' for e in log)
        ms = float(np.median([e['ms'] for e in log]))
        fractions = np.asarray(values, np.float64).reshape(len(lazy_stats), -1).sum(axis=1) / npoint
        lines.append(f'    {which} {what}: {ms:8.3f} ms  = {ms / floor_hbm:5.2f} x the HBM floor {floor_hbm:.3f} ms ({nbytes / ms / 1e9:5.3f} TB/s), '
                     f'{ms / floor_valu:5.2f} x the VALU floor   grid={log[0]["grid"]} block={min(log[0]["block"], 128)} '
                     f'fractions {np.array2string(fractions, precision=4)}')
    del pred, targ, climatology, lazy_stats, grp
    engine.clear_caches()
    torch.cuda.empty_cache()


def _evaluate(ctx, metric, agg, pred, targ):
  import torch  # pylint: disable=g-import-not-at-top
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  stats = metrics_base.compute_unique_statistics_for_all_metrics({'o': metric}, pred, targ)
  t1 = time.perf_counter()
  state = agg.aggregate_statistics(stats)
  ctx.synchronize()
  torch.cuda.synchronize()
  t2 = time.perf_counter()
  score = float(np.asarray(state.metric_values({'o': metric})['o.v'].values).ravel()[0])
  return (t1 - t0) * 1e3, (t2 - t1) * 1e3, score


def end_to_end(ctx, lines):
  import torch  # pylint: disable=g-import-not-at-top
  failures = []
  agg = aggregation.Aggregator(reduce_dims=list(DIMS))
  lines.append('(b) end to end, Opportunism(True, True, True) of device-resident tensors, every dim reduced: host wall time of the statistics + '
               'aggregate_statistics up to a synchronise, new tensors every repetition')
  for m, nt in SHAPES:
    lines.append(f'  f32{[m, nt] + list(GRID)}')
    medians, scores = {}, {}
    for fused, reps in ((True, 4), (False, 2)):
      lazy.FUSED_INTERVALS = fused
      times, error = [], None
      for rep in range(reps + 1):
        pred, targ, climatology = _inputs(100 + reps - rep, m, nt, torch.float32)  # (the last repetition scores the same fields on both routes)
        try:
          st, ag, score = _evaluate(ctx, categorical.Opportunism('number', climatology, True, True, True), agg, pred, targ)
        except RuntimeError as e:  # (torch.quantile refuses inputs beyond a size of its own: the host route has no result there)
          if fused:
            raise
          error = str(e).splitlines()[0]
        if rep and error is None:  # (the first repetition builds plans and weight tables)
          times.append((st, ag))
        del pred, targ, climatology
        engine.clear_caches()
        torch.cuda.empty_cache()
        if error is not None:
          break
      if error is not None:
        lines.append(f'    host route (WBX_FUSED_INTERVALS=0)  : raises RuntimeError: {error}')
        continue
      st, ag = np.median([a for a, _ in times]), np.median([b for _, b in times])
      medians[fused], scores[fused] = st + ag, score
      name = 'fused (wbx_ens_interval_partial)' if fused else 'host route (WBX_FUSED_INTERVALS=0)'
      lines.append(f'    {name:36s}: statistics {st:9.2f} ms   aggregate_statistics {ag:9.2f} ms   total {st + ag:9.2f} ms   ({reps} repetitions, medians)'
                   f'   score {score:.15f}')
    if False not in medians:
      continue
    # float32 payloads: the host route interpolates in float32, so single indicators may differ: reported, not gated
    lines.append(f'    |score fused - score host route| = {abs(scores[True] - scores[False]):.3e};  host route / fused = {medians[False] / medians[True]:.1f} x '
                 '(required: not slower)')
    if not medians[False] >= medians[True]:
      failures.append(f'M = {m}, {nt} fields: the fused route is slower than the host route')
  small = (3, 24, 36)
  scores = {}
  for fused in (True, False):
    lazy.FUSED_INTERVALS = fused
    pred, targ, climatology = _inputs(7, 11, small[0], torch.float64, small[1:])
    scores[fused] = _evaluate(ctx, categorical.Opportunism('number', climatology, True, True, True, (0.1, 0.9), (0.1, 0.9), (0.1, 0.9)),
                              agg, pred, targ)[2]
    engine.clear_caches()
  lazy.FUSED_INTERVALS = True
  rel = abs(scores[True] - scores[False]) / abs(scores[False])
  lines.append(f'(c) float64 f64{[11] + list(small)} (g = 0 at both levels): host route score {scores[False]!r}, fused {scores[True]!r}, '
               f'relative difference {rel:.3e} (bound 1e-12)')
  if not rel <= 1e-12:
    failures.append('the float64 scores of the two routes differ by more than 1e-12 of the score')
  return failures


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'intervals_kbench.txt'))
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-e2e', action='store_true')
  args = ap.parse_args()
  ctx = _hip.default_context()
  clock = ctx.clock_probe()
  lines = [f'tools/bench_intervals.py on {ctx.device_name()}; wbx_clock_probe {clock:.0f} MHz before']
  if not args.skip_kernel:
    kernel_times(ctx, lines, clock)
  failures = [] if args.skip_e2e else end_to_end(ctx, lines)
  lines.append(f'wbx_clock_probe {ctx.clock_probe():.0f} MHz after')
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(args.out, 'w') as f:
    f.write(text)
  if failures:  # (the figures are on file either way)
    sys.exit('; '.join(failures))


if __name__ == '__main__':
  main()
