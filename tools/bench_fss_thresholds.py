"""The FSS terms of thresholded continuous fields in one sweep per block of thresholds (wbx_fss_threshold_partial): kernel time against K
launches of wbx_fss_partial on pre-binarised fields, and FSS behind ContinuousToBinary through the public API end to end with the
switch on and off.

(a) Continuous f32[40, 721, 1440] predictions and targets generated on the device, K = 1, 4 and 8 thresholds, n = 3, 21 and 101, x
    summed (every dim reduced).  The yardstick is K launches of wbx_fss_partial on the K pairs of pre-binarised float32 fields under
    the same plan: the kernel cost of the route before the entry existed WITHOUT its host binarisation.  The fused call and the K
    launches alternate in one process, each side between one HIP event pair, medians of REPS.
    Gate: at K >= 2 the fused call is no slower than the K launches beyond the box spread README states (8 %); at K = 1 the ratio
    is recorded.  The tool exits 1 where the gate fails.
(b) One chunk f32[20, 721, 1440] (time, latitude, longitude) of device-resident continuous tensors through the public API:
    FSS([1, 3, 5, 11, 21]) behind ContinuousToBinary('both', five thresholds), GridAreaWeighting, every dim reduced.  Host wall time
    from compute_unique_statistics_for_all_metrics through Aggregator.aggregate_statistics up to a synchronise, the fused route against
    WBX_FUSED_FSS_THRESHOLDS=0 (the route before the entry existed) on the same payload in the same process, the first call of either
    route dropped, and the two scores.  Gate: the fused route is faster by more than the box spread.

Usage: python tools/bench_fss_thresholds.py [--out profiles/fss_thresholds_kbench.txt] [--skip-kernel] [--skip-e2e]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from weatherbenchx_amd import _hip, aggregation, engine, lazy, planner, weighting
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as metrics_base
from weatherbenchx_amd.metrics import spatial, wrappers

NT, GRID = 40, (721, 1440)
REPS = 10
SPREAD = 0.08  # README: the box spread of a median
DIMS = ('time', 'latitude', 'longitude')
SIZES_KERNEL = (3, 21, 101)
KS = (1, 4, 8)
THRESHOLDS = [0.5, 0.45, 0.55, 0.4, 0.6, 0.35, 0.65, 0.3]
SIZES_E2E = [1, 3, 5, 11, 21]
THRESHOLDS_E2E = [0.4, 0.45, 0.5, 0.55, 0.6]
THR = 'threshold'


def _fields(seed, shape):
  """Continuous fields with blobs a few points wide, in [0, 1]: a smooth field, and a noisy copy of it."""
  import torch  # pylint: disable=g-import-not-at-top
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  base = torch.rand(shape, generator=g, device='cuda', dtype=torch.float32)
  base = torch.nn.functional.avg_pool2d(base.reshape((-1, 1) + shape[-2:]), 5, stride=1, padding=2).reshape(shape)
  noise = torch.rand(shape, generator=g, device='cuda', dtype=torch.float32)
  return (base + 0.05 * (noise - 0.5)).contiguous(), base.contiguous()


def kernel_times(ctx, lines):
  import torch  # pylint: disable=g-import-not-at-top
  p, t = _fields(1, (NT,) + GRID)
  binarised = [((p > a).to(torch.float32), (t > a).to(torch.float32)) for a in THRESHOLDS[:max(KS)]]
  torch.cuda.synchronize()
  sizes = dict(zip(DIMS, (NT,) + GRID))
  lay = planner.layout_of
  ptr = lambda x: C.c_void_p(int(x.data_ptr()))
  lines.append(f'(a) kernel time, continuous f32{[NT] + list(GRID)}, x summed: one call of wbx_fss_threshold_partial against K launches of '
               f'wbx_fss_partial on pre-binarised fields, in turns, each side between one event pair, medians of {REPS}')
  fp = planner.build_fss_plan(DIMS, sizes, [lay(p, DIMS), lay(t, DIMS), None], DIMS, wrap_longitude=True)
  dplan = engine._FssPlanOnDevice(ctx, fp)  # pylint: disable=protected-access
  out_f = ctx.alloc(int(np.prod(fp.s1.partial_shape(3 * max(KS)), dtype=np.int64)) * 8)
  out_b = ctx.alloc(int(np.prod(fp.s1.partial_shape(3), dtype=np.int64)) * 8)
  thr = ctx.upload(np.asarray(THRESHOLDS, np.float64))
  ok = True
  for n in SIZES_KERNEL:
    for k in KS:
      def fused():
        return ctx.lib.wbx_fss_threshold_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, n, k, C.c_void_p(thr.ptr), ptr(p), ptr(t), None,
                                                 C.c_void_p(out_f.ptr))

      def separate():
        for pb, tb in binarised[:k]:
          rc = ctx.lib.wbx_fss_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, n, ptr(pb), ptr(tb), None, C.c_void_p(out_b.ptr))
          if rc:
            return rc
        return 0
      calls = {'fused': fused, 'separate': separate}
      times = {name: [] for name in calls}
      for rep in range(REPS + 2):
        for name, call in calls.items():
          ctx.timer_start()
          _hip.check(call(), name)
          ms = ctx.timer_stop()
          if rep >= 2:  # (the first two turns warm the code objects and the cache)
            times[name].append(ms)
      med = {name: float(np.median(v)) for name, v in times.items()}
      ratio = med['fused'] / med['separate']
      verdict = 'recorded' if k == 1 else ('ok' if ratio <= 1 + SPREAD else 'SLOWER')
      ok = ok and verdict != 'SLOWER'
      band = _hip.fss_band_rows(fp.nkey, fp.nchunk, fp.nlat, n)
      lines.append(f'    n={n:3d} K={k}: wbx_fss_threshold_partial {med["fused"]:7.3f} ms   {k} x wbx_fss_partial {med["separate"]:7.3f} ms   '
                   f'fused / separate = {ratio:.2f} ({verdict})   band={band} rows chunks={fp.nchunk}')
  del p, t, binarised
  torch.cuda.empty_cache()
  return ok


def _chunk(seed):
  import torch  # pylint: disable=g-import-not-at-top
  shape = (20,) + GRID
  p, t = _fields(seed, shape)
  lat, lon = np.linspace(-90, 90, GRID[0]), np.linspace(0, 360, GRID[1], endpoint=False)
  cs = {'time': np.arange(20), 'latitude': lat, 'longitude': lon}
  torch.cuda.synchronize()
  return ({'tp': xr.DataArray(p, dims=DIMS, coords=cs, name='tp')},
          {'tp': xr.DataArray(t, dims=DIMS, coords=cs, name='tp')})


def end_to_end(ctx, lines):
  import torch  # pylint: disable=g-import-not-at-top
  lines.append(f'(b) end to end, one chunk f32[20, 721, 1440] of device-resident continuous tensors, FSS({SIZES_E2E}) behind '
               f"ContinuousToBinary('both', {THRESHOLDS_E2E}), GridAreaWeighting, every dim reduced: host wall time of the statistics + "
               'aggregate_statistics up to a synchronise')
  pred, targ = _chunk(11)
  scores, medians = {}, {}
  for fused, reps in ((True, 4), (False, 2)):
    lazy.FUSED_FSS_THRESHOLDS = fused
    metrics = {'fss': wrappers.WrappedMetric(spatial.FSS(SIZES_E2E, wrap_longitude=True),
                                             [wrappers.ContinuousToBinary('both', THRESHOLDS_E2E, THR)])}
    times = []
    for rep in range(reps + 1):
      agg = aggregation.Aggregator(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()])
      fresh = lambda d: {'tp': xr.DataArray(d['tp'].data, dims=d['tp'].dims, coords=dict(d['tp'].coords), name='tp')}  # (no cached sums)
      a, b = fresh(pred), fresh(targ)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      stats = metrics_base.compute_unique_statistics_for_all_metrics(metrics, a, b)
      t1 = time.perf_counter()
      state = agg.aggregate_statistics(stats)
      ctx.synchronize()
      torch.cuda.synchronize()
      t2 = time.perf_counter()
      if rep:  # (the first call of either route builds plans and weight tables: dropped)
        times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
      scores[fused] = np.asarray(state.metric_values(metrics)['fss.tp'].values, np.float64)
      del stats, state, a, b
      engine.clear_caches()
      torch.cuda.empty_cache()
    st, ag = np.median([x for x, _ in times]), np.median([y for _, y in times])
    medians[fused] = st + ag
    name = 'fused (wbx_fss_threshold_partial)' if fused else 'WBX_FUSED_FSS_THRESHOLDS=0'
    lines.append(f'    {name:34s}: statistics {st:9.2f} ms   aggregate_statistics {ag:9.2f} ms   total {st + ag:9.2f} ms   '
                 f'({reps} repetitions, medians)')
    for row in scores[fused]:
      lines.append(f'    {"":34s}  scores {" ".join(f"{v:.12f}" for v in row)}')
  lazy.FUSED_FSS_THRESHOLDS = True
  rel = float(np.max(np.abs(scores[True] - scores[False]) / np.abs(scores[False])))
  ratio = medians[False] / medians[True]
  lines.append(f'    switch off / fused = {ratio:.1f} x; largest relative difference of the scores {rel:.3e}')
  return ratio > 1 + SPREAD


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'fss_thresholds_kbench.txt'))
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-e2e', action='store_true')
  args = ap.parse_args()
  ctx = _hip.default_context()
  lines = [f'tools/bench_fss_thresholds.py on {ctx.device_name()}; wbx_clock_probe {ctx.clock_probe():.0f} MHz before']
  ok = True
  if not args.skip_kernel:
    ok = kernel_times(ctx, lines) and ok
  if not args.skip_e2e:
    ok = end_to_end(ctx, lines) and ok
  lines.append(f'wbx_clock_probe {ctx.clock_probe():.0f} MHz after')
  lines.append('gate: ' + ('passed' if ok else 'FAILED'))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(args.out, 'w') as f:
    f.write(text)
  return 0 if ok else 1


if __name__ == '__main__':
  sys.exit(main())
