"""The three FSS terms in one sweep (wbx_fss_partial): kernel time against wbx_det_partial(WBX_DET3) over the same p and t, and FSS
through the public API end to end against the host route.

(a) f32[40, 721, 1440] 0 / 1 predictions and targets generated on the device, n = 3, 21 and 101, x summed (every dim reduced) and x
    kept ((time, latitude) reduced).  The launches of wbx_fss_partial alternate with wbx_det_partial(WBX_DET3) over the same p and t
    -- the yardstick that streams the same 8 B per point once -- each launch between a HIP event pair, medians of REPS.  The stencil
    reads every row twice (entering and leaving the window; the second time from cache where it still is) plus a halo of n - 1 rows
    per band of B: the band and the number of blocks are printed with the times.
(b) One chunk f32[20, 721, 1440] (time, latitude, longitude) of device-resident 0 / 1 tensors through the public API:
    FSS([1, 3, 5, 11, 21]), GridAreaWeighting, masked=True, every dim reduced.  The inputs carry no `mask` coordinate: the per-size
    erosion of one (spatial.get_fss_mask) is host work that both routes do alike.  Host wall time from
    compute_unique_statistics_for_all_metrics through Aggregator.aggregate_statistics up to a synchronise, the fused route against
    WBX_FUSED_FSS=0 on the same payload in the same process, the first call of either route dropped, and the two scores.

Usage: python tools/bench_fss.py [--out profiles/fss_kbench.txt] [--skip-kernel] [--skip-e2e]"""
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
from weatherbenchx_amd.metrics import spatial

NT, GRID = 40, (721, 1440)
REPS = 10
HBM_TBS = 8.0
DIMS = ('time', 'latitude', 'longitude')
SIZES_KERNEL = (3, 21, 101)
SIZES_E2E = [1, 3, 5, 11, 21]


def _fields(seed, shape):
  """0 / 1 fields with blobs a few points wide: a smooth field thresholded, and a noisy copy of it."""
  import torch  # pylint: disable=g-import-not-at-top
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  base = torch.rand(shape, generator=g, device='cuda', dtype=torch.float32)
  base = torch.nn.functional.avg_pool2d(base.reshape((-1, 1) + shape[-2:]), 5, stride=1, padding=2).reshape(shape)
  noise = torch.rand(shape, generator=g, device='cuda', dtype=torch.float32)
  return (base + 0.05 * (noise - 0.5) > 0.52).to(torch.float32), (base > 0.52).to(torch.float32)


def kernel_times(ctx, lines):
  import torch  # pylint: disable=g-import-not-at-top
  p, t = _fields(1, (NT,) + GRID)
  torch.cuda.synchronize()
  sizes = dict(zip(DIMS, (NT,) + GRID))
  lay = planner.layout_of
  npoint = NT * GRID[0] * GRID[1]
  floor = 8.0 * npoint / (HBM_TBS * 1e12) * 1e3
  ptr = lambda x: C.c_void_p(int(x.data_ptr()))
  lines.append(f'(a) kernel time, f32{[NT] + list(GRID)} 0 / 1 fields, {REPS} launches of each entry point in turns, each between an event pair, '
               f'medians; 8 B per point / {HBM_TBS:.0f} TB/s = {floor:.3f} ms')
  for what, reduce_dims in (('x summed', DIMS), ('x kept  ', DIMS[:2])):
    fp = planner.build_fss_plan(DIMS, sizes, [lay(p, DIMS), lay(t, DIMS), None], reduce_dims, wrap_longitude=True)
    dfss = engine._FssPlanOnDevice(ctx, fp)  # pylint: disable=protected-access
    plan = planner.build_s1_plan(DIMS, sizes, [lay(p, DIMS), lay(t, DIMS), None, None], reduce_dims, wdep_dims=set(), flags=0)
    ddet = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
    out_f = ctx.alloc(int(np.prod(fp.s1.partial_shape(3), dtype=np.int64)) * 8)
    out_d = ctx.alloc(int(np.prod(plan.partial_shape(3), dtype=np.int64)) * 8)
    det = lambda: ctx.lib.wbx_det_partial(ctx.handle, C.byref(ddet.struct), _hip.DET3, _hip.F32, ptr(p), ptr(t), None, None, C.c_void_p(out_d.ptr))
    for n in SIZES_KERNEL:
      fss = lambda: ctx.lib.wbx_fss_partial(ctx.handle, C.byref(dfss.struct), _hip.F32, n, ptr(p), ptr(t), None, C.c_void_p(out_f.ptr))
      calls = {'wbx_fss_partial': fss, 'wbx_det_partial(DET3)': det}
      times = {k: [] for k in calls}
      for rep in range(REPS + 2):
        for name, call in calls.items():
          ctx.timer_start()
          _hip.check(call(), name)
          ms = ctx.timer_stop()
          if rep >= 2:  # (the first two turns warm the code objects and the cache)
            times[name].append(ms)
      med = {k: float(np.median(v)) for k, v in times.items()}
      band = _hip.fss_band_rows(fp.nkey, fp.nchunk, fp.nlat, n)
      blocks = fp.nkey * fp.nchunk * -(-fp.nlat // band)
      lines.append(f'    {what} n={n:3d} wbx_fss_partial       : {med["wbx_fss_partial"]:7.3f} ms = {100 * floor / med["wbx_fss_partial"]:4.1f} % of the peak on '
                   f'8 B/point   band={band} rows (halo {n - 1}) blocks={blocks} chunks={fp.nchunk}')
      lines.append(f'    {what} n={n:3d} wbx_det_partial(DET3) : {med["wbx_det_partial(DET3)"]:7.3f} ms = {100 * floor / med["wbx_det_partial(DET3)"]:4.1f} % of the '
                   f'peak   keys x chunks={plan.nkey * plan.nchunk} vec={plan.vec}')
      lines.append(f'    {what} n={n:3d} wbx_fss_partial / wbx_det_partial(DET3) = {med["wbx_fss_partial"] / med["wbx_det_partial(DET3)"]:.2f}')
  del p, t
  torch.cuda.empty_cache()


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
  lines.append(f'(b) end to end, one chunk f32[20, 721, 1440] of device-resident tensors, FSS({SIZES_E2E}), GridAreaWeighting, masked=True, every dim '
               'reduced; the inputs carry NO `mask` coordinate, so no mask is in play on either route (the launches run without WBX_FLAG_MASKED and without a '
               'count lane): host wall time of the statistics + aggregate_statistics up to a synchronise')
  pred, targ = _chunk(11)
  scores, medians = {}, {}
  for fused, reps in ((True, 4), (False, 2)):
    lazy.FUSED_FSS = fused
    metrics = {'fss': spatial.FSS(SIZES_E2E, wrap_longitude=True)}
    times = []
    for rep in range(reps + 1):
      agg = aggregation.Aggregator(reduce_dims=list(DIMS), weigh_by=[weighting.GridAreaWeighting()], masked=True)
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
    name = 'fused (wbx_fss_partial)' if fused else 'host route (WBX_FUSED_FSS=0)'
    lines.append(f'    {name:30s}: statistics {st:9.2f} ms   aggregate_statistics {ag:9.2f} ms   total {st + ag:9.2f} ms   '
                 f'({reps} repetitions, medians)')
    lines.append(f'    {"":30s}  scores {" ".join(f"{v:.12f}" for v in scores[fused])}')
  lazy.FUSED_FSS = True
  rel = float(np.max(np.abs(scores[True] - scores[False]) / np.abs(scores[False])))
  lines.append(f'    host route / fused = {medians[False] / medians[True]:.1f} x; largest relative difference of the scores {rel:.3e}')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'fss_kbench.txt'))
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-e2e', action='store_true')
  args = ap.parse_args()
  ctx = _hip.default_context()
  lines = [f'tools/bench_fss.py on {ctx.device_name()}; wbx_clock_probe {ctx.clock_probe():.0f} MHz before']
  if not args.skip_kernel:
    kernel_times(ctx, lines)
  if not args.skip_e2e:
    end_to_end(ctx, lines)
  lines.append(f'wbx_clock_probe {ctx.clock_probe():.0f} MHz after')
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
