"""Thresholded contingency tables (wbx_contingency_partial): kernel time against the deterministic kernel on the same plan and
inputs, and one public-API chunk end to end against the host route.

(a) f32[40, 721, 1440] predictions and targets, every dim reduced: wbx_contingency_partial at K = 1, 4, 8, 16 thresholds,
    alternating launch by launch with wbx_det_partial(WBX_DET3) -- the same 8 bytes per point -- 20 timed launches each between
    wbx_mark pairs, medians.
(b) CSI at 5 thresholds of f32[20, 721, 1440] HOST arrays through the public API: host wall time around
    Aggregator.aggregate_statistics up to a synchronise, fused route against WBX_FUSED_CONTINGENCY=0 (new arrays every
    repetition, so both routes pay their uploads).

Usage: python tools/bench_contingency.py [--out profiles/contingency_kbench.txt] [--skip-e2e]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from weatherbenchx_amd import _hip, aggregation, engine, lazy, planner
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as mb, categorical, wrappers

DIMS = ('lead_time', 'latitude', 'longitude')
REPS = 20


def kernel_times(ctx, lines):
  shape = (40, 721, 1440)
  rng = np.random.default_rng(0)
  p = rng.gamma(2.0, size=shape).astype(np.float32)
  t = rng.gamma(2.0, size=shape).astype(np.float32)
  sizes = dict(zip(DIMS, shape))
  lay = planner.layout_of(p, DIMS)
  lay = planner.InputLayout(strides=dict(lay.strides), itemsize=4, base_alignment=256)
  plan = planner.build_s1_plan(DIMS, sizes, [lay, lay, None, None], DIMS, wdep_dims=set(), flags=0, allow_vec4=True)
  dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
  dp, dt = ctx.upload(p), ctx.upload(t)
  nbytes = 2 * p.nbytes
  lines.append(f'(a) kernel time, f32{list(shape)} p and t, all dims reduced: plan nkey={plan.nkey} nchunk={plan.nchunk} '
               f'depth_chunk={plan.depth_chunk} block={plan.block_threads} vec={plan.vec}; {REPS} launches each, alternating, medians')
  ptr = lambda b: C.c_void_p(b.ptr)
  for k in (1, 4, 8, 16):
    thr = ctx.upload(np.quantile(p[0, ::40, ::40].astype(np.float64), np.linspace(0.1, 0.95, k)))
    out_c = ctx.alloc(int(np.prod(plan.partial_shape(_hip.CONT_CELLS * k))) * 8)
    out_d = ctx.alloc(int(np.prod(plan.partial_shape(3))) * 8)

    def cont():
      _hip.check(ctx.lib.wbx_contingency_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, k, ptr(dp), ptr(dt), ptr(thr), None,
                                                 ptr(out_c)), 'wbx_contingency_partial')

    def det():
      _hip.check(ctx.lib.wbx_det_partial(ctx.handle, C.byref(dplan.struct), _hip.DET3, _hip.F32, ptr(dp), ptr(dt), None, None,
                                         ptr(out_d)), 'wbx_det_partial')
    for _ in range(3):
      cont()
      det()
    ctx.synchronize()
    ctx.marks_reset()
    marks = []
    for _ in range(REPS):
      m0 = ctx.mark()
      cont()
      m1 = ctx.mark()
      det()
      m2 = ctx.mark()
      marks.append((m0, m1, m2))
    ctx.synchronize()
    tc = np.median([ctx.mark_elapsed(a, b) for a, b, _ in marks])
    td = np.median([ctx.mark_elapsed(b, c) for _, b, c in marks])
    ctx.marks_reset()
    # the table of the first threshold adds up to the number of points
    got = ctx.download(out_c.ptr, plan.partial_shape(_hip.CONT_CELLS * k), np.float64).reshape(-1, _hip.CONT_CELLS * k)
    total = got.sum(axis=0).reshape(_hip.CONT_CELLS, k).sum(axis=0)
    assert (total == p.size).all(), total
    lines.append(f'    K={k:2d}: contingency {tc:7.4f} ms ({nbytes / tc / 1e9:6.3f} TB/s)   DET3 {td:7.4f} ms ({nbytes / td / 1e9:6.3f} TB/s)'
                 f'   ratio {tc / td:5.3f}')


def end_to_end(ctx, lines):
  shape = (20, 721, 1440)
  rng = np.random.default_rng(1)
  p = rng.gamma(2.0, size=shape).astype(np.float32)
  t = rng.gamma(2.0, size=shape).astype(np.float32)
  coords = {'lead_time': (np.arange(shape[0]) * 12).astype('timedelta64[h]').astype('timedelta64[ns]'),
            'latitude': np.linspace(-90, 90, shape[1]), 'longitude': np.linspace(0, 360, shape[2], endpoint=False)}
  thresholds = [0.5, 1.0, 2.0, 3.0, 5.0]
  metrics = {'csi': wrappers.WrappedMetric(categorical.CSI(), [wrappers.ContinuousToBinary('both', thresholds, 'threshold')])}
  agg = aggregation.Aggregator(reduce_dims=['latitude', 'longitude'])
  lines.append(f'(b) end to end, CSI at {len(thresholds)} thresholds of host f32{list(shape)} arrays, reduce (latitude, longitude): host wall '
               'time around aggregate_statistics up to a synchronise, new arrays every repetition')
  results = {}
  for fused, reps in ((True, 5), (False, 2)):
    lazy.FUSED_CONTINGENCY = fused
    times = []
    for rep in range(reps + 1):
      pred = {'v': xr.DataArray(p, dims=DIMS, coords=coords)}
      targ = {'v': xr.DataArray(t, dims=DIMS, coords=coords)}
      t0 = time.perf_counter()
      stats = mb.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
      t1 = time.perf_counter()
      state = agg.aggregate_statistics(stats)
      ctx.synchronize()
      t2 = time.perf_counter()
      if rep:  # (the first repetition builds plans and weight tables)
        times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    results[fused] = np.asarray(state.metric_values(metrics)['csi.v'].values)
    st, ag = np.median([a for a, _ in times]), np.median([b for _, b in times])
    lines.append(f'    {"fused (wbx_contingency_partial)" if fused else "host route (WBX_FUSED_CONTINGENCY=0)":38s}: statistics {st:9.2f} ms   '
                 f'aggregate_statistics {ag:9.2f} ms   ({reps} repetitions, medians)')
  lazy.FUSED_CONTINGENCY = True
  err = float(np.nanmax(np.abs(results[True] - results[False])))
  lines.append(f'    largest |CSI fused - CSI host route| = {err:.3e}')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'contingency_kbench.txt'))
  ap.add_argument('--skip-e2e', action='store_true')
  args = ap.parse_args()
  ctx = _hip.default_context()
  lines = [f'tools/bench_contingency.py on {ctx.device_name()}; wbx_clock_probe {ctx.clock_probe():.0f} MHz before']
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
