"""Contingency tables at threshold fields (wbx_contingency_field_partial): kernel time against the list kernel on the same plan and
inputs, and one public-API chunk end to end against the host route.

(a) f32[40, 721, 1440] predictions and targets, a float32 and a float64 field [K, 721, 1440] (it does not vary along the summed time
    axis), x summed (every dim reduced) and x kept (longitude kept): wbx_contingency_field_partial at K = 1, 4, 8, 16, alternating
    launch by launch with wbx_contingency_partial at the same K on the same plan -- the kernel that existed before, 8 bytes per
    point -- 10 timed launches each between wbx_mark pairs, medians.  Beside the time ratio: the ratio of algorithmic bytes per
    point, (8 + w K) / 8 for a field of w-byte elements were it read once per point (the bound from above: its re-reads along the
    time axis should come from cache), and (8 + w K / 40) / 8 were it read once (the bound from below).
(b) CSI at a 5-threshold percentile field of f32[20, 721, 1440] HOST arrays through the public API: host wall time around
    compute + Aggregator.aggregate_statistics up to a synchronise, fused route against WBX_FUSED_CONTINGENCY_FIELD=0 in the same
    process (new arrays every repetition, so both routes pay their uploads; the field is uploaded once).  The results must be
    identical to the last bit and the fused route not slower: the tool exits with status 1 otherwise.

Usage: python tools/bench_contingency_field.py [--out profiles/contingency_field_kbench.txt] [--skip-e2e]"""
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
REPS = 10


def kernel_times(ctx, lines):
  shape = (40, 721, 1440)
  rng = np.random.default_rng(0)
  p = rng.gamma(2.0, size=shape).astype(np.float32)
  t = rng.gamma(2.0, size=shape).astype(np.float32)
  levels = np.sort(rng.gamma(2.0, size=(16,) + shape[1:]), axis=0)  # [K, latitude, longitude] float64, increasing along K
  sizes = dict(zip(DIMS, shape))
  lay = planner.layout_of(p, DIMS)
  lay = planner.InputLayout(strides=dict(lay.strides), itemsize=4, base_alignment=256)
  dp, dt = ctx.upload(p), ctx.upload(t)
  ptr = lambda b: C.c_void_p(b.ptr)
  thr_stride = shape[1] * shape[2]
  for x_kept in (False, True):
    for thr_dtype, code in ((np.float32, _hip.F32), (np.float64, _hip.F64)):
      w = np.dtype(thr_dtype).itemsize
      lay_c = planner.InputLayout(strides={'latitude': shape[2], 'longitude': 1}, itemsize=w, base_alignment=256)
      reduce_dims = DIMS[:2] if x_kept else DIMS
      build = lambda vec4: planner.build_s1_plan(DIMS, sizes, [lay, lay, lay_c, None], reduce_dims, wdep_dims=set(), flags=0, allow_vec4=vec4)
      plan = build(True)
      if plan.plane_rows > 0:  # (as engine._planned_inner: 16-byte loads yes, plane mode no)
        plan = build(False)
      dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
      dc = ctx.upload(levels.astype(thr_dtype))
      lines.append(f'(a) kernel time, f32{list(shape)} p and t, {np.dtype(thr_dtype).name} field [K, 721, 1440], x {"kept" if x_kept else "summed"}: '
                   f'plan nkey={plan.nkey} nchunk={plan.nchunk} depth_chunk={plan.depth_chunk} block={plan.block_threads} vec={plan.vec}; '
                   f'{REPS} launches each, alternating, medians')
      for k in (1, 4, 8, 16):
        # the list kernel's thresholds: the field's means, so that both kernels count comparable shares
        thr = ctx.upload(levels[:k].mean(axis=(1, 2)))
        n_out = int(np.prod(plan.partial_shape(_hip.CONT_CELLS * k)))
        out_f, out_l = ctx.alloc(n_out * 8), ctx.alloc(n_out * 8)

        def field():
          _hip.check(ctx.lib.wbx_contingency_field_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, code, k, thr_stride, 0, ptr(dp), ptr(dt),
                                                           ptr(dc), None, ptr(out_f)), 'wbx_contingency_field_partial')

        def listed():
          _hip.check(ctx.lib.wbx_contingency_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, k, ptr(dp), ptr(dt), ptr(thr), None,
                                                     ptr(out_l)), 'wbx_contingency_partial')
        for _ in range(3):
          field()
          listed()
        ctx.synchronize()
        ctx.marks_reset()
        marks = []
        for _ in range(REPS):
          m0 = ctx.mark()
          field()
          m1 = ctx.mark()
          listed()
          m2 = ctx.mark()
          marks.append((m0, m1, m2))
        ctx.synchronize()
        tf = np.median([ctx.mark_elapsed(a, b) for a, b, _ in marks])
        tl = np.median([ctx.mark_elapsed(b, c) for _, b, c in marks])
        ctx.marks_reset()
        # every threshold's table adds up to the number of points
        got = ctx.download(out_f.ptr, plan.partial_shape(_hip.CONT_CELLS * k), np.float64)
        lanes = np.moveaxis(got, -2, 0).reshape(_hip.CONT_CELLS * k, -1).sum(axis=1)  # ([..., lane, j])
        total = lanes.reshape(_hip.CONT_CELLS, k).sum(axis=0)
        assert (total == p.size).all(), total
        lines.append(f'    K={k:2d}: field {tf:7.4f} ms   list {tl:7.4f} ms   time ratio {tf / tl:5.3f}   bytes per point (8 + {w} K) / 8 = '
                     f'{(8 + w * k) / 8:5.2f} if the field were read at every point, (8 + {w} K / 40) / 8 = {(8 + w * k / shape[0]) / 8:5.3f} read once')


def end_to_end(ctx, lines):
  shape = (20, 721, 1440)
  rng = np.random.default_rng(1)
  p = rng.gamma(2.0, size=shape).astype(np.float32)
  t = rng.gamma(2.0, size=shape).astype(np.float32)
  place = {'latitude': np.linspace(-90, 90, shape[1]), 'longitude': np.linspace(0, 360, shape[2], endpoint=False)}
  coords = dict(place, lead_time=(np.arange(shape[0]) * 12).astype('timedelta64[h]').astype('timedelta64[ns]'))
  q = np.array([50.0, 75.0, 90.0, 95.0, 99.0])
  levels = np.sort(rng.gamma(2.0, size=(len(q),) + shape[1:]), axis=0).astype(np.float32)
  field = xr.DataArray(levels, dims=('percentile',) + DIMS[1:], coords=dict(place, percentile=q))
  metrics = {'csi': wrappers.WrappedMetric(categorical.CSI(), [wrappers.ContinuousToBinary('both', xr.Dataset({'v': field}), 'percentile',
                                                                                          unique_name_suffix='climatology')])}
  agg = aggregation.Aggregator(reduce_dims=['latitude', 'longitude'])
  lines.append(f'(b) end to end, CSI at a {len(q)}-threshold float32 percentile field of host f32{list(shape)} arrays, reduce (latitude, longitude): '
               'host wall time around the statistics and aggregate_statistics up to a synchronise, new arrays every repetition')
  results, wall = {}, {}
  for fused, reps in ((True, 5), (False, 2)):
    lazy.FUSED_CONTINGENCY_FIELD = fused
    times = []
    for rep in range(reps + 1):
      pred = {'v': xr.DataArray(p, dims=DIMS, coords=coords, name='v')}
      targ = {'v': xr.DataArray(t, dims=DIMS, coords=coords, name='v')}
      t0 = time.perf_counter()
      stats = mb.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
      t1 = time.perf_counter()
      state = agg.aggregate_statistics(stats)
      ctx.synchronize()
      t2 = time.perf_counter()
      if rep:  # (the first repetition builds plans and weight tables and uploads the field)
        times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    results[fused] = np.asarray(state.metric_values(metrics)['csi.v'].values)
    st, ag = np.median([a for a, _ in times]), np.median([b for _, b in times])
    wall[fused] = st + ag
    lines.append(f'    {"fused (wbx_contingency_field_partial)" if fused else "host route (WBX_FUSED_CONTINGENCY_FIELD=0)":44s}: statistics {st:9.2f} ms   '
                 f'aggregate_statistics {ag:9.2f} ms   ({reps} repetitions, medians)')
  lazy.FUSED_CONTINGENCY_FIELD = True
  same = bool(np.array_equal(results[True], results[False], equal_nan=True))
  lines.append(f'    CSI identical to the last bit: {same};  host route / fused route = {wall[False] / wall[True]:.1f} x')
  return same and wall[True] <= wall[False]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'contingency_field_kbench.txt'))
  ap.add_argument('--skip-e2e', action='store_true')
  args = ap.parse_args()
  ctx = _hip.default_context()
  lines = [f'tools/bench_contingency_field.py on {ctx.device_name()}; wbx_clock_probe {ctx.clock_probe():.0f} MHz before']
  kernel_times(ctx, lines)
  ok = True
  if not args.skip_e2e:
    ok = end_to_end(ctx, lines)
  lines.append(f'wbx_clock_probe {ctx.clock_probe():.0f} MHz after')
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(args.out, 'w') as f:
    f.write(text)
  return 0 if ok else 1


if __name__ == '__main__':
  sys.exit(main())
