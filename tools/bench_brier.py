"""Brier-type errors of event probabilities (wbx_ens_brier_partial): kernel time against the ranked probability score kernel on the
same plan, inputs and thresholds, and one public-API chunk end to end against the host route.

(a) f32[51, 40, 721, 1440] predictions against f32[40, 721, 1440] targets (generated on the device), the member mean (denom = M):
    wbx_ens_brier_partial at K = 1, 4, 8, 16 thresholds, alternating launch by launch with wbx_ens_rps_partial (not fair) on the
    same plan and thresholds -- the same 208 bytes per point and the same compares, 1 lane written against 3 K -- 10 timed launches
    each between wbx_mark pairs, medians; every dim reduced (x summed) and longitude kept.  Recorded, not gated.
(b) MSE behind ContinuousToBinary('both') -> EnsembleMean('predictions') at 5 thresholds of f32[51, 1, 721, 1440] against
    f32[1, 721, 1440] HOST arrays through the public API: host wall time from Statistic.compute through
    Aggregator.aggregate_statistics up to a synchronise, fused route against WBX_FUSED_BRIER=0 (new arrays every repetition, so both
    routes pay their uploads).  `--e2e-route host` runs the host route alone and needs nothing of the fused one: the same file times
    a checkout from before the kernel existed.  Gated: host route / fused > 1.08 (the +-8 % box spread the README states); the
    process exits with status 1 where it is not.

Usage: python tools/bench_brier.py [--out profiles/brier_kbench.txt] [--skip-kernel] [--skip-e2e] [--e2e-route both|fused|host] [--e2e-grid NLAT NLON]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from weatherbenchx_amd import _hip, aggregation, engine, lazy, planner
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as mb, deterministic, wrappers

M = 51
REPS = 10
E2E_GATE = 1.08


def kernel_times(ctx, lines):
  import torch  # pylint: disable=g-import-not-at-top
  shape = (40, 721, 1440)
  dims = ('lead_time', 'latitude', 'longitude')
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  t = torch.randn(shape, generator=g, device='cuda')
  p = t[None] + torch.randn((M,) + shape, generator=g, device='cuda')
  torch.cuda.synchronize()
  npoint = int(np.prod(shape))
  nbytes = (M + 1) * npoint * 4
  sizes = dict(zip(dims, shape))
  strides = {'lead_time': shape[1] * shape[2], 'latitude': shape[2], 'longitude': 1}
  lay_p = planner.InputLayout(strides=dict(strides, number=npoint), itemsize=4, base_alignment=256)
  lay_t = planner.InputLayout(strides=dict(strides), itemsize=4, base_alignment=256)
  ptr = lambda v: C.c_void_p(int(v))
  lines.append(f'(a) kernel time, f32{[M] + list(shape)} against f32{list(shape)}, denom = M, {nbytes / 1e9:.2f} GB per launch; {REPS} launches each, '
               'alternating with wbx_ens_rps_partial (not fair) on the same plan and thresholds, medians')
  for what, reduce_dims in (('x summed (every dim reduced)', dims), ('x kept (longitude kept)', dims[:2])):
    plan = planner.build_s1_plan(dims, sizes, [lay_p, lay_t, None, None], reduce_dims, wdep_dims=set(), flags=0, allow_vec4=False)
    dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
    lines.append(f'  {what}: plan nkey={plan.nkey} nchunk={plan.nchunk} depth_chunk={plan.depth_chunk} nx={plan.nx} x_kept={plan.x_kept} '
                 f'block={plan.block_threads} vec={plan.vec}')
    out_b = ctx.alloc(int(np.prod(plan.partial_shape(_hip.BRIER_STATS * _hip.BRIER_MAX_THRESHOLDS))) * 8)
    out_r = ctx.alloc(int(np.prod(plan.partial_shape(1))) * 8)
    for k in (1, 4, 8, 16):
      thr = ctx.upload(np.linspace(-1.5, 1.5, k) if k > 1 else np.zeros(1))

      def brier():
        _hip.check(ctx.lib.wbx_ens_brier_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, M, npoint, M, k, ptr(thr.ptr),
                                                 ptr(p.data_ptr()), ptr(t.data_ptr()), None, ptr(out_b.ptr)), 'wbx_ens_brier_partial')

      def rps():
        _hip.check(ctx.lib.wbx_ens_rps_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, M, npoint, k, ptr(thr.ptr), ptr(thr.ptr), 1,
                                               ptr(p.data_ptr()), ptr(t.data_ptr()), None, ptr(out_r.ptr)), 'wbx_ens_rps_partial')
      for _ in range(2):
        brier()
        rps()
      ctx.synchronize()
      ctx.marks_reset()
      marks = []
      for _ in range(REPS):
        m0 = ctx.mark()
        brier()
        m1 = ctx.mark()
        rps()
        m2 = ctx.mark()
        marks.append((m0, m1, m2))
      ctx.synchronize()
      tb = np.median([ctx.mark_elapsed(a, b) for a, b, _ in marks])
      tr = np.median([ctx.mark_elapsed(b, c) for _, b, c in marks])
      ctx.marks_reset()
      got = ctx.download(out_b.ptr, plan.partial_shape(_hip.BRIER_STATS * k), np.float64)
      got = got.reshape(got.shape[:-2] + (_hip.BRIER_STATS, k, got.shape[-1]))  # [.., stat, k, j]
      score = np.moveaxis(got[..., 2, :, :], -2, 0).reshape(k, -1).sum(axis=1) / npoint  # the Brier score per threshold
      # the unfair RPS of the other kernel is the sum over thresholds of the same squared errors (its compare is <=, ours >: the same
      # split of a continuous sample)
      rps_mean = float(ctx.download(out_r.ptr, plan.partial_shape(1), np.float64).sum()) / npoint
      assert np.isfinite(got).all() and (score >= 0).all() and (score <= 1).all(), score
      assert abs(float(score.sum()) - rps_mean) < 1e-9 * max(1.0, rps_mean), (float(score.sum()), rps_mean)
      lines.append(f'    K={k:2d}: brier {tb:7.3f} ms ({nbytes / tb / 1e9:6.3f} TB/s)   rps {tr:7.3f} ms ({nbytes / tr / 1e9:6.3f} TB/s)'
                   f'   ratio {tb / tr:5.3f}   mean Brier score over thresholds {float(score.mean()):.6f}')


def end_to_end(ctx, lines, route, grid=(721, 1440)):
  shape = (1,) + tuple(grid)
  dims = ('lead_time', 'latitude', 'longitude')
  rng = np.random.default_rng(1)
  t = rng.gamma(2.0, size=shape).astype(np.float32)
  p = (t[None] * rng.gamma(8.0, 1 / 8.0, size=(M,) + shape)).astype(np.float32)
  coords = {'lead_time': (np.arange(shape[0]) * 12).astype('timedelta64[h]').astype('timedelta64[ns]'),
            'latitude': np.linspace(-90, 90, shape[1]), 'longitude': np.linspace(0, 360, shape[2], endpoint=False)}
  thresholds = [0.5, 1.0, 2.0, 3.0, 5.0]
  metrics = {'brier': wrappers.WrappedMetric(deterministic.MSE(), [wrappers.ContinuousToBinary('both', thresholds, 'threshold'),
                                                                   wrappers.EnsembleMean('predictions', 'number')])}
  agg = aggregation.Aggregator(reduce_dims=['latitude', 'longitude'])
  has_fused = hasattr(lazy, 'FUSED_BRIER')
  lines.append(f'(b) end to end, MSE behind ContinuousToBinary -> EnsembleMean at {len(thresholds)} thresholds of host f32{[M] + list(shape)} against '
               f'f32{list(shape)}, reduce (latitude, longitude): host wall time of compute + aggregate_statistics up to a synchronise, new arrays '
               'every repetition')
  results, medians = {}, {}
  routes = {'both': ((True, 5), (False, 5)), 'fused': ((True, 5),), 'host': ((False, 5),)}[route]
  for fused, reps in routes:
    if has_fused:
      lazy.FUSED_BRIER = fused
    else:
      assert not fused, 'this checkout has no fused route'
    times = []
    for rep in range(reps + 1):
      pred = {'v': xr.DataArray(p, dims=('number',) + dims, coords=coords)}
      targ = {'v': xr.DataArray(t, dims=dims, coords=coords)}
      t0 = time.perf_counter()
      stats = mb.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
      t1 = time.perf_counter()
      state = agg.aggregate_statistics(stats)
      ctx.synchronize()
      t2 = time.perf_counter()
      if rep:  # (the first repetition builds plans and weight tables)
        times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    results[fused] = np.asarray(state.metric_values(metrics)['brier.v'].values, np.float64)
    st, ag = np.median([a for a, _ in times]), np.median([b for _, b in times])
    medians[fused] = st + ag
    name = 'fused (wbx_ens_brier_partial)' if fused else ('host route (WBX_FUSED_BRIER=0)' if has_fused else 'host route (no fused route here)')
    lines.append(f'    {name:34s}: statistics {st:9.2f} ms   aggregate_statistics {ag:9.2f} ms   total {st + ag:9.2f} ms   ({reps} repetitions, medians)'
                 f'   Brier score at the first threshold {float(results[fused].ravel()[0]):.12f}')
  if has_fused:
    lazy.FUSED_BRIER = True
  if len(results) == 2:
    err = float(np.nanmax(np.abs(results[True] - results[False]) / np.abs(results[False])))
    ratio = medians[False] / medians[True]
    ok = ratio > E2E_GATE
    lines.append(f'    largest relative |fused - host route| = {err:.3e};  host route / fused = {ratio:.1f} x '
                 f'(gate: more than {E2E_GATE} x, the box spread: {"holds" if ok else "MISSED"})')
    return ok
  return True


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'brier_kbench.txt'))
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-e2e', action='store_true')
  ap.add_argument('--e2e-route', choices=('both', 'fused', 'host'), default='both')
  ap.add_argument('--e2e-grid', type=int, nargs=2, default=(721, 1440), metavar=('NLAT', 'NLON'))
  args = ap.parse_args()
  ctx = _hip.default_context()
  lines = [f'tools/bench_brier.py on {ctx.device_name()}; wbx_clock_probe {ctx.clock_probe():.0f} MHz before']
  ok = True
  if not args.skip_kernel:
    kernel_times(ctx, lines)
  if not args.skip_e2e:
    ok = end_to_end(ctx, lines, args.e2e_route, args.e2e_grid)
  lines.append(f'wbx_clock_probe {ctx.clock_probe():.0f} MHz after')
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(args.out, 'w') as f:
    f.write(text)
  sys.exit(0 if ok else 1)


if __name__ == '__main__':
  main()
