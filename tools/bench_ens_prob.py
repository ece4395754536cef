"""Contingency tables of ensemble event probabilities (wbx_ens_prob_contingency_partial): kernel time against the ranked
probability score kernel on the same plan and inputs, and one public-API chunk end to end against the host route.

(a) f32[51, 40, 721, 1440] predictions against f32[40, 721, 1440] targets (generated on the device): wbx_ens_prob_contingency_partial
    at (event thresholds, probability slots) = (1, 1), (1, 4), (1, 16), (4, 4), alternating launch by launch with
    wbx_ens_rps_partial at as many thresholds on the same plan -- the same loads, the same compares -- 10 timed launches each
    between wbx_mark pairs, medians; every dim reduced (x summed) and longitude kept.
(b) RelativeEconomicValue(ensemble_size=51) at one event threshold of f32[51, 1, 721, 1440] against f32[1, 721, 1440] HOST arrays
    through the public API: host wall time from Statistic.compute through Aggregator.aggregate_statistics up to a synchronise,
    fused route against WBX_FUSED_ENS_PROB=0 (new arrays every repetition, so both routes pay their uploads).

Usage: python tools/bench_ens_prob.py [--out profiles/ens_prob_kbench.txt] [--skip-kernel] [--skip-e2e] [--e2e-route both|fused|host] [--e2e-grid NLAT NLON]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from weatherbenchx_amd import _hip, aggregation, engine, lazy, planner
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as mb, multivariate, wrappers

M = 51
REPS = 10


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
  lines.append(f'(a) kernel time, f32{[M] + list(shape)} against f32{list(shape)}, {nbytes / 1e9:.2f} GB per launch; {REPS} launches each, '
               'alternating with wbx_ens_rps_partial (unfair, right-inclusive) at as many thresholds on the same plan, medians')
  for what, reduce_dims in (('x summed (every dim reduced)', dims), ('x kept (longitude kept)', dims[:2])):
    plan = planner.build_s1_plan(dims, sizes, [lay_p, lay_t, None, None], reduce_dims, wdep_dims=set(), flags=0, allow_vec4=False)
    dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
    lines.append(f'  {what}: plan nkey={plan.nkey} nchunk={plan.nchunk} depth_chunk={plan.depth_chunk} nx={plan.nx} x_kept={plan.x_kept} '
                 f'block={plan.block_threads} vec={plan.vec}')
    out_r = ctx.alloc(int(np.prod(plan.partial_shape(1))) * 8)
    for k, j in ((1, 1), (1, 4), (1, 16), (4, 4)):
      nl = _hip.EPC_CELLS * k * j
      out_c = ctx.alloc(int(np.prod(plan.partial_shape(nl))) * 8)
      thr = ctx.upload(np.linspace(-1.5, 1.5, k) if k > 1 else np.zeros(1))
      taus = (np.arange(j) + 0.5) / j  # probability thresholds as runs of member counts: c / M > tau
      lo = np.array([min(c for c in range(M + 2) if c == M + 1 or np.float32(c) / np.float32(M) > tau) for tau in taus])
      slots = ctx.upload(np.stack([lo, np.full(j, M)], axis=1).astype(np.int32))

      def epc():
        _hip.check(ctx.lib.wbx_ens_prob_contingency_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, M, npoint, k, ptr(thr.ptr), j,
                                                            ptr(slots.ptr), ptr(p.data_ptr()), ptr(t.data_ptr()), None, ptr(out_c.ptr)),
                   'wbx_ens_prob_contingency_partial')

      def rps():
        _hip.check(ctx.lib.wbx_ens_rps_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, M, npoint, k, ptr(thr.ptr), ptr(thr.ptr), 1,
                                               ptr(p.data_ptr()), ptr(t.data_ptr()), None, ptr(out_r.ptr)), 'wbx_ens_rps_partial')
      for _ in range(2):
        epc()
        rps()
      ctx.synchronize()
      ctx.marks_reset()
      marks = []
      for _ in range(REPS):
        m0 = ctx.mark()
        epc()
        m1 = ctx.mark()
        rps()
        m2 = ctx.mark()
        marks.append((m0, m1, m2))
      ctx.synchronize()
      tc = np.median([ctx.mark_elapsed(a, b) for a, b, _ in marks])
      tr = np.median([ctx.mark_elapsed(b, c) for _, b, c in marks])
      ctx.marks_reset()
      got = ctx.download(out_c.ptr, plan.partial_shape(nl), np.float64)
      total = got.reshape(-1, nl, got.shape[-1]).sum(axis=(0, 2)).reshape(_hip.EPC_CELLS, k * j)  # [..., lane, j] -> per lane
      assert np.isfinite(got).all() and (total.sum(axis=0) == npoint).all(), total  # the four cells of a pair hold every point once
      lines.append(f'    (K, J)=({k:2d}, {j:2d}): tables {tc:7.3f} ms ({nbytes / tc / 1e9:6.3f} TB/s)   rps {tr:7.3f} ms ({nbytes / tr / 1e9:6.3f} TB/s)'
                   f'   ratio {tc / tr:5.3f}   hit rate of pair 0 {total[0, 0] / max(total[0, 0] + total[2, 0], 1):.4f}')


def end_to_end(ctx, lines, route, grid=(721, 1440)):
  shape = (1,) + tuple(grid)
  dims = ('lead_time', 'latitude', 'longitude')
  rng = np.random.default_rng(1)
  t = rng.gamma(2.0, size=shape).astype(np.float32)
  p = (t[None] * rng.gamma(8.0, 1 / 8.0, size=(M,) + shape)).astype(np.float32)
  coords = {'lead_time': (np.arange(shape[0]) * 12).astype('timedelta64[h]').astype('timedelta64[ns]'),
            'latitude': np.linspace(-90, 90, shape[1]), 'longitude': np.linspace(0, 360, shape[2], endpoint=False)}
  chain = [wrappers.ContinuousToBinary('both', [2.0], 'event'), wrappers.EnsembleMean('predictions', 'number')]
  metrics = {'rev': wrappers.WrappedMetric(multivariate.RelativeEconomicValue(ensemble_size=M), chain)}
  agg = aggregation.Aggregator(reduce_dims=['latitude', 'longitude'])
  lines.append(f'(b) end to end, RelativeEconomicValue(ensemble_size={M}) at one event threshold of host f32{[M] + list(shape)} against '
               f'f32{list(shape)}, reduce (latitude, longitude): host wall time of compute + aggregate_statistics up to a synchronise, new '
               'arrays every repetition')
  results, medians = {}, {}
  routes = {'both': ((True, 5), (False, 3)), 'fused': ((True, 5),), 'host': ((False, 3),)}[route]
  for fused, reps in routes:
    lazy.FUSED_ENS_PROB = fused
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
    results[fused] = np.asarray(state.metric_values(metrics)['rev.v'].values)
    st, ag = np.median([a for a, _ in times]), np.median([b for _, b in times])
    medians[fused] = st + ag
    name = 'fused (wbx_ens_prob_contingency_partial)' if fused else 'host route (WBX_FUSED_ENS_PROB=0)'
    lines.append(f'    {name:42s}: statistics {st:9.2f} ms   aggregate_statistics {ag:9.2f} ms   total {st + ag:9.2f} ms   ({reps} repetitions, medians)'
                 f'   largest REV {float(np.nanmax(results[fused])):.12f}')
  lazy.FUSED_ENS_PROB = True
  if len(results) == 2:
    same = bool(np.array_equal(results[True], results[False], equal_nan=True))
    lines.append(f'    the same metric values on both routes: {same};  host route / fused = {medians[False] / medians[True]:.1f} x (gate: at least 5 x)')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ens_prob_kbench.txt'))
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-e2e', action='store_true')
  ap.add_argument('--e2e-route', choices=('both', 'fused', 'host'), default='both')
  ap.add_argument('--e2e-grid', type=int, nargs=2, default=(721, 1440), metavar=('NLAT', 'NLON'))
  args = ap.parse_args()
  ctx = _hip.default_context()
  lines = [f'tools/bench_ens_prob.py on {ctx.device_name()}; wbx_clock_probe {ctx.clock_probe():.0f} MHz before']
  if not args.skip_kernel:
    kernel_times(ctx, lines)
  if not args.skip_e2e:
    end_to_end(ctx, lines, args.e2e_route, args.e2e_grid)
  lines.append(f'wbx_clock_probe {ctx.clock_probe():.0f} MHz after')
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
