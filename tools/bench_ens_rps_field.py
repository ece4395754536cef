"""Ranked probability score of ensembles at threshold fields (wbx_ens_rps_field_partial): kernel time against the list kernel on the
same plan and inputs, and one public-API chunk end to end against the host route.

(a) f32[51, 40, 721, 1440] predictions against f32[40, 721, 1440] targets (generated on the device), fair, a float32 threshold field
    [K, 366, 721, 1440] of which the 40 leads gather 40 consecutive days: wbx_ens_rps_field_partial at K = 2, 4, 8, 16, one field
    for both sides (t_off = 0) and two stacked ones, alternating launch by launch with wbx_ens_rps_partial at the same K on the same
    plan, 10 timed launches each between wbx_mark pairs, medians; every dim reduced (x summed) and longitude kept.  Next to the
    ratio of the times stands the ratio of algorithmic bytes per point, (4 M + 4 + 4 K sides) / (4 M + 4).
(b) EnsembleRankedProbabilityScore at a Dataset of float32 terciles [2, 366, 721, 1440] of f32[51, 1, 721, 1440] against
    f32[1, 721, 1440] HOST arrays through the public API: host wall time from Statistic.compute through
    Aggregator.aggregate_statistics up to a synchronise, fused route against WBX_FUSED_ENS_RPS_FIELD=0 in the same run (new arrays
    every repetition, so both routes pay their uploads; the field is resident after the first repetition on both routes).
    `--e2e-route host` runs the host route alone and needs nothing of the fused one: the same file, copied into a checkout from
    before the kernel existed, times that package.

Usage: python tools/bench_ens_rps_field.py [--out profiles/ens_rps_field_kbench.txt] [--skip-kernel] [--skip-e2e] [--e2e-route both|fused|host] [--e2e-grid NLAT NLON]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from weatherbenchx_amd import _hip, aggregation, engine, lazy, planner
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import base as mb, probabilistic

M = 51
REPS = 10
NDAY = 366
E2E_GATE = 5.0  # host route / fused, the gate the list kernel was given


class _AsMetric(mb.PerVariableMetric):

  def __init__(self, statistic):
    self._statistic = statistic

  @property
  def statistics(self):
    return {'s': self._statistic}

  def _values_from_mean_statistics_per_variable(self, statistic_values):
    return statistic_values['s']


def kernel_times(ctx, lines):
  import torch  # pylint: disable=g-import-not-at-top
  shape = (40, 721, 1440)
  dims = ('lead_time', 'latitude', 'longitude')
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  t = torch.randn(shape, generator=g, device='cuda')
  p = t[None] + torch.randn((M,) + shape, generator=g, device='cuda')
  torch.cuda.synchronize()
  npoint, nplace = int(np.prod(shape)), shape[1] * shape[2]
  sizes = dict(zip(dims, shape))
  strides = {'lead_time': shape[1] * shape[2], 'latitude': shape[2], 'longitude': 1}
  lay_p = planner.InputLayout(strides=dict(strides, number=npoint), itemsize=4, base_alignment=256)
  lay_t = planner.InputLayout(strides=dict(strides), itemsize=4, base_alignment=256)
  lay_c = planner.InputLayout(strides={'latitude': shape[2], 'longitude': 1}, itemsize=4, base_alignment=256)
  days = (np.arange(shape[0]) + 340) % NDAY  # across the year end
  gather = planner.GatherSpec(('lead_time',), days.astype(np.int64) * nplace)
  ptr = lambda v: C.c_void_p(int(v))
  lines.append(f'(a) kernel time, f32{[M] + list(shape)} against f32{list(shape)}, fair, a float32 field [K, {NDAY}, {shape[1]}, {shape[2]}] '
               f'(two stacked: [2, K, ...]); {REPS} launches each, alternating with wbx_ens_rps_partial at the same K on the same plan, medians')
  for what, reduce_dims in (('x summed (every dim reduced)', dims), ('x kept (longitude kept)', dims[:2])):
    plan = planner.build_s1_plan(dims, sizes, [lay_p, lay_t, lay_c, None], reduce_dims, wdep_dims=set(), gather=gather, flags=_hip.FLAG_FAIR,
                                 allow_vec4=False)
    dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
    lines.append(f'  {what}: plan nkey={plan.nkey} nchunk={plan.nchunk} depth_chunk={plan.depth_chunk} nx={plan.nx} x_kept={plan.x_kept} '
                 f'block={plan.block_threads} vec={plan.vec}')
    out_f = ctx.alloc(int(np.prod(plan.partial_shape(1))) * 8)
    out_r = ctx.alloc(int(np.prod(plan.partial_shape(1))) * 8)
    for k in (2, 4, 8, 16):
      levels = np.linspace(-1.5, 1.5, k)
      thr = ctx.upload(levels)
      for sides in (1, 2):
        # the list's levels plus a small place-dependent offset: the same order of counts, thresholds that differ point by point
        field = torch.as_tensor(levels, dtype=torch.float32, device='cuda').reshape(1, k, 1, 1, 1) + \
            0.05 * torch.randn((sides, 1, NDAY, shape[1], shape[2]), generator=g, device='cuda')
        torch.cuda.synchronize()
        thr_stride, t_off = NDAY * nplace, (k * NDAY * nplace if sides == 2 else 0)

        def fld():
          _hip.check(ctx.lib.wbx_ens_rps_field_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, _hip.F32, M, npoint, k, thr_stride, t_off, 1,
                                                       ptr(p.data_ptr()), ptr(t.data_ptr()), ptr(field.data_ptr()), None, ptr(out_f.ptr)),
                     'wbx_ens_rps_field_partial')

        def lst():
          _hip.check(ctx.lib.wbx_ens_rps_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, M, npoint, k, ptr(thr.ptr), ptr(thr.ptr), 1,
                                                 ptr(p.data_ptr()), ptr(t.data_ptr()), None, ptr(out_r.ptr)), 'wbx_ens_rps_partial')
        for _ in range(2):
          fld()
          lst()
        ctx.synchronize()
        ctx.marks_reset()
        marks = []
        for _ in range(REPS):
          m0 = ctx.mark()
          fld()
          m1 = ctx.mark()
          lst()
          m2 = ctx.mark()
          marks.append((m0, m1, m2))
        ctx.synchronize()
        tf = np.median([ctx.mark_elapsed(a, b) for a, b, _ in marks])
        tl = np.median([ctx.mark_elapsed(b, c) for _, b, c in marks])
        ctx.marks_reset()
        got = ctx.download(out_f.ptr, plan.partial_shape(1), np.float64)
        mean, mean_l = float(got.sum()) / npoint, float(ctx.download(out_r.ptr, plan.partial_shape(1), np.float64).sum()) / npoint
        assert np.isfinite(got).all() and abs(mean - mean_l) < 0.05 * k, (mean, mean_l)
        nbytes_l = (4 * M + 4) * npoint
        nbytes_f = nbytes_l + 4 * k * sides * npoint
        lines.append(f'    K={k:2d} {"shared " if sides == 1 else "stacked"}: field {tf:7.3f} ms ({nbytes_f / tf / 1e9:6.3f} TB/s)   list {tl:7.3f} ms '
                     f'({nbytes_l / tl / 1e9:6.3f} TB/s)   ratio {tf / tl:5.3f}   ratio of bytes {nbytes_f / nbytes_l:5.3f}   '
                     f'mean RPS {mean:.6f} (list levels {mean_l:.6f})')
        del field


def end_to_end(ctx, lines, route, grid=(721, 1440)):
  shape = (1,) + tuple(grid)
  dims = ('init_time', 'lead_time', 'latitude', 'longitude')
  rng = np.random.default_rng(1)
  t = rng.gamma(2.0, size=(1,) + shape).astype(np.float32)
  p = (t[None] * rng.gamma(8.0, 1 / 8.0, size=(M, 1) + shape)).astype(np.float32)
  lat, lon = np.linspace(-90, 90, shape[1]), np.linspace(0, 360, shape[2], endpoint=False)
  coords = {'init_time': np.array(['2020-12-31'], 'datetime64[ns]'), 'lead_time': (np.arange(1) * 24).astype('timedelta64[h]').astype('timedelta64[ns]'),
            'latitude': lat, 'longitude': lon}
  lower = rng.gamma(2.0, size=(NDAY,) + tuple(grid)).astype(np.float32) * 0.6
  terciles = xr.DataArray(np.stack([lower, lower * 2 + 0.1]), dims=('bin', 'dayofyear', 'latitude', 'longitude'),
                          coords={'bin': np.arange(2), 'dayofyear': np.arange(1, NDAY + 1), 'latitude': lat, 'longitude': lon}, name='v')
  ds = xr.Dataset({'v': terciles})
  metrics = {'rps': _AsMetric(probabilistic.EnsembleRankedProbabilityScore(ds, ds, 'bin', 'bench'))}
  agg = aggregation.Aggregator(reduce_dims=['latitude', 'longitude'])
  lines.append(f'(b) end to end, fair tercile RPS (a Dataset of float32 [2, {NDAY}, {grid[0]}, {grid[1]}]) of host f32{[M, 1] + list(shape)} against '
               f'f32{[1] + list(shape)}, reduce (latitude, longitude): host wall time of compute + aggregate_statistics up to a synchronise, '
               'new arrays every repetition')
  results, medians = {}, {}
  has_switch = hasattr(lazy, 'FUSED_ENS_RPS_FIELD')
  for fused, reps in {'both': ((True, 5), (False, 5)), 'fused': ((True, 5),), 'host': ((False, 5),)}[route]:
    if has_switch:
      lazy.FUSED_ENS_RPS_FIELD = fused
    else:
      assert not fused, 'this checkout has no fused route'
    times = []
    for rep in range(reps + 1):
      pred = {'v': xr.DataArray(p, dims=('number',) + dims, coords=coords, name='v')}
      targ = {'v': xr.DataArray(t, dims=dims, coords=coords, name='v')}
      t0 = time.perf_counter()
      stats = mb.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
      t1 = time.perf_counter()
      state = agg.aggregate_statistics(stats)
      ctx.synchronize()
      t2 = time.perf_counter()
      if rep:  # (the first repetition builds plans, looks at the field's monotonicity and uploads it)
        times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    results[fused] = np.asarray(state.metric_values(metrics)['rps.v'].values)
    st, ag = np.median([a for a, _ in times]), np.median([b for _, b in times])
    medians[fused] = st + ag
    name = 'fused (wbx_ens_rps_field_partial)' if fused else ('host route (WBX_FUSED_ENS_RPS_FIELD=0)' if has_switch else 'host route (no fused route here)')
    lines.append(f'    {name:40s}: statistics {st:9.2f} ms   aggregate_statistics {ag:9.2f} ms   total {st + ag:9.2f} ms   ({reps} repetitions, medians)'
                 f'   RPS {float(results[fused].ravel()[0]):.12f}')
  if has_switch:
    lazy.FUSED_ENS_RPS_FIELD = True
  if len(results) < 2:
    return
  err = float(np.nanmax(np.abs(results[True] - results[False])))
  ratio = medians[False] / medians[True]
  lines.append(f'    largest |RPS fused - RPS host route| = {err:.3e};  host route / fused = {ratio:.1f} x (gate: at least {E2E_GATE:.0f} x: '
               f'{"met" if ratio >= E2E_GATE else "MISSED"})')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ens_rps_field_kbench.txt'))
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-e2e', action='store_true')
  ap.add_argument('--e2e-route', choices=('both', 'fused', 'host'), default='both')
  ap.add_argument('--e2e-grid', type=int, nargs=2, default=(721, 1440), metavar=('NLAT', 'NLON'))
  args = ap.parse_args()
  ctx = _hip.default_context()
  lines = [f'tools/bench_ens_rps_field.py on {ctx.device_name()}; wbx_clock_probe {ctx.clock_probe():.0f} MHz before']
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
