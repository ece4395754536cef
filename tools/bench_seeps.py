"""SEEPS from a per-place score table (wbx_seeps_partial): kernel time against wbx_det_partial(WBX_DET6) on the same plan, and SEEPS
through the public API end to end against the host route.

(a) f32[40, 721, 1440] predictions and targets (40 valid times, 6-hourly) and a wet-threshold climatology f32[4, 366, 721, 1440]
    (hour, dayofyear, latitude, longitude) gathered in place, all generated on the device; the score table f64[9, 721, 1440] of
    uniform dry fractions.  ONE stage-1 plan per reduction -- every dim reduced (x summed, with dword and with 16-byte loads) and
    (valid_time, latitude) reduced (x kept) -- and the two entry points launched on it in turns through the C ABI, each launch
    between a HIP event pair, medians of REPS.  DET6 reads the same three streams through the same gather and is the yardstick;
    next to it the share of the 8 TB/s peak on the 12 B per point both stream (the table's 8 B per point are expected from cache:
    a place comes back at every valid time).  Twice: with fields whose nine cells come about equally often, so that the lanes of a
    wave read nine different cells of the table, and with fields that are mostly dry, as precipitation is.
(b) One chunk f32[2, 20, 721, 1440] (init_time, lead_time, latitude, longitude) of device-resident tensors through the public API,
    GridAreaWeighting, masked=True, reduced over everything: host wall time from SEEPS.compute through
    Aggregator.aggregate_statistics up to a synchronise, the fused route against WBX_FUSED_SEEPS=0 on the same payload in the same
    process, and the two scores.

Usage: python tools/bench_seeps.py [--out profiles/seeps_kbench.txt] [--skip-kernel] [--skip-e2e]"""
import argparse
import ctypes as C
import dataclasses
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from weatherbenchx_amd import _hip, aggregation, engine, lazy, planner, weighting
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import categorical

NT, GRID = 40, (721, 1440)
CLIM = (4, 366)  # hours, days
REPS = 10
HBM_TBS = 8.0
DIMS = ('valid_time', 'latitude', 'longitude')
DRY = 0.00025


def _fields(seed, shape, power=4):
  """Two fields of 0.02 u^power, u uniform: a third of the values dry for power 4, three quarters for power 16."""
  import torch  # pylint: disable=g-import-not-at-top
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  draw = lambda: torch.rand(shape, generator=g, device='cuda', dtype=torch.float32) ** power * 0.02
  return draw(), draw()


def _climatology(seed, order):
  import torch  # pylint: disable=g-import-not-at-top
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  wet = 0.002 + 0.008 * torch.rand(order + GRID, generator=g, device='cuda', dtype=torch.float32)
  p1 = 0.05 + 0.9 * torch.rand(GRID, generator=g, device='cuda', dtype=torch.float32)
  return wet, p1


def kernel_times(ctx, lines):
  import torch  # pylint: disable=g-import-not-at-top
  wet, p1 = _climatology(2, CLIM)
  table = torch.as_tensor(categorical.seeps_score_table(p1, 0.1, 0.85).reshape((9,) + GRID)).cuda()
  torch.cuda.synchronize()
  place = GRID[0] * GRID[1]
  steps = np.arange(NT)
  offsets = ((steps % 4) * CLIM[1] + 59 + steps // 4).astype(np.int64) * place  # 6-hourly from day 60
  spec = planner.GatherSpec(dims=('valid_time',), table=offsets)
  sizes = dict(zip(DIMS, (NT,) + GRID))
  lay = lambda x, dims: planner.layout_of(x, dims)
  npoint = NT * place
  floor = 12.0 * npoint / (HBM_TBS * 1e12) * 1e3
  lines.append(f'(a) kernel time, f32{[NT] + list(GRID)} against f32{list(CLIM) + list(GRID)} gathered in place, {REPS} launches of each entry point in '
               f'turns on ONE plan, each between an event pair, medians; 12 B per point / {HBM_TBS:.0f} TB/s = {floor:.3f} ms')
  for mix, power in (('a third of the values dry, the nine cells about equally often', 4), ('three quarters of the values dry', 16)):
    p, t = _fields(1, (NT,) + GRID, power)
    torch.cuda.synchronize()
    layouts = [lay(p, DIMS), lay(t, DIMS), lay(wet[0, 0], DIMS[1:]), None]
    lines.append(f'  fields: {mix}')
    for what, reduce_dims, vecs in (('x summed', DIMS, (1, 4)), ('x kept  ', DIMS[:2], (1,))):
      for vec in vecs:
        plan = planner.build_s1_plan(DIMS, sizes, layouts, reduce_dims, wdep_dims=set(), gather=spec, flags=0, allow_vec4=False)
        plan = dataclasses.replace(plan, vec=vec)
        dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
        n = int(np.prod(plan.partial_shape(6), dtype=np.int64))
        out = ctx.alloc(n * 8)
        ptr = lambda x: C.c_void_p(int(x.data_ptr()))
        calls = {
            'wbx_seeps_partial': lambda: ctx.lib.wbx_seeps_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, C.c_double(DRY), ptr(p), ptr(t), ptr(wet),
                                                                   ptr(table), place, None, C.c_void_p(out.ptr)),
            'wbx_det_partial(DET6)': lambda: ctx.lib.wbx_det_partial(ctx.handle, C.byref(dplan.struct), _hip.DET6, _hip.F32, ptr(p), ptr(t), ptr(wet),
                                                                     None, C.c_void_p(out.ptr)),
        }
        times = {k: [] for k in calls}
        for rep in range(REPS + 2):
          for name, call in calls.items():
            ctx.timer_start()
            _hip.check(call(), name)
            ms = ctx.timer_stop()
            if rep >= 2:  # (the first two turns warm the code objects and the cache)
              times[name].append(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for name, ms in med.items():
          lines.append(f'    {what} vec={vec} {name:22s}: {ms:7.3f} ms = {12.0 * npoint / ms / 1e9:5.3f} TB/s on 12 B/point = '
                       f'{100 * floor / ms:4.1f} % of the peak   keys x chunks={plan.nkey * plan.nchunk} block={plan.block_threads}')
        lines.append(f'    {what} vec={vec} wbx_seeps_partial / wbx_det_partial(DET6) = {med["wbx_seeps_partial"] / med["wbx_det_partial(DET6)"]:.3f}')
    del p, t
  del wet, table
  torch.cuda.empty_cache()


def _chunk(seed):
  import torch  # pylint: disable=g-import-not-at-top
  shape = (2, 20) + GRID
  p, t = _fields(seed, shape)
  wet, p1 = _climatology(7, (CLIM[1], CLIM[0]))
  lat, lon = np.linspace(-90, 90, GRID[0]), np.linspace(0, 360, GRID[1], endpoint=False)
  cs = {'init_time': np.datetime64('2020-03-01T00', 'ns') + np.arange(2) * np.timedelta64(12, 'h'),
        'lead_time': (np.arange(20) * np.timedelta64(6, 'h')).astype('timedelta64[ns]'), 'latitude': lat, 'longitude': lon}
  cc = {'dayofyear': np.arange(1, 367), 'hour': np.arange(4) * 6, 'latitude': lat, 'longitude': lon}
  clim = {'tp_seeps_threshold': xr.DataArray(wet, dims=tuple(cc), coords=cc),
          'tp_seeps_dry_fraction': xr.DataArray(p1.reshape((1, 1) + GRID), dims=tuple(cc), coords=dict(cc, dayofyear=[1], hour=[0]))}
  dims = tuple(cs)
  torch.cuda.synchronize()
  return {'tp': xr.DataArray(p, dims=dims, coords=cs, name='tp')}, {'tp': xr.DataArray(t, dims=dims, coords=cs, name='tp')}, clim


def end_to_end(ctx, lines):
  import torch  # pylint: disable=g-import-not-at-top
  lines.append('(b) end to end, one chunk f32[2, 20, 721, 1440] of device-resident tensors, GridAreaWeighting, masked=True, every dim reduced: host '
               'wall time of SEEPS.compute + aggregate_statistics up to a synchronise')
  pred, targ, clim = _chunk(11)
  scores, medians = {}, {}
  for fused, reps in ((True, 5), (False, 2)):
    lazy.FUSED_SEEPS = fused
    stat = categorical.SEEPS(['tp'], clim, 0.25)
    times = []
    for rep in range(reps + 1):
      agg = aggregation.Aggregator(reduce_dims=list(pred['tp'].dims), weigh_by=[weighting.GridAreaWeighting()], masked=True)
      fresh = lambda d: {'tp': xr.DataArray(d['tp'].data, dims=d['tp'].dims, coords=dict(d['tp'].coords), name='tp')}  # (no cached sums)
      a, b = fresh(pred), fresh(targ)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      per_var = stat.compute(a, b)
      t1 = time.perf_counter()
      state = agg.aggregate_statistics({stat.unique_name: per_var})
      ctx.synchronize()
      torch.cuda.synchronize()
      t2 = time.perf_counter()
      if rep:  # (the first repetition builds plans, the table and weight tables)
        times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
      scores[fused] = float(np.asarray(state.mean_statistics()[stat.unique_name]['tp'].values))
      del per_var, state, a, b
      engine.clear_caches()
      torch.cuda.empty_cache()
    st, ag = np.median([x for x, _ in times]), np.median([y for _, y in times])
    medians[fused] = st + ag
    name = 'fused (wbx_seeps_partial)' if fused else 'host route (WBX_FUSED_SEEPS=0)'
    lines.append(f'    {name:32s}: compute {st:9.2f} ms   aggregate_statistics {ag:9.2f} ms   total {st + ag:9.2f} ms   ({reps} repetitions, medians)'
                 f'   score {scores[fused]:.15f}')
  lazy.FUSED_SEEPS = True
  rel = abs(scores[True] - scores[False]) / abs(scores[False])
  lines.append(f'    host route / fused = {medians[False] / medians[True]:.1f} x; relative difference of the scores {rel:.3e}')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'seeps_kbench.txt'))
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-e2e', action='store_true')
  args = ap.parse_args()
  ctx = _hip.default_context()
  lines = [f'tools/bench_seeps.py on {ctx.device_name()}; wbx_clock_probe {ctx.clock_probe():.0f} MHz before']
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
