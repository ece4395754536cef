"""Energy score of ensembles (wbx_ens_energy_partial): kernel time against its two floors, and one public-API evaluation end to
end against the host route.

(a) f32[51, 13, 721, 1440] predictions against f32[13, 721, 1440] targets, the norm over the level axis (stride 721 * 1440), and
    f32[9, 51, 721, 1440] against f32[9, 721, 1440], the norm over a leading window axis as TiledEnergyScore stores it (generated
    on the device), fair: 10 timed launches each between wbx_mark pairs (HIP events), medians; every dim reduced (x summed) and
    longitude kept.  Next to each: bytes / 8 TB/s, and 2 L M (M + 1) / 2 lane operations per point / (256 CUs x 64 lanes x the
    probed clock) -- one subtraction and one fma per element of every pair of the M + 1 vectors.
(b) EnergyScore(dim='level') of host f32[51, 13, NLAT, NLON] against f32[13, NLAT, NLON] through the public API: host wall time
    from Statistic.compute through Aggregator.aggregate_statistics up to a synchronise, fused route against WBX_FUSED_ENERGY=0 (new
    arrays every repetition, so both routes pay their uploads).  `--e2e-route host` runs the host route alone and needs nothing of
    the fused one: the same file times a checkout from before the kernel existed.

Usage: python tools/bench_energy.py [--out profiles/energy_kbench.txt] [--skip-kernel] [--skip-e2e] [--e2e-route both|fused|host] [--e2e-grid NLAT NLON]"""
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
GRID = (721, 1440)
HBM_TBS = 8.0
CUS, LANES = 256, 64


def kernel_times(ctx, lines, clock_mhz):
  import torch  # pylint: disable=g-import-not-at-top
  dims = ('latitude', 'longitude')
  sizes = dict(zip(dims, GRID))
  npoint = GRID[0] * GRID[1]
  ptr = lambda v: C.c_void_p(int(v))
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  lines.append(f'(a) kernel time, fair, {REPS} launches each between event pairs, medians; floors: bytes / {HBM_TBS:.0f} TB/s and '
               f'2 L M (M + 1) / 2 lane operations per point / ({CUS} CUs x {LANES} lanes x {clock_mhz:.0f} MHz)')
  for name, nl, member_stride, norm_stride_p, norm_stride_t in (
      ('levels in the middle: f32[51, 13, 721, 1440] against f32[13, 721, 1440]', 13, 13 * npoint, npoint, npoint),
      ('window outermost:     f32[9, 51, 721, 1440] against f32[9, 721, 1440]', 9, npoint, M * npoint, npoint)):
    t = torch.randn((nl,) + GRID, generator=g, device='cuda')
    p = torch.randn((M * nl,) + GRID, generator=g, device='cuda')  # (both storage orders are M * L fields of the grid)
    torch.cuda.synchronize()
    nbytes = (M + 1) * nl * npoint * 4
    ops = 2.0 * nl * M * (M + 1) / 2 * npoint
    floor_hbm = nbytes / (HBM_TBS * 1e12) * 1e3
    floor_valu = ops / (CUS * LANES * clock_mhz * 1e6) * 1e3
    lines.append(f'  {name}: {nbytes / 1e9:.2f} GB, {ops:.3g} lane operations; floors {floor_hbm:.3f} ms (HBM) and {floor_valu:.3f} ms (VALU)')
    strides = {'latitude': GRID[1], 'longitude': 1}
    lay = planner.InputLayout(strides=dict(strides), itemsize=4, base_alignment=256)
    for what, reduce_dims in (('x summed', dims), ('x kept  ', dims[:1])):
      plan = planner.build_s1_plan(dims, sizes, [lay, lay, None, None], reduce_dims, wdep_dims=set(), flags=_hip.FLAG_FAIR, allow_vec4=False)
      dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
      out = ctx.alloc(int(np.prod(plan.partial_shape(_hip.ENRG_LANES))) * 8)

      def launch():
        _hip.check(ctx.lib.wbx_ens_energy_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, M, member_stride, nl, norm_stride_p,
                                                  norm_stride_t, ptr(p.data_ptr()), ptr(t.data_ptr()), None, ptr(out.ptr)),
                   'wbx_ens_energy_partial')
      for _ in range(2):
        launch()
      ctx.synchronize()
      ctx.marks_reset()
      marks = []
      for _ in range(REPS):
        m0 = ctx.mark()
        launch()
        marks.append((m0, ctx.mark()))
      ctx.synchronize()
      ms = float(np.median([ctx.mark_elapsed(a, b) for a, b in marks]))
      ctx.marks_reset()
      got = ctx.download(out.ptr, plan.partial_shape(_hip.ENRG_LANES), np.float64)
      lanes = got.reshape(-1, _hip.ENRG_LANES, plan.nj).sum(axis=(0, 2)) / npoint
      assert np.isfinite(got).all(), 'non-finite partials'
      lines.append(f'    {what}: {ms:8.3f} ms  = {ms / floor_hbm:6.1f} x the HBM floor ({nbytes / ms / 1e9:5.3f} TB/s), {ms / floor_valu:5.1f} x the VALU floor'
                   f'   plan nkey={plan.nkey} nchunk={plan.nchunk} depth_chunk={plan.depth_chunk} block={plan.block_threads}'
                   f' tile={_hip.enrg_tile_points(M, plan.block_threads)}   mean skill {lanes[0]:.6f} spread {lanes[1]:.6f}')
    del p, t


def end_to_end(ctx, lines, route, grid):
  nl = 13
  shape = (nl,) + tuple(grid)
  dims = ('level', 'latitude', 'longitude')
  coords = {'level': np.arange(nl) * 50.0 + 100.0, 'latitude': np.linspace(-90, 90, shape[1]),
            'longitude': np.linspace(0, 360, shape[2], endpoint=False)}
  metrics = {'es': probabilistic.EnergyScore(dim='level', ensemble_dim='number')}
  agg = aggregation.Aggregator(reduce_dims=['latitude', 'longitude'])
  lines.append(f'(b) end to end, fair EnergyScore(dim=level) of host f32{[M] + list(shape)} against f32{list(shape)}, reduce (latitude, '
               'longitude): host wall time of compute + aggregate_statistics up to a synchronise, new arrays every repetition')
  has_switch = hasattr(lazy, 'FUSED_ENERGY')
  results, medians, failures = {}, {}, []
  routes = {'both': ((True, 5), (False, 3)), 'fused': ((True, 5),), 'host': ((False, 3),)}[route]
  for fused, reps in routes:
    if has_switch:
      lazy.FUSED_ENERGY = fused
    else:
      assert not fused, 'this checkout has no fused route'
    times = []
    for rep in range(reps + 1):
      rng = np.random.default_rng(100 + reps - rep)  # (new arrays every repetition; the last one scores the same arrays on every route)
      t = rng.normal(size=shape).astype(np.float32)
      p = (t[None] + rng.normal(size=(M,) + shape)).astype(np.float32)
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
    results[fused] = float(np.asarray(state.metric_values(metrics)['es.v'].values).ravel()[0])
    means = [float(np.asarray(state.sum_weighted_statistics[s.unique_name]['v'].values).ravel()[0])
             / float(np.asarray(state.sum_weights[s.unique_name]['v'].values).ravel()[0]) for s in metrics['es'].statistics.values()]
    magnitude = means[0] + 0.5 * means[1]  # mean skill + mean spread / 2: what the relative per-point bounds apply to
    st, ag = np.median([a for a, _ in times]), np.median([b for _, b in times])
    medians[fused] = st + ag
    name = 'fused (wbx_ens_energy_partial)' if fused else ('host route (WBX_FUSED_ENERGY=0)' if has_switch else 'host route (no fused route here)')
    lines.append(f'    {name:36s}: statistics {st:9.2f} ms   aggregate_statistics {ag:9.2f} ms   total {st + ag:9.2f} ms   ({reps} repetitions, medians)'
                 f'   score {results[fused]:.12f}')
  if has_switch:
    lazy.FUSED_ENERGY = True
  if len(results) == 2:
    u = 2.0 ** -24
    # per point: the fused route (L / 2 + 4) u + (M^2 + 4) 2^-53, the host route (L / 2 + 4 + 2 M) u (it adds the norms in float32)
    bound = ((nl / 2 + 4) * u + (M * M + 4) * 2.0 ** -53 + (nl / 2 + 4 + 2 * M) * u) * magnitude
    err = abs(results[True] - results[False])
    lines.append(f'    |score fused - score host route| = {err:.3e} (bound {bound:.3e}: both routes\' relative per-point bounds on mean skill + mean spread / 2);'
                 f'  host route / fused = {medians[False] / medians[True]:.1f} x (gate: at least 5 x)')
    if not err <= bound:
      failures.append(f'the scores of the two routes differ by {err:.3e}, more than the bound {bound:.3e}')
    if not medians[False] >= 5 * medians[True]:
      failures.append('the fused route is not 5 x faster than the host route')
  return failures


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'energy_kbench.txt'))
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-e2e', action='store_true')
  ap.add_argument('--e2e-route', choices=('both', 'fused', 'host'), default='both')
  ap.add_argument('--e2e-grid', type=int, nargs=2, default=(91, 180), metavar=('NLAT', 'NLON'))
  args = ap.parse_args()
  ctx = _hip.default_context()
  clock = ctx.clock_probe()
  lines = [f'tools/bench_energy.py on {ctx.device_name()}; wbx_clock_probe {clock:.0f} MHz before']
  if not args.skip_kernel:
    kernel_times(ctx, lines, clock)
  failures = [] if args.skip_e2e else end_to_end(ctx, lines, args.e2e_route, args.e2e_grid)
  lines.append(f'wbx_clock_probe {ctx.clock_probe():.0f} MHz after')
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(args.out, 'w') as f:
    f.write(text)
  if failures:  # (the figures are on file either way)
    sys.exit('; '.join(failures))


if __name__ == '__main__':
  main()
