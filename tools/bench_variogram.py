"""Variogram score of ensembles (wbx_ens_variogram_partial): kernel time against its floors, and TiledVariogramScore through the
public API end to end against the host route.

(a) f32[51, 13, 721, 1440] predictions against f32[13, 721, 1440] targets tiled 3 x 3 the way wrappers.Tile stores the windows of a
    host payload: a leading window axis of 9 over (level, 719 latitudes with a full window, 1440 longitudes), generated on the
    device; p = 0.5.  10 timed launches each between wbx_mark pairs (HIP events), medians; the frame reduced over (latitude,
    longitude) (x summed) and over latitude (x kept).  Next to each: bytes / 8 TB/s, and the VALU floor: TERM_INSTRUCTIONS vector
    instructions per term (read from the disassembly of the member loop of vgrm_x?_kernel<float, HALF, 8>) x
    M L (L - 1) / 2 terms per point / (256 CUs x 64 lanes x the probed clock).
(b) TiledVariogramScore(window_size=3) of device-resident f32[51, 13, NLAT, NLON] against f32[13, NLAT, NLON] through the public
    API: host wall time from Statistic.compute through Aggregator.aggregate_statistics up to a synchronise, the fused route against
    WBX_FUSED_VARIOGRAM=0 on the same payload in the same process (new tensors every repetition).  `--e2e-route host` runs the host
    route alone and needs nothing of the fused one: the same file times a checkout from before the kernel existed.
(c) the same metric on a small float64 payload on both routes: the switched-off route is the code the parent commit ran, and in
    float64 the two routes' scores must agree to the bound both routes' float64 arithmetic allows (printed with all digits).

Usage: python tools/bench_variogram.py [--out profiles/variogram_kbench.txt] [--skip-kernel] [--skip-e2e] [--e2e-route both|fused|host]
       [--e2e-grid NLAT NLON]"""
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
NLEVEL = 13
WINDOW = 9
REPS = 10
GRID = (721, 1440)
HBM_TBS = 8.0
CUS, LANES = 256, 64
TERM_INSTRUCTIONS = 12  # v_add_u32 x 3, v_sub_f32, v_cmp, v_cndmask x 2, v_ldexp x 2, v_sqrt_f32, v_cvt_f64_f32, v_add_f64


def kernel_times(ctx, lines, clock_mhz):
  import torch  # pylint: disable=g-import-not-at-top
  dims = ('level', 'latitude', 'longitude')
  shape = (NLEVEL, GRID[0] - 2, GRID[1])
  sizes = dict(zip(dims, shape))
  npoint = int(np.prod(shape))
  ptr = lambda v: C.c_void_p(int(v))
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  t = torch.randn((WINDOW,) + shape, generator=g, device='cuda')
  p = torch.randn((WINDOW * M,) + shape, generator=g, device='cuda')  # [window][member][level][latitude][longitude]
  torch.cuda.synchronize()
  nbytes = (M + 1) * WINDOW * npoint * 4
  terms = float(M) * WINDOW * (WINDOW - 1) / 2 * npoint
  floor_hbm = nbytes / (HBM_TBS * 1e12) * 1e3
  floor_valu = terms * TERM_INSTRUCTIONS / (CUS * LANES * clock_mhz * 1e6) * 1e3
  lines.append(f'(a) kernel time, p = 0.5, {REPS} launches each between event pairs, medians; floors: bytes / {HBM_TBS:.0f} TB/s and '
               f'{TERM_INSTRUCTIONS} instructions x M L (L - 1) / 2 terms per point / ({CUS} CUs x {LANES} lanes x {clock_mhz:.0f} MHz)')
  lines.append(f'  f32[{M}, {NLEVEL}, {GRID[0]}, {GRID[1]}] against f32[{NLEVEL}, {GRID[0]}, {GRID[1]}] tiled 3 x 3: f32[{WINDOW}, {M}, {shape[0]}, '
               f'{shape[1]}, {shape[2]}] against f32[{WINDOW}, {shape[0]}, {shape[1]}, {shape[2]}], the window axis outermost: {nbytes / 1e9:.2f} GB, '
               f'{terms:.3g} terms; floors {floor_hbm:.3f} ms (HBM) and {floor_valu:.3f} ms (VALU)')
  strides = {'level': shape[1] * shape[2], 'latitude': shape[2], 'longitude': 1}
  lay = planner.InputLayout(strides=dict(strides), itemsize=4, base_alignment=256)
  for what, reduce_dims in (('x summed', dims[1:]), ('x kept  ', dims[1:2])):
    plan = planner.build_s1_plan(dims, sizes, [lay, lay, None, None], reduce_dims, wdep_dims=set(), flags=0, allow_vec4=False)
    dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
    out = ctx.alloc(int(np.prod(plan.partial_shape(_hip.VGRAM_LANES))) * 8)

    def launch():
      _hip.check(ctx.lib.wbx_ens_variogram_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, M, npoint, WINDOW, M * npoint, npoint,
                                                   _hip.VGRAM_POW_HALF, ptr(p.data_ptr()), ptr(t.data_ptr()), None, ptr(out.ptr)),
                 'wbx_ens_variogram_partial')
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
    got = ctx.download(out.ptr, plan.partial_shape(_hip.VGRAM_LANES), np.float64)
    assert np.isfinite(got).all(), 'non-finite partials'
    lines.append(f'    {what}: {ms:8.3f} ms  = {ms / floor_hbm:6.1f} x the HBM floor ({nbytes / ms / 1e9:5.3f} TB/s), {ms / floor_valu:5.2f} x the VALU floor'
                 f'   plan x_dim={plan.x_dim} nkey={plan.nkey} nchunk={plan.nchunk} depth_chunk={plan.depth_chunk} nx={plan.nx} block={plan.block_threads if plan.x_kept else 256}'
                 + ('' if plan.x_kept else f' (x summed always runs 256 threads; the plan says {plan.block_threads})') +
                 f' tile={_hip.vgram_tile_points(WINDOW)} points, members staged {_hip.vgram_member_chunk(M, WINDOW)} at a time, '
                 f'loads coalesced along x (the window axis is outermost)   mean score {got.sum() / npoint:.6f}')
  del p, t


def _fields(rng_seed, shape, dtype, device):
  import torch  # pylint: disable=g-import-not-at-top
  rng = np.random.default_rng(rng_seed)
  t = rng.normal(size=shape).astype(dtype)
  p = (t[None] + rng.normal(size=(M,) + shape)).astype(dtype)
  if device:
    return torch.as_tensor(p).cuda(), torch.as_tensor(t).cuda()
  return p, t


def _evaluate(ctx, metrics, agg, p, t, dims, coords):
  import torch  # pylint: disable=g-import-not-at-top
  pred = {'v': xr.DataArray(p, dims=('number',) + dims, coords=coords)}
  targ = {'v': xr.DataArray(t, dims=dims, coords=coords)}
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  stats = mb.compute_unique_statistics_for_all_metrics(metrics, pred, targ)
  t1 = time.perf_counter()
  state = agg.aggregate_statistics(stats)
  ctx.synchronize()
  torch.cuda.synchronize()
  t2 = time.perf_counter()
  score = float(np.asarray(state.metric_values(metrics)['vs.v'].values).ravel()[0])
  return (t1 - t0) * 1e3, (t2 - t1) * 1e3, score


def end_to_end(ctx, lines, route, grid):
  shape = (NLEVEL,) + tuple(grid)
  dims = ('level', 'latitude', 'longitude')
  coords = {'level': np.arange(NLEVEL) * 50.0 + 100.0, 'latitude': np.linspace(-90, 90, shape[1]),
            'longitude': np.linspace(0, 360, shape[2], endpoint=False)}
  metrics = {'vs': probabilistic.TiledVariogramScore(window_size=3, ensemble_dim='number')}
  agg = aggregation.Aggregator(reduce_dims=['level', 'latitude', 'longitude'])
  lines.append(f'(b) end to end, TiledVariogramScore(window_size=3) of device-resident f32{[M] + list(shape)} against f32{list(shape)}, every dim '
               'reduced: host wall time of compute + aggregate_statistics up to a synchronise, new tensors every repetition')
  has_switch = hasattr(lazy, 'FUSED_VARIOGRAM')
  results, medians, failures = {}, {}, []
  routes = {'both': ((True, 5), (False, 3)), 'fused': ((True, 5),), 'host': ((False, 3),)}[route]
  for fused, reps in routes:
    if has_switch:
      lazy.FUSED_VARIOGRAM = fused
    else:
      assert not fused, 'this checkout has no fused route'
    times = []
    for rep in range(reps + 1):
      p, t = _fields(100 + reps - rep, shape, np.float32, True)  # (the last repetition scores the same fields on every route)
      st, ag, score = _evaluate(ctx, metrics, agg, p, t, dims, coords)
      if rep:  # (the first repetition builds plans and weight tables)
        times.append((st, ag))
      del p, t
    results[fused] = score
    st, ag = np.median([a for a, _ in times]), np.median([b for _, b in times])
    medians[fused] = st + ag
    name = 'fused (wbx_ens_variogram_partial)' if fused else ('host route (WBX_FUSED_VARIOGRAM=0)' if has_switch else 'host route (no fused route here)')
    lines.append(f'    {name:36s}: statistics {st:9.2f} ms   aggregate_statistics {ag:9.2f} ms   total {st + ag:9.2f} ms   ({reps} repetitions, medians)'
                 f'   score {results[fused]:.12f}')
  if len(results) == 2:
    # per pair both routes are within a few float32 roundings of the exact terms: |score difference| <= 1e-5 of the score is what
    # the per-point bounds of tests/variogram_cases.py come to on these fields (about 1e-6 each), with a factor of five to spare
    err, bound = abs(results[True] - results[False]), 1e-5 * abs(results[False])
    lines.append(f'    |score fused - score host route| = {err:.3e} (bound {bound:.3e});  host route / fused = {medians[False] / medians[True]:.1f} x '
                 '(gate: at least 5 x)')
    if not err <= bound:
      failures.append(f'the scores of the two routes differ by {err:.3e}, more than the bound {bound:.3e}')
    if not medians[False] >= 5 * medians[True]:
      failures.append('the fused route is not 5 x faster than the host route')
  # (c) float64: the switched-off route is the parent commit's code; the fused route must give its score to float64 accuracy: per
  # pair either route is within (M + 5) 2^-53 (ty + tx) of the exact difference e, about 6e-15, and on random fields (ty + tx) / |e|
  # stays far below the 100 that 1e-12 of the score leaves room for
  small = (3, 24, 36)
  coords = {'level': np.arange(3) * 50.0, 'latitude': np.linspace(-80, 80, small[1]), 'longitude': np.linspace(0, 360, small[2], endpoint=False)}
  scores = {}
  for fused in ((True, False) if has_switch and route == 'both' else (False,)):
    if has_switch:
      lazy.FUSED_VARIOGRAM = fused
    p, t = _fields(7, small, np.float64, True)
    scores[fused] = _evaluate(ctx, metrics, agg, p, t, dims, coords)[2]
    engine.clear_caches()
  if has_switch:
    lazy.FUSED_VARIOGRAM = True
  lines.append(f'(c) float64 f64{[M] + list(small)}: host route score {scores[False]!r}' + (
      f', fused {scores[True]!r}, relative difference {abs(scores[True] - scores[False]) / abs(scores[False]):.3e} (bound 1e-12)' if True in scores else ''))
  if True in scores and not abs(scores[True] - scores[False]) <= 1e-12 * abs(scores[False]):
    failures.append('the float64 scores of the two routes differ by more than 1e-12 of the score')
  return failures


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'variogram_kbench.txt'))
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-e2e', action='store_true')
  ap.add_argument('--e2e-route', choices=('both', 'fused', 'host'), default='both')
  ap.add_argument('--e2e-grid', type=int, nargs=2, default=(181, 360), metavar=('NLAT', 'NLON'))
  args = ap.parse_args()
  ctx = _hip.default_context()
  clock = ctx.clock_probe()
  lines = [f'tools/bench_variogram.py on {ctx.device_name()}; wbx_clock_probe {clock:.0f} MHz before']
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
