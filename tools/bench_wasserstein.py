"""Wasserstein distance between ensembles (wbx_ens_wasserstein_partial): kernel time against its floors, and WassersteinDistance
through the public API end to end against the host route.

(a) f32[51, 13, 721, 1440] predictions against f32[51, 13, 721, 1440] and against f32[10, 13, 721, 1440] targets, generated on the
    device, the member axes outermost.  10 timed launches each between wbx_mark pairs (HIP events), medians; the frame reduced over
    (latitude, longitude) (x summed) and over latitude (x kept).  Next to each: the HBM floor, (M + N) x 4 bytes per point /
    8 TB/s, and the VALU floor: the vector instructions a point cannot do without -- the two sorting networks (NINSTR of
    csrc/wbx_sortnet3_gen.hpp at the padded sizes), PIECE_INSTRUCTIONS per piece of the walk (read from the disassembly of
    wass_x?_kernel<float>), one conversion per target member and MEMBER_INSTRUCTIONS per loaded member (its NaN
    test and its LDS store or padding select) -- / (256 CUs x 64 lanes x the probed clock).
(b) WassersteinDistance of device-resident tensors of the same shapes through the public API: host wall time from Statistic.compute
    through Aggregator.aggregate_statistics up to a synchronise, the fused route against WBX_FUSED_WASSERSTEIN=0 on the same payload
    in the same process (new tensors every repetition).  `--e2e-route host` runs the host route alone and needs nothing of the
    fused one: the same file times a checkout from before the kernel existed.
(c) the same statistic on a small float64 payload on both routes: the switched-off route is the code the parent commit ran, and
    the two routes' scores must agree to the bound of tests/wasserstein_cases.py (printed with all digits).

Usage: python tools/bench_wasserstein.py [--out profiles/wasserstein_kbench.txt] [--skip-kernel] [--skip-e2e]
       [--e2e-route both|fused|host] [--e2e-shape NLEVEL NLAT NLON]"""
import argparse
import ctypes as C
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from weatherbenchx_amd import _hip, aggregation, engine, lazy, planner
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import probabilistic

M = 51
TARGET_SIZES = (51, 10)
SHAPE = (13, 721, 1440)
REPS = 10
HBM_TBS = 8.0
CUS, LANES = 256, 64
NETWORK = {4: 8, 8: 29, 16: 97, 32: 301, 50: 586, 51: 606, 64: 850}  # padded size -> NINSTR (csrc/wbx_sortnet3_gen.hpp)
PIECE_INSTRUCTIONS = 5   # v_lshl_add_u32 (LDS address), v_cvt_f64_i32 (c), v_cvt_f64_f32, v_add_f64, v_fma_f64
MEMBER_INSTRUCTIONS = 2  # v_cmp_u_f32 and ds_write_b32 (p) / v_cmp_u_f32 and the conversion the walk starts a member with (t)
DIMS = ('level', 'latitude', 'longitude')


def padded(m):
  return next(s for s in sorted(NETWORK) if m <= s)


def point_instructions(m, n):
  pieces = m + n - math.gcd(m, n)
  return NETWORK[padded(m)] + NETWORK[padded(n)] + PIECE_INSTRUCTIONS * pieces + MEMBER_INSTRUCTIONS * (m + n)


def kernel_times(ctx, lines, clock_mhz, shape):
  import torch  # pylint: disable=g-import-not-at-top
  sizes = dict(zip(DIMS, shape))
  npoint = int(np.prod(shape))
  ptr = lambda v: C.c_void_p(int(v))
  g = torch.Generator(device='cuda')
  g.manual_seed(0)
  p = torch.randn((M,) + shape, generator=g, device='cuda')
  lines.append(f'(a) kernel time, {REPS} launches each between event pairs, medians; floors: (M + N) x 4 B per point / {HBM_TBS:.0f} TB/s and '
               f'(NINSTR(M) + NINSTR(N) + {PIECE_INSTRUCTIONS} x pieces + {MEMBER_INSTRUCTIONS} x (M + N)) vector instructions per point / '
               f'({CUS} CUs x {LANES} lanes x {clock_mhz:.0f} MHz)')
  strides = {'level': shape[1] * shape[2], 'latitude': shape[2], 'longitude': 1}
  lay = planner.InputLayout(strides=dict(strides), itemsize=4, base_alignment=256)
  for n in TARGET_SIZES:
    t = torch.randn((n,) + shape, generator=g, device='cuda') + 0.5
    torch.cuda.synchronize()
    nbytes = (M + n) * npoint * 4
    instr = point_instructions(M, n)
    floor_hbm = nbytes / (HBM_TBS * 1e12) * 1e3
    floor_valu = float(npoint) * instr / (CUS * LANES * clock_mhz * 1e6) * 1e3
    lines.append(f'  f32{[M] + list(shape)} against f32{[n] + list(shape)}: {nbytes / 1e9:.2f} GB, {M + n - math.gcd(M, n)} pieces, {instr} instructions '
                 f'per point; floors {floor_hbm:.3f} ms (HBM) and {floor_valu:.3f} ms (VALU)')
    for what, reduce_dims in (('x summed', DIMS[1:]), ('x kept  ', DIMS[1:2])):
      plan = planner.build_s1_plan(DIMS, sizes, [lay, lay, None, None], reduce_dims, wdep_dims=set(), flags=0, allow_vec4=False)
      dplan = engine._PlanOnDevice(ctx, plan)  # pylint: disable=protected-access
      out = ctx.alloc(int(np.prod(plan.partial_shape(_hip.WASS_LANES))) * 8)

      def launch():
        _hip.check(ctx.lib.wbx_ens_wasserstein_partial(ctx.handle, C.byref(dplan.struct), _hip.F32, M, npoint, n, npoint, ptr(p.data_ptr()),
                                                       ptr(t.data_ptr()), None, ptr(out.ptr)), 'wbx_ens_wasserstein_partial')
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
      got = ctx.download(out.ptr, plan.partial_shape(_hip.WASS_LANES), np.float64)
      assert np.isfinite(got).all(), 'non-finite partials'
      lines.append(f'    {what}: {ms:8.3f} ms  = {ms / floor_hbm:5.2f} x the HBM floor ({nbytes / ms / 1e9:5.3f} TB/s), {ms / floor_valu:5.2f} x the VALU floor'
                   f'   plan x_dim={plan.x_dim} nkey={plan.nkey} nchunk={plan.nchunk} depth_chunk={plan.depth_chunk} nx={plan.nx} '
                   f'block={min(plan.block_threads, 128)} (the plan says {plan.block_threads})   mean distance {got.sum() / npoint:.6f}')
    del t
  del p


def _fields(seed, m, n, shape, dtype):
  import torch  # pylint: disable=g-import-not-at-top
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  p = torch.randn((m,) + shape, generator=g, device='cuda', dtype=dtype)
  t = torch.randn((n,) + shape, generator=g, device='cuda', dtype=dtype) + 0.5
  return p, t


def _evaluate(ctx, stat, agg, p, t, coords):
  import torch  # pylint: disable=g-import-not-at-top
  pred = {'v': xr.DataArray(p, dims=('number',) + DIMS, coords=coords)}
  targ = {'v': xr.DataArray(t, dims=('number',) + DIMS, coords=coords)}
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  stats = {stat.unique_name: stat.compute(pred, targ)}
  t1 = time.perf_counter()
  state = agg.aggregate_statistics(stats)
  ctx.synchronize()
  torch.cuda.synchronize()
  t2 = time.perf_counter()
  score = float(np.asarray(state.mean_statistics()[stat.unique_name]['v'].values).ravel()[0])
  return (t1 - t0) * 1e3, (t2 - t1) * 1e3, score


def end_to_end(ctx, lines, route, shape):
  import torch  # pylint: disable=g-import-not-at-top
  coords = {'level': np.arange(shape[0]) * 50.0 + 100.0, 'latitude': np.linspace(-90, 90, shape[1]),
            'longitude': np.linspace(0, 360, shape[2], endpoint=False)}
  stat = probabilistic.WassersteinDistance('number')
  agg = aggregation.Aggregator(reduce_dims=list(DIMS))
  has_switch = hasattr(lazy, 'FUSED_WASSERSTEIN')
  failures = []
  lines.append('(b) end to end, WassersteinDistance of device-resident tensors, every dim reduced: host wall time of compute + '
               'aggregate_statistics up to a synchronise, new tensors every repetition')
  routes = {'both': ((True, 4), (False, 2)), 'fused': ((True, 4),), 'host': ((False, 2),)}[route]
  for n in TARGET_SIZES:
    lines.append(f'  f32{[M] + list(shape)} against f32{[n] + list(shape)}')
    results, medians = {}, {}
    for fused, reps in routes:
      if has_switch:
        lazy.FUSED_WASSERSTEIN = fused
      else:
        assert not fused, 'this checkout has no fused route'
      times = []
      for rep in range(reps + 1):
        p, t = _fields(100 + reps - rep, M, n, shape, torch.float32)  # (the last repetition scores the same fields on every route)
        st, ag, score = _evaluate(ctx, stat, agg, p, t, coords)
        if rep:  # (the first repetition builds plans and weight tables)
          times.append((st, ag))
        del p, t
        torch.cuda.empty_cache()
      results[fused] = score
      st, ag = np.median([a for a, _ in times]), np.median([b for _, b in times])
      medians[fused] = st + ag
      name = 'fused (wbx_ens_wasserstein_partial)' if fused else ('host route (WBX_FUSED_WASSERSTEIN=0)' if has_switch else 'host route (no fused route here)')
      lines.append(f'    {name:38s}: statistics {st:9.2f} ms   aggregate_statistics {ag:9.2f} ms   total {st + ag:9.2f} ms   ({reps} repetitions, medians)'
                   f'   score {results[fused]:.15f}')
    if len(results) == 2:
      # per point both routes are within (M + N + 4) 2^-53 of the exact value, relatively (tests/wasserstein_cases.py), and so are the
      # means of these non-negative values up to the summation's own n 2^-53: 1e-12 of the score leaves two digits to spare
      err, bound = abs(results[True] - results[False]), 1e-12 * abs(results[False])
      lines.append(f'    |score fused - score host route| = {err:.3e} (bound {bound:.3e});  host route / fused = {medians[False] / medians[True]:.1f} x '
                   '(gate: more than 1.08 x, the box-to-box spread)')
      if not err <= bound:
        failures.append(f'N = {n}: the scores of the two routes differ by {err:.3e}, more than the bound {bound:.3e}')
      if not medians[False] > 1.08 * medians[True]:
        failures.append(f'N = {n}: the fused route does not win by more than the box-to-box spread')
  small = (3, 24, 36)
  coords = {'level': np.arange(3) * 50.0, 'latitude': np.linspace(-80, 80, small[1]), 'longitude': np.linspace(0, 360, small[2], endpoint=False)}
  scores = {}
  for fused in ((True, False) if has_switch and route == 'both' else (False,)):
    if has_switch:
      lazy.FUSED_WASSERSTEIN = fused
    p, t = _fields(7, M, 10, small, torch.float64)
    scores[fused] = _evaluate(ctx, stat, agg, p, t, coords)[2]
    engine.clear_caches()
  if has_switch:
    lazy.FUSED_WASSERSTEIN = True
  lines.append(f'(c) float64 f64{[M] + list(small)} against f64{[10] + list(small)}: host route score {scores[False]!r}' + (
      f', fused {scores[True]!r}, relative difference {abs(scores[True] - scores[False]) / abs(scores[False]):.3e} (bound 1e-12)' if True in scores else ''))
  if True in scores and not abs(scores[True] - scores[False]) <= 1e-12 * abs(scores[False]):
    failures.append('the float64 scores of the two routes differ by more than 1e-12 of the score')
  return failures


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'wasserstein_kbench.txt'))
  ap.add_argument('--skip-kernel', action='store_true')
  ap.add_argument('--skip-e2e', action='store_true')
  ap.add_argument('--e2e-route', choices=('both', 'fused', 'host'), default='both')
  ap.add_argument('--e2e-shape', type=int, nargs=3, default=SHAPE, metavar=('NLEVEL', 'NLAT', 'NLON'))
  args = ap.parse_args()
  ctx = _hip.default_context()
  clock = ctx.clock_probe()
  lines = [f'tools/bench_wasserstein.py on {ctx.device_name()}; wbx_clock_probe {clock:.0f} MHz before']
  if not args.skip_kernel:
    kernel_times(ctx, lines, clock, SHAPE)
  failures = [] if args.skip_e2e else end_to_end(ctx, lines, args.e2e_route, tuple(args.e2e_shape))
  lines.append(f'wbx_clock_probe {ctx.clock_probe():.0f} MHz after')
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(args.out, 'w') as f:
    f.write(text)
  if failures:  # (the figures are on file either way)
    sys.exit('; '.join(failures))


if __name__ == '__main__':
  main()
