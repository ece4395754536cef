// Wasserstein-1 distance between an ensemble of predictions and an ensemble of targets, summed like any other stage-1 statistic:
// WassersteinDistance (weatherbenchX/metrics/probabilistic.py) without the pooled float64 sort and the cumulative sums of the
// host route.
//
// Reference semantics restated.  Per point, with the sorted members p_(0) <= ... <= p_(M-1) and t_(0) <= ... <= t_(N-1):
//   W1 = int_0^1 |Qp(u) - Qt(u)| du = ( sum over pieces of c |p_(i) - t_(j)| ) / (M N)
// The pieces are the M + N - gcd(M, N) intervals between consecutive breakpoints of {i / M} u {j / N}; in units of 1 / (M N) a
// piece is c = min((i + 1) N, (j + 1) M) - max(i N, j M) long, i advances when (i + 1) N <= (j + 1) M and j when
// (j + 1) M <= (i + 1) N.  The sequence (i, j, c) depends on (M, N) only: it is wave-uniform and lives in scalar registers.
// Non-finite members follow what the pooled form of the reference makes of them: a NaN member on either side makes the point
// NaN, so do two or more +inf among the pooled M + N members and two or more -inf (the pooled form has an inf - inf gap); anything
// else is what the arithmetic gives (+inf for a single infinity of either sign, or one of each).  The quantile walk alone would
// not say so (p = [inf, inf], t = [0] gives +inf), hence the decision is explicit: a NaN flag gathered while the members are
// loaded, and the infinities of each sign counted -- up to two a side, which is all the rule asks -- at the ends of the sorted
// members, before any padding is looked at.
//
// Mapping.  One point per lane.  The M members of p are loaded into registers, padded with +inf to the next generated network size
// (4, 8, 16, 32, 50, 51, 64) and sorted there (SortNet3, wbx_sortnet3_gen.hpp; exact in the input type); the sorted column is
// parked in LDS member-major, element k of thread l at [k][l] (4-byte elements: bank = lane; 8-byte ones: two conflict-free
// halves).  t is loaded and sorted in the same registers.  The walk runs over j unrolled (t_(j) in a register) with a scalar
// i, reading the LDS column at the wave-uniform row i: no lane-dependent control flow, no register indexed at run time.  The
// padded sizes are dispatched inside the kernel (they are wave-uniform), so there are two kernels per dtype, not one per (M, N).
//
// Arithmetic: differences, their absolute values, the products with the integer c and the sum in float64 -- a piece is one rounded
// difference and one fused multiply-add onto the sum (v_fma_f64 with |d| as a source modifier: five vector instructions a piece) --,
// the sum in the order of the walk, one division by (double)(M N).  The result is a function of the inputs
// and the plan only: a lane adds its points in the order they come, lanes and waves are summed in fixed orders, no atomics.
#include "wbx_ens_park.hpp"  // the sort and the LDS column (wass_load_sort, wass_park)

namespace wbx {

struct WassArgs {
  int64_t tms;         // element stride between target members
  int32_t N, np, nt;   // target ensemble size; M and N padded to a generated network size
};

// The smallest generated network that holds m members (tests/wasserstein_cases.py restates it).
static inline int wass_padded(int m) {
  const int sizes[] = {4, 8, 16, 32, 50, 51, 64};
  for (int s : sizes)
    if (m <= s) return s;
  return 0;
}

// How many of a side's two largest (smallest) sorted members are +inf (-inf): the count of that side's infinities, capped at 2.
template <typename T>
__device__ __forceinline__ void wass_count_inf(int n, T lo1, T lo2, T hi1, T hi2, int& npos, int& nneg) {
  const T inf = (T)__builtin_huge_val();
  npos += (hi1 == inf) + (n > 1 && hi2 == inf);
  nneg += (lo1 == -inf) + (n > 1 && lo2 == -inf);
}

// Sum over the pieces of c |p_(i) - t_(j)|, p_(i) from the parked column, and the ends of the sorted t.
template <typename T, int NS>
__device__ __forceinline__ double wass_walk(const T* tp, int64_t stride, int M, int N, const T* col, int cs, bool& nan, int& npos,
                                            int& nneg) {
  T x[NS];
  wass_load_sort<T, NS>(tp, stride, N, x, nan);
  T hi1 = x[0], hi2 = x[0];
  double s = 0.0;
  int i = 0;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    if (j < N) {
      if (j == N - 1) hi1 = x[j];
      if (j == N - 2) hi2 = x[j];
      const double tj = (double)x[j];
      const int jm1 = (j + 1) * M;
      for (;;) {
        const int in0 = i * N, in1 = in0 + N;
        const int c = (in1 < jm1 ? in1 : jm1) - (in0 > j * M ? in0 : j * M);
        s = fma((double)c, fabs((double)col[i * cs] - tj), s);
        i += in1 <= jm1 ? 1 : 0;
        if (jm1 <= in1) break;
      }
    }
  }
  wass_count_inf<T>(N, x[0], x[NS > 1 ? 1 : 0], hi1, hi2, npos, nneg);
  return s;
}

// W1 of the point x of the row at ro[]; `col` is the thread's LDS column, `cs` its row stride in elements.
template <typename T>
__device__ __forceinline__ double wass_point(const S1Args& a, const WassArgs& e, const int64_t (&ro)[WBX_MAX_INPUTS], int64_t x, T* col,
                                             int cs) {
  const T* pp = reinterpret_cast<const T*>(a.in[0]) + ro[0] + x * a.xstride[0];
  const T* tp = reinterpret_cast<const T*>(a.in[1]) + ro[1] + x * a.xstride[1];
  const int M = a.M, N = e.N;
  bool nan = false;
  switch (e.np) {
    case 4: wass_park<T, 4>(pp, a.mstride, M, col, cs, nan); break;
    case 8: wass_park<T, 8>(pp, a.mstride, M, col, cs, nan); break;
    case 16: wass_park<T, 16>(pp, a.mstride, M, col, cs, nan); break;
    case 32: wass_park<T, 32>(pp, a.mstride, M, col, cs, nan); break;
    case 50: wass_park<T, 50>(pp, a.mstride, M, col, cs, nan); break;
    case 51: wass_park<T, 51>(pp, a.mstride, M, col, cs, nan); break;
    default: wass_park<T, 64>(pp, a.mstride, M, col, cs, nan); break;
  }
  int npos = 0, nneg = 0;
  wass_count_inf<T>(M, col[0], col[(M > 1 ? 1 : 0) * cs], col[(M - 1) * cs], col[(M > 1 ? M - 2 : 0) * cs], npos, nneg);
  double s;
  switch (e.nt) {
    case 4: s = wass_walk<T, 4>(tp, e.tms, M, N, col, cs, nan, npos, nneg); break;
    case 8: s = wass_walk<T, 8>(tp, e.tms, M, N, col, cs, nan, npos, nneg); break;
    case 16: s = wass_walk<T, 16>(tp, e.tms, M, N, col, cs, nan, npos, nneg); break;
    case 32: s = wass_walk<T, 32>(tp, e.tms, M, N, col, cs, nan, npos, nneg); break;
    case 50: s = wass_walk<T, 50>(tp, e.tms, M, N, col, cs, nan, npos, nneg); break;
    case 51: s = wass_walk<T, 51>(tp, e.tms, M, N, col, cs, nan, npos, nneg); break;
    default: s = wass_walk<T, 64>(tp, e.tms, M, N, col, cs, nan, npos, nneg); break;
  }
  const double w = s / (double)(M * N);
  return (nan || npos > 1 || nneg > 1) ? __builtin_nan("") : w;
}

// The decision per point, on the assembled value: the sum, then the count lane of a mask or of skipna.
struct WassSums {
  double s = 0.0, c = 0.0;
};

__device__ __forceinline__ void wass_account(const S1Args& a, const int64_t (&ro)[WBX_MAX_INPUTS], int64_t x, double v, WassSums& acc) {
  const bool valid = !(a.flags & WBX_FLAG_MASKED) || reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + x * a.xstride[3]] != 0;
  const bool g = valid && (!(a.flags & WBX_FLAG_SKIPNA) || v == v);  // (a NaN under a valid point poisons its partial)
  acc.s += g ? v : 0.0;
  acc.c += g ? 1.0 : 0.0;
}

extern __shared__ __attribute__((aligned(16))) unsigned char wass_lds[];  // [np][blockDim.x] elements of T

// x summed.  grid = nkey * nchunk; the waves of a block interleave over the chunk's rows, a lane sweeps a row 64 points apart.
template <typename T>
__global__ void __launch_bounds__(WASS_THREADS<T>) wass_xr_kernel(S1Args a, WassArgs e, int nacc) {
  T* col = reinterpret_cast<T*>(wass_lds) + threadIdx.x;
  const int cs = blockDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  WassSums acc;
  for (int64_t d = d0 + wave; d < d1; d += nwave) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, d, ro);
    for (int64_t x = lane; x < a.nx; x += 64) wass_account(a, ro, x, wass_point<T>(a, e, ro, x, col, cs), acc);
  }
  __shared__ double red[2][2];
  const double ws = wave_sum(acc.s), wc = wave_sum(acc.c);
  if (lane == 0) {
    red[wave][0] = ws;
    red[wave][1] = wc;
  }
  __syncthreads();
  if ((int)threadIdx.x < nacc) {
    double s = 0.0;
    for (int w = 0; w < nwave; ++w) s += red[w][threadIdx.x];
    a.out[(key * a.nchunk + chunk) * (int64_t)nacc + threadIdx.x] = s;
  }
}

// x kept.  grid = nkey * nxtile * nchunk; a lane owns one x and walks the chunk's rows.
template <typename T>
__global__ void __launch_bounds__(WASS_THREADS<T>) wass_xk_kernel(S1Args a, WassArgs e, int nacc) {
  T* col = reinterpret_cast<T*>(wass_lds) + threadIdx.x;
  const int cs = blockDim.x;
  int64_t b = blockIdx.x;
  const int chunk = (int)(b % a.nchunk);
  b /= a.nchunk;
  const int xt = (int)(b % a.nxtile);
  const int64_t key = b / a.nxtile;
  const int64_t x = (int64_t)xt * blockDim.x + threadIdx.x;
  if (x >= a.nx) return;
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  WassSums acc;
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, d, ro);
    wass_account(a, ro, x, wass_point<T>(a, e, ro, x, col, cs), acc);
  }
  double* o = a.out + ((key * a.nchunk + chunk) * (int64_t)nacc) * a.nx + x;
  o[0] = acc.s;
  if (nacc > 1) o[a.nx] = acc.c;
}

// A block runs the plan's threads up to what the column store holds (WASS_THREADS); the partial's layout does not depend on it.
template <typename T>
static int wass_launch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const WassArgs& e, int nacc) {
  const int threads = plan->block_threads < WASS_THREADS<T> ? plan->block_threads : WASS_THREADS<T>;
  const size_t lds = (size_t)e.np * threads * sizeof(T);
  int64_t grid;
  if (int rc = s1_grid(plan, plan->x_kept ? threads : 0, a, &grid)) return rc;
  hipLaunchKernelGGL(plan->x_kept ? wass_xk_kernel<T> : wass_xr_kernel<T>, dim3((unsigned)grid), dim3(threads), lds, ctx->stream, a, e,
                     nacc);
  WBX_HIP(hipGetLastError());
  return 0;
}

}  // namespace wbx

extern "C" int wbx_ens_wasserstein_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride, int N,
                                           int64_t target_member_stride, const void* p, const void* t, const uint8_t* mask,
                                           double* partial_out) {
  using namespace wbx;
  const S1Names names = {"wbx_ens_wasserstein_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  WBX_REQUIRE(M >= 1 && M <= WBX_WASS_MAX_MEMBERS && N >= 1 && N <= WBX_WASS_MAX_MEMBERS,
              "wbx_ens_wasserstein_partial: 1..%d members a side (got %d, %d)", WBX_WASS_MAX_MEMBERS, M, N);
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "wbx_ens_wasserstein_partial: unknown dtype %d", dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA)), "wbx_ens_wasserstein_partial: flags other than MASKED | SKIPNA (0x%x)",
              plan->flags);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "wbx_ens_wasserstein_partial: no plane mode, no folded x weights");
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, WBX_WASS_LANES);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  a.M = M;
  a.mstride = member_stride;
  WassArgs e;
  e.tms = target_member_stride;
  e.N = N;
  e.np = wass_padded(M);
  e.nt = wass_padded(N);
  if (dtype == WBX_F32) return wass_launch<float>(ctx, plan, a, e, nacc);
  return wass_launch<double>(ctx, plan, a, e, nacc);
}
