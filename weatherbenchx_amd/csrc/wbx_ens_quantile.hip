// Errors of ensemble quantiles, summed like any other stage-1 statistic: the error, the absolute error and the squared error of
// (the q_j quantile of a point's members) against (the target), per quantile level.
//
// Reference semantics restated (include/wbx.h has them in full): the chain of weatherbenchX/metrics/wrappers.py
//   EnsembleQuantiles('predictions', quantiles)   NumPy's `linear` quantile over the member dim, along a new leading quantile dim
// in front of Error / AbsoluteError / SquaredError (deterministic.py:91-123): MAE of the ensemble median, Bias / MSE / RMSE of
// deciles.  Per point the members are sorted in the input type, quantile j with the host's bound (k_j, g_j) is qerr_quantile below
// (NumPy's order of operations and NumPy's types, no fused multiply-add, NaN by the flag gathered while the members are loaded),
// e_j = q_j - (double)t, and the value lanes stat * nq + j hold e_j, |e_j| and e_j * e_j.
// NumPy's types: np.quantile subtracts the two neighbours BEFORE the float64 weight joins, so d = B - A is a difference in the
// members' type -- rounded to float32 for float32 members -- and everything after it is float64.  ivl_quantile (the interval
// statistics) widens the neighbours first; here the number has to be the host route's, bit for bit, so d is formed as NumPy forms it.
//
// Mapping.  One point per lane, as wbx_ens_interval.hip: the M members are loaded into registers, padded with +inf to the next
// generated network size and sorted there, the sorted column is parked in LDS member-major, and the two order statistics of each
// bound are read back at wave-uniform rows k and min(k + 1, M - 1): no register is indexed at run time, no lane-dependent control
// flow (a masked point is sorted like any other and adds 0).  The bounds are kernel arguments; the kernels are built for 1, 4, 8
// and 16 quantile slots and a launch takes the smallest that holds nq (dispatch_slots), so the median alone does not carry 64
// accumulators across the sort.  The padded sizes are dispatched inside the kernel.  A full sort is more than a handful of order
// statistics need: a network pruned to the wanted ranks is the tuning left.
//
// Sums are float64, a lane adds its points in the order they come, lanes (wave_sum's butterfly) and waves are summed in fixed
// orders, no atomics.  e_j, |e_j| and e_j^2 are NaN together, so a lane keeps ONE count per quantile and writes it to the three
// count lanes of that quantile.
#include "wbx_ens_park.hpp"

namespace wbx {

static_assert(WBX_IVL_MAX_MEMBERS == WBX_WASS_MAX_MEMBERS, "the column store of wbx_ens_park.hpp is sized for this many members");
static_assert(WBX_QERR_STATS == 3 && WBX_QERR_MAX_QUANTILES == 16, "dispatch_slots' largest instantiation; three sums per quantile");

constexpr int QERR_ERR = 0, QERR_ABS = 1, QERR_SQ = 2;  // value lane stat * nq + j
constexpr int QERR_MAX_WAVES = 2;                       // WASS_THREADS<float> / 64

struct QerrArgs {
  wbx_ivl_bound b[WBX_QERR_MAX_QUANTILES];  // host values; c_off is not read
  int32_t nq;
  int32_t np;  // M padded to a generated network size
};

// NumPy's linear quantile of the parked sorted column at the bound b, as np.quantile gives it for members of type T; `nan`: the point
// has a NaN member.
template <typename T>
__device__ __forceinline__ double qerr_quantile(const T* col, int cs, int M, const wbx_ivl_bound& b, bool nan) {
#pragma clang fp contract(off)
  const int k1 = b.k + 1 < M ? b.k + 1 : M - 1;
  const T lo = col[b.k * cs], hi = col[k1 * cs];
  const T dt = hi - lo;  // in the members' type, as NumPy's subtract(b, a) is
  const double A = (double)lo, B = (double)hi, d = (double)dt;
  const double up = d * b.g, down = d * (1.0 - b.g);
  const double q = b.g < 0.5 ? A + up : B - down;
  return nan ? __builtin_nan("") : q;
}

// One lane's sums: per statistic and quantile slot, the good (valid, non-NaN) points per slot, the valid points.
template <int NQ>
struct QerrSums {
  double s[WBX_QERR_STATS][NQ], good[NQ], valid;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < NQ; ++j) s[QERR_ERR][j] = s[QERR_ABS][j] = s[QERR_SQ][j] = good[j] = 0.0;
    valid = 0.0;
  }
};

// The point x of the row at ro[] into the lane's sums.  Slots j >= nq are not touched.
template <typename T, int NQ>
__device__ __forceinline__ void qerr_point(const S1Args& a, const QerrArgs& e, const int64_t (&ro)[WBX_MAX_INPUTS], int64_t x, T* col,
                                           int cs, QerrSums<NQ>& acc) {
#pragma clang fp contract(off)
  const T* pp = reinterpret_cast<const T*>(a.in[0]) + ro[0] + x * a.xstride[0];
  const int M = a.M;
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
  const double t = (double)ld_stream(reinterpret_cast<const T*>(a.in[1]) + ro[1] + x * a.xstride[1]);
  const bool valid = !(a.flags & WBX_FLAG_MASKED) || reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + x * a.xstride[3]] != 0;
  const bool skipna = a.flags & WBX_FLAG_SKIPNA;
  acc.valid += valid ? 1.0 : 0.0;
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    if (j < e.nq) {
      const double q = qerr_quantile<T>(col, cs, M, e.b[j], nan);
      const double err = q - t;
      const double sq = err * err;  // (rounded here: the sum below adds a number, not a product)
      const bool take = valid && (!skipna || err == err);
      acc.s[QERR_ERR][j] += take ? err : 0.0;
      acc.s[QERR_ABS][j] += take ? fabs(err) : 0.0;
      acc.s[QERR_SQ][j] += take ? sq : 0.0;
      acc.good[j] += take ? 1.0 : 0.0;
    }
  }
}

// Where lane i of a partial comes from among [stat * NQ + j | 3 NQ + j: good | 4 NQ: valid]: the value lanes stat * nq + j, then
// one count lane per value lane under skipna, one for all under a mask alone.
template <int NQ>
__device__ __forceinline__ int qerr_source(int i, int nq, uint32_t flags) {
  const int nl = WBX_QERR_STATS * nq;
  if (i < nl) return (i / nq) * NQ + i % nq;
  return (flags & WBX_FLAG_SKIPNA) ? WBX_QERR_STATS * NQ + (i - nl) % nq : 4 * NQ;
}

extern __shared__ __attribute__((aligned(16))) unsigned char qerr_lds[];  // [np][blockDim.x] elements of T

// x summed.  grid = nkey * nchunk; the waves of a block interleave over the chunk's rows, a lane sweeps a row 64 points apart.
template <typename T, int NQ>
__global__ void __launch_bounds__(WASS_THREADS<T>) qerr_xr_kernel(S1Args a, QerrArgs e, int nacc) {
  T* col = reinterpret_cast<T*>(qerr_lds) + threadIdx.x;
  const int cs = blockDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  QerrSums<NQ> acc;
  acc.clear();
  for (int64_t d = d0 + wave; d < d1; d += nwave) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, d, ro);
    for (int64_t x = lane; x < a.nx; x += 64) qerr_point<T, NQ>(a, e, ro, x, col, cs, acc);
  }
  constexpr int NRED = 4 * NQ + 1;
  __shared__ double red[QERR_MAX_WAVES][NRED];
#pragma unroll
  for (int st = 0; st < WBX_QERR_STATS; ++st) {
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const double s = wave_sum(acc.s[st][j]);
      if (lane == 0) red[wave][st * NQ + j] = s;
    }
  }
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const double s = wave_sum(acc.good[j]);
    if (lane == 0) red[wave][WBX_QERR_STATS * NQ + j] = s;
  }
  {
    const double s = wave_sum(acc.valid);
    if (lane == 0) red[wave][4 * NQ] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nacc; i += blockDim.x) {  // (up to 96 lanes, and a float64 block has 64 threads)
    const int src = qerr_source<NQ>(i, e.nq, a.flags);
    double s = 0.0;
    for (int w = 0; w < nwave; ++w) s += red[w][src];
    a.out[(key * a.nchunk + chunk) * (int64_t)nacc + i] = s;
  }
}

// x kept.  grid = nkey * nxtile * nchunk; a lane owns one x and walks the chunk's rows.
template <typename T, int NQ>
__global__ void __launch_bounds__(WASS_THREADS<T>) qerr_xk_kernel(S1Args a, QerrArgs e, int nacc) {
  T* col = reinterpret_cast<T*>(qerr_lds) + threadIdx.x;
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
  QerrSums<NQ> acc;
  acc.clear();
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, d, ro);
    qerr_point<T, NQ>(a, e, ro, x, col, cs, acc);
  }
  double* o = a.out + ((key * a.nchunk + chunk) * (int64_t)nacc) * a.nx + x;
  const bool skipna = a.flags & WBX_FLAG_SKIPNA;
  const int nl = WBX_QERR_STATS * e.nq;
#pragma unroll
  for (int st = 0; st < WBX_QERR_STATS; ++st) {
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      if (j < e.nq) {
        o[(int64_t)(st * e.nq + j) * a.nx] = acc.s[st][j];
        if (skipna) o[(int64_t)(nl + st * e.nq + j) * a.nx] = acc.good[j];
      }
    }
  }
  if (!skipna && (a.flags & WBX_FLAG_MASKED)) o[(int64_t)nl * a.nx] = acc.valid;
}

// A block runs the plan's threads up to what the column store holds (WASS_THREADS); the partial's layout does not depend on it.
template <typename T>
static int qerr_launch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const QerrArgs& e, int nacc) {
  const int threads = plan->block_threads < WASS_THREADS<T> ? plan->block_threads : WASS_THREADS<T>;
  const size_t lds = (size_t)e.np * threads * sizeof(T);
  int64_t grid;
  if (int rc = s1_grid(plan, plan->x_kept ? threads : 0, a, &grid)) return rc;
  return dispatch_slots(e.nq, [&](auto nq) {
    constexpr int NQ = decltype(nq)::value;
    void (*kernel)(S1Args, QerrArgs, int) = qerr_xr_kernel<T, NQ>;
    if (plan->x_kept) kernel = qerr_xk_kernel<T, NQ>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds, ctx->stream, a, e, nacc);
    WBX_HIP(hipGetLastError());
    return 0;
  });
}

}  // namespace wbx

extern "C" int wbx_ens_quantile_error_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride, int nq,
                                              const wbx_ivl_bound* bounds, const void* p, const void* t, const uint8_t* mask,
                                              double* partial_out) {
  using namespace wbx;
  const S1Names names = {"wbx_ens_quantile_error_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  WBX_REQUIRE(M >= 1 && M <= WBX_IVL_MAX_MEMBERS, "wbx_ens_quantile_error_partial: 1..%d members (got %d)", WBX_IVL_MAX_MEMBERS, M);
  WBX_REQUIRE(nq >= 1 && nq <= WBX_QERR_MAX_QUANTILES, "wbx_ens_quantile_error_partial: 1..%d quantiles per launch (got %d)",
              WBX_QERR_MAX_QUANTILES, nq);
  WBX_REQUIRE(bounds != nullptr, "wbx_ens_quantile_error_partial: bounds is NULL");
  QerrArgs e;
  memset(&e, 0, sizeof(e));
  for (int j = 0; j < nq; ++j) {
    WBX_REQUIRE(bounds[j].k >= 0 && bounds[j].k < M, "wbx_ens_quantile_error_partial: rank %d outside 0..%d", (int)bounds[j].k, M - 1);
    WBX_REQUIRE(bounds[j].g >= 0.0 && bounds[j].g < 1.0, "wbx_ens_quantile_error_partial: weight %g outside [0, 1)", bounds[j].g);
    e.b[j].k = bounds[j].k;
    e.b[j].g = bounds[j].g;
  }
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "wbx_ens_quantile_error_partial: unknown dtype %d", dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA)),
              "wbx_ens_quantile_error_partial: flags other than MASKED | SKIPNA (0x%x)", plan->flags);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "wbx_ens_quantile_error_partial: no plane mode, no folded x weights");
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, WBX_QERR_STATS * nq);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  a.M = M;
  a.mstride = member_stride;
  e.nq = nq;
  e.np = ivl_padded(M);
  if (dtype == WBX_F32) return qerr_launch<float>(ctx, plan, a, e, nacc);
  return qerr_launch<double>(ctx, plan, a, e, nacc);
}
