// Ranked probability score of an ensemble against a scalar target at a list of thresholds, summed like any other stage-1
// statistic: EnsembleRankedProbabilityScore (weatherbenchX/metrics/probabilistic.py:339-477) without the [K, M, frame] indicator
// arrays of its ContinuousToCDF transforms (wrappers.py).
//
// Reference semantics restated.  Per point, members x_0 .. x_{M-1}, target y, K prediction thresholds a_k, K target thresholds b_k:
//   c_k = #{m : x_m <= a_k}     o_k = [y <= b_k]            (< instead of <= when right_inclusive is false)
//   fair:    n_k = (M - 1) (c_k - o_k M)^2 - c_k (M - c_k)    D = M^2 (M - 1)     = (mean - o)^2 - var(ddof = 1) / M of a 0/1 sample
//   unfair:  n_k = (c_k - o_k M)^2                            D = M^2
//   RPS(point) = (sum_k n_k) / D;  NaN where a member or the target is NaN (sum(bin_dim, skipna=False) of NaN terms)
//
// Nothing here is floating-point accumulation.  A lane keeps the K counts of its point in registers while it walks the members
// (one compare and one add-with-carry per member and threshold, the thresholds wave-uniform in SGPRs), forms the point's integer
// numerator (|sum_k n_k| < 2^31 for M <= 256, K <= 16) and adds it to an int64 of its own.  A partial is that int64 sum S over
// its points, written once as (double)S / (double)D: the correctly rounded quotient of two integers (|S| < 2^53 is required of the
// plan), a function of the inputs and the plan only.
// x summed: a lane owns a point of the row, the end is an integer wave reduction and an integer sum over the block's waves
// through LDS.  x kept: a lane owns an x and walks the chunk's rows; no cross-lane traffic.
#include <cmath>
#include <type_traits>

#include "wbx_s1.hpp"

namespace wbx {

constexpr int ERPS_MAX_WAVES = 4;
constexpr int ERPS_FLIGHT = 8;  // member loads in flight per lane

// Threshold k as the type the compare runs in, wave-uniform (SGPRs).  float: for every float32 x
//   x <= thr (in float64) <=> x <= rd(thr) (in float32), rd = rounding toward -inf   (cont_threshold of wbx_contingency.hip)
//   x <  thr (in float64) <=> x <  ru(thr) (in float32), ru = rounding toward +inf
// and rounding to nearest is equivalent to neither (float(0.1) <= 0.1 is false).  Beyond the float32 range rd gives FLT_MAX /
// -inf and ru +inf / -FLT_MAX, which decide right as well.
template <typename T, bool RIGHT>
__device__ __forceinline__ T erps_threshold(const double* thr, int k) {
  const double v = ((const_ptr<double>)thr)[k];
  if constexpr (std::is_same<T, double>::value) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
  } else {
    float f = (float)v;  // to nearest
    const uint32_t b = __float_as_uint(f);
    if constexpr (RIGHT) {
      if ((double)f > v) f = __uint_as_float(f > 0.f ? b - 1u : (f < 0.f ? b + 1u : 0x80000001u));  // one step down
    } else {
      if ((double)f < v) f = __uint_as_float(f > 0.f ? b + 1u : (f < 0.f ? b - 1u : 0x00000001u));  // one step up
    }
    return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(f)));
  }
}

template <bool RIGHT, typename T>
__device__ __forceinline__ bool erps_below(T x, T thr) {
  if constexpr (RIGHT)
    return x <= thr;
  else
    return x < thr;
}

// The integer numerator sum_k n_k of the point whose members start at `pm` (element stride `ms`) and whose target is `y`;
// `nan` says whether a member or the target is NaN (the numerator is then meaningless).  Slots k >= nthr are skipped.
template <typename T, int NT, bool RIGHT>
__device__ __forceinline__ int32_t erps_point(const T* pm, int64_t ms, int M, T y, const T (&pa)[NT], const T (&tb)[NT], int nthr,
                                              bool fair, bool& nan) {
  int32_t c[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) c[q] = 0;
  bool bad = y != y;
  int m = 0;
  for (; m + ERPS_FLIGHT <= M; m += ERPS_FLIGHT) {
    T v[ERPS_FLIGHT];
#pragma unroll
    for (int u = 0; u < ERPS_FLIGHT; ++u) v[u] = ld_stream(pm + (int64_t)(m + u) * ms);
#pragma unroll
    for (int u = 0; u < ERPS_FLIGHT; ++u) {
      bad |= v[u] != v[u];
#pragma unroll
      for (int q = 0; q < NT; ++q) c[q] += erps_below<RIGHT>(v[u], pa[q]) ? 1 : 0;
    }
  }
  if (m < M) {  // the last, short group: the loads past the end re-read the last member and are not counted
    T v[ERPS_FLIGHT];
#pragma unroll
    for (int u = 0; u < ERPS_FLIGHT; ++u) v[u] = ld_stream(pm + (int64_t)(m + u < M ? m + u : M - 1) * ms);
#pragma unroll
    for (int u = 0; u < ERPS_FLIGHT; ++u) {
      if (m + u < M) {
        bad |= v[u] != v[u];
#pragma unroll
        for (int q = 0; q < NT; ++q) c[q] += erps_below<RIGHT>(v[u], pa[q]) ? 1 : 0;
      }
    }
  }
  nan = bad;
  int32_t n = 0;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    if (q < nthr) {
      const int32_t e = c[q] - (erps_below<RIGHT>(y, tb[q]) ? M : 0);
      n += fair ? (M - 1) * e * e - c[q] * (M - c[q]) : e * e;
    }
  }
  return n;
}

// One partial from its integer sums: S = sum of the numerators over the good (valid, non-NaN) points.
__device__ __forceinline__ void erps_write(double* o, int64_t nj, uint32_t flags, double denom, int64_t s, int64_t ngood,
                                           int64_t nvalid) {
  const bool skipna = flags & WBX_FLAG_SKIPNA;
  const bool poisoned = !skipna && ngood != nvalid;  // a NaN under a valid point
  o[0] = poisoned ? (double)NAN : (double)s / denom;
  if (skipna)
    o[nj] = (double)ngood;
  else if (flags & WBX_FLAG_MASKED)
    o[nj] = (double)nvalid;
}

// x summed.  grid = nkey * nchunk, block = plan->block_threads; rows are dealt to the waves as in s1_xr_kernel.
template <typename T, int NT, bool RIGHT>
__global__ void __launch_bounds__(256) erps_xr_kernel(S1Args a, const double* pthr, const double* tthr, int nthr, int nacc,
                                                      double denom) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwave = blockDim.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const bool masked = a.flags & WBX_FLAG_MASKED, fair = a.flags & WBX_FLAG_FAIR;

  T pa[NT], tb[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    pa[q] = erps_threshold<T, RIGHT>(pthr, q < nthr ? q : 0);
    tb[q] = erps_threshold<T, RIGHT>(tthr, q < nthr ? q : 0);
  }
  int64_t sum = 0, ngood = 0, nvalid = 0;

  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  for (int64_t dbatch = d0 + wave; dbatch < d1; dbatch += (int64_t)64 * nwave) {
    // lane l resolves the wave's l-th row; the sweep broadcasts the results (s1_xr_kernel)
    const int64_t dmine = dbatch + (int64_t)lane * nwave;
    int64_t rov[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, dmine < d1 ? dmine : d1 - 1, rov);
    const int64_t left = (d1 - dbatch + nwave - 1) / nwave;
    const int nrow = (int)(left < 64 ? left : 64);
    for (int l = 0; l < nrow; ++l) {
      int64_t ro[WBX_MAX_INPUTS];
#pragma unroll
      for (int i = 0; i < WBX_MAX_INPUTS; ++i) ro[i] = (i < 2 || i == 3) ? readlane64(rov[i], l) : 0;
      for (int64_t x = lane; x < a.nx; x += 64) {
        if (masked && reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + x * a.xstride[3]] == 0) continue;
        const T y = ld_stream(reinterpret_cast<const T*>(a.in[1]) + ro[1] + x * a.xstride[1]);
        bool nan;
        const int32_t n = erps_point<T, NT, RIGHT>(reinterpret_cast<const T*>(a.in[0]) + ro[0] + x * a.xstride[0], a.mstride, a.M, y,
                                                   pa, tb, nthr, fair, nan);
        nvalid += 1;
        ngood += nan ? 0 : 1;
        sum += nan ? 0 : n;
      }
    }
  }

  __shared__ int64_t red[ERPS_MAX_WAVES][3];
  sum = wave_sum_i64(sum);
  ngood = wave_sum_i64(ngood);
  nvalid = wave_sum_i64(nvalid);
  if (lane == 0) {
    red[wave][0] = sum;
    red[wave][1] = ngood;
    red[wave][2] = nvalid;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t s[3] = {0, 0, 0};
    for (int w = 0; w < nwave; ++w) {
      s[0] += red[w][0];
      s[1] += red[w][1];
      s[2] += red[w][2];
    }
    erps_write(a.out + (key * a.nchunk + chunk) * (int64_t)nacc, 1, a.flags, denom, s[0], s[1], s[2]);
  }
}

// x kept.  grid = nkey * nxtile * nchunk, block = plan->block_threads, one x per lane.
template <typename T, int NT, bool RIGHT>
__global__ void __launch_bounds__(256) erps_xk_kernel(S1Args a, const double* pthr, const double* tthr, int nthr, int nacc,
                                                      double denom) {
  int64_t b = blockIdx.x;
  const int chunk = (int)(b % a.nchunk);
  b /= a.nchunk;
  const int xt = (int)(b % a.nxtile);
  const int64_t key = b / a.nxtile;
  const int64_t x = (int64_t)xt * blockDim.x + threadIdx.x;
  if (x >= a.nx) return;
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const bool masked = a.flags & WBX_FLAG_MASKED, fair = a.flags & WBX_FLAG_FAIR;

  T pa[NT], tb[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    pa[q] = erps_threshold<T, RIGHT>(pthr, q < nthr ? q : 0);
    tb[q] = erps_threshold<T, RIGHT>(tthr, q < nthr ? q : 0);
  }
  int64_t sum = 0, ngood = 0, nvalid = 0;

  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, d, ro);
    if (masked && reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + x * a.xstride[3]] == 0) continue;
    const T y = ld_stream(reinterpret_cast<const T*>(a.in[1]) + ro[1] + x * a.xstride[1]);
    bool nan;
    const int32_t n = erps_point<T, NT, RIGHT>(reinterpret_cast<const T*>(a.in[0]) + ro[0] + x * a.xstride[0], a.mstride, a.M, y, pa,
                                               tb, nthr, fair, nan);
    nvalid += 1;
    ngood += nan ? 0 : 1;
    sum += nan ? 0 : n;
  }
  erps_write(a.out + ((key * a.nchunk + chunk) * (int64_t)nacc) * a.nx + x, a.nx, a.flags, denom, sum, ngood, nvalid);
}

// (the threshold slots beyond nthr repeat threshold 0 and are skipped when the numerator is formed)
template <typename T, bool RIGHT>
static int erps_dispatch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const double* pthr, const double* tthr, int nthr, int nacc,
                         double denom) {
  return dispatch_slots(nthr, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    return launch_xk_or_xr(ctx, plan, a, erps_xk_kernel<T, NT, RIGHT>, erps_xr_kernel<T, NT, RIGHT>, pthr, tthr, nthr, nacc, denom);
  });
}

}  // namespace wbx

extern "C" int wbx_ens_rps_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride, int nthr,
                                   const double* p_thresholds, const double* t_thresholds, int right_inclusive, const void* p,
                                   const void* t, const uint8_t* mask, double* partial_out) {
  using namespace wbx;
  // int32 numerator of a point: K (M - 1) M^2 < 2^31
  static_assert((int64_t)WBX_ERPS_MAX_THRESHOLDS * (WBX_ERPS_MAX_MEMBERS - 1) * WBX_ERPS_MAX_MEMBERS * WBX_ERPS_MAX_MEMBERS < ((int64_t)1 << 31),
                "a point's numerator must fit an int32");
  const S1Names names = {"wbx_ens_rps_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  WBX_REQUIRE(nthr >= 1 && nthr <= WBX_ERPS_MAX_THRESHOLDS, "wbx_ens_rps_partial: 1..%d thresholds per launch (got %d)",
              WBX_ERPS_MAX_THRESHOLDS, nthr);
  WBX_REQUIRE(M >= 1 && M <= WBX_ERPS_MAX_MEMBERS, "wbx_ens_rps_partial: 1..%d members (got %d)", WBX_ERPS_MAX_MEMBERS, M);
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "wbx_ens_rps_partial: unknown dtype %d", dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA | WBX_FLAG_FAIR)),
              "wbx_ens_rps_partial: flags other than MASKED | SKIPNA | FAIR (0x%x)", plan->flags);
  const bool fair = plan->flags & WBX_FLAG_FAIR;
  WBX_REQUIRE(!fair || M >= 2, "wbx_ens_rps_partial: the fair score needs at least 2 members (got %d)", M);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "wbx_ens_rps_partial: no plane mode, no folded x weights");
  // |S| stays exact in fp64: a partial meets at most depth_chunk * nx points of at most nthr (M - 1) M^2 each
  WBX_REQUIRE((double)plan->depth_chunk * (double)(plan->nx > 0 ? plan->nx : 1) * (double)nthr * (double)(M > 1 ? M - 1 : 1) * (double)M *
                      (double)M < 9007199254740992.0,
              "wbx_ens_rps_partial: 2^53 or more per partial (depth_chunk * nx * nthr * (M - 1) * M^2)");
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, 1);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  WBX_REQUIRE(p_thresholds != nullptr && t_thresholds != nullptr, "wbx_ens_rps_partial: a threshold table is NULL");
  a.M = M;
  a.mstride = member_stride;
  const double denom = fair ? (double)M * (double)M * (double)(M - 1) : (double)M * (double)M;
  if (dtype == WBX_F32)
    return right_inclusive ? erps_dispatch<float, true>(ctx, plan, a, p_thresholds, t_thresholds, nthr, nacc, denom)
                           : erps_dispatch<float, false>(ctx, plan, a, p_thresholds, t_thresholds, nthr, nacc, denom);
  return right_inclusive ? erps_dispatch<double, true>(ctx, plan, a, p_thresholds, t_thresholds, nthr, nacc, denom)
                         : erps_dispatch<double, false>(ctx, plan, a, p_thresholds, t_thresholds, nthr, nacc, denom);
}
