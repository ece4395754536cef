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
#include "wbx_ens_rps.hpp"

namespace wbx {

// Threshold k as the type the compare runs in, wave-uniform (SGPRs).  float: rounded as erps_round says.
template <typename T, bool RIGHT>
__device__ __forceinline__ T erps_threshold(const double* thr, int k) {
  const double v = ((const_ptr<double>)thr)[k];
  if constexpr (std::is_same<T, double>::value) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
  } else {
    return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(erps_round<RIGHT>(v))));
  }
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
  const S1Names names = {"wbx_ens_rps_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  if (int rc = erps_requirements(names.who, plan, dtype, M, nthr)) return rc;
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, 1);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  WBX_REQUIRE(p_thresholds != nullptr && t_thresholds != nullptr, "wbx_ens_rps_partial: a threshold table is NULL");
  a.M = M;
  a.mstride = member_stride;
  const double denom = erps_denominator(plan->flags & WBX_FLAG_FAIR, M);
  if (dtype == WBX_F32)
    return right_inclusive ? erps_dispatch<float, true>(ctx, plan, a, p_thresholds, t_thresholds, nthr, nacc, denom)
                           : erps_dispatch<float, false>(ctx, plan, a, p_thresholds, t_thresholds, nthr, nacc, denom);
  return right_inclusive ? erps_dispatch<double, true>(ctx, plan, a, p_thresholds, t_thresholds, nthr, nacc, denom)
                         : erps_dispatch<double, false>(ctx, plan, a, p_thresholds, t_thresholds, nthr, nacc, denom);
}
