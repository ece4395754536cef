// Ranked probability score of an ensemble against a scalar target at thresholds that are FIELDS: EnsembleRankedProbabilityScore
// (weatherbenchX/metrics/probabilistic.py:339-477) with `prediction_bin_thresholds` / `target_bin_thresholds` Datasets such as
// climatological terciles [bin, dayofyear, latitude, longitude], without the selected copy of the thresholds and the [K, M, frame]
// indicator arrays of its ContinuousToCDF transforms (wrappers.py).
//
// The score is the one of wbx_ens_rps.hip (c_k, o_k, n_k, D; integer sums, one correctly rounded quotient per partial) with the
// thresholds a_k, b_k read at the point.  The threshold field is input 2 of the plan, addressed like the climatology of
// wbx_ens_interval.hip (key_off[2], depth_off[2], xstride[2] and the gather tables, zero strides where it does not vary):
//   a_k = c[address + k * thr_stride]      b_k = c[address + k * thr_stride + t_off]      (t_off == 0: one load serves both)
// A point with a NaN among its nthr prediction or target thresholds is a NaN point like one with a NaN member or target
// (cdf.where(~isnan(da)).where(~isnan(thresholds)), then sum(bin_dim, skipna=False)).  Slots k >= nthr are not loaded and not counted.
//
// Compares decide as NumPy's promoted comparison: equal types as they are; float32 thresholds against float64 data widen exactly;
// float64 thresholds against float32 data are rounded per point (erps_round: toward -inf for <=, toward +inf for <) and the compare
// stays in float32 -- erps_threshold's scheme on vector registers.
// A lane holds its point's up to 2 x 16 thresholds and 16 counts in registers; the member walk and the numerator are erps_point.
#include "wbx_ens_rps.hpp"

namespace wbx {

struct ErpsFieldArgs {
  int64_t thr_stride, t_off;  // elements of the threshold type
  int32_t nthr, nacc;
  double denom;
};

// A threshold of the field as the type the data is compared in; NaN stays NaN.
template <typename T, typename TC, bool RIGHT>
__device__ __forceinline__ T erpf_convert(TC v) {
  if constexpr (std::is_same<T, float>::value && std::is_same<TC, double>::value)
    return erps_round<RIGHT>(v);
  else
    return (T)v;
}

// The nthr thresholds that start at `cp`, converted; `bad` gathers whether one of them is NaN.  The other slots hold 0 unread.
template <typename T, typename TC, int NT, bool RIGHT>
__device__ __forceinline__ void erpf_load(const TC* cp, const ErpsFieldArgs& e, T (&thr)[NT], bool& bad) {
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    thr[q] = (T)0;
    if (q < e.nthr) {
      thr[q] = erpf_convert<T, TC, RIGHT>(ld_stream(cp + q * e.thr_stride));
      bad |= thr[q] != thr[q];
    }
  }
}

// The numerator of the point x of the row at ro[]; `nan`: a member, the target or one of the point's thresholds is NaN.
template <typename T, typename TC, int NT, bool RIGHT>
__device__ __forceinline__ int32_t erpf_point(const S1Args& a, const ErpsFieldArgs& e, const int64_t (&ro)[WBX_MAX_INPUTS], int64_t x,
                                              bool fair, bool& nan) {
  const TC* cp = reinterpret_cast<const TC*>(a.in[2]) + ro[2] + x * a.xstride[2];
  const T y = ld_stream(reinterpret_cast<const T*>(a.in[1]) + ro[1] + x * a.xstride[1]);
  bool bad = false;
  T pa[NT], tb[NT];
  erpf_load<T, TC, NT, RIGHT>(cp, e, pa, bad);
  if (e.t_off != 0) {  // (wave-uniform)
    erpf_load<T, TC, NT, RIGHT>(cp + e.t_off, e, tb, bad);
  } else {
#pragma unroll
    for (int q = 0; q < NT; ++q) tb[q] = pa[q];
  }
  const int32_t n = erps_point<T, NT, RIGHT>(reinterpret_cast<const T*>(a.in[0]) + ro[0] + x * a.xstride[0], a.mstride, a.M, y, pa, tb,
                                             e.nthr, fair, nan);
  nan |= bad;
  return n;
}

// x summed.  grid = nkey * nchunk, block = plan->block_threads; rows are dealt to the waves as in erps_xr_kernel.
template <typename T, typename TC, int NT, bool RIGHT>
__global__ void __launch_bounds__(256) erpf_xr_kernel(S1Args a, ErpsFieldArgs e) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwave = blockDim.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const bool masked = a.flags & WBX_FLAG_MASKED, fair = a.flags & WBX_FLAG_FAIR;
  int64_t sum = 0, ngood = 0, nvalid = 0;

  int64_t kb[WBX_MAX_INPUTS];
  key_bases<3>(a, key, kb);
  for (int64_t dbatch = d0 + wave; dbatch < d1; dbatch += (int64_t)64 * nwave) {
    // lane l resolves the wave's l-th row; the sweep broadcasts the results (s1_xr_kernel)
    const int64_t dmine = dbatch + (int64_t)lane * nwave;
    int64_t rov[WBX_MAX_INPUTS];
    row_bases<3>(a, kb, key, dmine < d1 ? dmine : d1 - 1, rov);
    const int64_t left = (d1 - dbatch + nwave - 1) / nwave;
    const int nrow = (int)(left < 64 ? left : 64);
    for (int l = 0; l < nrow; ++l) {
      int64_t ro[WBX_MAX_INPUTS];
#pragma unroll
      for (int i = 0; i < WBX_MAX_INPUTS; ++i) ro[i] = readlane64(rov[i], l);
      for (int64_t x = lane; x < a.nx; x += 64) {
        if (masked && reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + x * a.xstride[3]] == 0) continue;
        bool nan;
        const int32_t n = erpf_point<T, TC, NT, RIGHT>(a, e, ro, x, fair, nan);
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
    erps_write(a.out + (key * a.nchunk + chunk) * (int64_t)e.nacc, 1, a.flags, e.denom, s[0], s[1], s[2]);
  }
}

// x kept.  grid = nkey * nxtile * nchunk, block = plan->block_threads, one x per lane.
template <typename T, typename TC, int NT, bool RIGHT>
__global__ void __launch_bounds__(256) erpf_xk_kernel(S1Args a, ErpsFieldArgs e) {
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
  int64_t sum = 0, ngood = 0, nvalid = 0;

  int64_t kb[WBX_MAX_INPUTS];
  key_bases<3>(a, key, kb);
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<3>(a, kb, key, d, ro);
    if (masked && reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + x * a.xstride[3]] == 0) continue;
    bool nan;
    const int32_t n = erpf_point<T, TC, NT, RIGHT>(a, e, ro, x, fair, nan);
    nvalid += 1;
    ngood += nan ? 0 : 1;
    sum += nan ? 0 : n;
  }
  erps_write(a.out + ((key * a.nchunk + chunk) * (int64_t)e.nacc) * a.nx + x, a.nx, a.flags, e.denom, sum, ngood, nvalid);
}

template <typename T, typename TC>
static int erpf_dispatch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const ErpsFieldArgs& e, bool right) {
  return dispatch_slots(e.nthr, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    if (right) return launch_xk_or_xr(ctx, plan, a, erpf_xk_kernel<T, TC, NT, true>, erpf_xr_kernel<T, TC, NT, true>, e);
    return launch_xk_or_xr(ctx, plan, a, erpf_xk_kernel<T, TC, NT, false>, erpf_xr_kernel<T, TC, NT, false>, e);
  });
}

}  // namespace wbx

extern "C" int wbx_ens_rps_field_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int thr_dtype, int M, int64_t member_stride,
                                         int nthr, int64_t thr_stride, int64_t t_off, int right_inclusive, const void* p, const void* t,
                                         const void* c, const uint8_t* mask, double* partial_out) {
  using namespace wbx;
  const S1Names names = {"wbx_ens_rps_field_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  if (int rc = erps_requirements(names.who, plan, dtype, M, nthr)) return rc;
  WBX_REQUIRE(thr_dtype == WBX_F32 || thr_dtype == WBX_F64, "wbx_ens_rps_field_partial: unknown thr_dtype %d", thr_dtype);
  WBX_REQUIRE(thr_stride != 0 || nthr == 1, "wbx_ens_rps_field_partial: thr_stride is 0 with %d thresholds", nthr);
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, 1);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  WBX_REQUIRE(c != nullptr, "wbx_ens_rps_field_partial: c is NULL");
  a.in[2] = c;
  a.M = M;
  a.mstride = member_stride;
  const ErpsFieldArgs e = {thr_stride, t_off, nthr, nacc, erps_denominator(plan->flags & WBX_FLAG_FAIR, M)};
  const bool right = right_inclusive != 0;
  if (dtype == WBX_F32)
    return thr_dtype == WBX_F32 ? erpf_dispatch<float, float>(ctx, plan, a, e, right) : erpf_dispatch<float, double>(ctx, plan, a, e, right);
  return thr_dtype == WBX_F32 ? erpf_dispatch<double, float>(ctx, plan, a, e, right) : erpf_dispatch<double, double>(ctx, plan, a, e, right);
}
