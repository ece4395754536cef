// Thresholded 2x2 contingency tables at thresholds that are FIELDS: TruePositives .. TrueNegatives behind
// ContinuousToBinary('both', field, dim) whose thresholds are a DataArray / Dataset (weatherbenchX/metrics/wrappers.py:50-88), such as
// "exceeds the local climatological 95th percentile", without the [K, frame] indicator arrays.
//
// The counts, the cells and the write of a partial are those of wbx_contingency.hip (integer counts TP = #(P and O), #P, #O per
// threshold, N good points, the cells formed once at the end) with the threshold read at the point.  The field is input 2 of the
// plan, addressed like the thresholds of wbx_ens_rps_field.hip (key_off[2], depth_off[2], xstride[2] and the gather tables, zero
// strides where it does not vary):
//   thr_k = c[address + (thr_first + k) * thr_stride]          P_k = p > thr_k, O_k = t > thr_k  (strict; one load serves both)
// A comparison with a NaN threshold is false -- the point counts towards TN when p and t are not NaN, (x > NaN).where(~isnan(x)) --
// UNLIKE wbx_ens_rps_field.hip, where a NaN threshold makes the point a NaN point.
//
// Compares decide as NumPy's promoted comparison: equal types as they are; float32 thresholds against float64 data widen exactly;
// float64 thresholds against float32 data are rounded per point toward -inf (erps_round<true>: x > v <=> !(x <= v) <=> x > rd(v)
// for non-NaN x) and the compare stays in float32.
// x summed: as in wbx_contingency.hip the counts are popcounts of wave-wide compare masks in wave-uniform registers, a point that
// does not count has both values replaced by -inf, which exceeds no threshold (-inf > -inf is false, and so is -inf > NaN).
// x kept: one lane owns one x and keeps the 3 * nthr + 2 counters in its own registers.
// A threshold is used exactly once per point: it is loaded, converted, compared and dropped in batches of CONTF_BATCH slots, never
// all NT of a lane at once (wbx_ens_rps_field.hip holds them for the member walk; its 16-slot kernels run one wave per SIMD).
#include "wbx_contingency.hpp"
#include "wbx_ens_rps.hpp"

namespace wbx {

constexpr int CONTF_BATCH = 4;  // threshold slots in flight per lane

struct ContFieldArgs {
  int64_t thr_stride, thr_first;  // elements of the threshold type; slots
  int32_t nthr, nacc;
};

// A threshold of the field as the type the data is compared in; NaN stays NaN.
template <typename T, typename TC>
__device__ __forceinline__ T contf_convert(TC v) {
  if constexpr (std::is_same<T, float>::value && std::is_same<TC, double>::value)
    return erps_round<true>(v);
  else
    return (T)v;
}

// Element offset of slot q's thresholds from the point's address.  Slots q >= nthr re-read the last threshold (inside the field);
// their counts are never written.
__device__ __forceinline__ int64_t contf_slot(const ContFieldArgs& e, int q) {
  return (e.thr_first + (q < e.nthr ? q : e.nthr - 1)) * e.thr_stride;
}

// The end of the x-summed kernel (the lines that end cont_xr_kernel, see wbx_contingency.hpp): the waves' wave-uniform counts summed
// through LDS, thread k writes threshold k of the partial of (key, chunk), whose rows are d0..d1.
template <int NT, bool MASKED>
__device__ __forceinline__ void contf_block_write(const S1Args& a, int nthr, int nacc, int64_t key, int chunk, int64_t d0, int64_t d1,
                                                 const uint32_t (&ctp)[NT], const uint32_t (&cp)[NT], const uint32_t (&co)[NT],
                                                 uint32_t ngood, uint32_t nvalid) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwave = blockDim.x >> 6;
  __shared__ uint32_t red[CONT_MAX_WAVES][3 * WBX_CONT_MAX_THRESHOLDS + 2];
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      red[wave][q] = ctp[q];
      red[wave][WBX_CONT_MAX_THRESHOLDS + q] = cp[q];
      red[wave][2 * WBX_CONT_MAX_THRESHOLDS + q] = co[q];
    }
    red[wave][3 * WBX_CONT_MAX_THRESHOLDS] = ngood;
    red[wave][3 * WBX_CONT_MAX_THRESHOLDS + 1] = nvalid;
  }
  __syncthreads();
  if ((int)threadIdx.x < nthr) {
    const int k = threadIdx.x;
    uint32_t s[5] = {0, 0, 0, 0, 0};
    for (int w = 0; w < nwave; ++w) {
      s[0] += red[w][k];
      s[1] += red[w][WBX_CONT_MAX_THRESHOLDS + k];
      s[2] += red[w][2 * WBX_CONT_MAX_THRESHOLDS + k];
      s[3] += red[w][3 * WBX_CONT_MAX_THRESHOLDS];
      s[4] += red[w][3 * WBX_CONT_MAX_THRESHOLDS + 1];
    }
    if constexpr (!MASKED) s[4] = d1 > d0 ? (uint32_t)((d1 - d0) * a.nx) : 0u;  // every point is valid
    cont_write(a.out + (key * a.nchunk + chunk) * (int64_t)nacc, 1, nthr, k, a.flags, s[0], s[1], s[2], s[3], s[4]);
  }
}

// x summed.  grid = nkey * nchunk, block = plan->block_threads; rows are dealt to the waves as in cont_xr_kernel.
template <typename T, typename TC, int V, int NT, bool MASKED>
__global__ void __launch_bounds__(256) contf_xr_kernel(S1Args a, ContFieldArgs e) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwave = blockDim.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  constexpr int B = NT < CONTF_BATCH ? NT : CONTF_BATCH;

  uint32_t ctp[NT], cp[NT], co[NT], ngood = 0, nvalid = 0;
#pragma unroll
  for (int q = 0; q < NT; ++q) ctp[q] = cp[q] = co[q] = 0;

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
      // every lane takes every trip (the compare masks are wave-wide): a lane beyond the row re-reads the row's last
      // elements and drops them
      for (int64_t x0 = 0; x0 < a.nx; x0 += 64 * V) {
        const int64_t x = x0 + (int64_t)lane * V;
        const bool inside = x < a.nx;  // (V == 4: nx % 4 == 0, the four are inside together)
        const int64_t xl = inside ? x : a.nx - V;
        T p[V], t[V];
        uint8_t m[V];
        cont_load<T, V>(a.in[0], ro[0], xl, a.xstride[0], p);
        cont_load<T, V>(a.in[1], ro[1], xl, a.xstride[1], t);
        if constexpr (MASKED) cont_load<uint8_t, V>(a.in[3], ro[3], xl, a.xstride[3], m);
        T ps[V], ts[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
          bool valid = inside;
          if constexpr (MASKED) {
            valid = valid && m[k] != 0;
            nvalid += (uint32_t)__popcll(__ballot(valid));
          }
          const bool ok = valid && p[k] == p[k] && t[k] == t[k];
          ngood += (uint32_t)__popcll(__ballot(ok));
          ps[k] = ok ? p[k] : (T)-INFINITY;
          ts[k] = ok ? t[k] : (T)-INFINITY;
        }
#pragma unroll
        for (int q0 = 0; q0 < NT; q0 += B) {
          TC c[B][V];
#pragma unroll
          for (int j = 0; j < B; ++j) cont_load<TC, V>(a.in[2], ro[2] + contf_slot(e, q0 + j), xl, a.xstride[2], c[j]);
#pragma unroll
          for (int j = 0; j < B; ++j) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
              const T thr = contf_convert<T, TC>(c[j][k]);
              const unsigned long long bp = __ballot(ps[k] > thr), bo = __ballot(ts[k] > thr);
              cp[q0 + j] += (uint32_t)__popcll(bp);
              co[q0 + j] += (uint32_t)__popcll(bo);
              ctp[q0 + j] += (uint32_t)__popcll(bp & bo);
            }
          }
        }
      }
    }
  }
  contf_block_write<NT, MASKED>(a, e.nthr, e.nacc, key, chunk, d0, d1, ctp, cp, co, ngood, nvalid);
}

// x kept.  grid = nkey * nxtile * nchunk, block = plan->block_threads, one x per lane (dword loads whatever plan->vec says).
template <typename T, typename TC, int NT, bool MASKED>
__global__ void __launch_bounds__(256) contf_xk_kernel(S1Args a, ContFieldArgs e) {
  int64_t b = blockIdx.x;
  const int chunk = (int)(b % a.nchunk);
  b /= a.nchunk;
  const int xt = (int)(b % a.nxtile);
  const int64_t key = b / a.nxtile;
  const int64_t x = (int64_t)xt * blockDim.x + threadIdx.x;
  if (x >= a.nx) return;
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  constexpr int B = NT < CONTF_BATCH ? NT : CONTF_BATCH;

  uint32_t ctp[NT], cp[NT], co[NT], ngood = 0, nvalid = 0;
#pragma unroll
  for (int q = 0; q < NT; ++q) ctp[q] = cp[q] = co[q] = 0;

  int64_t kb[WBX_MAX_INPUTS];
  key_bases<3>(a, key, kb);
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<3>(a, kb, key, d, ro);
    T p[1], t[1];
    uint8_t m[1] = {1};
    cont_load<T, 1>(a.in[0], ro[0], x, a.xstride[0], p);
    cont_load<T, 1>(a.in[1], ro[1], x, a.xstride[1], t);
    if constexpr (MASKED) cont_load<uint8_t, 1>(a.in[3], ro[3], x, a.xstride[3], m);
    const bool valid = m[0] != 0;
    const bool ok = valid && p[0] == p[0] && t[0] == t[0];
    nvalid += valid ? 1u : 0u;
    ngood += ok ? 1u : 0u;
    const T ps = ok ? p[0] : (T)-INFINITY, ts = ok ? t[0] : (T)-INFINITY;
#pragma unroll
    for (int q0 = 0; q0 < NT; q0 += B) {
      TC c[B][1];
#pragma unroll
      for (int j = 0; j < B; ++j) cont_load<TC, 1>(a.in[2], ro[2] + contf_slot(e, q0 + j), x, a.xstride[2], c[j]);
#pragma unroll
      for (int j = 0; j < B; ++j) {
        const T thr = contf_convert<T, TC>(c[j][0]);
        const bool bp = ps > thr, bo = ts > thr;
        cp[q0 + j] += bp ? 1u : 0u;
        co[q0 + j] += bo ? 1u : 0u;
        ctp[q0 + j] += (bp && bo) ? 1u : 0u;
      }
    }
  }
  double* o = a.out + ((key * a.nchunk + chunk) * (int64_t)e.nacc) * a.nx + x;
#pragma unroll
  for (int q = 0; q < NT; ++q)
    if (q < e.nthr) cont_write(o, a.nx, e.nthr, q, a.flags, ctp[q], cp[q], co[q], ngood, nvalid);
}

template <typename T, typename TC, bool MASKED>
static int contf_dispatch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const ContFieldArgs& e) {
  return dispatch_slots(e.nthr, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    const auto xk = contf_xk_kernel<T, TC, NT, MASKED>;
    return launch_xk_or_xr(ctx, plan, a, xk,
                           plan->vec == 4 ? contf_xr_kernel<T, TC, 4, NT, MASKED> : contf_xr_kernel<T, TC, 1, NT, MASKED>, e);
  });
}

template <typename T, typename TC>
static int contf_dispatch_mask(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const ContFieldArgs& e) {
  return (plan->flags & WBX_FLAG_MASKED) ? contf_dispatch<T, TC, true>(ctx, plan, a, e) : contf_dispatch<T, TC, false>(ctx, plan, a, e);
}

}  // namespace wbx

extern "C" int wbx_contingency_field_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int thr_dtype, int nthr, int64_t thr_stride,
                                             int64_t thr_first, const void* p, const void* t, const void* c, const uint8_t* mask,
                                             double* partial_out) {
  using namespace wbx;
  const S1Names names = {"wbx_contingency_field_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  if (int rc = cont_requirements(names.who, plan, dtype, nthr)) return rc;
  WBX_REQUIRE(thr_dtype == WBX_F32 || thr_dtype == WBX_F64, "wbx_contingency_field_partial: unknown thr_dtype %d", thr_dtype);
  WBX_REQUIRE(thr_stride != 0 || nthr == 1, "wbx_contingency_field_partial: thr_stride is 0 with %d thresholds", nthr);
  WBX_REQUIRE(thr_first >= 0, "wbx_contingency_field_partial: thr_first is negative (%lld)", (long long)thr_first);
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, WBX_CONT_CELLS * nthr);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  WBX_REQUIRE(c != nullptr, "wbx_contingency_field_partial: c is NULL");
  a.in[2] = c;
  const ContFieldArgs e = {thr_stride, thr_first, nthr, nacc};
  if (dtype == WBX_F32)
    return thr_dtype == WBX_F32 ? contf_dispatch_mask<float, float>(ctx, plan, a, e) : contf_dispatch_mask<float, double>(ctx, plan, a, e);
  return thr_dtype == WBX_F32 ? contf_dispatch_mask<double, float>(ctx, plan, a, e) : contf_dispatch_mask<double, double>(ctx, plan, a, e);
}
