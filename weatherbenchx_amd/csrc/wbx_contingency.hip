// Thresholded 2x2 contingency tables: the four cells TP / FP / FN / TN of (p > thr_k, t > thr_k) for a list of thresholds, summed
// like any other stage-1 statistic.
//
// Reference semantics restated:
//   ContinuousToBinary (weatherbenchX/metrics/wrappers.py:50-88)   b_k(x) = float(x > thr_k), NaN where x is NaN; a comparison
//       with a NaN threshold is false (0, not NaN)
//   TruePositives .. FalseNegatives (weatherbenchX/metrics/categorical.py:25-101)
//       cell(b(p), b(t)) as 0 / 1, NaN where b(p) * b(t) is NaN, i.e. where p or t is NaN -- for EVERY threshold
//
// Nothing here is floating-point accumulation.  Per threshold three integer counts -- TP = #(P and O), #P, #O -- plus the
// number of good (valid, non-NaN) points N and the number of valid points are kept, and the cells are formed once at the end:
//   TP, FP = #P - TP, FN = #O - TP, TN = N - #P - #O + TP     (exact in fp64; NaN when a NaN under a valid point poisons)
// x summed: the counts are wave-uniform.  A point that does not count (beyond nx, masked out, NaN) has both values replaced
// by -inf, which exceeds no threshold, so the vector pipe issues two compares per threshold and 64 points and the counts are
// popcounts of the compare masks in scalar registers; the end is an integer sum over the block's waves through LDS.
// x kept: one lane owns one x and keeps the 3 * nthr + 2 counters in its own registers.
// Counters are uint32: a launch whose partial could see 2^32 points is refused.
#include <cmath>
#include <type_traits>

#include "wbx_cont_threshold.hpp"
#include "wbx_contingency.hpp"

namespace wbx {

// x summed.  grid = nkey * nchunk, block = plan->block_threads; rows are dealt to the waves as in s1_xr_kernel.
template <typename T, int V, int NT, bool MASKED>
__global__ void __launch_bounds__(256) cont_xr_kernel(S1Args a, const double* thr_in, int nthr, int nacc) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwave = blockDim.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;

  T thr[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) thr[q] = cont_threshold<T>(thr_in, q, nthr);
  uint32_t ctp[NT], cp[NT], co[NT], ngood = 0, nvalid = 0;
#pragma unroll
  for (int q = 0; q < NT; ++q) ctp[q] = cp[q] = co[q] = 0;

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
#pragma unroll
        for (int k = 0; k < V; ++k) {
          bool valid = inside;
          if constexpr (MASKED) {
            valid = valid && m[k] != 0;
            nvalid += (uint32_t)__popcll(__ballot(valid));
          }
          const bool ok = valid && p[k] == p[k] && t[k] == t[k];
          ngood += (uint32_t)__popcll(__ballot(ok));
          const T ps = ok ? p[k] : (T)-INFINITY, ts = ok ? t[k] : (T)-INFINITY;
#pragma unroll
          for (int q = 0; q < NT; ++q) {
            const unsigned long long bp = __ballot(ps > thr[q]), bo = __ballot(ts > thr[q]);
            cp[q] += (uint32_t)__popcll(bp);
            co[q] += (uint32_t)__popcll(bo);
            ctp[q] += (uint32_t)__popcll(bp & bo);
          }
        }
      }
    }
  }

  // (wbx_contingency_field.hip has these lines as contf_block_write: as a shared function they change this unit's registers)
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

// x kept.  grid = nkey * nxtile * nchunk, block = plan->block_threads, one x per lane (dword loads whatever plan->vec says:
// four x per lane would be four sets of counters).
template <typename T, int NT, bool MASKED>
__global__ void __launch_bounds__(256) cont_xk_kernel(S1Args a, const double* thr_in, int nthr, int nacc) {
  int64_t b = blockIdx.x;
  const int chunk = (int)(b % a.nchunk);
  b /= a.nchunk;
  const int xt = (int)(b % a.nxtile);
  const int64_t key = b / a.nxtile;
  const int64_t x = (int64_t)xt * blockDim.x + threadIdx.x;
  if (x >= a.nx) return;
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;

  T thr[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) thr[q] = cont_threshold<T>(thr_in, q, nthr);
  uint32_t ctp[NT], cp[NT], co[NT], ngood = 0, nvalid = 0;
#pragma unroll
  for (int q = 0; q < NT; ++q) ctp[q] = cp[q] = co[q] = 0;

  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
#pragma unroll 4
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, d, ro);
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
    for (int q = 0; q < NT; ++q) {
      const bool bp = ps > thr[q], bo = ts > thr[q];
      cp[q] += bp ? 1u : 0u;
      co[q] += bo ? 1u : 0u;
      ctp[q] += (bp && bo) ? 1u : 0u;
    }
  }
  double* o = a.out + ((key * a.nchunk + chunk) * (int64_t)nacc) * a.nx + x;
#pragma unroll
  for (int q = 0; q < NT; ++q)
    if (q < nthr) cont_write(o, a.nx, nthr, q, a.flags, ctp[q], cp[q], co[q], ngood, nvalid);
}

template <typename T, bool MASKED>
static int cont_dispatch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const double* thr, int nthr, int nacc) {
  return dispatch_slots(nthr, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    const auto xk = cont_xk_kernel<T, NT, MASKED>;  // (named ahead of the ?: below: the code object keeps the kernels in the order they are named)
    return launch_xk_or_xr(ctx, plan, a, xk, plan->vec == 4 ? cont_xr_kernel<T, 4, NT, MASKED> : cont_xr_kernel<T, 1, NT, MASKED>, thr,
                           nthr, nacc);
  });
}

}  // namespace wbx

extern "C" int wbx_contingency_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int nthr, const void* p, const void* t,
                                       const double* thresholds, const uint8_t* mask, double* partial_out) {
  using namespace wbx;
  const S1Names names = {"wbx_contingency_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  if (int rc = cont_requirements(names.who, plan, dtype, nthr)) return rc;
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, WBX_CONT_CELLS * nthr);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  WBX_REQUIRE(thresholds != nullptr, "wbx_contingency_partial: thresholds is NULL");
  const bool masked = plan->flags & WBX_FLAG_MASKED;
  if (dtype == WBX_F32)
    return masked ? cont_dispatch<float, true>(ctx, plan, a, thresholds, nthr, nacc)
                  : cont_dispatch<float, false>(ctx, plan, a, thresholds, nthr, nacc);
  return masked ? cont_dispatch<double, true>(ctx, plan, a, thresholds, nthr, nacc)
                : cont_dispatch<double, false>(ctx, plan, a, thresholds, nthr, nacc);
}
