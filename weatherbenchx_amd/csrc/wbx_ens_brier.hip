// Brier-type errors of event probabilities: the error, the absolute error and the squared error of (the fraction of members over
// an event threshold) against (the target is over that threshold), per threshold, summed like any other stage-1 statistic.
//
// Reference semantics restated: the chain of weatherbenchX/metrics/wrappers.py
//   ContinuousToBinary('both', a, dim)                       members and target -> 0 / 1 per event threshold a_k
//   EnsembleMean('predictions', ensemble_dim)                the fraction c_k / M of members over a_k
//   or WeibullEnsembleToProbabilistic('predictions', ...)    c_k / (M + 1), Weibull's plotting position
// in front of Error / AbsoluteError / SquaredError (deterministic.py:91-123): Bias, MAE, MSE / RMSE of the event probability, the
// last of them the Brier score.  Per point, members x_m, target y, thresholds a_k and D = M or M + 1 (M == 1, D == 1: the
// deterministic pair behind the first transform alone):
//   c_k = #{m : x_m > a_k}     o_k = [y > a_k]     e_k = c_k - o_k D
//   Error = e_k / D     AbsoluteError = |e_k| / D     SquaredError = e_k^2 / D^2;  NaN where a member or the target is NaN
//
// Nothing here is floating-point accumulation.  A lane keeps the K counts of its point in registers while it walks the members
// (one compare and one add per member and threshold, the thresholds wave-uniform in SGPRs), forms e_k, |e_k| and e_k^2 once per
// threshold (|e_k| <= D <= 257) and adds them to 3 K int64 sums of its own.  A partial is the sum S of those numerators over its
// points, written once as (double)S / (double)D or (double)S / (double)(D D): the correctly rounded quotient of two integers
// (|S| < 2^53 is required of the plan), a function of the inputs and the plan only.
// x summed: a lane owns a point of the row, the end is an integer wave reduction and an integer sum over the block's waves
// through LDS.  x kept: a lane owns an x and walks the chunk's rows; no cross-lane traffic.
#include <cmath>
#include <type_traits>

#include "wbx_cont_threshold.hpp"
#include "wbx_s1.hpp"

namespace wbx {

constexpr int BRIER_MAX_WAVES = 4;
constexpr int BRIER_FLIGHT = 8;  // member loads in flight per lane
constexpr int BRIER_ERR = 0, BRIER_ABS = 1, BRIER_SQ = 2;  // value lane stat * nthr + k
static_assert(WBX_BRIER_STATS == 3 && WBX_BRIER_MAX_THRESHOLDS == 16, "dispatch_slots' largest instantiation; three sums per threshold");

// One lane's sums: the numerators per statistic and threshold slot, the good (valid, non-NaN) and the valid points.
template <int NK>
struct BrierSums {
  int64_t s[WBX_BRIER_STATS][NK], ngood, nvalid;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < NK; ++q) s[BRIER_ERR][q] = s[BRIER_ABS][q] = s[BRIER_SQ][q] = 0;
    ngood = nvalid = 0;
  }
};

// One valid point into the lane's sums.  Padding slots (k >= nthr) hold +inf: c = 0, o = 0, e = 0.
template <typename T, int NK>
__device__ __forceinline__ void brier_point(const S1Args& a, const int64_t (&ro)[WBX_MAX_INPUTS], int64_t x, const T (&thr)[NK],
                                            int32_t denom, BrierSums<NK>& n) {
  const T y = ld_stream(reinterpret_cast<const T*>(a.in[1]) + ro[1] + x * a.xstride[1]);
  const T* pm = reinterpret_cast<const T*>(a.in[0]) + ro[0] + x * a.xstride[0];
  const int64_t ms = a.mstride;
  const int M = a.M;
  bool bad = y != y;
  int32_t c[NK];
#pragma unroll
  for (int q = 0; q < NK; ++q) c[q] = 0;
  int m = 0;
  for (; m + BRIER_FLIGHT <= M; m += BRIER_FLIGHT) {
    T v[BRIER_FLIGHT];
#pragma unroll
    for (int u = 0; u < BRIER_FLIGHT; ++u) v[u] = ld_stream(pm + (int64_t)(m + u) * ms);
#pragma unroll
    for (int u = 0; u < BRIER_FLIGHT; ++u) {
      bad |= v[u] != v[u];
#pragma unroll
      for (int q = 0; q < NK; ++q) c[q] += v[u] > thr[q] ? 1 : 0;
    }
  }
  if (m < M) {  // the last, short group: the loads past the end re-read the last member and are not counted
    T v[BRIER_FLIGHT];
#pragma unroll
    for (int u = 0; u < BRIER_FLIGHT; ++u) v[u] = ld_stream(pm + (int64_t)(m + u < M ? m + u : M - 1) * ms);
#pragma unroll
    for (int u = 0; u < BRIER_FLIGHT; ++u) {
      if (m + u < M) {
        bad |= v[u] != v[u];
#pragma unroll
        for (int q = 0; q < NK; ++q) c[q] += v[u] > thr[q] ? 1 : 0;
      }
    }
  }
  n.nvalid += 1;
  n.ngood += bad ? 0 : 1;
#pragma unroll
  for (int q = 0; q < NK; ++q) {
    const int32_t e = bad ? 0 : c[q] - (y > thr[q] ? denom : 0);  // |e| <= denom <= 257
    n.s[BRIER_ERR][q] += e;
    n.s[BRIER_ABS][q] += e < 0 ? -e : e;
    n.s[BRIER_SQ][q] += e * e;
  }
}

// Value lane stat * nthr + k (and its count lane) of one partial from its integer sums, into lanes o[lane * nj].
__device__ __forceinline__ void brier_write(double* o, int64_t nj, int nthr, int stat, int k, uint32_t flags, int32_t denom, int64_t s,
                                            int64_t ngood, int64_t nvalid) {
  const bool skipna = flags & WBX_FLAG_SKIPNA;
  const bool poisoned = !skipna && ngood != nvalid;  // a NaN under a valid point
  const double d = stat == BRIER_SQ ? (double)denom * (double)denom : (double)denom;
  const int nl = WBX_BRIER_STATS * nthr, q = stat * nthr + k;
  o[(int64_t)q * nj] = poisoned ? (double)NAN : (double)s / d;
  if (skipna)
    o[(int64_t)(nl + q) * nj] = (double)ngood;
  else if ((flags & WBX_FLAG_MASKED) && q == 0)
    o[(int64_t)nl * nj] = (double)nvalid;
}

// x summed.  grid = nkey * nchunk, block = plan->block_threads; rows are dealt to the waves as in s1_xr_kernel.
template <typename T, int NK>
__global__ void __launch_bounds__(256) brier_xr_kernel(S1Args a, const double* thr_in, int nthr, int denom, int nacc) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwave = blockDim.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const bool masked = a.flags & WBX_FLAG_MASKED;

  T thr[NK];
#pragma unroll
  for (int q = 0; q < NK; ++q) thr[q] = cont_threshold<T>(thr_in, q, nthr);
  BrierSums<NK> n;
  n.clear();

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
        brier_point<T, NK>(a, ro, x, thr, denom, n);
      }
    }
  }

  constexpr int NRED = WBX_BRIER_STATS * WBX_BRIER_MAX_THRESHOLDS + 2;  // stat * NK + k of this instantiation; ngood, nvalid
  __shared__ int64_t red[BRIER_MAX_WAVES][NRED];
#pragma unroll
  for (int st = 0; st < WBX_BRIER_STATS; ++st) {
#pragma unroll
    for (int q = 0; q < NK; ++q) {
      const int64_t s = wave_sum_i64(n.s[st][q]);
      if (lane == 0) red[wave][st * NK + q] = s;
    }
  }
  {
    const int64_t s0 = wave_sum_i64(n.ngood), s1 = wave_sum_i64(n.nvalid);
    if (lane == 0) {
      red[wave][NRED - 2] = s0;
      red[wave][NRED - 1] = s1;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < WBX_BRIER_STATS * nthr) {
    const int st = threadIdx.x / nthr, k = threadIdx.x - st * nthr;
    int64_t s[3] = {0, 0, 0};
    for (int w = 0; w < nwave; ++w) {
      s[0] += red[w][st * NK + k];
      s[1] += red[w][NRED - 2];
      s[2] += red[w][NRED - 1];
    }
    brier_write(a.out + (key * a.nchunk + chunk) * (int64_t)nacc, 1, nthr, st, k, a.flags, denom, s[0], s[1], s[2]);
  }
}

// x kept.  grid = nkey * nxtile * nchunk, block = plan->block_threads, one x per lane.
template <typename T, int NK>
__global__ void __launch_bounds__(256) brier_xk_kernel(S1Args a, const double* thr_in, int nthr, int denom, int nacc) {
  int64_t b = blockIdx.x;
  const int chunk = (int)(b % a.nchunk);
  b /= a.nchunk;
  const int xt = (int)(b % a.nxtile);
  const int64_t key = b / a.nxtile;
  const int64_t x = (int64_t)xt * blockDim.x + threadIdx.x;
  if (x >= a.nx) return;
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const bool masked = a.flags & WBX_FLAG_MASKED;

  T thr[NK];
#pragma unroll
  for (int q = 0; q < NK; ++q) thr[q] = cont_threshold<T>(thr_in, q, nthr);
  BrierSums<NK> n;
  n.clear();

  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, d, ro);
    if (masked && reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + x * a.xstride[3]] == 0) continue;
    brier_point<T, NK>(a, ro, x, thr, denom, n);
  }
  double* o = a.out + ((key * a.nchunk + chunk) * (int64_t)nacc) * a.nx + x;
#pragma unroll
  for (int st = 0; st < WBX_BRIER_STATS; ++st) {
#pragma unroll
    for (int q = 0; q < NK; ++q) {
      if (q < nthr) brier_write(o, a.nx, nthr, st, q, a.flags, denom, n.s[st][q], n.ngood, n.nvalid);
    }
  }
}

// (the threshold slots beyond nthr hold +inf, add nothing and are not written)
template <typename T>
static int brier_dispatch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const double* thr, int nthr, int denom, int nacc) {
  return dispatch_slots(nthr, [&](auto nk) {
    constexpr int NK = decltype(nk)::value;
    return launch_xk_or_xr(ctx, plan, a, brier_xk_kernel<T, NK>, brier_xr_kernel<T, NK>, thr, nthr, denom, nacc);
  });
}

}  // namespace wbx

extern "C" int wbx_ens_brier_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride, int denom, int nthr,
                                     const double* thresholds, const void* p, const void* t, const uint8_t* mask, double* partial_out) {
  using namespace wbx;
  // int32 numerators of a point: e^2 <= (M + 1)^2
  static_assert((int64_t)(WBX_BRIER_MAX_MEMBERS + 1) * (WBX_BRIER_MAX_MEMBERS + 1) < ((int64_t)1 << 31), "a point's e^2 must fit an int32");
  const S1Names names = {"wbx_ens_brier_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  WBX_REQUIRE(nthr >= 1 && nthr <= WBX_BRIER_MAX_THRESHOLDS, "wbx_ens_brier_partial: 1..%d thresholds per launch (got %d)",
              WBX_BRIER_MAX_THRESHOLDS, nthr);
  WBX_REQUIRE(M >= 1 && M <= WBX_BRIER_MAX_MEMBERS, "wbx_ens_brier_partial: 1..%d members (got %d)", WBX_BRIER_MAX_MEMBERS, M);
  WBX_REQUIRE(M == 1 ? denom == 1 : (denom == M || denom == M + 1),
              "wbx_ens_brier_partial: denom is M or M + 1, and 1 for M == 1 (got denom %d, M %d)", denom, M);
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "wbx_ens_brier_partial: unknown dtype %d", dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA)), "wbx_ens_brier_partial: flags other than MASKED | SKIPNA (0x%x)",
              plan->flags);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "wbx_ens_brier_partial: no plane mode, no folded x weights");
  // |S| stays exact in fp64: a partial meets at most depth_chunk * nx points of at most denom^2 each
  WBX_REQUIRE((double)plan->depth_chunk * (double)(plan->nx > 0 ? plan->nx : 1) * (double)denom * (double)denom < 9007199254740992.0,
              "wbx_ens_brier_partial: 2^53 or more per partial (depth_chunk * nx * denom^2)");
  WBX_REQUIRE(thresholds != nullptr, "wbx_ens_brier_partial: the threshold table is NULL");
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, WBX_BRIER_STATS * nthr);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  a.M = M;
  a.mstride = M == 1 ? 0 : member_stride;
  if (dtype == WBX_F32) return brier_dispatch<float>(ctx, plan, a, thresholds, nthr, denom, nacc);
  return brier_dispatch<double>(ctx, plan, a, thresholds, nthr, denom, nacc);
}
