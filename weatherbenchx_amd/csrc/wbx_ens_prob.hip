// Contingency tables of ensemble event probabilities: the four cells TP / FP / FN / TN of (the fraction of members over an event
// threshold falls into a probability slot, the target is over that threshold) for a list of event thresholds and a list of
// probability slots, summed like any other stage-1 statistic.
//
// Reference semantics restated: the chain of weatherbenchX/metrics/wrappers.py
//   ContinuousToBinary('both', a, dim_e)           members and target -> 0 / 1 per event threshold a_k
//   EnsembleMean('predictions', ensemble_dim)      the fraction c_k / M of members over a_k, in float32
//   ContinuousToBinary('predictions', tau, dim_p)  or ContinuousToBins('predictions', edges, dim_p): probability slot j
// in front of TruePositives .. TrueNegatives (categorical.py:25-101).  Per point and event threshold
//   c_k = #{m : x_m > a_k}  in 0..M        o_k = [y > a_k]
// and whether slot j says "predicted" is a function of the integer c_k alone.  The host has worked that function out by running
// the host route's own transforms on c = 0..M and hands every slot over as a run of counts lo_j <= c <= hi_j (lo > hi: empty):
// the kernel never sees a probability.
//
// Nothing here is floating-point accumulation.  A lane owns a point: it walks the members (one compare and one add per member
// and event threshold, the thresholds wave-uniform in SGPRs), looks the K counts up in a table `c -> bits over j` that the block
// builds in LDS from the slots, which gives the point's P_kj as one word of bits, and adds those bits to its own uint32
// counters: #(P & O) and #P per (k, j), #O per k, good and valid points.  The cells are formed once per partial:
//   TP, FP = #P - TP, FN = #O - TP, TN = N - #P - #O + TP     (exact in fp64; NaN when a NaN under a valid point poisons)
// x summed: rows are walked as in s1_xr_kernel, the end is an integer wave reduction and an integer sum over the block's waves
// through LDS.  x kept: a lane owns an x and keeps its counters across the chunk's rows.  A launch whose partial could see 2^32
// points is refused.
#include <cmath>
#include <type_traits>

#include "wbx_cont_threshold.hpp"
#include "wbx_s1.hpp"

namespace wbx {

constexpr int EPC_MAX_WAVES = 4;
constexpr int EPC_FLIGHT = 8;                      // member loads in flight per lane
constexpr int EPC_PAIRS = WBX_EPC_MAX_PAIRS;       // (k, j) pairs per launch: bit q = k * nslot + j of a point's word
constexpr int EPC_TABLE = WBX_EPC_MAX_MEMBERS + 1;  // counts 0..M
constexpr int EPC_THRESHOLDS = WBX_EPC_MAX_PAIRS;   // event thresholds per launch: nthr <= nthr * nslot
static_assert(EPC_PAIRS == 16, "a point's #P bits and #(P & O) bits share one 32-bit word");

// The block's table: bit j of tab[c] says whether c members over the threshold put the point into slot j.
__device__ __forceinline__ void epc_table(uint32_t* tab, const int32_t* slots, int nslot, int M) {
  for (int c = threadIdx.x; c <= M; c += blockDim.x) {
    uint32_t bits = 0;
    for (int j = 0; j < nslot; ++j) {
      const int32_t lo = ((const_ptr<int32_t>)slots)[2 * j], hi = ((const_ptr<int32_t>)slots)[2 * j + 1];
      bits |= (lo <= c && c <= hi) ? 1u << j : 0u;
    }
    tab[c] = bits;
  }
  __syncthreads();
}

// The counts c_k of the point whose members start at `pm` (element stride `ms`); `bad` says whether a member is NaN.  Padding slots
// (k >= nthr) hold +inf and count nothing.
template <typename T, int NK>
__device__ __forceinline__ void epc_counts(const T* pm, int64_t ms, int M, const T (&thr)[NK], uint32_t (&c)[NK], bool& bad) {
#pragma unroll
  for (int q = 0; q < NK; ++q) c[q] = 0;
  int m = 0;
  for (; m + EPC_FLIGHT <= M; m += EPC_FLIGHT) {
    T v[EPC_FLIGHT];
#pragma unroll
    for (int u = 0; u < EPC_FLIGHT; ++u) v[u] = ld_stream(pm + (int64_t)(m + u) * ms);
#pragma unroll
    for (int u = 0; u < EPC_FLIGHT; ++u) {
      bad |= v[u] != v[u];
#pragma unroll
      for (int q = 0; q < NK; ++q) c[q] += v[u] > thr[q] ? 1u : 0u;
    }
  }
  if (m < M) {  // the last, short group: the loads past the end re-read the last member and are not counted
    T v[EPC_FLIGHT];
#pragma unroll
    for (int u = 0; u < EPC_FLIGHT; ++u) v[u] = ld_stream(pm + (int64_t)(m + u < M ? m + u : M - 1) * ms);
#pragma unroll
    for (int u = 0; u < EPC_FLIGHT; ++u) {
      if (m + u < M) {
        bad |= v[u] != v[u];
#pragma unroll
        for (int q = 0; q < NK; ++q) c[q] += v[u] > thr[q] ? 1u : 0u;
      }
    }
  }
}

// One lane's counters.
template <int NK, int NP>
struct EpcCounters {
  uint32_t tp[NP], np[NP], no[NK], ngood, nvalid;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < NP; ++q) tp[q] = np[q] = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) no[k] = 0;
    ngood = nvalid = 0;
  }
};

// One valid point into the lane's counters.
template <typename T, int NK, int NP>
__device__ __forceinline__ void epc_point(const S1Args& a, const int64_t (&ro)[WBX_MAX_INPUTS], int64_t x, const T (&thr)[NK], int nthr,
                                          int nslot, const uint32_t* tab, EpcCounters<NK, NP>& n) {
  const T y = ld_stream(reinterpret_cast<const T*>(a.in[1]) + ro[1] + x * a.xstride[1]);
  bool bad = y != y;
  uint32_t c[NK];
  epc_counts<T, NK>(reinterpret_cast<const T*>(a.in[0]) + ro[0] + x * a.xstride[0], a.mstride, a.M, thr, c, bad);
  n.nvalid += 1;
  n.ngood += bad ? 0u : 1u;
  uint32_t w = 0;  // bits 0..15: P_kj at q = k * nslot + j; bits 16..31: P_kj & O_k
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (k < nthr) {
      const uint32_t pk = tab[c[k]] << (k * nslot);  // (c <= M: inside the table)
      const bool o = !bad && y > thr[k];
      n.no[k] += o ? 1u : 0u;
      w |= pk | (o ? pk << EPC_PAIRS : 0u);
    }
  }
  w = bad ? 0u : w;
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    n.np[q] += (w >> q) & 1u;
    n.tp[q] += (w >> (EPC_PAIRS + q)) & 1u;
  }
}

// The four cells of pair q (and the count lanes) from the integer counts, into lanes o[lane * nj].
__device__ __forceinline__ void epc_write(double* o, int64_t nj, int npair, int q, uint32_t flags, uint32_t tp, uint32_t np, uint32_t no,
                                          uint32_t ngood, uint32_t nvalid) {
  const bool skipna = flags & WBX_FLAG_SKIPNA;
  const bool poisoned = !skipna && ngood != nvalid;  // a NaN under a valid point
  double v[WBX_EPC_CELLS] = {(double)tp, (double)(np - tp), (double)(no - tp), (double)(ngood - np - no + tp)};
#pragma unroll
  for (int c = 0; c < WBX_EPC_CELLS; ++c) o[(int64_t)(c * npair + q) * nj] = poisoned ? (double)NAN : v[c];
  const int nl = WBX_EPC_CELLS * npair;
  if (skipna) {
#pragma unroll
    for (int c = 0; c < WBX_EPC_CELLS; ++c) o[(int64_t)(nl + c * npair + q) * nj] = (double)ngood;
  } else if ((flags & WBX_FLAG_MASKED) && q == 0) {
    o[(int64_t)nl * nj] = (double)nvalid;
  }
}

__device__ __forceinline__ uint32_t epc_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// x summed.  grid = nkey * nchunk, block = plan->block_threads; rows are dealt to the waves as in s1_xr_kernel.
template <typename T, int NK, int NP>
__global__ void __launch_bounds__(256) epc_xr_kernel(S1Args a, const double* thr_in, int nthr, const int32_t* slots, int nslot, int nacc) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nwave = blockDim.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const bool masked = a.flags & WBX_FLAG_MASKED;

  __shared__ uint32_t tab[EPC_TABLE];
  epc_table(tab, slots, nslot, a.M);
  T thr[NK];
#pragma unroll
  for (int q = 0; q < NK; ++q) thr[q] = cont_threshold<T>(thr_in, q, nthr);
  EpcCounters<NK, NP> n;
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
        epc_point<T, NK, NP>(a, ro, x, thr, nthr, nslot, tab, n);
      }
    }
  }

  constexpr int NRED = 2 * EPC_PAIRS + EPC_THRESHOLDS + 2;  // tp, np per pair; no per threshold; ngood, nvalid
  static_assert(NK <= EPC_THRESHOLDS && NP <= EPC_PAIRS, "the rows of `red` hold the largest instantiation");
  __shared__ uint32_t red[EPC_MAX_WAVES][NRED];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const uint32_t s0 = epc_wave_sum(n.tp[q]), s1 = epc_wave_sum(n.np[q]);
    if (lane == 0) {
      red[wave][q] = s0;
      red[wave][EPC_PAIRS + q] = s1;
    }
  }
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const uint32_t s = epc_wave_sum(n.no[k]);
    if (lane == 0) red[wave][2 * EPC_PAIRS + k] = s;
  }
  {
    const uint32_t s0 = epc_wave_sum(n.ngood), s1 = epc_wave_sum(n.nvalid);
    if (lane == 0) {
      red[wave][NRED - 2] = s0;
      red[wave][NRED - 1] = s1;
    }
  }
  __syncthreads();
  const int npair = nthr * nslot;
  if ((int)threadIdx.x < npair) {
    const int q = threadIdx.x, k = q / nslot;
    uint32_t s[5] = {0, 0, 0, 0, 0};
    for (int w = 0; w < nwave; ++w) {
      s[0] += red[w][q];
      s[1] += red[w][EPC_PAIRS + q];
      s[2] += red[w][2 * EPC_PAIRS + k];
      s[3] += red[w][NRED - 2];
      s[4] += red[w][NRED - 1];
    }
    epc_write(a.out + (key * a.nchunk + chunk) * (int64_t)nacc, 1, npair, q, a.flags, s[0], s[1], s[2], s[3], s[4]);
  }
}

// x kept.  grid = nkey * nxtile * nchunk, block = plan->block_threads, one x per lane.
template <typename T, int NK, int NP>
__global__ void __launch_bounds__(256) epc_xk_kernel(S1Args a, const double* thr_in, int nthr, const int32_t* slots, int nslot, int nacc) {
  int64_t b = blockIdx.x;
  const int chunk = (int)(b % a.nchunk);
  b /= a.nchunk;
  const int xt = (int)(b % a.nxtile);
  const int64_t key = b / a.nxtile;
  const int64_t x = (int64_t)xt * blockDim.x + threadIdx.x;
  __shared__ uint32_t tab[EPC_TABLE];
  epc_table(tab, slots, nslot, a.M);  // (every thread of the block: the table is built behind a barrier)
  if (x >= a.nx) return;
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const bool masked = a.flags & WBX_FLAG_MASKED;

  T thr[NK];
#pragma unroll
  for (int q = 0; q < NK; ++q) thr[q] = cont_threshold<T>(thr_in, q, nthr);
  EpcCounters<NK, NP> n;
  n.clear();

  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, d, ro);
    if (masked && reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + x * a.xstride[3]] == 0) continue;
    epc_point<T, NK, NP>(a, ro, x, thr, nthr, nslot, tab, n);
  }
  double* o = a.out + ((key * a.nchunk + chunk) * (int64_t)nacc) * a.nx + x;
  const int npair = nthr * nslot;
  int k = 0, j = 0;  // of pair q
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    if (q < npair) {
      uint32_t no = 0;
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) no = kk == k ? n.no[kk] : no;
      epc_write(o, a.nx, npair, q, a.flags, n.tp[q], n.np[q], no, n.ngood, n.nvalid);
      if (++j == nslot) {
        j = 0;
        ++k;
      }
    }
  }
}

// (threshold slots beyond nthr hold +inf and are skipped; pair counters beyond nthr * nslot stay 0 and are not written)
template <typename T>
static int epc_dispatch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const double* thr, int nthr, const int32_t* slots, int nslot,
                        int nacc) {
  return dispatch_slots(nthr, [&](auto nk) {
    constexpr int NK = decltype(nk)::value;
    return dispatch_slots(nthr * nslot, [&](auto np) {
      constexpr int NP = decltype(np)::value < NK ? NK : decltype(np)::value;  // (nthr * nslot >= nthr: never smaller)
      return launch_xk_or_xr(ctx, plan, a, epc_xk_kernel<T, NK, NP>, epc_xr_kernel<T, NK, NP>, thr, nthr, slots, nslot, nacc);
    });
  });
}

}  // namespace wbx

extern "C" int wbx_ens_prob_contingency_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride, int nthr,
                                                const double* thresholds, int nslot, const int32_t* slots, const void* p, const void* t,
                                                const uint8_t* mask, double* partial_out) {
  using namespace wbx;
  const S1Names names = {"wbx_ens_prob_contingency_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  WBX_REQUIRE(nthr >= 1 && nslot >= 1 && (int64_t)nthr * nslot <= WBX_EPC_MAX_PAIRS,
              "wbx_ens_prob_contingency_partial: 1..%d (threshold, slot) pairs per launch (got %d x %d)", WBX_EPC_MAX_PAIRS, nthr, nslot);
  WBX_REQUIRE(M >= 1 && M <= WBX_EPC_MAX_MEMBERS, "wbx_ens_prob_contingency_partial: 1..%d members (got %d)", WBX_EPC_MAX_MEMBERS, M);
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "wbx_ens_prob_contingency_partial: unknown dtype %d", dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA)),
              "wbx_ens_prob_contingency_partial: flags other than MASKED | SKIPNA (0x%x)", plan->flags);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "wbx_ens_prob_contingency_partial: no plane mode, no folded x weights");
  // uint32 counters: a partial meets at most depth_chunk * nx points
  WBX_REQUIRE((double)plan->depth_chunk * (double)(plan->nx > 0 ? plan->nx : 1) < 4294967296.0,
              "wbx_ens_prob_contingency_partial: 2^32 or more points per partial (depth_chunk * nx)");
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, WBX_EPC_CELLS * nthr * nslot);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  WBX_REQUIRE(thresholds != nullptr && slots != nullptr, "wbx_ens_prob_contingency_partial: thresholds or slots is NULL");
  a.M = M;
  a.mstride = member_stride;
  if (dtype == WBX_F32) return epc_dispatch<float>(ctx, plan, a, thresholds, nthr, slots, nslot, nacc);
  return epc_dispatch<double>(ctx, plan, a, thresholds, nthr, slots, nslot, nacc);
}
