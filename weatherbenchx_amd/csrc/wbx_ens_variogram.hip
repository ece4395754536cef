// Variogram score of an ensemble, summed like any other stage-1 statistic: VariogramScore (weatherbenchX/metrics/probabilistic.py:
// 554-600) without the L whole-array passes of the host route.
//
// Reference semantics restated.  Per point, members x_m in R^L (m < M), target y in R^L, the run the L elements along the score's dim:
//   VS = sum_{i, j in [0, L)} ( |y_i - y_j|^p - (1 / M) sum_m |x_i^m - x_j^m|^p )^2
// over ordered pairs, the diagonal included.  The table is symmetric and its diagonal is |v - v|^p: 0 for a finite v, NaN for a NaN or
// infinite one.  So VS = 2 * (sum over i < j), exactly, and a point with ANY non-finite value among its (M + 1) L inputs is NaN
// while every other point is what the off-diagonal pairs give.  The off-diagonal arithmetic alone would not say so (one infinite
// member gives +inf there), hence the decision is explicit: one "all finite" flag per point, assembled while the values are staged.
//
// Mapping.  A block owns a tile of P adjacent x of one row (vgrm_tile_points: what VGRM_ITEMS_TOTAL (point, pair) items and the
// target area hold).  The targets of the tile are staged once, [P][L]; the members in chunks of mc members (vgrm_member_chunk: what
// the staging area holds), [P][mc][L], with loads coalesced along whichever of the run, x and the member axis has stride 1.  The run
// is resident whole.  A thread takes the items tid, tid + threads, ... (8 at most at 256 threads, 32 in the 64- and 128-thread
// blocks an x-kept plan may ask for); an item
// is one pair i < j of one point, its member sum stays in a float64 register across the chunks, and per member it reads two values
// from LDS.
//
// Arithmetic: the difference in the input type; |d|^p in the input type -- a correctly rounded square root of |d| for p = 0.5,
// |d| for p = 1, one rounded product d * d for p = 2 --; everything from the member sum onwards in float64: the M terms in member
// order, the division by M, the difference with the target's term, the square, the pair sum.  No moment identity: it cancels on
// exactly the good forecasts this scores, where the two terms are nearly equal.  (Finite inputs whose product overflows the input
// type at p = 2 are outside what is promised.)
//
// The result is a function of the inputs and the plan only: the pairs of a point are summed from LDS slots in a fixed order
// (VGRM_SPLIT interleaved runs, then those), doubled, replaced by NaN where the point's flag says so; the mask / skipna / NaN
// decision is taken once per point on that value, a thread adds the points it owns in the order they come, and one thread sums
// those.  No floating-point atomics.
#include <cmath>
#include <type_traits>

#include "wbx_s1.hpp"

namespace wbx {

constexpr int VGRM_PMAX = 64;            // points per tile at most
constexpr int VGRM_ITEMS_TOTAL = 2048;   // (point, pair) items per tile at most: 2016 pairs at L = 64
constexpr int VGRM_ITEMS = 32;           // items per thread at most (64- and 128-thread blocks)
constexpr int VGRM_ITEMS_256 = 8;        // ... of 256-thread blocks: a quarter of the accumulators, twice the waves per SIMD
constexpr int VGRM_STAGE = 6144;         // elements of the member staging area
constexpr int VGRM_TGT = 512;            // elements of the target area
constexpr int VGRM_SPLIT = 16;           // interleaved runs the pairs of a point are summed in
static_assert(WBX_VGRAM_MAX_RUN * (WBX_VGRAM_MAX_RUN - 1) / 2 <= VGRM_ITEMS_TOTAL, "one point must fit the items");
static_assert(VGRM_ITEMS * 64 >= VGRM_ITEMS_TOTAL && VGRM_ITEMS_256 * 256 >= VGRM_ITEMS_TOTAL, "a block must hold a tile's items");
static_assert(WBX_VGRAM_MAX_RUN <= VGRM_TGT && VGRM_TGT * 1 <= VGRM_STAGE, "one member of a full tile must fit the staging area");
static_assert(VGRM_STAGE * sizeof(float) >= (VGRM_ITEMS_TOTAL + VGRM_PMAX * VGRM_SPLIT) * sizeof(double),
              "the staging area also holds the pairs' terms and the runs' sums");
static_assert(WBX_VGRAM_MAX_RUN <= 256 && VGRM_PMAX <= 256, "an item packs point, i and j into bytes");

// Points per tile and members per chunk (tests/variogram_cases.py restates both).
static inline int vgrm_tile_points(int64_t L) {
  const int npair = (int)(L * (L - 1) / 2);
  int p = VGRM_PMAX;
  if (npair > 0 && VGRM_ITEMS_TOTAL / npair < p) p = VGRM_ITEMS_TOTAL / npair;
  if (VGRM_TGT / (int)L < p) p = VGRM_TGT / (int)L;
  return p < 1 ? 1 : p;
}
static inline int vgrm_member_chunk(int M, int64_t L, int P) {
  const int mc = VGRM_STAGE / (P * (int)L);
  return mc < M ? mc : M;
}

struct VgrmArgs {
  int64_t pls, tls;              // element strides of the run in p and t
  int32_t L, npair, P, mc, mode;  // run length, L (L - 1) / 2, points per tile, members per chunk;
                                  // staging order: 0 the run fastest, 1 x fastest, 2 members fastest
};

// |d|^p in the input type.  POW is the power's code (wbx.h).
template <typename T, int POW>
__device__ __forceinline__ T vgrm_pow(T d) {
  if constexpr (POW == WBX_VGRAM_POW_ONE) {
    return fabs(d);
  } else if constexpr (POW == WBX_VGRAM_POW_TWO) {  // (never contracted into the float64 member sum)
    if constexpr (std::is_same<T, float>::value)
      return __fmul_rn(d, d);
    else
      return __dmul_rn(d, d);
  } else {
    if constexpr (std::is_same<T, float>::value)
      return __fsqrt_rn(fabs(d));
    else
      return __dsqrt_rn(fabs(d));
  }
}

template <typename T>
struct VgrmBlock {
  T* stage;        // [P][mc][L]; afterwards double term[items], then double run[P][SPLIT]
  T* tgt;          // [P][L]
  uint32_t* itm;   // [P * npair]: point << 16 | i << 8 | j
  uint32_t* fin;   // [P]: 1 until a non-finite value of the point is staged
};

// One tile: points x0 .. x0 + npts - 1 of the row at ro[] -> the score of point threadIdx.x (threads < npts).
template <typename T, int POW, int ITEMS>
__device__ __forceinline__ double vgrm_tile(const S1Args& a, const VgrmArgs& e, const VgrmBlock<T>& B, const int64_t (&ro)[WBX_MAX_INPUTS],
                                            int64_t x0, int npts) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const T* p = reinterpret_cast<const T*>(a.in[0]) + ro[0] + x0 * a.xstride[0];
  const T* t = reinterpret_cast<const T*>(a.in[1]) + ro[1] + x0 * a.xstride[1];
  const int M = a.M, L = e.L;
  const int nitem = npts * e.npair;
  double acc[ITEMS];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) acc[k] = 0.0;

  for (int m0 = 0; m0 < M; m0 += e.mc) {
    const int mc = M - m0 < e.mc ? M - m0 : e.mc;
    const int nv = mc + (m0 == 0 ? 1 : 0);  // the first chunk brings the targets along as vector number mc
    // stage: every (vector, point, element) once, the index with stride 1 in memory fastest among the threads
    const unsigned n0 = e.mode == 0 ? L : (e.mode == 1 ? npts : nv);
    const unsigned n1 = e.mode == 0 ? npts : (e.mode == 1 ? L : npts);
    const unsigned total = (unsigned)L * npts * nv;
    for (unsigned idx = tid; idx < total; idx += nt) {
      const unsigned i0 = idx % n0, r = idx / n0, i1 = r % n1, i2 = r / n1;
      const int l = e.mode == 0 ? i0 : (e.mode == 1 ? i1 : i2);
      const int pt = e.mode == 0 ? i1 : (e.mode == 1 ? i0 : i1);
      const int v = e.mode == 0 ? i2 : (e.mode == 1 ? i2 : i0);
      T w;
      if (v < mc) {
        w = p[(int64_t)pt * a.xstride[0] + (int64_t)(m0 + v) * a.mstride + (int64_t)l * e.pls];
        B.stage[(pt * mc + v) * L + l] = w;
      } else {
        w = t[(int64_t)pt * a.xstride[1] + (int64_t)l * e.tls];
        B.tgt[pt * L + l] = w;
      }
      if (!__builtin_isfinite(w)) B.fin[pt] = 0;  // (every writer writes the same)
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int it = tid + k * nt;
      if (it < nitem) {
        const uint32_t w = B.itm[it];
        const T* row = B.stage + (int)(w >> 16) * mc * L;
        const int i = (w >> 8) & 255, j = w & 255;
        double s = acc[k];
#pragma unroll 4  // (four members' LDS reads in flight; the sum stays in member order)
        for (int m = 0; m < mc; ++m) s += (double)vgrm_pow<T, POW>(row[m * L + i] - row[m * L + j]);
        acc[k] = s;
      }
    }
    __syncthreads();  // the staging area is free again
  }

  // a pair's term: (|y_i - y_j|^p - member sum / M)^2
  double* term = reinterpret_cast<double*>(B.stage);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int it = tid + k * nt;
    if (it < nitem) {
      const uint32_t w = B.itm[it];
      const T* y = B.tgt + (int)(w >> 16) * L;
      const double ty = (double)vgrm_pow<T, POW>(y[(w >> 8) & 255] - y[w & 255]);
      const double d = ty - acc[k] / (double)M;
      term[it] = d * d;
    }
  }
  __syncthreads();
  // a point's pairs: VGRM_SPLIT interleaved runs ...
  double* run = term + VGRM_ITEMS_TOTAL;
  for (int q = tid; q < npts * VGRM_SPLIT; q += nt) {
    const int pt = q / VGRM_SPLIT, first = q % VGRM_SPLIT;
    double sum = 0.0;
    for (int b = first; b < e.npair; b += VGRM_SPLIT) sum += term[pt * e.npair + b];
    run[q] = sum;
  }
  __syncthreads();
  // ... and the runs, by the point's thread, which also takes the point's decision and resets its flag for the next tile
  double v = 0.0;
  if (tid < npts) {
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < VGRM_SPLIT; ++r) s += run[tid * VGRM_SPLIT + r];
    v = B.fin[tid] ? 2.0 * s : __builtin_nan("");
    B.fin[tid] = 1;
  }
  __syncthreads();  // the next tile stages over the sums
  return v;
}

// The decision per point, on the assembled value: the sum, then the count lane of a mask or of skipna.
struct VgrmSums {
  double s = 0.0, c = 0.0;
};

__device__ __forceinline__ void vgrm_account(uint32_t flags, bool valid, double v, VgrmSums& acc) {
  const bool g = valid && (!(flags & WBX_FLAG_SKIPNA) || v == v);  // (a NaN under a valid point poisons its partial)
  acc.s += g ? v : 0.0;
  acc.c += g ? 1.0 : 0.0;
}

template <typename T>
__device__ __forceinline__ void vgrm_setup(const VgrmArgs& e, T* stage, T* tgt, uint32_t* itm, uint32_t* fin, VgrmBlock<T>& B) {
  B.stage = stage;
  B.tgt = tgt;
  B.itm = itm;
  B.fin = fin;
  const int L = e.L;
  for (int r = threadIdx.x; r < e.P * L; r += blockDim.x) {  // row i of point pt: its pairs (i, j > i), rows first
    const int pt = r / L, i = r - pt * L;
    uint32_t* o = itm + pt * e.npair + i * (2 * L - i - 1) / 2 - (i + 1);
    for (int j = i + 1; j < L; ++j) o[j] = ((uint32_t)pt << 16) | ((uint32_t)i << 8) | (uint32_t)j;
  }
  for (int pt = threadIdx.x; pt < VGRM_PMAX; pt += blockDim.x) fin[pt] = 1;
  __syncthreads();
}

// x summed.  grid = nkey * nchunk, block = 256 threads.
template <typename T, int POW, int ITEMS>
__global__ void __launch_bounds__(256) vgrm_xr_kernel(S1Args a, VgrmArgs e, int nacc) {
  __shared__ __attribute__((aligned(16))) T stage[VGRM_STAGE];
  __shared__ T tgt[VGRM_TGT];
  __shared__ uint32_t itm[VGRM_ITEMS_TOTAL];
  __shared__ uint32_t fin[VGRM_PMAX];
  __shared__ double red[VGRM_PMAX][2];
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const bool masked = a.flags & WBX_FLAG_MASKED;
  VgrmBlock<T> B;
  vgrm_setup<T>(e, stage, tgt, itm, fin, B);
  VgrmSums acc;
  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, d, ro);
    for (int64_t x0 = 0; x0 < a.nx; x0 += e.P) {
      const int npts = (int)(a.nx - x0 < e.P ? a.nx - x0 : e.P);
      const double v = vgrm_tile<T, POW, ITEMS>(a, e, B, ro, x0, npts);
      if ((int)threadIdx.x < npts) {
        const bool valid = !masked || reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + (x0 + threadIdx.x) * a.xstride[3]] != 0;
        vgrm_account(a.flags, valid, v, acc);
      }
    }
  }
  if ((int)threadIdx.x < e.P) {
    red[threadIdx.x][0] = acc.s;
    red[threadIdx.x][1] = acc.c;
  }
  __syncthreads();
  if ((int)threadIdx.x < nacc) {  // lane q of the partial: the tile's threads in order
    double s = 0.0;
    for (int pt = 0; pt < e.P; ++pt) s += red[pt][threadIdx.x];
    a.out[(key * a.nchunk + chunk) * (int64_t)nacc + threadIdx.x] = s;
  }
}

// x kept.  grid = nkey * nxtile * nchunk, block = plan->block_threads; a block covers blockDim x in tiles of P.
template <typename T, int POW, int ITEMS>
__global__ void __launch_bounds__(256) vgrm_xk_kernel(S1Args a, VgrmArgs e, int nacc) {
  __shared__ __attribute__((aligned(16))) T stage[VGRM_STAGE];
  __shared__ T tgt[VGRM_TGT];
  __shared__ uint32_t itm[VGRM_ITEMS_TOTAL];
  __shared__ uint32_t fin[VGRM_PMAX];
  int64_t b = blockIdx.x;
  const int chunk = (int)(b % a.nchunk);
  b /= a.nchunk;
  const int xt = (int)(b % a.nxtile);
  const int64_t key = b / a.nxtile;
  const int64_t xlo = (int64_t)xt * blockDim.x;
  const int64_t xhi = xlo + blockDim.x < a.nx ? xlo + blockDim.x : a.nx;
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const bool masked = a.flags & WBX_FLAG_MASKED;
  VgrmBlock<T> B;
  vgrm_setup<T>(e, stage, tgt, itm, fin, B);
  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  for (int64_t x0 = xlo; x0 < xhi; x0 += e.P) {
    const int npts = (int)(xhi - x0 < e.P ? xhi - x0 : e.P);
    VgrmSums acc;
    for (int64_t d = d0; d < d1; ++d) {
      int64_t ro[WBX_MAX_INPUTS];
      row_bases<2>(a, kb, key, d, ro);
      const double v = vgrm_tile<T, POW, ITEMS>(a, e, B, ro, x0, npts);
      if ((int)threadIdx.x < npts) {
        const bool valid = !masked || reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + (x0 + threadIdx.x) * a.xstride[3]] != 0;
        vgrm_account(a.flags, valid, v, acc);
      }
    }
    if ((int)threadIdx.x < npts) {
      double* o = a.out + ((key * a.nchunk + chunk) * (int64_t)nacc) * a.nx + x0 + threadIdx.x;
      o[0] = acc.s;
      if (nacc > 1) o[a.nx] = acc.c;
    }
  }
}

// x kept runs the plan's block (a block covers that many x); x summed always runs 256 threads: an x-summed plan's block size says how
// streaming kernels sweep a row, while this kernel wants a tile's items over as many threads as its LDS lets a CU hold.
template <typename T, int POW>
static int vgrm_launch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const VgrmArgs& e, int nacc) {
  if (!plan->x_kept) {
    wbx_s1_plan wide = *plan;
    wide.block_threads = 256;
    return launch_xk_or_xr(ctx, &wide, a, vgrm_xk_kernel<T, POW, VGRM_ITEMS_256>, vgrm_xr_kernel<T, POW, VGRM_ITEMS_256>, e, nacc);
  }
  if (plan->block_threads == 256)
    return launch_xk_or_xr(ctx, plan, a, vgrm_xk_kernel<T, POW, VGRM_ITEMS_256>, vgrm_xr_kernel<T, POW, VGRM_ITEMS_256>, e, nacc);
  return launch_xk_or_xr(ctx, plan, a, vgrm_xk_kernel<T, POW, VGRM_ITEMS>, vgrm_xr_kernel<T, POW, VGRM_ITEMS_256>, e, nacc);
}

template <typename T>
static int vgrm_launch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const VgrmArgs& e, int power, int nacc) {
  if (power == WBX_VGRAM_POW_ONE) return vgrm_launch<T, WBX_VGRAM_POW_ONE>(ctx, plan, a, e, nacc);
  if (power == WBX_VGRAM_POW_TWO) return vgrm_launch<T, WBX_VGRAM_POW_TWO>(ctx, plan, a, e, nacc);
  return vgrm_launch<T, WBX_VGRAM_POW_HALF>(ctx, plan, a, e, nacc);
}

}  // namespace wbx

extern "C" int wbx_ens_variogram_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride, int64_t L,
                                         int64_t p_run_stride, int64_t t_run_stride, int power, const void* p, const void* t,
                                         const uint8_t* mask, double* partial_out) {
  using namespace wbx;
  const S1Names names = {"wbx_ens_variogram_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  WBX_REQUIRE(M >= 1 && M <= WBX_VGRAM_MAX_MEMBERS, "wbx_ens_variogram_partial: 1..%d members (got %d)", WBX_VGRAM_MAX_MEMBERS, M);
  WBX_REQUIRE(L >= 1 && L <= WBX_VGRAM_MAX_RUN, "wbx_ens_variogram_partial: a run of 1..%d elements (got %lld)", WBX_VGRAM_MAX_RUN,
              (long long)L);
  WBX_REQUIRE(power == WBX_VGRAM_POW_HALF || power == WBX_VGRAM_POW_ONE || power == WBX_VGRAM_POW_TWO,
              "wbx_ens_variogram_partial: unknown power code %d", power);
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "wbx_ens_variogram_partial: unknown dtype %d", dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA)), "wbx_ens_variogram_partial: flags other than MASKED | SKIPNA (0x%x)",
              plan->flags);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "wbx_ens_variogram_partial: no plane mode, no folded x weights");
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, WBX_VGRAM_LANES);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  a.M = M;
  a.mstride = member_stride;
  VgrmArgs e;
  e.pls = p_run_stride;
  e.tls = t_run_stride;
  e.L = (int32_t)L;
  e.npair = (int32_t)(L * (L - 1) / 2);
  e.P = vgrm_tile_points(L);
  e.mc = vgrm_member_chunk(M, L, e.P);
  e.mode = (L > 1 && (p_run_stride == 1 || p_run_stride == -1)) ? 0 : (plan->xstride[0] == 1 ? 1 : (member_stride == 1 ? 2 : 1));
  if (dtype == WBX_F32) return vgrm_launch<float>(ctx, plan, a, e, power, nacc);
  return vgrm_launch<double>(ctx, plan, a, e, power, nacc);
}
