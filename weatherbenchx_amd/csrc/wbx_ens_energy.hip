// Energy score of an ensemble, both terms in one pass, summed like any other stage-1 statistic: EnergyScoreSkill and
// EnergyScoreSpread (weatherbenchX/metrics/probabilistic.py:480-551) without the M - 1 whole-array passes of the host route.
//
// Reference semantics restated.  Per point, members x_m in R^L (m < M), target y in R^L, the norm over the L elements of the norm run:
//   lane 0 (skill)  = (sum_m ||x_m - y||) / M
//   lane 1 (spread) = (sum_{m != m'} ||x_m - x_m'||) / D,   D = M (M - 1) under WBX_FLAG_FAIR, M^2 otherwise
// NaN and inf are whatever IEEE arithmetic makes of them: a NaN member makes both lanes NaN, a NaN target lane 0 only, an infinite
// member against finite ones +inf, two infinite members of one sign NaN in lane 1 (inf - inf).  A member is never paired with itself.
//
// Mapping.  The target is vector number M: a point's work is the strict upper triangle of an (M + 1) x (M + 1) table of squared
// distances, pairs (m, M) feed lane 0, pairs (m, m') lane 1 (each unordered pair once: the ordered sum is twice that, exactly).
// A block owns a tile of P adjacent x of one row and stages [P][Lc][M + 1 padded to 4] values in LDS for a chunk of Lc elements of
// the norm run, with loads coalesced along whichever of the norm run, x and the member axis has stride 1.  A thread takes up to
// ENRG_ITEMS 4 x 4 blocks of vector pairs (52 = 13 x 4 vectors at M = 51: 91 blocks per point); its 16 accumulators per block
// stay in registers across the chunks, and per element of the run it reads 2 x 4 values from LDS for 16 subtractions and 16 fmas.
// Diagonal blocks skip i >= j, all blocks skip the padding slots.
//
// Arithmetic: difference, square and sum in the input type (fma, in the order of the run), a correctly rounded square root in the
// input type, everything after that in float64.  No Gram identity: it cancels on exactly the tight ensembles this scores.
//
// The result is a function of the inputs and the plan only: a thread sums the norms of a block in a fixed order, the blocks of a
// point are summed from LDS slots in a fixed order (ENRG_SPLIT interleaved runs, then those), the mask / skipna / poison decision
// is taken once per point and lane on the assembled value, a thread adds the points it owns in the order they come, and one thread
// sums those.  No floating-point atomics.
#include <cmath>
#include <type_traits>

#include "wbx_s1.hpp"

namespace wbx {

constexpr int ENRG_LC = 16;          // elements of the norm run per LDS chunk
constexpr int ENRG_PMAX = 64;        // points per tile at most
constexpr int ENRG_VECS = 416;       // P * (M + 1 padded to 4) at most: 8 points at M = 51
constexpr int ENRG_ITEMS = 3;        // 4 x 4 blocks per thread at most
constexpr int ENRG_SPLIT = 8;        // interleaved runs the blocks of a point are summed in
constexpr int ENRG_PAD = 4;          // elements between two points' slabs (their starts then fall into different LDS banks)
constexpr int ENRG_ELEMS = ENRG_VECS * ENRG_LC + ENRG_PMAX * ENRG_PAD;
constexpr int ENRG_MAX_BLOCKS = ((WBX_ENRG_MAX_MEMBERS + 4) / 4) * ((WBX_ENRG_MAX_MEMBERS + 4) / 4 + 1) / 2;
static_assert(ENRG_MAX_BLOCKS <= ENRG_ITEMS * 64, "one point must fit the smallest block's items");
static_assert(ENRG_ELEMS * sizeof(float) >= (ENRG_ITEMS * 256 * 2 + ENRG_PMAX * 2 * ENRG_SPLIT) * sizeof(double),
              "the staging area also holds the blocks' sums");
static_assert((WBX_ENRG_MAX_MEMBERS + 4) / 4 * 4 <= ENRG_VECS, "one point must fit the staging area");

// Points per tile: what the staging area and the threads' items hold (tests/energy_cases.py restates this).
static inline int enrg_tile_points(int M, int threads) {
  const int mp = (M + 4) / 4 * 4, nb = mp / 4, nblk = nb * (nb + 1) / 2;
  int p = ENRG_PMAX;
  if (ENRG_VECS / mp < p) p = ENRG_VECS / mp;
  if (ENRG_ITEMS * threads / nblk < p) p = ENRG_ITEMS * threads / nblk;
  return p < 1 ? 1 : p;
}

struct EnrgArgs {
  int64_t L, pls, tls;  // the norm run: length, element strides in p and t
  int32_t P, mode;      // points per tile; staging order: 0 the run fastest, 1 x fastest, 2 members fastest
  double members, denom;  // lane 0 = sum / members; lane 1 = 2 * sum / denom
};

template <typename T>
__device__ __forceinline__ T enrg_sqrt(T v) {
  if constexpr (std::is_same<T, float>::value)
    return __fsqrt_rn(v);
  else
    return __dsqrt_rn(v);
}

template <typename T>
struct EnrgBlock {
  using V4 = T __attribute__((ext_vector_type(4)));
  T* stage;  // 32-byte aligned: [P][Lc * MP + PAD]; afterwards double part[items][2], then double run[P][2][SPLIT]
  uint8_t* bij;                           // [nblk][2]
  int M, MP, nblk, pstride;
  int it_pt[ENRG_ITEMS], it_i[ENRG_ITEMS], it_j[ENRG_ITEMS];  // this thread's items: point of the tile, block row and column
};

// One tile: points x0 .. x0 + npts - 1 of the row at ro[] -> the assembled lanes v0, v1 of point threadIdx.x (threads < npts).
template <typename T>
__device__ __forceinline__ void enrg_tile(const S1Args& a, const EnrgArgs& e, const EnrgBlock<T>& B, const int64_t (&ro)[WBX_MAX_INPUTS],
                                          int64_t x0, int npts, double& v0, double& v1) {
  using V4 = typename EnrgBlock<T>::V4;
  const int tid = threadIdx.x, nt = blockDim.x;
  const T* p = reinterpret_cast<const T*>(a.in[0]) + ro[0] + x0 * a.xstride[0];
  const T* t = reinterpret_cast<const T*>(a.in[1]) + ro[1] + x0 * a.xstride[1];
  const int M = B.M, MP = B.MP;
  T acc[ENRG_ITEMS][16];
#pragma unroll
  for (int k = 0; k < ENRG_ITEMS; ++k)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[k][q] = (T)0;

  for (int64_t l0 = 0; l0 < e.L; l0 += ENRG_LC) {
    const int lc = (int)(e.L - l0 < ENRG_LC ? e.L - l0 : ENRG_LC);
    // stage: every (vector, point, element) once, the index with stride 1 in memory fastest among the threads
    const unsigned n0 = e.mode == 0 ? lc : (e.mode == 1 ? npts : M + 1);
    const unsigned n1 = e.mode == 0 ? npts : (e.mode == 1 ? lc : npts);
    const unsigned total = (unsigned)lc * npts * (M + 1);
    for (unsigned idx = tid; idx < total; idx += nt) {
      const unsigned i0 = idx % n0, r = idx / n0, i1 = r % n1, i2 = r / n1;
      const int l = e.mode == 0 ? i0 : (e.mode == 1 ? i1 : i2);
      const int pt = e.mode == 0 ? i1 : (e.mode == 1 ? i0 : i1);
      const int v = e.mode == 0 ? i2 : (e.mode == 1 ? i2 : i0);
      const T w = v < M ? p[(int64_t)pt * a.xstride[0] + (int64_t)v * a.mstride + (l0 + l) * e.pls]
                        : t[(int64_t)pt * a.xstride[1] + (l0 + l) * e.tls];
      B.stage[pt * B.pstride + l * MP + v] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ENRG_ITEMS; ++k) {
      if (B.it_pt[k] < npts) {
        const T* base = B.stage + B.it_pt[k] * B.pstride;
        for (int l = 0; l < lc; ++l) {
          const V4 av = *reinterpret_cast<const V4*>(base + l * MP + 4 * B.it_i[k]);
          const V4 bv = *reinterpret_cast<const V4*>(base + l * MP + 4 * B.it_j[k]);
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const T d = av[r] - bv[c];
              acc[k][r * 4 + c] = fma(d, d, acc[k][r * 4 + c]);
            }
        }
      }
    }
    __syncthreads();  // the staging area is free again
  }

  // a block's norms in the order (r, c): pairs with the target to lane 0, member pairs to lane 1
  double* part = reinterpret_cast<double*>(B.stage);
#pragma unroll
  for (int k = 0; k < ENRG_ITEMS; ++k) {
    if (B.it_pt[k] < npts) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int i = 4 * B.it_i[k] + r, j = 4 * B.it_j[k] + c;
          if (i < j && j <= M) {
            const double n = (double)enrg_sqrt<T>(acc[k][r * 4 + c]);
            if (j == M)
              s0 += n;
            else
              s1 += n;
          }
        }
      const int it = tid + k * nt;
      part[2 * it] = s0;
      part[2 * it + 1] = s1;
    }
  }
  __syncthreads();
  // a point's blocks: ENRG_SPLIT interleaved runs per lane ...
  double* run = part + 2 * ENRG_ITEMS * 256;
  for (int q = tid; q < npts * 2 * ENRG_SPLIT; q += nt) {
    const int pt = q / (2 * ENRG_SPLIT), s = q % (2 * ENRG_SPLIT), lane = s & 1, first = s >> 1;
    double sum = 0.0;
    for (int b = first; b < B.nblk; b += ENRG_SPLIT) sum += part[2 * (pt * B.nblk + b) + lane];
    run[q] = sum;
  }
  __syncthreads();
  // ... and the runs, by the point's thread
  v0 = v1 = 0.0;
  if (tid < npts) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int s = 0; s < ENRG_SPLIT; ++s) {
      s0 += run[tid * 2 * ENRG_SPLIT + 2 * s];
      s1 += run[tid * 2 * ENRG_SPLIT + 2 * s + 1];
    }
    v0 = s0 / e.members;
    v1 = (2.0 * s1) / e.denom;
  }
  __syncthreads();  // the next tile stages over the sums
}

// The decision per point and lane, on the assembled value: the two sums, then the two count lanes of skipna or (c0) the shared one
// of a mask alone.
struct EnrgSums {
  double s0 = 0.0, s1 = 0.0, c0 = 0.0, c1 = 0.0;
};

__device__ __forceinline__ void enrg_account(uint32_t flags, bool valid, double v0, double v1, EnrgSums& acc) {
  const bool skipna = flags & WBX_FLAG_SKIPNA;
  const bool g0 = valid && (!skipna || v0 == v0), g1 = valid && (!skipna || v1 == v1);  // (a NaN under a valid point poisons its lane)
  acc.s0 += g0 ? v0 : 0.0;
  acc.s1 += g1 ? v1 : 0.0;
  acc.c0 += g0 ? 1.0 : 0.0;
  acc.c1 += g1 ? 1.0 : 0.0;
}

// Lane q of a partial with `nacc` lanes from the sums.
__device__ __forceinline__ double enrg_lane(const EnrgSums& acc, int q) {
  return q == 0 ? acc.s0 : (q == 1 ? acc.s1 : (q == 2 ? acc.c0 : acc.c1));
}

template <typename T>
__device__ __forceinline__ void enrg_setup(const S1Args& a, const EnrgArgs& e, T* stage, uint8_t* bij, EnrgBlock<T>& B) {
  B.stage = stage;
  B.bij = bij;
  B.M = a.M;
  B.MP = (a.M + 4) / 4 * 4;
  const int nb = B.MP / 4;
  B.nblk = nb * (nb + 1) / 2;
  B.pstride = ENRG_LC * B.MP + ENRG_PAD;
  for (int b = threadIdx.x; b < B.nblk; b += blockDim.x) {  // block b -> (row, column), rows first
    int i = 0, left = b;
    while (left >= nb - i) {
      left -= nb - i;
      ++i;
    }
    bij[2 * b] = (uint8_t)i;
    bij[2 * b + 1] = (uint8_t)(i + left);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ENRG_ITEMS; ++k) {
    const int it = threadIdx.x + k * blockDim.x;
    const int pt = it / B.nblk, b = it - pt * B.nblk;
    B.it_pt[k] = pt < e.P ? pt : ENRG_PMAX;  // (never below npts)
    B.it_i[k] = bij[2 * b];
    B.it_j[k] = bij[2 * b + 1];
  }
}

// x summed.  grid = nkey * nchunk, block = plan->block_threads.
template <typename T>
__global__ void __launch_bounds__(256) enrg_xr_kernel(S1Args a, EnrgArgs e, int nacc) {
  __shared__ __attribute__((aligned(32))) T stage[ENRG_ELEMS];
  __shared__ uint8_t bij[2 * ENRG_MAX_BLOCKS];
  __shared__ double red[ENRG_PMAX][4];
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const bool masked = a.flags & WBX_FLAG_MASKED;
  EnrgBlock<T> B;
  enrg_setup<T>(a, e, stage, bij, B);
  EnrgSums acc;
  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<2>(a, kb, key, d, ro);
    for (int64_t x0 = 0; x0 < a.nx; x0 += e.P) {
      const int npts = (int)(a.nx - x0 < e.P ? a.nx - x0 : e.P);
      double v0, v1;
      enrg_tile<T>(a, e, B, ro, x0, npts, v0, v1);
      if ((int)threadIdx.x < npts) {
        const bool valid = !masked || reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + (x0 + threadIdx.x) * a.xstride[3]] != 0;
        enrg_account(a.flags, valid, v0, v1, acc);
      }
    }
  }
  if ((int)threadIdx.x < e.P) {
#pragma unroll
    for (int q = 0; q < 4; ++q) red[threadIdx.x][q] = enrg_lane(acc, q);
  }
  __syncthreads();
  if ((int)threadIdx.x < nacc) {  // lane q of the partial: the tile's threads in order
    double s = 0.0;
    for (int pt = 0; pt < e.P; ++pt) s += red[pt][threadIdx.x];
    a.out[(key * a.nchunk + chunk) * (int64_t)nacc + threadIdx.x] = s;
  }
}

// x kept.  grid = nkey * nxtile * nchunk, block = plan->block_threads; a block covers blockDim x in tiles of P.
template <typename T>
__global__ void __launch_bounds__(256) enrg_xk_kernel(S1Args a, EnrgArgs e, int nacc) {
  __shared__ __attribute__((aligned(32))) T stage[ENRG_ELEMS];
  __shared__ uint8_t bij[2 * ENRG_MAX_BLOCKS];
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
  EnrgBlock<T> B;
  enrg_setup<T>(a, e, stage, bij, B);
  int64_t kb[WBX_MAX_INPUTS];
  key_bases<2>(a, key, kb);
  for (int64_t x0 = xlo; x0 < xhi; x0 += e.P) {
    const int npts = (int)(xhi - x0 < e.P ? xhi - x0 : e.P);
    EnrgSums acc;
    for (int64_t d = d0; d < d1; ++d) {
      int64_t ro[WBX_MAX_INPUTS];
      row_bases<2>(a, kb, key, d, ro);
      double v0, v1;
      enrg_tile<T>(a, e, B, ro, x0, npts, v0, v1);
      if ((int)threadIdx.x < npts) {
        const bool valid = !masked || reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + (x0 + threadIdx.x) * a.xstride[3]] != 0;
        enrg_account(a.flags, valid, v0, v1, acc);
      }
    }
    if ((int)threadIdx.x < npts) {
      double* o = a.out + ((key * a.nchunk + chunk) * (int64_t)nacc) * a.nx + x0 + threadIdx.x;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < nacc) o[(int64_t)q * a.nx] = enrg_lane(acc, q);
    }
  }
}

}  // namespace wbx

extern "C" int wbx_ens_energy_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride, int64_t L,
                                      int64_t p_norm_stride, int64_t t_norm_stride, const void* p, const void* t, const uint8_t* mask,
                                      double* partial_out) {
  using namespace wbx;
  static_assert(WBX_ENRG_MAX_MEMBERS >= 64 && WBX_ENRG_MAX_MEMBERS + 4 <= 4 * 255, "block rows and columns are bytes");
  const S1Names names = {"wbx_ens_energy_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  WBX_REQUIRE(M >= 2 && M <= WBX_ENRG_MAX_MEMBERS, "wbx_ens_energy_partial: 2..%d members (got %d)", WBX_ENRG_MAX_MEMBERS, M);
  WBX_REQUIRE(L >= 1, "wbx_ens_energy_partial: the norm run needs at least 1 element (got %lld)", (long long)L);
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "wbx_ens_energy_partial: unknown dtype %d", dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA | WBX_FLAG_FAIR)),
              "wbx_ens_energy_partial: flags other than MASKED | SKIPNA | FAIR (0x%x)", plan->flags);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "wbx_ens_energy_partial: no plane mode, no folded x weights");
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  const int nacc = (int)partial_lanes(plan->flags, WBX_ENRG_LANES);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  a.M = M;
  a.mstride = member_stride;
  EnrgArgs e;
  e.L = L;
  e.pls = p_norm_stride;
  e.tls = t_norm_stride;
  e.P = enrg_tile_points(M, plan->block_threads);
  e.mode = (L > 1 && (p_norm_stride == 1 || p_norm_stride == -1)) ? 0 : (plan->xstride[0] == 1 ? 1 : (member_stride == 1 ? 2 : 1));
  e.members = (double)M;
  e.denom = (plan->flags & WBX_FLAG_FAIR) ? (double)M * (double)(M - 1) : (double)M * (double)M;
  if (dtype == WBX_F32) return launch_xk_or_xr(ctx, plan, a, enrg_xk_kernel<float>, enrg_xr_kernel<float>, e, nacc);
  return launch_xk_or_xr(ctx, plan, a, enrg_xk_kernel<double>, enrg_xr_kernel<double>, e, nacc);
}
