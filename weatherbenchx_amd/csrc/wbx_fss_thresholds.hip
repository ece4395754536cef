// The three terms of the fractions skill score of THRESHOLDED continuous fields -- what FSS is behind ContinuousToBinary('both') --
// for up to WBX_FSS_THR_MAX thresholds from one sweep over p and t per launch (include/wbx.h has the contract in full): no indicator
// field is formed, and every window sum is an integer count.
//
// The mapping is fss_kernel's (wbx_fss.hip): a block of 256 threads owns one (key, depth chunk, band of B output latitudes) and whole
// longitude circles, thread l owns the columns l + 256 c.  What differs:
//   * per owned column and threshold the VERTICAL window counts of p and t (members over the threshold) share one 32-bit register,
//     16 + 16 bits (a count is at most n <= 2047); the two NaN counts of the column share another, once, whatever the number of
//     thresholds.  Packed counts slide like plain ones: a row leaves only after it entered, so neither half ever borrows;
//   * per output row the packed counts are widened to 32 + 32 bits (a prefix value stays below nlon * n < 2^22) and go through the
//     block-wide inclusive prefix over the circle as ONE 64-bit integer per threshold, plus one for the NaN counts: KB + 1 scans a
//     row.  The run prefix is formed in place in LDS, so only the KB + 1 run totals are live across the wave scan;
//   * the fractions are (float)((double)count / (double)(n * n)) and the lanes of a threshold are summed exactly as fss_kernel sums
//     them -- thread (columns in order), wave shuffles, the wave's own LDS slot field after field, the four waves in order at the
//     end -- so lanes 3k..3k+2 (and their count lanes) are bit for bit what wbx_fss_partial writes on the float32 indicator fields.
// A launch carries KB thresholds (1 or 2: the entry cuts nthr into pairs, a last single threshold has its own instantiation);
// launches write disjoint lane slices of the partial.  No atomics.  Why two: DESIGN 4.17 (four fit the registers and the LDS, but
// leave one block a CU, and a lone wave per SIMD hides none of the scans' latency).
#include "wbx_cont_threshold.hpp"
#include "wbx_fss.hpp"

namespace wbx {

constexpr int FSS_KB = 2;  // thresholds per launch: 8 (KB + 1) B of prefix per column and 12 KiB of row accumulators per threshold in LDS
static_assert(WBX_FSS_THR_MAX % FSS_KB == 0, "whole launches up to the limit");
static_assert(WBX_FSS_MAX_NLON * 2047LL < (1LL << 32), "a prefix value fits half of a 64-bit integer");

struct FssThrArgs {
  const double* thr;  // DEVICE [nthr]
  int32_t k0, kb, nthr;  // this launch: thresholds [k0, k0 + kb) of nthr
};

__device__ __forceinline__ unsigned long long fss_widen(uint32_t v) {  // 16 + 16 -> 32 + 32
  return (unsigned long long)(v & 0xffffu) | ((unsigned long long)(v >> 16) << 32);
}

// grid = nkey * nchunk * nband, block = 256.  N1: n == 1 (no window, no border).
template <typename T, int NC, int KB, bool N1>
__global__ void __launch_bounds__(FSS_THREADS) fss_thr_kernel(FssArgs a, FssThrArgs h) {
  using u64 = unsigned long long;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t b = blockIdx.x;
  const int band = (int)(b % a.nband);
  b /= a.nband;
  const int chunk = (int)(b % a.nchunk);
  const int64_t key = b / a.nchunk;
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const int nlat = a.nlat, nlon = a.nlon, n = a.n, hw = (n - 1) / 2;
  const int y0 = band * a.B, y1 = y0 + a.B < nlat ? y0 + a.B : nlat;
  const int ys = y0 > hw ? y0 : hw, ye = y1 < nlat - hw ? y1 : nlat - hw;  // the band's rows that are no border rows: [ys, ye)
  const bool masked = a.flags & WBX_FLAG_MASKED, skipna = a.flags & WBX_FLAG_SKIPNA;
  const int nacc1 = skipna ? 2 * WBX_FSS_LANES : (masked ? WBX_FSS_LANES + 1 : WBX_FSS_LANES);  // accumulators of one threshold
  const int nval = WBX_FSS_LANES * h.nthr;                                                      // value lanes of the partial
  const int nacc = skipna ? 2 * nval : (masked ? nval + 1 : nval);                               // lanes_total
  const int kb = h.kb;
  const double area = (double)n * (double)n;

  T thr[KB];
#pragma unroll
  for (int q = 0; q < KB; ++q) thr[q] = cont_threshold<T>(h.thr + h.k0, q, kb);  // (slots past kb: +inf, never exceeded)

  // the lane of the partial that accumulator l of threshold q goes to, or -1: the shared count lane is the first launch's
  auto out_lane = [&](int q, int l) -> int {
    const int v = WBX_FSS_LANES * (h.k0 + q);
    if (l < WBX_FSS_LANES) return v + l;
    if (skipna) return nval + v + (l - WBX_FSS_LANES);
    return (h.k0 == 0 && q == 0) ? nval : -1;
  };

  constexpr int NS = N1 ? 1 : NC * FSS_THREADS;
  __shared__ u64 sS[KB + 1][NS];         // slot q < KB: the counts of threshold q (p low, t high); slot KB: the NaN counts
  __shared__ u64 wS[KB + 1][FSS_WAVES];
  __shared__ double racc[FSS_BMAX][FSS_WAVES][KB][FSS_NACC];  // x summed: slot [row][wave] belongs to lane 0 of that wave

  if (!a.x_kept) {
    for (int i = tid; i < FSS_BMAX * FSS_WAVES * KB * FSS_NACC; i += FSS_THREADS) (&racc[0][0][0][0])[i] = 0.0;
    __syncthreads();
  }

  int64_t kbase[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) kbase[i] = a.key_off[i] ? a.key_off[i][key] : 0;
  const T* pin = reinterpret_cast<const T*>(a.in[0]);
  const T* tin = reinterpret_cast<const T*>(a.in[1]);
  const uint8_t* min_ = reinterpret_cast<const uint8_t*>(a.in[2]);

  for (int64_t d = d0; d < d1; ++d) {
    int64_t base[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) base[i] = kbase[i] + (a.depth_off[i] ? a.depth_off[i][d] : 0);

    // the vertical window counts of the owned columns, p in the low half, t in the high half
    uint32_t cc[NC][KB], hh[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      hh[c] = 0;
#pragma unroll
      for (int q = 0; q < KB; ++q) cc[c][q] = 0;
    }
    T pv[NC], tv[NC];
    auto load_row = [&](int r) {  // 0 <= r < nlat
      const int64_t rp = base[0] + (int64_t)r * a.lat_stride[0], rt = base[1] + (int64_t)r * a.lat_stride[1];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int x = tid + c * FSS_THREADS;
        const int xs = x < nlon ? x : nlon - 1;  // (columns past the circle re-read its last point and are dropped below)
        pv[c] = pin[rp + (int64_t)xs * a.lon_stride[0]];
        tv[c] = tin[rt + (int64_t)xs * a.lon_stride[1]];
      }
    };
    auto slide = [&](int r, bool enters) {  // row r enters or leaves; 0 <= r < nlat
      load_row(r);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const bool in = tid + c * FSS_THREADS < nlon;
        const uint32_t hn = (uint32_t)(in && pv[c] != pv[c]) | ((uint32_t)(in && tv[c] != tv[c]) << 16);
        hh[c] = enters ? hh[c] + hn : hh[c] - hn;
#pragma unroll
        for (int q = 0; q < KB; ++q) {  // (a NaN member exceeds nothing)
          const uint32_t e = (uint32_t)(in && pv[c] > thr[q]) | ((uint32_t)(in && tv[c] > thr[q]) << 16);
          cc[c][q] = enters ? cc[c][q] + e : cc[c][q] - e;
        }
      }
    };
    if constexpr (!N1) {
      if (ys < ye) {
#pragma unroll 1
        for (int r = ys - hw; r < ys + hw; ++r) slide(r, true);  // (rolled: unrolled copies of the halo rows' loads cost registers)
      }
    }

    for (int y = y0; y < y1; ++y) {
      const bool brow = !N1 && (y < hw || y >= nlat - hw);  // block-uniform
      uint32_t nanbits = 0;  // bit c: the window of column c holds a NaN of p; bit 16 + c: of t (N1: the point itself)
      if constexpr (N1) {
        load_row(y);
#pragma unroll
        for (int c = 0; c < NC; ++c) nanbits |= ((uint32_t)(pv[c] != pv[c]) << c) | ((uint32_t)(tv[c] != tv[c]) << (16 + c));
      } else if (!brow) {
        slide(y + hw, true);
        // inclusive prefix over the circle, as in fss_kernel: the column counts go to LDS at their own positions; thread `tid` then
        // takes the RUN [NC tid, NC tid + NC) of the circle (padded with zeros to 256 NC columns) and forms the run's prefix IN
        // PLACE, the block scans the 256 run totals (one wave scan by shuffles, the four wave totals in order through LDS), and
        // the offset is added to the run.  Four barriers per row; this first one closes the previous row (or field).
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int x = tid + c * FSS_THREADS;  // < NC * 256: inside the arrays
#pragma unroll
          for (int q = 0; q < KB; ++q) sS[q][x] = fss_widen(cc[c][q]);
          sS[KB][x] = fss_widen(hh[c]);
        }
        __syncthreads();
        u64 off[KB + 1];
#pragma unroll
        for (int q = 0; q <= KB; ++q) {
          u64 r = 0;
#pragma unroll
          for (int j = 0; j < NC; ++j) {  // (the thread's own run: nobody else touches it before the last barrier below)
            r += sS[q][tid * NC + j];
            sS[q][tid * NC + j] = r;
          }
          // the sum of the runs in front of this one: the wave's inclusive scan shifted by a lane, then the waves in front
          const u64 incl = fss_wave_scan(r, lane);
          if (lane == 63) wS[q][wave] = incl;
          const u64 up = __shfl_up(incl, 1, 64);
          off[q] = lane == 0 ? 0 : up;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q <= KB; ++q) {
          u64 bw = 0;
#pragma unroll
          for (int w = 0; w < FSS_WAVES; ++w) bw += w < wave ? wS[q][w] : 0;
          const u64 o = off[q] + bw;
#pragma unroll
          for (int j = 0; j < NC; ++j) sS[q][tid * NC + j] += o;
        }
        __syncthreads();
        slide(y - hw, false);  // (registers only: the window reads below take the prefix out of LDS)
      }

      uint32_t validbits = ~0u;
      if (masked) {
        const int64_t rm = base[2] + (int64_t)y * a.lat_stride[2];
        validbits = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int x = tid + c * FSS_THREADS;
          validbits |= (uint32_t)(min_[rm + (int64_t)(x < nlon ? x : nlon - 1) * a.lon_stride[2]] != 0) << c;
        }
      }

      // the window of an owned column as (lo, hi] of the extended prefix; false where the point is a border point or past the circle
      auto window = [&](int x, int& lo, int& hi, bool& wlo, bool& whi) -> bool {
        if (!(x < nlon && (a.wrap || (x >= hw && x < nlon - hw)))) return false;
        lo = x - hw - 1;
        hi = x + hw;
        wlo = lo < 0;
        whi = hi >= nlon;
        lo = wlo ? lo + nlon : lo;  // n <= nlon: back inside [0, nlon)
        hi = whi ? hi - nlon : hi;
        return true;
      };
      auto window_sum = [&](int q, int lo, int hi, bool wlo, bool whi) -> u64 {  // (mod 2^64: both halves end in range)
        u64 s = sS[q][hi] - sS[q][lo];
        const u64 tot = sS[q][nlon - 1];
        s += wlo ? tot : 0;
        s += whi ? tot : 0;
        return s;
      };
      if constexpr (!N1) {
        if (!brow) {
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            int lo = 0, hi = 0;
            bool wlo = false, whi = false;
            if (window(tid + c * FSS_THREADS, lo, hi, wlo, whi)) {
              const u64 s = window_sum(KB, lo, hi, wlo, whi);
              nanbits |= ((uint32_t)((uint32_t)s != 0) << c) | ((uint32_t)((uint32_t)(s >> 32) != 0) << (16 + c));
            }
          }
        }
      }

      // the row's lanes of threshold q
      auto row_lanes = [&](int q) {
        {
          double acc[FSS_NACC];
#pragma unroll
          for (int l = 0; l < FSS_NACC; ++l) acc[l] = 0.0;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const int x = tid + c * FSS_THREADS;
            const bool in = x < nlon;
            const float nanf_ = __builtin_nanf("");
            float pf = 0.f, tf = 0.f;
            if constexpr (N1) {
              pf = (nanbits >> c) & 1 ? nanf_ : (pv[c] > thr[q] ? 1.f : 0.f);
              tf = (nanbits >> (16 + c)) & 1 ? nanf_ : (tv[c] > thr[q] ? 1.f : 0.f);
            } else if (!brow) {
              int lo = 0, hi = 0;
              bool wlo = false, whi = false;
              if (window(x, lo, hi, wlo, whi)) {
                const u64 s = window_sum(q, lo, hi, wlo, whi);
                pf = (nanbits >> c) & 1 ? nanf_ : (float)((double)(uint32_t)s / area);
                tf = (nanbits >> (16 + c)) & 1 ? nanf_ : (float)((double)(uint32_t)(s >> 32) / area);
              }
            }
            double v[WBX_FSS_LANES];
            fss_lanes<float>(pf, tf, v);
            const bool valid = (validbits >> c) & 1;
            double one[FSS_NACC];
#pragma unroll
            for (int l = 0; l < FSS_NACC; ++l) one[l] = 0.0;
#pragma unroll
            for (int l = 0; l < WBX_FSS_LANES; ++l) {
              const double val = valid ? v[l] : 0.0;  // a masked-out point contributes exactly 0 whatever it holds
              if (skipna) {
                const bool fin = !(val != val);
                one[l] = fin ? val : 0.0;
                one[WBX_FSS_LANES + l] = (fin && valid) ? 1.0 : 0.0;
              } else {
                one[l] = val;
              }
            }
            if (masked && !skipna) one[WBX_FSS_LANES] = valid ? 1.0 : 0.0;
            if (a.x_kept) {
              if (in) {
                double* o = a.out + (((key * nlat + y) * a.nchunk + chunk) * (int64_t)nacc) * nlon + x;
#pragma unroll
                for (int l = 0; l < FSS_NACC; ++l) {
                  const int ol = l < nacc1 ? out_lane(q, l) : -1;
                  if (ol >= 0) {
                    double* w = o + (int64_t)ol * nlon;
                    *w = d == d0 ? one[l] : *w + one[l];  // the thread owns the element: field after field
                  }
                }
              }
            } else {
#pragma unroll
              for (int l = 0; l < FSS_NACC; ++l) acc[l] += in ? one[l] : 0.0;
            }
          }
          if (!a.x_kept) {
#pragma unroll
            for (int l = 0; l < FSS_NACC; ++l) {
              if (l < nacc1) {  // (block-uniform)
                const double s = wave_sum(acc[l]);
                if (lane == 0) racc[y - y0][wave][q][l] += s;
              }
            }
          }
        }
      };
#pragma unroll
      for (int q = 0; q < KB; ++q)  // (unrolled: the window reads and wave sums of the thresholds are independent and overlap)
        if (q < kb) row_lanes(q);
    }
  }

  if (a.x_kept && d0 >= d1) {  // a chunk without fields (a plan whose chunks overshoot the depth): zeros
    for (int y = y0; y < y1; ++y)
      for (int q = 0; q < kb; ++q)
        for (int l = 0; l < nacc1; ++l) {
          const int ol = out_lane(q, l);
          if (ol < 0) continue;
          for (int x = tid; x < nlon; x += FSS_THREADS)
            a.out[((((key * nlat + y) * a.nchunk + chunk) * (int64_t)nacc) + ol) * nlon + x] = 0.0;
        }
  }
  if (!a.x_kept) {
    __syncthreads();
    const int per = kb * nacc1;
    for (int i = tid; i < (y1 - y0) * per; i += FSS_THREADS) {
      const int j = i / per, r = i - j * per, q = r / nacc1, l = r - q * nacc1;
      const int ol = out_lane(q, l);
      if (ol < 0) continue;
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < FSS_WAVES; ++w) s += racc[j][w][q][l];
      a.out[((key * nlat + (y0 + j)) * a.nchunk + chunk) * (int64_t)nacc + ol] = s;
    }
  }
}

template <typename T, int KB, bool N1>
static int fss_thr_launch(wbx_ctx* ctx, const FssArgs& a, const FssThrArgs& h, int64_t grid) {
  const int nc = (a.nlon + FSS_THREADS - 1) / FSS_THREADS;
  void (*k)(FssArgs, FssThrArgs) = nc <= 1   ? fss_thr_kernel<T, 1, KB, N1>
                                   : nc <= 2 ? fss_thr_kernel<T, 2, KB, N1>
                                   : nc <= 4 ? fss_thr_kernel<T, 4, KB, N1>
                                   : nc <= 6 ? fss_thr_kernel<T, 6, KB, N1>
                                             : fss_thr_kernel<T, 8, KB, N1>;
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(FSS_THREADS), 0, ctx->stream, a, h);
  WBX_HIP(hipGetLastError());
  return 0;
}

template <typename T, bool N1>
static int fss_thr_dispatch(wbx_ctx* ctx, const FssArgs& a, const FssThrArgs& h, int64_t grid) {
  if (h.kb <= 1) return fss_thr_launch<T, 1, N1>(ctx, a, h, grid);
  return fss_thr_launch<T, FSS_KB, N1>(ctx, a, h, grid);
}

}  // namespace wbx

extern "C" int wbx_fss_threshold_partial(wbx_ctx* ctx, const wbx_fss_plan* plan, int dtype, int n, int nthr, const double* thresholds,
                                         const void* p, const void* t, const uint8_t* mask, double* partial_out) {
  using namespace wbx;
  if (const int rc = fss_check("wbx_fss_threshold_partial", ctx, plan, dtype, n, p, t, mask, partial_out)) return rc;
  WBX_REQUIRE(nthr >= 1 && nthr <= WBX_FSS_THR_MAX, "wbx_fss_threshold_partial: 1..%d thresholds per call (got %d)", WBX_FSS_THR_MAX,
              nthr);
  WBX_REQUIRE(thresholds != nullptr, "wbx_fss_threshold_partial: the threshold table is NULL");
  if (plan->nkey == 0) return 0;
  WBX_HIP(hipSetDevice(ctx->device));
  const int64_t nval = (int64_t)WBX_FSS_LANES * nthr;
  const int64_t nacc = (plan->flags & WBX_FLAG_SKIPNA) ? 2 * nval : ((plan->flags & WBX_FLAG_MASKED) ? nval + 1 : nval);
  if (fss_empty(plan)) {
    const size_t cnt = (size_t)plan->nkey * plan->nlat * plan->nchunk * nacc * (size_t)(plan->x_kept ? plan->nlon : 1);
    if (cnt) WBX_HIP(hipMemsetAsync(partial_out, 0, cnt * sizeof(double), ctx->stream));
    return 0;
  }
  FssArgs a = fss_args(plan, n, p, t, mask, partial_out);
  const int B = fss_band_rows(plan, n);
  a.B = B;
  a.nband = (a.nlat + B - 1) / B;
  const int64_t grid = plan->nkey * plan->nchunk * a.nband;
  WBX_REQUIRE(grid < (int64_t)1 << 31, "wbx_fss_threshold_partial: grid too large (%lld blocks)", (long long)grid);
  for (int k0 = 0; k0 < nthr; k0 += FSS_KB) {  // disjoint lane slices of the partial, one launch each
    const FssThrArgs h = {thresholds, k0, nthr - k0 < FSS_KB ? nthr - k0 : FSS_KB, nthr};
    int rc;
    if (n == 1)
      rc = dtype == WBX_F32 ? fss_thr_dispatch<float, true>(ctx, a, h, grid) : fss_thr_dispatch<double, true>(ctx, a, h, grid);
    else
      rc = dtype == WBX_F32 ? fss_thr_dispatch<float, false>(ctx, a, h, grid) : fss_thr_dispatch<double, false>(ctx, a, h, grid);
    if (rc) return rc;
  }
  return 0;
}
