// Zonal spectra of predictions AND targets plus the deterministic lanes of the same (p, t[, c]) rows in ONE sweep.
//
// configs[3] / configs[4] ask for "spectra of p and t + the full deterministic suite in the same sweep" (SURVEY 8d).  As
// separate launches the z fields cross the HBM twice: wbx_det_partial reads p, t, c (12 B/point), the two spectrum launches
// read p and t again (8 B/point).  zspec1440_kernel already transforms TWO rows per wave (every quantity is a (row A, row B)
// pair of packed fp32): here the pair is (p[row], t[row]) instead of two consecutive rows of one field, so
//   * the 48 floats a lane holds of the pair in front of pass 1 are exactly the p and t values of its 24 points: with the
//     climatology row fetched alongside (one more 8-byte load per 2 points) the DET6 lanes e, |e|, e^2, (p-c)^2, (t-c)^2,
//     (p-c)(t-c) are accumulated there in fp64 -- the same arithmetic as DetOp (wbx_det.hip) -- folded over the wave with DPP
//     row operations and written as the row's entry of the stage-1 partial buffer (one key = one row: stage 2 is unchanged);
//   * the spectra of row A go to the predictions' accumulators, those of row B to the targets' (z14_pair<.., PT = true>).
// Algorithmic bytes: 12 B/point (8 without a climatology) for BOTH families.
// Registers: +24 (climatology prefetch) +24 (second set of spectrum sums) +12 (deterministic sums) on a kernel that sat at
// 168: eight one-wave teams per block = two waves per SIMD and up to 256 VGPRs (the spectrum kernel's throughput is flat
// from 8 to 12 teams per CU: 0.311 vs 0.291 ms per field).  What it took to fit (round 3, configs[4] chunk
// = 533 540 rows, `tools/kbench_det_spectrum.py`; the three separate launches: 2.59 ms):
//   * first version: 287 VGPRs needed, 31 spilled -- among them ten of the 24 PREFETCH loads, each stored to scratch behind a
//     full `s_waitcnt vmcnt(0)`: 3.75 ms.  The six deterministic sums are serial fma chains over a lane's 24 points, so the
//     compiler widened all 72 inputs and formed all 48 anomalies up front (~100 fp64 temporaries) to feed the chains;
//     scheduling barriers do not help (the hoisting happens on the IR).  An opaque asm redefinition of a point pair's inputs
//     AND of the running sums makes pair i start when pair i - 1 is done: 214 VGPRs, no scratch, 1.87 ms = 4.95 TB/s = 62 % of
//     the HBM peak on 12 B/point.
//   * the climatology row staged through the LDS instead of 24 registers (24 `global_load_lds_dword` per row into a 6 KB slot
//     per team, read back with ds_read2st64_b32): 192 VGPRs, 1.98 ms -- twice the vector-memory instructions for the same
//     bytes; not kept.
//   * without a climatology (DET3): 190 VGPRs, 1.44-1.51 ms (the two spectra alone: 1.22-1.26 ms).
//   * (r6) where the time went next: the kernel's time follows its vector-ALU time almost one to one at two waves per SIMD
//     (the deterministic lanes over every other point pair: 144 fp64 instructions fewer per row = -10.4 %), and every row
//     began with four dependent VECTOR-load round trips for its three base pointers.  Scalar lookups one row ahead + global instead of flat loads: 1.83 -> 1.68 ms (folded,
//     5.0 -> 5.5 TB/s), 232 VGPRs (profiles/r06_det_spectrum_scalar_lookup_ab.txt).
//
// Rows = the keys of the deterministic plan (wbx_s1_plan with x = longitude summed, nx = 1440, unit x strides, ndepth = 1,
// nchunk = 1), addressed through the plan's own offset / gather tables; `group` / `scale` are per key.
// Included by wbx_spectrum.hip (inside namespace wbx, after wbx_zspec1440.hpp).
#pragma once

// One-wave teams per block = per CU (the block's LDS fills it): two waves per SIMD at 232 VGPRs.  Twelve teams (three waves per
// SIMD, <= 168 VGPRs, every load of the next row at the end of the pair) ran the kernel alone 1-3 % faster but the configs[4]
// chunk loop slower, 2.92 against 2.85 ms per chunk: a 155 KB block owns its CU's LDS and the ensemble kernel of the other
// stream no longer fits beside it (profiles/r06_det_spectrum_3waves_ab.txt).
constexpr int ZD_TEAMS = 8;

// FOLD (r6, wbx_det_spectrum_folded): the rows' deterministic sums are not stored row by row for stage 2 -- each is multiplied by
// its row's weight `dscale[row]` (what stage 2's W holds for the row: the latitude weight) and added to the team's running sums
// PER LANE; the six wave sums and stores happen once per RECORD instead of once per row (6 % of the kernel,
// profiles/r06_det_spectrum_knockouts.txt), and the record carries them behind the two spectra (ZD_TAIL values: spec_close_kernel
// adds them over the records of a group in key order like every wavenumber).
constexpr int ZD_TAIL = 8;  // doubles behind the 2 x 721 spectrum values of a folded record (6 used)
template <bool HAS_C, bool FOLD = false>
__global__ void __launch_bounds__(64 * ZD_TEAMS) zspec1440_det_kernel(S1Args a, int64_t nrows, int rows_per_team,
                                                                      const float2* __restrict__ tables_g,
                                                                      const int32_t* __restrict__ group,
                                                                      const double* __restrict__ scale, SpecRecs recs,
                                                                      const double* __restrict__ dscale = nullptr) {
  constexpr int NA = HAS_C ? 6 : 3;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  float2* const tw1 = reinterpret_cast<float2*>(lds_raw);
  float2* const tw2 = tw1 + Z14_TW1;
  float2* const twr = tw2 + Z14_TW2;
  const int lane = (int)(threadIdx.x & 63);
  const int team = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nteam = (int)(blockDim.x >> 6);
  v4* const buf = reinterpret_cast<v4*>(twr + Z14_TWR) + team * Z14_BUF;
  for (int i = threadIdx.x; i < Z14_TABLES; i += blockDim.x) tw1[i] = tables_g[i];
  __syncthreads();
  const int64_t r0 = ((int64_t)blockIdx.x * nteam + team) * rows_per_team;
  const int64_t r1 = r0 + rows_per_team < nrows ? r0 + rows_per_team : nrows;
  const int64_t team_id = (int64_t)blockIdx.x * nteam + team;
  if (r0 >= r1) {  // only wave-level ordering below
    spec_rec_static(recs, (unsigned int)team_id, -1, 0ull, lane == 0);  // (the team's reserved slot stays empty)
    return;
  }
  constexpr int nk = Z14_N2 + 1;
  const Z14Lane c = z14_lane(lane, buf, tw2);
  const int L = c.L;
  const double quarter_inv_nn = 0.25 / ((double)Z14_N * (double)Z14_N);  // E and O are used without their factor 1/2

  double accp[6], accmp[6], acct[6], accmt[6];  // sums of k = L + 60 s and of 720 - k, predictions / targets
#pragma unroll
  for (int s = 0; s < 6; ++s) accp[s] = accmp[s] = acct[s] = accmt[s] = 0.0;
  double dsum[FOLD ? NA : 1];  // FOLD: this lane's weighted deterministic sums over the rows of the current record
#pragma unroll
  for (int l = 0; l < (FOLD ? NA : 1); ++l) dsum[l] = 0.0;
  int32_t cur = group[r0];
  unsigned int seq = 0;
  // (r5) one record of 2 x 721 values: the predictions' sums, then the targets'; the team's LAST record sits in its reserved slot
  auto flush = [&](int32_t next, bool last = false) {
    double* const rec = last ? spec_rec_static(recs, (unsigned int)team_id, cur, spec_key(team_id, 0xffffffu), lane == 0)
                             : spec_rec_open(recs, cur, spec_key(team_id, seq++), lane);
    z14_send<true>(rec, c, accp, accmp);
    z14_send<true>(rec + nk, c, acct, accmt);
#pragma unroll
    for (int s = 0; s < 6; ++s) accp[s] = accmp[s] = acct[s] = accmt[s] = 0.0;
    if constexpr (FOLD) {
#pragma unroll
      for (int l = 0; l < NA; ++l) {
        const double tot = wave_sum_uniform(lane < Z14_LANES ? dsum[l] : 0.0);  // (lanes 60..63 shadow lane 59)
        if (lane == 0) rec[2 * nk + l] = tot;
        dsum[l] = 0.0;
      }
      if (lane < ZD_TAIL - NA) rec[2 * nk + NA + lane] = 0.0;
    }
    cur = next;
  };

  v2 pa[12], pb[12], pc[12];  // the row's p, t and c values of this lane's 12 packed points, fetched one row ahead
  // A row's three base pointers come out of the plan's offset / gather tables, one row ahead.
  // (r6) Through the CONSTANT address space: scalar loads with SGPR results.  Up to round 6 `resolve` went through the generic
  // helpers (key_bases / row_bases): behind the asm statements' memory clobbers those are VECTOR loads, and the compiler had
  // laid them out as four dependent round trips at the top of every row -- six table entries, `s_waitcnt vmcnt(0)`, gk[row],
  // wait, gd[0], wait, gtab[..], wait -- each an L2 latency that the one other wave of the SIMD cannot cover.  Now: the
  // entries that do not depend on the row (depth_off[i][0], gd[0]) are read once; `lookup` issues the row's four scalar loads
  // at the TOP of the previous row and `pointers` consumes them behind its deterministic lanes (~300 instructions later), where
  // it issues the one dependent load (the climatology's gather table, a few hundred hot bytes), consumed behind pass 1.
  // NULL tables are stood in for by a one-element table of zeros (index mask 0): no control flow around a load.
  constexpr int NIN = HAS_C ? 3 : 2;
  const const_ptr<int64_t> zero64 = (const_ptr<int64_t>)wbx_zero_i64;
  const_ptr<int64_t> tk[NIN];
  int64_t mk[NIN], dep[NIN];
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    tk[i] = a.key_off[i] ? (const_ptr<int64_t>)a.key_off[i] : zero64;
    mk[i] = a.key_off[i] ? -1 : 0;
    dep[i] = a.depth_off[i] ? ((const_ptr<int64_t>)a.depth_off[i])[0] : 0;
  }
  const bool has_g = HAS_C && a.gtab != nullptr;
  const const_ptr<int32_t> tgk = (has_g && a.gk) ? (const_ptr<int32_t>)a.gk : (const_ptr<int32_t>)wbx_zero_i64;
  const int64_t mgk = (has_g && a.gk) ? -1 : 0;
  const const_ptr<int64_t> tg = has_g ? (const_ptr<int64_t>)a.gtab : zero64;
  const int64_t mg = has_g ? -1 : 0;
  const int64_t gd0 = (has_g && a.gd) ? (int64_t)((const_ptr<int32_t>)a.gd)[0] : 0;
  int64_t kbn[NIN];    // the looked-up row's key offsets, as loaded
  int32_t gkn = 0;     // ... its row of the gather table
  int64_t gvn = 0;     // ... its gather-table entry (elements), as loaded: added where the climatology row is fetched
  const const_ptr<int32_t> tgroup = (const_ptr<int32_t>)group;
  const const_ptr<double> tscale = (const_ptr<double>)scale;
  const const_ptr<double> tdscale = FOLD ? (const_ptr<double>)dscale : (const_ptr<double>)wbx_one_f64;
  auto lookup = [&](int64_t r) {
#pragma unroll
    for (int i = 0; i < NIN; ++i) kbn[i] = tk[i][r & mk[i]];
    if constexpr (HAS_C) gkn = tgk[r & mgk];
  };
  auto pointers = [&](const char*& up, const char*& ut, const char*& uc) {
    up = reinterpret_cast<const char*>(reinterpret_cast<const float*>(a.in[0]) + (kbn[0] + dep[0]));
    ut = reinterpret_cast<const char*>(reinterpret_cast<const float*>(a.in[1]) + (kbn[1] + dep[1]));
    if constexpr (HAS_C) {
      uc = reinterpret_cast<const char*>(reinterpret_cast<const float*>(a.in[2]) + (kbn[2] + dep[2]));
      gvn = tg[((int64_t)gkn * a.ngd + gd0) & mg];
    } else {
      uc = nullptr;
    }
  };
  // The next row's loads are spread over the transform so that they never sit on top of its register peak (pass 2 holds 60
  // registers of butterflies): p and the climatology behind pass 1's stores, t behind pass 2's.
  // (r6) The row pointers went through integers (uniform_ptr) and lost their address space: as generic pointers the 36 loads
  // of a row came out as flat_load -- issued to the LDS pipeline as well and counted on lgkmcnt, the counter every exchange of
  // the transform waits on.  `gv2` says "global" again.
  using gv2 = const __attribute__((address_space(1))) v2*;
  auto fetch_p = [&](const char* up, const char* uc) {
    // (the twelve loads of a row address it from its MIDDLE: offsets -2880 .. +2400 bytes all fit the instruction's 13-bit
    // immediate, so a row is one SGPR base + one 32-bit lane offset; from its start the last three needed a 64-bit base of their own)
    gv2 rowp = (gv2)(reinterpret_cast<const v2*>(up + 2880) + L);
#pragma unroll
    for (int i = 0; i < 12; ++i) pa[i] = __builtin_nontemporal_load(rowp + 60 * (i - 6));
    if constexpr (HAS_C) {
      gv2 rowc = (gv2)(reinterpret_cast<const v2*>(reinterpret_cast<const char*>(reinterpret_cast<const float*>(uc) + gvn) + 2880) + L);
#pragma unroll
      for (int i = 0; i < 12; ++i) pc[i] = __builtin_nontemporal_load(rowc + 60 * (i - 6));
    }
  };
  auto fetch_t = [&](const char* ut) {
    gv2 rowt = (gv2)(reinterpret_cast<const v2*>(ut + 2880) + L);
#pragma unroll
    for (int i = 0; i < 12; ++i) pb[i] = __builtin_nontemporal_load(rowt + 60 * (i - 6));
  };
  const char *np = nullptr, *nt = nullptr, *nc = nullptr;
  lookup(r0);
  pointers(np, nt, nc);
  fetch_p(np, nc);
  fetch_t(nt);
  int turn = team >> 2;  // waves t and t + 4 of a block share a SIMD: the user priority alternates row by row (see zspec1440_kernel)
  for (int64_t r = r0; r < r1; ++r) {
    turn ^= 1;
    if (turn == 0) __builtin_amdgcn_s_setprio(0);
    else __builtin_amdgcn_s_setprio(1);
    // (the row's own scalars; loading them a row ahead with the lookups measured the same -- 1.808 against 1.809-1.817 ms -- at
    // 250 instead of 232 registers and with three prefetched registers copied behind an `s_waitcnt vmcnt(0)` at the row's end)
    const int32_t g = tgroup[r];
    const double sc = tscale[r] * quarter_inv_nn;
    const double dw = FOLD ? tdscale[r] : 1.0;
    lookup(r + 1 < r1 ? r + 1 : r);  // (unconditional: the last row looks itself up again)
    // ---- the deterministic lanes of this row, on the raw values (lanes 60..63 shadow lane 59: counted out)
    __builtin_amdgcn_sched_barrier(0);
    double d[NA];
#pragma unroll
    for (int l = 0; l < NA; ++l) d[l] = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      // The six sums are serial fma chains over the lane's 24 points, so the compiler widens all 72 inputs and forms all 48
      // anomalies up front to have independent work for the chains' latency: ~100 fp64 temporaries (v160..v253 in the ISA), 287
      // VGPRs, the prefetch loads spilled behind vmcnt(0) waits.  An opaque redefinition of the point pair's inputs AND of the
      // running sums right where they are used makes point pair i start when pair i - 1 is done; the other wave of the SIMD
      // covers the chains' latency (an ordering point every second pair instead: 1.93 ms either way).
      if constexpr (HAS_C)
        asm volatile("" : "+v"(pa[i]), "+v"(pb[i]), "+v"(pc[i]), "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]), "+v"(d[5]));
      else
        asm volatile("" : "+v"(pa[i]), "+v"(pb[i]), "+v"(d[0]), "+v"(d[1]), "+v"(d[2]));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const double p = (double)(h ? pa[i].y : pa[i].x), t = (double)(h ? pb[i].y : pb[i].x);
        const double e = p - t;
        d[0] += e;
        d[1] += fabs(e);
        d[2] = fma(e, e, d[2]);
        if constexpr (HAS_C) {
          const double cv = (double)(h ? pc[i].y : pc[i].x);
          const double ap = p - cv, at = t - cv;
          d[3] = fma(ap, ap, d[3]);
          d[4] = fma(at, at, d[4]);
          d[5] = fma(ap, at, d[5]);
        }
      }
    }
    if constexpr (FOLD) {
      if (g != cur) flush(g);  // (the row belongs to the next record: close the running one first; wave-uniform)
#pragma unroll
      for (int l = 0; l < NA; ++l) dsum[l] = fma(d[l], dw, dsum[l]);
    } else {
#pragma unroll
      for (int l = 0; l < NA; ++l) {
        const double tot = wave_sum_uniform(lane < Z14_LANES ? d[l] : 0.0);
        if (lane == 0) a.out[r * NA + l] = tot;
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // the row's deterministic sums are done before the transform starts: their temporaries die here
    pointers(np, nt, nc);  // the next row's: `lookup`'s loads have had the lanes above to land
    __builtin_amdgcn_sched_barrier(0);  // (or the gather table's load sinks to its use behind pass 1 and is waited for on the spot)
    C2 v[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = {{pa[i].x, pb[i].x}, {pa[i].y, pb[i].y}};
    // (r6, measured and dropped: forming x - m with 48 opaque scalar subtractions that ARE this interleave instead of 48 moves + 24
    // packed subtractions -- bit-identical, 9 instructions fewer per row: 1.7226-1.7260 against 1.7260-1.7289 ms here, and the
    // three-wave spectrum kernel, at its 168 registers, reloads one more spilled value inside its loop: 0.355-0.357 -> 0.361 ms)
    const v2 msh = z14_demean(v);  // (the deterministic lanes above took the raw values)
    if (g != cur) flush(g);  // wave-uniform
    z14_pair<0, true, true>(v, buf, c, tw1, twr, sc, sc, false, g, accp, accmp, nullptr, [&](int i) {
      // (r6) Unconditional: behind a team's last row the row is asked for once more (`lookup` clamps; 1 row in ~260, found in the
      // L2 / Infinity Cache).  Under `r + 1 < r1` the loads sat in a block of their own: the compiler sank the gather-table
      // load into it (issued and waited for on the spot) and, at 254 registers, joined the two paths with copies of three
      // prefetched registers behind an `s_waitcnt vmcnt(0)` at the END of every row.
      if (i == 0) fetch_p(np, nc);
      if (i == 2) fetch_t(nt);
    }, acct, accmt, msh);
  }
  flush(cur, true);
}

// Measured and not kept (r4): the row's work split between two kinds of waves -- a block of eight transform teams that never
// touch global memory plus four loader waves (three waves per SIMD, 160 VGPRs) that stream p, t, c into registers, form the
// deterministic sums and hand the (p, t) pairs to the teams through their LDS buffers (one flag word per team, s_sleep polling,
// the next row of both its teams ready in a loader's registers).  Correct, and SLOWER on the same box: 1.07-1.08 ms per
// configs[3] chunk against 0.91-0.93 ms for one wave per row (configs[4]: 3.23 against 2.86 ms per chunk) -- the teams pay
// twelve more 16-byte LDS writes and reads per row and the hand-over, and the loaders' fp64 chains take vector-ALU slots from
// the transforms instead of filling idle ones.
