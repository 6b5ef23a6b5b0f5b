// LSTM recurrence, multi-CU form: the hidden units of one direction are split over a CLUSTER of
// G = H/64 workgroups (one per CU), so that each CU's slice of W_h is resident in its LDS for the
// whole launch and nothing is re-streamed from L2 per step.
//
// Why (measured): the single-CU kernels of lstm.hip spend 4.2-6.6k of their
// 10.6k cycles/step pulling the 384-448 KB of W_h that does not fit on chip through the one CU's
// L2 port (58 B/clk).  With G CUs the slice is H x 4*64 bf16 = 128 KB (H = 256) -> LDS.
// The price is one all-gather of h (forward) / one reduce-scatter of dh (backward) per step
// between the G CUs.  It is done with the placement-independent hand-off of
// cdna_hip_programming.md G16 "R2": the data IS the flag -- 8-byte {tag = step+1, payload}
// granules written with ONE relaxed agent-scope atomic store and polled with relaxed agent-scope
// atomic loads; no fence, no separate flag, correct for any workgroup->XCD placement.
// Slots are double-buffered by step parity (a producer can only reach step s+1 after every
// consumer has consumed step s-1, see the comment at the poll).  Every spin is bounded: on
// timeout the workgroup raises the error word and keeps going (garbage, but no hang).
//
// Same semantics / data layouts as lstm.hip (gates interleaved [T,B,dir,H,4], etc.).
//
// This unit: the bf16 kernels (fp32 operands: lstm_cluster_f32.hip, GRU: gru_cluster.hip).  What all three share is
// cluster_xch.h on the device and cluster_launch.h on the host, every switch and counter defined once in cluster_host.hip.
#include "cluster_launch.h"
#include <stdlib.h>
#include <type_traits>

namespace {
__device__ unsigned long long* g_cdbg = nullptr;   // debug phase timers (env ASR_LSTM_DBG=1)
// ---------------------------------------------------------------- forward, 8 waves
// Same cluster / exchange as above with TWO waves per SIMD: the 4-wave form spends ~2.2k of its
// 5.2k cycles/step in the gate math of 4 (row, unit) pairs per lane with nothing to hide the
// v_exp/v_rcp latency chains behind.  Here a wave owns 8 units: tile 0 = columns [i x 8 | ci x 8],
// tile 1 = [f x 8 | o x 8]; after the MFMAs lanes n and n^8 swap halves over DPP row_ror:8 so each
// lane ends up with all four gates of TWO (row, unit) pairs; the second wave of the SIMD fills
// the other's stalls.  LDS A-fragment reads double (8 waves x 8 KB) but hide behind the MFMAs.
// The kernel is instruction-issue bound (a wave issues ~1 instruction per 4 cycles; measured
// 435 instructions/step -> 3.5k cycles), so the step body is written for instruction count:
// exchange-buffer parity is a compile-time constant (loop unrolled by two), every address is an
// incrementally advanced register, the phase timers (DBG) are a template parameter, nothing in
// the loop is exec-masked.
// Served widths (asr_cluster_fwd_try): HSU = 64 at H = 256, 320, 512 (H = 320 has no other form), HSU = 32 at H = 256, 512.
// EARLY (default at H = 256, H = 320 and wherever HSU = 32, i.e. everywhere but H = 512 on 64 units per CU;
// ASR_LSTM_DFLAGS bit 5 inverts the default): the k-chunks of this CU's OWN slice of h -- which
// never leave the CU -- are multiplied for step s+1 right after they are written, i.e. before the wave starts polling
// for the peers' slices, so that part of the LDS-read + MFMA phase runs under the L2 hop.  The chunk order in the
// registers is rotated by the CU index so that the own chunks are always register chunks 0 .. KO-1.
// HSU = hidden units per CU (64: eight waves per CU, two per SIMD; 32: four waves per CU, ONE per SIMD -- twice the CUs
// per cluster, each wave alone on its SIMD's VALU / MFMA pipes and with half the LDS fragment traffic per CU).
// XW: the all-gather uses 4-byte self-tagged words (see xw_tag) -- a lane polls with 16-byte loads, each holding one row of
// the 8 units of a peer's wave (ceil((G-1)/4) loads per round instead of G-1 8-byte ones, half the bytes) and stages it
// with one ds_write_b128.  XW = false: 8-byte {step, payload} granules (ASR_LSTM_XW=0 / ASR_LSTM_DFLAGS bit 10).
// ABL (builds with -DASR_LSTM_ABLATE only, scripts/probe_lstm_ablate.py): bit k set = piece k of the step is left out (the
// results are garbage; the launch time against ABL = 0 is what that piece costs ON the serial chain).  0: the poll loop does
// not wait for valid tags, 1: no A-fragment reads from LDS, 2: no MFMAs, 3: no gate math, 4: no saved-activation stores,
// 5: no barriers, 6: no x-projection fetch, 7: no publish, 8: no LDS staging of the polled slices, 9: no poll loads at all.
template <int H, bool DBG, bool EARLY = false, int HSU = 64, int FPIN = 0, bool XW = true, int ABL = 0>
__global__ __launch_bounds__(HSU * 8, 1) void lstm_fwd_cluster8_kernel(
    int T_, int B_, int ndir, const f32x4_t* __restrict__ xg, const bf16_t* __restrict__ whp,
    const float* __restrict__ peep, const int32_t* __restrict__ seq_len, float forget_bias,
    float cell_clip, cbf16x4_t* __restrict__ gates, bf16_t* __restrict__ hout, float* __restrict__ cs,
    float* __restrict__ c_final, float* __restrict__ h_final, u64* __restrict__ xch,
    unsigned* __restrict__ err, int kflags, u64* __restrict__ znext, unsigned zwords, int tile0, int ntl) {
  zero_next_area(znext, zwords);
  constexpr int G = H / HSU;
  constexpr int CTW = HSU * 8;                             // threads per workgroup: a wave owns 8 units
  constexpr int KS = H / 32;
  constexpr int LDH = H + 8;
  constexpr int SLICE = 16 * (HSU / 2);                     // granules one CU publishes per step
  constexpr int KO = HSU / 32;                              // k-chunks of one CU's own slice
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* hs = reinterpret_cast<bf16_t*>(smem);            // [2][16][LDH]

  // 1-D grid laid out so that the G workgroups of a cluster get block ids congruent mod 8: the
  // dispatcher is observed to put block b on XCD b % 8, so a cluster shares ONE L2 (speed only:
  // the placement is verified below and the exchange falls back to write-through stores)
  // EARLY: k-chunk index modulo KS (a mask where KS is a power of two; H = 320 has 10 chunks: x < 2 KS there)
  auto krot = [](int x) -> int { return ((KS & (KS - 1)) == 0) ? (x & (KS - 1)) : (x >= KS ? x - KS : x); };
  const ClusterId cid = cluster_id<G>(ndir, tile0, ntl);
  if (!cid.valid) return;
  const int g = cid.g, d = cid.d, b0 = cid.tile * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, rg = lane >> 4;
  const bool lo = col < 8, odd = (col & 1) != 0;
  const bool rev = (d == 1);
  const bf16_t* wp = whp + (size_t)d * H * 4 * H;
  const int ul = wave * 8 + (col & 7);                     // unit inside this CU's slice
  const unsigned jw = g * HSU + ul;                         // global unit of this lane
  const int rbase = rg * 4 + (lo ? 0 : 2);                 // first of this lane's two batch rows

  int len[2];
  int tmax = 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) len[r] = seq_len[b0 + rbase + r];
  for (int i = 0; i < 16; ++i) tmax = max(tmax, seq_len[b0 + i]);
  tmax = min(tmax, T_);

  float c[2] = {0.f, 0.f}, hr[2] = {0.f, 0.f};
  const float wci = peep ? peep[(d * 3 + 0) * H + jw] : 0.f;
  const float wcf = peep ? peep[(d * 3 + 1) * H + jw] : 0.f;
  const float wco = peep ? peep[(d * 3 + 2) * H + jw] : 0.f;

  for (int i = threadIdx.x; i < 2 * 16 * LDH; i += CTW) hs[i] = 0;
  // B fragments straight out of the standard forward packing (tile = (unit/16)*4 + gate, column
  // unit%16): this lane's column of tile p is (gate p*2 + (col>>3), unit jw)
  bf16x8_t wreg[2][KS];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int tile = (jw >> 4) * 4 + p * 2 + (col >> 3);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if constexpr (EARLY) {
        const int kk = krot(ks + g * KO);                  // register chunk ks holds k-chunk kk
        wreg[p][ks] = *reinterpret_cast<const bf16x8_t*>(wp + (((size_t)tile * KS + kk) * 64 + rg * 16 + (jw & 15)) * 8);
      } else {
        wreg[p][ks] = *reinterpret_cast<const bf16x8_t*>(wp + (((size_t)tile * KS + ks) * 64 + rg * 16 + (jw & 15)) * 8);
      }
    }
  }

  u64* xhdr = xch + (size_t)cid.c * (XHDR + 2 * G * SLICE);
  u64* xbase = xhdr + XHDR;                                // [2 parity][G][8 waves][16 rows][4]
  bool timed_out = false;
  const bool colocated = same_xcd<G>(xhdr, g, timed_out);
  const bool fast = colocated && !(kflags & 1);            // same decision on every member
  // after the first timeout the limit drops to 0: the launch drains quickly instead of spinning T times
  unsigned spin_limit = (kflags & 2) ? 2000u : SPIN_LIMIT;
  if ((kflags & 2) && g == G - 1) return;                  // TEST ONLY (ASR_LSTM_DFLAGS bit 6): a member goes missing
  __syncthreads();

  // element offsets into the [T,B,ndir,H] arrays: os = frame s (padded rows write their zeros
  // there), oa = frame of the running step of an active row (s or len-1-s); both just advance
  const unsigned stride = (unsigned)B_ * ndir * H;
  const unsigned dstep = rev ? 0u - stride : stride;
  unsigned oa[2], os[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    os[r] = ((unsigned)(b0 + rbase + r) * ndir + d) * H + jw;
    oa[r] = os[r] + (rev ? (unsigned)max(len[r] - 1, 0) * stride : 0u);
  }
  // per-lane exchange addresses (both parities): publish slot, the three foreign slices this
  // wave polls (wave w polls the granules wave w of the peers publishes), LDS staging targets
  // Rows past their length: their saved activations are never read and their x-projection rows are not used, so both go
  // to ONE parked position per row -- the row's own frame tmax - 1, padding for any row that is ever inactive -- that
  // stays in the L2 instead of streaming the padded part of the batch through HBM (round 4: the "1.87x the algorithmic
  // bytes" of profiles/r03_pmc_hbm.md was exactly this: the batch is 49 % padding).  Only hout keeps its own frames:
  // the next layer reads zeros there.
  unsigned opark[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) opark[r] = os[r] + (unsigned)max(tmax - 1, 0) * stride;
  const int prow = rbase + (odd ? 1 : 0);
  const unsigned pofs = (unsigned)(wave * 64 + prow * 4 + ((col & 7) >> 1));   // publish slot in the slice
  const unsigned lofs = threadIdx.x;                                           // polled granule in a slice
  unsigned ldst[G - 1];                                    // byte offset inside one h buffer
  auto slice = [&](int P, int gg) -> u64* { return xbase + ((size_t)P * G + gg) * SLICE; };   // uniform
#pragma unroll
  for (int k = 0; k < G - 1; ++k) {
    const int gsrc = k + (k >= g ? 1 : 0);
    ldst[k] = ((unsigned)(((lane >> 2) & 15) * LDH + gsrc * HSU + (wave * 4 + (lane & 3)) * 2) * 2u) ^
              lds_swz((lane >> 2) & 15);
  }
  // XW: load j of a lane covers peer k = 4 j + lane / 16 (clamped: the spare lanes of the last load repeat its last peer --
  // same bytes, same LDS target, nothing exec-masked), row lane % 16 of that peer's wave `wave`: 16 bytes = 8 units
  constexpr int NL = XW ? ((G - 1) * 16 + 63) / 64 : 1;
  unsigned* xw = reinterpret_cast<unsigned*>(xbase);       // [2 parity][G][SLICE] words
  const __amdgpu_buffer_rsrc_t xwrs = __builtin_amdgcn_make_buffer_rsrc(xw, 0, 0x7fffffff, 0x00020000);
  unsigned xvoff[NL], xldst[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int k = min(j * 4 + (lane >> 4), G - 2);
    const int gsrc = k + (k >= g ? 1 : 0);
    xvoff[j] = (unsigned)(gsrc * SLICE + wave * 64 + (lane & 15) * 4) * 4u;
    xldst[j] = ((unsigned)((lane & 15) * LDH + gsrc * HSU + wave * 8) * 2u) ^ lds_swz(lane & 15);
  }
  const unsigned lown = ((unsigned)(prow * LDH + g * HSU + (ul & ~1)) * 2u) ^ lds_swz(prow);
  const unsigned lrd = ((unsigned)(col * LDH + rg * 8) * 2u) ^ lds_swz(col);

  // xproj rows of the running step, requested TWO steps ahead (slot = step parity): one step (~1.2 us) covers the
  // idle HBM latency but not always the latency beside the side streams' traffic (measured: 945 -> 931 us per launch)
  // (H = 512 keeps the one-step queue: the second slot costs 8 VGPRs the 8-CU form does not have -- 4 -> 12 spills)
  constexpr int XD = (H <= 320 || HSU == 32) ? 2 : 1;      // (one wave per SIMD may use the whole 512-register file)
  f32x4_t xq[XD][2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    xq[0][r] = xg[(0 < len[r]) ? oa[r] : opark[r]];
    if constexpr (XD == 2) xq[1][r] = (tmax > 1) ? xg[(1 < len[r]) ? oa[r] + dstep : opark[r]] : xq[0][r];
  }
  f32x4_t accn0 = {0.f, 0.f, 0.f, 0.f}, accn1 = {0.f, 0.f, 0.f, 0.f};   // EARLY: own-slice part of the next step

  unsigned long long* dbg = g_cdbg;
  unsigned long long ph[4] = {0, 0, 0, 0};
  unsigned long long ph4 = 0;
  unsigned nspin = 0;
  unsigned nonfin = 0;                                     // XW: OR of every published pair (one v_or per step)
#define C8_T() (DBG ? (__builtin_amdgcn_sched_barrier(0), __builtin_amdgcn_s_memtime()) : 0ull)
#define C8_FPIN(k) do { if constexpr (!DBG && ((FPIN >> (k)) & 1)) __builtin_amdgcn_sched_barrier(0); } while (0)

  auto step = [&](int s, auto PAR) {
    constexpr int P = decltype(PAR)::value;                // parity of step s
    C8_FPIN(0);
    const unsigned long long t0 = C8_T();
    const char* hcur = smem + P * 16 * LDH * 2;
    char* hnxt = smem + (1 - P) * 16 * LDH * 2;
    const f32x4_t x0 = xq[P % XD][0], x1 = xq[P % XD][1];
    // (requested here, at the top of the step: behind the poll loop at its end -- where the BPTT kernel's fetch belongs,
    // see there -- the forward kernel measured 1.21 ms per launch instead of 0.92)
    if (s + XD < tmax && !(ABL & 64)) {                    // lands during the next step(s)
#pragma unroll
      for (int r = 0; r < 2; ++r)
        xq[P % XD][r] = xg[(s + XD < len[r]) ? oa[r] + (unsigned)XD * dstep : opark[r]];
    }
    f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EARLY) { acc0 = accn0; acc1 = accn1; }    // own-slice chunks: done at the end of the last step
    // 8 A fragments in flight at once (left alone the scheduler recycles ONE register and exposes
    // the LDS latency KS times: 870 cycles for 16 MFMAs); H = 512 takes two such batches
#pragma unroll
    for (int kb = 0; kb < KS; kb += 8) {
      bf16x8_t afr[8];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        if (kb + ks >= KS) continue;                       // H = 320: 10 chunks = 8 + 2
        if constexpr ((ABL & 2) != 0) {
          afr[ks] = wreg[1][kb + ks];
        } else if constexpr (EARLY) {
          if (kb + ks >= KO) afr[ks] = *reinterpret_cast<const bf16x8_t*>(hcur + lrd + krot(kb + ks + g * KO) * 64);
        } else {
          afr[ks] = *reinterpret_cast<const bf16x8_t*>(hcur + lrd + (kb + ks) * 64);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (DBG && kb == 0) {                                // sub-phase: first A fragments landed
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(afr[ks]));
        ph4 += C8_T() - t0;
      }
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        if (EARLY && kb + ks < KO) continue;
        if (kb + ks >= KS) continue;
        if constexpr ((ABL & 4) != 0) {                     // keeps the dependence on every fragment, nothing else
          const xw4_t fb = __builtin_bit_cast(xw4_t, afr[ks]);
          acc0[0] = __uint_as_float(__float_as_uint(acc0[0]) ^ (fb[0] & 1u));
          acc1[0] = __uint_as_float(__float_as_uint(acc1[0]) ^ (fb[3] & 1u));
          continue;
        }
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[ks], wreg[0][kb + ks], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[ks], wreg[1][kb + ks], acc1, 0, 0, 0);
      }
    }
    if (DBG) { asm volatile("" : "+v"(acc0)); asm volatile("" : "+v"(acc1)); }
    C8_FPIN(1);
    const unsigned long long t1 = C8_T();
    // lanes n / n^8 swap halves: lo lanes (banks 0,1) keep rows 0,1 (own i,f + the partner's ci,o),
    // hi lanes (banks 2,3) rows 2,3 (own ci,o + the partner's i,f)
    float pi[2], pq[2], pf[2], po[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      pi[r] = dpp_ror8_into<0xC>(acc0[r], acc0[2 + r]);    // hi lanes <- partner's i of rows 2,3
      pq[r] = dpp_ror8_into<0x3>(acc0[2 + r], acc0[r]);    // lo lanes <- partner's ci of rows 0,1
      pf[r] = dpp_ror8_into<0xC>(acc1[r], acc1[2 + r]);
      po[r] = dpp_ror8_into<0x3>(acc1[2 + r], acc1[r]);
    }
    C8_FPIN(4);                                            // behind the DPP half swap
    const unsigned epoch = (unsigned)s + 1u;
    bool act[2];
    float ig[2], gg[2], fg[2], og[2], cn[2], hn[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) act[r] = s < len[r];
    const f32x4_t xr[2] = {x0, x1};
    if constexpr ((ABL & 8) != 0) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        ig[r] = pi[r] + xr[r][0]; gg[r] = pq[r] + xr[r][1]; fg[r] = pf[r] + xr[r][2]; og[r] = po[r] + xr[r][3];
        cn[r] = c[r];
        hn[r] = fminf(fmaxf((ig[r] + gg[r]) + (fg[r] + og[r]), -1.f), 1.f);
      }
    } else {
#pragma unroll
    for (int r = 0; r < 2; ++r) ig[r] = cfsig(pi[r] + xr[r][0] + wci * c[r]);
#pragma unroll
    for (int r = 0; r < 2; ++r) gg[r] = cftanh(pq[r] + xr[r][1]);
#pragma unroll
    for (int r = 0; r < 2; ++r) fg[r] = cfsig(pf[r] + xr[r][2] + forget_bias + wcf * c[r]);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      cn[r] = gg[r] * ig[r] + c[r] * fg[r];
      if (cell_clip > 0.f) cn[r] = fminf(fmaxf(cn[r], -cell_clip), cell_clip);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) og[r] = cfsig(po[r] + xr[r][3] + wco * cn[r]);
#pragma unroll
    for (int r = 0; r < 2; ++r) hn[r] = cftanh(cn[r]) * og[r];
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      c[r] = act[r] ? cn[r] : c[r];
      hr[r] = act[r] ? hn[r] : hr[r];
    }
    C8_FPIN(5);                                            // behind the gate math
    // publish: even lanes the (unit, unit+1) granule of row 0, odd lanes (unit-1, unit) of row 1
    const float nb = dpp_xor1(odd ? hr[0] : hr[1]);
    const unsigned pk = odd ? pack_bf16x2(nb, hr[1]) : pack_bf16x2(hr[0], nb);
    const unsigned etag = xw_tag(s);
    if constexpr ((ABL & 128) != 0) {
    } else if constexpr (XW) {
      unsigned* pw = uoff(xw + (size_t)(P * G + g) * SLICE, pofs);
      nonfin |= pk;                                        // bit 14 / 30 of a FINITE |h| <= 1 is clear (see the tail)
      const unsigned tv = (pk & ~XW_MASK) | etag;
      if (fast) __hip_atomic_store(pw, tv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // plain store, stays in the L2
      else __hip_atomic_store(pw, tv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      gpublish(uoff(slice(P, g), pofs), epoch, pk, fast);
    }
    C8_FPIN(6);                                            // behind the publish
    *reinterpret_cast<unsigned*>(hnxt + lown) = pk;
    // saved activations; rows past their length write frame s of the padding (hout: zeros,
    // gates / cs: never read there), so nothing is predicated
    unsigned off[2], offg[2];                              // hout position / saved-activation position
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      off[r] = act[r] ? oa[r] : os[r];
      offg[r] = act[r] ? oa[r] : opark[r];
    }
    // H = 256: the saved activations are stored BEHIND the poll loop, see there.  H = 512 stores them here: keeping the
    // values alive across the loop costs registers that form has not got (4 -> 12 spills, 43.3 -> 47.7 ms at cfg D).
    constexpr bool LATE_STORE = (H <= 320 || HSU == 32);
    unsigned offs[2] = {off[0], off[1]}, offgs[2] = {offg[0], offg[1]};
    if constexpr (!LATE_STORE) {
      const bool pact = odd ? act[1] : act[0];
      const unsigned poff = (odd ? off[1] : off[0]) - (odd ? 1u : 0u);
      *reinterpret_cast<unsigned*>(hout + poff) = pact ? pk : 0u;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        gates[offg[r]] = (cbf16x4_t){(__bf16)ig[r], (__bf16)gg[r], (__bf16)fg[r], (__bf16)og[r]};
        cs[offg[r]] = cn[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      oa[r] += dstep;
      os[r] += stride;
    }
    C8_FPIN(2);
    const unsigned long long t2 = C8_T();
    if constexpr (EARLY) {
      if (s + 1 < tmax) {                                  // block-uniform
        if constexpr (!(ABL & 32)) __syncthreads();        // the CU's own slice of h(s) is complete in hnxt
        bf16x8_t ao[KO];
#pragma unroll
        for (int k = 0; k < KO; ++k) ao[k] = *reinterpret_cast<const bf16x8_t*>(hnxt + lrd + krot(k + g * KO) * 64);
        accn0 = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        accn1 = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KO; ++k) {
          accn0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ao[k], wreg[0][k], accn0, 0, 0, 0);
          accn1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ao[k], wreg[1][k], accn1, 0, 0, 0);
        }
      }
    }
    {
      // The first poll round goes out BEHIND the own-slice MFMAs above, not in front of them (left alone the scheduler
      // hoists the poll loads to right behind the barrier, in front of the LDS read and the MFMAs): ~150 cycles later --
      // forward launch 840 -> 805 us at H = 256, 1400 -> 1358 at H = 512, 975 -> 967 at H = 320.  (Later still is worse again: + 128 cycles 818 us,
      // + 256 860, + 384 882; the fp32 kernel, whose own-slice MFMAs take three times as long, gains nothing from it.)
      // (Round 5, measured: TWO poll rounds in flight -- the second issued s_sleep(2 / 4 / 6) behind the first, before it
      // returns -- is slower by exactly the sleep: 693 -> 722 / 765 / 838 us per launch, same bits.  The L2 round trip of a
      // poll is ~200 cycles, so the one-round loop already samples every ~200 cycles; the 0.7 - 1.0 repolls per step of the
      // phase probe cost what they look like, not a fabric trip each.)
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (XW) {
        constexpr unsigned pbytes = (unsigned)P * G * SLICE * 4u;   // this parity's slices
        xw4_t v[NL];
        unsigned spins = 0;
#pragma unroll 1
        for (;;) {                                         // wave-uniform loop: no exec masking
          asm volatile("" ::: "memory");                   // every round is a fresh set of loads
          if constexpr ((ABL & 512) != 0) {
#pragma unroll
            for (int j = 0; j < NL; ++j) v[j] = (xw4_t){pk, pk, pk, pk};
            break;
          }
#pragma unroll
          for (int j = 0; j < NL; ++j)                      // L1-bypassing (sc1) 16-byte loads, counted on vmcnt by the compiler
            v[j] = __builtin_amdgcn_raw_buffer_load_b128(xwrs, xvoff[j], pbytes, 16);
          // v ^ tag has the two tag bits clear exactly where the word is this step's -- and is then the clean payload
          unsigned bad = 0;
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            v[j] ^= etag;
            bad |= v[j][0] | v[j][1] | v[j][2] | v[j][3];
          }
          if (__all((bad & XW_MASK) == 0u)) break;
          if constexpr ((ABL & 1) != 0) break;              // one round, whatever it carries
          if (++spins > spin_limit) { timed_out = true; spin_limit = 0; break; }
        }
        if (DBG) nspin += spins;
        C8_FPIN(7);                                        // behind the poll loop
        if constexpr ((ABL & 256) != 0) {
#pragma unroll
          for (int j = 0; j < NL; ++j) asm volatile("" ::"v"(v[j]));
        } else {
#pragma unroll
        for (int j = 0; j < NL; ++j) *reinterpret_cast<xw4_t*>(hnxt + xldst[j]) = v[j];
        }
        C8_FPIN(8);                                        // behind the LDS staging
      } else {
      u64 v[G - 1];
#pragma unroll
      for (int k = 0; k < G - 1; ++k) v[k] = gload(uoff(slice(P, k + (k >= g ? 1 : 0)), lofs));
      unsigned spins = 0;
#pragma unroll 1
      for (;;) {                                           // wave-uniform loop: no exec masking
        bool ok = true;
#pragma unroll
        for (int k = 0; k < G - 1; ++k) ok = ok && ((unsigned)(v[k] >> 32) == epoch);
        if (__all(ok)) break;
        if (++spins > spin_limit) { timed_out = true; spin_limit = 0; break; }
#pragma unroll
        for (int k = 0; k < G - 1; ++k) v[k] = gload(uoff(slice(P, k + (k >= g ? 1 : 0)), lofs));
      }
      if (DBG) nspin += spins;
      C8_FPIN(7);                                          // behind the poll loop
#pragma unroll
      for (int k = 0; k < G - 1; ++k) *reinterpret_cast<unsigned*>(hnxt + ldst[k]) = (unsigned)v[k];
      C8_FPIN(8);                                          // behind the LDS staging
      }
    }
    // saved activations: stored behind the poll loop -- on gfx950 loads and stores share one in-order counter, so a poll
    // issued after these stores waits for their acknowledgements too (0.921 -> 0.908 ms per launch)
    if constexpr (LATE_STORE && !(ABL & 16)) {
      const bool pact = odd ? act[1] : act[0];
      const unsigned poff = (odd ? offs[1] : offs[0]) - (odd ? 1u : 0u);
      *reinterpret_cast<unsigned*>(hout + poff) = pact ? pk : 0u;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        gates[offgs[r]] = (cbf16x4_t){(__bf16)ig[r], (__bf16)gg[r], (__bf16)fg[r], (__bf16)og[r]};
        cs[offgs[r]] = cn[r];
      }
    }
    C8_FPIN(3);
    const unsigned long long t3 = C8_T();
    if constexpr (!(ABL & 32)) __syncthreads();
    if (DBG) {
      const unsigned long long t4 = C8_T();
      ph[0] += t1 - t0; ph[1] += t2 - t1; ph[2] += t3 - t2; ph[3] += t4 - t3;
    }
  };
  int s = 0;
  for (; s + 1 < tmax; s += 2) {
    step(s, std::integral_constant<int, 0>{});
    step(s + 1, std::integral_constant<int, 1>{});
  }
  if (s < tmax) step(s, std::integral_constant<int, 0>{});
#undef C8_T
#undef C8_FPIN

  if (DBG && dbg && lane == 0 && cid.tile == 0 && g < 4) {
    unsigned long long* o = dbg + 256 + ((size_t)(d * 4 + g) * 8 + wave) * 8;   // [256, 768): 8-wave kernels
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = ph[k];
    o[4] = nspin;
    o[5] = tmax;
    o[6] = fast ? 1 : 0;
    o[7] = ph4;
  }
  if (timed_out) atomicOr(err, 1u);
  // XW forces bits 14 / 30 of a published word (the step tag), so a NaN / Inf h (exponent all ones) would reach the
  // peers as a finite value while its owner keeps the NaN: report it instead of laundering it.  h =
  // o * tanh(c) is in [-1, 1], whose bf16 forms all have bit 14 clear; any set bit 14 is a non-finite (or > 1) value.
  if (XW && (nonfin & XW_MASK)) atomicOr(err, 4u);
  // zero-fill the common padded tail [tmax, T): os already points at frame tmax
  for (int t = tmax; t < T_; ++t)
#pragma unroll
    for (int r = 0; r < 2; ++r) { hout[os[r]] = 0; os[r] += stride; }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const size_t o = ((size_t)d * B_ + b0 + rbase + r) * H + jw;
    if (c_final) c_final[o] = c[r];
    if (h_final) h_final[o] = hr[r];
  }
}

// (Round 6, profiles/r06_lstm_ablation.md -- the step with one piece compiled out at a time, ABL above: free-running (no
// poll at all) the forward step is 0.753 of its 0.929 us, i.e. the cross-CU exchange is 19 % of the step; the A-fragment
// reads cost 0.016 - 0.05 us (the "800 exposed LDS cycles" of the round-5 s_memtime table were the timers: s_memtime returns
// on the counter the LDS reads use), the MFMAs 0.10, gate math 0.11 - 0.13, the two barriers 0.11, staging 0.03 - 0.06,
// stores 0.044, x fetch 0.033, and 0.23 is publish / own-slice hop / DPP / addresses.  No piece is above 14 %.)
// (Round 6, built and measured, profiles/r06_helper_wave.md: a FIFTH wave per workgroup that owns the step's big arrays -- it
// fetched the x rows ahead into an LDS image and copied the saved activations from an LDS image to memory, so that the chain
// waves issued no global load / store at all.  Bit-identical.  An idle fifth wave costs nothing (690 vs 694 us per launch);
// the stores through it gain 1.2 % at H = 256 (686 us) and LOSE 18 % at H = 512 (2 004 -> 2 380 us); x through LDS loses
// 12 % whatever the prefetch depth (2 or 4 steps) and wherever the helper writes it (775 - 809 us).  Removed again.)
// (Round 5, built and measured: a forward kernel WITHOUT the LDS image -- the slice layout [wave][row][8 units] is already the
// A operand of v_mfma_f32_16x16x32_bf16, so every wave polled the 16 bytes per lane of ALL G slices and multiplied them as
// they came: no staging, no barrier, no LDS read on the chain.  Correct (same parity figures) and SLOWER: 695 -> 805 - 813 us
// per launch at H = 256.  A poll round is then 4 waves x 8 KB = 32 KB per CU through a 64 B/clk L2 port (~500 cycles)
// instead of 8 KB shared through the LDS (128 B/clk): the staging is what keeps the hop short.  Removed again.)

// ---------------------------------------------------------------- forward, H = 256 on 16 CUs x four waves x 4 units
// The next halving of the forward form above (HSU = 32 -> 16): a wave owns FOUR units, so its whole step is ONE 16-column
// MFMA tile -- column n = gate (n >> 2) of unit (n & 3) -- over the eight k-chunks (8 MFMAs instead of 16, 32 VGPRs of W_h
// instead of 64) and the gate math of ONE (row, unit) pair per lane.  After the MFMAs lane (gate q, unit u, row group rg)
// holds gate q of rows rg*4 .. rg*4+3; a 4 x 4 transpose over the lanes q = 0..3 of a DPP row (bank-masked row_ror:4/8/12
// moves: the bank mask picks the destination lanes, so the source register is a constant and nothing is selected with
// v_cndmask) leaves it with all four gates of (row rg*4 + q, unit u).
// Same bits as the HSU = 32 EARLY form: same operand roles in the MFMA, and the k-chunks of unit j are accumulated from
// chunk j / 32 upwards, cyclically -- the order that form's own-slice-early trick produces.  A CU's own 16 units are half a
// k-chunk, so nothing can be multiplied early here: all eight chunks go behind the poll, ONE barrier per step.
// Exchange: 4-byte self-tagged words (xw_tag), slice of a CU = [16 rows][16 units] bf16 = 512 bytes = 32 16-byte pieces
// (row, half).  The 16 slices of a cluster -- the CU's own among them, which therefore needs no LDS write of its own -- are
// 512 pieces: exactly two 16-byte polls per lane and round, wave w taking the whole slices of CUs 4w .. 4w+3, each piece
// staged with one ds_write_b128.  A pair of lanes (units u, u^1) publishes its word twice (same address, same value):
// nothing in the step is exec-masked, and the word must go out as ONE 4-byte store to validate itself.
// Everything else as above: h image XOR-swizzled and double-buffered by step parity, x rows requested two steps ahead,
// parked positions, saved activations stored behind the poll loop, bounded spins, zero_next_area.  ABL as above (bit 5
// leaves out the one barrier; there is no own-slice LDS write to ablate).
template <int FPIN = 0, int ABL = 0>
__global__ __launch_bounds__(256, 1) void lstm_fwd_cluster16_kernel(
    int T_, int B_, int ndir, const f32x4_t* __restrict__ xg, const bf16_t* __restrict__ whp,
    const float* __restrict__ peep, const int32_t* __restrict__ seq_len, float forget_bias,
    float cell_clip, cbf16x4_t* __restrict__ gates, bf16_t* __restrict__ hout, float* __restrict__ cs,
    float* __restrict__ c_final, float* __restrict__ h_final, u64* __restrict__ xch,
    unsigned* __restrict__ err, int kflags, u64* __restrict__ znext, unsigned zwords, int tile0, int ntl) {
  zero_next_area(znext, zwords);
  constexpr int H = 256, HSU = 16, G = H / HSU, KS = H / 32, LDH = H + 8;
  constexpr int SLICE = 16 * (HSU / 2);                     // words one CU publishes per step (slot stride as in the forms above)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* hs = reinterpret_cast<bf16_t*>(smem);            // [2][16][LDH]

  const ClusterId cid = cluster_id<G>(ndir, tile0, ntl);
  if (!cid.valid) return;
  const int g = cid.g, d = cid.d, b0 = cid.tile * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, rg = lane >> 4;
  const int q = col >> 2, u = col & 3;                     // gate of this lane's MFMA column, unit inside the wave
  const bool odd = (u & 1) != 0;
  const bool rev = (d == 1);
  const bf16_t* wp = whp + (size_t)d * H * 4 * H;
  const unsigned jw = g * HSU + wave * 4 + u;              // global unit of this lane
  const int row = rg * 4 + q;                              // this lane's batch row

  const int len = seq_len[b0 + row];
  int tmax = 0;
  for (int i = 0; i < 16; ++i) tmax = max(tmax, seq_len[b0 + i]);
  tmax = min(tmax, T_);

  float c = 0.f, hr = 0.f;
  const float wci = peep ? peep[(d * 3 + 0) * H + jw] : 0.f;
  const float wcf = peep ? peep[(d * 3 + 1) * H + jw] : 0.f;
  const float wco = peep ? peep[(d * 3 + 2) * H + jw] : 0.f;

  for (int i = threadIdx.x; i < 2 * 16 * LDH; i += 256) hs[i] = 0;
  // B fragments out of the standard forward packing (tile = (unit/16)*4 + gate, column unit%16): this lane's column is
  // (gate q, unit jw); register chunk ks holds k-chunk (ks + jw/32) % 8 -- the accumulation order of the HSU = 32 form
  bf16x8_t wreg[KS];
  const int k0 = g >> 1;
  {
    const int tile = (jw >> 4) * 4 + q;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int kk = (ks + k0) & (KS - 1);
      wreg[ks] = *reinterpret_cast<const bf16x8_t*>(wp + (((size_t)tile * KS + kk) * 64 + rg * 16 + (jw & 15)) * 8);
    }
  }

  u64* xhdr = xch + (size_t)cid.c * (XHDR + 2 * G * SLICE);
  u64* xbase = xhdr + XHDR;                                // as words: [2 parity][G][16 rows][8 words]
  bool timed_out = false;
  const bool colocated = same_xcd<G>(xhdr, g, timed_out);
  const bool fast = colocated && !(kflags & 1);            // same decision on every member
  unsigned spin_limit = (kflags & 2) ? 2000u : SPIN_LIMIT; // after the first timeout the limit drops to 0
  if ((kflags & 2) && g == G - 1) return;                  // TEST ONLY (ASR_LSTM_DFLAGS bit 6): a member goes missing
  __syncthreads();

  const unsigned stride = (unsigned)B_ * ndir * H;
  const unsigned dstep = rev ? 0u - stride : stride;
  unsigned os = ((unsigned)(b0 + row) * ndir + d) * H + jw;                    // frame s of this (row, unit)
  unsigned oa = os + (rev ? (unsigned)max(len - 1, 0) * stride : 0u);          // frame of the running step of an active row
  const unsigned opark = os + (unsigned)max(tmax - 1, 0) * stride;             // parked position (see the form above)
  const unsigned pofs = (unsigned)(row * 8 + wave * 2 + (u >> 1));             // publish word in the slice
  unsigned* xw = reinterpret_cast<unsigned*>(xbase);
  const __amdgpu_buffer_rsrc_t xwrs = __builtin_amdgcn_make_buffer_rsrc(xw, 0, 0x7fffffff, 0x00020000);
  // poll j of a lane: piece lane % 32 = (row, half) of the slice of CU wave * 4 + j * 2 + lane / 32
  unsigned xvoff[2], xldst[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gsrc = wave * 4 + j * 2 + (lane >> 5), pc = lane & 31, prow = pc >> 1;
    xvoff[j] = (unsigned)(gsrc * SLICE + pc * 4) * 4u;
    // the image is rotated by the CU's first k-chunk, so that register chunk ks reads LDS chunk ks at a constant offset
    xldst[j] = ((unsigned)(prow * LDH + ((gsrc * HSU + (pc & 1) * 8 - k0 * 32) & (H - 1))) * 2u) ^ lds_swz(prow);
  }
  const unsigned lrd = ((unsigned)(col * LDH + rg * 8) * 2u) ^ lds_swz(col);

  f32x4_t xq[2];                                           // xproj rows of the running step, requested TWO steps ahead
  xq[0] = xg[(0 < len) ? oa : opark];
  xq[1] = (tmax > 1) ? xg[(1 < len) ? oa + dstep : opark] : xq[0];

  unsigned nonfin = 0;                                     // OR of every published pair (see the tail of the form above)
#define C16_FPIN(k) do { if constexpr ((FPIN >> (k)) & 1) __builtin_amdgcn_sched_barrier(0); } while (0)
#define C16_G(v, QP, Q) v = __builtin_amdgcn_update_dpp(v, __float_as_int(acc[Q]), /* (no bit_cast of a vector element) */ \
                                                        (QP) == (Q) ? 0xE4 : 0x120 + 4 * (((Q) - (QP)) & 3), 0xF, 1 << (Q), false)
#define C16_GATE(name, QP) float name; { int v_ = 0; C16_G(v_, QP, 0); C16_G(v_, QP, 1); C16_G(v_, QP, 2); C16_G(v_, QP, 3); \
                                         name = __builtin_bit_cast(float, v_); }

  auto step = [&](int s, auto PAR) {
    constexpr int P = decltype(PAR)::value;                // parity of step s
    C16_FPIN(0);
    const char* hcur = smem + P * 16 * LDH * 2;
    char* hnxt = smem + (1 - P) * 16 * LDH * 2;
    const f32x4_t x0 = xq[P];
    if (s + 2 < tmax && !(ABL & 64)) xq[P] = xg[(s + 2 < len) ? oa + 2u * dstep : opark];   // lands during the next steps
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    bf16x8_t afr[KS];                                      // all eight A fragments in flight at once
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if constexpr ((ABL & 2) != 0) afr[ks] = wreg[ks ^ 1];
      else afr[ks] = *reinterpret_cast<const bf16x8_t*>(hcur + lrd + ks * 64);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if constexpr ((ABL & 4) != 0) {                       // keeps the dependence on every fragment, nothing else
        const xw4_t fb = __builtin_bit_cast(xw4_t, afr[ks]);
        acc[0] = __uint_as_float(__float_as_uint(acc[0]) ^ (fb[0] & 1u));
        continue;
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[ks], wreg[ks], acc, 0, 0, 0);
    }
    C16_FPIN(1);
    // 4 x 4 transpose over the lanes q = 0..3: gate q' of (row rg*4 + q, unit u) is acc[q] of lane (q', u, rg)
    C16_GATE(pi, 0) C16_GATE(pq, 1) C16_GATE(pf, 2) C16_GATE(po, 3)
    C16_FPIN(4);                                           // behind the DPP transpose
    const bool act = s < len;
    float ig, gg, fg, og, cn, hn;
    if constexpr ((ABL & 8) != 0) {
      ig = pi + x0[0]; gg = pq + x0[1]; fg = pf + x0[2]; og = po + x0[3];
      cn = c;
      hn = fminf(fmaxf((ig + gg) + (fg + og), -1.f), 1.f);
    } else {
      ig = cfsig(pi + x0[0] + wci * c);
      gg = cftanh(pq + x0[1]);
      fg = cfsig(pf + x0[2] + forget_bias + wcf * c);
      cn = gg * ig + c * fg;
      if (cell_clip > 0.f) cn = fminf(fmaxf(cn, -cell_clip), cell_clip);
      og = cfsig(po + x0[3] + wco * cn);
      hn = cftanh(cn) * og;
    }
    c = act ? cn : c;
    hr = act ? hn : hr;
    C16_FPIN(5);                                           // behind the gate math
    // publish: both lanes of a pair the (even unit, odd unit) word of their row
    const unsigned hb = f32_to_bf16(hr);
    const unsigned nb = (unsigned)__builtin_amdgcn_update_dpp(0, (int)hb, 0xB1, 0xF, 0xF, false);
    const unsigned pk = odd ? (nb | (hb << 16)) : (hb | (nb << 16));
    const unsigned etag = xw_tag(s);
    if constexpr ((ABL & 128) == 0) {
      unsigned* pw = uoff(xw + (size_t)(P * G + g) * SLICE, pofs);
      nonfin |= pk;
      const unsigned tv = (pk & ~XW_MASK) | etag;
      if (fast) __hip_atomic_store(pw, tv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // plain store, stays in the L2
      else __hip_atomic_store(pw, tv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    C16_FPIN(6);                                           // behind the publish
    const unsigned off = act ? oa : os, offg = act ? oa : opark;   // hout position / saved-activation position
    oa += dstep;
    os += stride;
    C16_FPIN(2);
    {
      __builtin_amdgcn_sched_barrier(0);
      constexpr unsigned pbytes = (unsigned)P * G * SLICE * 4u;   // this parity's slices
      xw4_t v[2];
      unsigned spins = 0;
#pragma unroll 1
      for (;;) {                                           // wave-uniform loop: no exec masking
        asm volatile("" ::: "memory");                     // every round is a fresh set of loads
        if constexpr ((ABL & 512) != 0) {
          v[0] = v[1] = (xw4_t){pk, pk, pk, pk};
          break;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)                         // L1-bypassing (sc1) 16-byte loads
          v[j] = __builtin_amdgcn_raw_buffer_load_b128(xwrs, xvoff[j], pbytes, 16);
        unsigned bad = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          v[j] ^= etag;                                    // tag bits clear exactly where the word is this step's
          bad |= v[j][0] | v[j][1] | v[j][2] | v[j][3];
        }
        if (__all((bad & XW_MASK) == 0u)) break;
        if constexpr ((ABL & 1) != 0) break;                // one round, whatever it carries
        if (++spins > spin_limit) { timed_out = true; spin_limit = 0; break; }
      }
      C16_FPIN(7);                                         // behind the poll loop
      if constexpr ((ABL & 256) != 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) asm volatile("" ::"v"(v[j]));
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) *reinterpret_cast<xw4_t*>(hnxt + xldst[j]) = v[j];
      }
      C16_FPIN(8);                                         // behind the LDS staging
    }
    // saved activations behind the poll loop (loads and stores share one in-order counter, see the form above)
    if constexpr (!(ABL & 16)) {
      hout[off] = act ? (bf16_t)hb : (bf16_t)0;
      gates[offg] = (cbf16x4_t){(__bf16)ig, (__bf16)gg, (__bf16)fg, (__bf16)og};
      cs[offg] = cn;
    }
    C16_FPIN(3);
    if constexpr (!(ABL & 32)) __syncthreads();
  };
  int s = 0;
  for (; s + 1 < tmax; s += 2) {
    step(s, std::integral_constant<int, 0>{});
    step(s + 1, std::integral_constant<int, 1>{});
  }
  if (s < tmax) step(s, std::integral_constant<int, 0>{});
#undef C16_FPIN
#undef C16_G
#undef C16_GATE

  if (timed_out) atomicOr(err, 1u);
  if (nonfin & XW_MASK) atomicOr(err, 4u);                 // a non-finite h must not be laundered by the forced tag bits
  for (int t = tmax; t < T_; ++t) { hout[os] = 0; os += stride; }   // common padded tail: os points at frame tmax
  const size_t o = ((size_t)d * B_ + b0 + row) * H + jw;
  if (c_final) c_final[o] = c;
  if (h_final) h_final[o] = hr;
}

// ---------------------------------------------------------------- backward
// K-partition: CU g owns the gate gradients of its 64 units (k' = unit*4+q in its slice) and the
// rows k' of W_h^T; each step it multiplies its dG slice by W_h^T[k' slice, all H] -> a partial
// dh_prev for ALL units, keeps the part for its own units and publishes the rest; the partials
// for its own units from the other CUs are gathered at the next step (reduce-scatter).
// ---------------------------------------------------------------- backward, 8 waves
// Built around what bounds these kernels (instruction issue + the cross-CU hop):
//  * a thread owns TWO (row, unit) pairs in the MFMA C layout: wave w = (hh = w >> 2, wt = w & 3),
//    lane (col, rg) -> unit wt*16 + col of the slice, rows rg*4 + hh*2 + {0,1};
//  * the own-unit tile wt is computed by BOTH waves wt and wt+4 (8 extra MFMAs per wave), so the
//    own partial is already in the right registers: no LDS hand-over, ONE barrier per step;
//  * foreign tiles (12 per CU) are spread 2/1 over the waves of each SIMD and published with one
//    16-byte store per lane: 4 rows of one unit, every fp32 word carrying the step's parity tag in
//    its mantissa LSB (the data is the flag, per word, so any store width is tear-proof);
//  * everything that does not depend on dh (tanh(c), the gate-derivative factors) is computed
//    while the polls for the peers' partials are in flight.
// xch per cluster: header + [2 parity][G dst][G src][4 tiles][64 lanes][4 words].
// HSU = hidden units per CU: 64 (eight waves: 4 unit tiles x 2 row halves) or 32 (four waves, ONE per SIMD: 2 unit tiles x
// 2 row halves, twice the CUs per cluster, the whole 512-entry register file per wave).
// PIN: bit k set = a scheduling barrier at phase boundary k of the step (0: top, 1: behind the fetch, 2: in front of the
// step's barrier, 3: end) -- the places where the timer build has its s_memtime reads.  -1: the default for the width.
// Measured, BPTT launch at H = 256 (four waves): no pins 888 us; {1,2} 888; {0,3} 859; {0,1,2} 859; {1,2,3} 859; {0,1,3} 855; all
// four 855 -- what matters is that nothing moves across the STEP boundary (the scheduler otherwise interleaves the next
// iteration's polls and address arithmetic with this iteration's MFMAs and exchange stores).  H = 512: none 1537, {0} 1538,
// {1} 1530, {2} 1529, {1,2} 1528, {3} 1605, {0,3} 1570, all four 1567 -- there the pins stay off.  Further points on top of the
// four at H = 256 (bits 4..8: behind the poll issue / the dh-independent math / the poll loop / the barrier / the gradient
// sums): 858 / 858 / 849 / 856 / 857 against 855 -- bit 6 is kept.  (H = 512 with bit 6 / {1,2,6} / bit 5: 1541 / 1535 / 1536
// against 1530; finer points -- between the foreign-tile chains and their stores / between those stores and the own-tile
// chain / in front of the A-fragment reads: 1575 / 1525 / 1523 against 1519; forward, between the two A-fragment batches:
// 1364 against 1353.)
// XP (default): the reduce-scatter slots are laid out for the CONSUMER -- a destination wave (hh, wt) finds the two rows it
// owns of TWO sources side by side in one 16-byte word per lane, [dst][tile][hh][source pair][lane]: ceil((G-1)/2)
// full-line 16-byte polls per round instead of G-1 8-byte ones that each use half of the 16 bytes per lane they touch
// (8-byte L2 accesses run at 0.54-0.70x the 16-byte rate, MI355X_MICROARCH.md).  The producers pay with two 8-byte
// stores per lane and tile (rows 0,1 -> the hh = 0 word, rows 2,3 -> hh = 1) instead of one 16-byte store.  Same words,
// same tags, same summation order: bit-identical to XP = false.  Which form runs: bwd_xp_enabled() (a win only on the
// eight-wave clusters, measured there).
// ABL (builds with -DASR_LSTM_ABLATE only): bit k set = piece k of the step is left out, as in the forward kernel.  0: the
// poll loop does not wait for valid tags, 1: no A-fragment reads from LDS, 2: no MFMAs, 3: no gate-gradient math, 4: no
// dgates store to memory, 5: no barrier, 6: no fetch of the saved activations, 7: no publish stores, 8: no dG write to
// LDS, 9: no poll loads at all.
// CLIPZ (asr_lstm_bwd_ex with bf16 operands, the projected LSTMCell layers): a state whose saved cs has |c| >= clipz passes no
// gradient to its gates or to c_prev (tf.clip_by_value); its own instantiations -- the default kernels' code does not change.
template <int H, bool DBG, int HSU = 64, int PIN = -1, bool XP = true, int ABL = 0, bool CLIPZ = false>
__global__ __launch_bounds__(HSU * 8, 1) void lstm_bwd_cluster8_kernel(
    int T_, int B_, int ndir, const float* __restrict__ dhout, const cbf16x4_t* __restrict__ gates,
    const float* __restrict__ cs, const bf16_t* __restrict__ whpb, const float* __restrict__ peep,
    const int32_t* __restrict__ seq_len, const float* __restrict__ d_c_final,
    const float* __restrict__ d_h_final, cbf16x4_t* __restrict__ dgates, float* __restrict__ dpeep_part,
    u64* __restrict__ xch, unsigned* __restrict__ err, int kflags, u64* __restrict__ znext, unsigned zwords, float clipz, int tile0, int ntl) {
  zero_next_area(znext, zwords);
  constexpr int PINM = PIN >= 0 ? PIN : ((HSU == 32 && H <= 320) ? (15 | 64) : 0);   // (H = 320 on eight waves: 1089 -> 1216 us with pins)
  constexpr int G = H / HSU;
  constexpr int TPC = HSU / 16;              // 16-unit output tiles per CU (4 / 2)
  constexpr int NWAVES = 2 * TPC;            // waves per workgroup
  constexpr int KC = 4 * HSU / 32;           // k-chunks of this CU's slice (8 / 4)
  constexpr int KSF = 4 * H / 32;            // k-chunks of the full packing
  constexpr int LDG = 4 * HSU + 8;
  constexpr size_t CL_U64 = XHDR + (size_t)2 * G * G * TPC * 64 * 2;   // u64 words per cluster
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // smem: [2][16][LDG] bf16 -- the own dG slice (MFMA A operand), double-buffered by iteration
  // parity so that ONE barrier per step orders writers and readers
  constexpr int DGB = 16 * LDG * 2;                        // bytes per buffer

  const ClusterId cid = cluster_id<G>(ndir, tile0, ntl);
  if (!cid.valid) return;
  const int g = cid.g, d = cid.d, b0 = cid.tile * 16;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, rg = lane >> 4;
  const int hh = wave / TPC, wt = wave % TPC;
  const bool rev = (d == 1);
  const bf16_t* wp = whpb + (size_t)d * H * 4 * H;
  const int ul = wt * 16 + col;
  const unsigned jw = g * HSU + ul;
  const int rbase = rg * 4 + hh * 2;

  int len[2];
  int tmax = 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) len[r] = seq_len[b0 + rbase + r];
  for (int i = 0; i < 16; ++i) tmax = max(tmax, seq_len[b0 + i]);
  tmax = min(tmax, T_);

  const float wci = peep ? peep[(d * 3 + 0) * H + jw] : 0.f;
  const float wcf = peep ? peep[(d * 3 + 1) * H + jw] : 0.f;
  const float wco = peep ? peep[(d * 3 + 2) * H + jw] : 0.f;

  // element offsets: os = frame s, oa = frame of step s for an active row (s or len-1-s)
  const unsigned stride = (unsigned)B_ * ndir * H;
  const unsigned dstep = rev ? stride : 0u - stride;      // oa moves with decreasing s
  unsigned oa[2], os[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned base = ((unsigned)(b0 + rbase + r) * ndir + d) * H + jw;
    os[r] = base + (unsigned)(tmax - 1) * stride;
    oa[r] = base + (unsigned)(rev ? len[r] - tmax : tmax - 1) * stride;
  }
  // inactive rows read nothing that is used: their fetches go to one parked position per row (frame tmax - 1, padding
  // for any row that is ever inactive) that stays in the L2 -- see the forward kernel
  unsigned opark[2] = {os[0], os[1]};
  // zero the gate gradients of the common padded tail [tmax, T)
  {
    const cbf16x4_t gzero = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
    for (int t = tmax; t < T_; ++t)
#pragma unroll
      for (int r = 0; r < 2; ++r) dgates[os[r] + (unsigned)(t - tmax + 1) * stride] = gzero;
  }

  float dhr[2], dcr[2], cc[2];
  float sums[7] = {0, 0, 0, 0, 0, 0, 0};     // dwci, dwcf, dwco, db_i, db_g, db_f, db_o
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const size_t o = ((size_t)d * B_ + b0 + rbase + r) * H + jw;
    dhr[r] = d_h_final ? d_h_final[o] : 0.f;
    dcr[r] = d_c_final ? d_c_final[o] : 0.f;
    cc[r] = (tmax > 0 && tmax - 1 < len[r]) ? cs[oa[r]] : 0.f;
  }
  // W_h^T fragments: own tile (4g + wt) and this wave's foreign tiles f = wave, 8 + wave, ...
  // foreign index f in [0, 4(G-1)): destination CU = (f >> 2) skipping g, tile inside it = f & 3
  constexpr int NFT = TPC * (G - 1);                       // foreign tiles per CU (12 / 28; HSU = 32: 14 / 30)
  // G = 4: every wave also computes its own-unit tile (both row-half waves redundantly: no hand-over, one
  //        barrier per step) next to NF = 2 / 1 foreign tiles.
  // G = 8: that would be 5 tiles x 32 fragment registers per wave and spills (measured: 8 k of the 10 k
  //        cycles per step); instead the 4 own + 28 foreign tiles are dealt 4 per wave, the own tile is
  //        computed once by the hh = 0 wave, which hands rows 2,3 to its hh = 1 partner through LDS (a
  //        second barrier per step, cheap next to 32 MFMAs per wave).
  // HSU = 32 (one wave per SIMD, 512 registers): the redundant own tile again, NF = 4 (H = 256) / 8 (H = 512) foreign sets.
  constexpr bool OWN_ONCE = (G == 8 && HSU == 64);
  constexpr int NF = OWN_ONCE ? 4 : (NFT + NWAVES - 1) / NWAVES;   // fragment sets per wave (last one: see below)
  auto ftile = [&](int f) { const int q = f / TPC; return ((q + (q >= g ? 1 : 0)) * TPC) | (f % TPC); };
  const int nt_own = g * TPC + wt;
  // OWN_ONCE: slot NF-1 is the own tile on hh = 0 waves and foreign tile 24 + wt on hh = 1 waves
  const bool last_f = OWN_ONCE ? (hh == 1) : (wave < NFT - NWAVES * (NF - 1));
  int nt_f[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    if (OWN_ONCE) nt_f[i] = (i < NF - 1) ? ftile(wave + 8 * i) : (hh == 1 ? ftile(24 + wt) : nt_own);
    else nt_f[i] = ftile((i < NF - 1 || last_f) ? wave + NWAVES * i : wave);
  }
  bf16x8_t wo[OWN_ONCE ? 1 : KC], wf[NF][KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    if (!OWN_ONCE)
      wo[kc] = *reinterpret_cast<const bf16x8_t*>(wp + (((size_t)nt_own * KSF + g * KC + kc) * 64 + lane) * 8);
#pragma unroll
    for (int i = 0; i < NF; ++i)
      wf[i][kc] = *reinterpret_cast<const bf16x8_t*>(wp + (((size_t)nt_f[i] * KSF + g * KC + kc) * 64 + lane) * 8);
  }
  // OWN_ONCE hand-over buffer behind the two dG images: [2 parity][4 tiles][64 lanes] x (row 2, row 3)
  float* ownx = reinterpret_cast<float*>(smem + 2 * DGB);

  u64* xhdr = xch + (size_t)cid.c * CL_U64;
  bool timed_out = false;
  const bool fast = same_xcd<G>(xhdr, g, timed_out) && !(kflags & 1);
  unsigned spin_limit = (kflags & 2) ? 2000u : SPIN_LIMIT;  // drops to 0 after the first timeout
  if ((kflags & 2) && g == G - 1) return;                  // TEST ONLY (ASR_LSTM_DFLAGS bit 6): a member goes missing
  f32x4_t* xs = reinterpret_cast<f32x4_t*>(xhdr + XHDR);   // [2][G dst][G src][4][64] x 16 B
  auto uslot = [&](int par, int dst, int src_, int tile) -> f32x4_t* {       // uniform part of a slot
    return xs + ((((size_t)par * G + dst) * G + src_) * TPC + tile) * 64;
  };
  const unsigned voff16 = (unsigned)lane * 16u;            // byte offset of this lane's 16-byte word group
  const unsigned pofs = (unsigned)lane * 2u + hh;          // u64 index of this lane's two rows in a slot
  // XP: 16-byte units [2 par][G dst][TPC][2 hh][NPAIR][64 lanes]; source g sits in pair k/2, half k%2 of destination
  // dst, k = g - (g > dst) its index among dst's peers
  constexpr int NPAIR = G / 2;                             // = ceil((G - 1) / 2)
  auto pslot = [&](int par, int dst, int tile, int h2, int pair) -> unsigned {   // uniform 16-byte index
    return (unsigned)((((par * G + dst) * TPC + tile) * 2 + h2) * NPAIR + pair) * 64u;
  };
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(xs, 0, 0x7fffffff, 0x00020000);
  // own dG rows -> LDS (bytes); rows rbase, rbase+1 are in the same swizzle class (rbase is even)
  const unsigned lwr[2] = {((unsigned)(rbase * LDG + ul * 4) * 2u) ^ lds_swz(rbase),
                           ((unsigned)((rbase + 1) * LDG + ul * 4) * 2u) ^ lds_swz(rbase + 1)};
  const unsigned lrd = ((unsigned)(col * LDG + rg * 8) * 2u) ^ lds_swz(col);   // A fragment reads

  // saved activations of iteration s, fetched one iteration ahead
  // saved activations of iteration s, fetched one iteration ahead (two ahead was measured: 1.34 -> 1.37 ms)
  cbf16x4_t pg[2];
  float pcp[2], pdh[2];
  auto prefetch = [&](int s_) {                            // oa/os already hold iteration s_
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const bool act = s_ < len[r];
      const bool ldp = (s_ > 0) && (s_ - 1 < len[r]);
      const unsigned offl = act ? oa[r] : opark[r];
      const unsigned offn = ldp ? oa[r] + dstep : opark[r];
      pg[r] = gates[offl];
      pcp[r] = cs[offn];
      pdh[r] = dhout[offl];
    }
  };
  if (tmax > 0) prefetch(tmax - 1);
  __syncthreads();

  unsigned long long* dbg = g_cdbg;
  unsigned long long ph[4] = {0, 0, 0, 0};
  unsigned nspin = 0;
#define C8_T() (DBG ? (__builtin_amdgcn_sched_barrier(0), __builtin_amdgcn_s_memtime()) : 0ull)
#define C8_PIN(k) do { if constexpr (!DBG && ((PINM >> (k)) & 1)) __builtin_amdgcn_sched_barrier(0); } while (0)

  auto step = [&](int s, auto PAR) {
    constexpr int P = decltype(PAR)::value;                // parity of THIS iteration's publish
    const int it = tmax - 1 - s;                           // 0, 1, ...
    C8_PIN(0);
    const unsigned long long t0 = C8_T();
    // ---- 1. polls for the partials the peers published at the previous iteration (parity 1-P)
    u64 pv[XP ? 1 : G - 1];
    xw4_t pq[XP ? NPAIR : 1];
    if (it > 0) {
      if constexpr (XP) {
#pragma unroll
        for (int p = 0; p < NPAIR; ++p)                     // L1-bypassing (sc1) 16-byte loads, counted on vmcnt by the compiler
          pq[p] = __builtin_amdgcn_raw_buffer_load_b128(xrs, voff16, pslot(1 - P, g, wt, hh, p) * 16u, 16);
      } else if constexpr ((ABL & 512) != 0) {
#pragma unroll
        for (int k = 0; k < G - 1; ++k) pv[k] = (u64)(unsigned)lane;
      } else {
#pragma unroll
        for (int k = 0; k < G - 1; ++k)
          pv[k] = gload(uoff(reinterpret_cast<const u64*>(uslot(1 - P, g, k + (k >= g ? 1 : 0), wt)), pofs));
      }
    }
    C8_PIN(4);                                             // behind the poll issue
    // ---- 2. everything that does not need dh
    bool act[2], ldp[2];
    float gi[2], gq[2], gf[2], go[2], cprev[2], a_o[2], b_c[2], c_g[2], c_i[2], c_f[2];
    unsigned off[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      act[r] = s < len[r];
      ldp[r] = (s > 0) && (s - 1 < len[r]);
      off[r] = act[r] ? oa[r] : os[r];
      gi[r] = (float)pg[r][0]; gq[r] = (float)pg[r][1]; gf[r] = (float)pg[r][2]; go[r] = (float)pg[r][3];
      cprev[r] = (act[r] && s > 0) ? pcp[r] : 0.f;
    }
    float tc[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) tc[r] = cftanh(cc[r]);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      a_o[r] = tc[r] * go[r] * (1.f - go[r]);
      b_c[r] = go[r] * (1.f - tc[r] * tc[r]);
      c_g[r] = gi[r] * (1.f - gq[r] * gq[r]);
      c_i[r] = gq[r] * gi[r] * (1.f - gi[r]);
      c_f[r] = cprev[r] * gf[r] * (1.f - gf[r]);
    }
    float pdh0 = pdh[0], pdh1 = pdh[1], pcp0 = pcp[0], pcp1 = pcp[1];
    const float cur0 = cc[0], cur1 = cc[1];
    if constexpr (HSU == 32) {
      // Everything that reads the values fetched one iteration ago is pinned HERE, ahead of the next fetch.  With 512
      // registers the allocator alternates the fetch's destination registers between the two unrolled iterations and
      // lets the last read of the old ones (cprev) sink below the new fetch; at the join behind the conditional fetch it
      // then has to wait with vmcnt(0) -- for the NEW fetch, i.e. for HBM, on every step (1.25 instead of 0.95 ms/launch).
      asm volatile("" : "+v"(pdh0), "+v"(pdh1), "+v"(pcp0), "+v"(pcp1), "+v"(cprev[0]), "+v"(cprev[1]));
      asm volatile("" : "+v"(c_g[0]), "+v"(c_g[1]), "+v"(c_i[0]), "+v"(c_i[1]), "+v"(c_f[0]), "+v"(c_f[1]));
      asm volatile("" : "+v"(a_o[0]), "+v"(a_o[1]), "+v"(b_c[0]), "+v"(b_c[1]), "+v"(gf[0]), "+v"(gf[1]));
    }
    // next iteration's inputs (independent of everything below)
#pragma unroll
    for (int r = 0; r < 2; ++r) { oa[r] += dstep; os[r] -= stride; }
    // The fetch of the next iteration's saved activations used to go out here, ahead of the poll loop; kflags bit 2
    // (ASR_LSTM_DFLAGS bit 7) puts it back for A-B runs.  It now goes out BEHIND the loop, see there.
    const bool early_fetch = (kflags & 4) != 0;
    if (s > 0 && early_fetch) prefetch(s - 1);
    C8_PIN(5);                                             // behind the dh-independent math
    // ---- 3. finish the polls: every word must carry the previous iteration's tag
    if (it > 0) {
      const unsigned want = (((unsigned)(it - 1) >> 1) + 1u) & 1u;
      const u64 wmask = 0x0000000100000001ull, wtag = want ? wmask : 0ull;
      unsigned spins = 0;
      float add0 = 0.f, add1 = 0.f;
      if constexpr (XP) {
#pragma unroll 1
        for (;;) {
          unsigned bad = 0;                                 // LSB of every live word must be the tag
#pragma unroll
          for (int p = 0; p < NPAIR; ++p) {
            bad |= (pq[p][0] ^ want) | (pq[p][1] ^ want);
            if (2 * p + 1 <= G - 2) bad |= (pq[p][2] ^ want) | (pq[p][3] ^ want);   // (G even: the last pair has one source)
          }
          if (__all((bad & 1u) == 0u)) break;
          if (++spins > spin_limit) { timed_out = true; spin_limit = 0; break; }
          asm volatile("" ::: "memory");                    // a fresh round of loads, not the old values
#pragma unroll
          for (int p = 0; p < NPAIR; ++p)
            pq[p] = __builtin_amdgcn_raw_buffer_load_b128(xrs, voff16, pslot(1 - P, g, wt, hh, p) * 16u, 16);
        }
#pragma unroll
        for (int k = 0; k < G - 1; ++k) {                   // fixed order: source index ascending, as XP = false
          add0 += __uint_as_float(pq[k >> 1][(k & 1) * 2 + 0] & ~1u);
          add1 += __uint_as_float(pq[k >> 1][(k & 1) * 2 + 1] & ~1u);
        }
      } else {
#pragma unroll 1
        for (;;) {
          bool ok = true;
#pragma unroll
          for (int k = 0; k < G - 1; ++k) ok = ok && ((pv[k] & wmask) == wtag);
          if (__all(ok)) break;
          if constexpr ((ABL & (1 | 512)) != 0) break;       // whatever the first round carried
          if (++spins > spin_limit) { timed_out = true; spin_limit = 0; break; }
#pragma unroll
          for (int k = 0; k < G - 1; ++k)
            pv[k] = gload(uoff(reinterpret_cast<const u64*>(uslot(1 - P, g, k + (k >= g ? 1 : 0), wt)), pofs));
        }
#pragma unroll
        for (int k = 0; k < G - 1; ++k) {                   // fixed order
          add0 += __uint_as_float((unsigned)pv[k] & ~1u);
          add1 += __uint_as_float((unsigned)(pv[k] >> 32) & ~1u);
        }
      }
      if (DBG) nspin += spins;
      dhr[0] += add0;
      dhr[1] += add1;
    }
    // The fetch of the next iteration's saved activations goes out BEHIND the poll loop.  Vector loads return in order: a
    // re-poll issued after a fetch that has to come from HBM cannot land before that fetch does, so with the fetch in
    // front of the loop the hand-off waited for DRAM on every step whose first poll came too early -- 1.22 ms per
    // launch against 0.94 ms behind it (11.93 -> 10.52 ms per headline step); the fetch still has the rest of the
    // step to arrive.  (Written as the second arm of a run-time switch on purpose: as an unconditional statement the
    // compiler schedules these independent loads differently and the launch takes 1.06 ms.)
    C8_PIN(6);                                             // behind the poll loop, in front of the fetch
    if constexpr ((ABL & 64) != 0) {
    } else if constexpr (HSU == 32) {
      // unconditional (the last iteration re-fetches its own rows: harmless) and pinned behind the loop by a compiler
      // barrier: behind a branch the wait-count pass waits with vmcnt(0) -- for THIS fetch -- at the join
      asm volatile("" ::: "memory");
      const bool more = s > 0;                             // block-uniform
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const bool actn = s - 1 < len[r];
        const bool ldpn = (s - 1 > 0) && (s - 2 < len[r]);
        const unsigned offl = more ? (actn ? oa[r] : opark[r]) : off[r];   // (oa / os already hold iteration s - 1)
        const unsigned offn = more ? (ldpn ? oa[r] + dstep : opark[r]) : off[r];
        pg[r] = gates[offl];
        pcp[r] = cs[offn];
        pdh[r] = dhout[offl];
      }
    } else {
      if (s > 0 && !early_fetch) prefetch(s - 1);
    }
    C8_PIN(1);
    const unsigned long long t1 = C8_T();
    // ---- 4. gate gradients of the own pairs
    const float pdhv[2] = {pdh0, pdh1}, pcpv[2] = {pcp0, pcp1}, curv[2] = {cur0, cur1};
    float zi[2], zg[2], zf[2], zo[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const float dh = pdhv[r] + dhr[r];
      if constexpr ((ABL & 8) != 0) {
        zi[r] = zg[r] = zf[r] = zo[r] = dh;
        dhr[r] = 0.f;
      } else {
      const float d_o = dh * a_o[r];
      const float dct = dcr[r] + dh * b_c[r] + d_o * wco;
      const float dc = (CLIPZ && fabsf(curv[r]) >= clipz) ? 0.f : dct;
      const float d_g = dc * c_g[r], d_i = dc * c_i[r], d_f = dc * c_f[r];
      dcr[r] = act[r] ? (dc * gf[r] + d_i * wci + d_f * wcf) : dcr[r];
      dhr[r] = act[r] ? 0.f : dhr[r];
      zi[r] = act[r] ? d_i : 0.f; zg[r] = act[r] ? d_g : 0.f;
      zf[r] = act[r] ? d_f : 0.f; zo[r] = act[r] ? d_o : 0.f;
      }
      cc[r] = ldp[r] ? pcpv[r] : 0.f;
      const cbf16x4_t pk = {(__bf16)zi[r], (__bf16)zg[r], (__bf16)zf[r], (__bf16)zo[r]};
      if constexpr (!(ABL & 256)) *reinterpret_cast<cbf16x4_t*>(smem + P * DGB + lwr[r]) = pk;
      if constexpr (!(ABL & 16)) dgates[off[r]] = pk;
      if constexpr ((ABL & (256 | 16)) == (256 | 16)) asm volatile("" ::"v"(pk));
    }
    C8_PIN(2);
    const unsigned long long t2 = C8_T();
    if constexpr (!(ABL & 32)) __syncthreads();
    C8_PIN(7);                                             // behind the step's barrier
    // peephole / bias gradient sums: off the critical path, behind the barrier
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      sums[0] += zi[r] * cprev[r]; sums[1] += zf[r] * cprev[r]; sums[2] += zo[r] * curv[r];
      sums[3] += zi[r]; sums[4] += zg[r]; sums[5] += zf[r]; sums[6] += zo[r];
    }
    C8_PIN(8);                                             // behind the gradient sums
    // ---- 5. partial dh_prev from the own dG slice; own tile stays, foreign tiles are published
    if (s > 0) {
      bf16x8_t afr[KC];
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        if constexpr ((ABL & 2) != 0) afr[kc] = wf[0][kc];
        else afr[kc] = *reinterpret_cast<const bf16x8_t*>(smem + P * DGB + lrd + kc * 64);
      }
      __builtin_amdgcn_sched_barrier(0);
      const unsigned tag = (((unsigned)it >> 1) + 1u) & 1u;
      auto tagged = [&](const f32x4_t& a) {
        f32x4_t o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __uint_as_float((__float_as_uint(a[i]) & ~1u) | tag);
        return o;
      };
      // one foreign tile's partial (4 rows of one unit per lane) to its destination
      auto publish = [&](int nt, const f32x4_t& tv, auto FAST) {
        constexpr bool F = decltype(FAST)::value;
        const int dst = nt / TPC, tile = nt % TPC;
        if constexpr ((ABL & 128) != 0) {
          asm volatile("" ::"v"(tv));
        } else if constexpr (XP) {
          // Compiler-issued buffer stores, NOT inline asm with an SGPR base: with 16 slot bases per step (H = 512) the
          // bases are spilled to VGPR lanes and restored by v_readlane right in front of the store, and a VALU-written
          // SGPR needs 5 wait states before a VMEM instruction may use it as its address -- a hazard the compiler
          // handles for its own instructions but cannot see inside an asm block (measured: wild stores, memory fault).
          typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
          const int k = g - (g > dst ? 1 : 0);
          const unsigned so0 = pslot(P, dst, tile, 0, k >> 1) * 16u + (unsigned)(k & 1) * 8u;
          const unsigned so1 = pslot(P, dst, tile, 1, k >> 1) * 16u + (unsigned)(k & 1) * 8u;
          const u32x2_t lo2 = {__float_as_uint(tv[0]), __float_as_uint(tv[1])};
          const u32x2_t hi2 = {__float_as_uint(tv[2]), __float_as_uint(tv[3])};
          __builtin_amdgcn_raw_buffer_store_b64(lo2, xrs, voff16, so0, F ? 0 : 16);   // plain (stays in the L2) / sc1
          __builtin_amdgcn_raw_buffer_store_b64(hi2, xrs, voff16, so1, F ? 0 : 16);
        } else {
          xstore16(uslot(P, dst, g, tile), voff16, tv, F);
        }
      };
      // the tiles other CUs wait for go first; while they issue, this wave outranks its SIMD sibling's
      // own-tile MFMAs (nobody waits for those before the next step's gate math)
      __builtin_amdgcn_s_setprio(2);
      if constexpr (HSU == 32) {
        // One wave per SIMD: nothing fills the gaps of a tile-by-tile schedule (four DEPENDENT MFMAs into one
        // accumulator, drain, tag, a branch on the store flavour, store: ~170 cycles per tile, 9 tiles at H = 512), and
        // every destination waits for the LAST of its partials anyway.  So: all NF chains advance together (k-chunk
        // outer, tile inner: independent accumulators back to back), then the stores go out in one straight run per
        // flavour.  (The last tile of a wave that has none is computed and not stored.)
        f32x4_t af[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i) af[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
#pragma unroll
          for (int i = 0; i < NF; ++i) {
            if constexpr ((ABL & 4) != 0) af[i][0] = __uint_as_float(__float_as_uint(af[i][0]) ^ (__builtin_bit_cast(xw4_t, afr[kc])[i & 3] & 1u));
            else af[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[kc], wf[i][kc], af[i], 0, 0, 0);
          }
        if (fast) {
#pragma unroll
          for (int i = 0; i < NF; ++i)
            if (i < NF - 1 || last_f) publish(nt_f[i], tagged(af[i]), std::integral_constant<bool, true>{});
        } else {
#pragma unroll
          for (int i = 0; i < NF; ++i)
            if (i < NF - 1 || last_f) publish(nt_f[i], tagged(af[i]), std::integral_constant<bool, false>{});
        }
      } else {
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          if (OWN_ONCE ? (i < NF - 1 || last_f) : (i < NF - 1 || last_f)) {      // wave-uniform: a foreign tile
            f32x4_t af = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) af = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[kc], wf[i][kc], af, 0, 0, 0);
            if (fast) publish(nt_f[i], tagged(af), std::integral_constant<bool, true>{});
            else publish(nt_f[i], tagged(af), std::integral_constant<bool, false>{});
          }
        }
      }
      __builtin_amdgcn_s_setprio(0);
      if constexpr (OWN_ONCE) {
        if (hh == 0) {                                     // own tile, once: rows 0,1 stay, rows 2,3 -> partner
          f32x4_t ao = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kc = 0; kc < KC; ++kc) ao = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[kc], wf[NF - 1][kc], ao, 0, 0, 0);
          dhr[0] += ao[0];
          dhr[1] += ao[1];
          float* o = ownx + ((P * 4 + wt) * 64 + lane) * 2;
          o[0] = ao[2];
          o[1] = ao[3];
        }
      } else {
        f32x4_t ao = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
          if constexpr ((ABL & 4) != 0) ao[hh ? 2 : 0] = __uint_as_float(__float_as_uint(ao[hh ? 2 : 0]) ^ (__builtin_bit_cast(xw4_t, afr[kc])[0] & 1u));
          else ao = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[kc], wo[kc], ao, 0, 0, 0);
        }
        dhr[0] += hh ? ao[2] : ao[0];
        dhr[1] += hh ? ao[3] : ao[1];
      }
    }
    if constexpr (OWN_ONCE) {
      __syncthreads();                                     // hand-over visible before the partner's next step
      if (s > 0 && hh == 1) {
        const float* o = ownx + ((P * 4 + wt) * 64 + lane) * 2;
        dhr[0] += o[0];
        dhr[1] += o[1];
      }
    }
    C8_PIN(3);
    const unsigned long long t3 = C8_T();
    if (DBG) { ph[0] += t1 - t0; ph[1] += t2 - t1; ph[2] += t3 - t2; }
  };
  (void)dbg;
  // parity of iteration `it` is it & 1; iterations come in pairs from it = 0
  int s = tmax - 1;
  for (; s >= 1; s -= 2) {
    step(s, std::integral_constant<int, 0>{});
    step(s - 1, std::integral_constant<int, 1>{});
  }
  if (s == 0) step(0, std::integral_constant<int, 0>{});
#undef C8_T
#undef C8_PIN

  if (DBG && dbg && lane == 0 && cid.tile == 0 && g < 4) {
    unsigned long long* o = dbg + 768 + ((size_t)(d * 4 + g) * 8 + wave) * 8;   // [768, 1280)
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = ph[k];
    o[4] = nspin;
    o[5] = tmax;
    o[6] = fast ? 1 : 0;
    o[7] = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xFu;
  }
  if (timed_out) atomicOr(err, 2u);
  if (dpeep_part) {
    // reduce over the 4 row groups of the wave, then over the two waves (hh) that share a unit
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      sums[k] += __shfl_xor(sums[k], 16, 64);
      sums[k] += __shfl_xor(sums[k], 32, 64);
    }
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);           // [7][HSU]
    if (hh == 1 && rg == 0) {
#pragma unroll
      for (int k = 0; k < 7; ++k) red[k * HSU + ul] = sums[k];
    }
    __syncthreads();
    if (hh == 0 && rg == 0) {
      float* p = dpeep_part + ((size_t)cid.tile * ndir + d) * 7 * H;
#pragma unroll
      for (int k = 0; k < 7; ++k) p[k * H + jw] = sums[k] + red[k * HSU + ul];
    }
  }
}

static unsigned long long* g_cdbg_host = nullptr;
static void cdbg_setup() {
  static bool done = false;
  if (done) return;
  done = true;
  const char* e = getenv("ASR_LSTM_DBG");
  if (!(e && e[0] == '1')) return;
  (void)hipMalloc(&g_cdbg_host, 1280 * sizeof(unsigned long long));
  (void)hipMemset(g_cdbg_host, 0, 1280 * sizeof(unsigned long long));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_cdbg), &g_cdbg_host, sizeof(g_cdbg_host));
}
}  // namespace

template <int H, int HSU = 64>
static bool cluster_fwd_launch(asr_handle* h, int T, int B, int ndir, const float* xproj, const void* whp,
                               const float* peep, const int32_t* seq_len, float fb, float clip, void* gates,
                               void* hout, float* cs, float* cf, float* hf, hipStream_t st, bool grouped) {
  constexpr int G = H / HSU;
  static_assert(G <= XHDR, "placement header too small");
  constexpr size_t cl_bytes = (XHDR + 2 * G * 16 * (HSU / 2)) * sizeof(u64);
  const ClusterCall cc = cluster_call(h, G, ndir, B, (size_t)T * B * ndir * H, cl_bytes, grouped);
  if (!cc.plan.n) return false;
  // EARLY (own-slice k-chunks multiplied under the L2 hop): measured at H = 256 (round 2, cfg B): 970 -> 938 us per
  // launch, at H = 320: 1069 -> 969; default at both.  ASR_LSTM_DFLAGS bit 5 (32) inverts the default for A/B measurements.
  const bool early = (H == 256 || H == 320 || HSU == 32) != ((dbg_flags() & 32) != 0);   // H = 320: 1069 -> 969 us per launch
  // forward all-gather in 4-byte self-tagged words (default) or 8-byte {step, payload} granules (ASR_LSTM_XW=0, flag bit 10)
  const bool xw = fwd_xw_enabled();
  auto k = g_cdbg_host ? (xw ? lstm_fwd_cluster8_kernel<H, true, false, HSU, 0, true> : lstm_fwd_cluster8_kernel<H, true, false, HSU, 0, false>)
                       : (early ? (xw ? lstm_fwd_cluster8_kernel<H, false, true, HSU, 0, true> : lstm_fwd_cluster8_kernel<H, false, true, HSU, 0, false>)
                                : (xw ? lstm_fwd_cluster8_kernel<H, false, false, HSU, 0, true> : lstm_fwd_cluster8_kernel<H, false, false, HSU, 0, false>));
  // scheduling barrier between the MFMA phase and the gate math (FPIN bit 1) at H = 256 on four waves; masks measured
  // there (us per launch): none 806, {0} 808, {1} 777, {2} 855, {3} 808, {0,1} 779, {1,2} 799, all 808; at H = 512 every mask
  // is slower than none (1350: 1355 .. 1399), and so is this one at H = 320 on eight waves (968 -> 984).  On top of {1}:
  // a second barrier behind the gate math (bit 5) 781 -> 776; behind the DPP half swap (bit 4) 850, behind the publish
  // (bit 6) 799, behind the poll loop (bit 7) 797, behind the LDS staging (bit 8) 797.  H = 512 with bit 5 / 6 / 7 alone:
  // 1365 / 1369 / 1391 against 1356
  if constexpr (HSU == 32 && H == 256) {
    if (early && !g_cdbg_host)
      k = xw ? lstm_fwd_cluster8_kernel<H, false, true, HSU, 2 | 32, true> : lstm_fwd_cluster8_kernel<H, false, true, HSU, 2 | 32, false>;
#ifdef ASR_LSTM_ABLATE
    // scripts/probe_lstm_ablate.py: ASR_LSTM_ABL_FWD selects an ablated build of the headline kernel (garbage results)
    if (const char* e = getenv("ASR_LSTM_ABL_FWD")) {
      switch (atoi(e)) {
#define ABLF(n) case n: k = lstm_fwd_cluster8_kernel<H, false, true, HSU, 2 | 32, true, n>; break;
        ABLF(1) ABLF(2) ABLF(4) ABLF(8) ABLF(16) ABLF(32) ABLF(64) ABLF(128) ABLF(256) ABLF(512)
        ABLF(513) ABLF(515) ABLF(519) ABLF(527) ABLF(545) ABLF(769) ABLF(1023) ABLF(6) ABLF(14) ABLF(48) ABLF(800)
#undef ABLF
        default: break;
      }
    }
#endif
  }
#ifdef ASR_LSTM_ABLATE
  if constexpr (HSU == 32 && H == 512) {                   // the width of cfg C / D / E: a shorter list
    if (const char* e = getenv("ASR_LSTM_ABL_FWD")) {
      if (early && xw && !g_cdbg_host) {
        switch (atoi(e)) {
#define ABLF(n) case n: k = lstm_fwd_cluster8_kernel<H, false, true, HSU, 0, true, n>; break;
          ABLF(1) ABLF(8) ABLF(16) ABLF(64) ABLF(512) ABLF(6) ABLF(513) ABLF(519) ABLF(527) ABLF(545) ABLF(1023)
#undef ABLF
          default: break;
        }
      }
    }
  }
#endif
  // (padding the LDS request past half a CU so that two 4-wave members can never share one was measured: no
  // difference, 866.7 vs 867.6 us -- the dispatcher spreads the members over the CUs by itself)
  const size_t lds = (size_t)2 * 16 * (H + 8) * 2;
  run_tile_groups(h, cc, B, ndir, cl_bytes, st, 0, [&](const XchAreas& xa, int ncl, int t0, int nt) {
    hipLaunchKernelGGL(k, dim3(cluster_grid(G, ncl)), dim3(HSU * 8), lds, st, T, B, ndir,
                       (const f32x4_t*)xproj, (const bf16_t*)whp, peep, seq_len, fb, clip, (cbf16x4_t*)gates,
                       (bf16_t*)hout, cs, cf, hf, xa.area, (unsigned*)cc.base, kernel_flags(), xa.znext, xa.zwords, t0, nt);
  });
  h->lstm_counts[HSU == 32 ? ASR_LSTM_FWD_BF16_HS32 : ASR_LSTM_FWD_BF16_HS64] += 1;   // asr_lstm_kernel_counts
  return true;
}

// H = 256 on clusters of 16 CUs x four waves x 4 units (lstm_fwd_cluster16_kernel).  4-byte exchange words only: with
// ASR_LSTM_XW=0 / flag bit 10, or the phase timers on, the caller goes on to the 32-unit form.
static bool cluster_fwd16_launch(asr_handle* h, int T, int B, int ndir, const float* xproj, const void* whp,
                                 const float* peep, const int32_t* seq_len, float fb, float clip, void* gates,
                                 void* hout, float* cs, float* cf, float* hf, hipStream_t st, bool grouped) {
  constexpr int H = 256, HSU = 16, G = H / HSU;
  static_assert(G <= XHDR, "placement header too small");
  constexpr size_t cl_bytes = (XHDR + 2 * G * 16 * (HSU / 2)) * sizeof(u64);
  if (!fwd_xw_enabled() || g_cdbg_host) return false;
  const ClusterCall cc = cluster_call(h, G, ndir, B, (size_t)T * B * ndir * H, cl_bytes, grouped);
  if (!cc.plan.n) return false;
  // scheduling-barrier mask (FPIN, the points of the forms above), searched over the same eight masks as the 8-CU form; us
  // per launch at T = 745, B = 16, two directions, two passes (median of 12 launches each): none 621 / 621, {0} 617 / 620,
  // {1} 626 / 628, {2} 619 / 620, {3} 622 / 623, {0,1} 627 / 625, {1,2} 625 / 624, all four 630 / 628; also {5} 620 / 616 and
  // the 8-CU form's {1,5} 623 / 622.  The barrier between the MFMAs and the gate math (bit 1), which that form gains 29 us
  // from, costs this one 4 - 8 us wherever it appears; the masks without it lie within the 5 us the passes differ by.
  // {0} (nothing moves across the step boundary) is kept: profiles/r10_fwd_cu16.md.
  auto k = lstm_fwd_cluster16_kernel<1>;
#ifdef ASR_LSTM_ABLATE
  // scripts/probe_lstm_ablate.py: ASR_LSTM_FPIN_FWD picks one of the searched masks, ASR_LSTM_ABL_FWD an ablated build
  if (const char* e = getenv("ASR_LSTM_FPIN_FWD")) {
    switch (atoi(e)) {
#define FPINF(n) case n: k = lstm_fwd_cluster16_kernel<n>; break;
      FPINF(0) FPINF(1) FPINF(2) FPINF(4) FPINF(8) FPINF(3) FPINF(6) FPINF(15) FPINF(34) FPINF(32)
#undef FPINF
      default: break;
    }
  }
  if (const char* e = getenv("ASR_LSTM_ABL_FWD")) {
    switch (atoi(e)) {
#define ABLF(n) case n: k = lstm_fwd_cluster16_kernel<1, n>; break;
      ABLF(1) ABLF(2) ABLF(4) ABLF(8) ABLF(16) ABLF(32) ABLF(64) ABLF(128) ABLF(256) ABLF(512)
      ABLF(513) ABLF(515) ABLF(519) ABLF(527) ABLF(545) ABLF(769) ABLF(1023) ABLF(6) ABLF(14) ABLF(48) ABLF(800)
#undef ABLF
      default: break;
    }
  }
#endif
  const size_t lds = (size_t)2 * 16 * (H + 8) * 2;
  run_tile_groups(h, cc, B, ndir, cl_bytes, st, 0, [&](const XchAreas& xa, int ncl, int t0, int nt) {
    hipLaunchKernelGGL(k, dim3(cluster_grid(G, ncl)), dim3(256), lds, st, T, B, ndir,
                       (const f32x4_t*)xproj, (const bf16_t*)whp, peep, seq_len, fb, clip, (cbf16x4_t*)gates,
                       (bf16_t*)hout, cs, cf, hf, xa.area, (unsigned*)cc.base, kernel_flags(), xa.znext, xa.zwords, t0, nt);
  });
  h->lstm_counts[ASR_LSTM_FWD_BF16_CU16] += 1;   // asr_lstm_kernel_counts
  return true;
}

bool asr_cluster_fwd_try(asr_handle* h, int T, int B, int H, int ndir, const float* xproj,
                         const void* whp, const float* peep, const int32_t* seq_len, float fb,
                         float clip, void* gates, void* hout, float* cs, float* cf, float* hf,
                         hipStream_t st) {
  if (!cluster_enabled() || (H != 256 && H != 512 && !(H == 320 && cluster_320_enabled()))) return false;
  cdbg_setup();
  return one_launch_else_groups([&](bool grouped) -> bool {
    if (H == 320) return cluster_fwd_launch<320>(h, T, B, ndir, xproj, whp, peep, seq_len, fb, clip, gates, hout, cs, cf, hf, st, grouped);
    // H = 256: the 16-CU form when it fits in one launch (a batch of more tiles runs as tile groups of the 32-unit form)
    if (H == 256 && !grouped && fwd256_units_per_cu() == 16 &&
        cluster_fwd16_launch(h, T, B, ndir, xproj, whp, peep, seq_len, fb, clip, gates, hout, cs, cf, hf, st, false))
      return true;
    if (fwd_units_per_cu() == 32) {
      const bool ok = H == 512
          ? cluster_fwd_launch<512, 32>(h, T, B, ndir, xproj, whp, peep, seq_len, fb, clip, gates, hout, cs, cf, hf, st, grouped)
          : cluster_fwd_launch<256, 32>(h, T, B, ndir, xproj, whp, peep, seq_len, fb, clip, gates, hout, cs, cf, hf, st, grouped);
      if (ok) return true;
    }
    return H == 512 ? cluster_fwd_launch<512>(h, T, B, ndir, xproj, whp, peep, seq_len, fb, clip, gates, hout, cs, cf, hf, st, grouped)
                    : cluster_fwd_launch<256>(h, T, B, ndir, xproj, whp, peep, seq_len, fb, clip, gates, hout, cs, cf, hf, st, grouped);
  });
}

template <int H, int HSU = 64>
static bool cluster_bwd_launch(asr_handle* h, int T, int B, int ndir, const float* dhout, const void* gates,
                               const float* cs, const void* whpb, const float* peep, const int32_t* seq_len,
                               const float* dcf, const float* dhf, void* dgates, float* dpeep_part,
                               hipStream_t st, bool grouped) {
  constexpr int G = H / HSU;
  static_assert(G <= XHDR, "placement header too small");
  constexpr size_t cl_bytes = (XHDR + (size_t)2 * G * G * (HSU / 16) * 64 * 2) * sizeof(u64);
  const ClusterCall cc = cluster_call(h, G, ndir, B, (size_t)T * B * ndir * H, cl_bytes, grouped);
  if (!cc.plan.n) return false;
  // two dG images; the H = 512 form adds the own-tile hand-over buffer behind them
  const size_t lds = (size_t)2 * 16 * (4 * HSU + 8) * 2 + ((G == 8 && HSU == 64) ? 2 * 4 * 64 * 8 : 0);
  // reduce-scatter slots in the consumer-major paired layout (default) or one 16-byte slot per (source, tile) (ASR_LSTM_XP=0)
  const bool xp = bwd_xp_enabled(HSU);
  auto k = g_cdbg_host ? (xp ? lstm_bwd_cluster8_kernel<H, true, HSU, -1, true> : lstm_bwd_cluster8_kernel<H, true, HSU, -1, false>)
                       : (xp ? lstm_bwd_cluster8_kernel<H, false, HSU, -1, true> : lstm_bwd_cluster8_kernel<H, false, HSU, -1, false>);
  if (h->bptt_clip > 0.f)   // asr_lstm_bwd_ex: the gradient-blocking clip of the projected LSTMCell layers
    k = xp ? lstm_bwd_cluster8_kernel<H, false, HSU, -1, true, 0, true> : lstm_bwd_cluster8_kernel<H, false, HSU, -1, false, 0, true>;
#ifdef ASR_LSTM_ABLATE
  if constexpr (HSU == 32 && H == 512) {
    if (const char* e = getenv("ASR_LSTM_ABL_BWD")) {
      switch (atoi(e)) {
#define ABLB(n) case n: k = lstm_bwd_cluster8_kernel<H, false, HSU, -1, false, n>; break;
        ABLB(1) ABLB(8) ABLB(64) ABLB(128) ABLB(512) ABLB(6) ABLB(513) ABLB(519) ABLB(527) ABLB(545) ABLB(641) ABLB(1023)
#undef ABLB
        default: break;
      }
    }
  }
  if constexpr (HSU == 32 && H == 256) {
    if (const char* e = getenv("ASR_LSTM_ABL_BWD")) {
      switch (atoi(e)) {
#define ABLB(n) case n: k = lstm_bwd_cluster8_kernel<H, false, HSU, -1, false, n>; break;
        ABLB(1) ABLB(2) ABLB(4) ABLB(8) ABLB(16) ABLB(32) ABLB(64) ABLB(128) ABLB(256) ABLB(512)
        ABLB(513) ABLB(515) ABLB(519) ABLB(527) ABLB(545) ABLB(641) ABLB(1023) ABLB(6) ABLB(14) ABLB(144) ABLB(80)
#undef ABLB
        default: break;
      }
    }
  }
#endif
  run_tile_groups(h, cc, B, ndir, cl_bytes, st, 0, [&](const XchAreas& xa, int ncl, int t0, int nt) {
    hipLaunchKernelGGL(k, dim3(cluster_grid(G, ncl)), dim3(HSU * 8), lds, st, T, B, ndir, dhout,
                       (const cbf16x4_t*)gates, cs, (const bf16_t*)whpb, peep, seq_len, dcf, dhf,
                       (cbf16x4_t*)dgates, dpeep_part, xa.area, (unsigned*)cc.base, kernel_flags(), xa.znext, xa.zwords,
                       h->bptt_clip, t0, nt);
  });
  h->lstm_counts[HSU == 32 ? ASR_LSTM_BWD_BF16_HS32 : ASR_LSTM_BWD_BF16_HS64] += 1;   // asr_lstm_kernel_counts
  return true;
}

bool asr_cluster_bwd_try(asr_handle* h, int T, int B, int H, int ndir, const float* dhout,
                         const void* gates, const float* cs, const void* whpb, const float* peep,
                         const int32_t* seq_len, const float* dcf, const float* dhf, void* dgates,
                         float* dpeep_part, hipStream_t st) {
  if (!cluster_enabled() || (H != 256 && H != 512 && !(H == 320 && cluster_320_enabled()))) return false;
  cdbg_setup();
  return one_launch_else_groups([&](bool grouped) -> bool {
    if (H == 320)
      return cluster_bwd_launch<320>(h, T, B, ndir, dhout, gates, cs, whpb, peep, seq_len, dcf, dhf, dgates, dpeep_part, st, grouped);
    if (bwd_units_per_cu() == 32) {
      // (falls through to the 64-unit form when the exchange area of the wider clusters does not fit)
      const bool ok = H == 512
          ? cluster_bwd_launch<512, 32>(h, T, B, ndir, dhout, gates, cs, whpb, peep, seq_len, dcf, dhf, dgates, dpeep_part, st, grouped)
          : cluster_bwd_launch<256, 32>(h, T, B, ndir, dhout, gates, cs, whpb, peep, seq_len, dcf, dhf, dgates, dpeep_part, st, grouped);
      if (ok) return true;
    }
    return H == 512 ? cluster_bwd_launch<512>(h, T, B, ndir, dhout, gates, cs, whpb, peep, seq_len, dcf, dhf, dgates, dpeep_part, st, grouped)
                    : cluster_bwd_launch<256>(h, T, B, ndir, dhout, gates, cs, whpb, peep, seq_len, dcf, dhf, dgates, dpeep_part, st, grouped);
  });
}

extern "C" int asr_debug_cluster_cycles(unsigned long long* out, int n) {
  if (!g_cdbg_host || n > 1280) return -1;
  return hipMemcpy(out, g_cdbg_host, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
