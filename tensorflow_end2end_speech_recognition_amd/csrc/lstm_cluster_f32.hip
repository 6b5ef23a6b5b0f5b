// LSTM recurrence on clusters of CUs with fp32 operands: one forward and one BPTT kernel over an operand policy
// (cluster_split3.h) -- OpF32, the exact fp32 MFMA, or OpSplit3, the three-term bf16 split -- and the BPTT of 64 units per CU.
// The cluster scheme is told in lstm_cluster.hip; shared parts: cluster_xch.h, cluster_launch.h.
#include "cluster_launch.h"
#include "cluster_split3.h"
#include <type_traits>

namespace {
// ---------------------------------------------------------------- fp32 operands
// (Written for H = 128 on two CUs with the exact fp32 MFMA, as told below.  Served today, asr_cluster_fwd_f32_try /
// asr_cluster_bwd_f32_try: lstm_fwd_cluster_f32_kernel and lstm_bwd_cluster_f32_kernel at 32 units per CU for H = 128, 256,
// 320, 512 -- under OpSplit3 at 128 and 256, under OpF32 at 320 and 512 and, when the three-term split is off (forward: or
// T >= 65536), at 128 and 256 as well; at 64 units per CU, H = 128 alone: the forward kernel under OpF32 and a BPTT of its
// own, lstm_bwd_cluster8_f32_kernel.  With 64 units per CU requested (ASR_LSTM_HS=64 / flag bit 9) the fp32 widths above
// 128 have no cluster form and run on the single-CU kernels.)
// BASELINE configs[0] (2 x 128 BLSTM-CTC, fp32) ran on the single-CU kernels of lstm.hip at 5.1 / 6.7 us per
// recurrence step: with fp32 operands the step is bound by the CU's fp32 matrix rate (v_mfma_f32_16x16x4_f32:
// 256 flop/clk/CU; h W_h of one step = 2.1 Mflop = 8.2 k cycles), not by streaming W_h.  The same cluster scheme
// halves that: G = H/64 = 2 CUs per (direction, tile), 64 units per CU, and the byte layouts of the bf16 H = 256
// form carry over unchanged (a row of h is 128 fp32 = 512 B, a fragment 16 B per lane, 8 fragments per tile, W_h
// slice in 64 VGPRs per wave).  What differs: four K = 4 MFMAs per fragment, one {tag, fp32} granule per (row,
// unit) pair in the all-gather (two per lane) instead of one {tag, 2 x bf16}, saved activations in fp32.

// LDS of a launch, which the kernels take their image strides from as well: forward two images (parity) of h [16][H],
// BPTT two of the CU's slice of dG [16][4 HSU] and the hand-over buffer [2 parity][HSU / 16 tiles][64 lanes] x (row 2, row 3)
template <class OP> constexpr size_t fwd_f32_lds_bytes(int H) { return (size_t)2 * op_image_bytes<OP>(H); }
template <class OP> constexpr size_t bwd_f32_lds_bytes(int HSU) {
  return (size_t)2 * op_image_bytes<OP>(4 * HSU) + (size_t)2 * (HSU / 16) * 64 * 8;
}

// EARLY: as in the bf16 kernel, the fragments of the CU's OWN slice of h (half of K with two CUs) are multiplied for
// step s+1 right after they are written, before the wave starts polling for the peer's half.
// HSU = units per CU: 64 (eight waves) or 32 (four waves, one per SIMD: twice the CUs, each wave alone on its SIMD's fp32
// matrix pipe -- the step is bound by that pipe: 2 waves x 64 K=4 MFMAs x 32 cycles per SIMD in the 8-wave form).
template <int H, bool EARLY, int HSU, class OP>
__global__ __launch_bounds__(HSU * 8, 1) void lstm_fwd_cluster_f32_kernel(
    int T_, int B_, int ndir, const f32x4_t* __restrict__ xg, const float* __restrict__ whp,
    const float* __restrict__ peep, const int32_t* __restrict__ seq_len, float forget_bias,
    float cell_clip, f32x4_t* __restrict__ gates, float* __restrict__ hout, float* __restrict__ cs,
    float* __restrict__ c_final, float* __restrict__ h_final, u64* __restrict__ xch,
    unsigned* __restrict__ err, int kflags, u64* __restrict__ znext, unsigned zwords, int tile0, int ntl) {
  zero_next_area(znext, zwords);
  constexpr int G = H / HSU;
  constexpr int CTW = HSU * 8;
  static_assert(OP::TERMS == 1 || (HSU == 32 && (H & (H - 1)) == 0), "split: four waves per CU, power-of-two width");
  constexpr int KS = H / OP::K;                            // fragments of k = OP::K
  constexpr int KS16 = H / 16;                             // fragments of the fp32 weight packing
  constexpr int LDH = op_ld<OP>(H);                        // elements per image row (an odd number of 16-byte slots)
  constexpr int ESZ = sizeof(typename OP::elem);
  constexpr int PLB = op_term_bytes<OP>(H);                // bytes of one term image
  constexpr int HB = op_image_bytes<OP>(H);                // bytes of one image of h
  constexpr int SLICE = 16 * HSU;                           // granules one CU publishes per step
  constexpr int KO = HSU / OP::K;                           // fragments of one CU's own slice
  // fragment index modulo KS (a mask where KS is a power of two; H = 320 has 20 fragments: x < 2 KS there)
  auto krotf = [](int x) -> int { return ((KS & (KS - 1)) == 0) ? (x & (KS - 1)) : (x >= KS ? x - KS : x); };
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typename OP::elem* hs = reinterpret_cast<typename OP::elem*>(smem);   // [2 parity][TERMS][16][LDH]

  const ClusterId cid = cluster_id<G>(ndir, tile0, ntl);
  if (!cid.valid) return;
  const int g = cid.g, d = cid.d, b0 = cid.tile * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, rg = lane >> 4;
  const bool lo = col < 8;
  const bool rev = (d == 1);
  const float* wp = whp + (size_t)d * H * 4 * H;
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

  for (int i = threadIdx.x; i < 2 * OP::TERMS * 16 * LDH; i += CTW) hs[i] = 0;
  // B fragments out of the standard fp32 forward packing (lstm.hip prep: tile = (unit/16)*4 + gate, fragment of k = 16, lane
  // (n, rg) holds k = 16 frag + 4 rg + e; the split re-cuts it into k = 32 chunks of three terms): this lane's column of
  // tile p is (gate p*2 + (col>>3), unit jw)
  typename OP::frag wreg[2][KS];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int tile = (jw >> 4) * 4 + p * 2 + (col >> 3);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int kk = EARLY ? krotf(ks + g * KO) : ks;            // EARLY: register fragment ks holds k-fragment kk
      OP::load_b(wp, (size_t)tile * KS16, kk, rg, jw & 15, wreg[p][ks]);
    }
  }

  u64* xhdr = xch + (size_t)cid.c * (XHDR + 2 * G * SLICE);
  u64* xbase = xhdr + XHDR;                                // [2 parity][G][8 waves][16 rows][8 units]
  bool timed_out = false;
  const bool colocated = same_xcd<G>(xhdr, g, timed_out);
  const bool fast = colocated && !(kflags & 1);
  unsigned spin_limit = (kflags & 2) ? 2000u : SPIN_LIMIT;
  if ((kflags & 2) && g == G - 1) return;                  // TEST ONLY: a member goes missing
  __syncthreads();

  const unsigned stride = (unsigned)B_ * ndir * H;
  const unsigned dstep = rev ? 0u - stride : stride;
  unsigned oa[2], os[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    os[r] = ((unsigned)(b0 + rbase + r) * ndir + d) * H + jw;
    oa[r] = os[r] + (rev ? (unsigned)max(len[r] - 1, 0) * stride : 0u);
  }
  // granule i of a wave's 128: row i >> 3, unit i & 7.  A lane publishes its two (row, unit) pairs and polls
  // granules lane and 64 + lane of wave `wave` of every peer.
  const unsigned pofs = (unsigned)(wave * 128 + rbase * 8 + (col & 7));
  const unsigned lofs = (unsigned)(wave * 128 + lane);
  unsigned ldst[G - 1][2];                                 // byte offsets inside one h buffer
  auto slice = [&](int P, int gg) -> u64* { return xbase + ((size_t)P * G + gg) * SLICE; };
#pragma unroll
  for (int k = 0; k < G - 1; ++k) {
    const int gsrc = k + (k >= g ? 1 : 0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = j * 8 + (lane >> 3);
      ldst[k][j] = ((unsigned)(row * LDH + gsrc * HSU + wave * 8 + (lane & 7)) * (unsigned)ESZ) ^ lds_swz(row);
    }
  }
  unsigned lown[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) lown[r] = ((unsigned)((rbase + r) * LDH + g * HSU + ul) * (unsigned)ESZ) ^ lds_swz(rbase + r);
  const unsigned lrd = ((unsigned)(col * LDH + rg * (OP::K / 4)) * (unsigned)ESZ) ^ lds_swz(col);

  // rows past their length: saved activations never read, x-projection rows not used -> under OP::PARK ONE parked position
  // per row (its frame tmax - 1) that stays in the L2 instead of streaming the padded part of the batch through HBM (see the
  // bf16 kernel); else the padded frame of the step
  unsigned opark[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) opark[r] = os[r] + (unsigned)max(tmax - 1, 0) * stride;
  f32x4_t xq[2][2];                                        // x projection rows, requested two steps ahead
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    xq[0][r] = xg[(0 < len[r]) ? oa[r] : OP::PARK ? opark[r] : os[r]];
    xq[1][r] = (tmax > 1) ? xg[(1 < len[r]) ? oa[r] + dstep : OP::PARK ? opark[r] : os[r] + stride] : xq[0][r];
  }
  f32x4_t accn0 = {0.f, 0.f, 0.f, 0.f}, accn1 = {0.f, 0.f, 0.f, 0.f};   // EARLY: own-slice part of the next step

  auto step = [&](int s, auto PAR) {
    constexpr int P = decltype(PAR)::value;
    const char* hcur = smem + P * HB;
    char* hnxt = smem + (1 - P) * HB;
    const f32x4_t x0 = xq[P][0], x1 = xq[P][1];
    if (s + 2 < tmax) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
        xq[P][r] = xg[(s + 2 < len[r]) ? oa[r] + 2u * dstep : OP::PARK ? opark[r] : os[r] + 2u * stride];
    }
    f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EARLY) { acc0 = accn0; acc1 = accn1; }    // own-slice fragments: done at the end of the last step
    {
      constexpr int K0 = EARLY ? KO : 0;
      if constexpr (KS <= 16) {
        typename OP::frag afr[KS];
#pragma unroll
        for (int ks = K0; ks < KS; ++ks) OP::load_a(hcur + lrd + (EARLY ? krotf(ks + g * KO) : ks) * 64, PLB, afr[ks]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = K0; ks < KS; ++ks) OP::mma2(afr[ks], wreg[0][ks], wreg[1][ks], acc0, acc1);
      } else {                                             // H >= 320 (exact): the weights hold 160+ registers; A in runs of 8
#pragma unroll
        for (int kb = K0; kb < KS; kb += 8) {
          typename OP::frag afr[8];
#pragma unroll
          for (int ks = 0; ks < 8; ++ks)
            if (kb + ks < KS) OP::load_a(hcur + lrd + (EARLY ? krotf(kb + ks + g * KO) : kb + ks) * 64, PLB, afr[ks]);
#pragma unroll
          for (int ks = 0; ks < 8; ++ks)
            if (kb + ks < KS) OP::mma2(afr[ks], wreg[0][kb + ks], wreg[1][kb + ks], acc0, acc1);
        }
      }
    }
    float pi[2], pq[2], pf[2], po[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      pi[r] = dpp_ror8_into<0xC>(acc0[r], acc0[2 + r]);
      pq[r] = dpp_ror8_into<0x3>(acc0[2 + r], acc0[r]);
      pf[r] = dpp_ror8_into<0xC>(acc1[r], acc1[2 + r]);
      po[r] = dpp_ror8_into<0x3>(acc1[2 + r], acc1[r]);
    }
    const unsigned epoch = (unsigned)s + 1u;
    bool act[2];
    float ig[2], gg[2], fg[2], og[2], cn[2], hn[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) act[r] = s < len[r];
    const f32x4_t xr[2] = {x0, x1};
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
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      c[r] = act[r] ? cn[r] : c[r];
      hr[r] = act[r] ? hn[r] : hr[r];
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      unsigned ghi, glo;
      OP::encode(hr[r], epoch, ghi, glo);
      gpublish(uoff(slice(P, g), pofs + 8u * r), ghi, glo, fast);
      OP::stage(hnxt, PLB, lown[r], glo, ghi);
    }
    unsigned offs[2], offgs[2];                            // hout position / saved-activation position
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      offs[r] = act[r] ? oa[r] : os[r];
      offgs[r] = act[r] ? oa[r] : OP::PARK ? opark[r] : os[r];
      oa[r] += dstep;
      os[r] += stride;
    }
    if constexpr (EARLY) {
      if (s + 1 < tmax) {                                  // block-uniform
        __syncthreads();                                   // the CU's own slice of h(s) is complete in hnxt
        typename OP::frag ao[KO];
#pragma unroll
        for (int k = 0; k < KO; ++k) OP::load_a(hnxt + lrd + krotf(k + g * KO) * 64, PLB, ao[k]);
        accn0 = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        accn1 = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KO; ++k) OP::mma2(ao[k], wreg[0][k], wreg[1][k], accn0, accn1);
      }
    }
    {
      u64 v[G - 1][2];
#pragma unroll
      for (int k = 0; k < G - 1; ++k)
#pragma unroll
        for (int j = 0; j < 2; ++j) v[k][j] = gload(uoff(slice(P, k + (k >= g ? 1 : 0)), lofs + 64u * j));
      unsigned spins = 0;
#pragma unroll 1
      for (;;) {                                           // wave-uniform loop: no exec masking
        bool ok = true;
#pragma unroll
        for (int k = 0; k < G - 1; ++k)
#pragma unroll
          for (int j = 0; j < 2; ++j) ok = ok && OP::tagged(v[k][j], epoch);
        if (__all(ok)) break;
        if (++spins > spin_limit) { timed_out = true; spin_limit = 0; break; }
#pragma unroll
        for (int k = 0; k < G - 1; ++k)
#pragma unroll
          for (int j = 0; j < 2; ++j) v[k][j] = gload(uoff(slice(P, k + (k >= g ? 1 : 0)), lofs + 64u * j));
      }
#pragma unroll
      for (int k = 0; k < G - 1; ++k)
#pragma unroll
        for (int j = 0; j < 2; ++j) OP::stage(hnxt, PLB, ldst[k][j], (unsigned)v[k][j], (unsigned)(v[k][j] >> 32));
    }
    // saved activations behind the poll loop (loads and stores share the wave's in-order counter); rows past their
    // length write frame s of the padding (hout: zeros; gates / cs: never read there)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      hout[offs[r]] = act[r] ? hr[r] : 0.f;
      gates[offgs[r]] = (f32x4_t){ig[r], gg[r], fg[r], og[r]};
      cs[offgs[r]] = cn[r];
    }
    __syncthreads();
  };
  int s = 0;
  for (; s + 1 < tmax; s += 2) {
    step(s, std::integral_constant<int, 0>{});
    step(s + 1, std::integral_constant<int, 1>{});
  }
  if (s < tmax) step(s, std::integral_constant<int, 0>{});

  if (timed_out) atomicOr(err, 1u);
  for (int t = tmax; t < T_; ++t)
#pragma unroll
    for (int r = 0; r < 2; ++r) { hout[os[r]] = 0.f; os[r] += stride; }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const size_t o = ((size_t)d * B_ + b0 + rbase + r) * H + jw;
    if (c_final) c_final[o] = c[r];
    if (h_final) h_final[o] = hr[r];
  }
}

// BPTT, fp32 operands: the H = 512 arrangement of the bf16 kernel (each tile computed ONCE: the hh = 0 waves take the
// four own-unit tiles and hand rows 2,3 to their hh = 1 partners through LDS, the hh = 1 waves take the four tiles of
// the peer's units and publish them) -- 64 K = 4 MFMAs per wave and step instead of the 128 + 64 of the redundant form.
template <int H>
__global__ __launch_bounds__(CT8, 1) void lstm_bwd_cluster8_f32_kernel(
    int T_, int B_, int ndir, const float* __restrict__ dhout, const f32x4_t* __restrict__ gates,
    const float* __restrict__ cs, const float* __restrict__ whpb, const float* __restrict__ peep,
    const int32_t* __restrict__ seq_len, const float* __restrict__ d_c_final,
    const float* __restrict__ d_h_final, f32x4_t* __restrict__ dgates, float* __restrict__ dpeep_part,
    u64* __restrict__ xch, unsigned* __restrict__ err, int kflags, u64* __restrict__ znext, unsigned zwords, float clipz, int tile0, int ntl) {
  static_assert(H / HS == 2, "one foreign tile per hh = 1 wave: two CUs per direction");
  zero_next_area(znext, zwords);
  constexpr int G = H / HS;
  constexpr int KC = 4 * HS / 16;            // fragments of this CU's slice of k' (16)
  constexpr int KSF = 4 * H / 16;            // fragments of the full packing
  constexpr int LDG = 4 * HS + 4;            // floats: 65 x 16 B per row
  constexpr size_t CL_U64 = XHDR + (size_t)2 * G * G * 4 * 64 * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int DGB = 16 * LDG * 4;                        // bytes per dG image

  const ClusterId cid = cluster_id<G>(ndir, tile0, ntl);
  if (!cid.valid) return;
  const int g = cid.g, d = cid.d, b0 = cid.tile * 16;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, rg = lane >> 4;
  const int hh = wave >> 2, wt = wave & 3;
  const bool rev = (d == 1);
  const float* wp = whpb + (size_t)d * H * 4 * H;
  const int ul = wt * 16 + col;
  const unsigned jw = g * HS + ul;
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

  const unsigned stride = (unsigned)B_ * ndir * H;
  const unsigned dstep = rev ? stride : 0u - stride;
  unsigned oa[2], os[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned base = ((unsigned)(b0 + rbase + r) * ndir + d) * H + jw;
    os[r] = base + (unsigned)(tmax - 1) * stride;
    oa[r] = base + (unsigned)(rev ? len[r] - tmax : tmax - 1) * stride;
  }
  {
    const f32x4_t gzero = {0.f, 0.f, 0.f, 0.f};
    for (int t = tmax; t < T_; ++t)
#pragma unroll
      for (int r = 0; r < 2; ++r) dgates[os[r] + (unsigned)(t - tmax + 1) * stride] = gzero;
  }

  float dhr[2], dcr[2], cc[2];
  float sums[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const size_t o = ((size_t)d * B_ + b0 + rbase + r) * H + jw;
    dhr[r] = d_h_final ? d_h_final[o] : 0.f;
    dcr[r] = d_c_final ? d_c_final[o] : 0.f;
    cc[r] = (tmax > 0 && tmax - 1 < len[r]) ? cs[oa[r]] : 0.f;
  }
  // this wave's tile of W_h^T (rows k' of the CU's slice): hh = 0 the own-unit tile 4g + wt, hh = 1 tile wt of the peer
  const int peer = 1 - g;
  const int nt = (hh == 0 ? g : peer) * 4 + wt;
  f32x4_t wf[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc)
    wf[kc] = *reinterpret_cast<const f32x4_t*>(wp + (((size_t)nt * KSF + g * KC + kc) * 64 + lane) * 4);
  float* ownx = reinterpret_cast<float*>(smem + 2 * DGB);  // [2 parity][4 tiles][64 lanes] x (row 2, row 3)

  u64* xhdr = xch + (size_t)cid.c * CL_U64;
  bool timed_out = false;
  const bool fast = same_xcd<G>(xhdr, g, timed_out) && !(kflags & 1);
  unsigned spin_limit = (kflags & 2) ? 2000u : SPIN_LIMIT;
  if ((kflags & 2) && g == G - 1) return;                  // TEST ONLY: a member goes missing
  f32x4_t* xs = reinterpret_cast<f32x4_t*>(xhdr + XHDR);   // [2][G dst][G src][4][64] x 16 B
  auto uslot = [&](int par, int dst, int src_, int tile) -> f32x4_t* {
    return xs + ((((size_t)par * G + dst) * G + src_) * 4 + tile) * 64;
  };
  const unsigned voff16 = (unsigned)lane * 16u;
  const unsigned pofs = (unsigned)lane * 2u + hh;          // u64 index of this lane's two rows in a slot
  const unsigned lwr[2] = {((unsigned)(rbase * LDG + ul * 4) * 4u) ^ lds_swz(rbase),
                           ((unsigned)((rbase + 1) * LDG + ul * 4) * 4u) ^ lds_swz(rbase + 1)};
  const unsigned lrd = ((unsigned)(col * LDG + rg * 4) * 4u) ^ lds_swz(col);

  f32x4_t pg[2];
  float pcp[2], pdh[2];
  auto prefetch = [&](int s_) {                            // oa/os already hold iteration s_
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const bool act = s_ < len[r];
      const bool ldp = (s_ > 0) && (s_ - 1 < len[r]);
      const unsigned offl = act ? oa[r] : os[r];
      const unsigned offn = ldp ? oa[r] + dstep : os[r];
      pg[r] = gates[offl];
      pcp[r] = cs[offn];
      pdh[r] = dhout[offl];
    }
  };
  if (tmax > 0) prefetch(tmax - 1);
  __syncthreads();

  auto step = [&](int s, auto PAR) {
    constexpr int P = decltype(PAR)::value;                // parity of THIS iteration's publish
    const int it = tmax - 1 - s;
    // ---- 1. poll for the partial the peer published at the previous iteration (parity 1-P)
    u64 pv = 0;
    if (it > 0) pv = gload(uoff(reinterpret_cast<const u64*>(uslot(1 - P, g, peer, wt)), pofs));
    // ---- 2. everything that does not need dh
    bool act[2], ldp[2];
    float gi[2], gq[2], gf[2], go[2], cprev[2], a_o[2], b_c[2], c_g[2], c_i[2], c_f[2];
    unsigned off[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      act[r] = s < len[r];
      ldp[r] = (s > 0) && (s - 1 < len[r]);
      off[r] = act[r] ? oa[r] : os[r];
      gi[r] = pg[r][0]; gq[r] = pg[r][1]; gf[r] = pg[r][2]; go[r] = pg[r][3];
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
    const float pdhv[2] = {pdh[0], pdh[1]}, pcpv[2] = {pcp[0], pcp[1]}, curv[2] = {cc[0], cc[1]};
#pragma unroll
    for (int r = 0; r < 2; ++r) { oa[r] += dstep; os[r] -= stride; }
    // ---- 3. finish the poll: both words must carry the previous iteration's tag
    if (it > 0) {
      const unsigned want = (((unsigned)(it - 1) >> 1) + 1u) & 1u;
      const u64 wmask = 0x0000000100000001ull, wtag = want ? wmask : 0ull;
      unsigned spins = 0;
#pragma unroll 1
      for (;;) {
        if (__all((pv & wmask) == wtag)) break;
        if (++spins > spin_limit) { timed_out = true; spin_limit = 0; break; }
        pv = gload(uoff(reinterpret_cast<const u64*>(uslot(1 - P, g, peer, wt)), pofs));
      }
      dhr[0] += __uint_as_float((unsigned)pv & ~1u);
      dhr[1] += __uint_as_float((unsigned)(pv >> 32) & ~1u);
    }
    // next iteration's saved activations: requested BEHIND the poll loop (see the bf16 kernel)
    if (s > 0) prefetch(s - 1);
    // ---- 4. gate gradients of the own pairs
    float zi[2], zg[2], zf[2], zo[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const float dh = pdhv[r] + dhr[r];
      const float d_o = dh * a_o[r];
      const float dct = dcr[r] + dh * b_c[r] + d_o * wco;
      const float dc = (clipz > 0.f && fabsf(curv[r]) >= clipz) ? 0.f : dct;   // asr_lstm_bwd_ex
      const float d_g = dc * c_g[r], d_i = dc * c_i[r], d_f = dc * c_f[r];
      dcr[r] = act[r] ? (dc * gf[r] + d_i * wci + d_f * wcf) : dcr[r];
      dhr[r] = act[r] ? 0.f : dhr[r];
      zi[r] = act[r] ? d_i : 0.f; zg[r] = act[r] ? d_g : 0.f;
      zf[r] = act[r] ? d_f : 0.f; zo[r] = act[r] ? d_o : 0.f;
      cc[r] = ldp[r] ? pcpv[r] : 0.f;
      const f32x4_t pk = {zi[r], zg[r], zf[r], zo[r]};
      *reinterpret_cast<f32x4_t*>(smem + P * DGB + lwr[r]) = pk;
      dgates[off[r]] = pk;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      sums[0] += zi[r] * cprev[r]; sums[1] += zf[r] * cprev[r]; sums[2] += zo[r] * curv[r];
      sums[3] += zi[r]; sums[4] += zg[r]; sums[5] += zf[r]; sums[6] += zo[r];
    }
    // ---- 5. partial dh_prev of this wave's tile from the own dG slice
    if (s > 0) {
      f32x4_t ac = {0.f, 0.f, 0.f, 0.f};
      // the tile the peer waits for outranks its SIMD sibling's own-unit tile (nobody waits for that one before the
      // next step's gate math): it is published after ~half of the SIMD's MFMA time instead of all of it
      if (hh == 1 && !(kflags & 8)) __builtin_amdgcn_s_setprio(2);
#pragma unroll
      for (int kb = 0; kb < KC; kb += 8) {
        f32x4_t afr[8];
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) afr[kc] = *reinterpret_cast<const f32x4_t*>(smem + P * DGB + lrd + (kb + kc) * 64);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) ac = mma_f32(afr[kc], wf[kb + kc], ac);
      }
      if (hh == 1) {                                       // the peer's units: publish, every word tagged
        const unsigned tag = (((unsigned)it >> 1) + 1u) & 1u;
        f32x4_t o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __uint_as_float((__float_as_uint(ac[i]) & ~1u) | tag);
        xstore16(uslot(P, peer, g, wt), voff16, o, fast);
        __builtin_amdgcn_s_setprio(0);
      } else {                                             // own units: rows 0,1 stay, rows 2,3 -> partner wave
        dhr[0] += ac[0];
        dhr[1] += ac[1];
        float* o = ownx + ((P * 4 + wt) * 64 + lane) * 2;
        o[0] = ac[2];
        o[1] = ac[3];
      }
    }
    __syncthreads();                                       // hand-over visible before the partner's next step
    if (s > 0 && hh == 1) {
      const float* o = ownx + ((P * 4 + wt) * 64 + lane) * 2;
      dhr[0] += o[0];
      dhr[1] += o[1];
    }
  };
  int s = tmax - 1;
  for (; s >= 1; s -= 2) {
    step(s, std::integral_constant<int, 0>{});
    step(s - 1, std::integral_constant<int, 1>{});
  }
  if (s == 0) step(0, std::integral_constant<int, 0>{});

  if (timed_out) atomicOr(err, 2u);
  if (dpeep_part) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      sums[k] += __shfl_xor(sums[k], 16, 64);
      sums[k] += __shfl_xor(sums[k], 32, 64);
    }
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);           // [7][HS]
    if (hh == 1 && rg == 0) {
#pragma unroll
      for (int k = 0; k < 7; ++k) red[k * HS + ul] = sums[k];
    }
    __syncthreads();
    if (hh == 0 && rg == 0) {
      float* p = dpeep_part + ((size_t)cid.tile * ndir + d) * 7 * H;
#pragma unroll
      for (int k = 0; k < 7; ++k) p[k * H + jw] = sums[k] + red[k * HS + ul];
    }
  }
}

// BPTT, fp32 operands, GENERAL form: clusters of G = H / HSU CUs (any even G), four waves per CU at HSU = 32 (one per SIMD:
// the fp32 step is bound by the SIMD's matrix pipe -- 32 cycles per K = 4 MFMA -- so a wave alone on its SIMD is what pays).
// Tile deal as in the bf16 kernel's each-tile-once arrangement: a CU owns TPC = HSU / 16 unit tiles and multiplies its dG
// slice by W_h^T for ALL H / 16 tiles; the TPC own + TPC (G - 1) foreign tiles are dealt G / 2 per wave -- an hh = 0 wave
// takes its own-unit tile (rows 2,3 handed to the hh = 1 partner through LDS) and G/2 - 1 foreign ones, an hh = 1 wave
// G / 2 foreign ones; foreign partials go out as 16-byte stores of self-tagged fp32 words, the chains of a wave's
// foreign tiles advance together and the stores follow in one run.  H = 128 runs on four CUs (the two-CU kernel above:
// 2011 us per launch at T = 778), H = 256 / 320 / 512 -- which had no fp32 cluster kernel -- on 8 / 10 / 16.
template <int H, int HSU, class OP>
__global__ __launch_bounds__(HSU * 8, 1) void lstm_bwd_cluster_f32_kernel(
    int T_, int B_, int ndir, const float* __restrict__ dhout, const f32x4_t* __restrict__ gates,
    const float* __restrict__ cs, const float* __restrict__ whpb, const float* __restrict__ peep,
    const int32_t* __restrict__ seq_len, const float* __restrict__ d_c_final,
    const float* __restrict__ d_h_final, f32x4_t* __restrict__ dgates, float* __restrict__ dpeep_part,
    u64* __restrict__ xch, unsigned* __restrict__ err, int kflags, u64* __restrict__ znext, unsigned zwords, float clipz, int tile0, int ntl) {
  zero_next_area(znext, zwords);
  constexpr int G = H / HSU;
  static_assert(G % 2 == 0 && G >= 2 && G <= XHDR, "even number of CUs per cluster");
  constexpr int TPC = HSU / 16, NWAVES = 2 * TPC;
  constexpr int KC = 4 * HSU / OP::K;        // fragments (k = OP::K) of this CU's slice of k'
  constexpr int KC16 = 4 * HSU / 16;         // ... in fragments of the fp32 weight packing
  constexpr int KSF = 4 * H / 16;            // fragments of the full packing
  constexpr int LDG = op_ld<OP>(4 * HSU);    // elements per row of a dG (term) image
  constexpr int ESZ = sizeof(typename OP::elem);
  constexpr int NF = G / 2;                  // tile slots per wave
  constexpr size_t CL_U64 = XHDR + (size_t)2 * G * G * TPC * 64 * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int PLB = op_term_bytes<OP>(4 * HSU);          // bytes of one term image
  constexpr int DGB = op_image_bytes<OP>(4 * HSU);         // bytes per dG image

  const ClusterId cid = cluster_id<G>(ndir, tile0, ntl);
  if (!cid.valid) return;
  const int g = cid.g, d = cid.d, b0 = cid.tile * 16;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, rg = lane >> 4;
  const int hh = wave / TPC, wt = wave % TPC;
  const bool rev = (d == 1);
  const float* wp = whpb + (size_t)d * H * 4 * H;
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

  const unsigned stride = (unsigned)B_ * ndir * H;
  const unsigned dstep = rev ? stride : 0u - stride;
  unsigned oa[2], os[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned base = ((unsigned)(b0 + rbase + r) * ndir + d) * H + jw;
    os[r] = base + (unsigned)(tmax - 1) * stride;
    oa[r] = base + (unsigned)(rev ? len[r] - tmax : tmax - 1) * stride;
  }
  // inactive rows read nothing that is used: under OP::PARK their fetches go to one parked position per row (frame
  // tmax - 1), else to the padded frame of the iteration
  const unsigned opark[2] = {os[0], os[1]};
  {
    const f32x4_t gzero = {0.f, 0.f, 0.f, 0.f};
    for (int t = tmax; t < T_; ++t)
#pragma unroll
      for (int r = 0; r < 2; ++r) dgates[os[r] + (unsigned)(t - tmax + 1) * stride] = gzero;
  }

  float dhr[2], dcr[2], cc[2];
  float sums[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const size_t o = ((size_t)d * B_ + b0 + rbase + r) * H + jw;
    dhr[r] = d_h_final ? d_h_final[o] : 0.f;
    dcr[r] = d_c_final ? d_c_final[o] : 0.f;
    cc[r] = (tmax > 0 && tmax - 1 < len[r]) ? cs[oa[r]] : 0.f;
  }
  // tile slots: i < NF - 1: foreign tile f = wave + NWAVES i;  slot NF - 1: hh = 0 the own tile, hh = 1 foreign tile
  // f = NWAVES (NF - 1) + wt.  Foreign index f -> destination CU (f / TPC, skipping g), its tile f % TPC.
  auto ftile = [&](int f) { const int q = f / TPC; return ((q + (q >= g ? 1 : 0)) * TPC) | (f % TPC); };
  int nt_f[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i)
    nt_f[i] = (i < NF - 1) ? ftile(wave + NWAVES * i) : (hh == 1 ? ftile(NWAVES * (NF - 1) + wt) : g * TPC + wt);
  typename OP::frag wf[NF][KC];            // W_h^T fragments (the split: re-cut into k = 32 chunks of three bf16 terms)
#pragma unroll
  for (int i = 0; i < NF; ++i)
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
      OP::load_b(wp, (size_t)nt_f[i] * KSF + g * KC16, kc, rg, col, wf[i][kc]);
  float* ownx = reinterpret_cast<float*>(smem + 2 * DGB);  // [2 parity][TPC tiles][64 lanes] x (row 2, row 3)

  u64* xhdr = xch + (size_t)cid.c * CL_U64;
  bool timed_out = false;
  const bool fast = same_xcd<G>(xhdr, g, timed_out) && !(kflags & 1);
  unsigned spin_limit = (kflags & 2) ? 2000u : SPIN_LIMIT;
  if ((kflags & 2) && g == G - 1) return;                  // TEST ONLY: a member goes missing
  f32x4_t* xs = reinterpret_cast<f32x4_t*>(xhdr + XHDR);   // [2][G dst][G src][TPC][64] x 16 B
  auto uslot = [&](int par, int dst, int src_, int tile) -> f32x4_t* {
    return xs + ((((size_t)par * G + dst) * G + src_) * TPC + tile) * 64;
  };
  const unsigned voff16 = (unsigned)lane * 16u;
  const unsigned pofs = (unsigned)lane * 2u + hh;          // u64 index of this lane's two rows in a slot
  const unsigned lwr[2] = {((unsigned)(rbase * LDG + ul * 4) * (unsigned)ESZ) ^ lds_swz(rbase),
                           ((unsigned)((rbase + 1) * LDG + ul * 4) * (unsigned)ESZ) ^ lds_swz(rbase + 1)};
  const unsigned lrd = ((unsigned)(col * LDG + rg * (OP::K / 4)) * (unsigned)ESZ) ^ lds_swz(col);

  f32x4_t pg[2];
  float pcp[2], pdh[2];
  if (tmax > 0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int s_ = tmax - 1;
      const bool act = s_ < len[r];
      const bool ldp = (s_ > 0) && (s_ - 1 < len[r]);
      pg[r] = gates[act ? oa[r] : OP::PARK ? opark[r] : os[r]];
      pcp[r] = cs[ldp ? oa[r] + dstep : OP::PARK ? opark[r] : os[r]];
      pdh[r] = dhout[act ? oa[r] : OP::PARK ? opark[r] : os[r]];
    }
  }
  __syncthreads();

  auto step = [&](int s, auto PAR) {
    // step boundary pinned (see the bf16 BPTT kernel): neutral at H = 128 / 256, 7.6 -> 4.4 ms per launch at H = 512, B = 32
    __builtin_amdgcn_sched_barrier(0);
    constexpr int P = decltype(PAR)::value;                // parity of THIS iteration's publish
    const int it = tmax - 1 - s;
    // ---- 1. polls for the partials the peers published at the previous iteration (parity 1-P)
    u64 pv[G - 1];
    if (it > 0) {
#pragma unroll
      for (int k = 0; k < G - 1; ++k)
        pv[k] = gload(uoff(reinterpret_cast<const u64*>(uslot(1 - P, g, k + (k >= g ? 1 : 0), wt)), pofs));
    }
    // ---- 2. everything that does not need dh
    bool act[2], ldp[2];
    float gi[2], gq[2], gf[2], go[2], cprev[2], a_o[2], b_c[2], c_g[2], c_i[2], c_f[2];
    unsigned off[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      act[r] = s < len[r];
      ldp[r] = (s > 0) && (s - 1 < len[r]);
      off[r] = act[r] ? oa[r] : os[r];
      gi[r] = pg[r][0]; gq[r] = pg[r][1]; gf[r] = pg[r][2]; go[r] = pg[r][3];
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
    // everything that reads the values fetched one iteration ago is pinned here, ahead of the next fetch (see the bf16 kernel)
    asm volatile("" : "+v"(pdh0), "+v"(pdh1), "+v"(pcp0), "+v"(pcp1), "+v"(cprev[0]), "+v"(cprev[1]));
    asm volatile("" : "+v"(c_g[0]), "+v"(c_g[1]), "+v"(c_i[0]), "+v"(c_i[1]), "+v"(c_f[0]), "+v"(c_f[1]));
    asm volatile("" : "+v"(a_o[0]), "+v"(a_o[1]), "+v"(b_c[0]), "+v"(b_c[1]), "+v"(gf[0]), "+v"(gf[1]));
#pragma unroll
    for (int r = 0; r < 2; ++r) { oa[r] += dstep; os[r] -= stride; }
    // ---- 3. finish the polls: every word must carry the previous iteration's tag
    if (it > 0) {
      const unsigned want = (((unsigned)(it - 1) >> 1) + 1u) & 1u;
      const u64 wmask = 0x0000000100000001ull, wtag = want ? wmask : 0ull;
      unsigned spins = 0;
#pragma unroll 1
      for (;;) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < G - 1; ++k) ok = ok && ((pv[k] & wmask) == wtag);
        if (__all(ok)) break;
        if (++spins > spin_limit) { timed_out = true; spin_limit = 0; break; }
#pragma unroll
        for (int k = 0; k < G - 1; ++k)
          pv[k] = gload(uoff(reinterpret_cast<const u64*>(uslot(1 - P, g, k + (k >= g ? 1 : 0), wt)), pofs));
      }
      float add0 = 0.f, add1 = 0.f;
#pragma unroll
      for (int k = 0; k < G - 1; ++k) {                     // fixed order
        add0 += __uint_as_float((unsigned)pv[k] & ~1u);
        add1 += __uint_as_float((unsigned)(pv[k] >> 32) & ~1u);
      }
      dhr[0] += add0;
      dhr[1] += add1;
    }
    // next iteration's saved activations: unconditional (the last iteration re-fetches its own rows) and pinned BEHIND
    // the poll loop by a compiler barrier
    {
      asm volatile("" ::: "memory");
      const bool more = s > 0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const bool actn = s - 1 < len[r];
        const bool ldpn = (s - 1 > 0) && (s - 2 < len[r]);
        const unsigned offl = more ? (actn ? oa[r] : OP::PARK ? opark[r] : os[r]) : off[r];
        const unsigned offn = more ? (ldpn ? oa[r] + dstep : OP::PARK ? opark[r] : os[r]) : off[r];
        pg[r] = gates[offl];
        pcp[r] = cs[offn];
        pdh[r] = dhout[offl];
      }
    }
    // ---- 4. gate gradients of the own pairs
    const float pdhv[2] = {pdh0, pdh1}, pcpv[2] = {pcp0, pcp1}, curv[2] = {cur0, cur1};
    float zi[2], zg[2], zf[2], zo[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const float dh = pdhv[r] + dhr[r];
      const float d_o = dh * a_o[r];
      const float dct = dcr[r] + dh * b_c[r] + d_o * wco;
      const float dc = (clipz > 0.f && fabsf(curv[r]) >= clipz) ? 0.f : dct;   // asr_lstm_bwd_ex
      const float d_g = dc * c_g[r], d_i = dc * c_i[r], d_f = dc * c_f[r];
      dcr[r] = act[r] ? (dc * gf[r] + d_i * wci + d_f * wcf) : dcr[r];
      dhr[r] = act[r] ? 0.f : dhr[r];
      zi[r] = act[r] ? d_i : 0.f; zg[r] = act[r] ? d_g : 0.f;
      zf[r] = act[r] ? d_f : 0.f; zo[r] = act[r] ? d_o : 0.f;
      cc[r] = ldp[r] ? pcpv[r] : 0.f;
      const f32x4_t pk = {zi[r], zg[r], zf[r], zo[r]};
      OP::store_a(smem + P * DGB, PLB, lwr[r], pk);
      dgates[off[r]] = pk;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      sums[0] += zi[r] * cprev[r]; sums[1] += zf[r] * cprev[r]; sums[2] += zo[r] * curv[r];
      sums[3] += zi[r]; sums[4] += zg[r]; sums[5] += zf[r]; sums[6] += zo[r];
    }
    // ---- 5. partial dh_prev of this wave's tiles from the own dG slice
    if (s > 0) {
      typename OP::frag afr[KC];
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) OP::load_a(smem + P * DGB + lrd + kc * 64, PLB, afr[kc]);
      __builtin_amdgcn_sched_barrier(0);
      f32x4_t ac[NF];
#pragma unroll
      for (int i = 0; i < NF; ++i) ac[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < KC; ++kc)
#pragma unroll
        for (int i = 0; i < NF; ++i) ac[i] = OP::mma(afr[kc], wf[i][kc], ac[i]);
      const unsigned tag = (((unsigned)it >> 1) + 1u) & 1u;
      auto tagged = [&](const f32x4_t& a) {
        f32x4_t o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __uint_as_float((__float_as_uint(a[i]) & ~1u) | tag);
        return o;
      };
      if (fast) {
#pragma unroll
        for (int i = 0; i < NF; ++i)
          if (i < NF - 1 || hh == 1) xstore16(uslot(P, nt_f[i] / TPC, g, nt_f[i] % TPC), voff16, tagged(ac[i]), true);
      } else {
#pragma unroll
        for (int i = 0; i < NF; ++i)
          if (i < NF - 1 || hh == 1) xstore16(uslot(P, nt_f[i] / TPC, g, nt_f[i] % TPC), voff16, tagged(ac[i]), false);
      }
      if (hh == 0) {                                       // own units: rows 0,1 stay, rows 2,3 -> partner wave
        dhr[0] += ac[NF - 1][0];
        dhr[1] += ac[NF - 1][1];
        float* o = ownx + ((P * TPC + wt) * 64 + lane) * 2;
        o[0] = ac[NF - 1][2];
        o[1] = ac[NF - 1][3];
      }
    }
    __syncthreads();                                       // hand-over visible before the partner's next step
    if (s > 0 && hh == 1) {
      const float* o = ownx + ((P * TPC + wt) * 64 + lane) * 2;
      dhr[0] += o[0];
      dhr[1] += o[1];
    }
  };
  int s = tmax - 1;
  for (; s >= 1; s -= 2) {
    step(s, std::integral_constant<int, 0>{});
    step(s - 1, std::integral_constant<int, 1>{});
  }
  if (s == 0) step(0, std::integral_constant<int, 0>{});

  if (timed_out) atomicOr(err, 2u);
  if (dpeep_part) {
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
}  // namespace

template <int HH, int HSU>
static bool cluster_fwd_f32_launch(asr_handle* h, int T, int B, int ndir, const float* xproj, const void* whp,
                                   const float* peep, const int32_t* seq_len, float fb, float clip, void* gates,
                                   void* hout, float* cs, float* cf, float* hf, hipStream_t st, bool grouped) {
  constexpr int G = HH / HSU;
  static_assert(G <= XHDR, "placement header too small");
  constexpr size_t cl_bytes = (XHDR + 2 * G * 16 * HSU) * sizeof(u64);
  const ClusterCall cc = cluster_call(h, G, ndir, B, (size_t)T * B * ndir * HH, cl_bytes, grouped);
  if (!cc.plan.n) return false;
  // EARLY own-slice products by default, except H = 512 where their extra live accumulators push the 256 weight
  // registers into scratch (measured 5.93 vs 5.36 ms per 778-step launch); ASR_LSTM_DFLAGS bit 5 inverts (A/B)
  const bool early = ((dbg_flags() & 32) == 0) != (HH >= 512);
  auto k = early ? lstm_fwd_cluster_f32_kernel<HH, true, HSU, OpF32> : lstm_fwd_cluster_f32_kernel<HH, false, HSU, OpF32>;
  size_t lds = fwd_f32_lds_bytes<OpF32>(HH);
  int form = HSU == 32 ? ASR_LSTM_FWD_F32_HS32 : ASR_LSTM_FWD_F32_HS64;
  if constexpr (HSU == 32 && (HH == 128 || HH == 256)) {
    if (cluster_f32_split_enabled() && T < 65536) {   // round 5: the same recurrence on the bf16 matrix pipe (three-term split; 16-bit step tags)
      k = early ? lstm_fwd_cluster_f32_kernel<HH, true, HSU, OpSplit3> : lstm_fwd_cluster_f32_kernel<HH, false, HSU, OpSplit3>;
      lds = fwd_f32_lds_bytes<OpSplit3>(HH);   // (at most 50 KB)
      form = ASR_LSTM_FWD_F32_SPLIT;
    }
  }
  if (lds > ((size_t)64 << 10))
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  run_tile_groups(h, cc, B, ndir, cl_bytes, st, 0, [&](const XchAreas& xa, int ncl, int t0, int nt) {
    hipLaunchKernelGGL(k, dim3(cluster_grid(G, ncl)), dim3(HSU * 8), lds, st, T, B, ndir, (const f32x4_t*)xproj,
                       (const float*)whp, peep, seq_len, fb, clip, (f32x4_t*)gates, (float*)hout, cs, cf, hf, xa.area,
                       (unsigned*)cc.base, kernel_flags(), xa.znext, xa.zwords, t0, nt);
  });
  h->lstm_counts[form] += 1;   // asr_lstm_kernel_counts
  return true;
}

// H = 128 / 256 / 320 / 512 on H/32 CUs x four waves, H = 128 also on two CUs x eight (the switches: cluster_host.hip)
bool asr_cluster_fwd_f32_try(asr_handle* h, int T, int B, int H, int ndir, const float* xproj,
                             const void* whp, const float* peep, const int32_t* seq_len, float fb,
                             float clip, void* gates, void* hout, float* cs, float* cf, float* hf,
                             hipStream_t st) {
#define ASR_F32_ARGS_F h, T, B, ndir, xproj, whp, peep, seq_len, fb, clip, gates, hout, cs, cf, hf, st, grouped
  return one_launch_else_groups([&](bool grouped) -> bool {
    if (!cluster_f32_enabled()) return false;
    if (fwd_units_per_cu() == 32) {
      if (H == 128) return cluster_fwd_f32_launch<128, 32>(ASR_F32_ARGS_F);
      if (!cluster_f32_wide_enabled()) return false;
      if (H == 256) return cluster_fwd_f32_launch<256, 32>(ASR_F32_ARGS_F);
      if (H == 320) return cluster_fwd_f32_launch<320, 32>(ASR_F32_ARGS_F);
      if (H == 512) return cluster_fwd_f32_launch<512, 32>(ASR_F32_ARGS_F);
      return false;
    }
    return H == 128 ? cluster_fwd_f32_launch<128, 64>(ASR_F32_ARGS_F) : false;
  });
#undef ASR_F32_ARGS_F
}

template <int HH, int HSU>
static bool cluster_bwd_f32_launch(asr_handle* h, int T, int B, int ndir, const float* dhout, const void* gates,
                                   const float* cs, const void* whpb, const float* peep, const int32_t* seq_len,
                                   const float* dcf, const float* dhf, void* dgates, float* dpeep_part, hipStream_t st,
                                   bool grouped) {
  constexpr int G = HH / HSU, TPC = HSU / 16;
  constexpr size_t cl_bytes = (XHDR + (size_t)2 * G * G * TPC * 64 * 2) * sizeof(u64);
  const ClusterCall cc = cluster_call(h, G, ndir, B, (size_t)T * B * ndir * HH, cl_bytes, grouped);
  if (!cc.plan.n) return false;
  // 64 units per CU (eight waves): H = 128 on two CUs alone, a kernel of its own with the same slots, LDS and arguments
  auto k = [] { if constexpr (HSU == 64) return lstm_bwd_cluster8_f32_kernel<HH>; else return lstm_bwd_cluster_f32_kernel<HH, HSU, OpF32>; }();
  size_t lds = bwd_f32_lds_bytes<OpF32>(HSU);   // two dG images + the hand-over buffer
  int form = HSU == 32 ? ASR_LSTM_BWD_F32_HS32 : ASR_LSTM_BWD_F32_HS64;
  if constexpr (HSU == 32 && (HH == 128 || HH == 256)) {
    if (cluster_f32_split_enabled()) {
      k = lstm_bwd_cluster_f32_kernel<HH, HSU, OpSplit3>;
      lds = bwd_f32_lds_bytes<OpSplit3>(HSU);
      form = ASR_LSTM_BWD_F32_SPLIT;
    }
  }
  run_tile_groups(h, cc, B, ndir, cl_bytes, st, 0, [&](const XchAreas& xa, int ncl, int t0, int nt) {
    hipLaunchKernelGGL(k, dim3(cluster_grid(G, ncl)), dim3(HSU * 8), lds, st, T, B, ndir,
                       dhout, (const f32x4_t*)gates, cs, (const float*)whpb, peep, seq_len, dcf, dhf, (f32x4_t*)dgates,
                       dpeep_part, xa.area, (unsigned*)cc.base, kernel_flags(), xa.znext, xa.zwords, h->bptt_clip, t0, nt);
  });
  h->lstm_counts[form] += 1;   // asr_lstm_kernel_counts
  return true;
}

bool asr_cluster_bwd_f32_try(asr_handle* h, int T, int B, int H, int ndir, const float* dhout,
                             const void* gates, const float* cs, const void* whpb, const float* peep,
                             const int32_t* seq_len, const float* dcf, const float* dhf, void* dgates,
                             float* dpeep_part, hipStream_t st) {
#define ASR_F32_ARGS_B h, T, B, ndir, dhout, gates, cs, whpb, peep, seq_len, dcf, dhf, dgates, dpeep_part, st, grouped
  return one_launch_else_groups([&](bool grouped) -> bool {
    if (!cluster_f32_enabled()) return false;
    if (bwd_units_per_cu() == 32) {
      if (H == 128) return cluster_bwd_f32_launch<128, 32>(ASR_F32_ARGS_B);
      if (!cluster_f32_wide_enabled()) return false;
      if (H == 256) return cluster_bwd_f32_launch<256, 32>(ASR_F32_ARGS_B);
      if (H == 320) return cluster_bwd_f32_launch<320, 32>(ASR_F32_ARGS_B);
      if (H == 512) return cluster_bwd_f32_launch<512, 32>(ASR_F32_ARGS_B);
      return false;
    }
    return H == 128 ? cluster_bwd_f32_launch<128, 64>(ASR_F32_ARGS_B) : false;
  });
#undef ASR_F32_ARGS_B
}

