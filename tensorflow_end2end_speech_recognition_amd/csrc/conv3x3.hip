// The 3x3 SAME convolution of the VGG front-end (models/encoders/core/vgg_blstm.py:107-177; row a5) for gfx950: the
// asr_conv3x3_* entry points and the kernels that exist for 3x3 only.  The per-frame images are small enough for a whole
// image WITH its zero border to sit in the LDS of one CU, so the hot shapes (64 / 128 channels, >= 64 images) run
// image-resident forms of the forward / data gradient (conv3x3_img_kernel) and of the weight gradient
// (conv3x3_wgrad_img_kernel); other shapes run the tiled implicit GEMMs of conv.hip on the Taps<3, 3, 1, 1> geometry
// (forward, data gradient) or the tiled weight gradient on the transposing LDS image (conv3x3_wgrad_tr_kernel).
// Operands, epilogues and results are the same in every form:
//   out[p, co] = act(sum_{tap, ci} x[p + s_tap, ci] Wt[co][tap * Cin + ci] + bias[co]),  s_tap = (tap / 3 - 1, tap % 3 - 1),
// x NHWC [Nimg, H, W, Cin], p = flat pixel index; the data gradient is the same product on dOut with the flipped-tap weight
// image.  A/B switches: ASR_CONV_IMG, ASR_CONV_STREAM, ASR_CONV_IMG_W8, ASR_CONV_WGRAD_IMG / _BIAS / _SPLIT / _TR / _BN64;
// ASR_CONV_DBG=1 records the phase timers that asr_debug_conv_cycles reads (scripts/probe_conv_phases.py).
#include "conv_common.h"
#include "mfma_tn.h"
#include <stdlib.h>

namespace {

// ---------------------------------------------------------------- 3x3 convolution, image-resident form (bf16)
// The per-frame images of the VGG front-end are small (40 x 11 x 64 ch = 56 KB, 20 x 6 x 128 ch = 31 KB), so a whole
// image WITH its zero border fits the LDS of one CU.  conv.hip's tiled conv_nt_kernel re-gathers every shifted pixel row from
// L2 for each of the nine taps and is bound by its CU's L2 port and by re-staging A through LDS (330 - 540 TFLOP/s on
// these shapes); here an image is staged ONCE (coalesced 16-byte copies, the next image's loads in flight under this
// image's products), the A fragments of all nine taps are 16-byte LDS reads at constant offsets from the centre pixel,
// and the weights -- the B operand -- sit in REGISTERS for the whole launch: a wave owns NTW 16-channel output tiles x all
// of K (288 VGPRs; one wave per SIMD, 512-entry register file), so nothing but A fragments moves per MFMA.
//   CIN = 64:  NTW = 4 -> a wave covers 64 output channels; waves split the image's 16-pixel tiles
//   CIN = 128: NTW = 2 -> waves split the output channels (and the pixel tiles when COUT = 64)
// One workgroup walks images blockIdx.x, + gridDim.x, ...  Same operands / epilogues / results as the tiled kernel
// (out[p, co] = act(sum_{tap, ci} x[p + s_tap, ci] Wt[co][tap * CIN + ci] + bias[co])).
// phase timers of the image loop (ASR_CONV_DBG=1; scripts/probe_conv_phases.py): per workgroup and wave, cycles summed over
// its images: [0] tile loop (of which [1] multiplies incl. their LDS reads, [2] epilogues), [3] wait for + LDS store of the
// next image, [4] the image's closing barrier, [5] images, [6] prefetch issue
__device__ unsigned long long* g_convdbg = nullptr;
// MAXV = staged 16-byte vectors per thread: ceil(H W CIN / 8 / 256) rounded up to an instantiated value (4 / 8 / 14 / 16) --
// the staging registers are what the CIN = 64 forms are short of (288 weight registers)
// ACT (compile time since round 5: a run-time `act` put branches into every epilogue piece, and a piece has to be straight-line
// code to be scheduled between the multiplies): 0 none, 1 ReLU, 2 data gradient gated by the sign of gate.act with a uniform
// scale (use_drop 0: 1, use_drop 2: 1 / keep), 4 the same with the Philox mask (use_drop 1), 3 forward ReLU + dropout.
// NW = waves per workgroup: 4 (one per SIMD) or, CIN = 64 only, 8 (two per SIMD, each wave two 16-channel output tiles = 144
// weight registers: the sibling wave fills the LDS latency and the epilogue's VALU work; round 5)
// STREAM (round 5, two LDS images): the next image is not held in MAXV staging registers for the whole image and written to LDS in
// one phase at its end (14 loads issued at once: 1.7 k cycles of issue stall, then 0.9 k cycles of LDS stores with nothing
// beside them, per 22.5 k-cycle image at 40 x 11 x 64) but STREAMED: every pixel tile requests two vectors at its top and stores
// the two of the tile before into the other image buffer -- eight staging registers instead of 16 - 64.
template <typename TO, int CIN, int COUT, int MAXV = 16, int ACT = 1, bool DBG = false, int NW = 4, bool STREAM = false>
__global__ __launch_bounds__(NW * 64, 1) void conv3x3_img_kernel(int Nimg, int H, int W, const bf16_t* __restrict__ X,
                                                             const bf16_t* __restrict__ Wt, TO* __restrict__ Out,
                                                             const float* __restrict__ bias, ConvGate gate,
                                                             int nbuf) {
  constexpr int KS = 9 * CIN / 32;                         // k-steps of 32
  constexpr int KPT = CIN / 32;                            // k-steps per tap
  constexpr int NTW = (CIN == 64 && NW == 4) ? 4 : 2;      // output tiles per wave
  constexpr int NTHR = NW * 64;
  constexpr int NGROUPS = (COUT / 16) / NTW;               // wave groups over the output channels
  constexpr int MPARTS = NW / NGROUPS;                     // waves sharing the pixel tiles of one channel group
  constexpr int PST = CIN * 2 + 16;                        // bytes per pixel in LDS (16-byte pad: conflict-free b128 reads)
  // the deferred epilogue keeps a second set of accumulators + gate operands alive: CIN = 64 with 14+ staged vectors (the
  // 40 x 11 images) has no registers for it (measured with it: spills in the tile loop, 2.87 -> 4.13 ms) and keeps the
  // epilogue behind its own tile; every other form defers (20 x 6 x 64 -> 128: 1.59 -> 1.23 ms, 128 -> 128: 2.44 -> 1.90 ms)
  constexpr bool DEFER = true;
  static_assert(NGROUPS >= 1 && NGROUPS <= NW && NW % NGROUPS == 0, "wave split");
  extern __shared__ __attribute__((aligned(16))) char csm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ng = wave % NGROUPS, mp = wave / NGROUPS;
  const int HW = H * W, WP = W + 2;
  const int img_bytes = (H + 2) * WP * PST;
  const int nvec = HW * CIN / 8;                           // 16-byte vectors of one image
  const int fr = lane & 15, fq = lane >> 4;

  // weights -> registers: B fragment (as first MFMA operand: rows = output channel) of tile nt, k-step ks:
  // lane (channel fr, k-group fq) holds Wt[n0 + fr][ks * 32 + fq * 8 .. + 7]
  bf16x8_t breg[NTW][KS];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const bf16_t* wp = Wt + (size_t)((ng * NTW + j) * 16 + fr) * (9 * CIN) + fq * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) breg[j][ks] = *reinterpret_cast<const bf16x8_t*>(wp + ks * 32);
  }
  // zero both images (borders stay zero for the whole launch)
  for (int i = tid * 16; i < nbuf * img_bytes; i += NTHR * 16) *reinterpret_cast<bf16x8_t*>(csm + i) = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
  __syncthreads();

  constexpr int SPT = 2;                                   // STREAM: vectors requested per pixel tile
  bf16x8_t stage[STREAM ? SPT : MAXV];                     // staged vectors per thread (nvec <= 256 MAXV)
  const int nvt = (nvec + NTHR - 1) / NTHR;                // vectors per thread and image
  auto gfetch = [&](int img) {
    const bf16x8_t* src = reinterpret_cast<const bf16x8_t*>(X + (size_t)img * HW * CIN);
    if constexpr (!STREAM) {
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int v = tid + i * NTHR;
        if (v < nvec) stage[i] = src[v];
      }
    }
  };
  const float invW = 1.0f / (float)W;
  // LDS position of vector v of an image (round 5: the quotient by the run-time W through the reciprocal -- exact for p < 2^22
  // -- instead of an integer division per staged vector: the 14 divisions were most of the 1.3 k cycles of this phase per image)
  auto vofs = [&](int v) -> int {
    const int p = v / (CIN / 8), cv = v % (CIN / 8);
    const int y = (int)(((float)p + 0.5f) * invW), x = p - y * W;
    return ((y + 1) * WP + x + 1) * PST + cv * 16;
  };
  auto lstore = [&](char* buf) {
    if constexpr (!STREAM) {
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int v = tid + i * NTHR;
        if (v < nvec) *reinterpret_cast<bf16x8_t*>(buf + vofs(v)) = stage[i];
      }
    }
  };
  // STREAM: vectors [i0, i0 + SPT) of this thread: request / store
  auto sfetch = [&](const bf16x8_t* src, int i0) {
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
      const int v = tid + (i0 + q) * NTHR;
      if (i0 + q < nvt && v < nvec) stage[q] = src[v];
    }
  };
  auto sstore = [&](char* buf, int i0) {
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
      const int v = tid + (i0 + q) * NTHR;
      if (i0 + q < nvt && v < nvec) *reinterpret_cast<bf16x8_t*>(buf + vofs(v)) = stage[q];
    }
  };
  int tapoff[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) tapoff[t] = ((t / 3 - 1) * WP + (t % 3 - 1)) * PST;
  const int ntm = (HW + 15) / 16;

  int img = blockIdx.x;
  if (img >= Nimg) return;
  if constexpr (STREAM) {                                  // the first image: straight through, once per launch
    const bf16x8_t* src0 = reinterpret_cast<const bf16x8_t*>(X + (size_t)img * HW * CIN);
    for (int i0 = 0; i0 < nvt; i0 += SPT) { sfetch(src0, i0); sstore(csm, i0); }
  } else {
    gfetch(img);
    lstore(csm);
  }
  __syncthreads();
  // Round 4: one wave per SIMD means every dependent trip of the epilogue was exposed -- the bias vector and (act == 2)
  // the gate operand were requested inside the epilogue, 4 + 4 global round trips per 16-pixel tile against 1 152 matrix
  // cycles (MfmaUtil 18 % at 64 -> 64, profiles/r03_pmc_util.md).  The bias now lives in registers for the launch, the gate
  // operand of a tile is requested at its top, and the first fragment group of the NEXT tile is read from LDS under the
  // last multiplies of this one.  Same arithmetic in the same order.
  // (round 5: the bias sits in LDS behind the images -- 16 registers the deferred epilogue needs; its read is one more
  // ds_read_b128 per piece beside the multiplies)
  float* bsm = reinterpret_cast<float*>(csm + nbuf * img_bytes);
  if (tid < COUT) bsm[tid] = bias ? bias[tid] : 0.f;
  __syncthreads();
  // taps per fragment group: CIN = 64 with the big staging set reads ONE tap (two fragments, 8 multiplies) ahead instead of
  // three -- 32 fragment registers that pay for the pending tile's accumulators
  constexpr int TG = (CIN == 64 && MAXV <= 8) ? 3 : 1, NG = 9 / TG, GF = TG * KPT;
  auto tile_ptr = [&](const char* base, int mt) -> const char* {
    const int p = mt * 16 + fr;
    const int pc = p < HW ? p : 0;
    const int y = (int)(((float)pc + 0.5f) * invW), x = pc - y * W;
    return base + ((y + 1) * WP + x + 1) * PST + fq * 16;
  };
  // Round 5 (phase timers, scripts/probe_conv_phases.py: of 24.6 k cycles per image and wave at 64 -> 64 the epilogues took
  // 5.5 k with nothing beside them -- one wave per SIMD, and the compiler does not pipeline across loop iterations): the
  // epilogue of a pixel tile is DEFERRED by one tile and issued in pieces (one 16-channel output tile each) between the
  // fragment groups of the NEXT tile's multiplies, across image boundaries too; the last tile of a workgroup is flushed
  // behind the image loop.  The pending tile's stores are raw buffer stores on a per-image descriptor: a lane whose pixel
  // lies past the image (the ragged last tile) or the very first "pending tile" of the workgroup (a zero-length
  // descriptor) is dropped by the bounds check -- no exec masking, no branch in the multiply stream.  Same arithmetic,
  // same values.
  const unsigned img_out_bytes = (unsigned)HW * COUT * (unsigned)sizeof(TO);
  f32x4_t accp[NTW];                                       // the pending tile: accumulators, gate operand, where it goes
  cg_us4_t gprep[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) { accp[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; gprep[j] = cg_us4_t{0, 0, 0, 0}; }
  __amdgpu_buffer_rsrc_t rsp = __builtin_amdgcn_make_buffer_rsrc(Out, 0, 0, 0x00020000);   // nothing pending: zero length
  unsigned offp = 0;                                       // byte offset of the pending pixel's channel 0 in its image
  size_t mp_elem = 0;                                      // element index of that pixel's channel 0 (gate / dropout counters)
  const float gscale = (ACT == 2 && gate.use_drop == 2) ? 1.f / gate.keep : 1.f;
  auto epilogue_piece = [&](int j) {
    const int nb = (ng * NTW + j) * 16 + fq * 4;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = accp[j][r];
    if constexpr (ACT == 0 || ACT == 1 || ACT == 3) {       // the forward products carry a bias (zeros in LDS without one)
      const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(bsm + nb);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += bv[r];
    }
    if constexpr (ACT == 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
    }
    // conv_gate_apply, branch-free (same expressions in the same order)
    if constexpr (ACT == 2) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = bf16_to_f32(gprep[j][r]) > 0.f ? v[r] * gscale : 0.f;
    }
    if constexpr (ACT == 4) {
      float mk[4];
      asr_dropout_words(gate.offset + (mp_elem + nb) / 4, gate.seed, gate.keep, 1.f / gate.keep, mk);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = bf16_to_f32(gprep[j][r]) > 0.f ? v[r] * mk[r] : 0.f;
    }
    if constexpr (ACT == 3) {
      float mk[4];
      asr_dropout_words(gate.offset + (mp_elem + nb) / 4, gate.seed, gate.keep, 1.f / gate.keep, mk);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = bf16_to_f32(f32_to_bf16(fmaxf(v[r], 0.f))) * mk[r];
    }
    typedef __attribute__((ext_vector_type(2))) unsigned cv_u2_t;
    typedef __attribute__((ext_vector_type(4))) unsigned cv_u4_t;
    if constexpr (sizeof(TO) == 4) {
      const cv_u4_t w = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
      __builtin_amdgcn_raw_buffer_store_b128(w, rsp, offp + (unsigned)nb * 4u, 0, 0);
    } else {
      const cv_u2_t w = {(unsigned)f32_to_bf16(v[0]) | ((unsigned)f32_to_bf16(v[1]) << 16),
                         (unsigned)f32_to_bf16(v[2]) | ((unsigned)f32_to_bf16(v[3]) << 16)};
      __builtin_amdgcn_raw_buffer_store_b64(w, rsp, offp + (unsigned)nb * 2u, 0, 0);
    }
  };
  unsigned long long ph[7] = {0, 0, 0, 0, 0, 0, 0};
#define CV_T() (DBG ? (__builtin_amdgcn_sched_barrier(0), __builtin_amdgcn_s_memtime()) : 0ull)
  for (int it = 0; img < Nimg; img += gridDim.x, ++it) {
    char* cur = csm + (nbuf == 2 ? (it & 1) * img_bytes : 0);
    const int nxt = img + gridDim.x;
    const unsigned long long tq0 = CV_T();
    if (nxt < Nimg) gfetch(nxt);                           // lands under this image's products
    const unsigned long long tq1 = CV_T();
    const bool morei = nxt < Nimg;                         // block-uniform
    const bf16x8_t* srcn = reinterpret_cast<const bf16x8_t*>(X + (size_t)(morei ? nxt : img) * HW * CIN);
    char* bufn = csm + ((it + 1) & 1) * img_bytes;         // STREAM implies two buffers
    int sq = 0;                                            // STREAM: this thread's next vector index
    const __amdgpu_buffer_rsrc_t rsc =
        __builtin_amdgcn_make_buffer_rsrc(Out + (size_t)img * HW * COUT, 0, img_out_bytes, 0x00020000);
    // (CIN = 64 keeps 288 weight registers + 64 staging registers: the 24 of the look-ahead group would spill)
    constexpr bool NEXTPF = CIN == 128;
    bf16x8_t anx[NEXTPF ? GF : 1];                         // group 0 of the tile about to start
    if (NEXTPF && mp < ntm) {
      const char* ap0 = tile_ptr(cur, mp);
#pragma unroll
      for (int q = 0; q < GF; ++q) anx[q] = *reinterpret_cast<const bf16x8_t*>(ap0 + tapoff[q / KPT] + (q % KPT) * 64);
    }
    // Two tiles per loop trip where the registers allow it (the pending / current accumulator sets then swap roles without
    // copies and the scheduler sees both tiles: 20 x 6 x 64 -> 128 ReLU 1.48 -> 1.21 ms, 128 -> 128 2.30 -> 2.04 ms); the gated
    // data gradient (ACT 2: two sets of gate operands) and the 40 x 11 x 64 form spill 13 - 31 registers that way and stay at one
    constexpr int UNR = (ACT >= 2 || MAXV > 8) ? 1 : 2;        // (the Philox epilogues measured slower unrolled: 1.96 -> 2.03 ms)
#pragma unroll UNR
    for (int mt = mp; mt < ntm; mt += MPARTS) {
      if constexpr (STREAM) {
        if (morei) {
          if (sq > 0) sstore(bufn, sq - SPT);              // what the tile before requested has landed (a tile of multiplies ago)
          sfetch(srcn, sq);
          sq += SPT;
        }
      }
      const int p = mt * 16 + fr;
      const char* ap = tile_ptr(cur, mt);
      const bool more = mt + MPARTS < ntm;                 // wave-uniform
      const char* apn = tile_ptr(cur, more ? mt + MPARTS : mt);
      const size_t m = (size_t)img * HW + (p < HW ? p : 0);
      cg_us4_t gpre[NTW];
#pragma unroll
      for (int j = 0; j < NTW; ++j) gpre[j] = cg_us4_t{0, 0, 0, 0};
      if constexpr (ACT == 2 || ACT == 4) {
#pragma unroll
        for (int j = 0; j < NTW; ++j) gpre[j] = conv_gate_load(gate, m * COUT + (ng * NTW + j) * 16 + fq * 4);
      }
      const unsigned long long tt0 = CV_T();
      f32x4_t acc[NTW];
#pragma unroll
      for (int j = 0; j < NTW; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      // A fragments in groups of TG taps, the next group's LDS reads issued ahead of this group's MFMAs (one wave per
      // SIMD: nothing else hides the LDS latency -- read-wait-multiply per fragment ran the matrix cores at ~15 %)
      bf16x8_t a[2][GF];
#pragma unroll
      for (int q = 0; q < GF; ++q) {
        if constexpr (NEXTPF) a[0][q] = anx[q];
        else a[0][q] = *reinterpret_cast<const bf16x8_t*>(ap + tapoff[q / KPT] + (q % KPT) * 64);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if (g + 1 < NG) {
#pragma unroll
          for (int q = 0; q < GF; ++q)
            a[(g + 1) & 1][q] = *reinterpret_cast<const bf16x8_t*>(ap + tapoff[(g + 1) * TG + q / KPT] + (q % KPT) * 64);
        } else if constexpr (NEXTPF) {
#pragma unroll
          for (int q = 0; q < GF; ++q)                      // the next tile's first group (this tile's again if it is the last)
            anx[q] = *reinterpret_cast<const bf16x8_t*>(apn + tapoff[q / KPT] + (q % KPT) * 64);
        }
        __builtin_amdgcn_sched_barrier(0);                 // (left alone the scheduler recycles ONE register quad)
#pragma unroll
        for (int q = 0; q < GF; ++q)
#pragma unroll
          for (int j = 0; j < NTW; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(breg[j][g * GF + q], a[g & 1][q], acc[j], 0, 0, 0);
        // the PENDING tile's epilogue, one output tile per piece, beside this group's multiplies
        if constexpr (DEFER) {
#pragma unroll
          for (int j = 0; j < NTW; ++j)
            if ((j * NG) / NTW == g) epilogue_piece(j);
        }
      }
      // this tile becomes the pending one
#pragma unroll
      for (int j = 0; j < NTW; ++j) { accp[j] = acc[j]; gprep[j] = gpre[j]; }
      rsp = rsc;
      offp = (unsigned)p * COUT * (unsigned)sizeof(TO);    // p >= HW: past the descriptor's length, the stores are dropped
      mp_elem = m * COUT;
      if constexpr (!DEFER) {
#pragma unroll
        for (int j = 0; j < NTW; ++j) epilogue_piece(j);
      }
      if (DBG) {
        const unsigned long long tt2 = CV_T();
        ph[1] += tt2 - tt0;
      }
    }
    // (Measured, round 4: barriers that wait for the LDS counter only -- s_waitcnt lgkmcnt(0) + s_barrier instead of
    // __syncthreads(), whose release fence also waits for the epilogue's global stores -- change nothing: 2.80 vs 2.76 ms.)
    const unsigned long long tq2 = CV_T();
    if constexpr (STREAM) {
      if (morei) {
        if (sq > 0) sstore(bufn, sq - SPT);
        for (; sq < nvt; sq += SPT) { sfetch(srcn, sq); sstore(bufn, sq); }   // more vectors than tiles x SPT: the rest, exposed
      }
    } else if (nxt < Nimg) {
      if (nbuf == 1) __syncthreads();                      // every wave is done with the only buffer
      lstore(csm + (nbuf == 2 ? ((it + 1) & 1) * img_bytes : 0));
    }
    const unsigned long long tq3 = CV_T();
    __syncthreads();
    if (DBG) {
      const unsigned long long tq4 = CV_T();
      ph[0] += tq2 - tq1; ph[3] += tq3 - tq2; ph[4] += tq4 - tq3; ph[5] += 1; ph[6] += tq1 - tq0;
    }
  }
  // flush: the last tile of this workgroup
  if constexpr (DEFER) {
#pragma unroll
    for (int j = 0; j < NTW; ++j) epilogue_piece(j);
  }
  if (DBG && g_convdbg && lane == 0 && blockIdx.x < 64) {
    unsigned long long* o = g_convdbg + ((size_t)blockIdx.x * 4 + wave) * 8;
#pragma unroll
    for (int k = 0; k < 7; ++k) o[k] = ph[k];
  }
#undef CV_T
}

// ---------------------------------------------------------------- 3x3 weight gradient, tiled, transposing LDS image
// Weight gradient: dW[tap*Cin + ci][co] = sum_p x[p + s_tap, ci] * dOut[p, co], i.e. gemm_tn_bf16_kernel (gemm.hip) with the
// A operand (reduction index = pixel, column = (tap, ci)) gathered from the image; B = dOut is plain.  On that kernel's LDS
// image (mfma_tn.h): a thread's gathered 16 bytes (8 channels of one tap at one pixel) are ONE ds_write_b128 into
// [subtile][k row][16 columns], and the MFMA fragments come out of it through the transposing reads (tn_frag) -- conv.hip's
// conv_wgrad_kernel interleaves pixel pairs into a [column][pixel] image with 64 four-byte LDS writes per thread per
// k-tile (twice the instructions of its 32 MFMAs).  ASR_CONV_WGRAD_TR=0 keeps that one (A/B).
template <int BN>
__global__ __launch_bounds__(256) void conv3x3_wgrad_tr_kernel(int Mpix, int H, int W, int Cin, int Cout,
                                                               const bf16_t* __restrict__ X,
                                                               const bf16_t* __restrict__ dY, int kchunk,
                                                               float* __restrict__ partial) {
  constexpr int BM = 128, BK = 64;
  constexpr int WN = BN / 64, WM = 4 / WN, TI = BM / WM / 16;   // BN = 64: four waves of 32 x 64, BN = 128: 2 x 2 of 64 x 64
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int M = 9 * Cin, N = Cout, K = Mpix, HW = H * W;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int kbeg = blockIdx.z * kchunk, kend = min(K, kbeg + kchunk);
  const int nkt = (kend - kbeg + BK - 1) / BK;

  // four (pixel, 8-column vector) items per operand per thread: vector mvec = tid & 15 of pixels (tid >> 4) + 16 q
  const int mvec = tid & 15, kr0 = tid >> 4;
  const int mcol = m0 + mvec * 8;                          // first of this thread's 8 virtual columns (tap, ci)
  const bool a_ok = mcol + 8 <= M, b_ok = mvec * 8 < BN && n0 + mvec * 8 + 8 <= N;
  const int tap = a_ok ? mcol / Cin : 0, ci = a_ok ? mcol - tap * Cin : 0;
  const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
  const ptrdiff_t sh = ((ptrdiff_t)dy * W + dx) * Cin + ci;
  const float invW = 1.0f / (float)W;
  const bf16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8_t ra[4], rb[4];
  // position of this thread's four pixels inside their images, carried from k-tile to k-tile (gload runs once per k-tile, in
  // order): the modulo by a run-time H W per pixel and k-tile -- ~60 instructions, four times -- was more VALU work than the
  // 32 MFMAs of the k-tile it feeds (MfmaUtil 27 %, profiles/r03_pmc_util.md)
  int remq[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) remq[q] = (kbeg + kr0 + 16 * q) % HW;
  auto gload = [&](int kt) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = kbeg + kt * BK + kr0 + 16 * q;         // pixel = reduction index
      const bool kin = p < kend;
      const int pp = kin ? p : 0;
      const int rem = remq[q];
      remq[q] += BK;
      while (remq[q] >= HW) remq[q] -= HW;
      const int y = (int)(((float)rem + 0.5f) * invW), x = rem - y * W;      // exact for rem < 2^22
      const bool ok = a_ok && kin && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
      ra[q] = ok ? *reinterpret_cast<const bf16x8_t*>(X + (ptrdiff_t)((size_t)pp * Cin) + sh) : zero;
      rb[q] = (b_ok && kin) ? *reinterpret_cast<const bf16x8_t*>(dY + (size_t)pp * Cout + n0 + mvec * 8) : zero;
    }
  };
  const unsigned wbase = (unsigned)(mvec >> 1) * TN_SUB + (unsigned)kr0 * 32u + (unsigned)(mvec & 1) * 16u;
  auto sstore = [&](char* st) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<bf16x8_t*>(st + wbase + q * 16 * 32) = ra[q];
      if (mvec * 8 < BN) *reinterpret_cast<bf16x8_t*>(st + TN_OPER + wbase + q * 16 * 32) = rb[q];
    }
  };

  f32x4_t acc[TI][4];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  if (nkt > 0) {
    gload(0);
    sstore(smem);
  }
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  const unsigned piece = (unsigned)(8 * fq + (fr >> 2)) * 32u + (unsigned)(fr & 3) * 8u;
  unsigned aoff[TI], boff[4];
#pragma unroll
  for (int i = 0; i < TI; ++i) aoff[i] = (unsigned)(wm * TI + i) * TN_SUB + piece;
#pragma unroll
  for (int i = 0; i < 4; ++i) boff[i] = (unsigned)TN_OPER + (unsigned)(wn * 4 + i) * TN_SUB + piece;
  for (int kt = 0; kt < nkt; ++kt) {
    const char* cur = smem + (kt & 1) * TN_STAGE;
    if (kt + 1 < nkt) gload(kt + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t a[TI], b[4];
#pragma unroll
      for (int i = 0; i < TI; ++i) a[i] = tn_frag(cur + aoff[i] + ks * 32 * 32);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = tn_frag(cur + boff[j] + ks * 32 * 32);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nkt) sstore(smem + ((kt + 1) & 1) * TN_STAGE);
    __syncthreads();
  }
  float* slab = partial + (size_t)blockIdx.z * M * N;
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int m = m0 + wm * (16 * TI) + i * 16 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nb = n0 + wn * 64 + j * 16 + fq * 4;
      if (nb >= N) continue;
      *reinterpret_cast<f32x4_t*>(slab + (size_t)m * N + nb) = acc[i][j];
    }
  }
}


// ---------------------------------------------------------------- 3x3 weight gradient, image-resident form (round 5)
// dW[tap * CIN + ci][co] = sum over images and pixels p of x[p + s_tap, ci] * dY[p, co].  The tiled kernels gather every
// shifted pixel row from L2 once per tap (nine times) and, at COUT = 64, multiply half-empty 128-column tiles: 6.4 ms for
// the 40 x 11 x 64 -> 64 layer of cfg C (299 TFLOP/s).  Here a workgroup stages a whole frame image of x (with its zero
// border) and 64 output channels of dY into LDS ONCE per image, in the pixel-major layout they have in memory, and takes both
// MFMA operands out of them with the transposing LDS read (ds_read_b64_tr_b16: each lane passes the address of 4 channels of
// ONE pixel and receives ONE channel at 4 consecutive pixels -- the row stride is free, so the padded image works as it lies
// and a tap is a constant byte offset).  Wave w owns the 16 input channels 16 w .. of all nine taps x the 64 output channels of
// the workgroup's column block (blockIdx.y): 36 accumulator tiles in registers for the whole launch; CIN / 16 waves.  The
// reduction runs over the pixels of an image in chunks of 32 and over the images blockIdx.x, + gridDim.x, ...; the next
// image's vectors are requested a few per chunk under the multiplies.  Each workgroup row writes ONE slab [9 CIN][COUT] (its
// 64 columns); the slabs are summed in a fixed order (deterministic).  HBM traffic: dY once, x once per
// 64-column block.  40 x 11 x 64 -> 64: 6.40 -> 2.59 ms (738 TFLOP/s) on the first build.
// NSPLIT: the workgroup's 64 output columns dealt over NSPLIT waves per input-channel group (CIN = 64: 2 -> eight waves, two per
// SIMD, each 9 x 2 accumulator tiles: the second wave of a SIMD fills the LDS latency of the first; 2.66 -> see the launcher)
// BIAS: the bias gradient (column sums of dY over all pixels) from the staged dY as well: the wave of input-channel group g
// multiplies a fragment of ONES with its dY fragments in the chunks c % (CIN / 16) == g (one more MFMA per NT tiles in a
// quarter / an eighth of the chunks, instead of a second pass over dY: 0.30 - 0.54 ms per layer of the cfg C step), and
// writes its partial sums as row 9 CIN + g of the slab; wgrad_img_reduce_kernel adds those rows over slabs and groups.
template <int CIN, int MAXVX, int MAXVY, int NSPLIT, bool BIAS = false>
__global__ __launch_bounds__(CIN * 4 * NSPLIT, 1) void conv3x3_wgrad_img_kernel(int Nimg, int H, int W, int Cout,
                                                                       const bf16_t* __restrict__ X,
                                                                       const bf16_t* __restrict__ dY,
                                                                       float* __restrict__ partial) {
  static_assert(CIN == 64 || CIN == 128, "one 16-channel group of x per wave, 4 or 8 waves");
  constexpr int NTH = CIN * 4 * NSPLIT;
  constexpr int CB = 64, NT = 4 / NSPLIT;                    // columns of one workgroup / output tiles of one wave
  constexpr int PSX = CIN * 2 + 16, PSY = CB * 2 + 16;       // bytes per pixel in LDS (16-byte pad: distinct banks per block row)
  constexpr int MAXV = MAXVX > MAXVY ? MAXVX : MAXVY;
  extern __shared__ __attribute__((aligned(16))) char wsm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = (tid >> 6) % (CIN / 16), nh = (tid >> 6) / (CIN / 16);   // input-channel group / column part of this wave
  const int HW = H * W, WP = W + 2;
  const int n0 = blockIdx.y * CB;
  const int nchunk = (HW + 31) / 32;
  const int ximg_bytes = (H + 2) * WP * PSX;
  char* xs = wsm;                                            // x image with its border
  char* ys = wsm + ximg_bytes;                               // dY image (64 channels), nchunk * 32 pixel rows (tail rows stay zero)
  const int yimg_bytes = nchunk * 32 * PSY;
  const int nvx = HW * CIN / 8, nvy = HW * CB / 8;           // 16-byte vectors of one image
  const float invW = 1.0f / (float)W;

  for (int i = tid * 16; i < ximg_bytes + yimg_bytes; i += NTH * 16)
    *reinterpret_cast<bf16x8_t*>(wsm + i) = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
  __syncthreads();

  bf16x8_t stx[MAXVX], sty[MAXVY];
  auto fetch1 = [&](int img, int i) {                        // vector i of this thread, both operands
    const int v = tid + i * NTH;
    if (i < MAXVX && v < nvx) stx[i < MAXVX ? i : 0] = reinterpret_cast<const bf16x8_t*>(X + (size_t)img * HW * CIN)[v];
    if (i < MAXVY && v < nvy) {
      const int p = v / (CB / 8), cv = v % (CB / 8);
      sty[i < MAXVY ? i : 0] = *reinterpret_cast<const bf16x8_t*>(dY + ((size_t)img * HW + p) * Cout + n0 + cv * 8);
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < MAXVX; ++i) {
      const int v = tid + i * NTH;
      if (v < nvx) {
        const int p = v / (CIN / 8), cv = v % (CIN / 8);
        const int y = (int)(((float)p + 0.5f) * invW), x = p - y * W;
        *reinterpret_cast<bf16x8_t*>(xs + ((y + 1) * WP + x + 1) * PSX + cv * 16) = stx[i];
      }
    }
#pragma unroll
    for (int i = 0; i < MAXVY; ++i) {
      const int v = tid + i * NTH;
      if (v < nvy) {
        const int p = v / (CB / 8), cv = v % (CB / 8);
        *reinterpret_cast<bf16x8_t*>(ys + p * PSY + cv * 16) = sty[i];
      }
    }
  };
  // lane -> its piece of a 4-pixel x 16-channel block: pixel row (lane & 15) >> 2 of k-group lane >> 4, channels 4 (lane & 3)..
  const int kg = lane >> 4, prow = (lane & 15) >> 2, c4 = lane & 3;
  const int xch = (wave * 16 + c4 * 4) * 2;                  // byte offset of this lane's 4 input channels
  const int ych = (nh * NT * 16 + c4 * 4) * 2;
  int tapoff[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) tapoff[t] = ((t / 3 - 1) * WP + (t % 3 - 1)) * PSX;
  // LDS byte offset of a pixel's centre tap in the x image.  A pixel past the image reads the LAST pixel of x (finite)
  // against a zero row of dY.
  auto xofs = [&](int p) -> int {
    const int pc = p < HW ? p : HW - 1;
    const int y = (int)(((float)pc + 0.5f) * invW), x = pc - y * W;
    return ((y + 1) * WP + x + 1) * PSX + xch;
  };
  typedef __attribute__((address_space(3))) bf16x4_t wl4_t;
  auto trfrag = [&](const char* lo, const char* hi) -> bf16x8_t {
    const bf16x4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wl4_t*)(lo));
    const bf16x4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wl4_t*)(hi));
    return (bf16x8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  };

  f32x4_t acc[9][NT];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  f32x4_t accb[BIAS ? NT : 1];
#pragma unroll
  for (int j = 0; j < (BIAS ? NT : 1); ++j) accb[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const bf16x8_t ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};

  int img = blockIdx.x;
  if (img < Nimg) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i) fetch1(img, i);
    lstore();
  }
  __syncthreads();
  for (; img < Nimg; img += gridDim.x) {
    const int nxt = img + gridDim.x;
    const bool more = nxt < Nimg;                            // block-uniform
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
      // the next image: vector pairs i = 2c, 2c + 1 in chunk c (2 nchunk >= MAXV for every supported image: the launcher checks)
      if (more) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i)
          if (i / 2 == c) fetch1(nxt, i);
      }
      const int p0 = c * 32 + kg * 8 + prow;
      const int xlo = xofs(p0), xhi = xofs(p0 + 4);
      const int ylo = p0 * PSY + ych, yhi = (p0 + 4) * PSY + ych;
      bf16x8_t b[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) b[j] = trfrag(ys + ylo + j * 32, ys + yhi + j * 32);
      if constexpr (BIAS) {
        if (c % (CIN / 16) == wave) {                        // wave-uniform
#pragma unroll
          for (int j = 0; j < NT; ++j) accb[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, b[j], accb[j], 0, 0, 0);
        }
      }
      bf16x8_t a[3];
      a[0] = trfrag(xs + xlo + tapoff[0], xs + xhi + tapoff[0]);
      a[1] = trfrag(xs + xlo + tapoff[1], xs + xhi + tapoff[1]);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        if (t + 2 < 9) a[(t + 2) % 3] = trfrag(xs + xlo + tapoff[t + 2], xs + xhi + tapoff[t + 2]);
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t % 3], b[j], acc[t][j], 0, 0, 0);
      }
    }
    __syncthreads();                                         // every wave is done with this image
    if (more) lstore();
    __syncthreads();
  }
  // slab of this workgroup row: lane holds rows rg*4 + r (input channel within the wave's group), column lane & 15 of tile j
  float* slab = partial + (size_t)blockIdx.x * (9 * CIN + (BIAS ? CIN / 16 : 0)) * Cout;
  const int col = lane & 15, rg = lane >> 4;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        slab[(size_t)(t * CIN + wave * 16 + rg * 4 + r) * Cout + n0 + (nh * NT + j) * 16 + col] = acc[t][j][r];
  if constexpr (BIAS) {                                      // all 16 rows of accb are the same column sums: row 0
    if (rg == 0) {
#pragma unroll
      for (int j = 0; j < NT; ++j) slab[(size_t)(9 * CIN + wave) * Cout + n0 + (nh * NT + j) * 16 + col] = accb[j][0];
    }
  }
}
// fixed-order sum of the slabs of conv3x3_wgrad_img_kernel<..., BIAS = true>: rows [0, Mw) -> dw, rows Mw .. Mw + G - 1 -> dbias
// Round 6: four columns per thread and eight slabs requested at a time, added in slab order -- the same sums in the same order
// as the one-load-per-addition loop this replaces, which ran at the memory latency per slab (0.98 ms for the 128 slabs of
// the 128 -> 128 layer at cfg C, three such passes on the lane that ends the step; the bytes take ~25 us).  N % 4 == 0 (the
// image-resident kernel wants Cout % 64 == 0); VEC = 0: dw is not 16-byte aligned, scalar stores.
template <int VEC>
__global__ void wgrad_img_reduce_kernel(const float* __restrict__ partial, int S, int Mw, int G, int N, float* __restrict__ dw,
                                        float* __restrict__ dbias, int accumulate) {
  const size_t slab = (size_t)(Mw + G) * N, wn = (size_t)Mw * N;
  const size_t nv = wn / 4, slab4 = slab / 4;
  const size_t nthreads = (size_t)gridDim.x * blockDim.x, tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const f32x4_t* p4 = reinterpret_cast<const f32x4_t*>(partial);
  for (size_t q = tid; q < nv; q += nthreads) {
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    int z = 0;
    for (; z + 8 <= S; z += 8) {
      f32x4_t t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = p4[(size_t)(z + u) * slab4 + q];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; z < S; ++z) v += p4[(size_t)z * slab4 + q];
    if (VEC) {
      f32x4_t* d = reinterpret_cast<f32x4_t*>(dw) + q;
      *d = accumulate ? *d + v : v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) dw[4 * q + k] = accumulate ? dw[4 * q + k] + v[k] : v[k];
    }
  }
  if (dbias) {
    for (size_t n = tid; n < (size_t)N; n += nthreads) {
      float v = 0.f;
      for (int z = 0; z < S; ++z)
        for (int g = 0; g < G; ++g) v += partial[(size_t)z * slab + wn + (size_t)g * N + n];
      dbias[n] = accumulate ? dbias[n] + v : v;
    }
  }
}

}  // namespace

// ---------------------------------------------------------------- entry points
extern "C" int asr_conv3x3_prep_weights(asr_handle* h, const float* w_hwio, int Cin, int Cout, void* wt_fwd,
                                        void* wt_bwd, asr_stream s) {
  return asr_conv_prep(h, "asr_conv3x3_prep_weights", 9, w_hwio, Cin, Cout, wt_fwd, wt_bwd, s);
}

static unsigned long long* g_convdbg_host = nullptr;
extern "C" int asr_debug_conv_cycles(unsigned long long* out, int n) {
  if (!g_convdbg_host || n > 64 * 4 * 8) return -1;
  return hipMemcpy(out, g_convdbg_host, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
// asr_conv_path_counts: the channel pair of a forward / data-gradient product (conv.hip's tiled launcher counts its own)
int asr_conv_pair_counter(int Cin, int Cout) {
  if (Cin == 64 && Cout == 64) return ASR_CONVP_PAIR_64_64;
  if (Cin == 64 && Cout == 128) return ASR_CONVP_PAIR_64_128;
  if (Cin == 128 && Cout == 128) return ASR_CONVP_PAIR_128_128;
  if (Cin == 128 && Cout == 64) return ASR_CONVP_PAIR_128_64;
  return ASR_CONVP_PAIR_OTHER;
}
// ... and one image-resident launch: the template arguments of the instantiation that was launched
static void conv_count_img(asr_handle* h, int ci, int co, int maxv, int act, int nbuf, bool stream, bool w8) {
  unsigned long long* c = h->conv_counts;
  c[ASR_CONVP_FORM_IMG] += 1;
  c[asr_conv_pair_counter(ci, co)] += 1;
  c[maxv == 2 ? ASR_CONVP_MAXV_2 : maxv == 4 ? ASR_CONVP_MAXV_4 : maxv == 8 ? ASR_CONVP_MAXV_8
    : maxv == 14 ? ASR_CONVP_MAXV_14 : ASR_CONVP_MAXV_16] += 1;
  c[ASR_CONVP_ACT_0 + act] += 1;
  c[nbuf == 1 ? ASR_CONVP_NBUF_1 : ASR_CONVP_NBUF_2] += 1;
  if (stream) c[ASR_CONVP_STREAM] += 1;
  if (w8) c[ASR_CONVP_W8] += 1;
}
template <typename TO>
static int conv3x3_launch(asr_handle* h, const void* x, int Nimg, int H, int W, int Cin, const void* wt,
                          const float* bias, int Cout, int act, void* out, hipStream_t st,
                          ConvGate gate = ConvGate{nullptr, 1.f, 0, 0, 0}) {
  const long long mp = (long long)Nimg * H * W;
  if (mp <= 0 || mp >= (1ll << 31)) ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_conv3x3: %lld pixels", mp);
  {
    // image-resident form: the image with its border fits one CU's LDS (twice: the next image is staged under the
    // products of this one) and there are enough images to fill the chip; ASR_CONV_IMG=0 keeps the tiled kernel (A/B)
    static const bool img_on = [] { const char* e = getenv("ASR_CONV_IMG"); return !(e && e[0] == '0'); }();
    const size_t img_bytes = (size_t)(H + 2) * (W + 2) * (Cin * 2 + 16);
    const int nvec = H * W * Cin / 8;
    const bool shape = (Cin == 64 || Cin == 128) && (Cout == 64 || Cout == 128);
    if (img_on && shape && nvec <= 16 * 256 && img_bytes <= (size_t)156 * 1024 && Nimg >= 64) {
      const int nbuf = 2 * img_bytes <= (size_t)158 * 1024 ? 2 : 1;
      const size_t lds = nbuf * img_bytes + 128 * sizeof(float);             // images + the bias vector
      const int mv = (nvec + 255) / 256;
      const unsigned grid = (unsigned)(Nimg < h->num_cu ? Nimg : h->num_cu);
      static unsigned long long* dbg_host = nullptr;
      static const bool dbg_on = [] { const char* e = getenv("ASR_CONV_DBG"); return e && e[0] == '1'; }();
      if (dbg_on && !dbg_host) {
        (void)hipMalloc(&dbg_host, 64 * 4 * 8 * sizeof(unsigned long long));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_convdbg), &dbg_host, sizeof(dbg_host));
        g_convdbg_host = dbg_host;
      }
      // compile-time epilogue: 0 none, 1 ReLU, 2 gated data gradient with a uniform scale, 4 with the Philox mask, 3 ReLU + dropout
      const int actc = act == 2 ? (gate.use_drop == 1 ? 4 : 2) : act;
      static const bool stream_on = [] { const char* e = getenv("ASR_CONV_STREAM"); return !(e && e[0] == '0'); }();
      const bool strm = stream_on && nbuf == 2;
#define ASR_CONV_IMG_A(CI, CO, MV, AC)                                                                               \
  do {                                                                                                               \
    /* measured (profiles/r05_conv_stream.md): streaming wins 5 % for 64 -> 64 without the gate loads, loses 3 - 12 % elsewhere */ \
    constexpr bool SOK = CI == 64 && CO == 64 && (AC == 1 || AC == 3);                                               \
    auto k = conv3x3_img_kernel<TO, CI, CO, MV, AC, false>;                                                          \
    bool streamed = false;                                                                                           \
    if constexpr (SOK) { if (strm) { k = conv3x3_img_kernel<TO, CI, CO, MV, AC, false, 4, true>; streamed = true; } } \
    if constexpr (AC == 1) { if (dbg_on) { k = conv3x3_img_kernel<TO, CI, CO, MV, AC, true>; streamed = false; } }   \
    conv_count_img(h, CI, CO, MV, AC, nbuf, streamed, false);                                                        \
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                 \
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, st, Nimg, H, W, (const bf16_t*)x, (const bf16_t*)wt, (TO*)out, \
                       bias, gate, nbuf);                                                                            \
  } while (0)
#define ASR_CONV_IMG8_A(CI, CO, MV, AC)                                                                              \
  do {                                                                                                               \
    auto k = conv3x3_img_kernel<TO, CI, CO, MV, AC, false, 8>;                                                       \
    conv_count_img(h, CI, CO, MV, AC, nbuf, false, true);                                                            \
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                 \
    hipLaunchKernelGGL(k, dim3(grid), dim3(512), lds, st, Nimg, H, W, (const bf16_t*)x, (const bf16_t*)wt, (TO*)out, \
                       bias, gate, nbuf);                                                                            \
  } while (0)
#define ASR_CONV_IMG(CI, CO, MV)                                                                                     \
  do {                                                                                                               \
    if constexpr (sizeof(TO) == 4) { ASR_CONV_IMG_A(CI, CO, MV, 0); }                                                \
    else {                                                                                                           \
      if (actc == 1) ASR_CONV_IMG_A(CI, CO, MV, 1);                                                                  \
      else if (actc == 2) ASR_CONV_IMG_A(CI, CO, MV, 2);                                                             \
      else if (actc == 3) ASR_CONV_IMG_A(CI, CO, MV, 3);                                                             \
      else if (actc == 4) ASR_CONV_IMG_A(CI, CO, MV, 4);                                                             \
      else ASR_CONV_IMG_A(CI, CO, MV, 0);                                                                            \
    }                                                                                                                \
  } while (0)
      // (the VGG front-end's images: 40 x 11 x 64 -> 14 staged vectors per thread, 20 x 6 x 64 -> 4, 20 x 6 x 128 -> 8)
      // eight waves (two per SIMD, two output tiles each) for the forward ReLU + dropout of small images: the sibling wave
      // hides the Philox rounds of the epilogue (20 x 6 x 64 -> 128: 1.96 -> 1.70 ms).  Measured, not used elsewhere: the
      // 40 x 11 forms spill 16 - 46 registers at 256 per wave (ACT 3: 3.54 -> 4.15 ms), the ReLU forms are unchanged (1.17 ms).
      static const bool w8_on = [] { const char* e = getenv("ASR_CONV_IMG_W8"); return !(e && e[0] == '0'); }();
      bool done8 = false;
      if constexpr (sizeof(TO) == 2) {
        if (Cin == 64 && w8_on && mv <= 4 && actc == 3) {
          if (Cout == 64) ASR_CONV_IMG8_A(64, 64, 2, 3); else ASR_CONV_IMG8_A(64, 128, 2, 3);
          done8 = true;
        }
      }
      if (done8) {}
      else if (Cin == 64 && Cout == 64) { if (mv <= 14) ASR_CONV_IMG(64, 64, 14); else ASR_CONV_IMG(64, 64, 16); }
      else if (Cin == 64 && Cout == 128) { if (mv <= 4) ASR_CONV_IMG(64, 128, 4); else ASR_CONV_IMG(64, 128, 16); }
      else if (Cin == 128 && Cout == 128) { if (mv <= 8) ASR_CONV_IMG(128, 128, 8); else ASR_CONV_IMG(128, 128, 16); }
      else { if (mv <= 8) ASR_CONV_IMG(128, 64, 8); else ASR_CONV_IMG(128, 64, 16); }
#undef ASR_CONV_IMG
#undef ASR_CONV_IMG_A
#undef ASR_CONV_IMG8_A
      ASR_CHECK_LAUNCH(h, "asr_conv3x3(image-resident)");
      return ASR_OK;
    }
  }
  // every other shape: the tiled kernel; the flipped image of the data gradient has the forward's geometry
  return asr_conv_nt<Taps33>(h, "asr_conv3x3", x, Nimg, H, W, Cin, wt, bias, Cout, act, gate, sizeof(TO) == 4, out,
                             (asr_stream)st);
}

extern "C" int asr_conv3x3_fwd(asr_handle* h, const void* x, int Nimg, int H, int W, int Cin, const void* wt_fwd,
                               const float* bias, int Cout, int relu, void* out, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!x || !wt_fwd || !out || Nimg < 1 || H < 1 || W < 1)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_conv3x3_fwd: bad args");
  if (Cin % 64 != 0 || Cout % 64 != 0)
    ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_conv3x3_fwd: Cin=%d, Cout=%d must be multiples of 64", Cin, Cout);
  return conv3x3_launch<bf16_t>(h, x, Nimg, H, W, Cin, wt_fwd, bias, Cout, relu ? 1 : 0, out, (hipStream_t)s);
}

extern "C" int asr_conv3x3_fwd_drop(asr_handle* h, const void* x, int Nimg, int H, int W, int Cin, const void* wt_fwd,
                                    const float* bias, int Cout, float keep_prob, uint64_t seed, uint64_t offset,
                                    void* out, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!x || !wt_fwd || !out || Nimg < 1 || H < 1 || W < 1 || !(keep_prob > 0.f && keep_prob <= 1.f))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_conv3x3_fwd_drop: bad args");
  if (Cin % 64 != 0 || Cout % 64 != 0)
    ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_conv3x3_fwd_drop: Cin=%d, Cout=%d must be multiples of 64", Cin, Cout);
  const ConvGate gate = {nullptr, keep_prob, seed, offset, 1};
  return conv3x3_launch<bf16_t>(h, x, Nimg, H, W, Cin, wt_fwd, bias, Cout, 3, out, (hipStream_t)s, gate);
}

extern "C" int asr_conv3x3_bwd_data(asr_handle* h, const void* dy, int Nimg, int H, int W, int Cout,
                                    const void* wt_bwd, int Cin, float* dx, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!dy || !wt_bwd || !dx || Nimg < 1 || H < 1 || W < 1)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_conv3x3_bwd_data: bad args");
  if (Cin % 64 != 0 || Cout % 64 != 0)
    ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_conv3x3_bwd_data: Cin=%d, Cout=%d must be multiples of 64", Cin, Cout);
  // the data gradient is a convolution of dOut (Cout channels) with the flipped-tap image -> Cin channels
  return conv3x3_launch<float>(h, dy, Nimg, H, W, Cout, wt_bwd, nullptr, Cin, 0, dx, (hipStream_t)s);
}

extern "C" int asr_conv3x3_bwd_data_relu(asr_handle* h, const void* dy, int Nimg, int H, int W, int Cout,
                                         const void* wt_bwd, int Cin, const void* act_below, float keep_prob,
                                         uint64_t seed, uint64_t offset, int use_drop, void* dpre_below, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!dy || !wt_bwd || !act_below || !dpre_below || Nimg < 1 || H < 1 || W < 1 ||
      (use_drop && !(keep_prob > 0.f && keep_prob <= 1.f)) || use_drop < 0 || use_drop > 2)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_conv3x3_bwd_data_relu: bad args");
  if (Cin % 64 != 0 || Cout % 64 != 0)
    ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_conv3x3_bwd_data_relu: Cin=%d, Cout=%d must be multiples of 64", Cin, Cout);
  const ConvGate gate = {(const bf16_t*)act_below, keep_prob, seed, offset, use_drop};
  return conv3x3_launch<bf16_t>(h, dy, Nimg, H, W, Cout, wt_bwd, nullptr, Cin, 2, dpre_below, (hipStream_t)s, gate);
}

// weight (+ bias) gradient: image-resident form, else tiled (tr image; ASR_CONV_WGRAD_TR=0: conv.hip's [column][pixel] image)
extern "C" int asr_colsum(asr_handle* h, int dtype, const void* a, int M, int N, int lda, float* out, asr_stream s);
static int conv3x3_bwd_weight_impl(asr_handle* h, const void* x, const void* dy, int Nimg, int H, int W,
                                   int Cin, int Cout, float* dw, float* dbias, int accumulate, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!x || !dy || !dw || Nimg < 1 || H < 1 || W < 1)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_conv3x3_bwd_weight: bad args");
  if (Cin % 8 != 0 || Cout % 8 != 0)
    ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_conv3x3_bwd_weight: Cin=%d, Cout=%d must be multiples of 8", Cin, Cout);
  const long long mp = (long long)Nimg * H * W;
  if (mp >= (1ll << 31)) ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_conv3x3_bwd_weight: %lld pixels", mp);
  const int Mpix = (int)mp, M = 9 * Cin, N = Cout;
  static const bool wgrad_tr = [] { const char* e = getenv("ASR_CONV_WGRAD_TR"); return !(e && e[0] == '0'); }();
  // COUT = 64 (or a last 64-column tile): 128 x 64 tiles, so that no MFMA multiplies zero columns -- measured 6.4 ms per
  // call against 6.0 for the 128 x 128 tiles at cfg C's second layer (the kernel is bound by gathering every pixel nine
  // times from L2, not by its MFMAs): OFF unless ASR_CONV_WGRAD_BN64=1
  static const bool bn64_on = [] { const char* e = getenv("ASR_CONV_WGRAD_BN64"); return e && e[0] == '1'; }();
  const bool bn64 = wgrad_tr && bn64_on && N % 128 == 64;
  const int tm = (M + 127) / 128, tn = bn64 ? (N + 63) / 64 : (N + 127) / 128;
  int S, kchunk;                                             // of the tiled forms (at most 512 slabs)
  const int rc = asr_conv_wgrad_plan(h, "asr_conv3x3_bwd_weight", Mpix, tm * tn, (size_t)M * N * sizeof(float), 512, &S, &kchunk);
  if (rc != ASR_OK) return rc;
  float* partial = (float*)h->scratch;
  hipStream_t st = (hipStream_t)s;
  {
    // image-resident form (round 5): x and dY images in LDS, 9 taps from one staging; ASR_CONV_WGRAD_IMG=0 keeps the tiled kernel
    static const bool wimg_on = [] { const char* e = getenv("ASR_CONV_WGRAD_IMG"); return !(e && e[0] == '0'); }();
    const int HWp = H * W, nchunk = (HWp + 31) / 32;
    const size_t lds = (size_t)(H + 2) * (W + 2) * (Cin * 2 + 16) + (size_t)nchunk * 32 * (64 * 2 + 16);
    const int nth = Cin * 4;
    const int mvx = (HWp * Cin / 8 + nth - 1) / nth, mvy = (HWp * 8 + nth - 1) / nth;   // staged vectors per thread
    const int mv = mvx > mvy ? mvx : mvy;
    static const bool wbias_on = [] { const char* e = getenv("ASR_CONV_WGRAD_BIAS"); return !(e && e[0] == '0'); }();
    const bool inb = dbias && wbias_on;                      // bias gradient inside the weight-gradient kernel
    const int G = inb ? Cin / 16 : 0;
    const size_t slab = (size_t)(M + G) * N * sizeof(float);
    size_t wgs = (h->scratch_bytes - ASR_XCH_BYTES) / slab;
    const size_t cols = (size_t)(Cout / 64);
    if (wgs * cols > (size_t)h->num_cu) wgs = (size_t)h->num_cu / cols;
    if (wgs > (size_t)Nimg) wgs = (size_t)Nimg;
    // (Cin = 128 runs eight waves, two per SIMD: 256 registers, of which 144 are accumulators -- small images only)
    if (wimg_on && (Cin == 64 || (Cin == 128 && mvx <= 4 && mvy <= 2)) && Cout % 64 == 0 && Nimg >= 64 &&
        lds <= (size_t)158 * 1024 && mv <= 14 && nchunk * 2 >= mv && wgs >= 32) {
#define ASR_WGRAD_IMG(CI, VX, VY, NS)                                                                                  \
  do {                                                                                                                 \
    auto kern = inb ? conv3x3_wgrad_img_kernel<CI, VX, VY, NS, true> : conv3x3_wgrad_img_kernel<CI, VX, VY, NS, false>; \
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                \
    hipLaunchKernelGGL(kern, dim3((unsigned)wgs, (unsigned)cols), dim3(CI * 4 * NS), lds, st, Nimg, H, W, Cout,        \
                       (const bf16_t*)x, (const bf16_t*)dy, partial);                                                  \
  } while (0)
      // (the VGG front-end's images: 40 x 11 x 64 -> 7 + 7 staged vectors per thread of eight waves, 20 x 6 x 64 -> 2 + 2,
      // 20 x 6 x 128 -> 4 + 2)
      static const bool split_on = [] { const char* e = getenv("ASR_CONV_WGRAD_SPLIT"); return !(e && e[0] == '0'); }();
      if (Cin == 64 && split_on) { if (mv <= 4) ASR_WGRAD_IMG(64, 2, 2, 2); else ASR_WGRAD_IMG(64, 7, 7, 2); }
      else if (Cin == 64) { if (mv <= 4) ASR_WGRAD_IMG(64, 4, 4, 1); else ASR_WGRAD_IMG(64, 14, 14, 1); }
      else ASR_WGRAD_IMG(128, 4, 2, 1);
#undef ASR_WGRAD_IMG
      h->conv_counts[Cin == 128 ? ASR_CONVP_WGRAD_IMG_128 : mv <= 4 ? ASR_CONVP_WGRAD_IMG_64_SMALL : ASR_CONVP_WGRAD_IMG_64_LARGE] += 1;
      if (Cin == 64 && split_on) h->conv_counts[ASR_CONVP_WGRAD_SPLIT] += 1;
      if (inb) h->conv_counts[ASR_CONVP_WGRAD_BIAS_IN_KERNEL] += 1;
      const size_t total = (size_t)M * N;
      if (inb) {
        const int rb = (int)((total / 4 + 255) / 256);
        if (((uintptr_t)dw) % 16 == 0) {
          hipLaunchKernelGGL(wgrad_img_reduce_kernel<1>, dim3(rb), dim3(256), 0, st, partial, (int)wgs, M, G, N, dw, dbias, accumulate);
          h->conv_counts[ASR_CONVP_WGRAD_REDUCE_VEC] += 1;
        } else {
          hipLaunchKernelGGL(wgrad_img_reduce_kernel<0>, dim3(rb), dim3(256), 0, st, partial, (int)wgs, M, G, N, dw, dbias, accumulate);
          h->conv_counts[ASR_CONVP_WGRAD_REDUCE_SCALAR] += 1;
        }
      } else
        asr_conv_slab_sum(partial, (int)wgs, total, dw, accumulate, st);
      ASR_CHECK_LAUNCH(h, "asr_conv3x3_bwd_weight(image-resident)");
      if (dbias && !inb) return asr_colsum(h, ASR_BF16, dy, Mpix, Cout, Cout, dbias, s);
      return ASR_OK;
    }
  }
  if (wgrad_tr) {
    const size_t lds = (size_t)2 * TN_STAGE;
    auto kern = bn64 ? conv3x3_wgrad_tr_kernel<64> : conv3x3_wgrad_tr_kernel<128>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(tn, tm, S), dim3(256), lds, st, Mpix, H, W, Cin, Cout,
                       (const bf16_t*)x, (const bf16_t*)dy, kchunk, partial);
    h->conv_counts[bn64 ? ASR_CONVP_WGRAD_TR_64 : ASR_CONVP_WGRAD_TR_128] += 1;
  } else {
    asr_conv_wgrad_tiled<Taps33>(x, dy, Mpix, H, W, Cin, Cout, S, kchunk, partial, st);
    h->conv_counts[ASR_CONVP_WGRAD_COLPIX] += 1;
  }
  asr_conv_slab_sum(partial, S, (size_t)M * N, dw, accumulate, st);
  ASR_CHECK_LAUNCH(h, "asr_conv3x3_bwd_weight");
  if (dbias) return asr_colsum(h, ASR_BF16, dy, Mpix, Cout, Cout, dbias, s);
  return ASR_OK;
}
extern "C" int asr_conv3x3_bwd_weight(asr_handle* h, const void* x, const void* dy, int Nimg, int H, int W,
                                      int Cin, int Cout, float* dw, int accumulate, asr_stream s) {
  return conv3x3_bwd_weight_impl(h, x, dy, Nimg, H, W, Cin, Cout, dw, nullptr, accumulate, s);
}
extern "C" int asr_conv3x3_bwd_weight_bias(asr_handle* h, const void* x, const void* dy, int Nimg, int H, int W,
                                           int Cin, int Cout, float* dw, float* dbias, asr_stream s) {
  if (h && !dbias) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_conv3x3_bwd_weight_bias: dbias is NULL");
  return conv3x3_bwd_weight_impl(h, x, dy, Nimg, H, W, Cin, Cout, dw, dbias, 0, s);
}

ASR_DEFINE_COUNTS_N(conv_path_counts, conv_counts)
