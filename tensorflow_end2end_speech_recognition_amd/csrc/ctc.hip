// CTC loss (alpha/beta DP + gradient), greedy decode, row softmax for gfx950.
//
// Replaces tf.nn.ctc_loss (CPU-only kernel in TF1 -> a device->host->device hop every
// step in the reference: models/ctc/ctc.py:289-297, joint_ctc_attention.py:308-316),
// tf.nn.ctc_greedy_decoder (ctc.py:341-342 == models/ctc/decoders/greedy_decoder.py:19-50)
// and tf.nn.softmax in CTC.posteriors (ctc.py:354-380).  blank = C-1.
//
// These are HBM/latency-bound passes over logits[T,B,C]; nothing here is GEMM-shaped:
//   1. row_lse:      one wave per (t,b) row: ln sum exp, and the emission probabilities of the row along the
//                    utterance's blank-extended label sequence (yext)          (1 read of logits)
//   2. alpha_beta:   ONE WAVE per recursion (alpha and beta of an utterance in two single-wave workgroups), LINEAR
//                    domain with a private exponent per state ({fp32 mantissa, int32 exponent}: the range of the
//                    log domain without its exp / log), K consecutive states per lane in registers, lane-boundary
//                    values over wave_shr / wave_shl DPP: no transcendental, no LDS, no barrier on the per-frame chain
//   3. grad:         one wave per (t,b): posterior occupations gamma_t(s) =
//                    alpha beta / (y p) are summed per class in a fixed order
//                    (blank by a wave tree reduction, labels by rank rounds) so the result
//                    is deterministic; writes softmax - occupation   (1 read + 1 write)
// A training step of a CTC model with a narrow head (C <= 64, E % 64 == 0, bf16 operands) runs the stretch between the last
// forward recurrence and the first BPTT kernel as THREE launches and one small product (asr_ctc_head_fwd, then
// asr_ctc_loss_ex):
//   1b. head_fwd:    ctc_head_fwd_kernel -- the top layer's dropout, logits = x W + b on MFMA and pass 1 on the logits tile
//                    while it is in LDS: replaces dropout_apply, the generic GEMM and row_lse (three launches, two queue
//                    gaps, one read pass over the logits) with the same bits
//   2.  alpha_beta   as above
//   3.  grad         ctc_grad_kernel<true> also stores the bf16 operand image [T*B, Kp] of what it writes (zero columns
//                    behind C): no cast pass; d(encoder output) is then the lean NT product image x Wp^T on valid frames
//                    with the top layer's dropout in its epilogue (models/ctc/ctc.py)
// Label smoothing of the head (asr_ctc_loss_ls, an extension) stays inside launch 3 -- ctc_grad_kernel<IMG, true> writes
// softmax - (1 - eps) occupation - eps / C and the row's KL term -- plus one small launch that sums the KL terms per utterance
// (3b); launch 2 is untouched, so the loss it returns is the plain one.
// Headline step (5 x 256, B = 16, T = 745, C = 39): 270 -> 221 us between the two recurrences
// (profiles/r09_ctc_head_tn_frames.md).  Other shapes, fp32 models and asr_ctc_loss keep launches 1, 2, 3.
#include "common.h"
#include <math.h>
#include <stdlib.h>

namespace {

constexpr float NEG_INF = -INFINITY;

constexpr double DNEG_INF = -INFINITY;

// ---- 1. row log-sum-exp + emissions of the extended label sequence ----------
// One wave per (t,b) row: lse[row] = ln sum_k exp(x_k) (fp64), then -- when yext is given -- the emission
// probabilities of the row's utterance along its blank-extended label sequence l' (s even: blank, s odd: label s>>1),
//   yext[b][t][s] = {m, e}: y_t(l'_s) = exp(x[l'_s] - lse) = m * 2^e, m in [0.5, 1] fp32, e int32   for s < S,
//   {0, ME_ZERO} for S <= s < SP  (SP = 64 * K, K states per lane of kernel 2)
// i.e. already in the form the recursion multiplies with.  This is the only thing the serial kernel reads per frame:
// contiguous, prefetchable, no gather and no exp on the chain.  yrev holds the same rows in reversed time order
// (row Tb-1-t): the beta recursion then walks memory forwards exactly like alpha, and the two share one loop body.
constexpr int ME_ZERO = -(1 << 24);      // exponent of the value 0 (any real exponent stays above -126 * T)
struct __attribute__((aligned(8))) MantExp { float m; int e; };

// One wave, one row: p = the row's C logits (global memory in row_lse_kernel, the LDS tile of ctc_head_fwd_kernel).
__device__ __forceinline__ void row_lse_row(const float* p, int row, int lane, int C, double* __restrict__ lse, int T,
                                            int B, const int32_t* __restrict__ labels_flat,
                                            const int32_t* __restrict__ label_offsets,
                                            const int32_t* __restrict__ seq_len, int SP, MantExp* __restrict__ yext,
                                            MantExp* __restrict__ yrev) {
  float m = NEG_INF;
  for (int k = lane; k < C; k += 64) m = fmaxf(m, p[k]);
  m = wave_reduce_max(m);
  double s = 0.0;
  for (int k = lane; k < C; k += 64) s += exp((double)p[k] - (double)m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const double z = (double)m + log(s);
  if (lane == 0) lse[row] = z;
  if (!yext) return;
  const int t = row / B, b = row - t * B;
  const int Tb = min(seq_len[b], T);
  if (t >= Tb) return;                                    // frames past the utterance are never read
  const int lo = label_offsets[b];
  const int S = 2 * (label_offsets[b + 1] - lo) + 1;
  const int32_t* lab = labels_flat + lo;
  MantExp* out = yext + ((size_t)b * T + t) * SP;
  MantExp* outr = yrev + ((size_t)b * T + (Tb - 1 - t)) * SP;   // the same frame where the beta recursion reads it
  const int blank = C - 1;
  for (int st = lane; st < SP; st += 64) {
    MantExp v = {0.f, ME_ZERO};
    if (st < S) {
      const int cls = (st & 1) ? lab[st >> 1] : blank;
      const double l2 = ((double)p[cls] - z) * 1.4426950408889634074;      // log2 y  (<= 0)
      if (l2 > -1.0e7) {                                                    // a logit of -inf: y = 0
        const double fl = floor(l2);
        v.e = (int)fl + 1;
        v.m = (float)exp2(l2 - fl - 1.0);                                   // 2^[-1, 0) = [0.5, 1)
      }
    }
    out[st] = v;
    outr[st] = v;
  }
}

__global__ __launch_bounds__(256) void row_lse_kernel(const float* __restrict__ x, int rows, int C,
                                                      double* __restrict__ lse, int T, int B,
                                                      const int32_t* __restrict__ labels_flat,
                                                      const int32_t* __restrict__ label_offsets,
                                                      const int32_t* __restrict__ seq_len, int SP,
                                                      MantExp* __restrict__ yext, MantExp* __restrict__ yrev,
                                                      int32_t* __restrict__ zero_word = nullptr) {
  // (the counter the recursion kernel adds to is cleared here: as a memset it was one more packet -- 5 us and a queue gap --
  // between the output layer and the recursions)
  if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  row_lse_row(x + (size_t)row * C, row, lane, C, lse, T, B, labels_flat, label_offsets, seq_len, SP, yext, yrev);
}

// ---- 1b. the CTC head in one launch: dropout of the top layer's output, logits = x W + b, and kernel 1 on the tile ---------
// One workgroup (4 waves) per 16 rows of hout [rows, E] bf16 (E % 64 == 0, C <= 64):
//   phase 1  the 16 x E tile, 16 bytes per thread and trip: the dropout multipliers of asr_dropout_apply (word e % 4 of the
//            Philox block at offset + e / 4, e the element's index in the whole tensor; product in fp32, rounded as
//            f32_to_bf16 rounds) -> x_op in memory (the head's weight-gradient product reads every row of it) and the A
//            tile in LDS.  Every element of hout is loaded by exactly one workgroup: the Philox work is done once.
//   phase 2  wave w owns the 16 classes 16 w ..: v_mfma_f32_16x16x32_bf16 over ascending k, operands (B fragment, A
//            fragment) as gemm_kernel issues them -- a lane's eight consecutive k of row / class (lane & 15) at k-slot
//            (lane >> 4) -- so the accumulators hold the bits of asr_gemm's 64 x 64 and 128 x 128 tiles; B fragments are
//            16-byte loads from the class-major weight image Wt [64, E] (rows >= C zero), all of a wave's in flight at once.
//   phase 3  + bias -> logits in memory (every row: callers receive them) and in LDS.
//   phase 4  wave w runs row_lse_row on rows 4 w .. 4 w + 3 of the tile: lse, yext, yrev as row_lse_kernel leaves them.
template <bool DROP>
__global__ __launch_bounds__(256) void ctc_head_fwd_kernel(
    const bf16_t* __restrict__ hout, int rows, int E, float keep, uint64_t seed, uint64_t offset,
    const bf16_t* __restrict__ Wt, const float* __restrict__ bias, int C, bf16_t* __restrict__ x_op,
    float* __restrict__ logits, double* __restrict__ lse, int T, int B, const int32_t* __restrict__ labels_flat,
    const int32_t* __restrict__ label_offsets, const int32_t* __restrict__ seq_len, int SP, MantExp* __restrict__ yext,
    MantExp* __restrict__ yrev, int32_t* __restrict__ zero_word) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int LDA = E + 8;                                   // bf16 elements: 16 bytes of padding per row
  bf16_t* As = reinterpret_cast<bf16_t*>(smem);            // [16][LDA]
  float* Ls = reinterpret_cast<float*>(smem + (size_t)16 * LDA * sizeof(bf16_t));   // [16][64]
  if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * 16;
  // phase 1
  const int vpr = E / 8;                                   // 16-byte vectors per row
  const float inv = 1.f / keep;
  for (int v = tid; v < 16 * vpr; v += 256) {
    const int r = v / vpr, kv = (v - r * vpr) * 8;
    const int row = r0 + r;
    bf16x8_t x = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row < rows) {
      const size_t e0 = (size_t)row * E + kv;
      x = *reinterpret_cast<const bf16x8_t*>(hout + e0);
      if constexpr (DROP) {
        float mk[8];
        asr_dropout_words(offset + e0 / 4, seed, keep, inv, mk);
        asr_dropout_words(offset + e0 / 4 + 1, seed, keep, inv, mk + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (short)f32_to_bf16(bf16_to_f32((bf16_t)x[j]) * mk[j]);
        *reinterpret_cast<bf16x8_t*>(x_op + e0) = x;
      }
    }
    *reinterpret_cast<bf16x8_t*>(As + r * LDA + kv) = x;
  }
  __syncthreads();
  // phase 2 + 3
  const int fr = lane & 15, fq = lane >> 4;
  if (wave * 16 < C) {
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    const bf16_t* wp = Wt + (size_t)(wave * 16 + fr) * E + fq * 8;
    const bf16_t* ap = As + fr * LDA + fq * 8;
    for (int k0 = 0; k0 < E; k0 += 256) {                  // eight 32-wide steps of B fragments in flight
      bf16x8_t b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u * 32 < E) b[u] = *reinterpret_cast<const bf16x8_t*>(wp + k0 + u * 32);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u * 32 < E) {
          const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(ap + k0 + u * 32);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[u], a, acc, 0, 0, 0);
        }
    }
    // lane holds logits[row r0 + fr][class 16 wave + 4 fq + 0..3]
    const int row = r0 + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = wave * 16 + fq * 4 + r;
      if (n < C) {
        const float v = acc[r] + bias[n];
        Ls[fr * 64 + n] = v;
        if (row < rows) logits[(size_t)row * C + n] = v;
      }
    }
  }
  __syncthreads();
  // phase 4
  for (int r = wave * 4; r < wave * 4 + 4; ++r) {
    const int row = r0 + r;
    if (row >= rows) break;
    row_lse_row(Ls + r * 64, row, lane, C, lse, T, B, labels_flat, label_offsets, seq_len, SP, yext, yrev);
  }
}

// the head's weight images from the fp32 variable W [E, C]: Wt [64, E] class-major for ctc_head_fwd_kernel (rows >= C
// zero) and Wp [E, Kp] (Kp = C rounded up to 64, columns >= C zero), the B^T operand of the lean NT product dlogits W^T;
// rounded as the operand shadow of the variable is (f32_to_bf16)
__global__ void ctc_head_images_kernel(const float* __restrict__ W, int E, int C, int Kp, bf16_t* __restrict__ Wt,
                                       bf16_t* __restrict__ Wp) {
  const size_t n = (size_t)E * Kp;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int e = (int)(i / Kp), c = (int)(i % Kp);
    const bf16_t v = c < C ? f32_to_bf16(W[(size_t)e * C + c]) : (bf16_t)0;
    Wp[i] = v;
    if (Wt && c < 64) Wt[(size_t)c * E + e] = v;
  }
}

__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ x,
                                                           float* __restrict__ y, int rows, int C) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = x + (size_t)row * C;
  float m = NEG_INF;
  for (int k = lane; k < C; k += 64) m = fmaxf(m, p[k]);
  m = wave_reduce_max(m);
  float s = 0.f;
  for (int k = lane; k < C; k += 64) s += expf(p[k] - m);
  s = wave_reduce_sum(s);
  const float inv = 1.f / s;
  for (int k = lane; k < C; k += 64) y[(size_t)row * C + k] = expf(p[k] - m) * inv;
}

// ---- 2. alpha / beta recursions --------------------------------------------
// ONE WAVE per recursion (grid = 2 x B workgroups of 64 threads: alpha of utterance b, beta of utterance b), in the
// LINEAR domain:
//   alpha_t(s) = (alpha_{t-1}(s) + alpha_{t-1}(s-1) + [skip] alpha_{t-1}(s-2)) * y_t(l'_s)
// with every state carried as {m, e} = m * 2^e (fp32 mantissa in [0.5, 1], private int32 exponent; 0 = {0, ME_ZERO}).
// That is the range of the log domain (the states of one frame of a peaked model differ by far more than fp64's
// 2^2046: a state that is negligible now can carry the whole likelihood a hundred frames later) without its cost:
// the sum aligns the three terms to their largest exponent (v_max3, 3 v_sub, 3 v_ldexp), the product adds exponents,
// v_frexp_* renormalises -- ~16 full-rate instructions per state and frame, no exp / log.  (The log-domain form this
// replaces spent ~1.1k cycles per frame in three exp + one log behind an LDS round trip and a 512-thread barrier.)
// Lane i owns the K consecutive states K*i .. K*i+K-1 in registers; the two states that cross a lane boundary move
// with wave_shr:1 / wave_shl:1 DPP -- no LDS, no barrier.  The recursion is started from a virtual frame
// (alpha_{-1} = indicator of state 0, beta_T = indicator of state S-1), which yields the usual initial rows.
// Emissions come from yext (kernel 1) through a register ring D frames deep; the main loop body is D frames of
// straight-line code (static ring registers, exact s_waitcnt counts), the < D remaining frames run from the ring.
// Per-frame precision: ~4 roundings of 2^-24 -> ~1e-5 relative on p(l|x) after 1000 frames, i.e. ~1e-8 relative on
// the loss; -ln p = -(ln(m1 2^(e1-E) + m2 2^(e2-E)) + E ln 2) over the two final states, in fp64.
__device__ __forceinline__ float dpp_shift_f(float v, bool right) {
  return __builtin_bit_cast(float, right ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, false)
                                         : __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xF, 0xF, false));
}
__device__ __forceinline__ int dpp_shift_e(int v, bool right) {   // the lane without a source gets the exponent of 0
  return right ? __builtin_amdgcn_update_dpp(ME_ZERO, v, 0x138, 0xF, 0xF, false)
               : __builtin_amdgcn_update_dpp(ME_ZERO, v, 0x130, 0xF, 0xF, false);
}

// Round 6: NW waves per recursion.  With long label sequences (S = 2 L + 1 up to 801 states at cfg D: K = 16 states per lane) a
// frame is K x ~16 dependent-ish instructions of ONE wave: 0.7 us at K = 8 (cfg C), 1.2 ms of a 58 ms step on the critical
// path between the forward and the backward pass.  The states are dealt over NW x 64 lanes instead (K / NW per lane, lane
// index = wave * 64 + lane); the two states that cross a WAVE boundary go through LDS (double-buffered by frame parity) behind
// ONE workgroup barrier per frame.  Same operands, same operations per state: the values are bit-identical to NW = 1.
struct CtcEdge { float m1, m2; int e1, e2; };
// ybase / ws: rows in RECURSION order (step 0, 1, ...): for beta that is reversed time (row i = frame Tb-1-i).
// `lane` is the lane index over all NW waves (0 .. 64 NW - 1); SPW = states per frame in memory (64 NW K).
template <int K, int D, bool BETA, int NW>
__device__ __forceinline__ void ctc_recursion(const MantExp* __restrict__ ybase, MantExp* __restrict__ ws, int Tb,
                                              int S, int lane, const int32_t* __restrict__ lab, float (&am)[K],
                                              int (&ae)[K], CtcEdge (*edge)[NW]) {
  constexpr int SP = 64 * K * NW;
  const int wave = lane >> 6, wl = lane & 63;
  // exponent offset of the skip term: 0 where the transition s-2 -> s (beta: s+2 -> s) exists, else "times 0"
  int skoff[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = K * lane + k;
    bool ok = false;
    if ((s & 1) && s < S) {
      if (!BETA) ok = s >= 3 && lab[s >> 1] != lab[(s >> 1) - 1];
      else ok = s + 2 < S && lab[s >> 1] != lab[(s >> 1) + 1];
    }
    skoff[k] = ok ? 0 : ME_ZERO;
  }
  // virtual start frame
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = K * lane + k;
    const bool on = BETA ? (s == S - 1) : (s == 0);
    am[k] = on ? 0.5f : 0.f;
    ae[k] = on ? 1 : ME_ZERO;
  }
  float rm[D][K];
  int re[D][K];
  auto fetch = [&](int slot, int step) {                   // emissions of recursion step `step` (clamped: no branch)
    const MantExp* src = ybase + (size_t)min(step, Tb - 1) * SP;
#pragma unroll
    for (int k = 0; k < K; ++k) { const MantExp v = src[k]; rm[slot][k] = v.m; re[slot][k] = v.e; }
  };
  auto frame = [&](int slot, int step) {
    float nm[K];
    int ne[K];
    // (K = 1: the second neighbour state is the first state of the lane TWO away; not instantiated, K >= 2 here)
    float p1m = dpp_shift_f(BETA ? am[0] : am[K - 1], !BETA), p2m = dpp_shift_f(BETA ? am[1] : am[K - 2], !BETA);
    int p1e = dpp_shift_e(BETA ? ae[0] : ae[K - 1], !BETA), p2e = dpp_shift_e(BETA ? ae[1] : ae[K - 2], !BETA);
    if constexpr (NW > 1) {
      // the lane at the wave's edge publishes what its neighbour WAVE needs, the lane at the other edge picks it up.
      // (Measured: computing the frame's states under the barrier and redoing the two edge states behind it is slower --
      // 1 219 against 1 177 us per call at cfg C: the frame is the LDS -> barrier -> LDS chain, not the state arithmetic.)
      CtcEdge* row = edge[step & 1];
      if (wl == (BETA ? 0 : 63)) row[wave] = (CtcEdge){BETA ? am[0] : am[K - 1], BETA ? am[1] : am[K - 2],
                                                        BETA ? ae[0] : ae[K - 1], BETA ? ae[1] : ae[K - 2]};
      __syncthreads();
      const int nbw = BETA ? wave + 1 : wave - 1;
      if (nbw >= 0 && nbw < NW) {                         // wave-uniform
        const CtcEdge nb = row[nbw];
        const bool at = wl == (BETA ? 63 : 0);
        p1m = at ? nb.m1 : p1m;  p2m = at ? nb.m2 : p2m;
        p1e = at ? nb.e1 : p1e;  p2e = at ? nb.e2 : p2e;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float m1, m2;
      int e1, e2;
      if (!BETA) {
        m1 = k >= 1 ? am[k - 1] : p1m;  e1 = k >= 1 ? ae[k - 1] : p1e;
        m2 = k >= 2 ? am[k - 2] : (k == 1 ? p1m : p2m);  e2 = k >= 2 ? ae[k - 2] : (k == 1 ? p1e : p2e);
      } else {
        m1 = k + 1 < K ? am[k + 1] : p1m;  e1 = k + 1 < K ? ae[k + 1] : p1e;
        m2 = k + 2 < K ? am[k + 2] : (k + 2 == K ? p1m : p2m);  e2 = k + 2 < K ? ae[k + 2] : (k + 2 == K ? p1e : p2e);
      }
      e2 += skoff[k];
      const int E = max(max(ae[k], e1), e2);
      const float sum = ldexpf(am[k], ae[k] - E) + ldexpf(m1, e1 - E) + ldexpf(m2, e2 - E);
      const float pr = sum * rm[slot][k];
      nm[k] = __builtin_amdgcn_frexp_mantf(pr);
      ne[k] = pr > 0.f ? E + re[slot][k] + __builtin_amdgcn_frexp_expf(pr) : ME_ZERO;
    }
    MantExp* dst = ws + (size_t)step * SP;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      am[k] = nm[k];
      ae[k] = ne[k];
      dst[k] = (MantExp){nm[k], ne[k]};
    }
  };
#pragma unroll
  for (int j = 0; j < D; ++j) fetch(j, j);
  int base = 0;
  for (; base + D <= Tb; base += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      frame(j, base + j);
      fetch(j, base + j + D);
    }
  }
#pragma unroll
  for (int j = 0; j < D; ++j)
    if (base + j < Tb) frame(j, base + j);                 // wave-uniform; slot j holds frame base + j
}

template <int K, int D, int NW = 1>
__global__ __launch_bounds__(64 * NW) void ctc_alpha_beta_kernel(
    const MantExp* __restrict__ yext, const MantExp* __restrict__ yrev, int T, int B, int C,
    const int32_t* __restrict__ labels_flat, const int32_t* __restrict__ label_offsets,
    const int32_t* __restrict__ seq_len, int Lcap, MantExp* __restrict__ alpha_ws, MantExp* __restrict__ beta_ws, int32_t* __restrict__ rank_ws,
    double* __restrict__ ll_ws, float* __restrict__ loss, int32_t* __restrict__ num_infeasible) {
  constexpr int SP = 64 * K * NW;
  static_assert(K >= 2, "two states cross a lane boundary");
  __shared__ CtcEdge edge[2][NW];
  __shared__ CtcEdge fin[NW];
  const int b = blockIdx.x >> 1;
  const bool is_beta = blockIdx.x & 1;
  const int lane = threadIdx.x;                            // over all NW waves
  const int lo = label_offsets[b];
  const int L = label_offsets[b + 1] - lo;
  const int S = 2 * L + 1;
  const int Tb = min(seq_len[b], T);
  const int32_t* lab = labels_flat + lo;

  if (!is_beta) {
    // rank of each label among equal earlier labels (fixed summation order in the grad kernel) and the position of
    // the first label of its class (where the grad kernel accumulates that class), packed rank | first << 16
    for (int i = lane; i < L && i < Lcap; i += 64 * NW) {
      const int li = lab[i];
      int r = 0, first = i;
      for (int k = i - 1; k >= 0; --k)
        if (lab[k] == li) { ++r; first = k; }
      rank_ws[(size_t)b * (Lcap > 0 ? Lcap : 1) + i] = r | (first << 16);
    }
  }
  if (Tb <= 0 || L > Lcap || S > SP) {
    if (!is_beta && lane == 0) {
      loss[b] = 0.f;
      ll_ws[b] = DNEG_INF;
      if (num_infeasible && Tb > 0) atomicAdd(num_infeasible, 1);
    }
    return;
  }
  const MantExp* ybase = (is_beta ? yrev : yext) + (size_t)b * T * SP + K * lane;
  float am[K];
  int ae[K];
  if (is_beta) {
    ctc_recursion<K, D, true, NW>(ybase, beta_ws + (size_t)b * T * SP + K * lane, Tb, S, lane, lab, am, ae, edge);
    return;
  }
  ctc_recursion<K, D, false, NW>(ybase, alpha_ws + (size_t)b * T * SP + K * lane, Tb, S, lane, lab, am, ae, edge);
  // p = alpha_T(S-1) + alpha_T(S-2): the two states live in lanes (S-1)/K and (S-2)/K
  float m1 = 0.f, m2 = 0.f;
  int e1 = ME_ZERO, e2 = ME_ZERO;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s = K * lane + k;
    if (s == S - 1) { m1 = am[k]; e1 = ae[k]; }
    if (s == S - 2) { m2 = am[k]; e2 = ae[k]; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                       // every lane but the owners holds {0, ME_ZERO}
    const float om1 = __shfl_xor(m1, o, 64), om2 = __shfl_xor(m2, o, 64);
    const int oe1 = __shfl_xor(e1, o, 64), oe2 = __shfl_xor(e2, o, 64);
    if (oe1 > e1) { m1 = om1; e1 = oe1; }
    if (oe2 > e2) { m2 = om2; e2 = oe2; }
  }
  if constexpr (NW > 1) {                                  // the owners of the two final states may sit in different waves
    if ((lane & 63) == 0) fin[lane >> 6] = (CtcEdge){m1, m2, e1, e2};
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        if (fin[w].e1 > e1) { m1 = fin[w].m1; e1 = fin[w].e1; }
        if (fin[w].e2 > e2) { m2 = fin[w].m2; e2 = fin[w].e2; }
      }
    }
  }
  if (lane == 0) {
    const int E = max(e1, e2);
    const bool ok = E > ME_ZERO;
    double ll = DNEG_INF;
    if (ok) ll = log(ldexp((double)m1, e1 - E) + ldexp((double)m2, e2 - E)) + (double)E * 0.6931471805599453094;
    loss[b] = ok ? (float)(-ll) : 0.f;
    ll_ws[b] = ll;
    if (!ok && num_infeasible) atomicAdd(num_infeasible, 1);
  }
}

// ---- 3. gradient -------------------------------------------------------------
// IMG: every value written to grad also goes, rounded as asr_cast_from_f32 rounds it, to the bf16 image gimg [T*B, Kp]
// (Kp >= C a multiple of 64, columns C .. Kp-1 zero in every row): the operand of the products that consume dlogits,
// without a cast pass over grad.
// LS (asr_ctc_loss_ls, an EXTENSION: label smoothing towards the uniform distribution over all C classes): the row's value
// becomes softmax - om * occupation - eC (om = 1 - eps, eC = eps / C), and lane 0 leaves the row's term of
// KL(uniform || softmax) = lse - mean_k x_k - ln C in klrow[t * B + b] (fp64; rows of padded frames and of infeasible
// utterances are not written and ctc_kl_finish_kernel does not read them).  LS = false reads none of om, eC, klrow.
template <bool IMG, bool LS = false>
__global__ __launch_bounds__(256) void ctc_grad_kernel(
    const float* __restrict__ logits, const double* __restrict__ lse, int T, int B, int C,
    const int32_t* __restrict__ labels_flat, const int32_t* __restrict__ label_offsets,
    const int32_t* __restrict__ seq_len, int SW, int SP, const MantExp* __restrict__ yext,
    const MantExp* __restrict__ alpha_ws, const MantExp* __restrict__ beta_ws,
    const int32_t* __restrict__ rank_ws, const double* __restrict__ ll_ws, float grad_scale,
    float* __restrict__ grad, bf16_t* __restrict__ gimg, int Kp, float om = 1.f, float eC = 0.f,
    double* __restrict__ klrow = nullptr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // Per wave: gam[SW] (state occupations), acc[(SW-1)/2] (occupation of a class, kept at the position of its FIRST
  // label) and a C-bit membership map of the label classes.  Nothing is sized by C x 4 bytes, so word-level
  // vocabularies (C = 18-27 k classes, examples/librispeech) fit: 4 x (SW + Lmax + C/32) words of LDS.
  const int LW = (SW - 1) / 2, BW = (C + 31) / 32;
  float* gam = reinterpret_cast<float*>(smem) + (size_t)wave * (SW + LW + BW);
  float* acc = gam + SW;
  unsigned* bits = reinterpret_cast<unsigned*>(acc + LW);
  const int b = blockIdx.y;
  const int t = blockIdx.x * 4 + wave;
  if (t >= T) return;
  float* g = grad + ((size_t)t * B + b) * C;
  bf16_t* gi = IMG ? gimg + ((size_t)t * B + b) * Kp : nullptr;
  auto put = [&](int k, float v) {
    g[k] = v;
    if constexpr (IMG) gi[k] = f32_to_bf16(v);
  };
  if constexpr (IMG) {
    for (int k = C + lane; k < Kp; k += 64) gi[k] = 0;
  }
  const int Tb = min(seq_len[b], T);
  const double ll = ll_ws[b];
  if (t >= Tb || !(ll > DNEG_INF)) {
    for (int k = lane; k < C; k += 64) put(k, 0.f);
    return;
  }
  const int lo = label_offsets[b];
  const int L = label_offsets[b + 1] - lo;
  const int S = 2 * L + 1;
  const int blank = C - 1;
  const int32_t* lab = labels_flat + lo;
  const int32_t* rk = rank_ws + (size_t)b * (LW > 0 ? LW : 1);
  const float* row = logits + ((size_t)t * B + b) * C;
  const double z = lse[(size_t)t * B + b];
  const MantExp* al = alpha_ws + ((size_t)b * T + t) * SP;
  const MantExp* be = beta_ws + ((size_t)b * T + (Tb - 1 - t)) * SP;   // stored in recursion order
  const MantExp* ye = yext + ((size_t)b * T + t) * SP;

  for (int k = lane; k < BW; k += 64) bits[k] = 0u;
  for (int i = lane; i < L; i += 64) acc[i] = 0.f;
  float blank_sum = 0.f;
  int maxrank = 0;
  for (int s = lane; s < S; s += 64) {
    // gamma_t(s) = alpha_t(s) beta_t(s) / (y_t(s) p): mantissas in fp64, exponents as integers, ln p = ll
    const MantExp av = al[s], bv = be[s], yv = ye[s];
    float gm = 0.f;
    if (av.m > 0.f && bv.m > 0.f)
      gm = (float)((double)av.m * (double)bv.m / (double)yv.m *
                   exp((double)(av.e + bv.e - yv.e) * 0.6931471805599453094 - ll));
    gam[s] = gm;
    if (!(s & 1)) blank_sum += gm;
    else maxrank = max(maxrank, rk[s >> 1] & 0xffff);
  }
  blank_sum = wave_reduce_sum(blank_sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) maxrank = max(maxrank, __shfl_xor(maxrank, o, 64));
  __builtin_amdgcn_wave_barrier();
  // labels: round r adds the r-th occurrence of every class to the slot of its first occurrence -> no two lanes
  // touch one slot in a round, and the summation order is fixed (deterministic)
  for (int r = 0; r <= maxrank; ++r) {
    for (int i = lane; i < L; i += 64) {
      const int pk = rk[i];
      if ((pk & 0xffff) == r) {
        acc[pk >> 16] += gam[2 * i + 1];
        if (r == 0) atomicOr(&bits[lab[i] >> 5], 1u << (lab[i] & 31));
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  // classes that are not labels (and not blank): softmax only; every address below is written exactly once
  if constexpr (LS) {                                      // (the same three kinds of class, smoothed)
    double sx = 0.0;                                       // the row sum of the KL term rides on the pass over the classes
    for (int k = lane; k < C; k += 64) {
      const double x = (double)row[k];
      sx += x;
      if (k == blank) put(k, ((float)exp(x - z) - om * blank_sum - eC) * grad_scale);
      else if (!((bits[k >> 5] >> (k & 31)) & 1u)) put(k, ((float)exp(x - z) - eC) * grad_scale);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sx += __shfl_xor(sx, o, 64);
    if (lane == 0) klrow[(size_t)t * B + b] = z - sx / (double)C - log((double)C);
    for (int i = lane; i < L; i += 64) {
      if ((rk[i] & 0xffff) == 0) {
        const int k = lab[i];
        put(k, ((float)exp((double)row[k] - z) - om * acc[i] - eC) * grad_scale);
      }
    }
    return;
  }
  for (int k = lane; k < C; k += 64) {
    if (k == blank) put(k, ((float)exp((double)row[k] - z) - blank_sum) * grad_scale);
    else if (!((bits[k >> 5] >> (k & 31)) & 1u)) put(k, (float)exp((double)row[k] - z) * grad_scale);
  }
  for (int i = lane; i < L; i += 64) {
    if ((rk[i] & 0xffff) == 0) {
      const int k = lab[i];
      put(k, ((float)exp((double)row[k] - z) - acc[i]) * grad_scale);
    }
  }
}

// ---- 3b. label smoothing: the KL term per utterance ---------------------------------------------------------------------
// The row terms of a call WITHOUT a gradient (want_grad = False: dev-style calls of the op itself): one wave per valid
// (t, b) row, the sum ctc_grad_kernel<.., true> forms, in the same order -> the same bits.
__global__ __launch_bounds__(256) void ctc_kl_rows_kernel(const float* __restrict__ logits, const double* __restrict__ lse,
                                                          int T, int B, int C, const int32_t* __restrict__ seq_len,
                                                          double* __restrict__ klrow) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= T * B) return;
  const int t = r / B, b = r - t * B;
  if (t >= min(seq_len[b], T)) return;                       // frames past the utterance are never read
  const float* row = logits + (size_t)r * C;
  double sx = 0.0;
  for (int k = lane; k < C; k += 64) sx += (double)row[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sx += __shfl_xor(sx, o, 64);
  if (lane == 0) klrow[r] = lse[r] - sx / (double)C - log((double)C);
}

// kl[b] = sum over the utterance's frames of klrow, one workgroup per utterance: thread i adds frames i, i + 256, ... in
// ascending order, then a fixed tree over the 256 partial sums -- no atomics, the same bits on every call.  Infeasible and
// empty utterances get 0 (their rows were never written).
__global__ __launch_bounds__(256) void ctc_kl_finish_kernel(const double* __restrict__ klrow, int T, int B,
                                                            const int32_t* __restrict__ seq_len,
                                                            const double* __restrict__ ll_ws, float* __restrict__ kl) {
  __shared__ double part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = min(seq_len[b], T);
  const bool ok = Tb > 0 && ll_ws[b] > DNEG_INF;
  double s = 0.0;
  if (ok)
    for (int t = tid; t < Tb; t += 256) s += klrow[(size_t)t * B + b];
  part[tid] = s;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) kl[b] = ok ? (float)part[0] : 0.f;
}

// ---- greedy decode -------------------------------------------------------------
// tf.nn.ctc_greedy_decoder (ctc.py:341-342) / GreedyDecoder (greedy_decoder.py:19-50): per-frame argmax (first maximum
// wins), collapse repeats, drop blanks.  Two launches:
//  1. ctc_argmax_kernel -- one WAVE per valid (t, b) row over the whole grid: the only pass over the logits, HBM-bound
//     (a 3 387-class row is 13.5 KB: with one workgroup per utterance -- the first version -- 8 utterances kept 8 CUs busy
//     and the pass ran at 24 GB/s); writes the frame's argmax to out_labels[b, t], which serves as the scratch row;
//  2. ctc_collapse_kernel -- one workgroup per utterance: its row of argmaxes -> LDS, ordered compaction back into
//     out_labels[b, :n], -1 behind it.
__global__ __launch_bounds__(256) void ctc_argmax_kernel(const float* __restrict__ logits, int T, int B, int C,
                                                         const int32_t* __restrict__ seq_len,
                                                         int32_t* __restrict__ out_labels) {
  const int lane = threadIdx.x & 63;
  const size_t nrows = (size_t)T * B;
  for (size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < nrows; row += (size_t)gridDim.x * 4) {
    const int t = (int)(row / B), b = (int)(row % B);
    if (t >= min(max(seq_len[b], 0), T)) continue;       // wave-uniform
    const float* p = logits + row * C;
    float best = NEG_INF;
    int bi = 0x7fffffff;
    for (int k = lane; k < C; k += 64) {
      const float v = p[k];
      if (v > best || (v == best && k < bi)) { best = v; bi = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) out_labels[(size_t)b * T + t] = (bi == 0x7fffffff) ? 0 : bi;
  }
}

__global__ __launch_bounds__(256) void ctc_collapse_kernel(int T, const int32_t* __restrict__ seq_len, int blank,
                                                           int32_t* __restrict__ out_labels,
                                                           int32_t* __restrict__ out_len) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* am = reinterpret_cast<int32_t*>(smem);  // [T] per-frame argmax
  __shared__ int32_t wsum[4];
  __shared__ int32_t carry;
  const int b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int Tb = min(max(seq_len[b], 0), T);
  for (int t = threadIdx.x; t < Tb; t += 256) am[t] = out_labels[(size_t)b * T + t];
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  // ordered compaction, 256 frames per pass
  for (int base = 0; base < Tb; base += 256) {
    const int t = base + threadIdx.x;
    int keep = 0, a = 0;
    if (t < Tb) {
      a = am[t];
      keep = (a != blank) && (t == 0 || a != am[t - 1]);
    }
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = carry;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (keep) out_labels[(size_t)b * T + off + before] = a;
    __syncthreads();
    if (threadIdx.x == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  const int n = carry;
  for (int i = n + threadIdx.x; i < T; i += 256) out_labels[(size_t)b * T + i] = -1;
  if (threadIdx.x == 0) out_len[b] = n;
}

// states per lane of the recursion kernel for an extended label sequence of SW = 2 Lmax + 1 states (0: too long)
inline int ctc_states_per_lane(int SW) {
  const int ks[7] = {3, 6, 8, 12, 16, 24, 32};
  for (int i = 0; i < 7; ++i)
    if (64 * ks[i] >= SW) return ks[i];
  return 0;
}
struct CtcWs {
  size_t lse, yext, yrev, alpha, beta, rank, ll, total;
  int K;
};
inline CtcWs ctc_ws_layout(int T, int B, int Lmax) {
  const int SW = 2 * Lmax + 1;
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  CtcWs w;
  w.K = ctc_states_per_lane(SW);
  const size_t SP = 64 * (size_t)(w.K ? w.K : 32);
  size_t o = 0;
  w.lse = o;   o += al((size_t)T * B * 8);
  w.yext = o;  o += al((size_t)B * T * SP * sizeof(MantExp));
  w.yrev = o;  o += al((size_t)B * T * SP * sizeof(MantExp));
  w.alpha = o; o += al((size_t)B * T * SP * sizeof(MantExp));
  w.beta = o;  o += al((size_t)B * T * SP * sizeof(MantExp));
  w.rank = o;  o += al((size_t)B * (Lmax > 0 ? Lmax : 1) * 4);
  w.ll = o;    o += al((size_t)B * 8);
  w.total = o;
  return w;
}
// asr_ctc_loss_ls: the plain layout (what asr_ctc_head_fwd writes stays a prefix) and behind it the KL row terms [T*B] fp64
inline size_t ctc_ls_ws_total(int T, int B, int Lmax) {
  return ctc_ws_layout(T, B, Lmax).total + ((size_t)T * B * 8 + 255) / 256 * 256;
}
struct CtcLs { float smoothing; float* kl; };

}  // namespace

extern "C" size_t asr_ctc_workspace_bytes(int T, int B, int max_label_len) {
  if (T < 0 || B < 0 || max_label_len < 0) return 0;
  return ctc_ws_layout(T, B, max_label_len).total;
}

extern "C" size_t asr_ctc_ls_workspace_bytes(int T, int B, int max_label_len) {
  if (T < 0 || B < 0 || max_label_len < 0) return 0;
  return ctc_ls_ws_total(T, B, max_label_len);
}

// lse_done: kernel 1 has already run on this workspace (asr_ctc_head_fwd); gimg / Kp: the bf16 image of grad (or NULL);
// ls: asr_ctc_loss_ls only (NULL: the plain loss, which reads nothing of it)
static int ctc_loss_impl(asr_handle* h, const float* logits, int T, int B, int C,
                         const int32_t* labels_flat, const int32_t* label_offsets,
                         const int32_t* seq_len, int max_label_len, float grad_scale, float* loss,
                         float* grad, int32_t* num_infeasible, void* workspace,
                         size_t workspace_bytes, int lse_done, void* gimg, int Kp, asr_stream s,
                         const CtcLs* ls = nullptr) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!logits || !label_offsets || !seq_len || !loss || T <= 0 || B <= 0 || C < 2 ||
      max_label_len < 0 || (max_label_len > 0 && !labels_flat))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_loss: bad args T=%d B=%d C=%d Lmax=%d", T, B, C, max_label_len);
  const int SW = 2 * max_label_len + 1;
  const CtcWs w = ctc_ws_layout(T, B, max_label_len);
  if (!w.K) ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_ctc_loss: label length %d > %d", max_label_len, (64 * 32 - 1) / 2);
  if (!workspace || workspace_bytes < w.total)
    ASR_FAIL(h, ASR_ERR_WORKSPACE, "asr_ctc_loss: workspace %zu < %zu bytes", workspace_bytes, w.total);
  if (ls && workspace_bytes < ctc_ls_ws_total(T, B, max_label_len))
    ASR_FAIL(h, ASR_ERR_WORKSPACE, "asr_ctc_loss_ls: workspace %zu < %zu bytes (asr_ctc_ls_workspace_bytes)", workspace_bytes,
             ctc_ls_ws_total(T, B, max_label_len));
  char* ws = (char*)workspace;
  double* lse = (double*)(ws + w.lse);
  MantExp* yext = (MantExp*)(ws + w.yext);
  MantExp* yrev = (MantExp*)(ws + w.yrev);
  MantExp* alpha = (MantExp*)(ws + w.alpha);
  MantExp* beta = (MantExp*)(ws + w.beta);
  int32_t* rank = (int32_t*)(ws + w.rank);
  double* ll = (double*)(ws + w.ll);
  hipStream_t st = (hipStream_t)s;
  const int rows = T * B;
  const int SP = 64 * w.K;
  if (!lse_done) {
    hipLaunchKernelGGL(row_lse_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, logits, rows, C, lse, T, B, labels_flat,
                       label_offsets, seq_len, SP, yext, yrev, num_infeasible);
    ASR_CHECK_LAUNCH(h, "asr_ctc_loss(row_lse)");
  }
  {
#define ASR_AB(KV, DV, NWV)                                                                              \
  hipLaunchKernelGGL((ctc_alpha_beta_kernel<KV, DV, NWV>), dim3(2 * B), dim3(64 * NWV), 0, st, yext, yrev, T, B, C, labels_flat, \
                     label_offsets, seq_len, max_label_len, alpha, beta, rank, ll, loss, num_infeasible)
    // ASR_CTC_WAVES=1: one wave per recursion whatever the label length (round 5; A/B and the bit-identity test)
    const char* env_w = getenv("ASR_CTC_WAVES");            // (read per call: the bit-identity test flips it inside one process)
    const bool multi = !(env_w && env_w[0] == '1');
    if (multi && w.K >= 6) {
      switch (w.K) {                          // K states per lane of ONE wave = K / NW per lane of NW waves
        case 6: ASR_AB(3, 8, 2); break;
        case 8: ASR_AB(2, 8, 4); break;
        case 12: ASR_AB(3, 8, 4); break;
        case 16: ASR_AB(4, 8, 4); break;
        case 24: ASR_AB(6, 4, 4); break;
        default: ASR_AB(8, 4, 4); break;
      }
    } else {
      switch (w.K) {
        case 3: ASR_AB(3, 8, 1); break;       // D frames of emissions in flight: D * K * 2 ring registers
        case 6: ASR_AB(6, 4, 1); break;
        case 8: ASR_AB(8, 4, 1); break;
        case 12: ASR_AB(12, 4, 1); break;
        case 16: ASR_AB(16, 3, 1); break;
        case 24: ASR_AB(24, 2, 1); break;
        default: ASR_AB(32, 2, 1); break;
      }
    }
#undef ASR_AB
  }
  ASR_CHECK_LAUNCH(h, "asr_ctc_loss(alpha_beta)");
  if (grad) {
    const size_t lds_g = (size_t)4 * (SW + (SW - 1) / 2 + (C + 31) / 32) * sizeof(float);
    if (lds_g > 160 * 1024)
      ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_ctc_loss: C=%d, Lmax=%d need %zu B of LDS", C, max_label_len, lds_g);
    if (ls) {
      double* klrow = (double*)(ws + w.total);
      const float om = 1.f - ls->smoothing, eC = ls->smoothing / (float)C;
#define ASR_GRAD_LS(IMG_, GI_, KP_)                                                                                          \
  do {                                                                                                                       \
    (void)hipFuncSetAttribute((const void*)ctc_grad_kernel<IMG_, true>, hipFuncAttributeMaxDynamicSharedMemorySize,          \
                              (int)lds_g);                                                                                   \
    hipLaunchKernelGGL((ctc_grad_kernel<IMG_, true>), dim3((T + 3) / 4, B), dim3(256), lds_g, st, logits, lse, T, B, C,      \
                       labels_flat, label_offsets, seq_len, SW, SP, yext, alpha, beta, rank, ll, grad_scale, grad, GI_, KP_, \
                       om, eC, klrow);                                                                                       \
  } while (0)
      if (gimg) ASR_GRAD_LS(true, (bf16_t*)gimg, Kp); else ASR_GRAD_LS(false, (bf16_t*)nullptr, 0);
#undef ASR_GRAD_LS
    } else if (gimg) {
      (void)hipFuncSetAttribute((const void*)ctc_grad_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g);
      hipLaunchKernelGGL(ctc_grad_kernel<true>, dim3((T + 3) / 4, B), dim3(256), lds_g, st, logits, lse, T, B, C,
                         labels_flat, label_offsets, seq_len, SW, SP, yext, alpha, beta, rank, ll, grad_scale, grad,
                         (bf16_t*)gimg, Kp);
    } else {
      (void)hipFuncSetAttribute((const void*)ctc_grad_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g);
      hipLaunchKernelGGL(ctc_grad_kernel<false>, dim3((T + 3) / 4, B), dim3(256), lds_g, st, logits, lse, T, B, C,
                         labels_flat, label_offsets, seq_len, SW, SP, yext, alpha, beta, rank, ll, grad_scale, grad,
                         (bf16_t*)nullptr, 0);
    }
    ASR_CHECK_LAUNCH(h, "asr_ctc_loss(grad)");
  }
  if (ls) {
    double* klrow = (double*)(ws + w.total);
    if (!grad) {
      hipLaunchKernelGGL(ctc_kl_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, logits, lse, T, B, C, seq_len, klrow);
      ASR_CHECK_LAUNCH(h, "asr_ctc_loss_ls(kl_rows)");
    }
    hipLaunchKernelGGL(ctc_kl_finish_kernel, dim3(B), dim3(256), 0, st, klrow, T, B, seq_len, ll, ls->kl);
    ASR_CHECK_LAUNCH(h, "asr_ctc_loss_ls(kl_finish)");
  }
  return ASR_OK;
}

extern "C" int asr_ctc_loss(asr_handle* h, const float* logits, int T, int B, int C,
                            const int32_t* labels_flat, const int32_t* label_offsets,
                            const int32_t* seq_len, int max_label_len, float grad_scale, float* loss,
                            float* grad, int32_t* num_infeasible, void* workspace,
                            size_t workspace_bytes, asr_stream s) {
  if (h) h->ctc_head_counts[2] += 1;
  return ctc_loss_impl(h, logits, T, B, C, labels_flat, label_offsets, seq_len, max_label_len, grad_scale, loss, grad,
                       num_infeasible, workspace, workspace_bytes, 0, nullptr, 0, s);
}

extern "C" int asr_ctc_loss_ex(asr_handle* h, const float* logits, int T, int B, int C,
                               const int32_t* labels_flat, const int32_t* label_offsets,
                               const int32_t* seq_len, int max_label_len, float grad_scale, float* loss,
                               float* grad, int32_t* num_infeasible, void* workspace,
                               size_t workspace_bytes, int lse_done, void* grad_bf16, int Kp, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (grad_bf16 && (!grad || Kp < C || Kp % 64 != 0))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_loss_ex: the bf16 image needs grad and Kp = %d >= C = %d, Kp %% 64 == 0", Kp, C);
  h->ctc_head_counts[1] += 1;
  return ctc_loss_impl(h, logits, T, B, C, labels_flat, label_offsets, seq_len, max_label_len, grad_scale, loss, grad,
                       num_infeasible, workspace, workspace_bytes, lse_done, grad_bf16, Kp, s);
}

// asr_ctc_loss_ex's arguments plus the smoothing eps in (0, 1) and kl [B]: loss stays the UNSMOOTHED CTC loss (the recursion
// launch is the plain one), grad = grad_scale (softmax - (1 - eps) occupation - eps / C), kl[b] = sum_t KL(uniform || softmax).
// Launches: [row_lse] alpha_beta grad kl_finish with a gradient (one more than asr_ctc_loss_ex), [row_lse] alpha_beta kl_rows
// kl_finish without.
extern "C" int asr_ctc_loss_ls(asr_handle* h, const float* logits, int T, int B, int C, const int32_t* labels_flat,
                               const int32_t* label_offsets, const int32_t* seq_len, int max_label_len, float grad_scale,
                               float smoothing, float* loss, float* kl, float* grad, int32_t* num_infeasible,
                               void* workspace, size_t workspace_bytes, int lse_done, void* grad_bf16, int Kp,
                               asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!(smoothing > 0.f && smoothing < 1.f))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_loss_ls: smoothing = %g outside (0, 1)", (double)smoothing);
  if (!kl) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_loss_ls: kl is NULL");
  if (grad_bf16 && (!grad || Kp < C || Kp % 64 != 0))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_loss_ls: the bf16 image needs grad and Kp = %d >= C = %d, Kp %% 64 == 0", Kp, C);
  h->ctc_ls_counts[0] += 1;
  if (lse_done) h->ctc_ls_counts[1] += 1;
  if (!grad) h->ctc_ls_counts[2] += 1;
  const CtcLs ls = {smoothing, kl};
  return ctc_loss_impl(h, logits, T, B, C, labels_flat, label_offsets, seq_len, max_label_len, grad_scale, loss, grad,
                       num_infeasible, workspace, workspace_bytes, lse_done, grad_bf16, Kp, s, &ls);
}

// today's logits product of the shape runs asr_gemm's generic kernel in ONE pass over K (no split-K slabs), whose
// accumulators ctc_head_fwd_kernel reproduces; a shape it would split keeps the separate launches
extern "C" int asr_ctc_head_ok(int rows, int E, int C) {
  if (rows < 1 || E < 64 || E % 64 != 0 || E > 1024 || C < 2 || C > 64) return 0;
  const long tiles128 = (long)((rows + 127) / 128) * ((C + 127) / 128);
  const long tiles64 = (long)((rows + 63) / 64) * ((C + 63) / 64);
  if (tiles128 < 320 && tiles64 < 256 && E >= 16 * 64) return 0;
  return 1;
}

extern "C" int asr_ctc_head_prep(asr_handle* h, const float* W, int E, int C, void* Wt, void* Wp, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!W || !Wp || E < 1 || C < 1 || (Wt && C > 64))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_head_prep: bad args E=%d C=%d", E, C);
  const int Kp = (C + 63) / 64 * 64;
  const size_t n = (size_t)E * Kp;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(ctc_head_images_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, W, E, C, Kp, (bf16_t*)Wt, (bf16_t*)Wp);
  ASR_CHECK_LAUNCH(h, "asr_ctc_head_prep");
  return ASR_OK;
}

extern "C" int asr_ctc_head_fwd(asr_handle* h, const void* hout, int T, int B, int E, float keep_prob, uint64_t seed,
                                uint64_t offset, const void* Wt, const float* bias, int C, const int32_t* labels_flat,
                                const int32_t* label_offsets, const int32_t* seq_len, int max_label_len, void* x_op,
                                float* logits, int32_t* num_infeasible, void* workspace, size_t workspace_bytes,
                                asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!hout || !Wt || !bias || !logits || !label_offsets || !seq_len || T <= 0 || B <= 0 || max_label_len < 0 ||
      (max_label_len > 0 && !labels_flat) || !(keep_prob == 0.f || (keep_prob > 0.f && keep_prob <= 1.f)) ||
      (keep_prob != 0.f && !x_op))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_head_fwd: bad args T=%d B=%d E=%d C=%d Lmax=%d keep_prob=%g", T, B, E, C,
             max_label_len, (double)keep_prob);
  if ((size_t)T * B > 0x7fffffffull / (size_t)(E > C ? E : C) || !asr_ctc_head_ok(T * B, E, C))
    ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_ctc_head_fwd: shape rows=%d E=%d C=%d (asr_ctc_head_ok)", T * B, E, C);
  if (((uintptr_t)hout) % 16 != 0 || ((uintptr_t)Wt) % 16 != 0 || (x_op && ((uintptr_t)x_op) % 16 != 0))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_head_fwd: operands must be 16-byte aligned");
  const CtcWs w = ctc_ws_layout(T, B, max_label_len);
  if (!w.K) ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_ctc_head_fwd: label length %d > %d", max_label_len, (64 * 32 - 1) / 2);
  if (!workspace || workspace_bytes < w.total)
    ASR_FAIL(h, ASR_ERR_WORKSPACE, "asr_ctc_head_fwd: workspace %zu < %zu bytes", workspace_bytes, w.total);
  char* ws = (char*)workspace;
  const int rows = T * B, SP = 64 * w.K;
  const size_t lds = (size_t)16 * (E + 8) * sizeof(bf16_t) + (size_t)16 * 64 * sizeof(float);
#define ASR_HEAD(DROP_)                                                                                                \
  hipLaunchKernelGGL(ctc_head_fwd_kernel<DROP_>, dim3((rows + 15) / 16), dim3(256), lds, (hipStream_t)s,             \
                     (const bf16_t*)hout, rows, E, keep_prob, seed, offset, (const bf16_t*)Wt, bias, C, (bf16_t*)x_op, \
                     logits, (double*)(ws + w.lse), T, B, labels_flat, label_offsets, seq_len, SP,                     \
                     (MantExp*)(ws + w.yext), (MantExp*)(ws + w.yrev), num_infeasible)
  if (keep_prob != 0.f) ASR_HEAD(true); else ASR_HEAD(false);
#undef ASR_HEAD
  ASR_CHECK_LAUNCH(h, "asr_ctc_head_fwd");
  h->ctc_head_counts[0] += 1;
  return ASR_OK;
}

ASR_DEFINE_COUNTS(ctc_head_counts, ctc_head_counts)
ASR_DEFINE_COUNTS(ctc_ls_counts, ctc_ls_counts)

extern "C" int asr_ctc_greedy_decode(asr_handle* h, const float* logits, int T, int B, int C,
                                     const int32_t* seq_len, int blank, int32_t* out_labels,
                                     int32_t* out_len, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!logits || !seq_len || !out_labels || !out_len || T <= 0 || B <= 0 || C < 1)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_greedy_decode: bad args T=%d B=%d C=%d", T, B, C);
  const size_t lds = (size_t)T * sizeof(int32_t);
  if (lds > 150 * 1024) ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "asr_ctc_greedy_decode: T=%d too long", T);
  (void)hipFuncSetAttribute((const void*)ctc_collapse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const size_t nrows = (size_t)T * B;
  const unsigned ablocks = (unsigned)((nrows + 3) / 4 < 16384 ? (nrows + 3) / 4 : 16384);
  hipLaunchKernelGGL(ctc_argmax_kernel, dim3(ablocks), dim3(256), 0, (hipStream_t)s, logits, T, B, C, seq_len, out_labels);
  hipLaunchKernelGGL(ctc_collapse_kernel, dim3(B), dim3(256), lds, (hipStream_t)s, T, seq_len, blank, out_labels,
                     out_len);
  ASR_CHECK_LAUNCH(h, "asr_ctc_greedy_decode");
  return ASR_OK;
}

extern "C" int asr_softmax_rows(asr_handle* h, const float* in, float* out, int rows, int C,
                                asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!in || !out || rows < 0 || C < 1) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_softmax_rows: bad args");
  if (rows == 0) return ASR_OK;
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)s, in, out, rows, C);
  ASR_CHECK_LAUNCH(h, "asr_softmax_rows");
  return ASR_OK;
}
