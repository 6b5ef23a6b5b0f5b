// GRU decoder cell of the attention models (decoder_type 'gru'): tf.contrib.rnn.GRUCell as the reference's decoder branch
// names it (attention_seq2seq.py:364-365, tf.contrib.rnn.GRUCell(self.num_units); num_units read as decoder_num_units).
//
//   [r, u] = sigmoid([x, h] W_g + b_g)      c = tanh([x, r*h] W_c + b_c)      hn = u*h + (1-u)*c
//
// The candidate needs r of ALL units, so a step has two phases whatever the kernels look like.  Every product reads ONE
// image W3 [(Din+1), 3U] (asr_gru_cell_prep): W_g | W_c with its h-rows zeroed, bias row last -- gate-major, so that the
// forward's x W3, the backward's dpre W3^T and the general path's asr_gemm_act all take it as it is.
//   two-launch form (B <= 32, Din % 64 == 0, U % 16 == 0): gru_skinny_kernel phase A (x W3 with sigmoid / r*h in the
//     epilogue, one gate of 32 -- or 16 -- units per workgroup) and phase B ((r*h) W_c[h rows], tanh, state update, scatter)
//   four-launch form (any shape): asr_gemm_act -> gru_gates_kernel -> asr_gemm_act -> gru_out_kernel, same outputs.
// The skinny kernels follow gemm.hip's gemm_skinny_f32_kernel (eight waves split K in 64-element units, exact fp32
// 16x16x4 MFMAs, next unit's loads in flight under the current one's multiplies, the eight partial tiles meet in LDS in a
// fixed order); they are separate kernels because their epilogues are the cell.
#include "common.h"
#include <math.h>

namespace {

constexpr int GS_WAVES = 8;

// what phase B (and the general path's second elementwise kernel) writes for element (b, j) once the h-part of the
// candidate's pre-activation is known
struct GruOut {
  const float *h_prev, *live, *out_mask;
  float *gates, *h_out, *cell_out, *h_out2, *cell_out2;
  int U, ld_c, ld_h2, ld_c2;
};

__device__ __forceinline__ void gru_out_elem(const GruOut& o, int b, int j, float hpart, float hp, float lv, float om) {
  const int U = o.U;
  float* g = o.gates + (size_t)b * 4 * U;
  const float u = g[U + j];
  const float c = tanhf_(g[2 * U + j] + hpart);          // (the x-part + b_c was parked in the c column by phase A)
  const float hn = u * hp + (1.f - u) * c;
  g[2 * U + j] = c;
  const float ho = lv > 0.f ? hn : hp;
  o.h_out[(size_t)b * U + j] = ho;
  if (o.h_out2) o.h_out2[(size_t)b * o.ld_h2 + j] = ho;
  const float co = o.out_mask ? hn * om : hn;
  o.cell_out[(size_t)b * o.ld_c + j] = co;
  if (o.cell_out2) o.cell_out2[(size_t)b * o.ld_c2 + j] = co;
}

__global__ void gru_image_kernel(const float* __restrict__ Wg, const float* __restrict__ bg, const float* __restrict__ Wc,
                                 const float* __restrict__ bc, int Din, int U, float* __restrict__ W3) {
  const size_t n = (size_t)(Din + 1) * 3 * U;
  const int Dx = Din - U;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / (3 * U)), col = (int)(i % (3 * U));
    float v;
    if (row == Din) v = col < 2 * U ? bg[col] : bc[col - 2 * U];
    else if (col < 2 * U) v = Wg[(size_t)row * 2 * U + col];
    else v = row < Dx ? Wc[(size_t)row * U + col - 2 * U] : 0.f;
    W3[i] = v;
  }
}

// general path, phase A's elementwise part: pre3 [B,3U] (bias included) -> gates r | u | cx | r*h
__global__ void gru_gates_kernel(const float* __restrict__ pre3, const float* __restrict__ h_prev, int B, int U,
                                 float* __restrict__ gates) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * U) return;
  const int b = i / U, j = i % U;
  const float* p = pre3 + (size_t)b * 3 * U;
  const float r = sigmoidf_(p[j]), u = sigmoidf_(p[U + j]);
  float* g = gates + (size_t)b * 4 * U;
  g[j] = r; g[U + j] = u; g[2 * U + j] = p[2 * U + j]; g[3 * U + j] = r * h_prev[i];
}

// general path, phase B's elementwise part: hpart [B,U] = (r*h) W_c[h rows]
__global__ void gru_out_kernel(const float* __restrict__ hpart, int B, GruOut o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * o.U) return;
  const int b = i / o.U, j = i % o.U;
  gru_out_elem(o, b, j, hpart[i], o.h_prev[i], o.live[b], o.out_mask ? o.out_mask[i] : 1.f);
}

// C tile = A[M,K] Bm, 16 rows x 16 NT adjacent columns per workgroup (NT = 2: full 128-byte lines of the row-major Bm).
// K % 16 == 0: a 64-element unit's 16-wide chunks past K are multiplied by zero.
// Phase A (!PHASE_B): Bm = W3 [K = Din rows, 3U]; blockIdx.x = gate * (U / TN) + unit block -- a workgroup owns ONE gate
// (r, u or the candidate's x-part) of TN units, since none of the three needs another's value: r -> sigmoid, r and r*h
// written; u -> sigmoid; candidate -> parked in the c column for phase B.  3U / TN x 2 row groups workgroups pull on W3.
// Phase B: Bm = W_c[h rows] [K = U, U], A = the r*h block of `gates`; epilogue gru_out_elem.
template <int NT, bool PHASE_B>
__global__ __launch_bounds__(64 * GS_WAVES) void gru_skinny_kernel(int M, int K, const float* __restrict__ A, int lda,
                                                                   const float* __restrict__ Bm, int ldb,
                                                                   const float* __restrict__ bias, GruOut o) {
  constexpr int TN = 16 * NT;
  __shared__ float red[GS_WAVES][16][TN + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, rg = lane >> 4;
  const int U = o.U, nbg = U / TN;
  const int gate = PHASE_B ? 0 : (int)blockIdx.x / nbg;
  const int j0 = ((int)blockIdx.x % nbg) * TN, c0 = gate * U + j0, m0 = blockIdx.y * 16;
  // the epilogue's own inputs are requested before the product's first load: thread idx < 16 TN owns (row, unit)
  const int e_m = m0 + (int)threadIdx.x / TN, e_ul = (int)threadIdx.x % TN, e_j = j0 + e_ul;
  const bool e_on = (int)threadIdx.x < 16 * TN && e_m < M;
  float e_hp = 0.f, e_lv = 0.f, e_om = 1.f, e_b = 0.f;
  if (e_on) {
    if (PHASE_B || gate == 0) e_hp = o.h_prev[(size_t)e_m * U + e_j];
    if (PHASE_B) {
      e_lv = o.live[e_m];
      if (o.out_mask) e_om = o.out_mask[(size_t)e_m * U + e_j];
    } else {
      e_b = bias[c0 + e_ul];
    }
  }
  struct Frag {
    f32x4_t a[4], b[NT][4];
    float keep[4];
  };
  f32x4_t acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const float* ap = A + (size_t)min(m0 + col, M - 1) * lda + rg * 4;   // rows past M read a valid row, masked at the store
  const int units = (K + 63) / 64;
  auto load = [&](int round, Frag& f) {
    const int unit = wave + round * GS_WAVES;
    const int kb = (unit < units ? unit : units - 1) * 64;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool valid = unit < units && kb + j * 16 < K;
      const int kk = valid ? kb + j * 16 : 0;                           // (an invalid chunk re-reads chunk 0, times zero)
      f.keep[j] = valid ? 1.f : 0.f;
      f.a[j] = *reinterpret_cast<const f32x4_t*>(ap + kk);              // A[row][kk + 4rg + e]
#pragma unroll
      for (int n = 0; n < NT; ++n) {                                    // B[kk + 4rg + e][c0 + 16n + col]
        const float* bp = Bm + (size_t)(kk + rg * 4) * ldb + c0 + n * 16 + col;
#pragma unroll
        for (int e = 0; e < 4; ++e) f.b[n][j][e] = bp[(size_t)e * ldb];
      }
    }
  };
  auto mma = [&](const Frag& f) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[j][e] * f.keep[j], f.b[n][j][e], acc[n], 0, 0, 0);
  };
  Frag f0, f1;
  load(0, f0);
  if (units <= GS_WAVES) {
    mma(f0);
  } else {
    const int rounds = ((units + GS_WAVES - 1) / GS_WAVES + 1) & ~1;
    for (int r = 0; r < rounds; r += 2) {
      load(r + 1, f1);
      __builtin_amdgcn_sched_barrier(0);
      mma(f0);
      __builtin_amdgcn_sched_barrier(0);
      load(r + 2, f0);
      __builtin_amdgcn_sched_barrier(0);
      mma(f1);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // lane holds C[m0 + rg*4 + r][c0 + 16n + col]
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][rg * 4 + r][n * 16 + col] = acc[n][r];
  __syncthreads();
  if (!e_on) return;
  const int m = (int)threadIdx.x / TN;
  float p = 0.f;
#pragma unroll
  for (int w = 0; w < GS_WAVES; ++w) p += red[w][m][e_ul];
  p += e_b;
  if constexpr (PHASE_B) {
    gru_out_elem(o, e_m, e_j, p, e_hp, e_lv, e_om);
  } else {
    float* g = o.gates + (size_t)e_m * 4 * U;
    if (gate == 0) {
      const float r = sigmoidf_(p);
      g[e_j] = r; g[3 * U + e_j] = r * e_hp;
    } else if (gate == 1) {
      g[U + e_j] = sigmoidf_(p);
    } else {
      g[2 * U + e_j] = p;
    }
  }
}

// backward, first elementwise kernel: dhn, du' -> dpre[:, U..2U), dp -> dpre[:, 2U..3U)
__global__ void gru_bwd1_kernel(const float* __restrict__ dcell, const float* __restrict__ dh_c,
                                const float* __restrict__ dh_c2, int ld2, const float* __restrict__ out_mask,
                                const float* __restrict__ live, const float* __restrict__ gates,
                                const float* __restrict__ h_prev, int B, int U, float* __restrict__ dpre,
                                float* __restrict__ dhn_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * U) return;
  const int b = i / U, j = i % U;
  float dhc = dh_c[i];
  if (dh_c2) dhc += dh_c2[(size_t)b * ld2 + j];
  const float lv = live[b] > 0.f ? 1.f : 0.f;
  const float dhn = (out_mask ? out_mask[i] * dcell[i] : dcell[i]) + lv * dhc;
  const float* g = gates + (size_t)b * 4 * U;
  const float u = g[U + j], c = g[2 * U + j], hp = h_prev[i];
  const float dc = dhn * (1.f - u), du = dhn * (hp - c);
  float* dp = dpre + (size_t)b * 3 * U;
  dp[U + j] = du * u * (1.f - u);
  dp[2 * U + j] = dc * (1.f - c * c);
  dhn_out[i] = dhn;
}

// backward, second elementwise kernel: dr' -> dpre[:, 0..U), the carried dh
__global__ void gru_bwd2_kernel(const float* __restrict__ d_rh, const float* __restrict__ dhn,
                                const float* __restrict__ dh_c, const float* __restrict__ dh_c2, int ld2,
                                const float* __restrict__ live, const float* __restrict__ gates,
                                const float* __restrict__ h_prev, int B, int U, float* __restrict__ dpre,
                                float* __restrict__ dh_carry) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * U) return;
  const int b = i / U, j = i % U;
  float dhc = dh_c[i];
  if (dh_c2) dhc += dh_c2[(size_t)b * ld2 + j];
  const float lv = live[b] > 0.f ? 1.f : 0.f;
  const float* g = gates + (size_t)b * 4 * U;
  const float r = g[j], u = g[U + j], drh = d_rh[i];
  dpre[(size_t)b * 3 * U + j] = drh * h_prev[i] * r * (1.f - r);
  dh_carry[i] = (1.f - lv) * dhc + dhn[i] * u + drh * r;
}

}  // namespace

extern "C" int asr_gru_cell_prep(asr_handle* h, const float* W_g, const float* b_g, const float* W_c, const float* b_c,
                                 int Din, int U, float* W3, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(W_g && b_g && W_c && b_c && W3 && U > 0 && Din > U, "asr_gru_cell_prep: bad args");
  const size_t n = (size_t)(Din + 1) * 3 * U;
  const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  hipLaunchKernelGGL(gru_image_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, W_g, b_g, W_c, b_c, Din, U, W3);
  ASR_CHECK_LAUNCH(h, "asr_gru_cell_prep");
  return ASR_OK;
}

extern "C" int asr_gru_cell_gemm_ok(int B, int Din, int U, int ldx) {
  return B >= 1 && B <= 32 && U >= 16 && U % 16 == 0 && Din > U && Din % 64 == 0 && ldx >= Din && ldx % 4 == 0;
}

static bool gru_fwd_args_ok(const float* x, int ldx, int Din, const float* W3, const float* W_ch, const float* h_prev,
                            const float* live, int B, int U, float* gates, float* h_out, float* cell_out, int ld_c,
                            float* h_out2, int ld_h2, float* cell_out2, int ld_c2) {
  return x && W3 && W_ch && h_prev && live && gates && h_out && cell_out && B > 0 && U > 0 && Din > U && ldx >= Din &&
         ld_c >= U && (!h_out2 || ld_h2 >= U) && (!cell_out2 || ld_c2 >= U);
}

extern "C" int asr_gru_cell_fwd_ex(asr_handle* h, const float* x, int ldx, int Din, const float* W3, const float* W_ch,
                                   const float* h_prev, const float* live, const float* out_mask, int B, int U,
                                   float* gates, float* h_out, float* cell_out, int ld_c, float* h_out2, int ld_h2,
                                   float* cell_out2, int ld_c2, float* work, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(work && gru_fwd_args_ok(x, ldx, Din, W3, W_ch, h_prev, live, B, U, gates, h_out, cell_out, ld_c, h_out2, ld_h2,
                                   cell_out2, ld_c2), "asr_gru_cell_fwd_ex: bad args");
  hipStream_t st = (hipStream_t)s;
  float* pre3 = work;                                      // [B,3U]
  float* hpart = work + (size_t)B * 3 * U;                 // [B,U]
  const int blocks = (B * U + 255) / 256;
  h->att_gru_counts[1] += 1;
  ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, B, 3 * U, Din, x, ldx, W3, 3 * U, pre3, 3 * U, W3 + (size_t)Din * 3 * U, 0,
                       0, s));
  hipLaunchKernelGGL(gru_gates_kernel, dim3(blocks), dim3(256), 0, st, pre3, h_prev, B, U, gates);
  ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, B, U, U, gates + 3 * U, 4 * U, W_ch, U, hpart, U, nullptr, 0, 0, s));
  const GruOut o = {h_prev, live, out_mask, gates, h_out, cell_out, h_out2, cell_out2, U, ld_c, ld_h2, ld_c2};
  hipLaunchKernelGGL(gru_out_kernel, dim3(blocks), dim3(256), 0, st, hpart, B, o);
  ASR_CHECK_LAUNCH(h, "asr_gru_cell_fwd_ex");
  return ASR_OK;
}

extern "C" int asr_gru_cell_gemm_fwd(asr_handle* h, const float* x, int ldx, int Din, const float* W3, const float* W_ch,
                                     const float* h_prev, const float* live, const float* out_mask, int B, int U,
                                     float* gates, float* h_out, float* cell_out, int ld_c, float* h_out2, int ld_h2,
                                     float* cell_out2, int ld_c2, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(gru_fwd_args_ok(x, ldx, Din, W3, W_ch, h_prev, live, B, U, gates, h_out, cell_out, ld_c, h_out2, ld_h2, cell_out2,
                           ld_c2) && asr_gru_cell_gemm_ok(B, Din, U, ldx) && ((uintptr_t)x) % 16 == 0 &&
               ((uintptr_t)gates) % 16 == 0,
           "asr_gru_cell_gemm_fwd: bad args (B <= 32, Din %% 64 == 0, U %% 16 == 0, 16-byte aligned rows)");
  hipStream_t st = (hipStream_t)s;
  const unsigned gy = (unsigned)((B + 15) / 16);
  const dim3 block(64 * GS_WAVES);
  const GruOut o = {h_prev, live, out_mask, gates, h_out, cell_out, h_out2, cell_out2, U, ld_c, ld_h2, ld_c2};
  const float* b3 = W3 + (size_t)Din * 3 * U;
  h->att_gru_counts[0] += 1;
  if (U % 32 == 0)
    hipLaunchKernelGGL((gru_skinny_kernel<2, false>), dim3(3 * U / 32, gy), block, 0, st, B, Din, x, ldx, W3, 3 * U, b3, o);
  else
    hipLaunchKernelGGL((gru_skinny_kernel<1, false>), dim3(3 * U / 16, gy), block, 0, st, B, Din, x, ldx, W3, 3 * U, b3, o);
  hipLaunchKernelGGL((gru_skinny_kernel<1, true>), dim3(U / 16, gy), block, 0, st, B, U, (const float*)(gates + 3 * U), 4 * U,
                     W_ch, U, (const float*)nullptr, o);
  ASR_CHECK_LAUNCH(h, "asr_gru_cell_gemm_fwd");
  return ASR_OK;
}

extern "C" int asr_gru_cell_bwd(asr_handle* h, const float* dcell, const float* dh_c, const float* dh_c2, int ld2,
                                const float* out_mask, const float* live, const float* gates, const float* h_prev,
                                const float* W3, const float* W_ch, int B, int Din, int U, float* dpre,
                                float* dh_prev_carry, float* d_in, int ld_din, float* work, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(dcell && dh_c && live && gates && h_prev && W3 && W_ch && dpre && dh_prev_carry && d_in && work && B > 0 &&
               U > 0 && Din > U && ld_din >= Din && (!dh_c2 || ld2 >= U) && dh_prev_carry != dh_c,
           "asr_gru_cell_bwd: bad args");
  hipStream_t st = (hipStream_t)s;
  float* d_rh = work;                                      // [B,U]
  float* dhn = work + (size_t)B * U;                       // [B,U]
  const int blocks = (B * U + 255) / 256;
  h->att_gru_counts[2] += 1;
  hipLaunchKernelGGL(gru_bwd1_kernel, dim3(blocks), dim3(256), 0, st, dcell, dh_c, dh_c2, ld2, out_mask, live, gates, h_prev,
                     B, U, dpre, dhn);
  ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 1, B, U, U, dpre + 2 * U, 3 * U, W_ch, U, d_rh, U, nullptr, 0, 0, s));
  hipLaunchKernelGGL(gru_bwd2_kernel, dim3(blocks), dim3(256), 0, st, d_rh, dhn, dh_c, dh_c2, ld2, live, gates, h_prev, B, U,
                     dpre, dh_prev_carry);
  ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 1, B, Din, 3 * U, dpre, 3 * U, W3, 3 * U, d_in, ld_din, nullptr, 0, 0, s));
  ASR_CHECK_LAUNCH(h, "asr_gru_cell_bwd");
  return ASR_OK;
}

ASR_DEFINE_COUNTS(att_gru_counts, att_gru_counts)

// ---------------------------------------------------------------- the cell part of a decoder-loop step (dec_loop.hip)
int asr_gru_dec_check(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g) {
  if (!g || !g->W_g || !g->b_g || !g->W_c || !g->b_c || !g->W3 || ((uintptr_t)g->W3) % 16 != 0)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_*_gru: bad arguments (the GRU part)");
  (void)a;
  return ASR_OK;
}

int asr_gru_dec_image(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, asr_stream s) {
  return asr_gru_cell_prep(h, g->W_g, g->b_g, g->W_c, g->b_c, a->Em + a->E2 + a->U, a->U, g->W3, s);
}

int asr_gru_dec_fwd_step(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, int k, int ks, float* dnext,
                         float* qz, asr_stream s) {
  const int B = a->B, U = a->U, Dx = a->Em + a->E2, Din = Dx + U, Dav = U + a->E2;
  const float* din = a->dec_in + (size_t)k * B * Din;
  float* gates = a->gates_all + (size_t)ks * B * 4 * U;
  const float* hp = a->h_all + (size_t)k * B * U;
  float* hn = a->h_all + (size_t)(k + 1) * B * U;
  float* av = a->av_in + (size_t)k * B * Dav;
  const float* live = a->live + (size_t)k * B;
  const float* mask = a->dmask ? a->dmask + (size_t)k * B * U : nullptr;
  const float* W_ch = g->W_c + (size_t)Dx * U;
  float* co2 = a->has_query_fc ? nullptr : qz;             // without a query FC the cell output IS the query
  if (g->fused && asr_gru_cell_gemm_ok(B, Din, U, Din) && ((uintptr_t)din) % 16 == 0 && ((uintptr_t)gates) % 16 == 0)
    return asr_gru_cell_gemm_fwd(h, din, Din, Din, g->W3, W_ch, hp, live, mask, B, U, gates, hn, av, Dav,
                                 dnext ? dnext + Dx : nullptr, Din, co2, a->A, s);
  return asr_gru_cell_fwd_ex(h, din, Din, Din, g->W3, W_ch, hp, live, mask, B, U, gates, hn, av, Dav,
                             dnext ? dnext + Dx : nullptr, Din, co2, a->A, a->work, s);
}

int asr_gru_dec_bwd_step(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, int k, const float* dcell,
                         const float* dh_c, const float* dh_c2, float* dh_carry, float* work2, asr_stream s) {
  const int B = a->B, U = a->U, Dx = a->Em + a->E2, Din = Dx + U;
  return asr_gru_cell_bwd(h, dcell, dh_c, dh_c2, Din, a->dmask ? a->dmask + (size_t)k * B * U : nullptr,
                          a->live + (size_t)k * B, a->gates_all + (size_t)k * B * 4 * U, a->h_all + (size_t)k * B * U, g->W3,
                          g->W_c + (size_t)Dx * U, B, Din, U, a->dpre_all + (size_t)k * B * 3 * U, dh_carry,
                          a->d_in_all + (size_t)k * B * Din, Din, work2, s);
}
