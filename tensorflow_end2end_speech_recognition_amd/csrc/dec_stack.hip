// Multi-layer LSTM decoder of the attention models (decoder_num_layers = L > 1): MultiRNNCell of L LSTMBlockCell(U), each
// in a DropoutWrapper(output_keep_prob).  Layer 0 is the decoder cell the loops of dec_loop.hip have always run; this
// file holds what the upper layers l = 1 .. L-1 add to a step (x_l = [ o_{l-1} | h_{l,k-1} ], 2U wide):
//   forward    one cell launch per upper layer with the existing kernels -- asr_lstm_cell_gemm_fwd on the layer's
//              interleaved image where asr_lstm_cell_gemm_ok(B, 2U, U, 2U), asr_gemm_act + asr_lstm_cell_fwd_ex elsewhere
//              (a beam's B*W rows);
//   backward   per lower layer l = L-2 .. 0: dx = dpre_{l+1} W_{l+1}^T [B,2U] and the cell backward of layer l on
//              dx[:, :U], as ONE launch (stack_dx_cell_bwd_kernel) at B <= 32, U % 16 == 0, 16-byte aligned operands,
//              and as asr_gemm_act x 2 + the plain cell backward launch at every other shape;
//   beam       stack_reorder_kernel: every upper layer's c / h rows and carried h-columns gathered by parent, one launch.
// The loops themselves (and layer 0, the query FC, the attention, the heads) are dec_loop.hip's.
#include "common.h"
#include "lstm_cell_bwd.h"
#include <math.h>

namespace {

constexpr int SB_WAVES = 8;                     // waves of a workgroup; they split K = 4U in 64-element units
constexpr int SB_ROWS = 32;                     // batch rows of a workgroup: two 16-row MFMA tiles

// dx [B,2U] = dpre_up [B,4U] . W_up^T (W_up [2U,4U] row-major: output column n reads the contiguous row n -- the weights
// stream through once, 16 rows per workgroup) with the cell backward of the layer below in the epilogue.  Modelled on
// att_dq_cell_bwd_kernel: skinny in M, exact-fp32 16x16x4 MFMAs, the waves' partial tiles meet in LDS in a fixed order
// (run-to-run deterministic).  grid.x = 2U / 16 column blocks, one workgroup covers all B <= 32 rows:
//   columns [0,U)   g = dx[:, n]: gradient w.r.t. the lower layer's masked output o_l -> lstm_cell_bwd_elem -> c.dpre, ...
//   columns [U,2U)  stored as d_hin [B,U]: what the upper layer's step k-1 adds to its carried dh
// Every global operand of the epilogue is requested before the product, so that the weight stream is the only round
// trip on the kernel's chain.  135 VGPRs (3 waves per SIMD; a workgroup needs 2), 17 KB LDS, no scratch (gfx950, -O3).
__global__ __launch_bounds__(512) void stack_dx_cell_bwd_kernel(const float* __restrict__ dpre_up,
                                                                const float* __restrict__ W_up, int B, int U,
                                                                float* __restrict__ d_hin, CellBwdArgs c) {
  __shared__ float red[SB_WAVES][SB_ROWS][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, rg = lane >> 4;
  const int K = 4 * U, n0 = blockIdx.x * 16;
  const bool lower = n0 < U;                    // (U % 16 == 0: a block lies in one half)
  const bool two = B > 16;                      // the second row tile holds rows
  // epilogue: thread idx owns output (row em, column n0 + en)
  const int idx = threadIdx.x, em = idx >> 4, en = idx & 15;
  const int eb = min(em, B - 1), ej = n0 + en;
  float e_lv = 0.f, e_dhn = 0.f, e_dcn = 0.f, e_g[4] = {0.f, 0.f, 0.f, 0.f}, e_cr = 0.f, e_cp = 0.f,
        e_w[3] = {0.f, 0.f, 0.f}, e_mask = 1.f;
  if (lower) {
    const size_t bu = (size_t)eb * U + ej;
    e_lv = c.live[eb];
    e_dhn = c.dh_next[bu];
    if (c.dh_next2) e_dhn += c.dh_next2[(size_t)eb * c.ld2 + ej];
    e_dcn = c.dc_next[bu];
#pragma unroll
    for (int q = 0; q < 4; ++q) e_g[q] = c.gates[(size_t)eb * 4 * U + q * U + ej];
    e_cr = c.c_raw[bu];
    e_cp = c.c_prev[bu];
    if (c.peep) {
#pragma unroll
      for (int q = 0; q < 3; ++q) e_w[q] = c.peep[q * U + ej];
    }
    if (c.use_mask) e_mask = c.use_mask[bu];
  }
  // the product: wave w multiplies the 64-wide K units w, w + 8, ...; lane (col, rg) holds row / weight-row `col` and
  // the k-slot rg of every 16x16x4 step (k = unit + 16 j + 4 rg + e for operand element (j, e) on both sides)
  const int r0 = min(col, B - 1), r1 = min(16 + col, B - 1);
  const float* a0 = dpre_up + (size_t)r0 * K + rg * 4;
  const float* a1 = dpre_up + (size_t)r1 * K + rg * 4;
  const float* wp = W_up + (size_t)(n0 + col) * K + rg * 4;
  f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const f32x4_t z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4_t xa[4], xb[4], xw[4];
  int k0 = wave * 64;
  if (k0 < K) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xa[j] = *reinterpret_cast<const f32x4_t*>(a0 + k0 + j * 16);
      xb[j] = two ? *reinterpret_cast<const f32x4_t*>(a1 + k0 + j * 16) : z4;
      xw[j] = *reinterpret_cast<const f32x4_t*>(wp + k0 + j * 16);
    }
  }
  for (; k0 < K; k0 += SB_WAVES * 64) {
    f32x4_t ya[4], yb[4], yw[4];
    const int k1 = k0 + SB_WAVES * 64;
    if (k1 < K) {                               // the next unit's loads fly under this unit's multiplies
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ya[j] = *reinterpret_cast<const f32x4_t*>(a0 + k1 + j * 16);
        yb[j] = two ? *reinterpret_cast<const f32x4_t*>(a1 + k1 + j * 16) : z4;
        yw[j] = *reinterpret_cast<const f32x4_t*>(wp + k1 + j * 16);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[j][e], xw[j][e], acc0, 0, 0, 0);
        if (two) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[j][e], xw[j][e], acc1, 0, 0, 0);
      }
    if (k1 < K) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { xa[j] = ya[j]; xb[j] = yb[j]; xw[j] = yw[j]; }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[wave][rg * 4 + r][col] = acc0[r];
    red[wave][16 + rg * 4 + r][col] = acc1[r];
  }
  __syncthreads();
  if (em >= B) return;
  float dx = 0.f;
#pragma unroll
  for (int w = 0; w < SB_WAVES; ++w) dx += red[w][em][en];
  const int b = em;
  if (!lower) {
    d_hin[(size_t)b * U + (ej - U)] = dx;
    return;
  }
  const int j = ej;
  const size_t bu = (size_t)b * U + j;
  float* dp = c.dpre + (size_t)b * 4 * U;
  float* pr = c.dpeep_rows ? c.dpeep_rows + (size_t)b * 3 * U : nullptr;
  if (!(e_lv > 0.f)) {                          // finished row: state passes through, no parameter gradient
    dp[j] = 0.f; dp[U + j] = 0.f; dp[2 * U + j] = 0.f; dp[3 * U + j] = 0.f;
    c.dc_prev[bu] = e_dcn;
    c.dh_prev_carry[bu] = e_dhn;
    if (pr) { pr[j] = 0.f; pr[U + j] = 0.f; pr[2 * U + j] = 0.f; }
    return;
  }
  const float dh = dx * e_mask + e_dhn;
  const CellBwdElem r = lstm_cell_bwd_elem(dh, e_dcn, e_g[0], e_g[1], e_g[2], e_g[3], e_cr, e_cp, e_w[0], e_w[1], e_w[2],
                                           c.clip);
  dp[j] = r.d_i; dp[U + j] = r.d_g; dp[2 * U + j] = r.d_f; dp[3 * U + j] = r.d_o;
  c.dc_prev[bu] = r.dc_prev;
  c.dh_prev_carry[bu] = 0.f;
  if (pr) { pr[j] = r.d_i * e_cp; pr[U + j] = r.d_f * e_cp; pr[2 * U + j] = r.d_o * e_cr; }
}

// Beam re-ordering of the upper layers: block 1 (the step's outputs) -> block 0 (what the next step reads), row r = b*W + w
// from row b*W + parent[r].  grid = (R*U / 256, upper layers); c / h [2,R,U], in [2,R,2U] (its columns [U,2U)).
struct StackRows {
  float* c[ASR_ATT_STACK_MAX];
  float* h[ASR_ATT_STACK_MAX];
  float* in[ASR_ATT_STACK_MAX];
};
__global__ __launch_bounds__(256) void stack_reorder_kernel(StackRows p, const int32_t* __restrict__ parent, int R, int W,
                                                            int U) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * U) return;
  const int l = blockIdx.y;
  const int r = idx / U, j = idx % U;
  const int par = min(max(parent[r], 0), W - 1);
  const size_t src = (size_t)(r / W) * W + par;
  float* c = p.c[l];
  float* h = p.h[l];
  float* in = p.in[l];
  c[idx] = c[(size_t)R * U + src * U + j];
  h[idx] = h[(size_t)R * U + src * U + j];
  in[(size_t)r * 2 * U + U + j] = in[(size_t)R * 2 * U + src * 2 * U + U + j];
}

inline bool al16(const void* p) { return ((uintptr_t)p) % 16 == 0; }

// the upper layer's forward step runs on its interleaved image (one launch)
inline bool stack_img(const asr_att_decoder* a, const asr_att_stack_layer& u) {
  return u.W_il && asr_lstm_cell_gemm_ok(a->B, 2 * a->U, a->U, 2 * a->U) && al16(u.in) && al16(u.W_il);
}

int stack_bwd_step(asr_handle* h, const float* dpre_up, const float* W_up, int B, int U, const CellBwdArgs& ca,
                   float* d_hin, float* work, int fused, asr_stream s) {
  if (fused && asr_att_stack_bwd_ok(B, U) && al16(dpre_up) && al16(W_up)) {
    h->att_stack_counts[2] += 1;
    hipLaunchKernelGGL(stack_dx_cell_bwd_kernel, dim3(2 * U / 16), dim3(512), 0, (hipStream_t)s, dpre_up, W_up, B, U, d_hin,
                       ca);
    ASR_CHECK_LAUNCH(h, "asr_att_stack_bwd_step");
    return ASR_OK;
  }
  // generic: the two column halves of dx as two products (the cell backward launch reads a contiguous [B,U] block), then
  // the plain cell backward launch
  ASR_NEED(work, "asr_att_stack_bwd_step: the generic form needs B*U floats of work space");
  h->att_stack_counts[3] += 1;
  ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 1, B, U, 4 * U, dpre_up, 4 * U, W_up, 4 * U, work, U, nullptr, 0, 0, s));
  ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 1, B, U, 4 * U, dpre_up, 4 * U, W_up + (size_t)U * 4 * U, 4 * U, d_hin, U,
                       nullptr, 0, 0, s));
  return asr_lstm_cell_bwd_args(h, work, ca, B, U, s);
}

}  // namespace

extern "C" int asr_att_stack_bwd_ok(int B, int U) { return B >= 1 && B <= SB_ROWS && U >= 16 && U % 16 == 0; }

extern "C" int asr_att_stack_bwd_step(asr_handle* h, const float* dpre_up, const float* W_up, int B, int U,
                                      const float* dc_next, const float* dh_next, const float* dh_next2, int ld2,
                                      const float* gates, const float* c_raw, const float* c_prev, const float* peep,
                                      const float* live, const float* use_mask, float* dpre, float* dc_prev,
                                      float* dh_prev_carry, float* dpeep_rows, float* d_hin_up, float* work, int fused,
                                      asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(dpre_up && W_up && B > 0 && U > 0 && dc_next && dh_next && gates && c_raw && c_prev && live && dpre && dc_prev &&
               dh_prev_carry && d_hin_up && (!dh_next2 || ld2 >= U), "asr_att_stack_bwd_step: bad arguments");
  const CellBwdArgs ca = {dc_next, dh_next, dh_next2, gates, c_raw, c_prev, peep, live, use_mask,
                          dpre, dc_prev, dh_prev_carry, dpeep_rows, ld2, 0.f};
  return stack_bwd_step(h, dpre_up, W_up, B, U, ca, d_hin_up, work, fused, s);
}

extern "C" int asr_att_stack_reorder(asr_handle* h, const asr_att_stack* sk, const int32_t* parent, int B, int W, int U,
                                     asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(sk && parent && B > 0 && W > 0 && U > 0 && sk->L >= 2 && sk->L <= ASR_ATT_STACK_MAX + 1 &&
               (size_t)B * W * U < ((size_t)1 << 30), "asr_att_stack_reorder: bad arguments");
  StackRows p;
  const int nup = sk->L - 1;
  for (int i = 0; i < ASR_ATT_STACK_MAX; ++i) {
    const asr_att_stack_layer& u = sk->up[i < nup ? i : 0];
    ASR_NEED(u.c && u.h && u.in, "asr_att_stack_reorder: a layer's c / h / in is missing");
    p.c[i] = u.c; p.h[i] = u.h; p.in[i] = u.in;
  }
  const int R = B * W;
  hipLaunchKernelGGL(stack_reorder_kernel, dim3((R * U + 255) / 256, nup), dim3(256), 0, (hipStream_t)s, p, parent, R, W, U);
  ASR_CHECK_LAUNCH(h, "asr_att_stack_reorder");
  return ASR_OK;
}

ASR_DEFINE_COUNTS(att_stack_counts, att_stack_counts)

// ---------------------------------------------------------------- the upper layers' part of the loops of dec_loop.hip
int asr_stack_dec_check(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, bool bwd) {
  if (!a || !sk || sk->L < 2 || sk->L > ASR_ATT_STACK_MAX + 1)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder (stack): L must be 2 .. %d", ASR_ATT_STACK_MAX + 1);
  for (int i = 0; i < sk->L - 1; ++i) {
    const asr_att_stack_layer& u = sk->up[i];
    if (!u.W || !u.b || !u.in || !u.c || !u.h || !u.gates || !u.craw)
      ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder (stack): layer %d: bad arguments", i + 1);
    if (bwd && (!u.dpre || !u.d_hin || !u.dc0 || !u.dh0 || (u.peep && !u.dpeep) || !sk->work))
      ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_bwd (stack): layer %d: bad arguments", i + 1);
  }
  return ASR_OK;
}

int asr_stack_dec_image(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, asr_stream s) {
  for (int i = 0; i < sk->L - 1; ++i) {
    const asr_att_stack_layer& u = sk->up[i];
    if (stack_img(a, u)) ASR_TRY(asr_lstm_cell_gemm_prep(h, u.W, u.b, 2 * a->U, a->U, u.W_il, s));
  }
  return ASR_OK;
}

int asr_stack_dec_fwd_step(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, int k, int ks, bool more,
                           float* qz, asr_stream s) {
  const int B = a->B, U = a->U, Dav = U + a->E2, nup = sk->L - 1;
  float* pre = a->work;                                    // [B,4U] and [B,U]: layer 0's launches are behind us
  float* hraw = pre + (size_t)B * 4 * U;
  const float* live = a->live + (size_t)k * B;
  for (int i = 0; i < nup; ++i) {
    const asr_att_stack_layer& u = sk->up[i];
    const bool top = i + 1 == nup;
    float* x = u.in + (size_t)k * B * 2 * U;
    const float* cp = u.c + (size_t)k * B * U;
    const float* hp = u.h + (size_t)k * B * U;
    float* cn = u.c + (size_t)(k + 1) * B * U;
    float* hn = u.h + (size_t)(k + 1) * B * U;
    float* gates = u.gates + (size_t)ks * B * 4 * U;
    float* craw = u.craw + (size_t)ks * B * U;
    const float* mask = u.dmask ? u.dmask + (size_t)k * B * U : nullptr;
    // the masked output: the next layer's input columns, or (top) the attentional vector's and the query
    float* out2 = top ? a->av_in + (size_t)k * B * Dav : sk->up[i + 1].in + (size_t)k * B * 2 * U;
    const int ld_out2 = top ? Dav : 2 * U;
    float* hnext = more ? x + (size_t)B * 2 * U + U : nullptr;
    if (stack_img(a, u)) {
      h->att_stack_counts[0] += 1;
      ASR_TRY(asr_lstm_cell_gemm_fwd(h, x, 2 * U, 2 * U, u.W_il, 1, cp, hp, u.peep, live, B, U, a->forget_bias, a->cell_clip,
                                     gates, craw, cn, hn, hraw, mask, top ? qz : nullptr, hnext, 2 * U, out2, ld_out2, s));
    } else {
      h->att_stack_counts[1] += 1;
      ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, B, 4 * U, 2 * U, x, 2 * U, u.W, 4 * U, pre, 4 * U, u.b, 0, 0, s));
      ASR_TRY(asr_lstm_cell_fwd_ex(h, pre, cp, hp, u.peep, live, B, U, a->forget_bias, a->cell_clip, gates, craw, cn, hn,
                                   hraw, mask, top ? qz : nullptr, hnext, 2 * U, out2, ld_out2, s));
    }
  }
  return ASR_OK;
}

// carried dc / dh of upper layer l: two buffers each at work + (l-1)*4*B*U
static inline float* stack_carry(const asr_att_decoder* a, const asr_att_stack* sk, int l, int which, int cur) {
  const size_t BU = (size_t)a->B * a->U;
  return sk->work + (size_t)(l - 1) * 4 * BU + (size_t)(which * 2 + cur) * BU;
}

CellBwdArgs asr_stack_cell_args(const asr_att_decoder* a, const asr_att_stack* sk, int l, int k, int cur) {
  const int B = a->B, U = a->U;
  const asr_att_stack_layer& u = sk->up[l - 1];
  const CellBwdArgs ca = {stack_carry(a, sk, l, 0, cur), stack_carry(a, sk, l, 1, cur),
                          k + 1 < a->To ? u.d_hin + (size_t)(k + 1) * B * U : nullptr,
                          u.gates + (size_t)k * B * 4 * U, u.craw + (size_t)k * B * U, u.c + (size_t)k * B * U, u.peep,
                          a->live + (size_t)k * B, u.dmask ? u.dmask + (size_t)k * B * U : nullptr,
                          u.dpre + (size_t)k * B * 4 * U, stack_carry(a, sk, l, 0, cur ^ 1), stack_carry(a, sk, l, 1, cur ^ 1),
                          u.dpeep ? u.dpeep + (size_t)k * B * 3 * U : nullptr, U, 0.f};   // (clip: straight-through)
  return ca;
}

int asr_stack_dec_bwd_lower(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, int l, int k,
                            const CellBwdArgs& ca, asr_stream s) {
  const int B = a->B, U = a->U;
  const asr_att_stack_layer& up = sk->up[l];               // layer l + 1
  float* work = sk->work + (size_t)(sk->L - 1) * 4 * B * U;
  return stack_bwd_step(h, up.dpre + (size_t)k * B * 4 * U, up.W, B, U, ca, up.d_hin + (size_t)k * B * U, work, sk->fused, s);
}

int asr_stack_dec_bwd_begin(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, asr_stream s) {
  const size_t BU = (size_t)a->B * a->U;
  for (int l = 1; l < sk->L; ++l)
    if (hipMemsetAsync(stack_carry(a, sk, l, 0, 0), 0, BU * sizeof(float), (hipStream_t)s) != hipSuccess ||
        hipMemsetAsync(stack_carry(a, sk, l, 1, 0), 0, BU * sizeof(float), (hipStream_t)s) != hipSuccess)
      ASR_FAIL(h, ASR_ERR_HIP, "asr_att_decoder_bwd_stack: memset");
  return ASR_OK;
}

int asr_stack_dec_bwd_end(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, int cur, asr_stream s) {
  const int B = a->B, U = a->U;
  for (int l = 1; l < sk->L; ++l) {
    const asr_att_stack_layer& u = sk->up[l - 1];
    ASR_TRY(asr_add_cols(h, stack_carry(a, sk, l, 1, cur), U, u.d_hin, U, u.dh0, U, B, U, s));
    if (hipMemcpyAsync(u.dc0, stack_carry(a, sk, l, 0, cur), (size_t)B * U * sizeof(float), hipMemcpyDeviceToDevice,
                       (hipStream_t)s) != hipSuccess)
      ASR_FAIL(h, ASR_ERR_HIP, "asr_att_decoder_bwd_stack: copy");
  }
  return ASR_OK;
}
