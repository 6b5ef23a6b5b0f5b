// Shared helpers for the gfx950 kernels of libasr_hip.so.  CDNA4 only: wave = 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/asr_hip.h"

struct asr_handle {
  int device;
  int num_cu;
  char name[128];
  char err[512];
  // device scratch owned by the handle (allocated once in asr_create, never in a hot call):
  // split-K slabs of asr_gemm.  Calls on one handle are single-stream by contract.
  void* scratch;
  size_t scratch_bytes;
  // exchange areas of the cluster recurrences (xch_take, cluster_host.hip): bytes of each area that hold stale tags, and the
  // area the next launch runs on
  size_t xch_dirty[2];
  int xch_next;
  // side-stream handles: number of leading XCDs the lean weight-gradient GEMM leaves to the recurrence clusters
  int xcd_skip;
  // workgroups the lean reduction-major GEMM aims at (0 = default 512); see asr_set_gemm_tn_workgroups
  int tn_wgs;
  // asr_lstm_bwd_ex: the clip the forward applied to the cell state when a clamped state must pass no gradient
  // (tf.clip_by_value of LSTMCell); 0 = the straight-through clip of LSTMBlockCell.  Set around the kernel dispatch only.
  float bptt_clip;
  // recurrence launches since the last asr_reset_recurrence_path_counts (plain host counters bumped at launch time):
  // {cluster launches, single-CU calls, calls split into more than one tile group} of the LSTM, then of the GRU
  unsigned long long rec_counts[6];
  // asr_gru_fwd / asr_gru_bwd calls since the last asr_reset_gru_kernel_counts by the form they ended in:
  // {fwd cluster, fwd persistent, fwd per step, bwd cluster, bwd persistent, bwd per step}
  unsigned long long gru_counts[6];
  // asr_lstm_fwd / asr_lstm_bwd(_ex) calls since the last asr_reset_lstm_kernel_counts by the form they ended in, indexed by
  // the ASR_LSTM_* enum of asr_hip.h (bumped where the form is chosen: lstm_cluster.hip / lstm_cluster_f32.hip for the clusters, lstm.hip else)
  unsigned long long lstm_counts[ASR_LSTM_KERNEL_N];
  // attention-decoder launches since the last asr_reset_att_path_counts, indexed by the ASR_ATT_* enum of asr_hip.h
  unsigned long long att_counts[ASR_ATT_PATH_N];
  // beam search launches since the last asr_reset_att_beam_counts: {select, reorder, backtrace}
  unsigned long long att_beam_counts[3];
  // joint CTC / attention beam search launches since the last asr_reset_att_joint_counts: {score, advance, joint_select}
  unsigned long long att_joint_counts[3];
  // LM-fused beam search calls since the last asr_reset_att_lm_counts: {lm_step, fused_select, lm_reorder}
  unsigned long long att_lm_counts[3];
  // 3x3 convolution launches since the last asr_reset_conv_path_counts, indexed by the ASR_CONVP_* enum of asr_hip.h
  unsigned long long conv_counts[ASR_CONVP_N];
  // listed-row GEMM calls since the last asr_reset_gemm_path_counts, indexed by the ASR_GEMMP_* enum of asr_hip.h
  unsigned long long gemm_counts[ASR_GEMMP_N];
  // LM-fused CTC prefix search since the last asr_reset_ctc_beam_lm_counts: {frame launches, lm steps, commits}
  unsigned long long ctc_beam_lm_counts[3];
  // CTC head since the last asr_reset_ctc_head_counts: {asr_ctc_head_fwd launches, asr_ctc_loss_ex calls, asr_ctc_loss calls}
  unsigned long long ctc_head_counts[3];
  // asr_ctc_loss_ls since the last asr_reset_ctc_ls_counts: {calls, calls with lse_done, calls without a gradient}
  unsigned long long ctc_ls_counts[3];
  // GRU decoder steps since the last asr_reset_att_gru_counts: {two-launch forward, four-launch forward, backward}
  unsigned long long att_gru_counts[3];
  // upper layers of a decoder stack since the last asr_reset_att_stack_counts: {forward on the image, forward as product +
  // cell, backward fused, backward generic}
  unsigned long long att_stack_counts[4];
  // asr_weight_noise_perturb since the last asr_reset_weight_noise_counts: {calls, elements, calls on the 16-byte path}
  unsigned long long weight_noise_counts[3];
  // asr_input_augment since the last asr_reset_input_augment_counts: {calls, elements, calls on the 16-byte path}
  unsigned long long input_augment_counts[3];
};

#define ASR_FAIL(h, code, ...)                                  \
  do {                                                          \
    if (h) snprintf((h)->err, sizeof((h)->err), __VA_ARGS__);   \
    return (code);                                              \
  } while (0)

#define ASR_CHECK_LAUNCH(h, what)                                                   \
  do {                                                                              \
    hipError_t e_ = hipGetLastError();                                              \
    if (e_ != hipSuccess) ASR_FAIL(h, ASR_ERR_HIP, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

// host entry points (a handle `h` in scope): reject an argument with a message / pass a callee's error on
#define ASR_NEED(cond, ...) do { if (!(cond)) ASR_FAIL(h, ASR_ERR_INVALID_ARG, __VA_ARGS__); } while (0)
#define ASR_TRY(call) do { const int rc_ = (call); if (rc_ != ASR_OK) return rc_; } while (0)

// getter and reset of one of the handle's launch-counter arrays, by export name and handle field; one line in the file that
// bumps the field.  The field's own size is the word count.
#define ASR_COUNTS_WORDS_(field) ((int)(sizeof(h->field) / sizeof(h->field[0])))
#define ASR_DEFINE_COUNTS_RESET_(name, field)                                  \
  extern "C" int asr_reset_##name(asr_handle* h) {                             \
    if (!h) return ASR_ERR_INVALID_ARG;                                        \
    for (int i = 0; i < ASR_COUNTS_WORDS_(field); ++i) h->field[i] = 0;        \
    return ASR_OK;                                                             \
  }
// fixed form: asr_<name>(h, out) writes every word of the field (3, 4 or 6; the header names the parameter out<N>)
#define ASR_DEFINE_COUNTS(name, field)                                         \
  extern "C" int asr_##name(asr_handle* h, unsigned long long* out) {          \
    if (!h || !out) return ASR_ERR_INVALID_ARG;                                \
    for (int i = 0; i < ASR_COUNTS_WORDS_(field); ++i) out[i] = h->field[i];   \
    return ASR_OK;                                                             \
  }                                                                            \
  ASR_DEFINE_COUNTS_RESET_(name, field)
// sized form (fields indexed by an enum of asr_hip.h that may grow): asr_<name>(h, out, n) writes n words, zeros past the
// field's end, fewer than the field has when n is smaller; n < 0 is ASR_ERR_INVALID_ARG
#define ASR_DEFINE_COUNTS_N(name, field)                                                       \
  extern "C" int asr_##name(asr_handle* h, unsigned long long* out, int n) {                   \
    if (!h || !out || n < 0) return ASR_ERR_INVALID_ARG;                                       \
    for (int i = 0; i < n; ++i) out[i] = i < ASR_COUNTS_WORDS_(field) ? h->field[i] : 0ull;    \
    return ASR_OK;                                                                             \
  }                                                                                            \
  ASR_DEFINE_COUNTS_RESET_(name, field)

typedef uint16_t bf16_t;  // raw bf16 bits

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;  // MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) float f32x4_t;   // MFMA 16x16 C/D fragment

__device__ __forceinline__ float bf16_to_f32(bf16_t v) {
  return __uint_as_float(((uint32_t)v) << 16);
}
// round-to-nearest-even, NaN stays NaN: gfx950's own conversion (v_cvt_pk_bf16_f32, two values per instruction) -- the
// integer form of rounds 1-3 (compare, select, two adds, two shifts per value) was a third of the VALU work of every
// bf16 epilogue; same result for every finite input and infinities
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
  return __builtin_bit_cast(unsigned short, (__bf16)f);
}

template <typename T> struct Elem;
template <> struct Elem<float> {
  static __device__ __forceinline__ float to_f32(float v) { return v; }
  static __device__ __forceinline__ float from_f32(float v) { return v; }
};
template <> struct Elem<bf16_t> {
  static __device__ __forceinline__ float to_f32(bf16_t v) { return bf16_to_f32(v); }
  static __device__ __forceinline__ bf16_t from_f32(float v) { return f32_to_bf16(v); }
};

// Gate nonlinearities.  Precise libm forms (expf/tanhf, <= 1-2 ulp): the fp32 path
// is the parity path (loss within 1e-4 relative of the oracle).
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return tanhf(x); }

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// sum over aligned groups of W lanes (W = 16, 32 or 64), result in every lane of the group.  The steps inside a
// 16-lane row are DPP modifiers on the add (quad_perm [1,0,3,2], [2,3,0,1], row_ror:4, row_ror:8), not LDS permutes.
template <int CTRL> __device__ __forceinline__ float dpp_mov_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int W> __device__ __forceinline__ float group_reduce_sum(float v) {
  v += dpp_mov_f32<0xB1>(v);
  v += dpp_mov_f32<0x4E>(v);
  v += dpp_mov_f32<0x124>(v);
  v += dpp_mov_f32<0x128>(v);
  if (W >= 32) v += __shfl_xor(v, 16, 64);
  if (W >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}
// tanh from the hardware exp2 / reciprocal: 1 - 2 / (exp(2x) + 1), absolute error < 2e-7 (each of v_exp_f32 and
// v_rcp_f32 is good to 1 ulp), saturating correctly at +-1.  For the attention energies -- sum_a v_a tanh(.) over every
// encoder frame and decoder step, which the libm form (~40 instructions) makes ALU-bound; NOT for the cell
// nonlinearities, which stay on tanhf_.
__device__ __forceinline__ float fast_tanhf(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.885390081777927f);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

// Philox4x32-10: the block of counter {lo, hi, 0, 0} of ctr under key = seed
__device__ __forceinline__ void asr_philox_block(uint64_t ctr, uint64_t seed, uint32_t c[4]) {
  c[0] = (uint32_t)ctr; c[1] = (uint32_t)(ctr >> 32); c[2] = 0u; c[3] = 0u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// Philox block -> the four dropout multipliers of elements 4 ctr' .. 4 ctr' + 3 (ctr = offset + element / 4);
// the generator of asr_dropout_mask (elementwise.hip), for the kernels that form the mask in their epilogue.
__device__ __forceinline__ void asr_dropout_words(uint64_t ctr, uint64_t seed, float keep, float inv, float m[4]) {
  uint32_t c[4];
  asr_philox_block(ctr, seed, c);
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = ((c[j] >> 8) * (1.0f / 16777216.0f) < keep) ? inv : 0.f;
}

// Philox block -> four standard normal values for elements 4 ctr' .. 4 ctr' + 3 (ctr = offset + element / 4), Box-Muller on
// the word pairs (c0, c1) and (c2, c3): u_a = ((c_even >> 8) + 1) 2^-24 in (0, 1], u_b = (c_odd >> 8) 2^-24 in [0, 1),
// r = sqrt(-2 ln u_a), z_even = r cos(2 pi u_b), z_odd = r sin(2 pi u_b); |z| <= sqrt(48 ln 2) = 5.768.  The generator of
// asr_weight_noise_perturb (weight_noise.hip), for kernels that form the same noise in an epilogue.  Accurate library ln /
// sin / cos (2 u_b is exact, sincospif reduces its argument exactly): within 1e-5 of the float64 statement.
__device__ __forceinline__ void asr_normal_words(uint64_t ctr, uint64_t seed, float z[4]) {
  uint32_t c[4];
  asr_philox_block(ctr, seed, c);
#pragma unroll
  for (int j = 0; j < 4; j += 2) {
    const float ua = (float)((c[j] >> 8) + 1u) * (1.0f / 16777216.0f);
    const float ub = (float)(c[j + 1] >> 8) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.f * logf(ua));
    float sn, cs;
    sincospif(2.f * ub, &sn, &cs);
    z[j] = r * cs;
    z[j + 1] = r * sn;
  }
}

// top ASR_XCH_BYTES of the scratch: granule exchange + error word of the multi-CU LSTM kernels
// (64 MB: two areas; the BPTT kernel's H = 512 clusters of 16 CUs take 1 MB of slots each, 16 clusters at B = 128)
static constexpr size_t ASR_XCH_BYTES = (size_t)64 << 20;
// bf16 operands (lstm_cluster.hip); false = not applicable, nothing launched
bool asr_cluster_fwd_try(asr_handle* h, int T, int B, int H, int ndir, const float* xproj,
                         const void* whp, const float* peep, const int32_t* seq_len, float fb,
                         float clip, void* gates, void* hout, float* cs, float* cf, float* hf,
                         hipStream_t st);
bool asr_cluster_bwd_try(asr_handle* h, int T, int B, int H, int ndir, const float* dhout,
                         const void* gates, const float* cs, const void* whpb, const float* peep,
                         const int32_t* seq_len, const float* dcf, const float* dhf, void* dgates,
                         float* dpeep_part, hipStream_t st);
// fp32 operands (lstm_cluster_f32.hip); same contract
bool asr_cluster_fwd_f32_try(asr_handle* h, int T, int B, int H, int ndir, const float* xproj,
                             const void* whp, const float* peep, const int32_t* seq_len, float fb,
                             float clip, void* gates, void* hout, float* cs, float* cf, float* hf,
                             hipStream_t st);
bool asr_cluster_bwd_f32_try(asr_handle* h, int T, int B, int H, int ndir, const float* dhout,
                             const void* gates, const float* cs, const void* whpb, const float* peep,
                             const int32_t* seq_len, const float* dcf, const float* dhf, void* dgates,
                             float* dpeep_part, hipStream_t st);

// GRU forward / backward on clusters (gru_cluster.hip); false = not applicable
bool asr_cluster_gru_fwd_try(asr_handle* h, int T, int B, int H, int ndir, const float* xg, const float* xc,
                             const float* wgh, const float* wch, const int32_t* seq_len, float* r, float* u, float* c,
                             float* rh, float* hout, float* h_final, hipStream_t st);

bool asr_cluster_gru_bwd_try(asr_handle* h, int T, int B, int H, int ndir, const float* dout, const float* d_h_final,
                             const float* hout, const float* r, const float* u, const float* c, const float* wghT,
                             const float* wchT, const int32_t* seq_len, float* dgate, float* dcand, hipStream_t st);

// the GRU cell's part of a decoder-loop step (gru_decoder.hip; the loops are dec_loop.hip's): argument check, the weight
// image once per loop call, the cell launches of forward step k (saved activations at row ks; dnext = the next step's
// input rows or NULL; qz = the step's query rows) and of backward step k (work2: 2*B*U floats)
int asr_gru_dec_check(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g);
int asr_gru_dec_image(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, asr_stream s);
int asr_gru_dec_fwd_step(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, int k, int ks, float* dnext,
                         float* qz, asr_stream s);
int asr_gru_dec_bwd_step(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, int k, const float* dcell,
                         const float* dh_c, const float* dh_c2, float* dh_carry, float* work2, asr_stream s);

// the upper layers of a multi-layer LSTM decoder (dec_stack.hip; the loops are dec_loop.hip's): argument check, the
// layers' weight images once per loop call, the upper layers' cell launches of forward step k (layer 0 has written
// up[0].in[k][:, :U]; saved activations at row ks; `more`: the next step's h-columns are written; qz: the step's query rows
// when there is no query FC, else NULL), and the per-loop parts of the backward (zeroed carries; dc0 / dh0 at the end)
int asr_stack_dec_check(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* k, bool bwd);
int asr_stack_dec_image(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* k, asr_stream s);
int asr_stack_dec_fwd_step(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, int k, int ks, bool more,
                           float* qz, asr_stream s);
int asr_stack_dec_bwd_begin(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, asr_stream s);
int asr_stack_dec_bwd_end(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, int cur, asr_stream s);

static inline int asr_dtype_ok(int dt) { return dt == ASR_F32 || dt == ASR_BF16; }
static inline size_t asr_dtype_size(int dt) { return dt == ASR_BF16 ? 2 : 4; }
