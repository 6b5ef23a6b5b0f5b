// What the decoder loops (dec_loop.hip) use of attention.hip's file scope: the launchers of the attention kernels with the
// operands the single-op entry points do not expose.  Internal to the library: none of it is exported.
#pragma once
#include "lstm_cell_bwd.h"

#pragma GCC visibility push(hidden)

// 0: not applicable, else LPF * 4 + NV  (A % 4 == 0, A <= 512, 16-byte aligned operands)
static inline int energy_vec_shape(int A, const void* keys, const void* qz, const void* v, const void* dkeys) {
  if (A % 4 != 0 || A > 512 || ((uintptr_t)keys | (uintptr_t)qz | (uintptr_t)v | (uintptr_t)dkeys) % 16 != 0) return 0;
  const int nvec = A / 4;
  return nvec <= 16 ? 16 * 4 + 1 : nvec <= 32 ? 32 * 4 + 1 : nvec <= 64 ? 64 * 4 + 1 : 64 * 4 + 2;
}

// the handle's scratch below the exchange area, or NULL when `bytes` do not fit
static inline float* att_scratch(asr_handle* h, size_t bytes) {
  return (bytes <= h->scratch_bytes - ASR_XCH_BYTES) ? (float*)h->scratch : nullptr;
}

struct SoftmaxBwdFold {        // see att_energy_bwd_vec_kernel
  const float* da;             // [B,T] d loss / d alpha  (NULL: not folded)
  const float* alpha;          // [B,T]
  const float* dotp;           // [ndot,B] partial sums of alpha . dalpha
  const float* norm;           // [B] sigmoid-smoothing normaliser or NULL
  int ndot;
  float sharp;
};

// energies + softmax + context of one decoder step as two launches (att_fused_fwd_kernel + combine); false = the shape is
// not covered (the caller takes the four-launch path).  ASR_ATT_FUSED=0 switches it off (A/B).
bool att_fused_step(asr_handle* h, const asr_att_decoder* a, const float* qz, float* alpha, float* ctx, float* ctx2,
                    int ld2, float* ctx3, int ld3, asr_stream s);

// the energy kernels behind asr_att_energy_* / asr_att_loc_energy_*, with the utterances' lengths (frames past them are
// skipped).  part_out / nch_out: the caller sums the chunk partials itself (att_dq_cell_bwd_launch does it on its
// operand load) -- no reduction launch, dqz / dv_rows are not written
int energy_fwd_launch(asr_handle* h, const float* keys, const float* qz, const float* v, int T, int B, int A, int mode,
                      float* energy, const int32_t* seq_len, asr_stream s);
int energy_bwd_launch(asr_handle* h, const float* denergy, const float* keys, const float* qz, const float* v, int T, int B,
                      int A, int mode, float* dkeys, float* dqz, float* dv_rows, const int32_t* seq_len,
                      const SoftmaxBwdFold* fold, asr_stream s, const float** part_out = nullptr, int* nch_out = nullptr);
int loc_energy_fwd_launch(asr_handle* h, const float* alpha_prev, const float* filt, const float* wfil, const float* keys,
                          const float* qz, const float* v, int T, int B, int A, int taps, float* energy,
                          const int32_t* seq_len, asr_stream s);
int loc_energy_bwd_launch(asr_handle* h, const float* denergy, const float* alpha_prev, const float* filt, const float* wfil,
                          const float* keys, const float* qz, const float* v, int T, int B, int A, int taps, float* dkeys,
                          float* dqz, float* dv_rows, float* dwfil_rows, float* dfilt_rows, float* dalpha_prev,
                          int accumulate, const int32_t* seq_len, asr_stream s);

// dctx = dctx_a (+ dctx_b with row stride ldb, may be NULL); the sum goes to dctx_out when that is given.
// fold (may be NULL): the caller's energy backward can take the softmax backward in (vectorised kernels on both sides,
// no carried-alpha gradient); when that applies, *fold is filled, denergy is NOT written and no softmax backward
// kernel is launched -- otherwise fold->da is left NULL and denergy holds the result as usual.
int softmax_ctx_bwd_launch(asr_handle* h, const float* dctx_a, const float* dctx_b, int ldb, float* dctx_out,
                           const float* alpha, const int32_t* seq_len, float sharpening, const void* enc, int enc_dtype,
                           int T, int B, int E, float* denergy, float* denc, const float* sigmoid_norm,
                           const float* dalpha_extra, SoftmaxBwdFold* fold, asr_stream s);

// query-FC backward + cell backward of one decoder step as one launch (att_dq_cell_bwd_kernel) on the energy backward's
// unreduced partials: U % DQ_CT == 0, A in {64, 128, 256, 512}, 16-byte aligned W_q / dqz / dv rows (the caller checks).
// DQ_NTL MFMA column tiles (16 units each) per workgroup: the measurements are with the kernel.
constexpr int DQ_NTL = 1, DQ_CT = 16 * DQ_NTL;
int att_dq_cell_bwd_launch(asr_handle* h, const float* part, int nch, int B, int A, int U, const float* Wq, int ldw,
                           const float* dcell, float* dqz, float* dv, const CellBwdArgs& c, asr_stream s);

#pragma GCC visibility pop
