/*
 * asr_hip.h -- C ABI of libasr_hip.so: MI355X (gfx950) kernels for the
 * BLSTM / VGG-BLSTM -> CTC / attention training + decode hot path of
 * hirofumi0810/tensorflow_end2end_speech_recognition.
 *
 * The reference is 100 % Python over TensorFlow 1.x; it has no FFI of its own.
 * The boundary below therefore stands in for the TensorFlow op call sites the
 * hot path dispatches to.  Each entry point cites the
 * reference call site it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - the caller owns every tensor and every per-call workspace argument (asr_*_workspace_bytes);
 *     the handle owns ONE scratch arena, allocated once by asr_create / asr_create_ex and reported by
 *     asr_scratch_bytes: deterministic split-K slabs and chunk partials of the calls that say so, and
 *     (its top 64 MiB) the exchange slots + error word of the multi-CU recurrence kernels.  A call
 *     that needs more than the arena holds returns ASR_ERR_WORKSPACE -- create the handle larger.
 *     No allocation and no synchronisation inside any call; everything is enqueued on `stream`;
 *   - row-major, contiguous unless a leading dimension (ld*) is given;
 *   - returns 0 on success, a negative asr_status otherwise;
 *     asr_last_error_string() explains the last failure on that handle;
 *   - one handle per GPU per process; calls on one handle are not thread-safe.
 *   - `dtype` selects the MFMA operand type of the matmul-shaped work:
 *     ASR_F32 = exact fp32 (v_mfma_f32_16x16x4_f32), ASR_BF16 = bf16 operands
 *     with fp32 accumulation (v_mfma_f32_16x16x32_bf16).  Gate math, cell
 *     state, CTC recursions, reductions and optimizer state are always fp32.
 */
#ifndef ASR_HIP_H_
#define ASR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct asr_handle asr_handle;
typedef void* asr_stream; /* hipStream_t */

typedef enum {
  ASR_OK = 0,
  ASR_ERR_INVALID_ARG = -1,
  ASR_ERR_UNSUPPORTED = -2,
  ASR_ERR_HIP = -3,
  ASR_ERR_WORKSPACE = -4
} asr_status;

typedef enum { ASR_F32 = 0, ASR_BF16 = 1 } asr_dtype;

/* tf.train.*Optimizer table of models/model_base.py:12-20 */
typedef enum {
  ASR_OPT_SGD = 0, ASR_OPT_MOMENTUM = 1, ASR_OPT_NESTEROV = 2, ASR_OPT_ADAGRAD = 3,
  ASR_OPT_ADADELTA = 4, ASR_OPT_RMSPROP = 5, ASR_OPT_ADAM = 6
} asr_optimizer;

/* ---- lifetime ------------------------------------------------------------ */
int asr_abi_version(void);                                         /* 5: round 6, additive (asr_lstm_bwd_ex; later within 5: the asr_conv3x5_* / asr_maxpool3x1_* entry points of cnn_zhang, then the asr_conv3x4_* / asr_bn_* / asr_softmax_xent_soft entry points of the student CNNs).  4: round 5, additive (asr_conv3x3_bwd_weight_bias, asr_conv3x3_smallc_bwd_weight_bias, asr_debug_* hooks).  3: round 4 (2: additions + the two size changes noted at asr_create_ex / asr_ctc_beam_workspace_bytes; 3: asr_att_decoder grew a trailing field) */
int asr_create(asr_handle** out, int device);                        /* 192 MiB scratch arena */
int asr_create_ex(asr_handle** out, int device, size_t scratch_bytes); /* >= 96 MiB (64 MiB of it: recurrence exchange areas) */
size_t asr_scratch_bytes(asr_handle* h);
int asr_destroy(asr_handle* h);
const char* asr_last_error_string(asr_handle* h);
/* Handles used for SIDE-stream work (weight-gradient GEMMs issued beside a recurrence kernel): the lean reduction-major
 * GEMM and its split-K reduction leave the first n XCDs (0 <= n <= 6) to the recurrence clusters, which sit on XCD
 * 0 .. (B/16)*ndir-1 and whose per-step hand-off goes through those XCDs' L2 (workgroup b of a 1-D grid runs on XCD
 * b % 8; workgroups that land on a skipped XCD retire at once).  Results are identical for every n. */
int asr_set_xcd_skip(asr_handle* h, int n);
/* Workgroups (output tiles x split-K slabs) the lean reduction-major GEMM (X^T dG, K = T*B) aims at on this handle;
 * 0 = the default (~2 per CU).  Weight-gradient GEMMs issued beside a recurrence kernel are given few (32: no split-K
 * slabs at all): they have a millisecond to finish and their slab traffic is what slows the recurrence down.  Results
 * differ only in the summation order of the K slabs (fixed for a given n: run-to-run deterministic). */
int asr_set_gemm_tn_workgroups(asr_handle* h, int n);
/* number of CUs / device name (for bench reporting) */
int asr_device_info(asr_handle* h, int* num_cu, char* name, int name_len);

/* ---- layout / elementwise ----------------------------------------------- */
/* [B,T,D] fp32 batch-major -> [T,B,D] time-major in `dtype`
 * (tf.transpose(inputs,[1,0,2]) at models/encoders/core/blstm.py:277-279). */
int asr_bt_to_tb(asr_handle* h, int dtype, const float* in_btd, void* out_tbd,
                 int B, int T, int D, asr_stream s);
/* same with output rows of ld_out >= D elements, columns D..ld_out-1 zero (the first layer's reduction width padded
 * to the GEMM's k tile, e.g. 120 -> 128) */
int asr_bt_to_tb_ld(asr_handle* h, int dtype, const float* in_btd, void* out_tbd,
                    int B, int T, int D, int ld_out, asr_stream s);
/* Batch assembly on the device.  Frame stacking / skipping of a zero-padded batch
 * x[B,T,F] (utils/io/inputs/frame_stacking.py:14-85): out[B, ceil(T/num_skip), F*num_stack], output frame k
 * = input frames k*num_skip .. +num_stack-1 side by side, zero where they run past the utterance;
 * out_len[b] = ceil(seq_len[b]/num_skip) (may be NULL).  num_stack < num_skip is an error as in the
 * reference (:30-31). */
int asr_stack_frames(asr_handle* h, const float* x, const int32_t* seq_len, int B, int T, int F,
                     int num_stack, int num_skip, float* out, int32_t* out_len, asr_stream s);
/* Context splicing per utterance over its own seq_len[b] frames (utils/io/inputs/splicing.py:9-73 as coded:
 * frames t-splice .. t-1 with first/last-frame replication, output laid out [channels][splice*num_stack][3]);
 * x[B,T,D], D = channels*3*num_stack; out[B,T,D*splice], zero for t >= seq_len[b]. */
int asr_splice(asr_handle* h, const float* x, const int32_t* seq_len, int B, int T, int D, int splice,
               int num_stack, float* out, asr_stream s);
/* Time subsampling between two recurrent layers (later within ABI 5; subsample_list / subsample_type of
 * examples/timit/config/ctc/regularization/blstm_ctc_subsample.yml and config/attention/att_baseline.yml; the 'concat'
 * form is the frame stacking of models/encoders/core/pyramidal_blstm.py:160-170 with its floor-halved lengths, :120-122).
 * One 2x reduction of the time-major x[T,Bp,W] in `dtype` (what a recurrence wrote) with frame counts len_in[Bp]:
 *   len_out[b] = len_in[b] >> 1 for all Bp rows (len_in clamped to [0,T]; an odd trailing frame is dropped),
 *   ASR_SUBSAMPLE_DROP  : y[b,t',:] = x[2t'+1,b,:]                  (W' = W; the forward direction has seen both frames)
 *   ASR_SUBSAMPLE_CONCAT: y[b,t',:] = [x[2t',b,:] ; x[2t'+1,b,:]]   (W' = 2W)
 * for t' < len_out[b] and zero for len_out[b] <= t' < T/2, written as the batch-major fp32 y[B, T/2, W'] (B <= Bp real
 * utterances) the next layer stack takes as its input.  x is never read at frames >= 2 len_out[b].  T/2 == 0 or B == 0:
 * only the lengths are written. */
typedef enum { ASR_SUBSAMPLE_DROP = 0, ASR_SUBSAMPLE_CONCAT = 1 } asr_subsample_type;
int asr_time_subsample_fwd(asr_handle* h, int dtype, int type, const void* x_tb, const int32_t* len_in, int T, int Bp,
                           int B, int W, float* y_bt, int32_t* len_out, asr_stream s);
/* Its exact transpose: dy[T/2,Bp,W'] fp32 time-major (the input gradient of the layer stack above) -> dx[T,Bp,W] fp32,
 * EVERY element written: drop dx[2t'+1] = dy[t'], concat dx[2t'] = dy[t'][:W] and dx[2t'+1] = dy[t'][W:] for
 * t' < len_out[b], zero everywhere else.  dy is never read at t' >= len_out[b]. */
int asr_time_subsample_bwd(asr_handle* h, int type, const float* dy_tb, const int32_t* len_out, int T, int Bp, int W,
                           float* dx_tb, asr_stream s);
/* Skip connections between two recurrent layers (later within ABI 5; encoder_residual / encoder_dense_residual of
 * config/ctc/encoders/residual_blstm_ctc.yml, dense_residual_blstm_ctc.yml, config/attention/encoders/
 * att_residual_blstm_location.yml, att_dense_residual_blstm_location.yml -- keys none of the reference's code reads; the
 * semantics are fixed in models/encoders/core/residual.py).  All tensors time-major [T,Bp,W]; seq_len[Bp] is clamped to
 * [0,T]; at t >= seq_len[b] nothing is loaded and every output is zero.  (keep_prob, seed, offset): the dropout mask
 * asr_dropout_mask would write for the [T,Bp,W] tensor with those arguments (element e: word e % 4 of the block at
 * offset + e / 4), formed in the kernel; keep_prob = 1: no dropout.
 * Forward: out = round_dtype(fl32(fl32(m * h) + skip)) with h, out in `dtype` and skip in skip_dtype (dtype or ASR_F32);
 * sum_out (nullable, fp32) = fl32(skip + out as stored) -- the running sum of the dense form; it may be `skip` itself when
 * that is fp32 (updated in place).  T == 0 or Bp == 0: nothing is launched. */
int asr_residual_fwd(asr_handle* h, int dtype, int skip_dtype, const void* h_tb, const void* skip,
                     const int32_t* seq_len, int T, int Bp, int W, float keep_prob, uint64_t seed, uint64_t offset,
                     void* out, float* sum_out, asr_stream s);
/* Backward (all fp32): g = fl32(dx_raw + carry); dout = fl32(m * g), what the layer's BPTT takes as its already-masked
 * output gradient; carry_out = g, or fl32(g + carry) with dense != 0 -- the un-masked gradient that travels further
 * down.  dout may be dx_raw and carry_out may be carry.  dx_raw may be unwritten memory at padded frames. */
int asr_residual_bwd(asr_handle* h, const float* dx_raw, const float* carry, const int32_t* seq_len, int T, int Bp,
                     int W, float keep_prob, uint64_t seed, uint64_t offset, int dense, float* dout, float* carry_out,
                     asr_stream s);
/* EXTENSION (later within ABI 5; weight_noise_std of config/ctc/regularization/blstm_ctc_weight_noise.yml (1e-5),
 * config/attention/regularization/att_blstm_location_weight_noise.yml and att_baseline.yml (1e-9) -- keys none of the
 * reference's code reads; Graves 2011 / 2013): Gaussian noise on a flat fp32 weight buffer for one training step, in one
 * pass:  backup[i] = w[i];  w[i] = fl32(w[i] + fl32(std * z[i])),  i < n.
 * z: Philox4x32-10 (the generator of asr_dropout_mask), block of counter {lo, hi, 0, 0} of offset + (i >> 2) under
 * key = seed; element 4q + j takes the word pair (c0, c1) for j = 0, 1 and (c2, c3) for j = 2, 3:
 *   u_a = ((c_even >> 8) + 1) 2^-24 in (0, 1],  u_b = (c_odd >> 8) 2^-24,  r = sqrt(-2 ln u_a),
 *   z = r cos(2 pi u_b) for even j, r sin(2 pi u_b) for odd j;  |z| <= 5.768.
 * ln / sin / cos are the accurate device-library forms: z is within 1e-5 of that statement in float64.  A slice that
 * starts at a multiple of 4 elements, called with offset + start / 4, gets the bits of the same elements of a whole-buffer
 * call.  std >= 0 and finite (else ASR_ERR_INVALID_ARG); std == 0 takes the backup and leaves w bit for bit.  backup must
 * not overlap w.  16-byte accesses where both pointers are 16-byte aligned, element by element otherwise and for the
 * n % 4 tail.  The clean weights come back by copying backup over w on the same stream; there is no entry point for it.
 * asr_weight_noise_counts: {calls, elements, calls on the 16-byte path} since the last reset. */
int asr_weight_noise_perturb(asr_handle* h, float* w, float* backup, size_t n, float std, uint64_t seed,
                             uint64_t offset, asr_stream s);
int asr_weight_noise_counts(asr_handle* h, unsigned long long* out3);
int asr_reset_weight_noise_counts(asr_handle* h);
/* EXTENSION (later within ABI 5; the reference declares _add_noise_to_inputs(inputs, stddev=0.075) at
 * models/model_base.py:40-55 with its body commented out; frequency / time masking: Park et al. 2019): input augmentation
 * of one training step in one pass over the batch-major features, x, y [B,T,F] fp32 contiguous, y must not overlap x (x is
 * never written), seq_len [B] int32 on the device, len_b = clamp(seq_len[b], 0, T).  For element i = (b T + t) F + f:
 *   1. t >= len_b (padded frame): y[i] gets the bits of x[i] -- no noise, no mask, a NaN is copied as it is.
 *   2. v = x[i]; with noise_std > 0: v = fl32(x[i] + fl32(noise_std * z_i)), z_i = word (i & 3) of the standard normal
 *      values of block offset + (i >> 2) under key = seed (the generator of asr_weight_noise_perturb, above); at
 *      noise_std == 0 nothing is added (-0.0 stays -0.0).
 *   3. masks: slot = one Philox4x32-10 block c = block(offset + 2^39 + 16 b + slot) under key = seed; frequency masks
 *      take slots 0 .. n_fmask-1, time masks slots 8 .. 8+n_tmask-1; mulhi(u, n) = (uint64(u) n) >> 32.
 *      frequency: Fcap = min(fmask_width, n_ch), fw = mulhi(c0, Fcap + 1), fs = mulhi(c1, n_ch - fw + 1); covers
 *        fs <= (f mod n_ch) < fs + fw -- the same band in every group of n_ch columns (static / delta / double-delta,
 *        stacked and spliced copies: columns are copies x 3 groups x n_ch);
 *      time: Tcap = min(tmask_width, (int)floorf(tmask_ratio * (float)len_b)) in fp32, tw = mulhi(c0, Tcap + 1),
 *        ts = mulhi(c1, len_b - tw + 1); covers ts <= t < ts + tw.
 *      A covered element becomes mask_value exactly, every other y[i] = v.
 * Counters used: noise offset + [0, 2^39), mask slots offset + 2^39 + [0, 16 B): calls at offset = k << 40 do not collide.
 * ASR_ERR_INVALID_ARG unless 1 <= n_ch <= F and F % n_ch == 0, 0 <= n_fmask, n_tmask <= 8, both widths >= 0,
 * 0 <= tmask_ratio <= 1, noise_std finite and >= 0, mask_value finite, B T F < 2^41.  One launch; 16-byte accesses for a
 * group of four flat elements where both pointers are 16-byte aligned and the group lies inside one utterance's valid (or
 * padded) frames, element by element otherwise; noise and masks all off: a device-to-device copy.
 * asr_input_augment_counts: {calls, elements, calls on the 16-byte path} since the last reset.
 * Call site: ModelBase._augment_inputs (a TRAINING compute_loss of CTC / MultitaskCTC / AttentionSeq2Seq /
 * JointCTCAttention, behind the upload of the inputs and lengths and in front of _build). */
int asr_input_augment(asr_handle* h, const float* x, float* y, const int32_t* seq_len, int B, int T, int F, int n_ch,
                      float noise_std, int n_fmask, int fmask_width, int n_tmask, int tmask_width, float tmask_ratio,
                      float mask_value, uint64_t seed, uint64_t offset, asr_stream s);
int asr_input_augment_counts(asr_handle* h, unsigned long long* out3);
int asr_reset_input_augment_counts(asr_handle* h);
/* out[c*ld_out + r] = in[r*ld_in + c] for an [rows, cols] matrix in `dtype` (LDS-tiled, both
 * sides coalesced).  The MFMA GEMM wants both operands reduction-contiguous; the k-major ones
 * (W_x as stored by TF: [Din, 4H], models/encoders/core/blstm.py:286-320 via LSTMBlockCell's
 * kernel) are transposed once per step instead of through bank-conflicting LDS scatter stores. */
int asr_transpose2d(asr_handle* h, int dtype, const void* in, int rows, int cols, int ld_in,
                    void* out, int ld_out, asr_stream s);
/* fp32 -> dtype cast / dtype -> fp32 of n elements (weight copies for the MFMA path) */
int asr_cast_from_f32(asr_handle* h, int dtype, const float* in, void* out, size_t n, asr_stream s);
int asr_cast_to_f32(asr_handle* h, int dtype, const void* in, float* out, size_t n, asr_stream s);
/* out[i] = in[i] * mask[i] (DropoutWrapper(output_keep_prob), blstm.py:308-311;
 * mask already holds 0 or 1/keep_prob).  in/out in `dtype`, mask fp32. */
int asr_apply_mask(asr_handle* h, int dtype, const void* in, const float* mask, void* out,
                   size_t n, asr_stream s);
/* Bernoulli(keep_prob)/keep_prob mask from a counter-based generator (seed, offset) */
/* Read pass over a device buffer (nothing is written): brings it into the memory-side cache ahead of a kernel whose
 * loads are latency-critical (the BPTT kernels' saved activations). */
int asr_touch(asr_handle* h, const void* p, size_t bytes, asr_stream s);
int asr_dropout_mask(asr_handle* h, float* mask, size_t n, float keep_prob,
                     uint64_t seed, uint64_t offset, asr_stream s);
/* The same mask formed where it is used (no mask tensor): out = in * mask(seed, offset) in `dtype`, bit-identical to
 * asr_dropout_mask + asr_apply_mask; and its backward through a ReLU, dpre = (out > 0 ? dout * mask : 0) =
 * asr_relu_bwd with that mask.  tf.nn.dropout on the gigabyte-sized activations of the VGG front-end
 * (vgg_blstm.py:121-157), where an fp32 mask would be three times the activation's own traffic. */
int asr_dropout_apply(asr_handle* h, int dtype, const void* in, void* out, size_t n, float keep_prob, uint64_t seed,
                      uint64_t offset, asr_stream s);
int asr_relu_bwd_drop(asr_handle* h, int dtype, const float* dout, const void* out, size_t n, float keep_prob,
                      uint64_t seed, uint64_t offset, void* dpre, asr_stream s);
/* out[N] = sum over rows of a[M,N] (bias gradients); a in `dtype`, out fp32 */
int asr_colsum(asr_handle* h, int dtype, const void* a, int M, int N, int lda,
               float* out, asr_stream s);

/* ---- GEMM (input projections, output FC, all backward contractions) ------ *
 * C[M,N] = op(A)[M,K] * op(B)[K,N] (+ bias[N]) (+ C if accumulate)
 * transA=0: A is [M,K] with lda; transA=1: A is stored [K,M] with lda.  Same for B.
 * A, B in `dtype`; C in `out_dtype`; bias fp32 or NULL.
 * Replaces fully_connected / the [x,h]W product of LSTMBlockCell hoisted over T
 * (models/ctc/ctc.py:198-233, models/encoders/core/blstm.py:286-320). */
int asr_gemm(asr_handle* h, int dtype, int out_dtype, int transA, int transB,
             int M, int N, int K, const void* A, int lda, const void* B, int ldb,
             void* C, int ldc, const float* bias, int accumulate, asr_stream s);

/* asr_gemm with a fused epilogue activation: act 0 = none, 1 = ReLU (conv_layer /
 * fully_connected(activation_fn=relu): models/encoders/core/cnn_util.py:78-84, vgg_blstm.py:165-173) */
int asr_gemm_act(asr_handle* h, int dtype, int out_dtype, int transA, int transB,
                 int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                 void* C, int ldc, const float* bias, int accumulate, int act, asr_stream s);
/* asr_gemm_act with fp32 output and an elementwise multiplier mul [M, N] (row stride ldmul, fp32) applied last:
 * C = act(op(A) op(B) + bias [+ C]) * mul.  The gradient of a layer input that went through a DropoutWrapper
 * (blstm.py:308-311: dx = dG W_x^T, then times the keep mask of the layer below) in one pass; same bits as
 * asr_gemm_act followed by asr_apply_mask. */
int asr_gemm_mul(asr_handle* h, int dtype, int transA, int transB, int M, int N, int K,
                 const void* A, int lda, const void* B, int ldb, float* C, int ldc,
                 const float* bias, int accumulate, int act, const float* mul, int ldmul, asr_stream s);
/* asr_gemm_mul whose multiplier is the dropout mask asr_dropout_mask(M*N, keep_prob, seed, offset) would produce, formed
 * in the epilogue from its Philox counter instead of read from a mask tensor (C contiguous: ldc == N, N % 4 == 0):
 * a recurrent layer's dx times the DropoutWrapper mask of the layer below (blstm.py:308-311), without that tensor. */
int asr_gemm_drop(asr_handle* h, int dtype, int transA, int transB, int M, int N, int K, const void* A, int lda,
                  const void* B, int ldb, float* C, int ldc, const float* bias, int accumulate, int act, float keep_prob,
                  uint64_t seed, uint64_t offset, asr_stream s);
/* The same products (fp32 output) on LISTED ROWS only: rows[0 .. num_rows) are row numbers of the [M, N] result, int32,
 * ASCENDING, each in [0, M), on the device.  Row rows[i] of C is computed from row rows[i] of A (with row rows[i] of
 * mul, or with the dropout mask of row rows[i] of the full [M, N] tensor) and gets, bit for bit, the value the full
 * product gives it.  Contract: the listed rows are written; every other row of C is EITHER left untouched OR written
 * with the full product's value -- the caller must not care which.  mul (or NULL) as asr_gemm_mul; keep_prob == 0: no
 * dropout, else as asr_gemm_drop (ldc == N, N % 4 == 0; not together with mul).  M, lda, ldc, ldmul describe the FULL
 * operands.  Where the lean NT kernels would take the full product (bf16 operands, transA = 0, transB = 1, K % 64 == 0,
 * N % 128 == 0, M >= 1024, 16-byte aligned rows) the launch covers ceil(num_rows / tile) row tiles instead of
 * ceil(M / tile); everywhere else the list is ignored and the full product runs as asr_gemm_mul / asr_gemm_drop run it.
 * num_rows == 0 launches nothing.  For intermediates whose unlisted rows are never used as values: the x-projection and
 * the between-layer dx of a recurrent stack at padded frames (models/encoders/core/rnn_util.py). */
int asr_gemm_rows(asr_handle* h, int dtype, int transA, int transB, int M, int N, int K, const void* A, int lda,
                  const void* B, int ldb, float* C, int ldc, const float* bias, int accumulate, int act,
                  const float* mul, int ldmul, float keep_prob, uint64_t seed, uint64_t offset, const int32_t* rows,
                  int num_rows, asr_stream s);
/* What the GEMM calls on this handle ran since the last reset (host integers bumped at launch time: no device
 * work, no synchronisation); out[i], i < min(n, ASR_GEMMP_N), in the order of the enum, the rest of `out` zeroed. */
enum {
  ASR_GEMMP_ROWS_128 = 0,         /* listed-row launches of the 128 x 128 NT kernel */
  ASR_GEMMP_ROWS_256,             /* listed-row launches of the 256 x 256 NT kernel */
  ASR_GEMMP_ROWS_FULL,            /* calls that ignored their list and ran the full product */
  ASR_GEMMP_TN_FRAMES,            /* asr_gemm_tn_frames calls on the lean TN kernel, padded frames not loaded */
  ASR_GEMMP_TN_FRAMES_GENERIC,    /* asr_gemm_tn_frames calls on the generic kernel (shape outside the lean TN path) */
  ASR_GEMMP_HEAD_BWD_LEAN,        /* asr_ctc_head_bwd calls on the lean NT kernels (listed rows where a list is given) */
  ASR_GEMMP_HEAD_BWD_FULL,        /* asr_ctc_head_bwd calls that ran the full generic product */
  /* The kernel a FULL product ended in: one of the next ten per product that asr_gemm / asr_gemm_act / asr_gemm_mul /
   * asr_gemm_drop ran.  The calls counted above that fall to the full product (ROWS_FULL, TN_FRAMES_GENERIC,
   * HEAD_BWD_FULL) run it through the same code and bump one of these as well; the listed-row launches, the lean
   * tn-frames launches and the lean head-bwd launches do not. */
  ASR_GEMMP_SKINNY_NN16,          /* skinny fp32 kernel (M <= 32), B row-major, 16 columns per workgroup */
  ASR_GEMMP_SKINNY_NN32,          /* the same, 32 columns per workgroup */
  ASR_GEMMP_SKINNY_NT16,          /* skinny fp32 kernel, B^T rows, 16 columns per workgroup */
  ASR_GEMMP_SKINNY_NT32,          /* the same, 32 columns per workgroup (N >= 6144) */
  ASR_GEMMP_NT128,                /* lean bf16 NT kernel, 128 x 128 tiles */
  ASR_GEMMP_NT256,                /* lean bf16 NT kernel, 256 x 256 tiles */
  ASR_GEMMP_TN_LEAN,              /* lean bf16 TN kernel + split-K reducer */
  ASR_GEMMP_GENERIC128,           /* generic kernel, 128 x 128 tiles */
  ASR_GEMMP_GENERIC64,            /* generic kernel, 64 x 64 tiles, one pass over K */
  ASR_GEMMP_GENERIC64_SPLITK,     /* generic kernel, 64 x 64 tiles, split-K slabs + reducer */
  ASR_GEMMP_MUL_PASS,             /* asr_gemm_mul calls whose multiplier ran as a second pass (mul_rows_kernel) */
  ASR_GEMMP_DROP_PASS,            /* asr_gemm_drop calls whose dropout ran as a second pass (asr_dropout_apply) */
  ASR_GEMMP_N
};
int asr_gemm_path_counts(asr_handle* h, unsigned long long* out, int n);
int asr_reset_gemm_path_counts(asr_handle* h);
/* C [M, N] fp32 (+= C with accumulate) = A^T B, A [K, M] and B [K, N] bf16, for operands whose K rows are the frames of a
 * time-major [T, Bp] batch: row k is utterance k % Bp at frame frame0 + k / Bp (K % Bp == 0; frame0 > 0 for a view that
 * starts at a later frame), seq_len [>= Bp] int32 on the device.  CONTRACT: B is exactly zero in every row of a padded
 * frame (frame >= seq_len[utterance]) -- the dgates the BPTT kernels write.  Those rows are then not loaded from either
 * operand (A may hold anything there), and the result is bit for bit asr_gemm's (transA = 1): the lean TN kernel with
 * the same tiles, split-K slabs and reducer where asr_gemm would take it, elsewhere the generic kernel asr_gemm runs for
 * the shape, with the same predicate on its loads. */
int asr_gemm_tn_frames(asr_handle* h, int M, int N, int K, const void* A, int lda, const void* B, int ldb, float* C,
                       int ldc, int accumulate, const int32_t* seq_len, int Bp, int frame0, asr_stream s);

/* ---- VGG front-end (models/encoders/core/vgg_blstm.py:107-177) --------------- *
 * Images are NHWC: [N = B*T frames, H = channels(40), W = splice*stack, C].
 * 3x3 SAME convolution = asr_im2col3x3 (patches[m, tap*Cin+ci], row stride ldp >= 9*Cin,
 * m = (n*H+h)*W+w) followed by asr_gemm_act(patches, weight[9*Cin, Cout], bias, relu);
 * backward: dW = patches^T dpre, dpatches = dpre W^T, asr_col2im3x3 gathers dpatches back. */
int asr_im2col3x3(asr_handle* h, int dtype, const void* in, int N, int H, int W, int Cin, int ldp,
                  void* patches, asr_stream s);
int asr_col2im3x3(asr_handle* h, const float* dpatches, int N, int H, int W, int Cin, int ldp,
                  float* din, asr_stream s);
/* General SAME convolution (NHWC x HWIO, any kernel / stride) as im2col + asr_gemm: conv_layer of the CLDNN front-end
 * (models/encoders/core/cldnn_wang.py:141-177: 11x21 stride (3,2), 11x11 stride (1,2), 3x3; cnn_util.py:50-84).
 * patches [N*Ho*Wo, ldp] (`dtype`), column (ky*kw + kx)*Cin + ci, Ho = ceil(H/sh), Wo = ceil(W/sw), TensorFlow's SAME
 * padding (the odd cell goes after).  asr_col2im: gradient w.r.t. the input from the gradient of the patches (fp32). */
int asr_im2col(asr_handle* h, int dtype, const void* in_nhwc, int N, int H, int W, int Cin, int kh, int kw,
               int sh, int sw, int ldp, void* patches, asr_stream s);
int asr_col2im(asr_handle* h, const float* dpatches, int N, int H, int W, int Cin, int kh, int kw,
               int sh, int sw, int ldp, float* din_nhwc, asr_stream s);
/* Implicit-GEMM form of the same 3x3 SAME convolution for bf16 operands (no patch matrix: a 64-wide
 * k-tile is one tap x 64 input channels, read straight from the NHWC image; conv_layer of
 * models/encoders/core/cnn_util.py:14-84, VGG blocks of vgg_blstm.py:113-157).
 *   prep:  from the HWIO fp32 master [3,3,Cin,Cout]: wt_fwd[Cout][9*Cin] and the flipped-tap image
 *          wt_bwd[Cin][9*Cout] (both bf16, reduction-contiguous);
 *   fwd:   out[N,H,W,Cout] bf16 = relu?(conv(x) + bias)             (Cin, Cout multiples of 64);
 *   bwd_data:   dx[N,H,W,Cin] fp32 = conv of dy (bf16) with wt_bwd;
 *   bwd_weight: dw[9*Cin, Cout] fp32 (+= if accumulate) = sum over pixels of x(shifted) (x) dy,
 *               deterministic split-K over the pixels through the handle scratch. */
int asr_conv3x3_prep_weights(asr_handle* h, const float* w_hwio, int Cin, int Cout, void* wt_fwd,
                             void* wt_bwd, asr_stream s);
int asr_conv3x3_fwd(asr_handle* h, const void* x, int N, int H, int W, int Cin, const void* wt_fwd,
                    const float* bias, int Cout, int relu, void* out, asr_stream s);
/* conv_layer + tf.nn.dropout (vgg_blstm.py:113-157) in one launch (round 4): out = dropout(round(relu(conv + bias))) with the
 * mask of asr_dropout_apply(keep_prob, seed, offset) formed in the epilogue -- bit for bit asr_dropout_apply of
 * asr_conv3x3_fwd's output; the undropped activation is never written (the backward needs only its sign where the mask
 * kept it: use_drop == 2 below). */
int asr_conv3x3_fwd_drop(asr_handle* h, const void* x, int N, int H, int W, int Cin, const void* wt_fwd,
                         const float* bias, int Cout, float keep_prob, uint64_t seed, uint64_t offset, void* out,
                         asr_stream s);
int asr_conv3x3_bwd_data(asr_handle* h, const void* dy, int N, int H, int W, int Cout,
                         const void* wt_bwd, int Cin, float* dx, asr_stream s);
/* asr_conv3x3_bwd_data followed by asr_relu_bwd(_drop) of the layer below, in the epilogue: dpre_below (bf16
 * [N,H,W,Cin]) = (act_below > 0) ? dx * dropout mask(seed, offset) : 0 -- the fp32 dx is never written.
 * use_drop: 0 no dropout, 1 the mask is formed from (keep_prob, seed, offset), 2 act_below IS the dropped activation
 * (asr_conv3x3_fwd_drop / asr_conv3x3_smallc_fwd_drop): it is > 0 exactly where active and kept, dx is scaled by 1 / keep. */
int asr_conv3x3_bwd_data_relu(asr_handle* h, const void* dy, int N, int H, int W, int Cout, const void* wt_bwd, int Cin,
                              const void* act_below, float keep_prob, uint64_t seed, uint64_t offset, int use_drop,
                              void* dpre_below, asr_stream s);
int asr_conv3x3_bwd_weight(asr_handle* h, const void* x, const void* dy, int N, int H, int W,
                           int Cin, int Cout, float* dw, int accumulate, asr_stream s);
/* the weight AND the bias gradient of a convolution layer (tf.nn.bias_add's gradient, cnn_util.py:49-84: dbias[Cout] =
 * column sums of dy over all N H W pixels) in one call: where the image-resident weight-gradient kernel applies, the bias
 * sums come from the dy images it has staged in LDS anyway (fixed summation order); otherwise this is
 * asr_conv3x3_bwd_weight followed by asr_colsum.  Both outputs are overwritten. */
int asr_conv3x3_bwd_weight_bias(asr_handle* h, const void* x, const void* dy, int N, int H, int W,
                                int Cin, int Cout, float* dw, float* dbias, asr_stream s);
/* tf.nn.max_pool 2x2 stride 2 SAME (cnn_util.py:13-28): out [N, ceil(H/2), ceil(W/2), C];
 * argmax (uint8, 0..3 = position in the window) drives the backward pass. */
int asr_maxpool2x2_fwd(asr_handle* h, int dtype, const void* in, int N, int H, int W, int C,
                       void* out, uint8_t* argmax, asr_stream s);
/* max_pool + tf.nn.dropout in one launch: out = dropout(round(max)) (== asr_dropout_apply of asr_maxpool2x2_fwd's output).
 * C % 4 == 0, 16-byte aligned arrays. */
int asr_maxpool2x2_fwd_drop(asr_handle* h, int dtype, const void* in, int N, int H, int W, int C, void* out,
                            uint8_t* argmax, float keep_prob, uint64_t seed, uint64_t offset, asr_stream s);
int asr_maxpool2x2_bwd(asr_handle* h, const float* dout, const uint8_t* argmax, int N, int H, int W,
                       int C, float* din, asr_stream s);
/* dpre = dout * (out > 0) (* mask if given), written in `dtype` (ReLU + dropout backward) */
/* 3x3 SAME convolution with few input channels (9 Cin <= 32, Cout == 64: the first VGG layer, vgg_blstm.py:113-121),
 * direct -- no patch matrix: out (bf16 [N,H,W,64]) = act(conv(x bf16 [N,H,W,Cin], w2d bf16 [9 Cin, 64]) + bias), and
 * its weight gradient dw fp32 [9 Cin, 64] = patches(x)^T dpre (dpre bf16 [N,H,W,64]; deterministic two-stage sum). */
int asr_conv3x3_smallc_fwd(asr_handle* h, const void* x, int N, int H, int W, int Cin, const void* w2d,
                           const float* bias, int Cout, int relu, void* out, asr_stream s);
int asr_conv3x3_smallc_fwd_drop(asr_handle* h, const void* x, int N, int H, int W, int Cin, const void* w2d,
                                const float* bias, int Cout, float keep_prob, uint64_t seed, uint64_t offset, void* out,
                                asr_stream s);      /* ReLU + dropout in the epilogue, as asr_conv3x3_fwd_drop */
int asr_conv3x3_smallc_bwd_weight(asr_handle* h, const void* x, const void* dpre, int N, int H, int W, int Cin,
                                  int Cout, float* dw, asr_stream s);
/* + the bias gradient dbias[64] = column sums of dpre, from a column of ones in the patch operand (as
 * asr_conv3x3_bwd_weight_bias) */
int asr_conv3x3_smallc_bwd_weight_bias(asr_handle* h, const void* x, const void* dpre, int N, int H, int W, int Cin,
                                       int Cout, float* dw, float* dbias, asr_stream s);
/* asr_dropout_apply (on the pooled gradient, when use_drop) -> asr_maxpool2x2_bwd -> asr_relu_bwd of the convolution
 * under the pool, as one pass without the full-resolution fp32 gradient in between: dpre[n,h,w,c] (operand dtype) =
 * (act[n,h,w,c] > 0 && argmax[o] == 2 (h & 1) + (w & 1)) ? dout[o] * mask(o) : 0, o = pooled cell (n, h/2, w/2, c).
 * C % 4 == 0, 16-byte aligned arrays.
 * use_drop == 2: `act` is the POOLED activation after its dropout ([N, ceil(H/2), ceil(W/2), C], asr_maxpool2x2_fwd_drop, or
 * the plain pooled output with keep_prob 1): dpre = (act[o] > 0 && argmax[o] == position) ? dout[o] / keep_prob : 0 -- the
 * full-resolution ReLU output is not read. */
int asr_maxpool2x2_relu_bwd(asr_handle* h, int dtype, const float* dout, const uint8_t* argmax, const void* act, int N,
                            int H, int W, int C, void* dpre, float keep_prob, uint64_t seed, uint64_t offset,
                            int use_drop, asr_stream s);
int asr_relu_bwd(asr_handle* h, int dtype, const float* dout, const void* out, const float* mask,
                 size_t n, void* dpre, asr_stream s);
/* dpre = (out > 0) ? dout * (1 / keep) : 0 with `out` a DROPPED ReLU output (asr_conv3x3_fwd_drop etc.): the same values as
   asr_relu_bwd_drop over the undropped output, without forming the mask */
int asr_relu_bwd_scaled(asr_handle* h, int dtype, const float* dout, const void* out, size_t n, float keep, void* dpre,
                        asr_stream s);

/* ---- the cnn_zhang convolution stack (later within ABI version 5, additive) ------------------------- *
 * conv_layer 3 (frequency) x 5 (time), SAME, stride 1 (cnn_util.py:50-84) of CNN2..CNN10, cnn_zhang.py:117-146, as
 * implicit GEMMs with bf16 operands and fp32 accumulation (no patch matrix), Cin and Cout multiples of 64:
 *   prep_weights: fp32 HWIO master [3][5][Cin][Cout] -> wt_fwd bf16 [Cout][15 Cin] and the flipped-tap image
 *                 wt_bwd bf16 [Cin][15 Cout] of the data gradient;
 *   fwd:          out bf16 [N,H,W,Cout] = relu?(conv(x bf16 [N,H,W,Cin]) + bias);
 *   fwd_drop:     + tf.nn.dropout in the epilogue, bit for bit asr_dropout_apply(keep_prob, seed, offset) of fwd's output;
 *   bwd_data:     dx fp32 [N,H,W,Cin] = conv of dy bf16 [N,H,W,Cout] with wt_bwd;
 *   bwd_data_relu: the same with the ReLU / dropout backward of the layer below in the epilogue, exactly as
 *                 asr_conv3x3_bwd_data_relu (use_drop 0 / 1 / 2) -> dpre_below bf16 [N,H,W,Cin];
 *   bwd_weight_bias: dw fp32 [15 Cin, Cout] and dbias fp32 [Cout] (NULL: skipped), overwritten; pixel-range slabs in the
 *                 handle scratch summed in a fixed order (bitwise reproducible), Cin and Cout multiples of 8. */
int asr_conv3x5_prep_weights(asr_handle* h, const float* w_hwio, int Cin, int Cout, void* wt_fwd, void* wt_bwd,
                             asr_stream s);
int asr_conv3x5_fwd(asr_handle* h, const void* x, int N, int H, int W, int Cin, const void* wt_fwd, const float* bias,
                    int Cout, int relu, void* out, asr_stream s);
int asr_conv3x5_fwd_drop(asr_handle* h, const void* x, int N, int H, int W, int Cin, const void* wt_fwd,
                         const float* bias, int Cout, float keep_prob, uint64_t seed, uint64_t offset, void* out,
                         asr_stream s);
int asr_conv3x5_bwd_data(asr_handle* h, const void* dy, int N, int H, int W, int Cout, const void* wt_bwd, int Cin,
                         float* dx, asr_stream s);
int asr_conv3x5_bwd_data_relu(asr_handle* h, const void* dy, int N, int H, int W, int Cout, const void* wt_bwd, int Cin,
                              const void* act_below, float keep_prob, uint64_t seed, uint64_t offset, int use_drop,
                              void* dpre_below, asr_stream s);
int asr_conv3x5_bwd_weight_bias(asr_handle* h, const void* x, const void* dy, int N, int H, int W, int Cin, int Cout,
                                float* dw, float* dbias, asr_stream s);
/* max_pool [3,1] stride [3,1] SAME of CNN1 (cnn_zhang.py:124-128, cnn_util.py:13-28): out [N, ceil(H/3), W, C]; the pad
 * rows go (3 ceil(H/3) - H) / 2 before and the rest after (F = 40: 1 / 1, F = 41: 0 / 1) and are never selected;
 * argmax (uint8, 0..2 = row in the window) takes the first of equal values.  use_drop: tf.nn.dropout of the pooled output
 * in the same pass (== asr_dropout_apply(keep_prob, seed, offset) of it).  C % 4 == 0.
 * bwd: gather form, din (same dtype and shape as the input) = dout of the window where the row was its maximum, else 0. */
int asr_maxpool3x1_fwd(asr_handle* h, int dtype, const void* in, int N, int H, int W, int C, void* out, uint8_t* argmax,
                       float keep_prob, uint64_t seed, uint64_t offset, int use_drop, asr_stream s);
int asr_maxpool3x1_bwd(asr_handle* h, int dtype, const void* dout, const uint8_t* argmax, int N, int H, int W, int C,
                       void* din, asr_stream s);

/* ---- the student CNNs (later within ABI version 5, additive) ------------------------------------------ *
 * conv_layer 3 (frequency) x 4 (time), SAME (one column before, two after), stride 1, of CNN2
 * (student_cnn_ctc.py:111-117, student_cnn_compact_ctc.py, student_cnn_xe.py:103-109, student_cnn_compact_xe.py): the
 * asr_conv3x5_* kernels on the 12-tap geometry, Cin and Cout multiples of 64.  prep_weights: fp32 HWIO [3][4][Cin][Cout]
 * -> wt_fwd bf16 [Cout][12 Cin], wt_bwd bf16 [Cin][12 Cout] (flipped taps); fwd: out = relu?(conv(x) + bias), bf16 or
 * (out_f32) fp32 [N,H,W,Cout]; bwd_data: dx fp32 [N,H,W,Cin]; bwd_weight_bias: dw fp32 [12 Cin, Cout], dbias fp32 [Cout]
 * (NULL: skipped), overwritten, fixed-order slab sum. */
int asr_conv3x4_prep_weights(asr_handle* h, const float* w_hwio, int Cin, int Cout, void* wt_fwd, void* wt_bwd,
                             asr_stream s);
int asr_conv3x4_fwd(asr_handle* h, const void* x, int N, int H, int W, int Cin, const void* wt_fwd, const float* bias,
                    int Cout, int relu, int out_f32, void* out, asr_stream s);
int asr_conv3x4_bwd_data(asr_handle* h, const void* dy, int N, int H, int W, int Cout, const void* wt_bwd, int Cin,
                         float* dx, asr_stream s);
int asr_conv3x4_bwd_weight_bias(asr_handle* h, const void* x, const void* dy, int N, int H, int W, int Cin, int Cout,
                                float* dw, float* dbias, asr_stream s);
/* batch_normalization (cnn_util.py:87-149: eps 1e-3, momentum 0.9, non-fused) over fp32 NHWC activations
 * [M = N H W rows, C channels], C % 64 == 0; `ws` holds asr_bn_workspace_bytes(M, C) bytes.
 *   stats: tf.nn.moments over all M rows (biased variance), fixed-order Chan merges -> stats fp32 [5][C] = mean, var,
 *          rstd = 1 / sqrt(var + eps), and (when avg_mean / avg_var are given) the pending moving averages
 *          avg * momentum + stat * (1 - momentum) of the UPDATE_OPS (cnn_util.py:138-145), for the caller to commit;
 *   apply: tf.nn.batch_normalization(x, mean, var, beta, gamma, eps) (cnn_util.py:133-134; mean / var = the batch
 *          statistics or the moving averages) fused with the following max_pool: pool 1 = [3,1] / [3,1] SAME over H
 *          (argmax as asr_maxpool3x1_fwd), pool 0 = [1,1] (identity); out in out_dtype;
 *   bwd:   dz = gradient at the pooled output (fp32), stats = what asr_bn_stats returned; dgamma = sum(dy xhat), dbeta =
 *          sum(dy) (fixed order, overwritten), dx = gamma rstd (dy - dbeta / M - xhat dgamma / M), zero where x <= 0
 *          when relu_gate (x = the ReLU output the statistics were taken over), in out_dtype. */
size_t asr_bn_workspace_bytes(long long M, int C);
int asr_bn_stats(asr_handle* h, const float* x, long long M, int C, float eps, float momentum, const float* avg_mean,
                 const float* avg_var, float* stats, void* ws, asr_stream s);
int asr_bn_apply(asr_handle* h, int out_dtype, const float* x, int N, int H, int W, int C, const float* mean,
                 const float* var, const float* gamma, const float* beta, float eps, int pool, void* out,
                 uint8_t* argmax, asr_stream s);
int asr_bn_bwd(asr_handle* h, int out_dtype, const float* dz, const uint8_t* argmax, int pool, const float* x, int N,
               int H, int W, int C, const float* stats, const float* gamma, int relu_gate, float* dgamma, float* dbeta,
               void* dx, void* ws, asr_stream s);
/* tf.nn.softmax_cross_entropy_with_logits(labels = targets, logits) of StudentCTC.compute_xe_loss
 * (student_ctc.py:321-327): row_loss[r] = -sum_c targets log softmax(logits); dlogits (NULL: skipped) = TF's gradient
 * (softmax(logits) - targets) * grad_scale.  One block per row, fixed reduction order. */
int asr_softmax_xent_soft(asr_handle* h, const float* logits, const float* targets, int rows, int C, float grad_scale,
                          float* row_loss, float* dlogits, asr_stream s);

/* ---- LSTM recurrence ------------------------------------------------------ *
 * One layer, `ndir` directions (1 = LSTMEncoder, 2 = BLSTMEncoder), all T steps:
 * tf.contrib.rnn.LSTMBlockCell(forget_bias, clip_cell, use_peephole) under
 * tf.nn.(bidirectional_)dynamic_rnn(sequence_length) --
 * models/encoders/core/blstm.py:286-323, lstm.py:253-285.
 *
 * Gate layout.  The TF variable `kernel` [Din+H, 4H] has gate-major columns q*H + j
 * (q = i, ci, f, o).  The device-side activation tensors keep the four gates of a unit
 * INTERLEAVED (column j*4 + q) so that the recurrence kernels move one 16-byte (fp32) or
 * 8-byte (bf16) quadruple per (utterance, unit) pair:
 *     xproj / gates / dgates : [T, B, ndir, H, 4]
 *
 * asr_lstm_prep_weights: once per (layer, direction) per step, from kernel/bias (fp32):
 *   wx_il   [Din, 4H] `dtype`  W_x with interleaved columns (B operand of the hoisted GEMM)
 *   bias_il [4H] fp32          bias, interleaved
 *   packed_fwd / packed_bwd    W_h = kernel[Din:] in MFMA B-fragment order for
 *                              h[16,H] x W_h  and  dG[16,4H] x W_h^T   (H*4H `dtype` each) */
int asr_lstm_prep_weights(asr_handle* h, int dtype, const float* kernel, const float* bias,
                          int Din, int H, void* wx_il, float* bias_il,
                          void* packed_fwd, void* packed_bwd, asr_stream s);
/* asr_lstm_prep_layer: the same images for ALL directions of a layer in one launch, in the form the layer's GEMMs
 * consume (no transposes / concatenations afterwards).  vars[ndir*5] (host array of device pointers), per direction:
 * {kernel [Din+H,4H], bias [4H], w_i_diag, w_f_diag, w_o_diag [H]} -- the five tf.get_variable()s of one
 * LSTMBlockCell (blstm.py:287-305; SURVEY App. C names); the peephole pointers may be NULL iff peep_out is NULL.
 *   wxT     [ndir*4H, ldk] `dtype`  W_x^T, interleaved rows, directions stacked, columns Din..ldk-1 zero
 *                                   (xproj = x [T*B, ldk] . wxT^T: one GEMM for both directions)
 *   wx_cat  [Din, ndir*4H] `dtype`  W_x, interleaved columns, directions side by side (dx = dG . wx_cat^T)
 *   bias_cat[ndir*4H] fp32, packed_fwd / packed_bwd [ndir][H*4H] `dtype`, peep_out [ndir][3][H] fp32 */
int asr_lstm_prep_layer(asr_handle* h, int dtype, int ndir, const float* const* vars, int Din, int ldk, int H,
                        void* wxT, void* wx_cat, float* bias_cat, void* packed_fwd, void* packed_bwd,
                        float* peep_out, asr_stream s);
/* asr_lstm_prep_layers: the images of asr_lstm_prep_layer for a whole stack of layers, byte for byte, in ONE launch
 * (one per 16 layers beyond that).  `layers`: host array of nlayers descriptors, read during the call only (they travel
 * in the kernel arguments: no device table, no copy on the stream); every field means what the argument of the same
 * name means to asr_lstm_prep_layer.  All layers share `dtype`.  Nothing is launched if any descriptor is refused. */
typedef struct asr_lstm_prep_desc {
  int ndir;
  const float* const* vars;
  int Din, ldk, H;
  void *wxT, *wx_cat;
  float* bias_cat;
  void *packed_fwd, *packed_bwd;
  float* peep_out;
} asr_lstm_prep_desc;
int asr_lstm_prep_layers(asr_handle* h, int dtype, int nlayers, const asr_lstm_prep_desc* layers, asr_stream s);
/* asr_lstm_grad_finish: the way back for one layer's gradients, one launch.  dw_il [ndir][rows = Din+H][4H] fp32 with
 * interleaved columns (output of the weight-gradient GEMMs) and dpeep_dbias [ndir][7][H] (asr_lstm_bwd) are written
 * to grads[ndir*5] = the gradient buffers of the same five variables, in TF's layouts (kernel gate-major). */
int asr_lstm_grad_finish(asr_handle* h, int ndir, float* const* grads, int rows, int H, const float* dw_il,
                         const float* dpeep_dbias, int has_peep, asr_stream s);
/* [rows, 4H] fp32 with interleaved columns -> gate-major columns (dW after the GEMMs) */
int asr_gate_deinterleave(asr_handle* h, const float* in, int ld_in, float* out, int ld_out,
                          int rows, int H, asr_stream s);

/* Forward.  xproj[T,B,ndir,H,4] fp32 = x*wx_il + bias_il (from asr_gemm).
 * wh_packed: ndir fwd-packed buffers back to back.  peep: [ndir][3][H] fp32
 * (w_i_diag, w_f_diag, w_o_diag) or NULL (use_peephole=False).
 * gates[T,B,ndir,H,4] `dtype`: post-activation i, ci, f, o (valid frames only);
 * hout[T,B,ndir*H] `dtype`: cell outputs, zero for t >= seq_len[b];
 * cs[T,B,ndir*H] fp32: cell state per frame (after clipping);
 * c_final/h_final [ndir][B][H] fp32 (may be NULL): state at the last valid step.
 * cell_clip <= 0 disables clipping.  B must be a multiple of 16 (pad with
 * seq_len 0 rows); H in {64,128,192,256,320,512}. */
int asr_lstm_fwd(asr_handle* h, int dtype, int T, int B, int H, int ndir,
                 const float* xproj, const void* wh_packed, const float* peep,
                 const int32_t* seq_len, float forget_bias, float cell_clip,
                 void* gates, void* hout, float* cs, float* c_final, float* h_final,
                 asr_stream s);

/* Backward through time.  dhout[T,B,ndir*H] fp32: gradient w.r.t. hout (already
 * multiplied by the dropout mask if any).  d_c_final/d_h_final [ndir][B][H] or NULL.
 * gates/cs from forward.  wh_packed_bwd: ndir bwd-packed buffers.
 * dgates[T,B,ndir,H,4] in `dtype`: gradient w.r.t. the pre-activations (interleaved, zero
 * at padded frames) -- feeds the dW_x, dW_h, dx GEMMs.
 * dpeep_dbias [ndir][7][H] fp32 (may be NULL; overwritten): rows 0-2 = gradients of the
 * peepholes (w_i_diag, w_f_diag, w_o_diag), rows 3-6 = gradient of the bias, i.e. the column
 * sums of dgates per gate block (i, ci, f, o) -- accumulated in registers during BPTT.
 * dpeep_workspace: (B/16)*ndir*7*H floats (per batch-tile partials, reduced in a fixed
 * order so the result is run-to-run deterministic); required iff dpeep_dbias != NULL. */
int asr_lstm_bwd(asr_handle* h, int dtype, int T, int B, int H, int ndir,
                 const float* dhout, const void* gates, const float* cs,
                 const void* wh_packed_bwd, const float* peep, const int32_t* seq_len,
                 const float* d_c_final, const float* d_h_final,
                 void* dgates, float* dpeep_dbias, float* dpeep_workspace, asr_stream s);
/* The same with clip_no_grad: 0 = asr_lstm_bwd (LSTMBlockCell: the fused gradient op does not know cell_clip, the clip is
 * straight-through).  > 0 = the forward ran with cell_clip = clip_no_grad and the cell is tf.contrib.rnn.LSTMCell
 * (models/encoders/core/blstm.py:187-230 of the reference, the num_proj cell), whose tf.clip_by_value passes NO gradient
 * through a clamped state: a frame whose saved cs has |c| >= clip_no_grad sends nothing to its gates or to c_prev
 * (its output gate still receives its gradient).  Either operand dtype. */
int asr_lstm_bwd_ex(asr_handle* h, int dtype, int T, int B, int H, int ndir,
                    const float* dhout, const void* gates, const float* cs,
                    const void* wh_packed_bwd, const float* peep, const int32_t* seq_len,
                    const float* d_c_final, const float* d_h_final, float clip_no_grad,
                    void* dgates, float* dpeep_dbias, float* dpeep_workspace, asr_stream s);

/* The recurrences run as clusters of H/32 (or H/64) workgroups per (direction, 16-utterance tile) that hand their
 * slices of h / dh to each other inside the launch (bounded spins).  This synchronises the device and reports the
 * sticky error word (ASR_ERR_HIP when non-zero) -- call at a sync point.  Bits: 1 = a forward hand-off timed out,
 * 2 = a backward hand-off timed out (never expected), 4 = a bf16 forward recurrence published a NON-FINITE hidden state
 * (the model diverged: its 4-byte self-tagged exchange words would otherwise hand the peers a finite value).
 * Saved activations (gates, cs) of frames past an utterance's length are UNSPECIFIED (rows past their length park
 * their accesses): only asr_lstm_bwd consumes them and it never reads those positions; hout and dgates ARE
 * zero there. */
int asr_check_async_errors(asr_handle* h, unsigned* flags_out);
/* Non-blocking form for training loops: enqueues ONE 4-byte device->host copy of the sticky error word on `s` into
 * host_flags (pinned host memory owned by the caller; valid once work on `s` up to here has completed) -- the Python
 * front end arms it after every optimizer step and inspects the previous step's word (ops.ErrorWatch), so a timed-out
 * hand-off raises within one step instead of silently training on garbage. */
int asr_peek_async_errors(asr_handle* h, unsigned* host_flags, asr_stream s);
/* Resets the sticky error word (after it has been reported). */
int asr_clear_async_errors(asr_handle* h, asr_stream s);
/* Debug / test switches of the cluster kernels (process-wide, same bits as the environment variable ASR_LSTM_DFLAGS):
 * 16 = force the placement-independent write-through exchange, 64 = TEST ONLY, make every hand-off time out;
 * 32 / 128 / 256 = A-B switches of kernel variants (own-slice products ahead of the poll, the BPTT kernel's fetch ahead of
 * its poll loop, MFMA priority in the fp32 BPTT kernel), result-neutral; 512 = clusters of H/64 CUs x eight waves instead
 * of H/32 CUs x four (H = 256 / 512). */
int asr_debug_set_lstm_flags(int flags);
/* 1 (default; env ASR_GRU_PERSISTENT): asr_gru_fwd / asr_gru_bwd run ONE launch per call -- for 64 / 128 / 256 / 320 units on
 * clusters of H/32 CUs (round 6: the recurrent blocks as three-bf16-term fragments in registers, two all-gathers per step;
 * env ASR_GRU_CLUSTER=0 keeps the single-CU form), else on one CU per (direction, tile) with the state in LDS and both
 * products on exact-fp32 MFMA where the LDS images fit; 0: the launch-per-step kernels. */
int asr_debug_set_gru_persistent(int on);

/* Tile groups of the cluster recurrences.  A cluster launch needs every workgroup resident at once, one per CU:
 * 8 * G * ceil(clusters / 8) of them, G = workgroups per cluster (H/32 or H/64), clusters = tiles * ndir, tiles = B / 16.
 * A batch that needs more than the chip has runs as several launches over consecutive tile ranges on the caller's
 * stream (asr_lstm_fwd / asr_lstm_bwd / asr_gru_fwd / asr_gru_bwd do this by themselves; results are bit-identical to one
 * launch).  This is the plan they use -- pure integer arithmetic, no handle, no GPU: the minimal number of groups
 * {first_tile[i], ntiles[i]}, consecutive and covering [0, tiles), each with 8 * G * ceil(ntiles * ndir / 8) <= cu_budget.
 * Returns the number of groups (at most max_groups of them are written; either array may be NULL), 0 when not even one
 * tile fits (the callers then run the single-CU kernels), ASR_ERR_INVALID_ARG on bad arguments. */
int asr_cluster_tile_groups(int G, int ndir, int tiles, int cu_budget, int* first_tile, int* ntiles, int max_groups);
/* Which path the recurrence calls on this handle took since the last reset (host integers bumped at launch time, no
 * device work, no synchronisation): out6 = {LSTM cluster launches (one per tile group), LSTM single-CU calls, LSTM calls
 * split into more than one tile group, and the same three for the GRU (its launch-per-step form counts as one
 * single-CU call)}.  Single-CU calls at a cluster width are the slow path (1.2 - 3.6 x per training step where
 * measured). */
int asr_recurrence_path_counts(asr_handle* h, unsigned long long* out6);
int asr_reset_recurrence_path_counts(asr_handle* h);
/* The form each asr_gru_fwd / asr_gru_bwd call on this handle ended in since the last reset (host integers like the ones
 * above, one bumped per call where the form is chosen): out6 = {forward on clusters, forward persistent on one CU per
 * (direction, tile), forward launched per step, and the same three for the backward}.  The counters above are left as
 * they are: both single-CU forms count there as one single-CU call. */
int asr_gru_kernel_counts(asr_handle* h, unsigned long long* out6);
int asr_reset_gru_kernel_counts(asr_handle* h);
/* The same for the LSTM recurrence: the form each asr_lstm_fwd / asr_lstm_bwd(_ex) call on this handle ended in since the
 * last reset.  One counter is bumped per call where the form is chosen (a call that runs as several tile groups counts
 * once); out[i], i < min(n, ASR_LSTM_KERNEL_N), in the order of the enum below, the rest of `out` zeroed.  The template
 * choices inside a form (EARLY, exchange word format, slot layout, CLIPZ, write-through) are not counted: the flags of
 * asr_debug_set_lstm_flags set them directly.  asr_recurrence_path_counts is left as it is. */
enum {
  ASR_LSTM_FWD_BF16_CU16 = 0,     /* bf16, H = 256 on clusters of 16 CUs (lstm_fwd_cluster16_kernel) */
  ASR_LSTM_FWD_BF16_HS32,         /* bf16 clusters, 32 units per CU (H = 256, 512) */
  ASR_LSTM_FWD_BF16_HS64,         /* bf16 clusters, 64 units per CU (H = 256, 320, 512) */
  ASR_LSTM_FWD_F32_SPLIT,         /* fp32 as three bf16 terms, 32 units per CU (lstm_fwd_cluster_f32_kernel under OpSplit3; H = 128, 256) */
  ASR_LSTM_FWD_F32_HS32,          /* exact fp32 clusters, 32 units per CU (H = 128, 256, 320, 512) */
  ASR_LSTM_FWD_F32_HS64,          /* exact fp32 clusters, 64 units per CU (H = 128) */
  ASR_LSTM_FWD_SINGLE_BF16,       /* lstm_fwd_kernel<bf16>, one CU per (direction, tile) */
  ASR_LSTM_FWD_SINGLE_F32,        /* lstm_fwd_kernel<float> */
  ASR_LSTM_BWD_BF16_HS32,         /* bf16 BPTT clusters, 32 units per CU (H = 256, 512) */
  ASR_LSTM_BWD_BF16_HS64,         /* bf16 BPTT clusters, 64 units per CU (H = 256, 320, 512) */
  ASR_LSTM_BWD_F32_SPLIT,         /* lstm_bwd_cluster_f32_kernel under OpSplit3 (H = 128, 256) */
  ASR_LSTM_BWD_F32_HS32,          /* lstm_bwd_cluster_f32_kernel under OpF32, 32 units per CU (H = 128, 256, 320, 512) */
  ASR_LSTM_BWD_F32_HS64,          /* lstm_bwd_cluster8_f32_kernel, 64 units per CU (H = 128) */
  ASR_LSTM_BWD_SINGLE_BF16,       /* lstm_bwd_kernel<bf16> */
  ASR_LSTM_BWD_SINGLE_F32,        /* lstm_bwd_kernel<float> */
  ASR_LSTM_KERNEL_N
};
int asr_lstm_kernel_counts(asr_handle* h, unsigned long long* out, int n);
int asr_reset_lstm_kernel_counts(asr_handle* h);
/* Which kernels the attention decoder calls on this handle launched since the last reset (host integers bumped at
 * launch time like the recurrence counters above: no device work, no synchronisation, no effect on any launch).
 * out[i], i < min(n, ASR_ATT_PATH_N), in the order of the enum below; entries of `out` past ASR_ATT_PATH_N are zeroed.
 * The step counters count decoder-loop steps (asr_att_decoder_fwd / _infer / _bwd); the lane-shape counters count
 * launches, whether they come from a loop or from the single-kernel entry points (asr_att_energy_fwd, ...). */
enum {
  ASR_ATT_FWD_STEP_FUSED = 0,     /* energies + softmax + context as att_fused_fwd_kernel + combine */
  ASR_ATT_FWD_STEP_4LAUNCH,       /* energy kernel, softmax, context partials, reduction */
  ASR_ATT_FWD_CELL_BF16,          /* product + cell in one launch on the bf16 weight image */
  ASR_ATT_FWD_CELL_F32IMG,        /* product + cell in one launch on the fp32 gate-interleaved image */
  ASR_ATT_FWD_CELL_GEMM,          /* asr_gemm_act, then the cell kernel */
  ASR_ATT_BWD_STEP_FUSED_Q,       /* query-FC backward + cell backward + partial sums in one launch */
  ASR_ATT_BWD_STEP_UNFUSED,       /* reduction, GEMM or column add, cell backward */
  ASR_ATT_BWD_CELL_BF16,          /* dpre W^T on the bf16 weight rows */
  ASR_ATT_BWD_CELL_GEMM,          /* dpre W^T by asr_gemm_act */
  ASR_ATT_BWD_SOFTMAX_FOLDED,     /* softmax backward inside the energy backward */
  ASR_ATT_BWD_SOFTMAX_SEPARATE,   /* its own kernel */
  ASR_ATT_ENERGY_FWD_L16, ASR_ATT_ENERGY_FWD_L32, ASR_ATT_ENERGY_FWD_L64, ASR_ATT_ENERGY_FWD_L64X2, ASR_ATT_ENERGY_FWD_GENERAL,
  ASR_ATT_ENERGY_BWD_L16, ASR_ATT_ENERGY_BWD_L32, ASR_ATT_ENERGY_BWD_L64, ASR_ATT_ENERGY_BWD_L64X2, ASR_ATT_ENERGY_BWD_GENERAL,
  ASR_ATT_LOC_FWD_L16, ASR_ATT_LOC_FWD_L32, ASR_ATT_LOC_FWD_L64, ASR_ATT_LOC_FWD_GENERAL,
  ASR_ATT_LOC_BWD_L16, ASR_ATT_LOC_BWD_L32, ASR_ATT_LOC_BWD_L64, ASR_ATT_LOC_BWD_GENERAL,
  ASR_ATT_FUSED_FWD_L16, ASR_ATT_FUSED_FWD_L32, ASR_ATT_FUSED_FWD_L64, ASR_ATT_FUSED_FWD_L64X2,   /* lanes of the fused step */
  ASR_ATT_PATH_N
};
int asr_att_path_counts(asr_handle* h, unsigned long long* out, int n);
int asr_reset_att_path_counts(asr_handle* h);
/* The same for the 3x3 convolution entry points (asr_conv3x3_fwd / _fwd_drop / _bwd_data / _bwd_data_relu / _bwd_weight /
 * _bwd_weight_bias): which kernel instantiation each launch on this handle was, since the last reset.  Host integers
 * bumped at the launch site; out[i], i < min(n, ASR_CONVP_N), in the order of the enum below, the rest of `out` zeroed.
 * A forward or data-gradient launch bumps its form and the channel pair of its product (the data gradient of a Cin ->
 * Cout layer is a Cout -> Cin product); an image-resident one also the instantiated MAXV (staged vectors per thread),
 * the compile-time epilogue ACT, the number of LDS image buffers and STREAM / W8 when that variant ran; a tiled one the
 * column width of its conv_nt_kernel tiles.  A weight-gradient call bumps exactly one of the WGRAD_IMG_* / WGRAD_TR_* /
 * WGRAD_COLPIX forms, and for the image-resident forms SPLIT (two waves per input-channel group), BIAS_IN_KERNEL (bias
 * gradient from the staged dY) and, with BIAS_IN_KERNEL, the reduce kernel that summed the slabs. */
enum {
  ASR_CONVP_FORM_IMG = 0,         /* conv3x3_img_kernel: the image with its border in LDS, weights in registers */
  ASR_CONVP_FORM_TILED,           /* conv_nt_kernel on the 3x3 tap geometry */
  ASR_CONVP_PAIR_64_64, ASR_CONVP_PAIR_64_128, ASR_CONVP_PAIR_128_128, ASR_CONVP_PAIR_128_64,
  ASR_CONVP_PAIR_OTHER,           /* any other channel pair of the product (always tiled) */
  ASR_CONVP_MAXV_2, ASR_CONVP_MAXV_4, ASR_CONVP_MAXV_8, ASR_CONVP_MAXV_14, ASR_CONVP_MAXV_16,
  ASR_CONVP_ACT_0,                /* no epilogue (and every fp32 data gradient) */
  ASR_CONVP_ACT_1,                /* ReLU */
  ASR_CONVP_ACT_2,                /* data gradient gated by the layer below, uniform scale (use_drop 0 / 2) */
  ASR_CONVP_ACT_3,                /* forward ReLU + dropout */
  ASR_CONVP_ACT_4,                /* gated data gradient with the Philox mask (use_drop 1) */
  ASR_CONVP_NBUF_1, ASR_CONVP_NBUF_2,
  ASR_CONVP_STREAM,               /* the next image streamed into the second buffer two vectors per pixel tile */
  ASR_CONVP_W8,                   /* eight waves (forward ReLU + dropout of small 64-channel images) */
  ASR_CONVP_TILED_BN128, ASR_CONVP_TILED_BN64,
  ASR_CONVP_WGRAD_IMG_64_SMALL,   /* conv3x3_wgrad_img_kernel, 64 input channels, at most 4 staged vectors per thread */
  ASR_CONVP_WGRAD_IMG_64_LARGE,   /* ... 5 to 14 */
  ASR_CONVP_WGRAD_IMG_128,        /* ... 128 input channels */
  ASR_CONVP_WGRAD_SPLIT,
  ASR_CONVP_WGRAD_BIAS_IN_KERNEL,
  ASR_CONVP_WGRAD_REDUCE_VEC,     /* wgrad_img_reduce_kernel<1>: dw 16-byte aligned */
  ASR_CONVP_WGRAD_REDUCE_SCALAR,  /* wgrad_img_reduce_kernel<0> */
  ASR_CONVP_WGRAD_TR_128,         /* conv3x3_wgrad_tr_kernel<128> */
  ASR_CONVP_WGRAD_TR_64,          /* conv3x3_wgrad_tr_kernel<64> (ASR_CONV_WGRAD_BN64=1) */
  ASR_CONVP_WGRAD_COLPIX,         /* conv_wgrad_kernel on the [column][pixel] LDS image (ASR_CONV_WGRAD_TR=0) */
  ASR_CONVP_N
};
int asr_conv_path_counts(asr_handle* h, unsigned long long* out, int n);
int asr_reset_conv_path_counts(asr_handle* h);
/* TEST ONLY (process-wide): the number of co-resident workgroups a cluster launch may use; 0 (default) = the device's CU
 * count.  Any other value is clamped to [0, CU count] where it is used, so it can only LOWER the grid of a launch -- the
 * tests exercise tile groups at B = 80 - 272 with it.  A plain process-wide int, not thread-safe: set it while no
 * recurrence call is running on any handle. */
int asr_debug_set_cluster_cu_budget(int n);

/* Debug / measurement: are 16-byte per-lane stores seen whole by 16-byte loads of another CU?  Workgroup 0 stores
 * {i, i, i, i}, i = 1 .. iters, into buf[16 lane .. ] (64 lanes; plain stores, or write-through when write_through != 0);
 * workgroup `peer` (8: the same XCD as workgroup 0, 1: another one) polls them with L1-bypassing loads.
 * out[3 lane .. +2] = {loads, loads whose four dwords differed, distinct values seen}.  Evidence for DESIGN section 8
 * item 1-i (the product path exchanges 8-byte granules and per-word tags only). */
int asr_debug_tear_probe(asr_handle* h, unsigned* buf, unsigned iters, int peer, int write_through,
                         unsigned long long* out, asr_stream s);

/* Debug: records, per workgroup of a probe grid launched on `s`, {XCC id, HW_ID register} into out[2*nblocks]
 * (device memory); every workgroup stays resident for spin_cycles so that the grid spreads over the CUs. */
int asr_debug_placement(asr_handle* h, unsigned* out, int nblocks, int spin_cycles, asr_stream s);
/* test aid: fills every CU's LDS with NaN bit patterns (a kernel that reads LDS words nobody wrote then fails every time
 * instead of once in a few cold starts); tests/conftest.py runs it in front of every test under ASR_POISON_LDS=1 */
int asr_debug_poison_lds(asr_handle* h, asr_stream s);

/* ---- GRU recurrence ------------------------------------------------------- *
 * tf.contrib.rnn.GRUCell under tf.nn.(bidirectional_)dynamic_rnn(sequence_length) -- the reference's GRUEncoder /
 * BGRUEncoder (models/encoders/core/gru.py:58-76, :126-152).  fp32.  One layer, ndir directions, all steps:
 *     [r, u] = sigmoid(xg_t + h W_gh),  c = tanh(xc_t + (r * h) W_ch),  h' = u * h + (1 - u) * c
 * xg [T,B,ndir,2H] = x W_g[:D] + b_g and xc [T,B,ndir,H] = x W_c[:D] + b_c are the caller's hoisted GEMMs;
 * wgh [ndir][H][2H] / wch [ndir][H][H] the recurrent blocks of the two kernels (row-major), wghT / wchT their
 * transposes ([ndir][2H][H] / [ndir][H][H]).  tmax = max(seq_len) (host value: the step loop is issued by the host).
 * Saved for the backward pass, all [T,B,ndir,H] at the frame a row worked on: r, u, c, rh = r * h_prev.
 * hout [T,B,ndir*H] (zero past seq_len); hstate2: 2*ndir*B*H floats of work space, the final state [ndir,B,H] is
 * left in its first half.  r, u, c past a row's length are unspecified, rh there is left as the caller set it (zeros:
 * the candidate kernel's weight gradient contracts it over all T*B rows); a timed-out cluster hand-off sets the sticky
 * error word of asr_check_async_errors (bit 1 forward, bit 2 backward) as the LSTM clusters do.
 * asr_gru_bwd: dout [T,B,ndir*H] (+ d_h_final [ndir,B,H] or NULL) -> dgate [T,B,ndir,2H] (d r_pre | d u_pre) and
 * dcand [T,B,ndir,H] (d c_pre), zero where no row is active; the weight / input gradients are GEMMs over them
 * (dW_g = [x; h_prev]^T dgate, dW_c = [x; rh]^T dcand, dx = dgate W_gx^T + dcand W_cx^T).  work2: 2*ndir*B*H floats. */
int asr_gru_fwd(asr_handle* h, int T, int B, int H, int ndir, const float* xg, const float* xc,
                const float* wgh, const float* wch, const int32_t* seq_len, int tmax, float* r, float* u,
                float* c, float* rh, float* hout, float* hstate2, asr_stream s);
int asr_gru_bwd(asr_handle* h, int T, int B, int H, int ndir, const float* dout, const float* d_h_final,
                const float* hout, const float* r, const float* u, const float* c, const float* wghT,
                const float* wchT, const int32_t* seq_len, int tmax, float* dgate, float* dcand,
                float* work2, asr_stream s);

/* ---- CTC ------------------------------------------------------------------ *
 * tf.nn.ctc_loss(labels, logits, seq_len, preprocess_collapse_repeated=False,
 * ctc_merge_repeated=True, time_major=True) -- models/ctc/ctc.py:289-297,
 * models/attention/joint_ctc_attention.py:308-316.  blank = C-1.
 * logits[T,B,C] fp32; labels_flat: concatenated label ids (int32), label_offsets[B+1];
 * loss[B] fp32; grad[T,B,C] fp32 = d loss[b] / d logits * grad_scale (pass 1/B to get the
 * gradient of the batch mean of ctc.py:298); zero for t >= seq_len[b].
 * Infeasible utterances give loss 0 and grad 0 (ignore_longer_outputs_than_inputs=True);
 * their count is written to *num_infeasible (device int32, may be NULL).
 * workspace: asr_ctc_workspace_bytes(T,B,max label length). */
size_t asr_ctc_workspace_bytes(int T, int B, int max_label_len);
int asr_ctc_loss(asr_handle* h, const float* logits, int T, int B, int C,
                 const int32_t* labels_flat, const int32_t* label_offsets,
                 const int32_t* seq_len, int max_label_len, float grad_scale,
                 float* loss, float* grad, int32_t* num_infeasible,
                 void* workspace, size_t workspace_bytes, asr_stream s);
/* asr_ctc_loss with two additions (same kernels, same bits in loss / grad / *num_infeasible):
 *  lse_done != 0: asr_ctc_head_fwd has already left the row log-sum-exps, the emissions and the cleared counter in THIS
 *    workspace for THESE logits; the first of the three launches is skipped.
 *  grad_bf16 != NULL (needs grad): [T*B, Kp] bf16, Kp >= C a multiple of 64 -- every value written to grad is also stored
 *    there rounded as asr_cast_from_f32 rounds it, columns C .. Kp-1 zero in every row: the operand image of the products
 *    that consume dlogits, without a cast pass. */
int asr_ctc_loss_ex(asr_handle* h, const float* logits, int T, int B, int C,
                    const int32_t* labels_flat, const int32_t* label_offsets,
                    const int32_t* seq_len, int max_label_len, float grad_scale,
                    float* loss, float* grad, int32_t* num_infeasible,
                    void* workspace, size_t workspace_bytes, int lse_done, void* grad_bf16, int Kp, asr_stream s);
/* EXTENSION (not in the reference: its blstm_ctc_ls.yml sets label_smoothing_prob, none of its code reads the key): label
 * smoothing of a CTC head towards the uniform distribution over all C classes, blank included.  asr_ctc_loss_ex's
 * arguments plus smoothing = eps in (0, 1) (else ASR_ERR_INVALID_ARG) and kl [B]:
 *   loss[b] = the UNSMOOTHED CTC loss, the bits of asr_ctc_loss on the same inputs for every eps
 *   kl[b]   = sum_{t < min(seq_len[b], T)} KL(uniform || softmax(logits[t,b,:])) = sum_t (lse - mean_k x_k - ln C)
 *   grad    = grad_scale * (softmax - (1 - eps) * occupation - eps / C): the gradient of (1 - eps) loss[b] + eps kl[b],
 *             written by the gradient kernel in its one pass over the row (grad_bf16: the image of THESE values)
 * The caller forms (1 - eps) loss + eps kl.  Infeasible utterances and seq_len[b] == 0 give loss 0, kl 0, grad 0; frames
 * t >= seq_len[b] are never read (grad and image rows 0).  Logits must be finite (a -inf logit makes KL infinite).
 * grad may be NULL (kl is still produced).  Row terms are formed in fp64 and reduced per utterance in a fixed order: the
 * same bits on every call.  workspace: asr_ctc_ls_workspace_bytes -- the layout of asr_ctc_workspace_bytes is a prefix of
 * it, so asr_ctc_head_fwd on such a workspace followed by lse_done = 1 here is the smoothed head in three launches.
 * asr_ctc_ls_counts: {calls, calls with lse_done, calls without grad} since the last reset. */
size_t asr_ctc_ls_workspace_bytes(int T, int B, int max_label_len);
int asr_ctc_loss_ls(asr_handle* h, const float* logits, int T, int B, int C,
                    const int32_t* labels_flat, const int32_t* label_offsets,
                    const int32_t* seq_len, int max_label_len, float grad_scale, float smoothing,
                    float* loss, float* kl, float* grad, int32_t* num_infeasible,
                    void* workspace, size_t workspace_bytes, int lse_done, void* grad_bf16, int Kp, asr_stream s);
int asr_ctc_ls_counts(asr_handle* h, unsigned long long* out3);
int asr_reset_ctc_ls_counts(asr_handle* h);
/* The output layer of a CTC model and the first CTC launch in ONE kernel (bf16 operands, E % 64 == 0, C <= 64):
 *   x_op   = dropout(hout)               [T*B, E] bf16, asr_dropout_apply(keep_prob, seed, offset) bit for bit, every row
 *                                        (keep_prob == 0: no dropout, x_op is not written and may be NULL -- hout IS the operand)
 *   logits = x_op W + bias               [T*B, C] fp32, every row, the bits of asr_gemm on the operand image of W
 *   and in the workspace (asr_ctc_workspace_bytes) the row log-sum-exps, the emissions along the label sequences and the
 *   cleared *num_infeasible, as asr_ctc_loss's first launch leaves them: follow with asr_ctc_loss_ex(lse_done = 1).
 * Wt: the class-major image of asr_ctc_head_prep.  asr_ctc_head_ok(rows, E, C): 1 where the call applies -- the shapes
 * whose logits product asr_gemm runs in one pass over K; others return ASR_ERR_UNSUPPORTED (run the separate launches).
 * asr_ctc_head_prep: W [E, C] fp32 -> Wt [64, E] bf16 (classes >= C zero; NULL for C > 64) and Wp [E, Kp] bf16 (Kp = C
 * rounded up to 64, columns >= C zero: the transposed operand of dlogits W^T on the image of asr_ctc_loss_ex).
 * asr_ctc_head_counts: {asr_ctc_head_fwd launches, asr_ctc_loss_ex calls, asr_ctc_loss calls} since the last reset. */
int asr_ctc_head_ok(int rows, int E, int C);
int asr_ctc_head_prep(asr_handle* h, const float* W, int E, int C, void* Wt, void* Wp, asr_stream s);
int asr_ctc_head_fwd(asr_handle* h, const void* hout, int T, int B, int E, float keep_prob, uint64_t seed,
                     uint64_t offset, const void* Wt, const float* bias, int C, const int32_t* labels_flat,
                     const int32_t* label_offsets, const int32_t* seq_len, int max_label_len, void* x_op, float* logits,
                     int32_t* num_infeasible, void* workspace, size_t workspace_bytes, asr_stream s);
/* d(encoder output) [M, E] fp32 = dl [M, Kp] (asr_ctc_loss_ex's bf16 image) x Wp [E, Kp]^T (asr_ctc_head_prep), times the
 * dropout mask asr_dropout_mask(M*E, keep_prob, seed, offset) of the top layer (keep_prob == 0: none), E % 4 == 0.  rows /
 * num_rows: asr_gemm_rows' contract (NULL: every row) -- listed rows get the full product's bits, the others are left
 * untouched or written; the same kernels, counted as ASR_GEMMP_HEAD_BWD_* of asr_gemm_path_counts. */
int asr_ctc_head_bwd(asr_handle* h, int M, int E, int Kp, const void* dl, const void* Wp, float* denc, float keep_prob,
                     uint64_t seed, uint64_t offset, const int32_t* rows, int num_rows, asr_stream s);
int asr_ctc_head_counts(asr_handle* h, unsigned long long* out3);
int asr_reset_ctc_head_counts(asr_handle* h);

/* tf.nn.ctc_greedy_decoder(merge_repeated=True) -- models/ctc/ctc.py:341-342 and
 * models/ctc/decoders/greedy_decoder.py:19-50.  logits[T,B,C]; out_labels[B,T] int32
 * padded with -1; out_len[B]. */
int asr_ctc_greedy_decode(asr_handle* h, const float* logits, int T, int B, int C,
                          const int32_t* seq_len, int blank,
                          int32_t* out_labels, int32_t* out_len, asr_stream s);

/* Prefix beam search -- models/ctc/decoders/beam_search_decoder.py:53-152
 * (also stands in for tf.nn.ctc_beam_search_decoder, models/ctc/ctc.py:344-346).
 * logits[T,B,C] fp32 (log-softmax is taken inside); out_labels[B,T] padded -1;
 * out_len[B]; out_score[B] = -log p of the best prefix (float64).
 * beam_width <= 128.  Scores are fp64, ties are broken like the reference's stable sort. */
size_t asr_ctc_beam_workspace_bytes(int T, int B, int C, int beam_width);
int asr_ctc_beam_decode(asr_handle* h, const float* logits, int T, int B, int C,
                        const int32_t* seq_len, int blank, int beam_width,
                        int32_t* out_labels, int32_t* out_len, double* out_score,
                        void* workspace, size_t workspace_bytes, asr_stream s);

/* row softmax: CTC.posteriors (models/ctc/ctc.py:354-380) */
int asr_softmax_rows(asr_handle* h, const float* in, float* out, int rows, int C, asr_stream s);

/* ---- attention decoder (models/attention/...) -------------------------------- *
 * Encoder outputs and keys are TIME-MAJOR: enc[T,B,E], keys[T,B,A]; per-utterance vectors [B,*].
 *
 * One LSTMBlockCell step of the decoder RNN (attention_seq2seq.py:352-371): pre[B,4U] fp32 =
 * [x,h]W + b with TF gate-major columns (i, ci, f, o); peep [3][U] or NULL.  live[B] (1/0):
 * rows already finished keep their state (dynamic_decode impute_finished,
 * decoders/dynamic_decoder.py:171-193).  Outputs: gates[B,4U] post-activation, c_raw/h_raw = new
 * cell/output before the finished-carry, c_out/h_out = carried state. */
int asr_lstm_cell_fwd(asr_handle* h, const float* pre, const float* c_prev, const float* h_prev,
                      const float* peep, const float* live, int B, int U, float forget_bias,
                      float cell_clip, float* gates, float* c_raw, float* c_out, float* h_out,
                      float* h_raw, asr_stream s);
/* The same step with its results also written where the NEXT kernels of the decoder step read them, so that no copy
 * launch sits between them (attention_decoder.py:142-229: the cell output feeds the attention layer and the
 * attentional vector, the carried h the next step's cell input):
 *   cell_out [B,U] (may be NULL) = h_raw * out_mask (out_mask [B,U] fp32 or NULL: DropoutWrapper(output_keep_prob));
 *   cell_out2 (may be NULL): the same values at cell_out2[b*ld_c2 + j]  (a column block of a wider row-major array);
 *   h_out2   (may be NULL): h_out at h_out2[b*ld_h2 + j]. */
int asr_lstm_cell_fwd_ex(asr_handle* h, const float* pre, const float* c_prev, const float* h_prev,
                         const float* peep, const float* live, int B, int U, float forget_bias,
                         float cell_clip, float* gates, float* c_raw, float* c_out, float* h_out,
                         float* h_raw, const float* out_mask, float* cell_out, float* h_out2, int ld_h2,
                         float* cell_out2, int ld_c2, asr_stream s);
/* asr_gemm_act(x [B,K] (row stride ldx) x W [K,4U] + b) -> asr_lstm_cell_fwd_ex as ONE launch (a decoder step's first two
 * kernels): the product runs on the gate-INTERLEAVED weight image W_il [(K + 1), 4U] (column 4 u + g = gate g of unit u, the
 * last row the bias; written by asr_lstm_cell_gemm_prep once per weight update), so a workgroup holds all four gates of its
 * units and applies the cell in its epilogue; the pre-activations are never written.  Same arithmetic in the same order
 * as the two separate calls: bit-identical outputs.  asr_lstm_cell_gemm_ok: B <= 32, K % 64 == 0, U % 8 == 0, ldx % 4 == 0. */
int asr_lstm_cell_gemm_ok(int B, int K, int U, int ldx);
int asr_lstm_cell_gemm_prep(asr_handle* h, const float* W, const float* bias, int K, int U, float* W_il, asr_stream s);
int asr_lstm_cell_gemm_fwd(asr_handle* h, const float* x, int ldx, int K, const float* W_il, int has_bias,
                           const float* c_prev, const float* h_prev, const float* peep, const float* live,
                           int B, int U, float forget_bias, float cell_clip, float* gates, float* c_raw,
                           float* c_out, float* h_out, float* h_raw, const float* out_mask, float* cell_out,
                           float* h_out2, int ld_h2, float* cell_out2, int ld_c2, asr_stream s);
/* The same pair with bf16 WEIGHTS (fp32 activations, exact fp32 products of an fp32 value and a bf16-valued one): `img`
 * (asr_lstm_cell_gemm_h_bytes) holds, written by asr_lstm_cell_gemm_prep_h, the gate-interleaved kernel in the order the
 * multiplies consume it (four 16-byte loads per lane and 64-row unit), the interleaved fp32 bias, and a plain bf16 copy of
 * W whose rows asr_lstm_cell_gemm_bwd_h (dx [B,K] = dpre [B,4U] W^T, the backward product of a decoder step) streams. */
size_t asr_lstm_cell_gemm_h_bytes(int K, int U);
int asr_lstm_cell_gemm_prep_h(asr_handle* h, const float* W, const float* bias, int K, int U, void* img, asr_stream s);
int asr_lstm_cell_gemm_fwd_h(asr_handle* h, const float* x, int ldx, int K, const void* img,
                             const float* c_prev, const float* h_prev, const float* peep, const float* live,
                             int B, int U, float forget_bias, float cell_clip, float* gates, float* c_raw,
                             float* c_out, float* h_out, float* h_raw, const float* out_mask, float* cell_out,
                             float* h_out2, int ld_h2, float* cell_out2, int ld_c2, asr_stream s);
int asr_lstm_cell_gemm_bwd_h(asr_handle* h, const float* dpre, int B, int K, int U, const void* img, float* dx, int lddx,
                             asr_stream s);
/* dh_use: gradient on the cell output of live rows; dc_next/dh_next: gradient on the carried state.
 * dpre[B,4U]; dc_prev; dh_prev_carry (pass-through part, add (dpre W^T)[h] for live rows);
 * dpeep_rows[B][3][U] per-row peephole gradient terms (sum over rows/steps on the caller side). */
int asr_lstm_cell_bwd(asr_handle* h, const float* dh_use, const float* dc_next, const float* dh_next,
                      const float* gates, const float* c_raw, const float* c_prev, const float* peep,
                      const float* live, int B, int U, float* dpre, float* dc_prev,
                      float* dh_prev_carry, float* dpeep_rows, asr_stream s);
/* The same with the forward's cell clip: a state the forward clamped (tf.clip_by_value inside LSTMCell,
 * models/recurrent/layers/lstm.py:152-157) passes no gradient to the gates or to c_prev; c_raw holds the clamped value,
 * |c_raw| >= cell_clip marks it.  cell_clip <= 0: identical to asr_lstm_cell_bwd.  (asr_att_decoder_bwd does NOT do
 * this: the attention decoder's cell is tf.contrib.rnn.LSTMBlockCell, attention_seq2seq.py:354-363, whose gradient op has
 * no clip attribute -- the clamp is transparent to the gradient there, as in the encoders' fused cells.) */
int asr_lstm_cell_bwd_ex(asr_handle* h, const float* dh_use, const float* dc_next, const float* dh_next,
                         const float* gates, const float* c_raw, const float* c_prev, const float* peep,
                         const float* live, int B, int U, float cell_clip, float* dpre, float* dc_prev,
                         float* dh_prev_carry, float* dpeep_rows, asr_stream s);
/* Attention energies (attention_layer.py:115-347).  mode 0 (bahdanau_content / location / hybrid):
 * energy[b,t] = sum_a v[a] * tanh(keys[t,b,a] + qz[b,a])   (keys NULL for 'location');
 * mode 1 (dot_product / luong_dot / luong_general): energy[b,t] = sum_a keys[t,b,a] * qz[b,a].
 * qz = W_query s (+ W_filter bias where the type has location features). */
int asr_att_energy_fwd(asr_handle* h, const float* keys, const float* qz, const float* v, int T,
                       int B, int A, int mode, float* energy, asr_stream s);
/* dkeys[T,B,A] += (may be NULL); dqz[B,A] = ; dv_rows[B,A] = per-utterance v gradient (may be NULL) */
int asr_att_energy_bwd(asr_handle* h, const float* denergy, const float* keys, const float* qz,
                       const float* v, int T, int B, int A, int mode, float* dkeys, float* dqz,
                       float* dv_rows, asr_stream s);
/* energy*mask + (1-mask)*float32.min, * sharpening, softmax over t, context = sum_t alpha enc
 * (attention_layer.py:75-111).  alpha[B,T], ctx[B,E].  enc[T,B,E] in `enc_dtype`: a bf16-operand model passes
 * the bf16 copy of the encoder output it already keeps, halving the two per-step streams over enc.
 * sigmoid_norm NULL: softmax.  Non-NULL ([B], written): `sigmoid_smoothing` (attention_layer.py:92-96),
 * alpha = sigmoid(e) / sum_t sigmoid(e), and sigmoid_norm[b] = that sum -- hand it back to the backward. */
int asr_att_softmax_ctx_fwd(asr_handle* h, const float* energy, const int32_t* seq_len,
                            float sharpening, const void* enc, int enc_dtype, int T, int B, int E,
                            float* alpha, float* ctx, float* sigmoid_norm, asr_stream s);
/* the same with the context also written to up to two column blocks of wider row-major arrays
 * (ctx2[b*ld2 + e], ctx3[b*ld3 + e]; NULL = not wanted): the next step's cell input and the attentional vector's */
int asr_att_softmax_ctx_fwd_ex(asr_handle* h, const float* energy, const int32_t* seq_len,
                               float sharpening, const void* enc, int enc_dtype, int T, int B, int E,
                               float* alpha, float* ctx, float* sigmoid_norm, float* ctx2, int ld2,
                               float* ctx3, int ld3, asr_stream s);
/* denergy[B,T] = ; denc[T,B,E] += alpha * dctx.  denc may be NULL: a decoder loop then keeps alpha and
 * dctx of every step and forms d_enc = sum_steps alpha (x) dctx with ONE GEMM per utterance at the end
 * instead of a read-modify-write of the whole [T,B,E] tensor per step. */
int asr_att_softmax_ctx_bwd(asr_handle* h, const float* dctx, const float* alpha,
                            const int32_t* seq_len, float sharpening, const void* enc, int enc_dtype,
                            int T, int B, int E, float* denergy, float* denc,
                            const float* sigmoid_norm, const float* dalpha_extra, asr_stream s);
/* dalpha_extra [B,T] (may be NULL): a further gradient w.r.t. alpha, added before the softmax gradient -- with
 * carried location features the NEXT decoder step's conv1d hands one back (asr_att_loc_energy_bwd).
 *
 * Location / hybrid attention with the previous step's weights carried (attention_layer.py:191-265; the recurrence
 * the reference wrote down -- its graph feeds zeros at every step, SURVEY Appendix A Q1, which stays the default of
 * the Python model: prev_alpha='zeros' | 'carry'):
 *   f = tf.nn.conv1d(alpha_prev[B,T,1], filter[taps,1,10], stride 1, 'SAME')    taps = 201 (location) / 200 (hybrid),
 *       zero padding (taps-1)/2 frames before, the rest after; cross-correlation
 *   energy[b,t] = sum_a v[a] tanh( keys[t,b,a] + qz[b,a] + (f W_filter)[b,t,a] )     keys NULL for 'location';
 *       qz = W_query s + b_filter as for asr_att_energy_fwd.
 * filt [taps,10] (the [taps,1,10] variable), wfil [10,A] (W_filter/weights). */
int asr_att_loc_energy_fwd(asr_handle* h, const float* alpha_prev, const float* filt, const float* wfil,
                           const float* keys, const float* qz, const float* v, int T, int B, int A, int taps,
                           float* energy, asr_stream s);
/* Gradients of the above for one decoder step.  dkeys[T,B,A] += (may be NULL); dqz[B,A], dv_rows[B,A] written;
 * dwfil_rows[B,10,A] and dfilt_rows[B,taps,10]: per-utterance gradients of W_filter/weights and filter, overwritten
 * when accumulate == 0 and added to otherwise (a decoder loop accumulates over its steps and sums over B once);
 * dalpha_prev[B,T] written: gradient w.r.t. the previous step's weights (-> dalpha_extra of that step).
 * Partials go through the handle scratch in a fixed order: run-to-run deterministic. */
int asr_att_loc_energy_bwd(asr_handle* h, const float* denergy, const float* alpha_prev, const float* filt,
                           const float* wfil, const float* keys, const float* qz, const float* v, int T, int B,
                           int A, int taps, float* dkeys, float* dqz, float* dv_rows, float* dwfil_rows,
                           float* dfilt_rows, float* dalpha_prev, int accumulate, asr_stream s);
/* ---- the decoder loop, native ----------------------------------------------------------------------------- *
 * dynamic_decode over a TrainingHelper (decoders/dynamic_decoder.py:68-218, attention_decoder.py:142-229): all To steps
 * of the attention decoder issued from ONE call -- the per-step sequence cell-input GEMM -> asr_lstm_cell_fwd_ex ->
 * query GEMM -> asr_att_(loc_)energy_fwd -> asr_att_softmax_ctx_fwd_ex, i.e. exactly the entry points above in the
 * order a host loop would call them (a Python host spends ~15 us per call, ~9 calls per step, 400 steps: the loop was
 * host-bound), and the reverse sequence for the gradients (where adjacent steps of that sequence have a fused kernel --
 * the dctx add inside the d-alpha kernel, the softmax backward inside the energy backward, mask and carried-dh add
 * inside the cell backward -- the loop uses it; the arithmetic is that of the separate entry points).  Every array is the caller's; per-step arrays are [To, ...]
 * row blocks.  Layouts: dec_in [To,B,Em+E2+U] = embedded input | previous context | previous h (the embedding columns
 * and row 0 filled by the caller, the rest by the loop), av_in [To,B,U+E2] = cell output (after its dropout mask) |
 * context; c_all / h_all [To+1,B,U]: carried state BEFORE step k at row k (row 0 = initial state from the bridge). */
typedef struct asr_att_decoder {
  int To, B, T, U, Em, E2, A;       /* A: width of keys / qz */
  int att_mode;                     /* 0 additive (v tanh(keys + qz)), 1 dot */
  int has_query_fc;                 /* qz = cell_out W_q (+ b_q); 0: qz = cell_out (then A == U) */
  int carry_alpha, taps;            /* location features of the previous step's weights (asr_att_loc_energy_*) */
  int enc_dtype;
  float forget_bias, cell_clip, sharpening;
  const float *W_cell, *b_cell, *peep;          /* [Em+E2+U,4U], [4U], [3,U] or NULL */
  const float *W_q, *b_q, *v;                   /* [U,A] (row stride ld_wq) or NULL, [A] or NULL, [A] or NULL */
  int ld_wq;
  const float *keys;                            /* [T,B,A] or NULL */
  const void *enc;                              /* [T,B,E2] in enc_dtype */
  const int32_t *seq_len;                       /* [B] */
  const float *filt, *wfil, *alpha_zero;        /* carry_alpha: [taps,1,10], [10,A], zeros [B,T] */
  const float *live, *dmask;                    /* [To,B]; [To,B,U] or NULL */
  float *dec_in, *av_in, *alpha_all, *snorm_all;/* snorm_all [To,B] or NULL (sigmoid smoothing) */
  float *gates_all, *craw_all, *c_all, *h_all, *qz_all;   /* [To,B,4U], [To,B,U], [To+1,B,U] x2, [To,B,A] */
  float *work;                                  /* forward: B*(4U + U + T + E2) floats; backward: see asr_att_decoder_bwd */
  /* backward only */
  const float *dav_cell, *dav_ctx;              /* [To,B,U] (used as work space: overwritten), [To,B,E2] */
  float *dctx_all, *dpre_all, *dqz_all, *dv_all, *dpeep_all, *d_in_all;   /* [To,B,E2|4U|A|A or NULL|3U or NULL|Em+E2+U] */
  float *dkeys, *dwfil_rows, *dfilt_rows;       /* [T,B,A] += or NULL; carry_alpha: [B,10,A], [B,taps,10] */
  float *dc0, *dh0;                             /* [B,U] out: gradient w.r.t. the initial state */
  /* forward / inference, optional (abi 3): (Em+E2+U+1) x 4U floats of work space.  When given (and asr_lstm_cell_gemm_ok)
   * the loop writes the gate-interleaved image of W_cell | b_cell there once (asr_lstm_cell_gemm_prep) and every step runs
   * the cell-input product and the LSTM cell as ONE launch (asr_lstm_cell_gemm_fwd) -- same values, bit for bit. */
  float *W_cell_il;
  /* forward / inference / backward, optional: asr_lstm_cell_gemm_h_bytes(Em+E2+U, U) bytes of work space.  When given (and
   * asr_lstm_cell_gemm_ok, U % 16 == 0) the loops write the bf16 images of W_cell there (asr_lstm_cell_gemm_prep_h) and the
   * cell-input product (+ cell) of every forward step and the dpre W_cell^T product of every backward step stream bf16
   * weights: the rounding point of a bf16-operand model's decoder kernel (oracle: operand_round on lstm_cell/kernel).
   * Takes precedence over W_cell_il. */
  void *W_cell_h;
} asr_att_decoder;
int asr_att_decoder_fwd(asr_handle* h, const asr_att_decoder* a, asr_stream s);
/* ---- greedy inference, native ------------------------------------------------------------------------------ *
 * dynamic_decode over a GreedyEmbeddingHelper with impute_finished (attention_seq2seq.py:462-509,
 * decoders/dynamic_decoder.py:148-197): the reference's in-graph while_loop, here ONE call that issues, per step, the
 * forward step of asr_att_decoder_fwd, the attentional-vector FC + tanh, the output layer, and a selection kernel
 * (argmax -> emitted id, per-row finished flag, embedding of the id into the next step's input row, imputed context).
 * `a` as for asr_att_decoder_fwd with To = max_decode_length, dmask NULL, a->live == f->live ([To+1,B], row 0 set by the
 * caller: 1 for rows that decode), gates_all / craw_all / qz_all ONE step long (reused), snorm_all [To,B] or NULL;
 * dec_in row 0 = embedding(start token) | zero context | initial h.  Outputs: ids_all [To,B] (0 once a row has
 * finished), logits_all [To,B,C2] and av_all [To,B,U] (NOT imputed: multiply by live[k] for the reference's emitted
 * fields), a->alpha_all [To,B,T], live [To+1,B], live_count [To+1] (live rows at the START of step k; entry 0 is the
 * caller's).  The number of decoded steps is the first k with live_count[k] == 0 (or To).
 * Early exit: with host_live_count (pinned host int32 [To+1]) and check_every > 0 the call stops issuing steps once a
 * check point's asynchronous copy shows no live row; it waits only for the copy of two check points ago (the issue loop
 * stays 2-3 intervals ahead of the device, the pipeline is never drained); *steps_issued tells how many steps were
 * enqueued (>= the number decoded). */
typedef struct asr_att_infer {
  const float *W_av, *W_out, *b_out;            /* [U+E2,U], [U,C2], [C2] or NULL */
  const float *embedding;                       /* [vocabulary, Em] */
  int C2, eos;
  float *live;                                  /* [To+1,B] */
  float *av_all, *logits_all;                   /* [To,B,U], [To,B,C2] */
  int32_t *ids_all, *live_count;                /* [To,B], [To+1] */
  int32_t *host_live_count;                     /* pinned host [To+1] or NULL */
  int check_every;
} asr_att_infer;
int asr_att_decoder_infer(asr_handle* h, const asr_att_decoder* a, const asr_att_infer* f, int* steps_issued,
                          asr_stream s);
/* ---- scheduled sampling in the training loop, native (later within ABI 5, additive) --------------------------- *
 * EXTENSION: the reference names scheduled_sampling_prob / scheduled_sampling_ramp_max_step in
 * examples/timit/config/attention/att_baseline.yml and none of its code reads them; the meaning given here is that of
 * tf.contrib.seq2seq.ScheduledEmbeddingTrainingHelper with the argmax in place of a sample.  asr_att_decoder_fwd in which
 * the token fed at step k may be the model's own prediction:
 *     fed[0, b] = teacher_ids[0, b]
 *     fed[k, b] = argmax_c logits[k-1, b, c]   if draw[k, b] != 0 and a->live[k, b] != 0      (k >= 1)
 *               = teacher_ids[k, b]            otherwise (finished and padding rows keep the teacher's token)
 * The argmax is over the raw logits of the previous step (no imputation, no temperature), the first maximum wins (as
 * asr_argmax_rows).  Per step the call issues the forward step of asr_att_decoder_fwd (saved activations at row k, a->dmask
 * honoured), the head asr_att_decoder_infer issues behind it (attentional-vector FC, tanh, output layer) and one selection
 * kernel that writes ids_fed[k+1] and embedding[fed] * emb_mask[k+1] into the Em embedding columns of dec_in[k+1]; row 0 of
 * dec_in and of ids_fed is the caller's, as is the drawing of `draw`.  The fed ids are constants of the backward pass
 * (asr_att_decoder_bwd as it is; the embedding gradient scatters to ids_fed).  av_all / logits_all are not imputed. */
typedef struct asr_att_decoder_ss {
  const float *W_av, *W_out, *b_out;            /* [U+E2,U], [U,C2], [C2] or NULL */
  const float *embedding;                       /* [C2, Em] */
  int C2;
  const int32_t *teacher_ids;                   /* [To,B], each in [0, C2) */
  const float *draw;                            /* [To,B]: != 0 feeds the prediction (row 0 is not read) */
  const float *emb_mask;                        /* [To,B,Em] or NULL (row 0 is not read) */
  float *av_all, *logits_all;                   /* [To,B,U], [To,B,C2] */
  int32_t *ids_fed;                             /* [To,B]; rows 1 .. To-1 written */
} asr_att_decoder_ss;
int asr_att_decoder_fwd_ss(asr_handle* h, const asr_att_decoder* a, const asr_att_decoder_ss* f, asr_stream s);
/* ---- beam search over the attention decoder, native (later within ABI 5) ------------------------------------ *
 * The reference's BeamSearchDecoder (models/attention/decoders/beam_search/beam_search_decoder.py; dead code there: it
 * imports an RNNDecoder that does not exist, the functions below are complete).  Per utterance W slots; the device batch
 * is R = B*W rows, row b*W + w.
 *
 * asr_att_beam_select: beam_search_step (beam_search_decoder.py:234-332) with mask_probs (util.py:37-68) and
 * normalize_score (util.py:71-95), one workgroup per utterance, fp32.  logits [B*W,C2]; state in: log_probs [B*W],
 * finished / lengths [B*W] int32.  p = log_softmax(row); a finished row has p[eos] = 0 and nothing else;
 * total = log_probs + p; candidate length = lengths + (c != eos && !finished); score = total / ((5 + len)^lpw / 6^lpw)
 * -- QUIRK kept: lpw == 1 leaves score = total (util.py:90-91).  first_step != 0: only slot 0's candidates count
 * (:287-290).  The W best by (score descending, flat index w*C2 + c ascending: tf.nn.top_k's order) give
 * word = flat % C2, parent = flat / C2 [B,W], score [B,W], and the next state: log_probs = total,
 * finished = finished[parent] | word == eos, lengths = lengths[parent] + (word != eos && !finished_next).  The state may
 * be updated in place (out == in).  unfinished (or NULL): += the number of unfinished slots of the next state.
 * 1 <= W <= 32, W <= C2, 0 <= eos < C2.
 * asr_att_beam_reorder: what step k+1 reads becomes the parent's (tf.gather by beam_parent_ids, :206-212, and
 * helper.next_inputs on the chosen ids, :224-228): row r = b*W + w of c_dst / h_dst [R,U], of columns Em.. of din_dst
 * [R,Em+E2+U] (previous context | previous h) and, with T > 0, of alpha_dst [R,T] is row b*W + parent[r] of the *_src
 * array; columns 0..Em of din_dst are embedding row word[r] (vocab rows).  Out of place: no dst may alias its src.
 * asr_att_beam_backtrace: gather_tree_py (util.py:14-26) over the first `steps` rows of word / parent [To,B,W], one thread
 * per (utterance, final slot): ids [B,W,To] = the path that ends in that slot, cut behind its first eos (zeros there),
 * hyp_len [B,W] = ids kept (the eos included), final_score [B,W] = score[steps-1]. */
int asr_att_beam_select(asr_handle* h, const float* logits, int B, int W, int C2, int eos, float length_penalty_weight,
                        int first_step, const float* log_probs_in, const int32_t* finished_in, const int32_t* lengths_in,
                        int32_t* word, int32_t* parent, float* score, float* log_probs_out, int32_t* finished_out,
                        int32_t* lengths_out, int32_t* unfinished, asr_stream s);
int asr_att_beam_reorder(asr_handle* h, const int32_t* parent, const int32_t* word, int B, int W, int U, int Em, int E2,
                         int T, int vocab, const float* c_src, const float* h_src, const float* din_src,
                         const float* alpha_src, const float* embedding, float* c_dst, float* h_dst, float* din_dst,
                         float* alpha_dst, asr_stream s);
int asr_att_beam_backtrace(asr_handle* h, const int32_t* word, const int32_t* parent, const float* score, int steps, int To,
                           int B, int W, int eos, int32_t* ids, int32_t* hyp_len, float* final_score, asr_stream s);
/* asr_att_decoder_beam: the whole search from ONE call (BeamSearchDecoder.step under dynamic_decode, :173-231; finalize,
 * :125-150).  Per step it issues the forward step of asr_att_decoder_fwd and the output head exactly as
 * asr_att_decoder_infer does, on all R rows (no imputation: a->live is [R] ones), then asr_att_beam_select and
 * asr_att_beam_reorder; after the last step asr_att_beam_backtrace.  `a`: B = R, To = max_decode_length, encoder
 * arrays tiled to R rows; the loop carries ONE step of state, so the step arrays are two row blocks -- dec_in [2,R,Din],
 * c_all / h_all [2,R,U]: block 0 is what a step reads (the caller fills it: embedding(start) | zero context | h0; c0; h0,
 * each utterance's row repeated W times), block 1 receives the step's raw outputs, which the reorder gathers back into
 * block 0 -- and av_in / alpha_all / snorm_all / gates_all / craw_all / qz_all are one step long.  a->alpha_zero is not
 * read: the carried weights are m->alpha_prev ([R,T], zeros on entry).  `f`: W_av, W_out, b_out, embedding, C2, eos,
 * host_live_count, check_every (its array fields are not used).  Early exit as asr_att_decoder_infer, on m->unfinished
 * ([To+1]; entry k+1 = unfinished slots after step k): surplus steps change nothing -- an utterance whose slots have
 * all finished has exactly W finite candidates, in their standing order.  *steps_issued = the steps the back-trace
 * covers. */
typedef struct asr_att_beam {
  int W;
  float length_penalty_weight;
  int32_t *word, *parent;                       /* [To,B/W utterances,W] per-step outputs */
  float *score;                                 /* [To,B/W,W] */
  float *log_probs;                             /* state [R]: zeros on entry */
  int32_t *finished, *lengths;                  /* state [R]: zeros on entry */
  float *alpha_prev;                            /* [R,T] (carry_alpha) or NULL */
  float *av, *logits;                           /* scratch [R,U], [R,C2] */
  int32_t *unfinished;                          /* [To+1] */
  int32_t *ids, *hyp_len;                       /* [B/W,W,To], [B/W,W] */
  float *final_score;                           /* [B/W,W] */
} asr_att_beam;
int asr_att_decoder_beam(asr_handle* h, const asr_att_decoder* a, const asr_att_infer* f, const asr_att_beam* m,
                         int* steps_issued, asr_stream s);
/* Launches of the three beam kernels on this handle since the last reset, {select, reorder, backtrace} (host integers,
 * like asr_att_path_counts; a list of their own so that the ASR_ATT_* enum keeps its length). */
int asr_att_beam_counts(asr_handle* h, unsigned long long* out3);
int asr_reset_att_beam_counts(asr_handle* h);
/* ---- joint CTC / attention beam search, native (later within ABI 5, additive) ------------------------------- *
 * EXTENSION (the reference has no such decoder): one-pass joint decoding (Watanabe et al. 2017, Hori et al. 2017), every
 * partial hypothesis scored by (1 - ctc_weight) * log p_att + ctc_weight * log p_ctc(prefix).  Float64 statement:
 * models/attention/decoders/beam_search/ctc_prefix_score.py.  Attention classes C2 = n_labels + 2 (<SOS> = n_labels,
 * <EOS> = n_labels + 1), CTC classes Cc > n_labels with blank >= n_labels (the models: Cc = n_labels + 1, blank = n_labels);
 * label c of one is label c of the other.  y [T,By,Cc] fp32 log-posteriors, utterance b < B in batch row b (By >= B: the
 * posteriors are NOT tiled to the B*W device rows, row r reads b = r / W); seq_len [B].  Prefix state r [B*W,2,T] fp32:
 * r[row,0,t] / r[row,1,t] = log-probability of the frame paths over 0..t that collapse to the row's hypothesis and end in a
 * non-blank / a blank; entries t >= seq_len[b] are neither read nor written.  last [B*W] int32: the hypothesis's last
 * label, -1 when it is empty.  1 <= W <= 32.
 *
 * asr_log_softmax_rows: y = x - logsumexp(x) per row of x [rows,cols] (one wave per row; log(asr_softmax_rows) would lose
 * the small posteriors).  y may be x.
 * asr_ctc_prefix_init: the empty hypothesis in every row -- r_n = -inf, r_b[t] = sum of y[tau,b,blank] over tau <= t,
 * summed sequentially in ascending tau; last = -1, ctc_score = 0 (either may be NULL).
 * asr_ctc_prefix_score: psi [B*W,K] for the candidates cand [B*W,K] (attention class ids, K <= 64): for a label the
 * log-probability that the utterance's collapsed CTC output STARTS WITH hypothesis.label, for <EOS> log p_ctc(hypothesis),
 * for <SOS> or an id outside 0 .. n_labels + 1 -inf; a row with finished != 0 (finished may be NULL) has -inf but for
 * <EOS>.  An infeasible prefix is exactly -inf, never NaN.  One wave per row, a lane per candidate; psi of a label is
 * logsumexp over t of phi[t] + y[t,b,c] (phi from r, shared by the row), summed 64 frames at a time in ascending t.
 * asr_ctc_prefix_advance: r_dst row b*W + w = the state of (hypothesis of row b*W + parent[b,w]) . word[b,w]: the
 * recursion's r_n' / r_b' for a label (T dependent steps of two logaddexp, one wave per row), the parent's arrays bit for
 * bit for <EOS> (which is also every finished parent's word).  last_src is the PARENTS' array.  Out of place.
 * asr_att_beam_select_joint: asr_att_beam_select with fused scores.  Per unfinished slot the candidates are its W best
 * classes other than <EOS> by attention logit (ties by lower index) and <EOS> -- with attention-only scores that pruning
 * is lossless, here it is the preselection (the "CTC pre-beam"), fixed at W; a finished slot has its <EOS> alone, p = 0;
 * first_step: slot 0 only.  total = log_probs + log_softmax(logits)[c]; ctc = psi, or ctc_score_in of a finished slot;
 * a candidate with ctc = -inf is dropped; score = ((1 - ctc_weight) * total + ctc_weight * ctc) / penalty(length) with the
 * length rule and the lpw == 1 quirk of asr_att_beam_select; the W best by (score descending, flat index ascending) give
 * word / parent / score [B,W] and the next state log_probs = total (attention alone: the weight applies to totals),
 * ctc_score = ctc, finished, lengths, last = word (the parent's for <EOS>).  State out may be state in.  Three launches
 * (candidates, asr_ctc_prefix_score's kernel, rank -- the kernel pair of asr_att_beam_select_fused, att_beam.hip,
 * instantiated without the LM stream); cand / cand_total / psi: scratch [B*W,W+1].  W <= n_labels + 1,
 * 0 < ctc_weight <= 1 (0 is asr_att_beam_select's job).  seq_len >= 1 is the caller's contract (the statement raises; the
 * entries cannot look at device lengths).  At 0 frames nothing faults: the utterance has the empty hypothesis alone
 * (psi(<EOS>) = 0, labels -inf), and a place no candidate with a finite CTC score reaches -- only possible there -- comes out
 * as a finished <EOS> slot (parent = the place, the parent's ctc_score and last) with score and log_probs -inf. */
int asr_log_softmax_rows(asr_handle* h, const float* x, float* y, size_t rows, int cols, asr_stream s);
int asr_ctc_prefix_init(asr_handle* h, const float* y, const int32_t* seq_len, int B, int W, int T, int By, int Cc,
                        int blank, float* r, int32_t* last, float* ctc_score, asr_stream s);
int asr_ctc_prefix_score(asr_handle* h, const float* y, const int32_t* seq_len, int B, int W, int T, int By, int Cc,
                         int blank, int n_labels, const float* r, const int32_t* last, const int32_t* finished,
                         const int32_t* cand, int K, float* psi, asr_stream s);
int asr_ctc_prefix_advance(asr_handle* h, const float* y, const int32_t* seq_len, int B, int W, int T, int By, int Cc,
                           int blank, int n_labels, const float* r_src, const int32_t* last_src, const int32_t* parent,
                           const int32_t* word, float* r_dst, asr_stream s);
int asr_att_beam_select_joint(asr_handle* h, const float* logits, int B, int W, int n_labels, float length_penalty_weight,
                              float ctc_weight, int first_step, const float* y, const int32_t* seq_len, int T, int By, int Cc,
                              int blank, const float* r, const float* log_probs_in, const int32_t* finished_in,
                              const int32_t* lengths_in, const int32_t* last_in, const float* ctc_score_in, int32_t* cand,
                              float* cand_total, float* psi, int32_t* word, int32_t* parent, float* score,
                              float* log_probs_out, int32_t* finished_out, int32_t* lengths_out, int32_t* last_out,
                              float* ctc_score_out, int32_t* unfinished, asr_stream s);
/* asr_att_decoder_beam_joint: asr_att_decoder_beam with asr_att_beam_select_joint as its selection and
 * asr_ctc_prefix_advance behind it -- the same per-step issue, early exit and back-trace; a, f, m as there (f->C2 must be
 * n_labels + 2, f->eos n_labels + 1).  The call initialises the prefix state itself (asr_ctc_prefix_init) and flips
 * between the two blocks of r / last every step.  Surplus steps change nothing: a finished slot keeps total, ctc_score
 * and its state.  T is a->T. */
typedef struct asr_att_beam_ctc {
  const float *y;                               /* [T,By,Cc] log-posteriors */
  const int32_t *seq_len;                       /* [B/W utterances] */
  int By, Cc, blank, n_labels;
  float ctc_weight;                             /* in (0, 1] */
  float *r;                                     /* state [2,R,2,T] (two blocks, no initialisation needed) */
  int32_t *last;                                /* state [2,R] */
  float *ctc_score;                             /* [R]: out, the hypotheses' CTC scores after the last step */
  int32_t *cand;                                /* scratch [R,W+1] */
  float *cand_total, *psi;                      /* scratch [R,W+1] each */
} asr_att_beam_ctc;
int asr_att_decoder_beam_joint(asr_handle* h, const asr_att_decoder* a, const asr_att_infer* f, const asr_att_beam* m,
                               const asr_att_beam_ctc* j, int* steps_issued, asr_stream s);
/* Launches on this handle since the last reset, {score, advance, joint_select}: asr_ctc_prefix_score calls (those of
 * asr_att_beam_select_joint included), asr_ctc_prefix_advance calls, asr_att_beam_select_joint calls. */
int asr_att_joint_counts(asr_handle* h, unsigned long long* out3);
int asr_reset_att_joint_counts(asr_handle* h);
/* ---- shallow fusion with an RNN language model in the beam search, native (later within ABI 5, additive) ------ *
 * EXTENSION.  The reference intended it and has none: models/lm/{base,char_rnnlm,word_rnnlm}.py raise NotImplementedError,
 * models/ctc/decoders/charlm_beam_search_decoder.py is empty, and its CTC BeamSearchDecoder.__call__ takes `alpha`
 * ("language model weight") and carries `# TODO: add LM score here` (models/ctc/decoders/beam_search_decoder.py:53,61,132).
 * Shallow fusion as Hori et al. 2017; float64 statement: models/attention/decoders/beam_search/lm_fusion.py.
 * The LM (models/lm/rnnlm.py): an embedding [C2,Em_lm], L unidirectional LSTMBlockCell layers of H units (forget bias 1, no
 * peepholes, optional cell clip; gate columns i, ci, f, o), an output layer [H,C2] + bias, over the attention classes C2 =
 * n_labels + 2.  fp32 throughout.  R = B*W device rows, row b*W + w.
 *
 * struct asr_att_lm.  Weights: W = the layers' kernels one behind the other, layer l [(Din_l + H), 4H] with Din_0 = Em_lm,
 * Din_l = H; b [L,4H].  W_il (optional): the gate-interleaved images one behind the other, layer l (Din_l + H + 1) x 4H floats
 * -- asr_lm_prep writes the images of the layers for which asr_lstm_cell_gemm_ok(R, Din_l + H, H, Din_l + H) holds, once per
 * decode, and asr_lm_step then runs those layers' product + cell as one launch (asr_lstm_cell_gemm_fwd); the others (and
 * every layer without W_il) run asr_gemm_act + asr_lstm_cell_fwd_ex.  asr_lstm_cell_gemm_ok needs R <= 32 and
 * (Din_l + H) % 64 == 0: both paths are live (asr_att_path_counts: ASR_ATT_FWD_CELL_F32IMG / ASR_ATT_FWD_CELL_GEMM count
 * these launches too).  State: c / h [2,L,R,H] -- block 0 is what a step reads, block 1 receives the step's new state (as
 * the beam loop's c_all / h_all); in: the layers' cell-input rows one behind the other, layer 0 [R,Em_lm+H], layer l >= 1
 * [R,2H], each row x | h_prev, so one product per layer suffices: x of layer 0 is the LM embedding of the row's last word,
 * x of layer l >= 1 is written by layer l-1's cell (its cell_out2), h_prev by asr_lm_beam_reorder (on entry: embedding of
 * <SOS> | zeros; c, h block 0 zeros).  live [R] ones; work: R * 10 * H floats.
 * asr_lm_step, in this order: per layer l = 0 .. L-1 the product + cell (above) from in (layer l), c / h block 0 into c / h
 * block 1 (and the next layer's x columns); then lm_logits [R,C2] = h block 1 of layer L-1 x W_out + b_out (asr_gemm_act),
 * raw logits -- no log-softmax pass: the selection normalises them in its own row reduction.
 * asr_att_beam_select_fused: asr_att_beam_select / _joint on two or three score streams (one templated kernel pair with
 * asr_att_beam_select_joint, att_beam.hip: the candidates kernel with or without the LM stream, the rank kernel per set
 * of streams).
 *  1. candidates kernel, a wave per row: lse_att and lse_lm, each in the order of asr_att_beam_select (lane l takes classes
 *     l, l + 64, ... ascending into a running maximum, xor butterfly 32 .. 1; the sum of exp(x - max) the same way;
 *     lse = max + log(sum)); p_att = x - lse_att, p_lm = z - lse_lm; local = p_att + lm_weight * p_lm; the W best classes
 *     other than <EOS> by local (ties by lower index) and <EOS> -> cand, cand_total = log_probs + p_att,
 *     cand_lm = lm_score + p_lm [R,W+1].  A finished row: its <EOS> alone with p_att = p_lm = 0; first_step: slot 0 only.
 *     NOTE the preselection is by the LOCAL fused score, not by the attention logit as asr_att_beam_select_joint's: without
 *     CTC it is lossless (within a row all classes but <EOS> share length and carried totals), with CTC it is the pre-beam.
 *  2. ctc_weight > 0: asr_ctc_prefix_score's kernel on cand, unchanged.
 *  3. rank kernel, a workgroup per utterance: ctc = psi or a finished slot's ctc_score; fused = (1 - ctc_weight) *
 *     cand_total, + ctc_weight * ctc when ctc_weight > 0, + lm_weight * cand_lm, added in that order;
 *     score = fused / penalty(length) with the length rule and lpw == 1 quirk of asr_att_beam_select; a candidate with
 *     ctc = -inf is dropped; the W best by (score descending, flat index ascending) give word / parent / score and the next
 *     state log_probs = cand_total, lm_score = cand_lm, ctc_score, finished, lengths, last as asr_att_beam_select_joint.
 *  1 <= W <= 32, W <= C2 - 1, lm_weight > 0 (0 is the other two selections' job), 0 <= ctc_weight <= 1.  ctc_weight == 0:
 *  y, seq_len, r, last_*, ctc_score_*, psi are not read and may be NULL.  State out may be state in.  With CTC, at 0 frames:
 *  the documented behaviour of asr_att_beam_select_joint (a place nothing reaches also keeps the parent's lm_score).
 * asr_lm_beam_reorder: row r = b*W + w of every layer of c_dst / h_dst [L,R,H] is row b*W + parent[r] of c_src / h_src; the
 * h_prev columns of every layer of in_dst receive the same h rows; the x columns of layer 0 of in_dst are LM embedding row
 * word[r].  Out of place, one launch for all layers.
 * asr_att_decoder_beam_lm: the loop of asr_att_decoder_beam (j NULL) / asr_att_decoder_beam_joint (j given, whose
 * ctc_weight is then in (0, 1]) with, per step on the one stream: the decoder step and head (shared code), asr_lm_step,
 * asr_att_beam_select_fused, asr_ctc_prefix_advance when j is given, asr_att_beam_reorder (those two in the order of
 * asr_att_decoder_beam_joint: they are independent of each other), asr_lm_beam_reorder (block 1 -> block 0).  asr_lm_prep runs once before the first step.  Early exit, back-trace and outputs as those loops; lm_score [R]
 * (zeros on entry) comes out as the hypotheses' LM totals.  Surplus steps change nothing: a finished slot keeps total,
 * lm_score, ctc_score (its LM state moves on, unread). */
typedef struct asr_att_lm {
  int L, H, Em_lm, R, C2;
  float cell_clip, lm_weight;
  const float *emb;                             /* [C2,Em_lm] */
  const float *W, *b;                           /* the layers' [Din_l+H,4H] one behind the other; [L,4H] */
  const float *W_out, *b_out;                   /* [H,C2], [C2] */
  float *W_il;                                  /* optional: the layers' (Din_l+H+1) x 4H images one behind the other */
  float *c, *h;                                 /* state [2,L,R,H] */
  float *in;                                    /* layer 0 [R,Em_lm+H], layers l >= 1 [R,2H], one behind the other */
  const float *live;                            /* [R] ones */
  float *work;                                  /* R * 10 * H floats */
  float *lm_logits;                             /* [R,C2] */
  float *lm_score;                              /* state [R]: zeros on entry, out */
  int32_t *cand;                                /* scratch [R,W+1] (the loop uses these, not the asr_att_beam_ctc's) */
  float *cand_total, *cand_lm;                  /* scratch [R,W+1] each */
} asr_att_lm;
int asr_lm_prep(asr_handle* h, const asr_att_lm* lm, asr_stream s);
int asr_lm_step(asr_handle* h, const asr_att_lm* lm, asr_stream s);
int asr_att_beam_select_fused(asr_handle* h, const float* logits, const float* lm_logits, int B, int W, int n_labels,
                              float length_penalty_weight, float ctc_weight, float lm_weight, int first_step, const float* y,
                              const int32_t* seq_len, int T, int By, int Cc, int blank, const float* r,
                              const float* log_probs_in, const int32_t* finished_in, const int32_t* lengths_in,
                              const int32_t* last_in, const float* ctc_score_in, const float* lm_score_in, int32_t* cand,
                              float* cand_total, float* cand_lm, float* psi, int32_t* word, int32_t* parent, float* score,
                              float* log_probs_out, int32_t* finished_out, int32_t* lengths_out, int32_t* last_out,
                              float* ctc_score_out, float* lm_score_out, int32_t* unfinished, asr_stream s);
int asr_lm_beam_reorder(asr_handle* h, const int32_t* parent, const int32_t* word, int B, int W, int L, int H, int Em_lm,
                        int vocab, const float* c_src, const float* h_src, const float* emb, float* c_dst, float* h_dst,
                        float* in_dst, asr_stream s);
int asr_att_decoder_beam_lm(asr_handle* h, const asr_att_decoder* a, const asr_att_infer* f, const asr_att_beam* m,
                            const asr_att_beam_ctc* j, const asr_att_lm* lm, int* steps_issued, asr_stream s);
/* Calls on this handle since the last reset, {lm_step, fused_select, lm_reorder}. */
int asr_att_lm_counts(asr_handle* h, unsigned long long* out3);
int asr_reset_att_lm_counts(asr_handle* h);
/* ---- CTC prefix beam search with RNN language-model fusion, native (later within ABI 5, additive) ------------- *
 * EXTENSION: the reference's CTC BeamSearchDecoder.__call__ takes alpha ("language model weight") and beta ("insertion
 * bonus"), carries `# TODO: add LM score here` (models/ctc/decoders/beam_search_decoder.py:53,61-62,132) and ships an empty
 * models/ctc/decoders/charlm_beam_search_decoder.py.  Float64 statement: this package's file of that name.
 * asr_ctc_beam_decode's search in which every EXTENSION of a prefix by a class c != blank uses
 *     p_t + alpha * log p_lm(c | <SOS>, prefix) + beta
 * in place of p_t (both the c != last and the c == last / p_b-only branch); the blank update and the merging case get
 * neither term.  log p_lm = log-softmax over all V classes of the LM's raw fp32 logits row, taken in fp64.  The CTC model
 * has C classes, CTC label c is LM class c; the LM has V >= C + 1 classes, its <SOS> / <EOS> lie outside the CTC labels.
 * No <EOS> term at the end, no word-level LM, no n-best output.  1 <= W <= 32 (the LM beam kernels' limit), W <= C - 1.
 *
 * asr_ctc_beam_lm_frame: frame t of the search for all B utterances (one workgroup each); the beam lives in the
 * workspace between the calls (t = 0 initialises it, so the frames must come in order on one stream).  lm_logits [B*W,V]
 * (row b*W + w: the LM's distribution after the prefix in slot w; NULL with alpha == 0: bonus only).  An utterance with
 * t >= seq_len[b] is left as it is (parent = w, word = -1).  Out, per new slot: parent [B,W] (the old slot), word [B,W]
 * (the appended label, or -1 when the slot's prefix was already in the old beam -- a stay, possibly carrying merged
 * extension mass); optionally (may be NULL) the new state: st_pb / st_pnb [B,W] fp64, st_lm [B,W] fp32, st_nb [B].
 * asr_ctc_beam_decode_lm: the whole search from one call, everything on the one stream, no host synchronisation:
 * asr_lm_prep once; one asr_lm_step (the empty prefix: on entry every LM row holds <SOS>'s embedding and zero state, as
 * for asr_att_decoder_beam_lm; lm->R == B*W, lm->C2 is V; lm_weight, lm_score, cand* of the struct are not used); then per
 * frame t = 0 .. T-1: the frame kernel; and, unless it was the last frame, asr_lm_beam_reorder (state block 1 -> block 0
 * by parent, x = embedding of word), asr_lm_step into the other of two logits buffers, and the commit kernel (rows with
 * word == -1 take back their parent's state and logits row).  Then the back-trace: out_labels [B,T] padded -1, out_len [B],
 * out_score [B] fp64 = -logsumexp(p_b, p_nb) of the best entry INCLUDING the LM and bonus terms, out_lm_score [B] fp32 =
 * its alpha-unweighted sum of log p_lm.  lm == NULL needs alpha == 0 (no LM launches at all).  seq_len[b] == 0: the empty
 * hypothesis, score 0.  alpha == 0 and beta == 0: asr_ctc_beam_decode's result, bit for bit. */
size_t asr_ctc_beam_lm_workspace_bytes(int T, int B, int C, int beam_width, int V);
int asr_ctc_beam_lm_frame(asr_handle* h, const float* logits, int t, int T, int B, int C, const int32_t* seq_len, int blank,
                          int beam_width, double alpha, double beta, const float* lm_logits, int V, int32_t* parent,
                          int32_t* word, double* st_pb, double* st_pnb, float* st_lm, int32_t* st_nb, void* workspace,
                          size_t workspace_bytes, asr_stream s);
int asr_ctc_beam_decode_lm(asr_handle* h, const float* logits, int T, int B, int C, const int32_t* seq_len, int blank,
                           int beam_width, double alpha, double beta, const asr_att_lm* lm, int32_t* out_labels,
                           int32_t* out_len, double* out_score, float* out_lm_score, void* workspace,
                           size_t workspace_bytes, asr_stream s);
/* Launches on this handle since the last reset, {frame kernels, lm steps, commits}. */
int asr_ctc_beam_lm_counts(asr_handle* h, unsigned long long* out3);
int asr_reset_ctc_beam_lm_counts(asr_handle* h);
/* work: B*(5*U + 3*T + E2) floats.  dav_cell is consumed (its rows accumulate the query-path gradient in place). */
int asr_att_decoder_bwd(asr_handle* h, const asr_att_decoder* a, asr_stream s);
/* ---- GRU decoder cell (later within ABI 5, additive) ---------------------------------------------------------- *
 * decoder_type 'gru': tf.contrib.rnn.GRUCell as the decoder cell (attention_seq2seq.py:364-365; DEVIATION: the
 * reference reads self.num_units there, which does not exist -- it is read as decoder_num_units).  With U units,
 * x = embedding | previous context (Dx columns), Din = Dx + U, and one input row = x | h:
 *     [r, u] = sigmoid([x, h] W_g + b_g)        W_g [Din,2U] (columns r | u), b_g [2U]
 *     c      = tanh([x, r*h] W_c + b_c)         W_c [Din,U], b_c [U]
 *     hn     = u*h + (1-u)*c;  cell_out = hn * out_mask;  h' = live ? hn : h
 * No peepholes, no forget bias, no cell clip (GRUCell has none).  fp32 weights only.
 * asr_gru_cell_prep writes the image W3 [(Din+1), 3U] every product below reads: columns [0,2U) = W_g, columns [2U,3U) =
 * W_c with its U h-rows ZEROED (so x W3 gives the gate pre-activations and the x-part of the candidate's in one product,
 * and dpre W3^T the whole cell-input gradient but the r*h path), row Din = b_g | b_c.
 * Forward of one step: gates [B,4U] = r | u | c | r*h is what the backward needs (the candidate's x-part passes through
 * the c columns between the two phases); h_out [B,U]; cell_out (row stride ld_c >= U); h_out2 / cell_out2 (may be NULL):
 * the same values into column blocks of wider arrays (row strides ld_h2 / ld_c2).  x rows have stride ldx and hold
 * x | h_prev, h_prev [B,U] is the same state contiguous.  W_ch = W_c + Dx*U (the h-rows of the candidate kernel, [U,U]).
 * asr_gru_cell_fwd_ex: any shape, four launches (asr_gemm_act -> gates -> asr_gemm_act -> output); work: B*4U floats.
 * asr_gru_cell_gemm_fwd: two launches, each a skinny exact-fp32 MFMA product with the cell arithmetic in its epilogue
 * (A: x W3, sigmoid, r*h; B: (r*h) W_ch, tanh, state update and scatter); asr_gru_cell_gemm_ok states its shapes:
 * B <= 32, Din % 64 == 0, U % 16 == 0, ldx % 4 == 0 (and 16-byte aligned x, gates).
 * Rows with live == 0 carry h; rows are independent, so padding rows need only hold finite-or-not initialised memory. */
int asr_gru_cell_prep(asr_handle* h, const float* W_g, const float* b_g, const float* W_c, const float* b_c, int Din,
                      int U, float* W3, asr_stream s);
int asr_gru_cell_gemm_ok(int B, int Din, int U, int ldx);
int asr_gru_cell_fwd_ex(asr_handle* h, const float* x, int ldx, int Din, const float* W3, const float* W_ch,
                        const float* h_prev, const float* live, const float* out_mask, int B, int U, float* gates,
                        float* h_out, float* cell_out, int ld_c, float* h_out2, int ld_h2, float* cell_out2, int ld_c2,
                        float* work, asr_stream s);
int asr_gru_cell_gemm_fwd(asr_handle* h, const float* x, int ldx, int Din, const float* W3, const float* W_ch,
                          const float* h_prev, const float* live, const float* out_mask, int B, int U, float* gates,
                          float* h_out, float* cell_out, int ld_c, float* h_out2, int ld_h2, float* cell_out2, int ld_c2,
                          asr_stream s);
/* Backward of one step.  dcell [B,U]: gradient w.r.t. cell_out; dh_c (+ dh_c2 with row stride ld2, may be NULL): the
 * carried gradient w.r.t. h'.  With dhn = out_mask*dcell + live*dh_c:
 *     dc = dhn*(1-u); du = dhn*(h-c); dp = dc*(1-c^2); d_rh = dp W_ch^T; dr = d_rh*h
 *     dpre [B,3U] = dr*r*(1-r) | du*u*(1-u) | dp
 *     d_in [B,Din] = dpre W3^T        (x columns: d_x; h columns: dg W_g[h rows]^T)
 *     dh_prev_carry [B,U] = (1-live)*dh_c + dhn*u + d_rh*r      (the caller adds d_in's h columns)
 * Launches: elementwise (dp, du, dhn) -> asr_gemm_act (d_rh) -> elementwise (dr, carry) -> asr_gemm_act (d_in); the
 * mask and the dh_c2 add are folded into the first kernel.  work: 2*B*U floats.  Weight gradients are the caller's,
 * batched over steps: dW3 = in^T dpre (W_g = columns [0,2U); W_c x-rows = columns [2U,3U) of rows < Dx),
 * dW_c[h rows] = (r*h)^T dp, biases = column sums. */
int asr_gru_cell_bwd(asr_handle* h, const float* dcell, const float* dh_c, const float* dh_c2, int ld2,
                     const float* out_mask, const float* live, const float* gates, const float* h_prev,
                     const float* W3, const float* W_ch, int B, int Din, int U, float* dpre, float* dh_prev_carry,
                     float* d_in, int ld_din, float* work, asr_stream s);
/* The decoder loops with the GRU cell: asr_att_decoder_fwd / _bwd / _infer / _beam with the cell launches replaced by the
 * ones above and everything else (query FC, attention, head, selection, re-ordering) issued exactly as there.  `a` as for
 * those calls except: W_cell, b_cell, peep, craw_all, dc0 are not read (NULL allowed); c_all is read only by the beam
 * loop (asr_att_beam_reorder gathers it: give it zeros [2,R,U]); gates_all [To,B,4U] holds r | u | c | r*h; dpre_all is
 * [To,B,3U] (asr_gru_cell_bwd's dpre); forget_bias / cell_clip / W_cell_il / W_cell_h are ignored.  g->W3: (Din+1)*3U
 * floats of work space, written once per call (asr_gru_cell_prep).  The two-launch form runs where
 * asr_gru_cell_gemm_ok(B, Din, U, Din) and g->fused != 0, the four-launch form everywhere else (a beam's B*W rows). */
typedef struct asr_att_gru {
  const float *W_g, *b_g, *W_c, *b_c;           /* [Din,2U], [2U], [Din,U], [U]; rows: embedding | context | h */
  float *W3;                                    /* work space, (Din+1)*3U floats */
  int fused;                                    /* 0: always the four-launch form (A/B) */
} asr_att_gru;
int asr_att_decoder_fwd_gru(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, asr_stream s);
int asr_att_decoder_bwd_gru(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, asr_stream s);
int asr_att_decoder_infer_gru(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, const asr_att_infer* f,
                              int* steps_issued, asr_stream s);
int asr_att_decoder_beam_gru(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, const asr_att_infer* f,
                             const asr_att_beam* m, int* steps_issued, asr_stream s);
/* GRU decoder steps on this handle since the last reset: {two-launch forward steps, four-launch forward steps,
 * backward steps} (the loops and the single-step entry points both count). */
int asr_att_gru_counts(asr_handle* h, unsigned long long* out3);
int asr_reset_att_gru_counts(asr_handle* h);
/* ---- multi-layer LSTM decoder (later within ABI 5, additive) ---------------------------------------------------- *
 * decoder_num_layers = L > 1: the decoder cell is MultiRNNCell of L LSTMBlockCell(U), each in a DropoutWrapper(output
 * keep).  Layer 0 is the cell of asr_att_decoder (input row embedding | previous context | its own previous h); upper
 * layer l = 1 .. L-1 reads x_l = [ o_{l-1} | h_{l,k-1} ] (2U wide), o_l = mask_l * h_l; the top layer's o_{L-1} is the
 * decoder's cell output (query, av_in[:, :U]).  A row with live == 0 keeps the state of every layer.  Everything behind
 * the cell -- query FC, energies, softmax + context, the fused attention step, the heads, the selections -- is the
 * code of the one-layer calls.  The upper layers run in fp32 on the weights given here, also where layer 0 streams bf16
 * images.  One asr_att_stack_layer per upper layer, up[l-1] for layer l; step arrays as asr_att_decoder's:
 *   W [2U,4U] (rows o_{l-1} then h; gate-major columns i, ci, f, o), b [4U], peep [3,U] or NULL, dmask [To,B,U] or NULL;
 *   in [To,B,2U]: the saved input rows -- columns [0,U) written by the layer below at the same step, columns [U,2U) by the
 *     layer itself at the step before; the caller fills in[0][:, U:] with the layer's initial h;
 *   c, h [To+1,B,U] (row 0: the initial state); gates [To,B,4U], craw [To,B,U];
 *   W_il: optional (2U+1)*4U floats of work space -- where asr_lstm_cell_gemm_ok(B, 2U, U, 2U) holds the loop writes the
 *     layer's interleaved image there once per call and its step is ONE launch (asr_lstm_cell_gemm_fwd), elsewhere (and
 *     without it) asr_gemm_act + asr_lstm_cell_fwd_ex;
 *   backward only: dpre [To,B,4U], d_hin [To,B,U] (the h-columns of the step's dpre W^T: what the layer's step before
 *     adds to its carried dh), dpeep [To,B,3U] or NULL (needed with peep), dc0, dh0 [B,U] (out: gradient w.r.t. the
 *     layer's initial state).
 * work (backward only): (L-1)*4*B*U + B*U floats -- per upper layer the carried dc / dh, two buffers each (ping-pong),
 * and one [B,U] block of the generic form.
 * Inference (asr_att_decoder_infer_stack): in / c / h as in training (To = max_decode_length), gates / craw ONE step.
 * Beam (asr_att_decoder_beam_stack): in [2,R,2U], c / h [2,R,U] -- block 0 is what a step reads (the caller fills c, h
 * and in[:, U:] with the initial state, each utterance's row W times), block 1 receives the step's outputs and
 * asr_att_stack_reorder gathers it back by parent; gates / craw one step.
 * Backward of step k (asr_att_decoder_bwd_stack): the top layer's cell backward takes the place of the one-layer
 * loop's (fused with the query FC where that loop fuses it); then for l = L-2 .. 0
 *     dx = dpre_{l+1}[k] W_{l+1}^T [B,2U];  d_hin_{l+1}[k] = dx[:, U:];  cell backward of layer l on  mask_l * dx[:, :U]
 *     (+ carried dc_l, carried dh_l + d_hin_l[k+1]; layer 0: the h-columns of d_in_all[k+1])   ->   dpre_l[k]
 * as ONE launch (exact-fp32 MFMA product, the cell in its epilogue) where asr_att_stack_bwd_ok(B, U) holds -- B <= 32,
 * U % 16 == 0 -- and `fused` != 0, and as asr_gemm_act x 2 (the two column halves) + the plain cell backward launch at
 * every other shape.  Layer 0's own d_in product follows as ever.  cell_clip is straight-through at every layer.  Weight
 * gradients are the caller's, batched over the steps: dW_l = in_l^T dpre_l, db_l = column sums, peepholes from dpeep.
 * Not with scheduled sampling, the joint or the LM-fused search (those loops run one layer). */
#define ASR_ATT_STACK_MAX 7                     /* upper layers: decoder_num_layers <= 8 */
typedef struct asr_att_stack_layer {
  const float *W, *b, *peep, *dmask;
  float *in, *c, *h, *gates, *craw, *W_il;
  float *dpre, *d_hin, *dpeep, *dc0, *dh0;      /* backward only */
} asr_att_stack_layer;
typedef struct asr_att_stack {
  int L;                                        /* decoder_num_layers, 2 .. ASR_ATT_STACK_MAX + 1 */
  int fused;                                    /* 0: the generic backward form at every shape (A/B) */
  asr_att_stack_layer up[ASR_ATT_STACK_MAX];    /* up[l-1]: layer l */
  float *work;                                  /* backward only */
} asr_att_stack;
int asr_att_decoder_fwd_stack(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* k, asr_stream s);
int asr_att_decoder_bwd_stack(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* k, asr_stream s);
int asr_att_decoder_infer_stack(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* k, const asr_att_infer* f,
                                int* steps_issued, asr_stream s);
int asr_att_decoder_beam_stack(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* k, const asr_att_infer* f,
                               const asr_att_beam* m, int* steps_issued, asr_stream s);
/* One launch: for every upper layer, row r = b*W + w of block 0 of c, h [2,R,U] and of columns [U,2U) of in [2,R,2U]
 * becomes row b*W + parent[r] of block 1 (out of place).  parent [B,W], each in [0, W). */
int asr_att_stack_reorder(asr_handle* h, const asr_att_stack* k, const int32_t* parent, int B, int W, int U, asr_stream s);
/* The backward of one lower layer at one step, on its own: dx [B,2U] = dpre_up [B,4U] W_up^T ([2U,4U]), d_hin_up [B,U] =
 * dx[:, U:], and the cell backward (operands as asr_lstm_cell_bwd's, plus dh_next2 with row stride ld2 and use_mask, both
 * may be NULL) on dx[:, :U].  fused != 0 and asr_att_stack_bwd_ok(B, U) (and 16-byte aligned dpre_up, W_up): the one-launch
 * form; else the generic one (work: B*U floats). */
int asr_att_stack_bwd_ok(int B, int U);
int asr_att_stack_bwd_step(asr_handle* h, const float* dpre_up, const float* W_up, int B, int U, const float* dc_next,
                           const float* dh_next, const float* dh_next2, int ld2, const float* gates, const float* c_raw,
                           const float* c_prev, const float* peep, const float* live, const float* use_mask, float* dpre,
                           float* dc_prev, float* dh_prev_carry, float* dpeep_rows, float* d_hin_up, float* work, int fused,
                           asr_stream s);
/* Upper-layer steps on this handle since the last reset: {forward on the image (one launch), forward as product + cell
 * (two launches), backward fused (one launch), backward generic}. */
int asr_att_stack_counts(asr_handle* h, unsigned long long* out4);
int asr_reset_att_stack_counts(asr_handle* h);
/* out[b, j] = x[b*ldx + j] + y[b*ldy + j], j < W (row blocks of wider arrays; out may alias x) */
int asr_add_cols(asr_handle* h, const float* x, int ldx, const float* y, int ldy, float* out, int ldo, int B, int W,
                 asr_stream s);
int asr_tanh_fwd(asr_handle* h, const float* x, float* y, size_t n, asr_stream s);
int asr_tanh_bwd(asr_handle* h, const float* dy, const float* y, float* dx, size_t n, asr_stream s);
/* tf.nn.embedding_lookup (attention_seq2seq.py:439) and its gradient (deterministic) */
int asr_embedding_gather(asr_handle* h, const float* W, const int32_t* ids, int rows, int E,
                         float* out, asr_stream s);
int asr_embedding_scatter(asr_handle* h, const float* dout, const int32_t* ids, int rows, int E,
                          int vocab, float* dW, asr_stream s);
/* sparse softmax cross-entropy per row of logits[rows,C] (+eps), weighted (sequence_loss,
 * attention_seq2seq.py:625-637): row_loss[r] = w[r]*xent; dlogits = (softmax-onehot)*w*dscale */
int asr_seq_xent(asr_handle* h, const float* logits, const int32_t* targets, const float* weights,
                 int rows, int C, float eps, float dscale, float* row_loss, float* dlogits,
                 asr_stream s);
/* EXTENSION (later within ABI 5): asr_seq_xent against the label-smoothed target q = (1 - smoothing) * onehot + smoothing / C
 * (label_smoothing_prob of the reference's examples/timit/config/attention/att_baseline.yml and
 * regularization/att_blstm_location_ls.yml; none of its code reads the key): row_loss[r] = w[r] * (lse - (1 - smoothing)
 * (x_tgt + eps) - (smoothing / C) sum_c (x_c + eps)), dlogits = (softmax - q) * w * dscale; rows with w == 0 are exact
 * zeros.  0 <= smoothing < 1; smoothing == 0 is asr_seq_xent bit for bit. */
int asr_seq_xent_ls(asr_handle* h, const float* logits, const int32_t* targets, const float* weights,
                    int rows, int C, float eps, float smoothing, float dscale, float* row_loss, float* dlogits,
                    asr_stream s);
int asr_argmax_rows(asr_handle* h, const float* x, int rows, int C, int32_t* out, asr_stream s);

/* ---- gradient clipping + optimizers -------------------------------------- *
 * Multi-tensor over one flat fp32 parameter buffer; tensor i is
 * [offsets[i], offsets[i+1]).  tf.clip_by_norm per variable
 * (models/model_base.py:148-152): g *= clip / max(||g||_2, clip). */
/* Norms are reduced in fixed 4096-element chunks (deterministic).  asr_clip_plan (host
 * helper) fills chunk_start_host[num_tensors+1] from HOST offsets; upload it once.
 * partial_ws: chunk_start[num_tensors] (= total_chunks) floats of device scratch. */
int asr_clip_plan(asr_handle* h, const int64_t* offsets_host, int num_tensors,
                  int64_t* chunk_start_host);
int asr_clip_by_norm_multi(asr_handle* h, float* grads, const int64_t* offsets,
                           const int64_t* chunk_start, int num_tensors, int64_t total_chunks,
                           float clip_norm, float* partial_ws, asr_stream s);
/* weight decay term of ctc.py:280-286: grads += wd * params on tensors with decay_mask[i]!=0;
 * l2_out (device fp32, may be NULL) receives wd * sum(0.5*||p||^2). */
int asr_weight_decay(asr_handle* h, float* grads, const float* params, const int64_t* offsets,
                     const uint8_t* decay_mask, int num_tensors, float wd, float* l2_out,
                     asr_stream s);
/* One optimizer step over n fp32 parameters with TF1 default hyper-parameters
 * (models/model_base.py:68-95).  slot0/slot1: optimizer state
 * (momentum / accumulators / m,v), `step` = 1-based step count (Adam bias correction). */
int asr_optimizer_step(asr_handle* h, int optimizer, float* params, const float* grads,
                       float* slot0, float* slot1, size_t n, float lr, int64_t step,
                       asr_stream s);
/* p[i] = (a[i] + b[i]) * scale helpers for the tower mean of utils/training/multi_gpu.py:39-40 */
int asr_scale(asr_handle* h, float* x, size_t n, float scale, asr_stream s);

/* ---- data-parallel collective (RCCL over xGMI) ------------------------------------------------ *
 * The tower mean of utils/training/multi_gpu.py:13-48 (average_gradients: per variable, stack the N towers'
 * already-clipped gradients and reduce_mean) and its caller examples/librispeech/training/train_ctc.py:112-147, as
 * ONE all-reduce(sum) over the flat fp32 gradient buffer + x 1/world -- one process per GPU.  librccl.so is opened
 * with dlopen (asr_comm_set_library names it; default: the loader's librccl.so.1) so that a host that already has
 * one loaded (PyTorch) shares the instance.  Bootstrap as for NCCL: rank 0 calls asr_comm_unique_id (128 bytes,
 * host memory), the host program hands the bytes to every rank, every rank calls asr_comm_init. */
typedef struct asr_comm asr_comm;
int asr_comm_set_library(const char* path);
int asr_comm_unique_id(void* id128_host);
int asr_comm_init(asr_comm** out, asr_handle* h, int rank, int world, const void* id128_host);
int asr_comm_destroy(asr_comm* c);
int asr_comm_info(asr_comm* c, int* rank, int* world);
/* buf[0..n) <- mean over ranks, in place, asynchronous on `s`; every rank calls it with the same n.  buf: any 4-byte
 * aligned device pointer. */
int asr_allreduce_mean(asr_comm* c, float* buf, size_t n, asr_stream s);

#ifdef __cplusplus
}
#endif
#endif /* ASR_HIP_H_ */
