// The attention decoder's native loops: teacher-forced forward, scheduled-sampling forward, greedy inference, beam
// search (attention alone, joint with CTC prefix scores, fused with a language model) and the backward, each one call
// that issues every launch of every step.  Host code and the two token-selection kernels only: the attention kernels
// and their launchers are attention.hip's (att_launch.h), the GRU cell's launches gru_decoder.hip's, the upper layers
// of a decoder stack dec_stack.hip's, the beam selection / re-ordering / backtrace att_beam.hip's.
#include "common.h"
#include "att_launch.h"
#include "argmax_first.h"
#include <math.h>

// Which cell a loop runs: g != nullptr (the *_gru entry points) the GRU of gru_decoder.hip, sk != nullptr (the *_stack
// entry points) upper LSTM layers above the LSTM cell (dec_stack.hip); neither is every call without a suffix.
struct DecCell {
  const asr_att_gru* g;
  const asr_att_stack* sk;
};

// What a loop call must bring (everything refused is ASR_ERR_INVALID_ARG):
//   every call     a; To, B, T, U, E2, A >= 1, Em >= 0; att_mode 0 or 1; W_q with a query FC, A == U without; v (mode 0) /
//                  keys (mode 1); enc, seq_len; the step arrays live, dec_in, av_in, alpha_all, gates_all, h_all, qz_all;
//                  work; with carry_alpha: filt, wfil, alpha_zero, taps >= 1
//   LSTM cell      W_cell, b_cell, craw_all, c_all              (plain and stack calls; not asked of a GRU call)
//   GRU            asr_gru_dec_check on the GRU block; a stack with it is refused
//   stack          asr_stack_dec_check on the stack block, then everything of the LSTM cell for layer 0
//   backward       dav_cell, dav_ctx, dctx_all, dpre_all, dqz_all, d_in_all, dh0; dv_all (mode 0); with carry_alpha:
//                  dwfil_rows, dfilt_rows
//   backward, LSTM dc0; dpeep_all with peepholes                (a GRU has no cell state and ignores peep)
static int dec_check(asr_handle* h, const asr_att_decoder* a, bool bwd, DecCell c) {
  if (!a) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder: bad arguments");
  if (c.sk && c.g) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder: a stack runs LSTM cells only");
  if (c.sk) ASR_TRY(asr_stack_dec_check(h, a, c.sk, bwd));
  if (c.g) ASR_TRY(asr_gru_dec_check(h, a, c.g));
  const bool common = a->To >= 1 && a->B >= 1 && a->T >= 1 && a->U >= 1 && a->Em >= 0 && a->E2 >= 1 && a->A >= 1 &&
                      (a->att_mode == 0 || a->att_mode == 1) && (a->has_query_fc ? a->W_q != nullptr : a->A == a->U) &&
                      (a->att_mode == 0 ? a->v != nullptr : a->keys != nullptr) && a->enc && a->seq_len && a->live &&
                      a->dec_in && a->av_in && a->alpha_all && a->gates_all && a->h_all && a->qz_all && a->work &&
                      (!a->carry_alpha || (a->filt && a->wfil && a->alpha_zero && a->taps >= 1));
  const bool lstm = c.g || (a->W_cell && a->b_cell && a->craw_all && a->c_all);
  if (!common || !lstm) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder: bad arguments");
  if (!bwd) return ASR_OK;
  const bool bwd_common = a->dav_cell && a->dav_ctx && a->dctx_all && a->dpre_all && a->dqz_all && a->d_in_all && a->dh0 &&
                          (a->att_mode != 0 || a->dv_all) && (!a->carry_alpha || (a->dwfil_rows && a->dfilt_rows));
  const bool bwd_lstm = c.g || (a->dc0 && (!a->peep || a->dpeep_all));
  if (!bwd_common || !bwd_lstm) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_bwd: bad arguments");
  return ASR_OK;
}

// The fused cell launch of a step needs the caller's work space for a weight image: the interleaved fp32 one
// (asr_lstm_cell_gemm_fwd) or the bf16 ones (asr_lstm_cell_gemm_*_h, both loops)
static inline bool dec_cell_image_ok(const asr_att_decoder* a, const void* image) {
  const int Din = a->Em + a->E2 + a->U;
  return image && asr_lstm_cell_gemm_ok(a->B, Din, a->U, Din) && ((uintptr_t)a->dec_in | (uintptr_t)image) % 16 == 0;
}
static inline bool dec_cell_gemm(const asr_att_decoder* a) { return dec_cell_image_ok(a, a->W_cell_il); }
static inline bool dec_cell_gemm_h(const asr_att_decoder* a) { return a->U % 16 == 0 && dec_cell_image_ok(a, a->W_cell_h); }
static int dec_cell_image(asr_handle* h, const asr_att_decoder* a, DecCell c, asr_stream s) {
  if (c.sk) ASR_TRY(asr_stack_dec_image(h, a, c.sk, s));   // (the upper layers' images; layer 0's below, as ever)
  if (c.g) return asr_gru_dec_image(h, a, c.g, s);
  if (dec_cell_gemm_h(a)) return asr_lstm_cell_gemm_prep_h(h, a->W_cell, a->b_cell, a->Em + a->E2 + a->U, a->U, a->W_cell_h, s);
  if (!dec_cell_gemm(a)) return ASR_OK;
  return asr_lstm_cell_gemm_prep(h, a->W_cell, a->b_cell, a->Em + a->E2 + a->U, a->U, a->W_cell_il, s);
}

// One forward step of the decoder loop: cell-input GEMM -> cell -> query FC -> energies -> softmax + context.  k indexes
// the step arrays that carry the recurrence (dec_in, av_in, c / h, alpha, live); ks the saved activations only the
// backward reads (gates, raw cell, query: the inference loop reuses row 0).
// c.g: the cell launches are the GRU's (asr_gru_dec_fwd_step, same scatter targets); everything behind them is shared.
// c.sk: layer 0's masked output goes to the input row of layer 1 instead of av / the query, and the upper layers' cell
// launches follow it (asr_stack_dec_fwd_step: the top layer writes av[:, :U] and the query).
static int dec_fwd_step(asr_handle* h, const asr_att_decoder* a, DecCell c, int k, int ks, bool more, asr_stream s) {
  const asr_att_stack* sk = c.sk;
  const int B = a->B, U = a->U, T = a->T, E2 = a->E2, Em = a->Em, A = a->A;
  const int Din = Em + E2 + U, Dav = U + E2;
  float* pre = a->work;                                    // [B,4U]
  float* hraw = pre + (size_t)B * 4 * U;                   // [B,U]
  float* energy = hraw + (size_t)B * U;                    // [B,T]
  float* ctx = energy + (size_t)B * T;                     // [B,E2]
  float* din = a->dec_in + (size_t)k * B * Din;
  float* dnext = more ? din + (size_t)B * Din : nullptr;
  float* av = a->av_in + (size_t)k * B * Dav;
  float* qz = a->qz_all + (size_t)ks * B * A;
  if (c.g) {
    ASR_TRY(asr_gru_dec_fwd_step(h, a, c.g, k, ks, dnext, qz, s));
  } else {
    // the cell output (times its dropout mask) lands in av[:, :U]; without a query FC it IS the query
    float* q0 = (a->has_query_fc || sk) ? nullptr : qz;
    float* out0 = sk ? sk->up[0].in + (size_t)k * B * 2 * U : av;
    const int ld0 = sk ? 2 * U : Dav;
    // the cell's operands are the same behind whichever launch forms the gates' pre-activations
    auto cell = [&](auto launch, auto... gates_from) {
      return launch(h, gates_from..., a->c_all + (size_t)k * B * U, a->h_all + (size_t)k * B * U, a->peep,
                    a->live + (size_t)k * B, B, U, a->forget_bias, a->cell_clip, a->gates_all + (size_t)ks * B * 4 * U,
                    a->craw_all + (size_t)ks * B * U, a->c_all + (size_t)(k + 1) * B * U, a->h_all + (size_t)(k + 1) * B * U,
                    hraw, a->dmask ? a->dmask + (size_t)k * B * U : nullptr, q0, dnext ? dnext + Em + E2 : nullptr, Din,
                    out0, ld0, s);
    };
    if (dec_cell_gemm_h(a)) {         // product + cell as one launch on the bf16 fragment image (dec_cell_image)
      h->att_counts[ASR_ATT_FWD_CELL_BF16] += 1;
      ASR_TRY(cell(asr_lstm_cell_gemm_fwd_h, din, Din, Din, a->W_cell_h));
    } else if (dec_cell_gemm(a)) {    // ... on the fp32 interleaved weight image
      h->att_counts[ASR_ATT_FWD_CELL_F32IMG] += 1;
      ASR_TRY(cell(asr_lstm_cell_gemm_fwd, din, Din, Din, a->W_cell_il, a->b_cell ? 1 : 0));
    } else {
      h->att_counts[ASR_ATT_FWD_CELL_GEMM] += 1;
      ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, B, 4 * U, Din, din, Din, a->W_cell, 4 * U, pre, 4 * U, a->b_cell, 0, 0, s));
      ASR_TRY(cell(asr_lstm_cell_fwd_ex, pre));
    }
  }
  if (sk) ASR_TRY(asr_stack_dec_fwd_step(h, a, sk, k, ks, more, a->has_query_fc ? nullptr : qz, s));
  if (a->has_query_fc)
    ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, B, A, U, av, Dav, a->W_q, a->ld_wq, qz, A, a->b_q, 0, 0, s));
  if (att_fused_step(h, a, qz, a->alpha_all + (size_t)k * B * T, ctx, av + U, Dav, dnext ? dnext + Em : nullptr, Din, s)) {
    h->att_counts[ASR_ATT_FWD_STEP_FUSED] += 1;
    ASR_CHECK_LAUNCH(h, "asr_att_decoder_fwd(fused step)");
    return ASR_OK;
  }
  h->att_counts[ASR_ATT_FWD_STEP_4LAUNCH] += 1;
  if (a->carry_alpha)
    ASR_TRY(loc_energy_fwd_launch(h, k > 0 ? a->alpha_all + (size_t)(k - 1) * B * T : a->alpha_zero, a->filt, a->wfil,
                                  a->keys, qz, a->v, T, B, A, a->taps, energy, a->seq_len, s));
  else
    ASR_TRY(energy_fwd_launch(h, a->keys, qz, a->v, T, B, A, a->att_mode, energy, a->seq_len, s));
  ASR_TRY(asr_att_softmax_ctx_fwd_ex(h, energy, a->seq_len, a->sharpening, a->enc, a->enc_dtype, T, B, E2,
                                     a->alpha_all + (size_t)k * B * T, ctx,
                                     a->snorm_all ? a->snorm_all + (size_t)k * B : nullptr, av + U, Dav,
                                     dnext ? dnext + Em : nullptr, Din, s));
  return ASR_OK;
}

// The head of a step, for the loops that need the logits while they run: av_out = tanh(av_in . W_av) [rows,U], logits_out
// = av_out . W_out + b_out [rows,C2].  f: asr_att_infer or asr_att_decoder_ss (W_av, W_out, b_out, C2).
template <typename Head>
static int dec_head_step(asr_handle* h, const asr_att_decoder* a, const Head* f, int rows, const float* av_in, float* av_out,
                         float* logits_out, asr_stream s) {
  const int U = a->U, Dav = U + a->E2, C2 = f->C2;
  ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, rows, U, Dav, av_in, Dav, f->W_av, U, av_out, U, nullptr, 0, 0, s));
  ASR_TRY(asr_tanh_fwd(h, av_out, av_out, (size_t)rows * U, s));
  return asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, rows, C2, U, av_out, U, f->W_out, C2, logits_out, C2, f->b_out, 0, 0, s);
}

// Early exit of a decode loop without draining the pipeline: every `every` steps the loop's device counter of that step
// (rows still live / slots unfinished) is copied to the caller's pinned words behind the step's kernels.  A check point
// looks at the newest copy that has ALREADY landed and, so that the host cannot run arbitrarily far past the end of the
// decode (it enqueues a step in a fraction of the time the device takes to run one), waits for the copy of two check
// points ago: the issue loop stays 2 .. 3 intervals ahead of the device, never idle, and at most that many surplus steps
// are enqueued.  The result does not depend on how many were: a step with nothing live changes nothing but its own
// (imputed: zero) outputs, and the caller trims at the first such step.
struct EarlyExit {
  static constexpr int NEV = 3;
  hipEvent_t ev[NEV] = {nullptr, nullptr, nullptr};
  int every = 0;
  ~EarlyExit() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  // every_ > 0 switches the checks on; false: an event could not be created
  bool begin(int every_) {
    every = every_;
    for (int i = 0; every && i < NEV; ++i)
      if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return false;
    return true;
  }
  // in front of step k; true: issue no further step -- the decode has ended, or (*rc = ASR_ERR_HIP) a call failed
  bool check(int k, const int32_t* device_counter, int32_t* host_words, hipStream_t st, int* rc) {
    if (!every || k % every != 0 || k == 0) return false;
    const int c = k / every;                               // this check point; c - 1 was recorded one interval ago
    bool done = false;
    if (c >= 3) {
      (void)hipEventSynchronize(ev[(c - 2) % NEV]);
      done = host_words[(c - 2) * every] == 0;
    }
    if (!done && c >= 2 && hipEventQuery(ev[(c - 1) % NEV]) == hipSuccess) done = host_words[(c - 1) * every] == 0;
    if (done) return true;
    if (hipMemcpyAsync(host_words + k, device_counter + k, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipEventRecord(ev[c % NEV], st) != hipSuccess) {
      *rc = ASR_ERR_HIP;
      return true;
    }
    return false;
  }
};

static int dec_fwd_loop(asr_handle* h, const asr_att_decoder* a, DecCell c, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_TRY(dec_check(h, a, false, c));
  ASR_TRY(dec_cell_image(h, a, c, s));
  for (int k = 0; k < a->To; ++k) ASR_TRY(dec_fwd_step(h, a, c, k, k, k + 1 < a->To, s));
  return ASR_OK;
}
extern "C" int asr_att_decoder_fwd(asr_handle* h, const asr_att_decoder* a, asr_stream s) {
  return dec_fwd_loop(h, a, {nullptr, nullptr}, s);
}
extern "C" int asr_att_decoder_fwd_gru(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, asr_stream s) {
  if (!h || !g) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_fwd_gru: bad arguments");
  return dec_fwd_loop(h, a, {g, nullptr}, s);
}
extern "C" int asr_att_decoder_fwd_stack(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, asr_stream s) {
  if (!h || !sk) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_fwd_stack: bad arguments");
  return dec_fwd_loop(h, a, {nullptr, sk}, s);
}

// ---------------------------------------------------------------- greedy inference loop
namespace {
// One workgroup per batch row, behind the output layer of decoder step k: id = argmax(logits) (first maximum wins, as
// asr_argmax_rows), emitted id = id for a row that was live at the start of the step and 0 otherwise (impute_finished),
// live[k+1] = live[k] && id != eos, live_count[k+1] += live[k+1]; the NEXT step's input row gets the embedding of id
// (whatever the row's state: GreedyEmbeddingHelper.next_inputs does not look at `finished`) and its context columns
// are zeroed for rows that had finished before this step (dynamic_decode zeroes next_inputs' attention part with the
// imputed outputs, dynamic_decoder.py:172-190).
__global__ __launch_bounds__(256) void att_infer_select_kernel(const float* __restrict__ logits, int C2, int eos,
                                                               const float* __restrict__ live_k, float* __restrict__ live_n,
                                                               int32_t* __restrict__ count_n, int32_t* __restrict__ ids,
                                                               const float* __restrict__ emb, int Em, float* __restrict__ dnext,
                                                               int Din, int E2) {
  const int b = blockIdx.x;
  const int id = argmax_first_block256(logits + (size_t)b * C2, C2);
  const float lv = live_k[b];
  if (threadIdx.x == 0) {
    ids[b] = lv != 0.f ? id : 0;
    const float ln = (lv != 0.f && id != eos) ? 1.f : 0.f;
    live_n[b] = ln;
    if (ln != 0.f) atomicAdd(count_n, 1);
  }
  if (dnext) {
    float* d = dnext + (size_t)b * Din;
    const float* e = emb + (size_t)id * Em;
    for (int j = threadIdx.x; j < Em; j += 256) d[j] = e[j];
    if (lv == 0.f)
      for (int j = threadIdx.x; j < E2; j += 256) d[Em + j] = 0.f;
  }
}
}  // namespace

static int dec_infer_loop(asr_handle* h, const asr_att_decoder* a, DecCell c, const asr_att_infer* f, int* steps_issued,
                          asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_TRY(dec_check(h, a, false, c));
  if (!f || !f->W_av || !f->W_out || !f->embedding || !f->live || !f->av_all || !f->logits_all || !f->ids_all ||
      !f->live_count || f->C2 < 1 || f->eos < 0 || f->live != a->live || a->dmask)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_infer: bad arguments");
  const int B = a->B, U = a->U, E2 = a->E2, Em = a->Em, To = a->To, C2 = f->C2;
  const int Din = Em + E2 + U, Dav = U + E2;
  hipStream_t st = (hipStream_t)s;
  if (hipMemsetAsync(f->live_count + 1, 0, (size_t)To * sizeof(int32_t), st) != hipSuccess)
    ASR_FAIL(h, ASR_ERR_HIP, "asr_att_decoder_infer: memset");
  EarlyExit early;                                         // on the count of live rows
  if (!early.begin((f->host_live_count && f->check_every > 0) ? f->check_every : 0))
    ASR_FAIL(h, ASR_ERR_HIP, "asr_att_decoder_infer: event");
  int k = 0;                                               // steps issued; on an error, the step that failed
  const int rc = [&]() -> int {
    ASR_TRY(dec_cell_image(h, a, c, s));
    for (; k < To; ++k) {
      int erc = ASR_OK;
      if (early.check(k, f->live_count, f->host_live_count, st, &erc)) return erc;
      const bool more = k + 1 < To;
      // (saved-activation arrays the backward would need are reused every step: index 0)
      ASR_TRY(dec_fwd_step(h, a, c, k, 0, more, s));
      float* lg = f->logits_all + (size_t)k * B * C2;
      ASR_TRY(dec_head_step(h, a, f, B, a->av_in + (size_t)k * B * Dav, f->av_all + (size_t)k * B * U, lg, s));
      hipLaunchKernelGGL(att_infer_select_kernel, dim3(B), dim3(256), 0, st, lg, C2, f->eos, f->live + (size_t)k * B,
                         f->live + (size_t)(k + 1) * B, f->live_count + k + 1, f->ids_all + (size_t)k * B, f->embedding, Em,
                         more ? a->dec_in + (size_t)(k + 1) * B * Din : nullptr, Din, E2);
    }
    return ASR_OK;
  }();
  if (rc != ASR_OK) ASR_FAIL(h, rc, "asr_att_decoder_infer: step %d failed", k);
  ASR_CHECK_LAUNCH(h, "asr_att_decoder_infer");
  if (steps_issued) *steps_issued = k;
  return ASR_OK;
}
extern "C" int asr_att_decoder_infer(asr_handle* h, const asr_att_decoder* a, const asr_att_infer* f, int* steps_issued,
                                     asr_stream s) {
  return dec_infer_loop(h, a, {nullptr, nullptr}, f, steps_issued, s);
}
extern "C" int asr_att_decoder_infer_gru(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, const asr_att_infer* f,
                                         int* steps_issued, asr_stream s) {
  if (!h || !g) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_infer_gru: bad arguments");
  return dec_infer_loop(h, a, {g, nullptr}, f, steps_issued, s);
}
extern "C" int asr_att_decoder_infer_stack(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk,
                                           const asr_att_infer* f, int* steps_issued, asr_stream s) {
  if (!h || !sk) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_infer_stack: bad arguments");
  return dec_infer_loop(h, a, {nullptr, sk}, f, steps_issued, s);
}

// ---------------------------------------------------------------- scheduled-sampling training loop
namespace {
// One workgroup per batch row, behind the output layer of decoder step k; every pointer is the row block of step k + 1
// except `logits` (step k).  The token step k + 1 is fed: the argmax of step k's raw logits (first maximum wins, the
// reduction of att_infer_select_kernel) where the row's draw is set and the row is still live at k + 1, the teacher's
// token otherwise -- the reduction runs only when it is used (the test is uniform over the workgroup).  The fed id goes
// to ids_n and its embedding, times the row's embedding-dropout mask, into the Em embedding columns of the next input row;
// the context and h columns of that row are the loop's.
__global__ __launch_bounds__(256) void att_ss_select_kernel(const float* __restrict__ logits, int C2,
                                                            const float* __restrict__ draw_n, const float* __restrict__ live_n,
                                                            const int32_t* __restrict__ teacher_n, int32_t* __restrict__ ids_n,
                                                            const float* __restrict__ emb, int Em,
                                                            const float* __restrict__ mask_n, float* __restrict__ dnext,
                                                            int Din) {
  const int b = blockIdx.x;
  int id = teacher_n[b];
  if (draw_n[b] != 0.f && live_n[b] != 0.f) id = argmax_first_block256(logits + (size_t)b * C2, C2);
  if (threadIdx.x == 0) ids_n[b] = id;
  float* d = dnext + (size_t)b * Din;
  const float* e = emb + (size_t)id * Em;
  if (mask_n) {
    const float* mk = mask_n + (size_t)b * Em;
    for (int j = threadIdx.x; j < Em; j += 256) d[j] = e[j] * mk[j];
  } else {
    for (int j = threadIdx.x; j < Em; j += 256) d[j] = e[j];
  }
}
}  // namespace

extern "C" int asr_att_decoder_fwd_ss(asr_handle* h, const asr_att_decoder* a, const asr_att_decoder_ss* f, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  const DecCell c = {nullptr, nullptr};
  ASR_TRY(dec_check(h, a, false, c));
  if (!f || !f->W_av || !f->W_out || !f->embedding || !f->teacher_ids || !f->draw || !f->av_all || !f->logits_all ||
      !f->ids_fed || f->C2 < 1 || a->Em < 1)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_fwd_ss: bad arguments");
  const int B = a->B, U = a->U, E2 = a->E2, Em = a->Em, To = a->To, C2 = f->C2;
  const int Din = Em + E2 + U, Dav = U + E2;
  ASR_TRY(dec_cell_image(h, a, c, s));
  for (int k = 0; k < To; ++k) {
    const bool more = k + 1 < To;
    ASR_TRY(dec_fwd_step(h, a, c, k, k, more, s));
    float* lg = f->logits_all + (size_t)k * B * C2;
    ASR_TRY(dec_head_step(h, a, f, B, a->av_in + (size_t)k * B * Dav, f->av_all + (size_t)k * B * U, lg, s));
    if (!more) break;
    const size_t n = (size_t)(k + 1) * B;
    hipLaunchKernelGGL(att_ss_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)s, lg, C2, f->draw + n, a->live + n,
                       f->teacher_ids + n, f->ids_fed + n, f->embedding, Em, f->emb_mask ? f->emb_mask + n * Em : nullptr,
                       a->dec_in + n * Din, Din);
  }
  ASR_CHECK_LAUNCH(h, "asr_att_decoder_fwd_ss");
  return ASR_OK;
}

// ---------------------------------------------------------------- beam search loop
// BeamSearchDecoder.step under dynamic_decode (beam_search/beam_search_decoder.py:173-231) and finalize (:125-150).  The
// loop carries one step of state: block 0 of dec_in / c_all / h_all is what a step reads, block 1 takes its raw
// outputs, and the reorder kernel gathers block 1 back into block 0 by parent -- so every step is dec_fwd_step at
// k = 0 with a next row, the very launches asr_att_decoder_infer issues, and the carried attention weights are the
// `alpha_zero` of that step.  Early exit: EarlyExit on the count of unfinished slots.
// j != nullptr: the joint CTC / attention search (asr_att_decoder_beam_joint) -- the selection is
// asr_att_beam_select_joint on the prefix state of block k & 1 of j->r / j->last, and asr_ctc_prefix_advance writes the
// other block from the parents'.  Without j the calls are those this loop has always issued.
// lm != nullptr: shallow fusion with a language model (asr_att_decoder_beam_lm, lm_fusion.hip) -- asr_lm_step behind the
// head, asr_att_beam_select_fused as the selection (with or without j; a j whose ctc_weight is not in (0, 1] is refused:
// the fused rank kernel would leave its `last` block unwritten), asr_lm_beam_reorder at the end of the step.  Only the
// selection differs between the three searches; the state advance and the re-ordering behind it are shared.  Without lm
// nothing of this is issued.
// c.g (asr_att_decoder_beam_gru): the GRU cell in the step; a->c_all is then a block of zeros the re-ordering gathers as
// it always has.  c.sk (asr_att_decoder_beam_stack): the upper layers' rows are re-ordered behind layer 0's.
static int att_beam_loop(asr_handle* h, const asr_att_decoder* a_, DecCell c, const asr_att_infer* f, const asr_att_beam* m,
                         const asr_att_beam_ctc* j, const asr_att_lm* lm, int* steps_issued, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  const asr_att_gru* g = c.g;
  const asr_att_stack* sk = c.sk;
  const char* who = sk ? "asr_att_decoder_beam_stack" : g ? "asr_att_decoder_beam_gru" : lm ? "asr_att_decoder_beam_lm" : j ? "asr_att_decoder_beam_joint" : "asr_att_decoder_beam";
  if (!a_ || !m) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: bad arguments", who);
  asr_att_decoder carried = *a_;                           // the caller's block with the loop's carried alpha in it
  if (carried.carry_alpha) carried.alpha_zero = m->alpha_prev;
  const asr_att_decoder* a = &carried;
  ASR_TRY(dec_check(h, a, false, c));
  if (g && !a->c_all) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: c_all (zeros [2,R,U]) is needed by the re-ordering", who);
  if (!f || !f->W_av || !f->W_out || !f->embedding || f->C2 < 1 || f->eos < 0 || f->eos >= f->C2 || a->dmask || m->W < 1 ||
      m->W > 32 || m->W > f->C2 || a->B % m->W != 0 || !m->word || !m->parent || !m->score || !m->log_probs || !m->finished ||
      !m->lengths || !m->av || !m->logits || !m->unfinished || !m->ids || !m->hyp_len || !m->final_score ||
      (a->carry_alpha && !m->alpha_prev))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: bad arguments", who);
  const int R = a->B, W = m->W, Bu = R / W, U = a->U, E2 = a->E2, Em = a->Em, To = a->To, C2 = f->C2, T = a->T;
  const int Din = Em + E2 + U;
  hipStream_t st = (hipStream_t)s;
  if (lm) {
    if (lm->R != R || lm->C2 != C2 || f->eos != C2 - 1 || C2 < 3 || W > C2 - 1 || !lm->lm_score || !lm->cand ||
        !lm->cand_total || !lm->cand_lm || !(lm->lm_weight > 0.f) || (j && !(j->ctc_weight > 0.f && j->ctc_weight <= 1.f)))
      ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: bad arguments (the language model part)", who);
    ASR_TRY(asr_lm_prep(h, lm, s));
  }
  if (j) {
    if (!j->y || !j->seq_len || !j->r || !j->last || !j->ctc_score || !j->cand || !j->cand_total || !j->psi ||
        C2 != j->n_labels + 2 || f->eos != j->n_labels + 1)
      ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: bad arguments (the CTC part)", who);
    ASR_TRY(asr_ctc_prefix_init(h, j->y, j->seq_len, Bu, W, T, j->By, j->Cc, j->blank, j->r, j->last, j->ctc_score, s));
  }
  if (hipMemsetAsync(m->unfinished, 0, (size_t)(To + 1) * sizeof(int32_t), st) != hipSuccess)
    ASR_FAIL(h, ASR_ERR_HIP, "%s: memset", who);
  EarlyExit early;
  if (!early.begin((f->host_live_count && f->check_every > 0) ? f->check_every : 0))
    ASR_FAIL(h, ASR_ERR_HIP, "%s: event", who);
  float* din1 = a->dec_in + (size_t)R * Din;
  float* c1 = a->c_all + (size_t)R * U;
  float* h1 = a->h_all + (size_t)R * U;
  ASR_TRY(dec_cell_image(h, a, c, s));
  int k = 0;
  for (; k < To; ++k) {
    int rc = ASR_OK;
    if (early.check(k, m->unfinished, f->host_live_count, st, &rc)) {
      if (rc != ASR_OK) return rc;
      break;
    }
    ASR_TRY(dec_fwd_step(h, a, c, 0, 0, true, s));         // (a failing call has set the message)
    ASR_TRY(dec_head_step(h, a, f, R, a->av_in, m->av, m->logits, s));
    const size_t o = (size_t)k * R;
    // the prefix state of this step and the next (j): blocks k & 1 and (k + 1) & 1
    const size_t rblk = (size_t)R * 2 * T;
    float* r_cur = j ? j->r + (size_t)(k & 1) * rblk : nullptr;
    float* r_nxt = j ? j->r + (size_t)((k + 1) & 1) * rblk : nullptr;
    int32_t* last_cur = j ? j->last + (size_t)(k & 1) * R : nullptr;
    int32_t* last_nxt = j ? j->last + (size_t)((k + 1) & 1) * R : nullptr;
    // the selection: fused with the language model's step in front of it, joint, or attention alone
    if (lm) {
      ASR_TRY(asr_lm_step(h, lm, s));
      ASR_TRY(asr_att_beam_select_fused(h, m->logits, lm->lm_logits, Bu, W, C2 - 2, m->length_penalty_weight,
                                        j ? j->ctc_weight : 0.f, lm->lm_weight, k == 0, j ? j->y : nullptr,
                                        j ? j->seq_len : nullptr, T, j ? j->By : 0, j ? j->Cc : 0, j ? j->blank : 0, r_cur,
                                        m->log_probs, m->finished, m->lengths, last_cur, j ? j->ctc_score : nullptr,
                                        lm->lm_score, lm->cand, lm->cand_total, lm->cand_lm, j ? j->psi : nullptr,
                                        m->word + o, m->parent + o, m->score + o, m->log_probs, m->finished, m->lengths,
                                        last_nxt, j ? j->ctc_score : nullptr, lm->lm_score, m->unfinished + k + 1, s));
    } else if (j) {
      ASR_TRY(asr_att_beam_select_joint(h, m->logits, Bu, W, j->n_labels, m->length_penalty_weight, j->ctc_weight, k == 0,
                                        j->y, j->seq_len, T, j->By, j->Cc, j->blank, r_cur, m->log_probs, m->finished,
                                        m->lengths, last_cur, j->ctc_score, j->cand, j->cand_total, j->psi, m->word + o,
                                        m->parent + o, m->score + o, m->log_probs, m->finished, m->lengths, last_nxt,
                                        j->ctc_score, m->unfinished + k + 1, s));
    } else {
      ASR_TRY(asr_att_beam_select(h, m->logits, Bu, W, C2, f->eos, m->length_penalty_weight, k == 0, m->log_probs,
                                  m->finished, m->lengths, m->word + o, m->parent + o, m->score + o, m->log_probs,
                                  m->finished, m->lengths, m->unfinished + k + 1, s));
    }
    // what the next step reads: the prefix state of the winners (j), the decoder's rows, the language model's rows (lm)
    if (j)
      ASR_TRY(asr_ctc_prefix_advance(h, j->y, j->seq_len, Bu, W, T, j->By, j->Cc, j->blank, j->n_labels, r_cur, last_cur,
                                     m->parent + o, m->word + o, r_nxt, s));
    ASR_TRY(asr_att_beam_reorder(h, m->parent + o, m->word + o, Bu, W, U, Em, E2, a->carry_alpha ? T : 0, C2, c1, h1, din1,
                                 a->carry_alpha ? a->alpha_all : nullptr, f->embedding, a->c_all, a->h_all, a->dec_in,
                                 a->carry_alpha ? m->alpha_prev : nullptr, s));
    if (sk) ASR_TRY(asr_att_stack_reorder(h, sk, m->parent + o, Bu, W, U, s));   // the upper layers' rows
    if (lm) {
      const size_t lblk = (size_t)lm->L * R * lm->H;       // block 1 (the step's new state) -> block 0
      ASR_TRY(asr_lm_beam_reorder(h, m->parent + o, m->word + o, Bu, W, lm->L, lm->H, lm->Em_lm, C2, lm->c + lblk,
                                  lm->h + lblk, lm->emb, lm->c, lm->h, lm->in, s));
    }
  }
  if (k < 1) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: no step issued", who);
  ASR_TRY(asr_att_beam_backtrace(h, m->word, m->parent, m->score, k, To, Bu, W, f->eos, m->ids, m->hyp_len, m->final_score, s));
  if (steps_issued) *steps_issued = k;
  return ASR_OK;
}

extern "C" int asr_att_decoder_beam(asr_handle* h, const asr_att_decoder* a, const asr_att_infer* f, const asr_att_beam* m,
                                    int* steps_issued, asr_stream s) {
  return att_beam_loop(h, a, {nullptr, nullptr}, f, m, nullptr, nullptr, steps_issued, s);
}
extern "C" int asr_att_decoder_beam_joint(asr_handle* h, const asr_att_decoder* a, const asr_att_infer* f, const asr_att_beam* m,
                                          const asr_att_beam_ctc* j, int* steps_issued, asr_stream s) {
  if (!h || !j) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_beam_joint: bad arguments");
  return att_beam_loop(h, a, {nullptr, nullptr}, f, m, j, nullptr, steps_issued, s);
}
extern "C" int asr_att_decoder_beam_lm(asr_handle* h, const asr_att_decoder* a, const asr_att_infer* f, const asr_att_beam* m,
                                       const asr_att_beam_ctc* j, const asr_att_lm* lm, int* steps_issued, asr_stream s) {
  if (!h || !lm) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_beam_lm: bad arguments");
  return att_beam_loop(h, a, {nullptr, nullptr}, f, m, j, lm, steps_issued, s);
}
extern "C" int asr_att_decoder_beam_gru(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, const asr_att_infer* f,
                                        const asr_att_beam* m, int* steps_issued, asr_stream s) {
  if (!h || !g) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_beam_gru: bad arguments");
  return att_beam_loop(h, a, {g, nullptr}, f, m, nullptr, nullptr, steps_issued, s);
}
extern "C" int asr_att_decoder_beam_stack(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk,
                                          const asr_att_infer* f, const asr_att_beam* m, int* steps_issued, asr_stream s) {
  if (!h || !sk) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_beam_stack: bad arguments");
  return att_beam_loop(h, a, {nullptr, sk}, f, m, nullptr, nullptr, steps_issued, s);
}

// c.g (asr_att_decoder_bwd_gru): the cell backward and the cell-input product of a step are the GRU's
// (asr_gru_dec_bwd_step); the query-FC backward in front of them is the unfused branch's.
// c.sk (asr_att_decoder_bwd_stack): the cell backward of a step is the TOP layer's; behind it, per lower layer, the dx
// product of the layer above with that layer's cell backward (asr_stack_dec_bwd_lower), down to layer 0, whose own
// cell-input product follows as ever.
static int dec_bwd_loop(asr_handle* h, const asr_att_decoder* a, DecCell c, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_TRY(dec_check(h, a, true, c));
  const asr_att_gru* g = c.g;
  const asr_att_stack* sk = c.sk;
  const int B = a->B, U = a->U, T = a->T, E2 = a->E2, Em = a->Em, A = a->A, To = a->To;
  const int Din = Em + E2 + U;
  hipStream_t st = (hipStream_t)s;
  // work: dc / carried-dh state (two buffers each, ping-pong), denergy, dalpha_prev x2
  float* dcs[2] = {a->work, a->work + (size_t)B * U};
  float* dhc[2] = {a->work + (size_t)2 * B * U, a->work + (size_t)3 * B * U};
  float* dalp[2] = {a->work + (size_t)4 * B * U, a->work + (size_t)4 * B * U + (size_t)B * T};
  float* denergy = dalp[1] + (size_t)B * T;
  if (hipMemsetAsync(dcs[0], 0, (size_t)B * U * sizeof(float), st) != hipSuccess ||
      hipMemsetAsync(dhc[0], 0, (size_t)B * U * sizeof(float), st) != hipSuccess)
    ASR_FAIL(h, ASR_ERR_HIP, "asr_att_decoder_bwd: memset");
  // the bf16 images of W_cell are written again here (one launch per loop): the call does not depend on the forward
  // loop having run with the same work space
  const bool cell_h = !g && dec_cell_gemm_h(a);
  if (g) ASR_TRY(asr_gru_dec_image(h, a, g, s));
  if (sk) ASR_TRY(asr_stack_dec_bwd_begin(h, a, sk, s));
  if (cell_h) ASR_TRY(asr_lstm_cell_gemm_prep_h(h, a->W_cell, a->b_cell, Din, U, a->W_cell_h, s));
  int cur = 0;
  const float* dalpha_next = nullptr;
  for (int k = To - 1; k >= 0; --k) {
    // d loss / d ctx_k = attentional-vector part + the context columns of step k+1's cell-input gradient; the sum is
    // formed inside the d-alpha kernel (and kept in dctx_all for the d_enc contraction after the loop)
    float* dctx = a->dctx_all + (size_t)k * B * E2;
    const float* dav_ctx = a->dav_ctx + (size_t)k * B * E2;
    const float* d_in_next = (k + 1 < To) ? a->d_in_all + (size_t)(k + 1) * B * Din : nullptr;
    const float* alpha_k = a->alpha_all + (size_t)k * B * T;
    const float* qz = a->qz_all + (size_t)k * B * A;
    float* dqz = a->dqz_all + (size_t)k * B * A;
    float* dv = a->dv_all ? a->dv_all + (size_t)k * B * A : nullptr;
    // the softmax backward is folded into the energy backward when both sides run their vectorised kernels
    SoftmaxBwdFold fold = {nullptr, nullptr, nullptr, nullptr, 0, 0.f};
    SoftmaxBwdFold* fp = (!a->carry_alpha && energy_vec_shape(A, a->keys, qz, a->v, a->dkeys)) ? &fold : nullptr;
    const float* snorm = a->snorm_all ? a->snorm_all + (size_t)k * B : nullptr;
    if (d_in_next) {
      ASR_TRY(softmax_ctx_bwd_launch(h, dav_ctx, d_in_next + Em, Din, dctx, alpha_k, a->seq_len, a->sharpening, a->enc,
                                     a->enc_dtype, T, B, E2, denergy, nullptr, snorm, dalpha_next, fp, s));
    } else {
      if (hipMemcpyAsync(dctx, dav_ctx, (size_t)B * E2 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
        ASR_FAIL(h, ASR_ERR_HIP, "asr_att_decoder_bwd: copy");
      ASR_TRY(softmax_ctx_bwd_launch(h, dctx, nullptr, 0, nullptr, alpha_k, a->seq_len, a->sharpening, a->enc,
                                     a->enc_dtype, T, B, E2, denergy, nullptr, snorm, dalpha_next, fp, s));
    }
    h->att_counts[(fp && fp->da) ? ASR_ATT_BWD_SOFTMAX_FOLDED : ASR_ATT_BWD_SOFTMAX_SEPARATE] += 1;
    if (a->carry_alpha) {
      float* dap = dalp[k & 1];
      ASR_TRY(loc_energy_bwd_launch(h, denergy, k > 0 ? a->alpha_all + (size_t)(k - 1) * B * T : a->alpha_zero, a->filt,
                                    a->wfil, a->keys, qz, a->v, T, B, A, a->taps, a->dkeys, dqz, dv, a->dwfil_rows,
                                    a->dfilt_rows, dap, k != To - 1, a->seq_len, s));
      dalpha_next = dap;
    }
    float* dcell = const_cast<float*>(a->dav_cell) + (size_t)k * B * U;
    float* dpre = a->dpre_all + (size_t)k * B * 4 * U;
    float* dpeep = a->dpeep_all ? a->dpeep_all + (size_t)k * B * 3 * U : nullptr;
    const float* dh2 = d_in_next ? d_in_next + Em + E2 : nullptr;
    const float* dmask = a->dmask ? a->dmask + (size_t)k * B * U : nullptr;
    // query-FC backward + cell backward in ONE launch that also sums the energy backward's chunk partials, when the
    // shapes allow (a query FC over A = 64 / 128 / 256 / 512 columns, U % 16 == 0, 16-byte aligned rows, no carried alpha)
    const bool fused_q = !g && !a->carry_alpha && a->has_query_fc && (A == 64 || A == 128 || A == 256 || A == 512) && U % DQ_CT == 0 &&
                         a->ld_wq % 4 == 0 && ((uintptr_t)a->W_q) % 16 == 0 && ((uintptr_t)dqz) % 16 == 0 &&
                         (!dv || ((uintptr_t)dv) % 16 == 0);
    h->att_counts[fused_q ? ASR_ATT_BWD_STEP_FUSED_Q : ASR_ATT_BWD_STEP_UNFUSED] += 1;
    // layer 0's cell backward (the only one without a stack)
    const CellBwdArgs ca0 = {dcs[cur], dhc[cur], dh2, a->gates_all + (size_t)k * B * 4 * U, a->craw_all + (size_t)k * B * U,
                             a->c_all + (size_t)k * B * U, a->peep, a->live + (size_t)k * B, dmask,
                             dpre, dcs[cur ^ 1], dhc[cur ^ 1], dpeep, Din, 0.f};   // (clip: see the unfused call below)
    if (fused_q) {
      const float* part = nullptr;
      int nchq = 0;
      ASR_TRY(energy_bwd_launch(h, denergy, a->keys, qz, a->v, T, B, A, a->att_mode, a->dkeys, dqz, dv, a->seq_len, fp, s,
                                &part, &nchq));
      ASR_TRY(att_dq_cell_bwd_launch(h, part, nchq, B, A, U, a->W_q, a->ld_wq, dcell, dqz, dv,
                                     sk ? asr_stack_cell_args(a, sk, sk->L - 1, k, cur) : ca0, s));
    } else {
      if (!a->carry_alpha)
        ASR_TRY(energy_bwd_launch(h, denergy, a->keys, qz, a->v, T, B, A, a->att_mode, a->dkeys, dqz, dv, a->seq_len, fp, s));
      if (a->has_query_fc)
        ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 1, B, U, A, dqz, A, a->W_q, a->ld_wq, dcell, U, nullptr, 1, 0, s));
      else
        ASR_TRY(asr_add_cols(h, dcell, U, dqz, A, dcell, U, B, U, s));
      if (g) {       // (mask and the h-columns of step k+1's cell-input gradient are folded in as below; dcs is its work space)
        ASR_TRY(asr_gru_dec_bwd_step(h, a, g, k, dcell, dhc[cur], dh2, dhc[cur ^ 1], dcs[0], s));
        cur ^= 1;
        continue;
      }
      // the cell kernel applies the output dropout mask to dcell and adds the h-columns of step k+1's cell-input
      // gradient to the carried dh itself
      // (clip 0: the decoder cell is tf.contrib.rnn.LSTMBlockCell (attention_seq2seq.py:354-365), whose gradient op
      // ignores cell_clip: the clamp is straight-through here)
      ASR_TRY(asr_lstm_cell_bwd_args(h, dcell, sk ? asr_stack_cell_args(a, sk, sk->L - 1, k, cur) : ca0, B, U, s));
    }
    if (sk)                                // down the stack: dx of layer l + 1 and the cell backward of layer l, l = L-2 .. 0
      for (int l = sk->L - 2; l >= 0; --l)
        ASR_TRY(asr_stack_dec_bwd_lower(h, a, sk, l, k, l ? asr_stack_cell_args(a, sk, l, k, cur) : ca0, s));
    float* d_in = a->d_in_all + (size_t)k * B * Din;
    h->att_counts[cell_h ? ASR_ATT_BWD_CELL_BF16 : ASR_ATT_BWD_CELL_GEMM] += 1;
    if (cell_h) ASR_TRY(asr_lstm_cell_gemm_bwd_h(h, dpre, B, Din, U, a->W_cell_h, d_in, Din, s));   // bf16 weight rows
    else ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 1, B, Din, 4 * U, dpre, 4 * U, a->W_cell, 4 * U, d_in, Din, nullptr, 0, 0, s));
    cur ^= 1;
  }
  ASR_TRY(asr_add_cols(h, dhc[cur], U, a->d_in_all + Em + E2, Din, a->dh0, U, B, U, s));
  if (sk) ASR_TRY(asr_stack_dec_bwd_end(h, a, sk, cur, s));
  if (g) return ASR_OK;                                    // (no cell state, no dc0)
  if (hipMemcpyAsync(a->dc0, dcs[cur], (size_t)B * U * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
    ASR_FAIL(h, ASR_ERR_HIP, "asr_att_decoder_bwd: copy");
  return ASR_OK;
}

extern "C" int asr_att_decoder_bwd(asr_handle* h, const asr_att_decoder* a, asr_stream s) {
  return dec_bwd_loop(h, a, {nullptr, nullptr}, s);
}
extern "C" int asr_att_decoder_bwd_gru(asr_handle* h, const asr_att_decoder* a, const asr_att_gru* g, asr_stream s) {
  if (!h || !g) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_bwd_gru: bad arguments");
  return dec_bwd_loop(h, a, {g, nullptr}, s);
}
extern "C" int asr_att_decoder_bwd_stack(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, asr_stream s) {
  if (!h || !sk) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_att_decoder_bwd_stack: bad arguments");
  return dec_bwd_loop(h, a, {nullptr, sk}, s);
}
