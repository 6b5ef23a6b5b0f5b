// Shallow fusion of an RNN language model into the attention beam search (Hori et al. 2017; an EXTENSION -- the reference's
// models/lm/ classes raise NotImplementedError and its decoders carry `# TODO: add LM score here`,
// models/ctc/decoders/beam_search_decoder.py:132): the language model -- one LM step on the beam's rows and the re-ordering of
// the LM state.  The selection over the attention, LM and (for joint models) CTC prefix scores is asr_att_beam_select_fused
// (att_beam.hip).  The float64 statement is models/attention/decoders/beam_search/lm_fusion.py; the loop that issues these
// is asr_att_decoder_beam_lm (dec_loop.hip, the beam search loop).  The LM step has no recurrence kernel of its own: it
// runs the decoder cell's entries.
#include "common.h"
#include <math.h>

namespace {

constexpr int FUSED_MAX_W = 32;

// One workgroup per row r = b*W + w: the LM state the next step reads is the parent's (the LM has consumed the parent's last
// word; the chosen word is the next step's input).  Per layer l: c_dst / h_dst [l, r] = c_src / h_src [l, b*W + parent[r]],
// and the same h row into the h_prev columns of the layer's cell-input rows; layer 0's x columns = emb[word[r]].  Out of
// place: several children may read one parent row.
__global__ __launch_bounds__(256) void lm_beam_reorder_kernel(
    const int32_t* __restrict__ parent, const int32_t* __restrict__ word, int R, int W, int L, int H, int Em, int vocab,
    const float* __restrict__ c_src, const float* __restrict__ h_src, const float* __restrict__ emb, float* __restrict__ c_dst,
    float* __restrict__ h_dst, float* __restrict__ in_dst) {
  const int r = blockIdx.x, tid = threadIdx.x;
  int pa = parent[r], wd = word[r];
  pa = pa < 0 ? 0 : (pa >= W ? W - 1 : pa);                 // (never out of range from the select kernel: bounds only)
  wd = wd < 0 ? 0 : (wd >= vocab ? vocab - 1 : wd);
  const size_t pr = (size_t)(r / W) * W + pa;
  for (int l = 0; l < L; ++l) {
    const size_t lo = (size_t)l * R * H;
    // layer 0 rows are Em + H wide, the others 2H; the layers lie one behind the other
    const int xw = l == 0 ? Em : H;
    float* in_row = in_dst + (l == 0 ? (size_t)0 : (size_t)R * (Em + H) + (size_t)(l - 1) * R * 2 * H) + (size_t)r * (xw + H);
    for (int j = tid; j < H; j += 256) {
      const float hv = h_src[lo + pr * H + j];
      c_dst[lo + (size_t)r * H + j] = c_src[lo + pr * H + j];
      h_dst[lo + (size_t)r * H + j] = hv;
      in_row[xw + j] = hv;
    }
    if (l == 0)
      for (int j = tid; j < Em; j += 256) in_row[j] = emb[(size_t)wd * Em + j];
  }
}

}  // namespace

static int lm_check(asr_handle* h, const asr_att_lm* lm, const char* who) {
  if (!lm || lm->L < 1 || lm->H < 1 || lm->Em_lm < 1 || lm->R < 1 || lm->C2 < 1 || !lm->emb || !lm->W || !lm->b || !lm->W_out ||
      !lm->c || !lm->h || !lm->in || !lm->live || !lm->work || !lm->lm_logits || !(lm->cell_clip >= 0.f))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: bad arguments (the language model)", who);
  return ASR_OK;
}

// layer l: width of x, offset of its kernel in W, of its image in W_il, of its rows in `in`
static inline int lm_xw(const asr_att_lm* lm, int l) { return l == 0 ? lm->Em_lm : lm->H; }
static inline size_t lm_w_off(const asr_att_lm* lm, int l) {
  return l == 0 ? 0 : ((size_t)(lm->Em_lm + lm->H) + (size_t)(l - 1) * 2 * lm->H) * 4 * lm->H;
}
static inline size_t lm_il_off(const asr_att_lm* lm, int l) {
  return l == 0 ? 0 : ((size_t)(lm->Em_lm + lm->H + 1) + (size_t)(l - 1) * (2 * lm->H + 1)) * 4 * lm->H;
}
static inline size_t lm_in_off(const asr_att_lm* lm, int l) {
  return l == 0 ? 0 : (size_t)lm->R * (lm->Em_lm + lm->H) + (size_t)(l - 1) * lm->R * 2 * lm->H;
}
static inline bool lm_layer_fused(const asr_att_lm* lm, int l) {
  const int K = lm_xw(lm, l) + lm->H;
  return lm->W_il && asr_lstm_cell_gemm_ok(lm->R, K, lm->H, K) && ((uintptr_t)(lm->in + lm_in_off(lm, l))) % 16 == 0 &&
         ((uintptr_t)(lm->W_il + lm_il_off(lm, l))) % 16 == 0;
}

extern "C" int asr_lm_prep(asr_handle* h, const asr_att_lm* lm, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_TRY(lm_check(h, lm, "asr_lm_prep"));
  for (int l = 0; l < lm->L; ++l)
    if (lm_layer_fused(lm, l))
      ASR_TRY(asr_lstm_cell_gemm_prep(h, lm->W + lm_w_off(lm, l), lm->b + (size_t)l * 4 * lm->H, lm_xw(lm, l) + lm->H, lm->H,
                                      lm->W_il + lm_il_off(lm, l), s));
  return ASR_OK;
}

extern "C" int asr_lm_step(asr_handle* h, const asr_att_lm* lm, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_TRY(lm_check(h, lm, "asr_lm_step"));
  const int R = lm->R, H = lm->H, L = lm->L;
  const size_t blk = (size_t)L * R * H;
  float* pre = lm->work;                                     // [R,4H]
  float* gates = pre + (size_t)R * 4 * H;                    // [R,4H]
  float* craw = gates + (size_t)R * 4 * H;                   // [R,H]
  float* hraw = craw + (size_t)R * H;                        // [R,H]
  h->att_lm_counts[0] += 1;
  for (int l = 0; l < L; ++l) {
    const int K = lm_xw(lm, l) + H;
    float* x = lm->in + lm_in_off(lm, l);
    const float* cp = lm->c + (size_t)l * R * H;
    const float* hp = lm->h + (size_t)l * R * H;
    float* cn = lm->c + blk + (size_t)l * R * H;
    float* hn = lm->h + blk + (size_t)l * R * H;
    // the layer's output is the next layer's x: written there by the cell itself
    float* nx = l + 1 < L ? lm->in + lm_in_off(lm, l + 1) : nullptr;
    if (lm_layer_fused(lm, l)) {
      h->att_counts[ASR_ATT_FWD_CELL_F32IMG] += 1;
      ASR_TRY(asr_lstm_cell_gemm_fwd(h, x, K, K, lm->W_il + lm_il_off(lm, l), 1, cp, hp, nullptr, lm->live, R, H, 1.f,
                                     lm->cell_clip, gates, craw, cn, hn, hraw, nullptr, nullptr, nullptr, 0, nx, 2 * H, s));
    } else {
      h->att_counts[ASR_ATT_FWD_CELL_GEMM] += 1;
      ASR_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, R, 4 * H, K, x, K, lm->W + lm_w_off(lm, l), 4 * H, pre, 4 * H,
                           lm->b + (size_t)l * 4 * H, 0, 0, s));
      ASR_TRY(asr_lstm_cell_fwd_ex(h, pre, cp, hp, nullptr, lm->live, R, H, 1.f, lm->cell_clip, gates, craw, cn, hn, hraw,
                                   nullptr, nullptr, nullptr, 0, nx, 2 * H, s));
    }
  }
  return asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, R, lm->C2, H, lm->h + blk + (size_t)(L - 1) * R * H, H, lm->W_out, lm->C2,
                      lm->lm_logits, lm->C2, lm->b_out, 0, 0, s);
}

extern "C" int asr_lm_beam_reorder(asr_handle* h, const int32_t* parent, const int32_t* word, int B, int W, int L, int H,
                                   int Em_lm, int vocab, const float* c_src, const float* h_src, const float* emb, float* c_dst,
                                   float* h_dst, float* in_dst, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(parent && word && c_src && h_src && emb && c_dst && h_dst && in_dst, "asr_lm_beam_reorder: null");
  ASR_NEED(B >= 1 && W >= 1 && W <= FUSED_MAX_W && L >= 1 && H >= 1 && Em_lm >= 1 && vocab >= 1, "asr_lm_beam_reorder: bad shape");
  ASR_NEED(c_src != c_dst && h_src != h_dst, "asr_lm_beam_reorder: the gather is out of place");
  h->att_lm_counts[2] += 1;
  hipLaunchKernelGGL(lm_beam_reorder_kernel, dim3(B * W), dim3(256), 0, (hipStream_t)s, parent, word, B * W, W, L, H, Em_lm,
                     vocab, c_src, h_src, emb, c_dst, h_dst, in_dst);
  ASR_CHECK_LAUNCH(h, "asr_lm_beam_reorder");
  return ASR_OK;
}

ASR_DEFINE_COUNTS(att_lm_counts, att_lm_counts)
