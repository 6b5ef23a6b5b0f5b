// Shallow fusion of an RNN language model into the attention beam search (Hori et al. 2017; an EXTENSION -- the reference's
// models/lm/ classes raise NotImplementedError and its decoders carry `# TODO: add LM score here`,
// models/ctc/decoders/beam_search_decoder.py:132): one LM step on the beam's rows, the selection over the attention, LM and
// (for joint models) CTC prefix scores, and the re-ordering of the LM state.  The float64 statement is
// models/attention/decoders/beam_search/lm_fusion.py; the loop that issues these is asr_att_decoder_beam_lm (attention.hip,
// the beam search loop).  The LM step has no recurrence kernel of its own: it runs the decoder cell's entries.
#include "common.h"
#include <math.h>

namespace {

constexpr int FUSED_MAX_W = 32;
constexpr int FUSED_CAND = FUSED_MAX_W * (FUSED_MAX_W + 1);

// (value, index) order of tf.nn.top_k, as att_beam.hip
__device__ __forceinline__ bool fused_before(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

// max + log(sum exp(x - max)) of a row, in the order of att_beam_select_kernel: lane l takes the columns l, l + 64, ... in
// ascending order into a running maximum / sum, the 64 partials meet in a butterfly (xor 32 .. 1).
__device__ __forceinline__ float row_lse(const float* __restrict__ x, int C2, int lane) {
  float m = -INFINITY;
  for (int c = lane; c < C2; c += 64) m = fmaxf(m, x[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float sum = 0.f;
  for (int c = lane; c < C2; c += 64) sum += expf(x[c] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  return m + logf(sum);
}

// Fused selection, stage 1: one wave per slot row.  Both rows of logits are read here and nowhere else (no log-softmax
// pass over lm_logits): lse_att, lse_lm (row_lse), local[c] = (x[c] - lse_att) + mu * (z[c] - lse_lm), the row's W best
// classes other than <EOS> by local (ties by lower index; one per round, the best that comes after the previous one, as
// att_joint_candidates_kernel) and <EOS>.  cand [R, W+1] (-1: no candidate), total = log_probs + (x[c] - lse_att),
// lmt = lm_score + (z[c] - lse_lm).  A finished row has its <EOS> alone (p_att = p_lm = 0); at the first step only slot 0
// has candidates.
__global__ __launch_bounds__(64) void att_fused_candidates_kernel(
    const float* __restrict__ logits, const float* __restrict__ lm_logits, int W, int C2, int eos, float mu, int first_step,
    const float* __restrict__ lp_in, const int32_t* __restrict__ fin_in, const float* __restrict__ lm_in,
    int32_t* __restrict__ cand, float* __restrict__ total, float* __restrict__ lmt) {
  const int row = blockIdx.x, lane = threadIdx.x, w = row % W;
  int my_c = -1;                                             // lane j <= W keeps candidate j and writes it at the end
  float my_tot = -INFINITY, my_lm = -INFINITY;
  const float lp = lp_in[row], ls = lm_in[row];
  if (first_step && w > 0) {                                 // (wave-uniform) every slot holds the same hypothesis
  } else if (fin_in[row] != 0) {
    if (lane == W) { my_c = eos; my_tot = lp + 0.f; my_lm = ls + 0.f; }
  } else {
    const float* x = logits + (size_t)row * C2;
    const float* z = lm_logits + (size_t)row * C2;
    const float lse_a = row_lse(x, C2, lane);
    const float lse_l = row_lse(z, C2, lane);
    float pv = INFINITY;
    int pi = -1;
    for (int j = 0; j < W; ++j) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int c = lane; c < C2; c += 64) {
        const float v = (x[c] - lse_a) + mu * (z[c] - lse_l);
        if (c != eos && fused_before(pv, pi, v, c) && fused_before(v, c, bv, bi)) { bv = v; bi = c; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (fused_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      if (bi == 0x7fffffff) break;                           // (wave-uniform) fewer than W other classes, or NaNs
      if (lane == j) { my_c = bi; my_tot = lp + (x[bi] - lse_a); my_lm = ls + (z[bi] - lse_l); }
      pv = bv; pi = bi;
    }
    if (lane == W) { my_c = eos; my_tot = lp + (x[eos] - lse_a); my_lm = ls + (z[eos] - lse_l); }
  }
  if (lane <= W) {
    const bool ok = my_c >= 0 && my_tot == my_tot && my_lm == my_lm;          // (no NaN takes a place)
    const size_t o = (size_t)row * (W + 1) + lane;
    cand[o] = ok ? my_c : -1;
    total[o] = ok ? my_tot : -INFINITY;
    lmt[o] = ok ? my_lm : -INFINITY;
  }
}

// Fused selection, stage 3 (stage 2, with CTC, is ctc_prefix_score_kernel on cand): one workgroup per utterance,
// att_joint_rank_kernel with the LM term.  fused = (1 - lam) * total [+ lam * ctc] + mu * lmt, added in that order (the CTC
// term only when has_ctc; without it nothing of the CTC arrays is read); score = fused / (pow(5 + len, a) / pow(6, a))
// (a == 1: fused, the quirk of normalize_score).  All *_in state is read before the first barrier: out may be in.
__global__ __launch_bounds__(256) void att_fused_rank_kernel(
    const int32_t* __restrict__ cand, const float* __restrict__ total, const float* __restrict__ lmt,
    const float* __restrict__ psi, int W, int C2, int eos, float lpw, float lam, float mu, int has_ctc, const int32_t* fin_in,
    const int32_t* len_in, const int32_t* last_in, const float* ctc_in, const float* lm_in, int32_t* __restrict__ word,
    int32_t* __restrict__ parent, float* __restrict__ score, float* lp_out, int32_t* fin_out, int32_t* len_out,
    int32_t* last_out, float* ctc_out, float* lm_out, int32_t* __restrict__ unfinished) {
  __shared__ int s_fin[FUSED_MAX_W], s_len[FUSED_MAX_W], s_last[FUSED_MAX_W];
  __shared__ float s_ctc[FUSED_MAX_W], s_lm[FUSED_MAX_W];
  __shared__ float c_score[FUSED_CAND], c_total[FUSED_CAND], c_ctc[FUSED_CAND], c_lm[FUSED_CAND];
  __shared__ int c_flat[FUSED_CAND];
  __shared__ float r_score[FUSED_MAX_W], r_total[FUSED_MAX_W], r_ctc[FUSED_MAX_W], r_lm[FUSED_MAX_W];
  __shared__ int r_flat[FUSED_MAX_W];
  __shared__ int s_live;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ncand = W * (W + 1);
  if (tid < W) {
    s_fin[tid] = fin_in[b * W + tid] != 0;
    s_len[tid] = len_in[b * W + tid];
    s_last[tid] = has_ctc ? last_in[b * W + tid] : -1;
    s_ctc[tid] = has_ctc ? ctc_in[b * W + tid] : 0.f;
    s_lm[tid] = lm_in[b * W + tid];
    r_score[tid] = -INFINITY; r_total[tid] = -INFINITY; r_ctc[tid] = -INFINITY; r_lm[tid] = -INFINITY; r_flat[tid] = -1;
  }
  if (tid == 0) s_live = 0;
  __syncthreads();
  const float pen6 = powf(6.f, lpw);
  for (int i = tid; i < ncand; i += 256) {
    const int w = i / (W + 1);
    const size_t o = (size_t)b * ncand + i;
    const int c = cand[o];
    int flat = -1;
    float sc = -INFINITY, tot = -INFINITY, ctc = has_ctc ? -INFINITY : 0.f, lm = -INFINITY;
    if (c >= 0 && c < C2) {
      tot = total[o];
      lm = lmt[o];
      float fused = (1.f - lam) * tot;
      if (has_ctc) {
        ctc = s_fin[w] ? s_ctc[w] : psi[o];
        fused = fused + lam * ctc;
      }
      fused = fused + mu * lm;
      const int len = s_len[w] + ((c != eos && !s_fin[w]) ? 1 : 0);
      sc = lpw == 1.f ? fused : fused / (powf(5.f + (float)len, lpw) / pen6);
      if (ctc != -INFINITY && sc == sc) flat = w * C2 + c;   // (sc == sc: no NaN takes a place)
    }
    c_score[i] = sc; c_total[i] = tot; c_ctc[i] = ctc; c_lm[i] = lm; c_flat[i] = flat;
  }
  __syncthreads();
  // rank of every survivor among the survivors; flat indices are distinct, so are the ranks
  for (int i = tid; i < ncand; i += 256) {
    const int fi = c_flat[i];
    if (fi < 0) continue;
    const float si = c_score[i];
    int rank = 0;
    for (int j = 0; j < ncand; ++j) {
      const int fj = c_flat[j];
      if (fj >= 0 && fused_before(c_score[j], fj, si, fi)) ++rank;
    }
    if (rank < W) { r_score[rank] = si; r_total[rank] = c_total[i]; r_ctc[rank] = c_ctc[i]; r_lm[rank] = c_lm[i]; r_flat[rank] = fi; }
  }
  __syncthreads();
  if (tid < W) {
    // (a place nothing reached -- fewer than W candidates with a finite CTC score, or NaNs -- repeats the slot as a finished
    // <EOS> that keeps the parent's ctc_score and lm_score)
    const bool hit = r_flat[tid] >= 0;
    const int flat = hit ? r_flat[tid] : tid * C2 + eos;
    const int wd = flat % C2, pa = flat / C2;
    const int fin = (s_fin[pa] || wd == eos) ? 1 : 0;
    const size_t o = (size_t)b * W + tid;
    word[o] = wd;
    parent[o] = pa;
    score[o] = r_score[tid];
    lp_out[o] = r_total[tid];
    lm_out[o] = hit ? r_lm[tid] : s_lm[pa];
    fin_out[o] = fin;
    len_out[o] = s_len[pa] + ((wd != eos && !fin) ? 1 : 0);
    if (has_ctc) {
      ctc_out[o] = hit ? r_ctc[tid] : s_ctc[pa];
      last_out[o] = wd == eos ? s_last[pa] : wd;
    }
    if (!fin) atomicAdd(&s_live, 1);
  }
  __syncthreads();
  if (tid == 0 && unfinished && s_live) atomicAdd(unfinished, s_live);
}

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

#define FUSED_NEED(cond, msg) do { if (!(cond)) ASR_FAIL(h, ASR_ERR_INVALID_ARG, msg); } while (0)
#define FUSED_TRY(call) do { const int rc_ = (call); if (rc_ != ASR_OK) return rc_; } while (0)

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
  FUSED_TRY(lm_check(h, lm, "asr_lm_prep"));
  for (int l = 0; l < lm->L; ++l)
    if (lm_layer_fused(lm, l))
      FUSED_TRY(asr_lstm_cell_gemm_prep(h, lm->W + lm_w_off(lm, l), lm->b + (size_t)l * 4 * lm->H, lm_xw(lm, l) + lm->H, lm->H,
                                        lm->W_il + lm_il_off(lm, l), s));
  return ASR_OK;
}

extern "C" int asr_lm_step(asr_handle* h, const asr_att_lm* lm, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  FUSED_TRY(lm_check(h, lm, "asr_lm_step"));
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
      FUSED_TRY(asr_lstm_cell_gemm_fwd(h, x, K, K, lm->W_il + lm_il_off(lm, l), 1, cp, hp, nullptr, lm->live, R, H, 1.f,
                                       lm->cell_clip, gates, craw, cn, hn, hraw, nullptr, nullptr, nullptr, 0, nx, 2 * H, s));
    } else {
      h->att_counts[ASR_ATT_FWD_CELL_GEMM] += 1;
      FUSED_TRY(asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, R, 4 * H, K, x, K, lm->W + lm_w_off(lm, l), 4 * H, pre, 4 * H,
                             lm->b + (size_t)l * 4 * H, 0, 0, s));
      FUSED_TRY(asr_lstm_cell_fwd_ex(h, pre, cp, hp, nullptr, lm->live, R, H, 1.f, lm->cell_clip, gates, craw, cn, hn, hraw,
                                     nullptr, nullptr, nullptr, 0, nx, 2 * H, s));
    }
  }
  return asr_gemm_act(h, ASR_F32, ASR_F32, 0, 0, R, lm->C2, H, lm->h + blk + (size_t)(L - 1) * R * H, H, lm->W_out, lm->C2,
                      lm->lm_logits, lm->C2, lm->b_out, 0, 0, s);
}

extern "C" int asr_att_beam_select_fused(asr_handle* h, const float* logits, const float* lm_logits, int B, int W, int n_labels,
                                         float lpw, float ctc_weight, float lm_weight, int first_step, const float* y,
                                         const int32_t* seq_len, int T, int By, int Cc, int blank, const float* r,
                                         const float* lp_in, const int32_t* fin_in, const int32_t* len_in,
                                         const int32_t* last_in, const float* ctc_in, const float* lm_in, int32_t* cand,
                                         float* cand_total, float* cand_lm, float* psi, int32_t* word, int32_t* parent,
                                         float* score, float* lp_out, int32_t* fin_out, int32_t* len_out, int32_t* last_out,
                                         float* ctc_out, float* lm_out, int32_t* unfinished, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  FUSED_NEED(logits && lm_logits && lp_in && fin_in && len_in && lm_in && cand && cand_total && cand_lm && word && parent &&
                 score && lp_out && fin_out && len_out && lm_out, "asr_att_beam_select_fused: null");
  FUSED_NEED(B >= 1 && n_labels >= 1 && W >= 1 && W <= FUSED_MAX_W, "asr_att_beam_select_fused: bad shape");
  FUSED_NEED(W <= n_labels + 1, "asr_att_beam_select_fused: beam width exceeds the labels and <EOS> step 0 selects among");
  FUSED_NEED(lm_weight > 0.f && lm_weight < INFINITY, "asr_att_beam_select_fused: lm_weight must be a finite number > 0");
  FUSED_NEED(ctc_weight >= 0.f && ctc_weight <= 1.f, "asr_att_beam_select_fused: ctc_weight must be in [0, 1]");
  const int has_ctc = ctc_weight > 0.f ? 1 : 0;
  if (has_ctc)
    FUSED_NEED(y && seq_len && r && last_in && ctc_in && psi && last_out && ctc_out && T >= 1 && By >= B && n_labels < Cc &&
                   blank >= n_labels && blank < Cc, "asr_att_beam_select_fused: bad arguments (the CTC part)");
  const int C2 = n_labels + 2, eos = n_labels + 1;
  FUSED_NEED((long long)W * C2 <= 0x7fffffffLL, "asr_att_beam_select_fused: flat index overflow");
  hipStream_t st = (hipStream_t)s;
  h->att_lm_counts[1] += 1;
  hipLaunchKernelGGL(att_fused_candidates_kernel, dim3(B * W), dim3(64), 0, st, logits, lm_logits, W, C2, eos, lm_weight,
                     first_step, lp_in, fin_in, lm_in, cand, cand_total, cand_lm);
  ASR_CHECK_LAUNCH(h, "asr_att_beam_select_fused(candidates)");
  if (has_ctc)
    FUSED_TRY(asr_ctc_prefix_score(h, y, seq_len, B, W, T, By, Cc, blank, n_labels, r, last_in, fin_in, cand, W + 1, psi, s));
  hipLaunchKernelGGL(att_fused_rank_kernel, dim3(B), dim3(256), 0, st, cand, cand_total, cand_lm, psi, W, C2, eos, lpw, ctc_weight,
                     lm_weight, has_ctc, fin_in, len_in, last_in, ctc_in, lm_in, word, parent, score, lp_out, fin_out, len_out,
                     last_out, ctc_out, lm_out, unfinished);
  ASR_CHECK_LAUNCH(h, "asr_att_beam_select_fused(rank)");
  return ASR_OK;
}

extern "C" int asr_lm_beam_reorder(asr_handle* h, const int32_t* parent, const int32_t* word, int B, int W, int L, int H,
                                   int Em_lm, int vocab, const float* c_src, const float* h_src, const float* emb, float* c_dst,
                                   float* h_dst, float* in_dst, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  FUSED_NEED(parent && word && c_src && h_src && emb && c_dst && h_dst && in_dst, "asr_lm_beam_reorder: null");
  FUSED_NEED(B >= 1 && W >= 1 && W <= FUSED_MAX_W && L >= 1 && H >= 1 && Em_lm >= 1 && vocab >= 1, "asr_lm_beam_reorder: bad shape");
  FUSED_NEED(c_src != c_dst && h_src != h_dst, "asr_lm_beam_reorder: the gather is out of place");
  h->att_lm_counts[2] += 1;
  hipLaunchKernelGGL(lm_beam_reorder_kernel, dim3(B * W), dim3(256), 0, (hipStream_t)s, parent, word, B * W, W, L, H, Em_lm,
                     vocab, c_src, h_src, emb, c_dst, h_dst, in_dst);
  ASR_CHECK_LAUNCH(h, "asr_lm_beam_reorder");
  return ASR_OK;
}

extern "C" int asr_att_lm_counts(asr_handle* h, unsigned long long* out3) {
  if (!h || !out3) return ASR_ERR_INVALID_ARG;
  for (int i = 0; i < 3; ++i) out3[i] = h->att_lm_counts[i];
  return ASR_OK;
}
extern "C" int asr_reset_att_lm_counts(asr_handle* h) {
  if (!h) return ASR_ERR_INVALID_ARG;
  for (int i = 0; i < 3; ++i) h->att_lm_counts[i] = 0;
  return ASR_OK;
}
