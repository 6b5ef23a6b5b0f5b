// Beam search over the attention decoder (models/attention/decoders/beam_search/ of the reference): the per-step
// selection, the re-ordering of what the next step reads, and the back-trace.  The loop that issues them is
// asr_att_decoder_beam (attention.hip, next to the greedy loop whose per-step code it shares).
#include "common.h"
#include <math.h>

namespace {

constexpr int BEAM_MAX_W = 32;
constexpr int BEAM_THREADS = 1024;                          // 16 waves: a wave per slot row (two rows each from W = 17)
constexpr int BEAM_CAND = BEAM_MAX_W * (BEAM_MAX_W + 1);    // per row: its W best other classes and <EOS>

// (value, index) order of tf.nn.top_k: larger value first, equal values by ascending index
__device__ __forceinline__ bool beam_before(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

// One workgroup per utterance: beam_search_step (beam_search_decoder.py:234-332), fp32.
//
// Pruning loses nothing.  Within a slot row every class but <EOS> has the same candidate length, hence the same positive
// divisor: scores are ordered as the logits are, and a class outside the row's W best logits (ties by lower index, the
// order the flat index gives) has W row-mates ahead of it in the utterance-wide order -- it cannot be among the W
// selected.  So per row the W best non-<EOS> logits are extracted by comparing logits (no rounding is involved in that
// choice: where fp32 rounds the scores of two different logits of a row to one value, the logits still decide) and
// <EOS> is added; the W * (W + 1) survivors are ranked against each other by (score descending, flat index
// ascending).  A finished row contributes its <EOS> alone (mask_probs gives the others float32.min, and there are
// always W finite candidates: one per slot after step 0, min(C2, W + 1) >= W in slot 0 at step 0).
//
// Reduction order (the tests' 1e-4 bound on score / log_probs counts these roundings): lane l of the row's wave takes
// the classes l, l + 64, ... in ascending order into a running maximum, the 64 maxima meet in a butterfly (xor 32, 16,
// ... 1); the sum of exp(x - max) the same way: per lane sequentially over its classes, then the butterfly.
// lse = max + log(sum); p = x - lse; total = log_probs + p; score = total / (pow(5 + len, a) / pow(6, a)).
__global__ __launch_bounds__(BEAM_THREADS) void att_beam_select_kernel(
    const float* __restrict__ logits, int W, int C2, int eos, float lpw, int first_step,
    const float* lp_in, const int32_t* fin_in, const int32_t* len_in,      // (the state may be updated in place: the
    int32_t* __restrict__ word, int32_t* __restrict__ parent,               //  *_out arrays may be the *_in arrays; all
    float* __restrict__ score, float* lp_out, int32_t* fin_out,             //  reads happen before the first barrier)
    int32_t* len_out, int32_t* __restrict__ unfinished) {
  __shared__ float s_lp[BEAM_MAX_W];
  __shared__ int s_fin[BEAM_MAX_W], s_len[BEAM_MAX_W];
  __shared__ float c_score[BEAM_CAND], c_total[BEAM_CAND];
  __shared__ int c_flat[BEAM_CAND];
  __shared__ float r_score[BEAM_MAX_W], r_total[BEAM_MAX_W];
  __shared__ int r_flat[BEAM_MAX_W];
  __shared__ int s_live;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncand = W * (W + 1);
  if (tid < W) {
    s_lp[tid] = lp_in[b * W + tid];
    s_fin[tid] = fin_in[b * W + tid] != 0;
    s_len[tid] = len_in[b * W + tid];
    r_score[tid] = -INFINITY; r_total[tid] = -INFINITY; r_flat[tid] = -1;
  }
  if (tid == 0) s_live = 0;
  for (int i = tid; i < ncand; i += BEAM_THREADS) { c_score[i] = -INFINITY; c_total[i] = -INFINITY; c_flat[i] = -1; }
  __syncthreads();
  const float pen6 = powf(6.f, lpw);
  for (int w = wave; w < W; w += BEAM_THREADS / 64) {
    if (first_step && w > 0) break;                        // (wave-uniform) every slot holds the same hypothesis
    const float lpw_ = s_lp[w];
    const int len = s_len[w];
    float* cs = c_score + w * (W + 1);
    float* ct = c_total + w * (W + 1);
    int* cf = c_flat + w * (W + 1);
    if (s_fin[w]) {                                        // all its mass on <EOS>: p = 0, the length stays
      if (lane == 0) {
        const float total = lpw_ + 0.f;
        const float sc = lpw == 1.f ? total : total / (powf(5.f + (float)len, lpw) / pen6);
        if (sc == sc) { cs[W] = sc; ct[W] = total; cf[W] = w * C2 + eos; }
      }
      continue;
    }
    const float* x = logits + ((size_t)b * W + w) * C2;
    float m = -INFINITY;
    for (int c = lane; c < C2; c += 64) m = fmaxf(m, x[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.f;
    for (int c = lane; c < C2; c += 64) sum += expf(x[c] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float lse = m + logf(sum);
    const float pen_grow = lpw == 1.f ? 1.f : powf(5.f + (float)(len + 1), lpw) / pen6;
    const float pen_stay = lpw == 1.f ? 1.f : powf(5.f + (float)len, lpw) / pen6;
    // the W best logits among the classes other than <EOS>, one per round: the best that comes after the previous one
    float pv = INFINITY;
    int pi = -1;
    for (int j = 0; j < W; ++j) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int c = lane; c < C2; c += 64) {
        const float v = x[c];
        if (c != eos && beam_before(pv, pi, v, c) && beam_before(v, c, bv, bi)) { bv = v; bi = c; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (beam_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      if (bi == 0x7fffffff) break;                         // (wave-uniform) fewer than W other classes, or NaNs
      if (lane == 0) {
        const float total = lpw_ + (bv - lse);
        const float sc = total / pen_grow;
        if (sc == sc) { cs[j] = sc; ct[j] = total; cf[j] = w * C2 + bi; }
      }
      pv = bv; pi = bi;
    }
    if (lane == 0) {
      const float total = lpw_ + (x[eos] - lse);
      const float sc = total / pen_stay;
      if (sc == sc) { cs[W] = sc; ct[W] = total; cf[W] = w * C2 + eos; }
    }
  }
  __syncthreads();
  // rank of every survivor among the survivors; flat indices are distinct, so are the ranks
  for (int i = tid; i < ncand; i += BEAM_THREADS) {
    const int fi = c_flat[i];
    if (fi < 0) continue;
    const float si = c_score[i];
    int rank = 0;
    for (int j = 0; j < ncand; ++j) {
      const int fj = c_flat[j];
      if (fj >= 0 && beam_before(c_score[j], fj, si, fi)) ++rank;
    }
    if (rank < W) { r_score[rank] = si; r_total[rank] = c_total[i]; r_flat[rank] = fi; }
  }
  __syncthreads();
  if (tid < W) {
    // (a place nothing reached -- only possible with NaN logits -- repeats the slot as a finished <EOS>)
    const int flat = r_flat[tid] >= 0 ? r_flat[tid] : tid * C2 + eos;
    const int wd = flat % C2, pa = flat / C2;
    const int fin = (s_fin[pa] || wd == eos) ? 1 : 0;
    const size_t o = (size_t)b * W + tid;
    word[o] = wd;
    parent[o] = pa;
    score[o] = r_score[tid];
    lp_out[o] = r_total[tid];
    fin_out[o] = fin;
    len_out[o] = s_len[pa] + ((wd != eos && !fin) ? 1 : 0);
    if (!fin) atomicAdd(&s_live, 1);
  }
  __syncthreads();
  if (tid == 0 && unfinished && s_live) atomicAdd(unfinished, s_live);
}

// One workgroup per row r = b*W + w of the next step's input: everything step k+1 reads from step k is the parent's
// (tf.gather by beam_parent_ids, beam_search_decoder.py:206-212), the embedding is that of the chosen word (:224-228).
// Out of place: several children may read one parent row.
__global__ __launch_bounds__(256) void att_beam_reorder_kernel(
    const int32_t* __restrict__ parent, const int32_t* __restrict__ word, int W, int U, int Em, int E2, int T, int vocab,
    const float* __restrict__ c_src, const float* __restrict__ h_src, const float* __restrict__ din_src,
    const float* __restrict__ alpha_src, const float* __restrict__ emb, float* __restrict__ c_dst,
    float* __restrict__ h_dst, float* __restrict__ din_dst, float* __restrict__ alpha_dst) {
  const int r = blockIdx.x, tid = threadIdx.x;
  int pa = parent[r], wd = word[r];
  pa = pa < 0 ? 0 : (pa >= W ? W - 1 : pa);                 // (never out of range from the select kernel: bounds only)
  wd = wd < 0 ? 0 : (wd >= vocab ? vocab - 1 : wd);
  const size_t pr = (size_t)(r / W) * W + pa;
  const int Din = Em + E2 + U;
  for (int j = tid; j < U; j += 256) {
    c_dst[(size_t)r * U + j] = c_src[pr * U + j];
    h_dst[(size_t)r * U + j] = h_src[pr * U + j];
  }
  for (int j = tid; j < E2 + U; j += 256) din_dst[(size_t)r * Din + Em + j] = din_src[pr * Din + Em + j];
  for (int j = tid; j < Em; j += 256) din_dst[(size_t)r * Din + j] = emb[(size_t)wd * Em + j];
  if (alpha_dst)
    for (int j = tid; j < T; j += 256) alpha_dst[(size_t)r * T + j] = alpha_src[pr * T + j];
}

// One thread per (utterance, final slot): gather_tree_py (util.py:14-26), then the cut behind the first <EOS>.
__global__ __launch_bounds__(256) void att_beam_backtrace_kernel(
    const int32_t* __restrict__ word, const int32_t* __restrict__ parent, const float* __restrict__ score, int steps, int To,
    int B, int W, int eos, int32_t* __restrict__ ids, int32_t* __restrict__ hyp_len, float* __restrict__ final_score) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * W) return;
  const int b = i / W, w = i % W;
  int32_t* out = ids + (size_t)i * To;
  int p = w;
  for (int level = steps - 1; level >= 0; --level) {
    const size_t o = ((size_t)level * B + b) * W;
    out[level] = word[o + p];
    const int q = parent[o + p];
    p = q < 0 ? 0 : (q >= W ? W - 1 : q);
  }
  int n = steps;
  for (int level = 0; level < steps; ++level)
    if (out[level] == eos) { n = level + 1; break; }
  for (int level = n; level < To; ++level) out[level] = 0;
  hyp_len[i] = n;
  final_score[i] = score[((size_t)(steps - 1) * B + b) * W + w];
}

}  // namespace

#define BEAM_NEED(cond, msg) do { if (!(cond)) ASR_FAIL(h, ASR_ERR_INVALID_ARG, msg); } while (0)

extern "C" int asr_att_beam_select(asr_handle* h, const float* logits, int B, int W, int C2, int eos, float lpw,
                                   int first_step, const float* lp_in, const int32_t* fin_in, const int32_t* len_in,
                                   int32_t* word, int32_t* parent, float* score, float* lp_out, int32_t* fin_out,
                                   int32_t* len_out, int32_t* unfinished, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  BEAM_NEED(logits && lp_in && fin_in && len_in && word && parent && score && lp_out && fin_out && len_out,
            "asr_att_beam_select: null");
  BEAM_NEED(B >= 1 && C2 >= 1 && eos >= 0 && eos < C2, "asr_att_beam_select: bad shape");
  BEAM_NEED(W >= 1 && W <= BEAM_MAX_W, "asr_att_beam_select: beam width must be in 1 .. 32");
  BEAM_NEED(W <= C2, "asr_att_beam_select: beam width exceeds the number of classes");
  BEAM_NEED((long long)W * C2 <= 0x7fffffffLL, "asr_att_beam_select: flat index overflow");
  h->att_beam_counts[0] += 1;
  hipLaunchKernelGGL(att_beam_select_kernel, dim3(B), dim3(BEAM_THREADS), 0, (hipStream_t)s, logits, W, C2, eos, lpw,
                     first_step, lp_in, fin_in, len_in, word, parent, score, lp_out, fin_out, len_out, unfinished);
  ASR_CHECK_LAUNCH(h, "asr_att_beam_select");
  return ASR_OK;
}

extern "C" int asr_att_beam_reorder(asr_handle* h, const int32_t* parent, const int32_t* word, int B, int W, int U, int Em,
                                    int E2, int T, int vocab, const float* c_src, const float* h_src, const float* din_src,
                                    const float* alpha_src, const float* embedding, float* c_dst, float* h_dst,
                                    float* din_dst, float* alpha_dst, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  BEAM_NEED(parent && word && c_src && h_src && din_src && c_dst && h_dst && din_dst && (Em == 0 || embedding),
            "asr_att_beam_reorder: null");
  BEAM_NEED(B >= 1 && W >= 1 && W <= BEAM_MAX_W && U >= 1 && Em >= 0 && E2 >= 1 && T >= 0 && vocab >= 1,
            "asr_att_beam_reorder: bad shape");
  BEAM_NEED((T == 0) == (alpha_dst == nullptr) && (T == 0 || alpha_src), "asr_att_beam_reorder: alpha arrays and T disagree");
  BEAM_NEED(c_src != c_dst && h_src != h_dst && din_src != din_dst && (!alpha_dst || alpha_src != alpha_dst),
            "asr_att_beam_reorder: the gather is out of place");
  h->att_beam_counts[1] += 1;
  hipLaunchKernelGGL(att_beam_reorder_kernel, dim3(B * W), dim3(256), 0, (hipStream_t)s, parent, word, W, U, Em, E2, T,
                     vocab, c_src, h_src, din_src, alpha_src, embedding, c_dst, h_dst, din_dst, alpha_dst);
  ASR_CHECK_LAUNCH(h, "asr_att_beam_reorder");
  return ASR_OK;
}

extern "C" int asr_att_beam_backtrace(asr_handle* h, const int32_t* word, const int32_t* parent, const float* score,
                                      int steps, int To, int B, int W, int eos, int32_t* ids, int32_t* hyp_len,
                                      float* final_score, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  BEAM_NEED(word && parent && score && ids && hyp_len && final_score, "asr_att_beam_backtrace: null");
  BEAM_NEED(B >= 1 && W >= 1 && W <= BEAM_MAX_W && steps >= 1 && steps <= To, "asr_att_beam_backtrace: bad shape");
  h->att_beam_counts[2] += 1;
  hipLaunchKernelGGL(att_beam_backtrace_kernel, dim3((B * W + 255) / 256), dim3(256), 0, (hipStream_t)s, word, parent,
                     score, steps, To, B, W, eos, ids, hyp_len, final_score);
  ASR_CHECK_LAUNCH(h, "asr_att_beam_backtrace");
  return ASR_OK;
}

extern "C" int asr_att_beam_counts(asr_handle* h, unsigned long long* out3) {
  if (!h || !out3) return ASR_ERR_INVALID_ARG;
  for (int i = 0; i < 3; ++i) out3[i] = h->att_beam_counts[i];
  return ASR_OK;
}
extern "C" int asr_reset_att_beam_counts(asr_handle* h) {
  if (!h) return ASR_ERR_INVALID_ARG;
  for (int i = 0; i < 3; ++i) h->att_beam_counts[i] = 0;
  return ASR_OK;
}
