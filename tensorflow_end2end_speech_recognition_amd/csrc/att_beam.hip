// Beam search over the attention decoder (models/attention/decoders/beam_search/ of the reference): every per-step
// selection -- on the attention scores alone (att_beam_select_kernel) and on attention scores fused with CTC prefix
// scores and / or a language model's (the att_select_candidates_kernel / att_select_rank_kernel pair: joint CTC /
// attention search, Watanabe et al. 2017, Hori et al. 2017, and shallow LM fusion; float64 statements in
// beam_search/ctc_prefix_score.py and beam_search/lm_fusion.py) --, the re-ordering of what the next step reads, and the
// back-trace.  The loops that issue them are asr_att_decoder_beam{,_joint,_lm} (dec_loop.hip, next to the greedy loop
// whose per-step code they share); the prefix scorer is ctc_prefix.hip, the language model lm_fusion.hip.
#include "common.h"
#include <math.h>

namespace {

constexpr int BEAM_MAX_W = 32;
constexpr int BEAM_THREADS = 1024;                          // 16 waves: a wave per slot row (two rows each from W = 17)
constexpr int BEAM_CAND = BEAM_MAX_W * (BEAM_MAX_W + 1);    // per row: its W best other classes and <EOS>

// (value, index) order of tf.nn.top_k: larger value first, equal values by ascending index
__device__ __forceinline__ bool beam_before(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

// max + log(sum exp(x - max)) of a row, by the row's wave: lane l takes the columns l, l + 64, ... in ascending order into
// a running maximum, the 64 maxima meet in a butterfly (xor 32, 16, ... 1); the sum of exp(x - max) the same way: per lane
// sequentially over its columns, then the butterfly.  (The tests' 1e-4 bound on score / log_probs counts these roundings.)
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

// rank of the survivor (si, fi) among the ncand candidates (c_flat < 0: not a survivor); flat indices are distinct, so
// are the ranks
__device__ __forceinline__ int beam_rank(const float* c_score, const int* c_flat, int ncand, float si, int fi) {
  int rank = 0;
  for (int j = 0; j < ncand; ++j) {
    const int fj = c_flat[j];
    if (fj >= 0 && beam_before(c_score[j], fj, si, fi)) ++rank;
  }
  return rank;
}

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
// lse = max + log(sum) in row_lse's reduction order; p = x - lse; total = log_probs + p;
// score = total / (pow(5 + len, a) / pow(6, a)).  (The log-sum-exp and the rank loop are spelled out here and not calls
// of row_lse / beam_rank: with either call the compiler allocates this kernel's registers differently, and its code is
// kept as it was.)
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

// ---- the selection over several score streams: attention + CTC prefix scores (CTC), + a language model (LM), or both.
// att_beam_select_kernel split in two around the prefix scorer, which needs the candidates:
//   1. att_select_candidates_kernel<LM>      one wave per slot row: the row's W + 1 candidates and their totals
//   2. ctc_prefix_score_kernel on cand        (CTC only; ctc_prefix.hip)
//   3. att_select_rank_kernel<CTC, LM>        one workgroup per utterance: fused scores, the W best, the next state
//
// Stage 1.  The row's log-softmax (row_lse), its W best classes other than <EOS> (ties by lower index; one per round, the
// best that comes after the previous one, as att_beam_select_kernel) and <EOS>.  cand [R, W+1] (-1: no candidate),
// total [R, W+1] = log_probs + (x[c] - lse).  A finished row has its <EOS> alone (p = 0); at the first step only slot 0
// has candidates.
//   !LM: the rounds compare the raw logits x[c] -- not x[c] - lse: two distinct logits can round to one difference, and
//        then the index rather than the logit would break the tie.  lm_logits, lm_in and lmt are not touched.
//    LM: both rows of logits are read here and nowhere else (no log-softmax pass over lm_logits); the rounds compare
//        local[c] = (x[c] - lse) + mu * (z[c] - lse_lm), and lmt [R, W+1] = lm_score + (z[c] - lse_lm) comes out too.
template <bool LM>
__global__ __launch_bounds__(64) void att_select_candidates_kernel(
    const float* __restrict__ logits, const float* __restrict__ lm_logits, int W, int C2, int eos, float mu, int first_step,
    const float* __restrict__ lp_in, const int32_t* __restrict__ fin_in, const float* __restrict__ lm_in,
    int32_t* __restrict__ cand, float* __restrict__ total, float* __restrict__ lmt) {
  const int row = blockIdx.x, lane = threadIdx.x, w = row % W;
  int my_c = -1;                                             // lane j <= W keeps candidate j and writes it at the end
  float my_tot = -INFINITY, my_lm = -INFINITY;
  const float lp = lp_in[row], ls = LM ? lm_in[row] : 0.f;
  if (first_step && w > 0) {                                 // (wave-uniform) every slot holds the same hypothesis
  } else if (fin_in[row] != 0) {
    if (lane == W) {
      my_c = eos; my_tot = lp + 0.f;
      if constexpr (LM) my_lm = ls + 0.f;
    }
  } else {
    const float* x = logits + (size_t)row * C2;
    const float* z = LM ? lm_logits + (size_t)row * C2 : nullptr;
    const float lse = row_lse(x, C2, lane);
    const float lse_l = LM ? row_lse(z, C2, lane) : 0.f;
    float pv = INFINITY;
    int pi = -1;
    for (int j = 0; j < W; ++j) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int c = lane; c < C2; c += 64) {
        float v;
        if constexpr (LM) v = (x[c] - lse) + mu * (z[c] - lse_l);
        else v = x[c];
        if (c != eos && beam_before(pv, pi, v, c) && beam_before(v, c, bv, bi)) { bv = v; bi = c; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (beam_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      if (bi == 0x7fffffff) break;                           // (wave-uniform) fewer than W other classes, or NaNs
      if (lane == j) {
        my_c = bi;
        if constexpr (LM) { my_tot = lp + (x[bi] - lse); my_lm = ls + (z[bi] - lse_l); }
        else my_tot = lp + (bv - lse);                       // (bv is x[bi])
      }
      pv = bv; pi = bi;
    }
    if (lane == W) {
      my_c = eos; my_tot = lp + (x[eos] - lse);
      if constexpr (LM) my_lm = ls + (z[eos] - lse_l);
    }
  }
  if (lane <= W) {
    const bool ok = my_c >= 0 && my_tot == my_tot && (!LM || my_lm == my_lm);          // (no NaN takes a place)
    const size_t o = (size_t)row * (W + 1) + lane;
    cand[o] = ok ? my_c : -1;
    total[o] = ok ? my_tot : -INFINITY;
    if constexpr (LM) lmt[o] = ok ? my_lm : -INFINITY;
  }
}

// The weighted sum of a candidate's score streams.  hipcc contracts a * b + c * d into an fma around whichever product its
// heuristics pick, and which one depends on the code around the expression; so the roundings are spelled out, per
// instantiation those of the kernel it replaced (read off its gfx950 code):
//   <CTC, !LM>  the joint selection's `(1 - lam) * tot + lam * ctc` compiled to two rounded products (one v_pk_mul_f32)
//               and an add: no fma;
//   <*, LM>     the LM-fused selection's `f = (1 - lam) * tot; if (ctc) f = f + lam * ctc; f = f + mu * lm;` compiled
//               to one rounded product and an fma per further stream.
template <bool CTC, bool LM>
__device__ __forceinline__ float fused_score(float lam, float mu, float tot, float ctc, float lm) {
#pragma clang fp contract(off)
  if constexpr (!LM) {
    return (1.f - lam) * tot + lam * ctc;
  } else {
    float fused = (1.f - lam) * tot;
    if constexpr (CTC) fused = __builtin_fmaf(lam, ctc, fused);
    return __builtin_fmaf(mu, lm, fused);
  }
}

// Stage 3.  Per candidate ctc = psi, or the slot's carried ctc_score if it had finished (0 without CTC); a candidate
// whose ctc is -inf is dropped; fused = (1 - lam) * total [+ lam * ctc] [+ mu * lmt] (fused_score);
// score = fused / (pow(5 + len, a) / pow(6, a)) (a == 1: fused, the quirk of normalize_score).  The W best by (score
// descending, flat index w*C2 + c ascending) give word / parent / score and the next state: log_probs = total
// (attention alone), finished, lengths as att_beam_select_kernel, and per stream ctc_score = ctc with last = the word
// unless it is <EOS> (then the parent's), lm_score = lmt.  Without CTC nothing of psi, last_in, ctc_in, last_out,
// ctc_out is touched (they may be null); without LM nothing of lmt, lm_in, lm_out.  All *_in state is read before the
// first barrier: out may be in.
template <bool CTC, bool LM>
__global__ __launch_bounds__(256) void att_select_rank_kernel(
    const int32_t* __restrict__ cand, const float* __restrict__ total, const float* __restrict__ lmt,
    const float* __restrict__ psi, int W, int C2, int eos, float lpw, float lam, float mu, const int32_t* fin_in,
    const int32_t* len_in, const int32_t* last_in, const float* ctc_in, const float* lm_in, int32_t* __restrict__ word,
    int32_t* __restrict__ parent, float* __restrict__ score, float* lp_out, int32_t* fin_out, int32_t* len_out,
    int32_t* last_out, float* ctc_out, float* lm_out, int32_t* __restrict__ unfinished) {
  constexpr int NW_CTC = CTC ? BEAM_MAX_W : 1, NC_CTC = CTC ? BEAM_CAND : 1;            // (a stream that is off keeps no LDS)
  constexpr int NW_LM = LM ? BEAM_MAX_W : 1, NC_LM = LM ? BEAM_CAND : 1;
  __shared__ int s_fin[BEAM_MAX_W], s_len[BEAM_MAX_W], s_last[NW_CTC];
  __shared__ float s_ctc[NW_CTC], s_lm[NW_LM];
  __shared__ float c_score[BEAM_CAND], c_total[BEAM_CAND], c_ctc[NC_CTC], c_lm[NC_LM];
  __shared__ int c_flat[BEAM_CAND];
  __shared__ float r_score[BEAM_MAX_W], r_total[BEAM_MAX_W], r_ctc[NW_CTC], r_lm[NW_LM];
  __shared__ int r_flat[BEAM_MAX_W];
  __shared__ int s_live;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ncand = W * (W + 1);
  if (tid < W) {
    s_fin[tid] = fin_in[b * W + tid] != 0;
    s_len[tid] = len_in[b * W + tid];
    if constexpr (CTC) { s_last[tid] = last_in[b * W + tid]; s_ctc[tid] = ctc_in[b * W + tid]; r_ctc[tid] = -INFINITY; }
    if constexpr (LM) { s_lm[tid] = lm_in[b * W + tid]; r_lm[tid] = -INFINITY; }
    r_score[tid] = -INFINITY; r_total[tid] = -INFINITY; r_flat[tid] = -1;
  }
  if (tid == 0) s_live = 0;
  __syncthreads();
  const float pen6 = powf(6.f, lpw);
  for (int i = tid; i < ncand; i += 256) {
    const int w = i / (W + 1);
    const size_t o = (size_t)b * ncand + i;
    const int c = cand[o];
    int flat = -1;
    float sc = -INFINITY, tot = -INFINITY, ctc = CTC ? -INFINITY : 0.f, lm = -INFINITY;
    if (c >= 0 && c < C2) {
      tot = total[o];
      if constexpr (LM) lm = lmt[o];
      if constexpr (CTC) ctc = s_fin[w] ? s_ctc[w] : psi[o];
      const float fused = fused_score<CTC, LM>(lam, mu, tot, ctc, lm);
      const int len = s_len[w] + ((c != eos && !s_fin[w]) ? 1 : 0);
      sc = lpw == 1.f ? fused : fused / (powf(5.f + (float)len, lpw) / pen6);
      if (ctc != -INFINITY && sc == sc) flat = w * C2 + c;   // (sc == sc: no NaN takes a place)
    }
    c_score[i] = sc; c_total[i] = tot; c_flat[i] = flat;
    if constexpr (CTC) c_ctc[i] = ctc;
    if constexpr (LM) c_lm[i] = lm;
  }
  __syncthreads();
  for (int i = tid; i < ncand; i += 256) {
    const int fi = c_flat[i];
    if (fi < 0) continue;
    const float si = c_score[i];
    const int rank = beam_rank(c_score, c_flat, ncand, si, fi);
    if (rank < W) {
      r_score[rank] = si; r_total[rank] = c_total[i]; r_flat[rank] = fi;
      if constexpr (CTC) r_ctc[rank] = c_ctc[i];
      if constexpr (LM) r_lm[rank] = c_lm[i];
    }
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
    if constexpr (LM) lm_out[o] = hit ? r_lm[tid] : s_lm[pa];
    fin_out[o] = fin;
    len_out[o] = s_len[pa] + ((wd != eos && !fin) ? 1 : 0);
    if constexpr (CTC) {
      ctc_out[o] = hit ? r_ctc[tid] : s_ctc[pa];
      last_out[o] = wd == eos ? s_last[pa] : wd;
    }
    if (!fin) atomicAdd(&s_live, 1);
  }
  __syncthreads();
  if (tid == 0 && unfinished && s_live) atomicAdd(unfinished, s_live);
}

}  // namespace

extern "C" int asr_att_beam_select(asr_handle* h, const float* logits, int B, int W, int C2, int eos, float lpw,
                                   int first_step, const float* lp_in, const int32_t* fin_in, const int32_t* len_in,
                                   int32_t* word, int32_t* parent, float* score, float* lp_out, int32_t* fin_out,
                                   int32_t* len_out, int32_t* unfinished, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(logits && lp_in && fin_in && len_in && word && parent && score && lp_out && fin_out && len_out,
           "asr_att_beam_select: null");
  ASR_NEED(B >= 1 && C2 >= 1 && eos >= 0 && eos < C2, "asr_att_beam_select: bad shape");
  ASR_NEED(W >= 1 && W <= BEAM_MAX_W, "asr_att_beam_select: beam width must be in 1 .. 32");
  ASR_NEED(W <= C2, "asr_att_beam_select: beam width exceeds the number of classes");
  ASR_NEED((long long)W * C2 <= 0x7fffffffLL, "asr_att_beam_select: flat index overflow");
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
  ASR_NEED(parent && word && c_src && h_src && din_src && c_dst && h_dst && din_dst && (Em == 0 || embedding),
           "asr_att_beam_reorder: null");
  ASR_NEED(B >= 1 && W >= 1 && W <= BEAM_MAX_W && U >= 1 && Em >= 0 && E2 >= 1 && T >= 0 && vocab >= 1,
           "asr_att_beam_reorder: bad shape");
  ASR_NEED((T == 0) == (alpha_dst == nullptr) && (T == 0 || alpha_src), "asr_att_beam_reorder: alpha arrays and T disagree");
  ASR_NEED(c_src != c_dst && h_src != h_dst && din_src != din_dst && (!alpha_dst || alpha_src != alpha_dst),
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
  ASR_NEED(word && parent && score && ids && hyp_len && final_score, "asr_att_beam_backtrace: null");
  ASR_NEED(B >= 1 && W >= 1 && W <= BEAM_MAX_W && steps >= 1 && steps <= To, "asr_att_beam_backtrace: bad shape");
  h->att_beam_counts[2] += 1;
  hipLaunchKernelGGL(att_beam_backtrace_kernel, dim3((B * W + 255) / 256), dim3(256), 0, (hipStream_t)s, word, parent,
                     score, steps, To, B, W, eos, ids, hyp_len, final_score);
  ASR_CHECK_LAUNCH(h, "asr_att_beam_backtrace");
  return ASR_OK;
}

ASR_DEFINE_COUNTS(att_beam_counts, att_beam_counts)

// What asr_att_beam_select_joint (ctc, !lm) and asr_att_beam_select_fused (lm, ctc iff ctc_weight > 0) do once their
// arguments are checked: candidates, the prefix scorer on them with CTC, rank.  `who`: the entry point's launch labels.
static int att_select_streams(asr_handle* h, const char* const who[2], bool ctc, bool lm, const float* logits,
                              const float* lm_logits, int B, int W, int n_labels, float lpw, float ctc_weight, float lm_weight,
                              int first_step, const float* y, const int32_t* seq_len, int T, int By, int Cc, int blank,
                              const float* r, const float* lp_in, const int32_t* fin_in, const int32_t* len_in,
                              const int32_t* last_in, const float* ctc_in, const float* lm_in, int32_t* cand, float* cand_total,
                              float* cand_lm, float* psi, int32_t* word, int32_t* parent, float* score, float* lp_out,
                              int32_t* fin_out, int32_t* len_out, int32_t* last_out, float* ctc_out, float* lm_out,
                              int32_t* unfinished, asr_stream s) {
  const int C2 = n_labels + 2, eos = n_labels + 1;
  hipStream_t st = (hipStream_t)s;
  const auto candidates = lm ? att_select_candidates_kernel<true> : att_select_candidates_kernel<false>;
  const auto rank = !lm ? att_select_rank_kernel<true, false>
                        : ctc ? att_select_rank_kernel<true, true> : att_select_rank_kernel<false, true>;
  hipLaunchKernelGGL(candidates, dim3(B * W), dim3(64), 0, st, logits, lm_logits, W, C2, eos, lm_weight, first_step, lp_in,
                     fin_in, lm_in, cand, cand_total, cand_lm);
  ASR_CHECK_LAUNCH(h, who[0]);
  if (ctc) ASR_TRY(asr_ctc_prefix_score(h, y, seq_len, B, W, T, By, Cc, blank, n_labels, r, last_in, fin_in, cand, W + 1, psi, s));
  hipLaunchKernelGGL(rank, dim3(B), dim3(256), 0, st, cand, cand_total, cand_lm, psi, W, C2, eos, lpw, ctc_weight, lm_weight,
                     fin_in, len_in, last_in, ctc_in, lm_in, word, parent, score, lp_out, fin_out, len_out, last_out, ctc_out,
                     lm_out, unfinished);
  ASR_CHECK_LAUNCH(h, who[1]);
  return ASR_OK;
}

static bool ctc_shape_ok(int B, int T, int By, int Cc, int blank, int n_labels) {
  return T >= 1 && By >= B && n_labels < Cc && blank >= n_labels && blank < Cc;
}

extern "C" int asr_att_beam_select_joint(asr_handle* h, const float* logits, int B, int W, int n_labels, float lpw,
                                         float ctc_weight, int first_step, const float* y, const int32_t* seq_len, int T, int By,
                                         int Cc, int blank, const float* r, const float* lp_in, const int32_t* fin_in,
                                         const int32_t* len_in, const int32_t* last_in, const float* ctc_in, int32_t* cand,
                                         float* cand_total, float* psi, int32_t* word, int32_t* parent, float* score,
                                         float* lp_out, int32_t* fin_out, int32_t* len_out, int32_t* last_out, float* ctc_out,
                                         int32_t* unfinished, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(logits && y && seq_len && r && lp_in && fin_in && len_in && last_in && ctc_in && cand && cand_total && psi &&
               word && parent && score && lp_out && fin_out && len_out && last_out && ctc_out,
           "asr_att_beam_select_joint: null");
  ASR_NEED(B >= 1 && W >= 1 && W <= BEAM_MAX_W && n_labels >= 1 && ctc_shape_ok(B, T, By, Cc, blank, n_labels),
           "asr_att_beam_select_joint: bad shape");
  ASR_NEED(W <= n_labels + 1, "asr_att_beam_select_joint: beam width exceeds the labels and <EOS> step 0 selects among");
  ASR_NEED(ctc_weight > 0.f && ctc_weight <= 1.f, "asr_att_beam_select_joint: ctc_weight must be in (0, 1]");
  ASR_NEED((long long)W * (n_labels + 2) <= 0x7fffffffLL, "asr_att_beam_select_joint: flat index overflow");
  static const char* const who[2] = {"asr_att_beam_select_joint(candidates)", "asr_att_beam_select_joint(rank)"};
  h->att_joint_counts[2] += 1;
  return att_select_streams(h, who, true, false, logits, nullptr, B, W, n_labels, lpw, ctc_weight, 0.f, first_step, y, seq_len, T,
                            By, Cc, blank, r, lp_in, fin_in, len_in, last_in, ctc_in, nullptr, cand, cand_total, nullptr, psi,
                            word, parent, score, lp_out, fin_out, len_out, last_out, ctc_out, nullptr, unfinished, s);
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
  ASR_NEED(logits && lm_logits && lp_in && fin_in && len_in && lm_in && cand && cand_total && cand_lm && word && parent &&
               score && lp_out && fin_out && len_out && lm_out, "asr_att_beam_select_fused: null");
  ASR_NEED(B >= 1 && n_labels >= 1 && W >= 1 && W <= BEAM_MAX_W, "asr_att_beam_select_fused: bad shape");
  ASR_NEED(W <= n_labels + 1, "asr_att_beam_select_fused: beam width exceeds the labels and <EOS> step 0 selects among");
  ASR_NEED(lm_weight > 0.f && lm_weight < INFINITY, "asr_att_beam_select_fused: lm_weight must be a finite number > 0");
  ASR_NEED(ctc_weight >= 0.f && ctc_weight <= 1.f, "asr_att_beam_select_fused: ctc_weight must be in [0, 1]");
  const bool ctc = ctc_weight > 0.f;
  if (ctc)
    ASR_NEED(y && seq_len && r && last_in && ctc_in && psi && last_out && ctc_out && ctc_shape_ok(B, T, By, Cc, blank, n_labels),
             "asr_att_beam_select_fused: bad arguments (the CTC part)");
  ASR_NEED((long long)W * (n_labels + 2) <= 0x7fffffffLL, "asr_att_beam_select_fused: flat index overflow");
  static const char* const who[2] = {"asr_att_beam_select_fused(candidates)", "asr_att_beam_select_fused(rank)"};
  h->att_lm_counts[1] += 1;
  return att_select_streams(h, who, ctc, true, logits, lm_logits, B, W, n_labels, lpw, ctc_weight, lm_weight, first_step, y,
                            seq_len, T, By, Cc, blank, r, lp_in, fin_in, len_in, last_in, ctc_in, lm_in, cand, cand_total, cand_lm,
                            psi, word, parent, score, lp_out, fin_out, len_out, last_out, ctc_out, lm_out, unfinished, s);
}
