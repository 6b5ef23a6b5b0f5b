// One-pass joint CTC / attention beam search (Watanabe et al. 2017, Hori et al. 2017): the CTC prefix scores of the
// candidates of a beam search step, the state they are computed from, and the selection by fused score.  The float64
// statement is models/attention/decoders/beam_search/ctc_prefix_score.py; the loop that issues these is
// asr_att_decoder_beam_joint (attention.hip, the beam search loop with this selection in place of asr_att_beam_select).
//
// Vocabularies: attention classes C2 = N + 2 (labels, <SOS> = N, <EOS> = N + 1); CTC classes Cc = N + 1 (blank = N by
// default).  y [T, By, Cc] are log-posteriors (asr_log_softmax_rows of the CTC head's logits); device row r = b*W + w reads
// utterance b = r / W, the posteriors are not tiled.  State r [R, 2, T] fp32: r[row, 0, t] = r_n[t], r[row, 1, t] = r_b[t],
// written and read for t < seq_len[b] only.
#include "common.h"
#include <math.h>

namespace {

constexpr int JOINT_MAX_W = 32;
constexpr int JOINT_CAND = JOINT_MAX_W * (JOINT_MAX_W + 1);
constexpr int JOINT_CH = 64;                                // frames per chunk: one per lane

// (value, index) order of tf.nn.top_k, as att_beam.hip
__device__ __forceinline__ bool joint_before(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

// log(exp(a) + exp(b)); -inf for two -inf (never NaN: +inf does not occur)
__device__ __forceinline__ float lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log1pf(expf(fminf(a, b) - m));
}

// One wave per row: out = x - (max + log(sum exp(x - max))).  Lane l takes the columns l, l + 64, ... in ascending order
// into a running maximum / sum, the 64 partials meet in a butterfly (xor 32 .. 1): the order of att_beam_select_kernel.
__global__ __launch_bounds__(256) void log_softmax_rows_kernel(const float* x, float* out,     // (out may be x)
                                                               long long rows, int cols) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* p = x + (size_t)row * cols;
  float m = -INFINITY;
  for (int c = lane; c < cols; c += 64) m = fmaxf(m, p[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float sum = 0.f;
  for (int c = lane; c < cols; c += 64) sum += expf(p[c] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  const float lse = m + logf(sum);
  float* q = out + (size_t)row * cols;
  for (int c = lane; c < cols; c += 64) q[c] = p[c] - lse;
}

// The empty hypothesis, one thread per row: r_n = -inf, r_b[t] = y[0, blank] + ... + y[t, blank] summed in ascending t.
__global__ __launch_bounds__(64) void ctc_prefix_init_kernel(const float* __restrict__ y, const int32_t* __restrict__ seq_len,
                                                             int R, int W, int T, int By, int Cc, int blank,
                                                             float* __restrict__ r, int32_t* __restrict__ last,
                                                             float* __restrict__ ctc_score) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= R) return;
  const int b = row / W;
  int Tb = seq_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  float* rn = r + (size_t)row * 2 * T;
  float* rb = rn + T;
  float acc = 0.f;
  for (int t = 0; t < Tb; ++t) {
    acc += y[((size_t)t * By + b) * Cc + blank];
    rn[t] = -INFINITY;
    rb[t] = acc;
  }
  if (last) last[row] = -1;
  if (ctc_score) ctc_score[row] = 0.f;
}

// psi [R, K] of the candidates cand [R, K] (attention class ids; anything outside 0 .. N + 1 gives -inf), one wave per
// row, lane k < K its candidate k.
//
// For a label c the recursion's psi does not depend on the extended state: psi = logsumexp over t < T_b of
// phi[t] + y[t, c], with phi[0] = 0 for the empty hypothesis and -inf otherwise, and for t >= 1
// phi[t] = r_b[t-1] if c == last, logaddexp(r_n[t-1], r_b[t-1]) otherwise.  So there is no dependent chain here:
// per 64-frame chunk the lanes form both phi (frame = lane, coalesced reads of r) into LDS, every candidate lane then
// gathers its 64 y[t, b, c] at once (independent loads), takes the chunk's maximum, rescales its running sum when the
// maximum grows, and adds exp(v - max) frame by frame in ascending t.  psi = max + log(sum).
// <EOS>: logaddexp(r_n[T_b-1], r_b[T_b-1]) = log p_ctc(g).  <SOS>: -inf.  A finished row: -inf but for <EOS>.
__global__ __launch_bounds__(64) void ctc_prefix_score_kernel(
    const float* __restrict__ y, const int32_t* __restrict__ seq_len, const float* __restrict__ r,
    const int32_t* __restrict__ last, const int32_t* __restrict__ finished, const int32_t* __restrict__ cand, int W, int K,
    int T, int By, int Cc, int blank, int N, float* __restrict__ psi) {
  __shared__ float s_same[JOINT_CH], s_diff[JOINT_CH];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int b = row / W;
  int Tb = seq_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  const float* rn = r + (size_t)row * 2 * T;
  const float* rb = rn + T;
  const int lst = last[row];
  const bool fin = finished && finished[row] != 0;
  const int c = lane < K ? cand[(size_t)row * K + lane] : -1;
  const bool is_label = c >= 0 && c < N && c != blank && c < Cc && !fin;
  const bool same = is_label && c == lst;
  float m = -INFINITY, sum = 0.f;
  for (int t0 = 0; t0 < Tb; t0 += JOINT_CH) {
    const int t = t0 + lane;
    float ps = -INFINITY, pd = -INFINITY;
    if (t < Tb) {
      if (t == 0) {
        ps = pd = lst < 0 ? 0.f : -INFINITY;
      } else {
        const float a = rn[t - 1], bb = rb[t - 1];
        ps = bb;
        pd = lae(a, bb);
      }
    }
    __syncthreads();                                         // the previous chunk has been read
    s_same[lane] = ps;
    s_diff[lane] = pd;
    __syncthreads();
    if (is_label) {
      float v[JOINT_CH];
      float mc = -INFINITY;
#pragma unroll
      for (int j = 0; j < JOINT_CH; ++j) {
        const int tj = t0 + j;
        const float yv = tj < Tb ? y[((size_t)tj * By + b) * Cc + c] : -INFINITY;
        v[j] = (same ? s_same[j] : s_diff[j]) + yv;
        mc = fmaxf(mc, v[j]);
      }
      if (mc != -INFINITY) {
        if (mc > m) { sum *= expf(m - mc); m = mc; }
#pragma unroll
        for (int j = 0; j < JOINT_CH; ++j) sum += expf(v[j] - m);
      }
    }
  }
  if (lane < K) {
    float out = -INFINITY;
    if (is_label) out = m == -INFINITY ? -INFINITY : m + logf(sum);
    else if (c == N + 1) out = Tb > 0 ? lae(rn[Tb - 1], rb[Tb - 1]) : (lst < 0 ? 0.f : -INFINITY);
    psi[(size_t)row * K + lane] = out;
  }
}

// The state of the W winners, one wave per new row = b*W + w, out of place (several children may extend one parent):
// the parent's arrays, bit for bit, when the word is <EOS> (a finished parent's word always is); otherwise the extension
//   r_n'[0] = y[0, c] if the parent is empty else -inf;  r_b'[0] = -inf
//   r_n'[t] = logaddexp(r_n'[t-1], phi[t]) + y[t, c];  r_b'[t] = logaddexp(r_n'[t-1], r_b'[t-1]) + y[t, blank]
// Per 64-frame chunk the lanes read the parent's r, y[t, c] and y[t, blank] (frame = lane) and form phi into LDS, lane 0
// runs the 64 dependent steps (two logaddexp each) on LDS, and the lanes write the chunk back coalesced.
__global__ __launch_bounds__(64) void ctc_prefix_advance_kernel(
    const float* __restrict__ y, const int32_t* __restrict__ seq_len, const float* __restrict__ r_src,
    const int32_t* __restrict__ last_src, const int32_t* __restrict__ parent, const int32_t* __restrict__ word, int W, int T,
    int By, int Cc, int blank, int N, float* __restrict__ r_dst) {
  __shared__ float s_phi[JOINT_CH], s_yc[JOINT_CH], s_yb[JOINT_CH], s_n[JOINT_CH], s_b[JOINT_CH];
  __shared__ float s_carry[2];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int b = row / W;
  int Tb = seq_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  int pa = parent[row];
  pa = pa < 0 ? 0 : (pa >= W ? W - 1 : pa);                 // (never out of range from the select kernel: bounds only)
  const int wd = word[row];
  const size_t prow = (size_t)b * W + pa;
  const float* pn = r_src + prow * 2 * T;
  const float* pb = pn + T;
  float* dn = r_dst + (size_t)row * 2 * T;
  float* db = dn + T;
  if (!(wd >= 0 && wd < N && wd < Cc && wd != blank)) {     // (wave-uniform) <EOS>: the parent's state
    for (int t = lane; t < Tb; t += 64) { dn[t] = pn[t]; db[t] = pb[t]; }
    return;
  }
  const int lst = last_src[prow];
  const bool same = wd == lst;
  for (int t0 = 0; t0 < Tb; t0 += JOINT_CH) {
    const int t = t0 + lane;
    if (t < Tb) {
      float phi;
      if (t == 0) phi = -INFINITY;                           // (not read: frame 0 has its own rule)
      else {
        const float a = pn[t - 1], bb = pb[t - 1];
        phi = same ? bb : lae(a, bb);
      }
      s_phi[lane] = phi;
      s_yc[lane] = y[((size_t)t * By + b) * Cc + wd];
      s_yb[lane] = y[((size_t)t * By + b) * Cc + blank];
    }
    __syncthreads();
    if (lane == 0) {
      const int n = Tb - t0 < JOINT_CH ? Tb - t0 : JOINT_CH;
      float cn, cb;
      int j = 0;
      if (t0 == 0) {
        cn = lst < 0 ? s_yc[0] : -INFINITY;
        cb = -INFINITY;
        s_n[0] = cn; s_b[0] = cb;
        j = 1;
      } else {
        cn = s_carry[0]; cb = s_carry[1];
      }
      for (; j < n; ++j) {
        const float nn = lae(cn, s_phi[j]) + s_yc[j];
        const float nb = lae(cn, cb) + s_yb[j];
        cn = nn; cb = nb;
        s_n[j] = cn; s_b[j] = cb;
      }
      s_carry[0] = cn; s_carry[1] = cb;
    }
    __syncthreads();
    if (t < Tb) { dn[t] = s_n[lane]; db[t] = s_b[lane]; }
    __syncthreads();                                         // before the next chunk overwrites the LDS arrays
  }
}

// Joint selection, stage 1: one wave per slot row.  The extraction of att_beam_select_kernel (same reduction order, see
// there): the row's log-softmax, its W best classes other than <EOS> by logit (ties by lower index), and <EOS>.
// cand [R, W+1] (-1: no candidate) and total [R, W+1] = log_probs + log_softmax(logits)[c].  A finished row has its <EOS>
// alone (p = 0); at the first step only slot 0 has candidates.
__global__ __launch_bounds__(64) void att_joint_candidates_kernel(
    const float* __restrict__ logits, int W, int C2, int eos, int first_step, const float* __restrict__ lp_in,
    const int32_t* __restrict__ fin_in, int32_t* __restrict__ cand, float* __restrict__ total) {
  const int row = blockIdx.x, lane = threadIdx.x, w = row % W;
  int my_c = -1;                                             // lane j <= W keeps candidate j and writes it at the end
  float my_tot = -INFINITY;
  const float lp = lp_in[row];
  if (first_step && w > 0) {                                 // (wave-uniform) every slot holds the same hypothesis
  } else if (fin_in[row] != 0) {
    if (lane == W) { my_c = eos; my_tot = lp + 0.f; }
  } else {
    const float* x = logits + (size_t)row * C2;
    float m = -INFINITY;
    for (int c = lane; c < C2; c += 64) m = fmaxf(m, x[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.f;
    for (int c = lane; c < C2; c += 64) sum += expf(x[c] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float lse = m + logf(sum);
    float pv = INFINITY;
    int pi = -1;
    for (int j = 0; j < W; ++j) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int c = lane; c < C2; c += 64) {
        const float v = x[c];
        if (c != eos && joint_before(pv, pi, v, c) && joint_before(v, c, bv, bi)) { bv = v; bi = c; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (joint_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      if (bi == 0x7fffffff) break;                           // (wave-uniform) fewer than W other classes, or NaNs
      if (lane == j) { my_c = bi; my_tot = lp + (bv - lse); }
      pv = bv; pi = bi;
    }
    if (lane == W) { my_c = eos; my_tot = lp + (x[eos] - lse); }
  }
  if (lane <= W) {
    const bool ok = my_c >= 0 && my_tot == my_tot;           // (no NaN takes a place)
    cand[(size_t)row * (W + 1) + lane] = ok ? my_c : -1;
    total[(size_t)row * (W + 1) + lane] = ok ? my_tot : -INFINITY;
  }
}

// Joint selection, stage 3 (stage 2 is ctc_prefix_score_kernel on cand): one workgroup per utterance.  Per candidate
// ctc = psi, or the slot's carried ctc_score if it had finished; a candidate whose ctc is -inf is dropped;
// joint = (1 - lambda) * total + lambda * ctc; score = joint / (pow(5 + len, a) / pow(6, a)) (a == 1: joint, the quirk of
// normalize_score).  The W best by (score descending, flat index w*C2 + c ascending) give word / parent / score and the
// next state: log_probs = total (attention alone), ctc_score = ctc, finished, lengths as att_beam_select_kernel, last =
// the word unless it is <EOS> (then the parent's).  All *_in state is read before the first barrier: out may be in.
__global__ __launch_bounds__(256) void att_joint_rank_kernel(
    const int32_t* __restrict__ cand, const float* __restrict__ total, const float* __restrict__ psi, int W, int C2, int eos,
    float lpw, float lam, const int32_t* fin_in, const int32_t* len_in, const int32_t* last_in, const float* ctc_in,
    int32_t* __restrict__ word, int32_t* __restrict__ parent, float* __restrict__ score, float* lp_out, int32_t* fin_out,
    int32_t* len_out, int32_t* last_out, float* ctc_out, int32_t* __restrict__ unfinished) {
  __shared__ int s_fin[JOINT_MAX_W], s_len[JOINT_MAX_W], s_last[JOINT_MAX_W];
  __shared__ float s_ctc[JOINT_MAX_W];
  __shared__ float c_score[JOINT_CAND], c_total[JOINT_CAND], c_ctc[JOINT_CAND];
  __shared__ int c_flat[JOINT_CAND];
  __shared__ float r_score[JOINT_MAX_W], r_total[JOINT_MAX_W], r_ctc[JOINT_MAX_W];
  __shared__ int r_flat[JOINT_MAX_W];
  __shared__ int s_live;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ncand = W * (W + 1);
  if (tid < W) {
    s_fin[tid] = fin_in[b * W + tid] != 0;
    s_len[tid] = len_in[b * W + tid];
    s_last[tid] = last_in[b * W + tid];
    s_ctc[tid] = ctc_in[b * W + tid];
    r_score[tid] = -INFINITY; r_total[tid] = -INFINITY; r_ctc[tid] = -INFINITY; r_flat[tid] = -1;
  }
  if (tid == 0) s_live = 0;
  __syncthreads();
  const float pen6 = powf(6.f, lpw);
  for (int i = tid; i < ncand; i += 256) {
    const int w = i / (W + 1);
    const size_t o = (size_t)b * ncand + i;
    const int c = cand[o];
    int flat = -1;
    float sc = -INFINITY, tot = -INFINITY, ctc = -INFINITY;
    if (c >= 0 && c < C2) {
      tot = total[o];
      ctc = s_fin[w] ? s_ctc[w] : psi[o];
      const int len = s_len[w] + ((c != eos && !s_fin[w]) ? 1 : 0);
      const float joint = (1.f - lam) * tot + lam * ctc;
      sc = lpw == 1.f ? joint : joint / (powf(5.f + (float)len, lpw) / pen6);
      if (ctc != -INFINITY && sc == sc) flat = w * C2 + c;   // (sc == sc: no NaN takes a place)
    }
    c_score[i] = sc; c_total[i] = tot; c_ctc[i] = ctc; c_flat[i] = flat;
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
      if (fj >= 0 && joint_before(c_score[j], fj, si, fi)) ++rank;
    }
    if (rank < W) { r_score[rank] = si; r_total[rank] = c_total[i]; r_ctc[rank] = c_ctc[i]; r_flat[rank] = fi; }
  }
  __syncthreads();
  if (tid < W) {
    // (a place nothing reached -- fewer than W candidates with a finite CTC score -- repeats the slot as a finished <EOS>)
    const bool hit = r_flat[tid] >= 0;
    const int flat = hit ? r_flat[tid] : tid * C2 + eos;
    const int wd = flat % C2, pa = flat / C2;
    const int fin = (s_fin[pa] || wd == eos) ? 1 : 0;
    const size_t o = (size_t)b * W + tid;
    word[o] = wd;
    parent[o] = pa;
    score[o] = r_score[tid];
    lp_out[o] = r_total[tid];
    ctc_out[o] = hit ? r_ctc[tid] : s_ctc[pa];
    fin_out[o] = fin;
    len_out[o] = s_len[pa] + ((wd != eos && !fin) ? 1 : 0);
    last_out[o] = wd == eos ? s_last[pa] : wd;
    if (!fin) atomicAdd(&s_live, 1);
  }
  __syncthreads();
  if (tid == 0 && unfinished && s_live) atomicAdd(unfinished, s_live);
}

}  // namespace

#define JOINT_NEED(cond, msg) do { if (!(cond)) ASR_FAIL(h, ASR_ERR_INVALID_ARG, msg); } while (0)

extern "C" int asr_log_softmax_rows(asr_handle* h, const float* x, float* y, size_t rows, int cols, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  JOINT_NEED(x && y && rows >= 1 && cols >= 1 && (rows + 3) / 4 <= 0x7fffffffULL, "asr_log_softmax_rows: bad arguments");
  hipLaunchKernelGGL(log_softmax_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)s, x, y,
                     (long long)rows, cols);
  ASR_CHECK_LAUNCH(h, "asr_log_softmax_rows");
  return ASR_OK;
}

static int joint_shape_ok(int B, int W, int T, int By, int Cc, int blank, int N) {
  return B >= 1 && W >= 1 && W <= JOINT_MAX_W && T >= 1 && By >= B && N >= 1 && N < Cc && blank >= N && blank < Cc;
}

extern "C" int asr_ctc_prefix_init(asr_handle* h, const float* y, const int32_t* seq_len, int B, int W, int T, int By, int Cc,
                                   int blank, float* r, int32_t* last, float* ctc_score, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  JOINT_NEED(y && seq_len && r, "asr_ctc_prefix_init: null");
  JOINT_NEED(joint_shape_ok(B, W, T, By, Cc, blank, 1), "asr_ctc_prefix_init: bad shape");
  const int R = B * W;
  hipLaunchKernelGGL(ctc_prefix_init_kernel, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)s, y, seq_len, R, W, T, By, Cc,
                     blank, r, last, ctc_score);
  ASR_CHECK_LAUNCH(h, "asr_ctc_prefix_init");
  return ASR_OK;
}

extern "C" int asr_ctc_prefix_score(asr_handle* h, const float* y, const int32_t* seq_len, int B, int W, int T, int By, int Cc,
                                    int blank, int n_labels, const float* r, const int32_t* last, const int32_t* finished,
                                    const int32_t* cand, int K, float* psi, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  JOINT_NEED(y && seq_len && r && last && cand && psi, "asr_ctc_prefix_score: null");
  JOINT_NEED(joint_shape_ok(B, W, T, By, Cc, blank, n_labels), "asr_ctc_prefix_score: bad shape");
  JOINT_NEED(K >= 1 && K <= 64, "asr_ctc_prefix_score: 1 .. 64 candidates per row");
  h->att_joint_counts[0] += 1;
  hipLaunchKernelGGL(ctc_prefix_score_kernel, dim3(B * W), dim3(64), 0, (hipStream_t)s, y, seq_len, r, last, finished, cand, W,
                     K, T, By, Cc, blank, n_labels, psi);
  ASR_CHECK_LAUNCH(h, "asr_ctc_prefix_score");
  return ASR_OK;
}

extern "C" int asr_ctc_prefix_advance(asr_handle* h, const float* y, const int32_t* seq_len, int B, int W, int T, int By,
                                      int Cc, int blank, int n_labels, const float* r_src, const int32_t* last_src,
                                      const int32_t* parent, const int32_t* word, float* r_dst, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  JOINT_NEED(y && seq_len && r_src && last_src && parent && word && r_dst, "asr_ctc_prefix_advance: null");
  JOINT_NEED(joint_shape_ok(B, W, T, By, Cc, blank, n_labels), "asr_ctc_prefix_advance: bad shape");
  JOINT_NEED(r_src != r_dst, "asr_ctc_prefix_advance: the extension is out of place");
  h->att_joint_counts[1] += 1;
  hipLaunchKernelGGL(ctc_prefix_advance_kernel, dim3(B * W), dim3(64), 0, (hipStream_t)s, y, seq_len, r_src, last_src, parent,
                     word, W, T, By, Cc, blank, n_labels, r_dst);
  ASR_CHECK_LAUNCH(h, "asr_ctc_prefix_advance");
  return ASR_OK;
}

extern "C" int asr_att_beam_select_joint(asr_handle* h, const float* logits, int B, int W, int n_labels, float lpw,
                                         float ctc_weight, int first_step, const float* y, const int32_t* seq_len, int T, int By,
                                         int Cc, int blank, const float* r, const float* lp_in, const int32_t* fin_in,
                                         const int32_t* len_in, const int32_t* last_in, const float* ctc_in, int32_t* cand,
                                         float* cand_total, float* psi, int32_t* word, int32_t* parent, float* score,
                                         float* lp_out, int32_t* fin_out, int32_t* len_out, int32_t* last_out, float* ctc_out,
                                         int32_t* unfinished, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  JOINT_NEED(logits && y && seq_len && r && lp_in && fin_in && len_in && last_in && ctc_in && cand && cand_total && psi &&
                 word && parent && score && lp_out && fin_out && len_out && last_out && ctc_out,
             "asr_att_beam_select_joint: null");
  JOINT_NEED(joint_shape_ok(B, W, T, By, Cc, blank, n_labels), "asr_att_beam_select_joint: bad shape");
  JOINT_NEED(W <= n_labels + 1, "asr_att_beam_select_joint: beam width exceeds the labels and <EOS> step 0 selects among");
  JOINT_NEED(ctc_weight > 0.f && ctc_weight <= 1.f, "asr_att_beam_select_joint: ctc_weight must be in (0, 1]");
  const int C2 = n_labels + 2, eos = n_labels + 1;
  JOINT_NEED((long long)W * C2 <= 0x7fffffffLL, "asr_att_beam_select_joint: flat index overflow");
  hipStream_t st = (hipStream_t)s;
  h->att_joint_counts[2] += 1;
  hipLaunchKernelGGL(att_joint_candidates_kernel, dim3(B * W), dim3(64), 0, st, logits, W, C2, eos, first_step, lp_in, fin_in,
                     cand, cand_total);
  ASR_CHECK_LAUNCH(h, "asr_att_beam_select_joint(candidates)");
  const int rc = asr_ctc_prefix_score(h, y, seq_len, B, W, T, By, Cc, blank, n_labels, r, last_in, fin_in, cand, W + 1, psi, s);
  if (rc != ASR_OK) return rc;
  hipLaunchKernelGGL(att_joint_rank_kernel, dim3(B), dim3(256), 0, st, cand, cand_total, psi, W, C2, eos, lpw, ctc_weight,
                     fin_in, len_in, last_in, ctc_in, word, parent, score, lp_out, fin_out, len_out, last_out, ctc_out,
                     unfinished);
  ASR_CHECK_LAUNCH(h, "asr_att_beam_select_joint(rank)");
  return ASR_OK;
}

extern "C" int asr_att_joint_counts(asr_handle* h, unsigned long long* out3) {
  if (!h || !out3) return ASR_ERR_INVALID_ARG;
  for (int i = 0; i < 3; ++i) out3[i] = h->att_joint_counts[i];
  return ASR_OK;
}
extern "C" int asr_reset_att_joint_counts(asr_handle* h) {
  if (!h) return ASR_ERR_INVALID_ARG;
  for (int i = 0; i < 3; ++i) h->att_joint_counts[i] = 0;
  return ASR_OK;
}
