// The CTC prefix scorer of the one-pass joint CTC / attention beam search (Watanabe et al. 2017, Hori et al. 2017): the CTC
// prefix scores of the candidates of a beam search step and the state they are computed from.  The selection by fused
// score that runs it between its two kernels is asr_att_beam_select_joint / _fused (att_beam.hip).  The float64 statement
// is models/attention/decoders/beam_search/ctc_prefix_score.py; the loops that issue these are asr_att_decoder_beam_joint
// and asr_att_decoder_beam_lm (dec_loop.hip).
//
// Vocabularies: attention classes C2 = N + 2 (labels, <SOS> = N, <EOS> = N + 1); CTC classes Cc = N + 1 (blank = N by
// default).  y [T, By, Cc] are log-posteriors (asr_log_softmax_rows of the CTC head's logits); device row r = b*W + w reads
// utterance b = r / W, the posteriors are not tiled.  State r [R, 2, T] fp32: r[row, 0, t] = r_n[t], r[row, 1, t] = r_b[t],
// written and read for t < seq_len[b] only.
#include "common.h"
#include <math.h>

namespace {

constexpr int JOINT_MAX_W = 32;
constexpr int JOINT_CH = 64;                                // frames per chunk: one per lane

// log(exp(a) + exp(b)); -inf for two -inf (never NaN: +inf does not occur)
__device__ __forceinline__ float lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log1pf(expf(fminf(a, b) - m));
}

// One wave per row: out = x - (max + log(sum exp(x - max))).  Lane l takes the columns l, l + 64, ... in ascending order
// into a running maximum / sum, the 64 partials meet in a butterfly (xor 32 .. 1): the order of row_lse (att_beam.hip).
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

}  // namespace

extern "C" int asr_log_softmax_rows(asr_handle* h, const float* x, float* y, size_t rows, int cols, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(x && y && rows >= 1 && cols >= 1 && (rows + 3) / 4 <= 0x7fffffffULL, "asr_log_softmax_rows: bad arguments");
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
  ASR_NEED(y && seq_len && r, "asr_ctc_prefix_init: null");
  ASR_NEED(joint_shape_ok(B, W, T, By, Cc, blank, 1), "asr_ctc_prefix_init: bad shape");
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
  ASR_NEED(y && seq_len && r && last && cand && psi, "asr_ctc_prefix_score: null");
  ASR_NEED(joint_shape_ok(B, W, T, By, Cc, blank, n_labels), "asr_ctc_prefix_score: bad shape");
  ASR_NEED(K >= 1 && K <= 64, "asr_ctc_prefix_score: 1 .. 64 candidates per row");
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
  ASR_NEED(y && seq_len && r_src && last_src && parent && word && r_dst, "asr_ctc_prefix_advance: null");
  ASR_NEED(joint_shape_ok(B, W, T, By, Cc, blank, n_labels), "asr_ctc_prefix_advance: bad shape");
  ASR_NEED(r_src != r_dst, "asr_ctc_prefix_advance: the extension is out of place");
  h->att_joint_counts[1] += 1;
  hipLaunchKernelGGL(ctc_prefix_advance_kernel, dim3(B * W), dim3(64), 0, (hipStream_t)s, y, seq_len, r_src, last_src, parent,
                     word, W, T, By, Cc, blank, n_labels, r_dst);
  ASR_CHECK_LAUNCH(h, "asr_ctc_prefix_advance");
  return ASR_OK;
}

ASR_DEFINE_COUNTS(att_joint_counts, att_joint_counts)
