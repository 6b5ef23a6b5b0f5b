// CTC prefix beam search with shallow fusion of an RNN language model and an insertion bonus, on gfx950.
//
// EXTENSION.  The reference wanted it and has none: its CTC BeamSearchDecoder.__call__ takes `alpha` ("language model
// weight") and `beta` ("insertion bonus") (models/ctc/decoders/beam_search_decoder.py:53,61-62), carries
// `# TODO: add LM score here` (:132) and ships an empty models/ctc/decoders/charlm_beam_search_decoder.py.  The float64
// statement is this package's models/ctc/decoders/charlm_beam_search_decoder.py: the reference's loop (:53-152, same dict,
// same vocab-major insertion order, same stable sort) in which every EXTENSION of `prefix` by a class c != blank uses
//     p_t + alpha * log p_lm(c | <SOS>, prefix) + beta
// in place of p_t (the c != prefix_end branch and the c == prefix_end / p_b-only branch); the blank update and the merging
// case (the unchanged prefix collecting p_nb + p_t) get neither term.  The LM factor depends on the resulting prefix alone,
// so dict merging stays consistent.
//
// beam.hip searches a whole utterance in one launch; here the LM has to step between the frames, so the search is cut into
// one launch per frame, one workgroup per utterance, with the beam persistent in the workspace: the trie (parent, label),
// and per entry the 64-bit prefix hash, its parent's hash, length, last label, fp64 p_b / p_nb and the fp32 LM total.
// The hash, the orderable keys, the tie index and the fp64 log-softmax are beam.hip's, operation for operation (512 threads,
// the same strides and butterflies): with alpha == 0 and beta == 0 the result is asr_ctc_beam_decode's bit for bit.
//
// Frame kernel, for an utterance with t < seq_len[b] (others only write parent = slot, word = -1):
//   1. lp = log_softmax(logits[t, b, :]) in fp64 (LDS);
//   2. per live entry j: z_j = fp64 log-sum-exp of its fp32 LM logits row [V] (a wave per entry; converted, then reduced in
//      fp64), so that log p_lm(c | prefix_j) = (double)row_j[c] - z_j;
//   3. the nb stay candidates (blank update + merging case, no LM term; plus, when the entry's parent prefix is in the beam,
//      the parent's extension by the entry's last label WITH the parent's LM term: the extension that lands on a prefix of
//      the beam), then the nb x C extension totals  base_j(c) + ((lp[c] + alpha * log p_lm_j(c)) + beta),
//      base_j(c) = p_b if c == last_j else logsumexp(p_b, p_nb); blank and the merged pairs are masked out;
//   4. exact top-W by (orderable fp64 total, ~insertion index), the composite key of beam.hip, so ties resolve as the
//      reference's stable sort: a threshold at or below the W-th largest key from the 32 sixteen-lane rows' maxima, the
//      candidates at or above it ("contenders", usually a few times W) ranked by counting; when more than 512 contend
//      (ties at the threshold) W rounds of a block-wide arg-max over per-thread running maxima instead;
//   5. per new slot: parent_slot, word (the appended label, -1 for a stay), the new entry, a new trie node for an extension.
// Pruning: none.  beam.hip's class / pair pruning assumes that every entry sees the same class scores, which no longer
// holds; every (entry, class) pair is a candidate here -- W x C keys, 1.3 k at C = 62 / W = 20 -- so the search is exact by
// construction.  The keys live in LDS when they fit (<= 88 KB), else in the workspace.
//
// asr_ctc_beam_decode_lm, launch order on the one stream (the host never synchronises): asr_lm_prep; asr_lm_step (the empty
// prefix's distribution; the logits go to buffer 0); then per frame t = 0 .. T-1: the frame kernel reading buffer t % 2,
// and, unless t == T-1, asr_lm_beam_reorder (state block 1 -> block 0 by parent_slot, x = embedding of word),
// asr_lm_step (block 0 -> block 1, logits into buffer (t + 1) % 2) and the commit kernel: a row whose word is -1 did not
// move -- it takes the gathered state back (block 0 -> block 1) and its parent's logits row from the other buffer (out of
// place: several rows may read one parent row).  Last the back-trace kernel.  T frame launches, T LM steps, T - 1 commits.
#include "common.h"
#include "beam_keys.h"
#include <math.h>

namespace {

constexpr int LMB_MAX_W = 32;     // asr_lm_beam_reorder's limit
constexpr int LMB_NT = 512;       // beam.hip's default workgroup: the log-softmax reduces in the same order
constexpr int LMB_CONT = 512;     // contenders the ranking of step 4 holds (<= LMB_NT: one thread each)

struct LmEntry {           // one beam entry, as it lies in the workspace between the frames
  double pb, pnb;
  unsigned long long hash, phash;   // hash of the prefix / of its parent prefix
  int node, len, last;
  float lm;                         // sum of log p_lm over the prefix' labels
};

// composite order of two candidates: (key, tie index), larger first
__device__ __forceinline__ bool comp_before(unsigned long long k, unsigned n, unsigned long long ok, unsigned on) {
  return k > ok || (k == ok && n > on);
}

__global__ __launch_bounds__(LMB_NT) void ctc_beam_lm_frame_kernel(
    const float* __restrict__ logits, int t, int T, int B, int C, const int32_t* __restrict__ seq_len, int blank, int W,
    double alpha, double beta, const float* __restrict__ lm_logits, int V, LmEntry* __restrict__ ent_ws,
    int32_t* __restrict__ meta_ws, int2* __restrict__ node_ws, unsigned long long* __restrict__ key_ws, int keys_in_lds,
    int32_t* __restrict__ parent_out, int32_t* __restrict__ word_out, double* __restrict__ st_pb, double* __restrict__ st_pnb,
    float* __restrict__ st_lm, int32_t* __restrict__ st_nb) {
  constexpr int NT = LMB_NT, NW = NT / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* lp = reinterpret_cast<double*>(smem);                                                   // [C]
  unsigned long long* lkeys = reinterpret_cast<unsigned long long*>(smem + (((size_t)C * 8 + 15) & ~(size_t)15));
  __shared__ LmEntry beam[LMB_MAX_W];
  __shared__ double s_L[LMB_MAX_W], s_pb[LMB_MAX_W], s_pnb[LMB_MAX_W], s_z[LMB_MAX_W];
  __shared__ unsigned long long s_key[LMB_MAX_W], w_key[LMB_MAX_W];
  __shared__ unsigned s_idx[LMB_MAX_W];
  __shared__ int s_parent[LMB_MAX_W], w_id[LMB_MAX_W];
  __shared__ double red[NW];
  __shared__ unsigned long long r_key[2][NW];
  __shared__ unsigned r_nidx[2][NW];
  __shared__ int r_id[2][NW];
  __shared__ unsigned long long g_key[NT / 16], s_tau[2];    // the 16-lane rows' largest keys; [0]: the contenders' threshold
  __shared__ int s_cnt[4];                                   // [0]: contenders
  __shared__ unsigned long long c_key[LMB_CONT];
  __shared__ unsigned c_n[LMB_CONT];
  __shared__ int c_id[LMB_CONT];

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = min(max(seq_len[b], 0), T);
  LmEntry* ent = ent_ws + (size_t)b * W;
  int32_t* meta = meta_ws + (size_t)b * 2;                  // {entries in the beam, trie nodes}
  int2* nodes = node_ws + (size_t)b * ((size_t)T * W + 1);
  unsigned long long* ck = keys_in_lds ? lkeys : key_ws + (size_t)b * ((size_t)W * C + W);

  if (t == 0 && tid == 0) {                                  // the empty prefix (also what a 0-frame utterance ends with)
    LmEntry e;
    e.pb = 0.0; e.pnb = DNEG; e.hash = 0x1234567ull; e.phash = 0; e.node = 0; e.len = 0; e.last = -1; e.lm = 0.f;
    ent[0] = e;
    nodes[0] = make_int2(-1, -1);
    meta[0] = 1; meta[1] = 1;
  }
  if (t >= Tb) {                                             // (block-uniform) nothing moves: every slot keeps its LM row
    if (tid < W) { parent_out[(size_t)b * W + tid] = tid; word_out[(size_t)b * W + tid] = -1; }
    return;
  }
  const int nb = t == 0 ? 1 : meta[0];
  const int n_nodes = t == 0 ? 1 : meta[1];
  if (tid < nb) {
    if (t == 0) {
      LmEntry e;
      e.pb = 0.0; e.pnb = DNEG; e.hash = 0x1234567ull; e.phash = 0; e.node = 0; e.len = 0; e.last = -1; e.lm = 0.f;
      beam[0] = e;
    } else {
      beam[tid] = ent[tid];
    }
  }
  // ---- 1. fp64 log-softmax of the frame (beam.hip's order: float maximum, strided fp64 sums, butterfly, waves in order)
  const float* row = logits + ((size_t)t * B + b) * C;
  float m = -INFINITY;
  for (int c = tid; c < C; c += NT) {
    const float x = row[c];
    lp[c] = (double)x;
    m = fmaxf(m, x);
  }
  m = wave_reduce_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  double mm = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) mm = fmax(mm, red[w]);
  __syncthreads();
  double ssum = 0.0;
  for (int c = tid; c < C; c += NT) ssum += exp(lp[c] - mm);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ssum += __shfl_xor(ssum, o, 64);
  if (lane == 0) red[wave] = ssum;
  __syncthreads();
  double zs = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) zs += red[w];
  const double z = mm + log(zs);
  for (int c = tid; c < C; c += NT) lp[c] = lp[c] - z;
  // ---- 2. the LM rows' normalisers, a wave per live entry: fp32 logits converted, maximum and sum in fp64
  const bool use_lm = lm_logits != nullptr;
  if (use_lm) {
    for (int j = wave; j < nb; j += NW) {
      const float* lr = lm_logits + ((size_t)b * W + j) * V;
      double mx = DNEG;
      for (int c = lane; c < V; c += 64) mx = fmax(mx, (double)lr[c]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
      double sm = 0.0;
      for (int c = lane; c < V; c += 64) sm += exp((double)lr[c] - mx);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
      if (lane == 0) s_z[j] = mx + log(sm);
    }
  }
  if (tid < LMB_MAX_W) s_parent[tid] = -1;
  __syncthreads();
  // log p_lm of class c after entry j's prefix, and what an extension uses in place of p_t
  auto lm_lp = [&](int j, int c) -> double {
    return use_lm ? (double)lm_logits[((size_t)b * W + j) * V + c] - s_z[j] : 0.0;
  };
  auto fused_pt = [&](int j, int c) -> double { return (lp[c] + alpha * lm_lp(j, c)) + beta; };
  // ---- 3a. parent lookup + stay candidates (beam.hip step 2; the extension that lands on a beam prefix carries the LM term)
  if (tid < nb) {
    const unsigned long long eph = beam[tid].phash;
    const int elen = beam[tid].len;
    int par = -1;
    for (int j = nb - 1; j >= 0; --j)                        // the first (lowest) entry that spells the parent prefix
      if (beam[j].hash == eph && beam[j].len + 1 == elen) par = j;
    s_parent[tid] = par;
    const LmEntry e = beam[tid];
    const double lpb = lp[blank];
    const double pb = lse3d(DNEG, e.pb + lpb, e.pnb + lpb);
    double pnb = DNEG;
    unsigned first = (unsigned)blank * (2u * W) + 2u * tid;
    if (e.len > 0) {
      const double lpl = lp[e.last];
      double from_parent = DNEG;
      if (par >= 0) {
        const LmEntry p = beam[par];
        const double ptp = fused_pt(par, e.last);
        from_parent = (e.last == p.last) ? p.pb + ptp : lse2d(p.pb, p.pnb) + ptp;
      }
      const double own = e.pnb + lpl;
      if (par >= 0 && par < tid) pnb = lse2d(lse2d(DNEG, from_parent), own);   // dict order
      else if (par >= 0) pnb = lse2d(lse2d(DNEG, own), from_parent);
      else pnb = own;
      if (e.last != blank) {
        unsigned a = (unsigned)e.last * (2u * W) + 2u * tid + 1u;
        if (par >= 0) a = min(a, (unsigned)e.last * (2u * W) + 2u * par);
        first = min(first, a);
      }
    }
    s_pb[tid] = pb; s_pnb[tid] = pnb;
    s_key[tid] = okey(lse2d(pb, pnb));
    s_idx[tid] = ~first;
    s_L[tid] = lse2d(e.pb, e.pnb);
  }
  __syncthreads();
  // ---- 3b. candidate keys: [0, nb) the stays, then class-major nb + c * nb + j = entry j extended by class c; 0 = excluded
  const int M = nb + nb * C;
  if (tid < nb) ck[tid] = s_key[tid];
  {
    int c = tid / nb, j = tid - c * nb;
    const int dc = NT / nb, dj = NT - dc * nb;
    for (int e = tid; e < nb * C; e += NT) {
      unsigned long long k = 0ull;
      if (c != blank) k = okey(((c == beam[j].last) ? beam[j].pb : s_L[j]) + fused_pt(j, c));
      ck[nb + e] = k;
      c += dc; j += dj;
      if (j >= nb) { j -= nb; ++c; }
    }
  }
  __syncthreads();
  if (tid < nb && s_parent[tid] >= 0 && beam[tid].last != blank)             // merged pairs are not new prefixes
    ck[nb + beam[tid].last * nb + s_parent[tid]] = 0ull;
  __syncthreads();
  // ---- 4. exact top-W by (key, tie index).
  auto nidx_of = [&](int id) -> unsigned {
    if (id < nb) return s_idx[id];
    const int e = id - nb, c = e / nb, j = e - c * nb;
    return ~((unsigned)c * (2u * W) + 2u * j);
  };
  // 4a. a threshold at or below the W-th largest key: the NT / 16 = 32 rows of 16 lanes each name their largest key --
  //     32 distinct candidates -- and the W-th largest of those (W <= 32) has W candidates at or above it.  Fewer than W
  //     rows with a candidate: no threshold (0), everything contends.
  {
    unsigned long long mk = 0ull;
    for (int id = tid; id < M; id += NT) {
      const unsigned long long k = ck[id];
      mk = k > mk ? k : mk;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const unsigned long long ok = __shfl_xor(mk, o, 64);
      mk = ok > mk ? ok : mk;
    }
    if ((lane & 15) == 0) g_key[tid >> 4] = mk;
    if (tid == 0) { s_tau[0] = 0ull; s_cnt[0] = 0; }
  }
  __syncthreads();
  if (tid < NT / 16) {
    const unsigned long long mine = g_key[tid];
    int above = 0;                                           // rows before this one in the strict order (key, lower row)
#pragma unroll 8
    for (int j = 0; j < NT / 16; ++j) {
      const unsigned long long kj = g_key[j];
      above += (int)((kj > mine) | ((kj == mine) & (j < tid)));
    }
    if (mine != 0ull && above == W - 1) s_tau[0] = mine;     // (exactly one row, if any)
  }
  __syncthreads();
  // 4b. the contenders (key >= threshold: a superset of the top W, ties included) are ranked by counting, a thread each;
  //     composite keys are distinct, so are the ranks, and rank r < W is the new slot r.  The order the contenders land in
  //     is arbitrary (an atomic counter) and does not matter.
  {
    const unsigned long long tau = s_tau[0];
    for (int id = tid; id < M; id += NT) {
      const unsigned long long k = ck[id];
      if (k != 0ull && k >= tau) {
        const int pos = atomicAdd(&s_cnt[0], 1);
        if (pos < LMB_CONT) { c_key[pos] = k; c_n[pos] = nidx_of(id); c_id[pos] = id; }
      }
    }
  }
  __syncthreads();
  const int nc = s_cnt[0];
  int nw = 0;
  if (nc <= LMB_CONT) {                                      // (block-uniform)
    nw = min(W, nc);
    if (tid < nc) {
      const unsigned long long k = c_key[tid];
      const unsigned n = c_n[tid];
      int rank = 0;
#pragma unroll 4
      for (int j = 0; j < nc; ++j) rank += (int)comp_before(c_key[j], c_n[j], k, n);
      if (rank < W) { w_key[rank] = k; w_id[rank] = c_id[tid]; }
    }
  } else {
    // 4c. more contenders than that (ties at the threshold: flat or quantised posteriors): W rounds of a block-wide arg-max.
    //     A thread keeps the best of its share (ids tid, tid + NT, ...); per round the block's best wins, its owner drops it
    //     and rescans.  One barrier per round (the exchange arrays alternate).
    unsigned long long bk = 0ull;
    unsigned bn = 0u;
    int bi = -1;
    auto rescan = [&]() {
      bk = 0ull; bn = 0u; bi = -1;
      for (int id = tid; id < M; id += NT) {
        const unsigned long long k = ck[id];
        if (k == 0ull || k < bk) continue;
        const unsigned n = nidx_of(id);
        if (bi < 0 || comp_before(k, n, bk, bn)) { bk = k; bn = n; bi = id; }
      }
    };
    rescan();
    for (int r = 0; r < W; ++r) {
      unsigned long long k = bk;
      unsigned n = bn;
      int id = bi;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ok = __shfl_xor(k, o, 64);
        const unsigned on = __shfl_xor(n, o, 64);
        const int oid = __shfl_xor(id, o, 64);
        if (oid >= 0 && (id < 0 || comp_before(ok, on, k, n))) { k = ok; n = on; id = oid; }
      }
      const int p = r & 1;
      if (lane == 0) { r_key[p][wave] = k; r_nidx[p][wave] = n; r_id[p][wave] = id; }
      __syncthreads();
      k = r_key[p][0]; n = r_nidx[p][0]; id = r_id[p][0];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const unsigned long long ok = r_key[p][w];
        const unsigned on = r_nidx[p][w];
        const int oid = r_id[p][w];
        if (oid >= 0 && (id < 0 || comp_before(ok, on, k, n))) { k = ok; n = on; id = oid; }
      }
      if (id < 0) break;                                     // (block-uniform) fewer than W valid candidates
      if (tid == 0) { w_key[r] = k; w_id[r] = id; }
      nw = r + 1;
      if (id == bi) {                                        // composite keys are distinct: exactly one owner
        ck[id] = 0ull;
        rescan();
      }
    }
  }
  __syncthreads();
  // ---- 5. the next beam, in rank order; a new trie node per extension (ids n_nodes + rank: stays leave gaps)
  if (tid < W) {
    int pa = 0, wd = -1;
    if (tid < nw) {
      const int id = w_id[tid];
      LmEntry ne;
      if (id < nb) {
        ne = beam[id];
        ne.pb = s_pb[id]; ne.pnb = s_pnb[id];
        pa = id;
      } else {
        const int e = id - nb, c = e / nb, j = e - c * nb;
        const LmEntry p = beam[j];
        ne.pb = DNEG; ne.pnb = unokey(w_key[tid]);           // the key IS the total (order-preserving bijection)
        ne.phash = p.hash; ne.hash = hmix(p.hash, c);
        ne.len = p.len + 1; ne.last = c;
        ne.lm = p.lm + (float)lm_lp(j, c);
        ne.node = n_nodes + tid;
        nodes[ne.node] = make_int2(p.node, c);
        pa = j; wd = c;
      }
      ent[tid] = ne;
      if (st_pb) st_pb[(size_t)b * W + tid] = ne.pb;
      if (st_pnb) st_pnb[(size_t)b * W + tid] = ne.pnb;
      if (st_lm) st_lm[(size_t)b * W + tid] = ne.lm;
    }
    parent_out[(size_t)b * W + tid] = pa;
    word_out[(size_t)b * W + tid] = wd;
  }
  if (tid == 0) {
    meta[0] = nw; meta[1] = n_nodes + nw;
    if (st_nb) st_nb[b] = nw;
  }
}

// A row whose prefix did not grow (word == -1) keeps what its parent slot had: the gathered state (block 0, where
// asr_lm_beam_reorder put it) goes back to block 1 and the parent's logits row comes over from the other buffer.  Rows that
// grew were written by asr_lm_step.  One workgroup per row r = b*W + w.
__global__ __launch_bounds__(256) void ctc_beam_lm_commit_kernel(
    const int32_t* __restrict__ parent, const int32_t* __restrict__ word, int R, int W, int L, int H, int V,
    const float* __restrict__ c0, const float* __restrict__ h0, float* __restrict__ c1, float* __restrict__ h1,
    const float* __restrict__ z_src, float* __restrict__ z_dst) {
  const int r = blockIdx.x, tid = threadIdx.x;
  if (word[r] >= 0) return;
  int pa = parent[r];
  pa = pa < 0 ? 0 : (pa >= W ? W - 1 : pa);                  // (bounds only: the frame kernel writes 0 .. W-1)
  const size_t pr = (size_t)(r / W) * W + pa;
  for (int l = 0; l < L; ++l) {
    const size_t o = ((size_t)l * R + r) * H;
    for (int j = tid; j < H; j += 256) { c1[o + j] = c0[o + j]; h1[o + j] = h0[o + j]; }
  }
  for (int j = tid; j < V; j += 256) z_dst[(size_t)r * V + j] = z_src[pr * V + j];
}

// best hypothesis = entry 0; walk the trie back
__global__ __launch_bounds__(64) void ctc_beam_lm_backtrace_kernel(
    int T, int W, const LmEntry* __restrict__ ent_ws, const int2* __restrict__ node_ws, int32_t* __restrict__ out_labels,
    int32_t* __restrict__ out_len, double* __restrict__ out_score, float* __restrict__ out_lm) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const LmEntry e = ent_ws[(size_t)b * W];
  const int2* nodes = node_ws + (size_t)b * ((size_t)T * W + 1);
  const int n = min(max(e.len, 0), T);
  for (int i = n + tid; i < T; i += 64) out_labels[(size_t)b * T + i] = -1;
  if (tid == 0) {
    int node = e.node;
    for (int i = n - 1; i >= 0; --i) {
      const int2 nd = nodes[node];
      out_labels[(size_t)b * T + i] = nd.y;
      node = nd.x;
    }
    out_len[b] = n;
    out_score[b] = -lse2d(e.pb, e.pnb);
    if (out_lm) out_lm[b] = e.lm;
  }
}

struct LmBeamWs { size_t ent, meta, nodes, keys, parent, word, z, total; };
inline LmBeamWs lmb_ws_layout(int T, int B, int C, int W, int V) {
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  LmBeamWs w;
  size_t o = 0;
  w.ent = o;    o += al((size_t)B * W * sizeof(LmEntry));
  w.meta = o;   o += al((size_t)B * 2 * sizeof(int32_t));
  w.nodes = o;  o += al((size_t)B * ((size_t)T * W + 1) * sizeof(int2));
  w.keys = o;   o += al((size_t)B * ((size_t)W * C + W) * sizeof(unsigned long long));   // when they do not fit in LDS
  w.parent = o; o += al((size_t)B * W * sizeof(int32_t));
  w.word = o;   o += al((size_t)B * W * sizeof(int32_t));
  w.z = o;      o += al((size_t)2 * B * W * (size_t)(V > 0 ? V : 0) * sizeof(float));    // the two LM logits buffers
  w.total = o;
  return w;
}

constexpr size_t LMB_LDS_KEYS = 88 * 1024;      // beside lp (<= 48 KB) and ~13 KB of static arrays: under 160 KB

int lmb_check(asr_handle* h, const char* who, const float* logits, int T, int B, int C, const int32_t* seq_len, int blank,
              int W, double alpha, double beta) {
  if (!logits || !seq_len || T <= 0 || B <= 0 || C < 2 || blank < 0 || blank >= C || W < 1 || !(alpha == alpha) ||
      !(beta == beta) || isinf(alpha) || isinf(beta))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: bad args T=%d B=%d C=%d beam=%d", who, T, B, C, W);
  if (W > LMB_MAX_W || W > C - 1)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: beam_width %d outside 1 .. min(%d, C - 1 = %d)", who, W, LMB_MAX_W, C - 1);
  if ((size_t)C * 8 > 48 * 1024) ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "%s: C=%d too large for LDS", who, C);
  return ASR_OK;
}

// dynamic LDS of the frame kernel: lp [C] and, when they fit, the W C + W candidate keys
struct LmbLds { size_t bytes; int keys_in_lds; };
LmbLds lmb_lds(int C, int W) {
  const size_t lds_c = ((size_t)C * 8 + 15) & ~(size_t)15;
  const size_t key_bytes = ((size_t)W * C + W) * 8;
  LmbLds l;
  l.keys_in_lds = key_bytes <= LMB_LDS_KEYS ? 1 : 0;
  l.bytes = lds_c + (l.keys_in_lds ? key_bytes : 0);
  return l;
}
// once per call, not per frame: the attribute is a host-side driver call
void lmb_allow_lds(int C, int W) {
  (void)hipFuncSetAttribute((const void*)ctc_beam_lm_frame_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lmb_lds(C, W).bytes);
}

int lmb_launch_frame(asr_handle* h, const float* logits, int t, int T, int B, int C, const int32_t* seq_len, int blank, int W,
                     double alpha, double beta, const float* lm_logits, int V, char* ws, const LmBeamWs& w, int32_t* parent,
                     int32_t* word, double* st_pb, double* st_pnb, float* st_lm, int32_t* st_nb, hipStream_t st) {
  const size_t lds = lmb_lds(C, W).bytes;
  const int in_lds = lmb_lds(C, W).keys_in_lds;
  h->ctc_beam_lm_counts[0] += 1;
  hipLaunchKernelGGL(ctc_beam_lm_frame_kernel, dim3(B), dim3(LMB_NT), lds, st, logits, t, T, B, C, seq_len, blank, W, alpha,
                     beta, lm_logits, V, (LmEntry*)(ws + w.ent), (int32_t*)(ws + w.meta), (int2*)(ws + w.nodes),
                     (unsigned long long*)(ws + w.keys), in_lds, parent, word, st_pb, st_pnb, st_lm, st_nb);
  ASR_CHECK_LAUNCH(h, "asr_ctc_beam_lm_frame");
  return ASR_OK;
}

}  // namespace

extern "C" size_t asr_ctc_beam_lm_workspace_bytes(int T, int B, int C, int beam_width, int V) {
  if (T < 0 || B < 0 || C < 1 || beam_width < 1 || V < 0) return 0;
  return lmb_ws_layout(T, B, C, beam_width, V).total;
}

extern "C" int asr_ctc_beam_lm_frame(asr_handle* h, const float* logits, int t, int T, int B, int C, const int32_t* seq_len,
                                     int blank, int beam_width, double alpha, double beta, const float* lm_logits, int V,
                                     int32_t* parent, int32_t* word, double* st_pb, double* st_pnb, float* st_lm,
                                     int32_t* st_nb, void* workspace, size_t workspace_bytes, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_TRY(lmb_check(h, "asr_ctc_beam_lm_frame", logits, T, B, C, seq_len, blank, beam_width, alpha, beta));
  if (!parent || !word || t < 0 || t >= T) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_beam_lm_frame: bad args t=%d", t);
  if (lm_logits ? V < C : alpha != 0.0)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_beam_lm_frame: alpha=%g needs LM logits rows of V >= C classes (V=%d)", alpha, V);
  const LmBeamWs w = lmb_ws_layout(T, B, C, beam_width, 0);
  if (!workspace || workspace_bytes < w.total)
    ASR_FAIL(h, ASR_ERR_WORKSPACE, "asr_ctc_beam_lm_frame: workspace %zu < %zu bytes", workspace_bytes, w.total);
  lmb_allow_lds(C, beam_width);
  return lmb_launch_frame(h, logits, t, T, B, C, seq_len, blank, beam_width, alpha, beta, lm_logits, V, (char*)workspace, w,
                          parent, word, st_pb, st_pnb, st_lm, st_nb, (hipStream_t)s);
}

extern "C" int asr_ctc_beam_decode_lm(asr_handle* h, const float* logits, int T, int B, int C, const int32_t* seq_len,
                                      int blank, int beam_width, double alpha, double beta, const asr_att_lm* lm,
                                      int32_t* out_labels, int32_t* out_len, double* out_score, float* out_lm_score,
                                      void* workspace, size_t workspace_bytes, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_TRY(lmb_check(h, "asr_ctc_beam_decode_lm", logits, T, B, C, seq_len, blank, beam_width, alpha, beta));
  if (!out_labels || !out_len || !out_score) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_beam_decode_lm: null output");
  const int W = beam_width, R = B * W;
  int V = 0;
  if (lm) {
    V = lm->C2;
    if (lm->R != R || V < C + 1 || lm->L < 1 || lm->H < 1 || lm->Em_lm < 1 || !lm->c || !lm->h || !lm->in || !lm->emb)
      ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_beam_decode_lm: the language model has R=%d rows, V=%d classes; need R=%d, V>=%d",
               lm->R, V, R, C + 1);
  } else if (alpha != 0.0) {
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_beam_decode_lm: alpha=%g without a language model", alpha);
  }
  const LmBeamWs w = lmb_ws_layout(T, B, C, W, V);
  if (!workspace || workspace_bytes < w.total)
    ASR_FAIL(h, ASR_ERR_WORKSPACE, "asr_ctc_beam_decode_lm: workspace %zu < %zu bytes", workspace_bytes, w.total);
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)s;
  int32_t* parent = (int32_t*)(ws + w.parent);
  int32_t* word = (int32_t*)(ws + w.word);
  float* zbuf[2] = {(float*)(ws + w.z), (float*)(ws + w.z) + (size_t)R * V};
  lmb_allow_lds(C, W);
  asr_att_lm step;
  if (lm) {
    step = *lm;
    step.lm_logits = zbuf[0];
    ASR_TRY(asr_lm_prep(h, &step, s));
    ASR_TRY(asr_lm_step(h, &step, s));                       // the empty prefix: <SOS> from the zero state
    h->ctc_beam_lm_counts[1] += 1;
  }
  const size_t blk = lm ? (size_t)lm->L * R * lm->H : 0;
  for (int t = 0; t < T; ++t) {
    ASR_TRY(lmb_launch_frame(h, logits, t, T, B, C, seq_len, blank, W, alpha, beta, lm ? zbuf[t & 1] : nullptr, V, ws, w,
                             parent, word, nullptr, nullptr, nullptr, nullptr, st));
    if (!lm || t == T - 1) continue;
    ASR_TRY(asr_lm_beam_reorder(h, parent, word, B, W, lm->L, lm->H, lm->Em_lm, V, lm->c + blk, lm->h + blk, lm->emb, lm->c,
                                lm->h, lm->in, s));
    step.lm_logits = zbuf[(t + 1) & 1];
    ASR_TRY(asr_lm_step(h, &step, s));
    h->ctc_beam_lm_counts[1] += 1;
    hipLaunchKernelGGL(ctc_beam_lm_commit_kernel, dim3(R), dim3(256), 0, st, parent, word, R, W, lm->L, lm->H, V, lm->c, lm->h,
                       lm->c + blk, lm->h + blk, zbuf[t & 1], zbuf[(t + 1) & 1]);
    ASR_CHECK_LAUNCH(h, "asr_ctc_beam_decode_lm(commit)");
    h->ctc_beam_lm_counts[2] += 1;
  }
  hipLaunchKernelGGL(ctc_beam_lm_backtrace_kernel, dim3(B), dim3(64), 0, st, T, W, (const LmEntry*)(ws + w.ent),
                     (const int2*)(ws + w.nodes), out_labels, out_len, out_score, out_lm_score);
  ASR_CHECK_LAUNCH(h, "asr_ctc_beam_decode_lm(backtrace)");
  return ASR_OK;
}

ASR_DEFINE_COUNTS(ctc_beam_lm_counts, ctc_beam_lm_counts)
