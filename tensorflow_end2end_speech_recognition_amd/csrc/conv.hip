// The implicit-GEMM convolutions of any tap geometry (conv_common.h: Taps) for gfx950, SAME padding, stride 1, over
// per-frame images [N, H, W, C] NHWC: the 3 (frequency) x 5 (time) conv_layer of the cnn_zhang encoder
// (models/encoders/core/cnn_zhang.py:41-174, after Zhang et al. 2017; cnn_util.py:50-84) with its max_pool [3,1] / [3,1]
// SAME (cnn_util.py:13-28), the 3x4 convolution of the student CNNs (asr_conv3x4_*), and the tiled forms of the VGG
// front-end's 3x3 (entry points and image-resident forms: conv3x3.hip).
//
// bf16 operands and fp32 accumulation (v_mfma_f32_16x16x32_bf16): the A tile is gathered straight from the image, one
// 64-wide k-tile = (one tap, 64 consecutive input channels) = 128 contiguous bytes of the shifted pixel, zero where the
// shifted pixel falls off the frame.  Through im2col + GEMM a 256-channel 3x5 layer would write and re-read a
// [pixels x 3840] patch matrix (15x its activation bytes); here no patch is ever stored, and the weight image of a layer
// (<= 1.9 MB) stays in L2.
//   forward        out[p, co] = act(sum_{tap, ci} x[p + s_tap, ci] Wf[co][tap Cin + ci] + bias[co])
//   data gradient  the same product on dOut with the flipped-tap image Wb (s_{ntaps - 1 - tap} = -s_tap for odd widths), the
//                  ReLU / dropout backward of the layer below in the epilogue (conv_gate_apply)
//   weight grad    dW[tap Cin + ci][co] = sum_p x[p + s_tap, ci] dOut[p, co]: pixel-range slabs in the scratch arena, then
//                  a fixed-order sum of the slabs (no float atomics: bitwise reproducible)
// s_tap = (tap / KW - OY, tap % KW - OX); 3x5: row (frequency) offset -1..1, column (time) offset -2..2.
#include "conv_common.h"
#include <limits.h>
#include <type_traits>

namespace {

// Implicit GEMM: Mpix x Cout x (TP::N Cin); 256 threads = 2 x 2 waves over a 128 x BN tile, k-tile 64, two LDS stages with
// the next k-tile's global loads in flight during the MFMAs.  Requires Cin % 64 == 0, Cout % BN == 0.
template <typename TO, int BN, typename TP>
__global__ __launch_bounds__(256) void conv_nt_kernel(int Mpix, int H, int W, int Cin, int Cout,
                                                      const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wt,
                                                      TO* __restrict__ Out, const float* __restrict__ bias, int act,
                                                      ConvGate gate) {
  constexpr int BM = 128, BK = 64, LD = BK + 8;
  constexpr int STAGE = (BM + BN) * LD;
  constexpr int WN = BN / 2, TN = WN / 16;
  constexpr int NB = BN * 8 / 256;                         // B vectors per thread per k-tile
  __shared__ __attribute__((aligned(16))) bf16_t S[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = Cout / BN;
  const int m0 = (blockIdx.x / ntn) * BM, n0 = (blockIdx.x % ntn) * BN;
  const int K = TP::N * Cin, nkt = K / BK, kpt = Cin / BK;
  const int HW = H * W;

  int py[4], px[4];
  const bf16_t* pa[4];
  unsigned so[4];
  bool mok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = tid + i * 256, r = v >> 3, kv = (v & 7) * 8;
    const int m = m0 + r;
    mok[i] = m < Mpix;
    const int mm = mok[i] ? m : 0;
    const int rem = mm % HW;
    py[i] = rem / W;
    px[i] = rem % W;
    pa[i] = X + (size_t)mm * Cin + kv;
    so[i] = (unsigned)(r * LD + kv);
  }
  const bf16_t* pb[NB];
  unsigned sob[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int v = tid + i * 256, r = v >> 3, kv = (v & 7) * 8;
    pb[i] = Wt + (size_t)(n0 + r) * K + kv;
    sob[i] = (unsigned)(BM * LD + r * LD + kv);
  }
  const bf16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8_t ra[4], rb[NB];
  auto gload = [&](int kt) {
    const int tap = kt / kpt, ci0 = (kt - tap * kpt) * BK;
    const int dy = tap / TP::KW - TP::OY, dx = tap - (tap / TP::KW) * TP::KW - TP::OX;
    const ptrdiff_t sh = ((ptrdiff_t)dy * W + dx) * Cin + ci0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = mok[i] && (unsigned)(py[i] + dy) < (unsigned)H && (unsigned)(px[i] + dx) < (unsigned)W;
      ra[i] = ok ? *reinterpret_cast<const bf16x8_t*>(pa[i] + sh) : zero;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) rb[i] = *reinterpret_cast<const bf16x8_t*>(pb[i] + (size_t)kt * BK);
  };
  auto sstore = [&](bf16_t* st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<bf16x8_t*>(st + so[i]) = ra[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) *reinterpret_cast<bf16x8_t*>(st + sob[i]) = rb[i];
  };

  f32x4_t acc[4][TN];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  gload(0);
  sstore(S);
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  const unsigned aoff = (unsigned)((wm * 64 + fr) * LD + fq * 8);
  const unsigned boff = (unsigned)(BM * LD + (wn * WN + fr) * LD + fq * 8);
  for (int kt = 0; kt < nkt; ++kt) {
    const bf16_t* cur = S + (kt & 1) * STAGE;
    if (kt + 1 < nkt) gload(kt + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t a[4], b[TN];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(cur + aoff + i * 16 * LD + ks * 32);
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(cur + boff + j * 16 * LD + ks * 32);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nkt) sstore(S + ((kt + 1) & 1) * STAGE);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + fr;
    if (m >= Mpix) continue;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nb = n0 + wn * WN + j * 16 + fq * 4;
      TO* cp = Out + (size_t)m * Cout + nb;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r];
      if (bias) {
        const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(bias + nb);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bv[r];
      }
      if (act) conv_gate_apply(act, gate, (size_t)m * Cout + nb, v);
      if constexpr (sizeof(TO) == 4) {
        *reinterpret_cast<f32x4_t*>(cp) = (f32x4_t){v[0], v[1], v[2], v[3]};
      } else {
        typedef __attribute__((ext_vector_type(4))) unsigned short us4_t;
        *reinterpret_cast<us4_t*>(cp) = (us4_t){f32_to_bf16(v[0]), f32_to_bf16(v[1]), f32_to_bf16(v[2]), f32_to_bf16(v[3])};
      }
    }
  }
}

// weight images from the HWIO fp32 master [KH][KW][Cin][Cout] (tap = kh * KW + kw, KTAPS = KH KW):
//   wf[co][tap Cin + ci] = w[tap][ci][co]                    (forward:   B^T of x * W)
//   wb[ci][(KTAPS - 1 - tap) Cout + co] = w[tap][ci][co]     (data grad: B^T of dOut * flipped W)
template <int KTAPS>
__global__ void conv_prep_kernel(const float* __restrict__ w, int Cin, int Cout, bf16_t* __restrict__ wf,
                                 bf16_t* __restrict__ wb) {
  const size_t total = (size_t)KTAPS * Cin * Cout;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int co = i % Cout, ci = (i / Cout) % Cin, tap = i / ((size_t)Cin * Cout);
    const bf16_t v = f32_to_bf16(w[i]);
    wf[(size_t)co * KTAPS * Cin + (size_t)tap * Cin + ci] = v;
    wb[(size_t)ci * KTAPS * Cout + (size_t)(KTAPS - 1 - tap) * Cout + co] = v;
  }
}

// Weight gradient, slab z of the pixel range [z kchunk, (z + 1) kchunk): partial[z][m][n], m = tap Cin + ci.  A tile =
// 128 (tap, ci) columns x 64 pixels gathered from the image, B tile = 64 pixels x 128 output channels; both staged in
// LDS as [column][pixel] (pixel pairs packed into 32-bit words), XOR-swizzled by 16-byte groups.
template <typename TP>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(int Mpix, int H, int W, int Cin, int Cout,
                                                         const bf16_t* __restrict__ X, const bf16_t* __restrict__ dY,
                                                         int kchunk, float* __restrict__ partial) {
  constexpr int KTAPS = TP::N;
  constexpr int BM = 128, BN = 128, BK = 64, LD = BK + 8;
  constexpr int STAGE = (BM + BN) * LD;
  __shared__ __attribute__((aligned(16))) bf16_t S[2 * STAGE];
  const int M = KTAPS * Cin, N = Cout, K = Mpix, HW = H * W;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int kbeg = blockIdx.z * kchunk, kend = min(K, kbeg + kchunk);
  const int nkt = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;

  const int mvec = tid & 15;
  const int kp0 = tid >> 4;
  const int mcol = m0 + mvec * 8;                          // first of this thread's 8 (tap, ci) columns
  const bool a_ok = mcol + 8 <= M, b_ok = n0 + mvec * 8 + 8 <= N;
  const int tap = a_ok ? mcol / Cin : 0, ci = a_ok ? mcol - tap * Cin : 0;
  const int dy = tap / TP::KW - TP::OY, dx = tap - (tap / TP::KW) * TP::KW - TP::OX;
  const ptrdiff_t sh = ((ptrdiff_t)dy * W + dx) * Cin + ci;
  const bf16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8_t ra[2][2], rb[2][2];
  auto gload = [&](int kt) {
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int p = kbeg + kt * BK + 2 * (kp0 + 16 * it) + hh;          // pixel = reduction index
        const bool kin = p < kend;
        const int pp = kin ? p : 0;
        const int rem = pp % HW;
        const int y = rem / W, x = rem - y * W;
        const bool ok = a_ok && kin && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
        ra[it][hh] = ok ? *reinterpret_cast<const bf16x8_t*>(X + (ptrdiff_t)((size_t)pp * Cin) + sh) : zero;
        rb[it][hh] = (b_ok && kin) ? *reinterpret_cast<const bf16x8_t*>(dY + (size_t)pp * Cout + n0 + mvec * 8) : zero;
      }
  };
  const unsigned sw = (unsigned)(mvec & 7);
  auto sstore = [&](bf16_t* st) {
    char* base = reinterpret_cast<char*>(st);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const unsigned k2 = (unsigned)(2 * (kp0 + 16 * it));
      const unsigned inrow = (((k2 >> 3) ^ sw) << 4) + (k2 & 7u) * 2u;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned off = (unsigned)(mvec * 8 + j) * LD * 2u + inrow;
        *reinterpret_cast<unsigned*>(base + off) =
            (unsigned)(unsigned short)ra[it][0][j] | ((unsigned)(unsigned short)ra[it][1][j] << 16);
        *reinterpret_cast<unsigned*>(base + BM * LD * 2 + off) =
            (unsigned)(unsigned short)rb[it][0][j] | ((unsigned)(unsigned short)rb[it][1][j] << 16);
      }
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  if (nkt > 0) {
    gload(0);
    sstore(S);
  }
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  unsigned arow[4], brow[4], au[4], bu[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned ra_ = (unsigned)(wm * 64 + i * 16 + fr), rb_ = (unsigned)(wn * 64 + i * 16 + fr);
    arow[i] = ra_ * LD * 2u;
    brow[i] = (unsigned)BM * LD * 2u + rb_ * LD * 2u;
    au[i] = (unsigned)fq ^ ((ra_ >> 3) & 7u);
    bu[i] = (unsigned)fq ^ ((rb_ >> 3) & 7u);
  }
  for (int kt = 0; kt < nkt; ++kt) {
    const char* cur = reinterpret_cast<const char*>(S + (kt & 1) * STAGE);
    if (kt + 1 < nkt) gload(kt + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(cur + arow[i] + ((au[i] ^ (unsigned)(ks * 4)) << 4));
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(cur + brow[j] + ((bu[j] ^ (unsigned)(ks * 4)) << 4));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nkt) sstore(S + ((kt + 1) & 1) * STAGE);
    __syncthreads();
  }
  float* slab = partial + (size_t)blockIdx.z * M * N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nb = n0 + wn * 64 + j * 16 + fq * 4;
      if (nb >= N) continue;
      *reinterpret_cast<f32x4_t*>(slab + (size_t)m * N + nb) = acc[i][j];
    }
  }
}

// dw[i] (+)= sum_{z = 0 .. S-1} partial[z][i], slabs added in index order (eight requests in flight)
__global__ void conv_slab_sum_kernel(const float* __restrict__ partial, int S, size_t total, float* __restrict__ dw,
                                     int accumulate) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    int z = 0;
    for (; z + 8 <= S; z += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = partial[(size_t)(z + u) * total + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; z < S; ++z) v += partial[(size_t)z * total + i];
    dw[i] = accumulate ? dw[i] + v : v;
  }
}

// max_pool [3,1] stride [3,1] SAME over H (cnn_util.py:13-28): Ho = ceil(H / 3), pad rows pt = (3 Ho - H) / 2 before and
// the rest after (TensorFlow puts the odd one after); window ho = rows 3 ho - pt .. 3 ho - pt + 2, padding never
// selected.  arg = window row 0..2 of the maximum, the FIRST of equal values (the strict '>' of maxpool_fwd_kernel).
// Four channels per thread (C % 4 == 0).  use_drop: tf.nn.dropout on the pooled output in the same pass.
template <typename T>
__global__ void maxpool3x1_fwd_kernel(const T* __restrict__ in, int N, int H, int W, int C, T* __restrict__ out,
                                      uint8_t* __restrict__ arg, float keep, uint64_t seed, uint64_t offset, int use_drop) {
  const int Ho = (H + 2) / 3, pt = (3 * Ho - H) / 2, C4 = C / 4;
  const size_t total = (size_t)N * Ho * W * C4;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(idx % C4);
    const size_t q = idx / C4;
    const int w = (int)(q % W);
    const size_t q2 = q / W;
    const int ho = (int)(q2 % Ho);
    const size_t n = q2 / Ho;
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bi[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int h = 3 * ho - pt + k;
      if (h < 0 || h >= H) continue;
      const T* p = in + ((n * H + h) * W + w) * C + (size_t)c4 * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = Elem<T>::to_f32(p[j]);
        if (v > best[j]) { best[j] = v; bi[j] = k; }
      }
    }
    const size_t e = idx * 4;
    if (use_drop) {                                        // e % 4 == 0: exactly one Philox block
      float mk[4];
      asr_dropout_words(offset + e / 4, seed, keep, 1.f / keep, mk);
#pragma unroll
      for (int j = 0; j < 4; ++j) best[j] = Elem<T>::to_f32(Elem<T>::from_f32(best[j])) * mk[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out[e + j] = Elem<T>::from_f32(best[j]);
      arg[e + j] = (uint8_t)bi[j];
    }
  }
}
// gather form (deterministic): every input row lies in exactly one window (stride == window), din = dout of that window
// where the row was its maximum, else 0
template <typename T>
__global__ void maxpool3x1_bwd_kernel(const T* __restrict__ dout, const uint8_t* __restrict__ arg, int N, int H, int W,
                                      int C, T* __restrict__ din) {
  const int Ho = (H + 2) / 3, pt = (3 * Ho - H) / 2;
  const size_t total = (size_t)N * H * W * C;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const size_t q = idx / C;
    const int w = (int)(q % W);
    const size_t q2 = q / W;
    const int h = (int)(q2 % H);
    const size_t n = q2 / H;
    const int ho = (h + pt) / 3, k = (h + pt) - 3 * ho;
    const size_t o = ((n * Ho + ho) * W + w) * C + c;
    din[idx] = arg[o] == k ? dout[o] : Elem<T>::from_f32(0.f);
  }
}

static inline int grid_for(size_t total) {
  const size_t b = (total + 255) / 256;
  return (int)(b < 16384 ? (b ? b : 1) : 16384);
}

}  // namespace

template <typename TP>
int asr_conv_nt(asr_handle* h, const char* what, const void* x, int N, int H, int W, int Cin, const void* wt,
                const float* bias, int Cout, int act, const ConvGate& gate, bool out_f32, void* out, asr_stream s) {
  if (!x || !wt || !out || N < 1 || H < 1 || W < 1) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: bad args", what);
  // K / N: reduction and output channels of this product (the data gradient's are the layer's Cout / Cin)
  if (Cin % 64 != 0 || Cout % 64 != 0 || Cin < 64 || Cout < 64)
    ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "%s: %d input and %d output channels of the product must be multiples of 64", what,
             Cin, Cout);
  const long long mp = (long long)N * H * W;
  if (mp >= (1ll << 31) - 128) ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "%s: %lld pixels", what, mp);
  const int Mpix = (int)mp;
  const bool bn128 = Cout % 128 == 0;
  const long long blocks = (long long)((Mpix + 127) / 128) * (Cout / (bn128 ? 128 : 64));
  if (blocks >= (1ll << 31)) ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "%s: grid too large", what);
  hipStream_t st = (hipStream_t)s;
#define ASR_CNT(TO, BN) \
  hipLaunchKernelGGL((conv_nt_kernel<TO, BN, TP>), dim3((unsigned)blocks), dim3(256), 0, st, Mpix, H, W, Cin, Cout, \
                     (const bf16_t*)x, (const bf16_t*)wt, (TO*)out, bias, act, gate)
  if (out_f32) { if (bn128) ASR_CNT(float, 128); else ASR_CNT(float, 64); }
  else { if (bn128) ASR_CNT(bf16_t, 128); else ASR_CNT(bf16_t, 64); }
#undef ASR_CNT
  if constexpr (std::is_same<TP, Taps33>::value) {         // asr_conv_path_counts: the 3x3 entry points' tiled launches
    h->conv_counts[ASR_CONVP_FORM_TILED] += 1;
    h->conv_counts[asr_conv_pair_counter(Cin, Cout)] += 1;
    h->conv_counts[bn128 ? ASR_CONVP_TILED_BN128 : ASR_CONVP_TILED_BN64] += 1;
  }
  ASR_CHECK_LAUNCH(h, what);
  return ASR_OK;
}
template int asr_conv_nt<Taps33>(asr_handle*, const char*, const void*, int, int, int, int, const void*, const float*, int,
                                 int, const ConvGate&, bool, void*, asr_stream);

int asr_conv_prep(asr_handle* h, const char* what, int ntaps, const float* w_hwio, int Cin, int Cout, void* wt_fwd,
                  void* wt_bwd, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!w_hwio || !wt_fwd || !wt_bwd || Cin < 1 || Cout < 1) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: bad args", what);
  auto k = ntaps == 9 ? conv_prep_kernel<9> : ntaps == 12 ? conv_prep_kernel<12> : ntaps == 15 ? conv_prep_kernel<15> : nullptr;
  if (!k) ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "%s: %d taps", what, ntaps);
  hipLaunchKernelGGL(k, dim3(grid_for((size_t)ntaps * Cin * Cout)), dim3(256), 0, (hipStream_t)s, w_hwio, Cin, Cout,
                     (bf16_t*)wt_fwd, (bf16_t*)wt_bwd);
  ASR_CHECK_LAUNCH(h, what);
  return ASR_OK;
}

int asr_conv_wgrad_plan(asr_handle* h, const char* what, int Mpix, int tiles, size_t slab_bytes, int max_slabs, int* S,
                        int* kchunk) {
  const size_t room = h->scratch_bytes > ASR_XCH_BYTES ? h->scratch_bytes - ASR_XCH_BYTES : 0;
  int s = (2048 + tiles - 1) / tiles;
  const int maxS = (Mpix + 511) / 512;
  if (s > maxS) s = maxS;
  if (s > max_slabs) s = max_slabs;
  if ((size_t)s > room / slab_bytes) s = (int)(room / slab_bytes);
  if (s < 1) ASR_FAIL(h, ASR_ERR_WORKSPACE, "%s: scratch too small", what);
  *kchunk = ((Mpix + s - 1) / s + 63) / 64 * 64;
  *S = (Mpix + *kchunk - 1) / *kchunk;
  return ASR_OK;
}

template <typename TP>
void asr_conv_wgrad_tiled(const void* x, const void* dy, int Mpix, int H, int W, int Cin, int Cout, int S, int kchunk,
                          float* partial, hipStream_t st) {
  hipLaunchKernelGGL(conv_wgrad_kernel<TP>, dim3((Cout + 127) / 128, (TP::N * Cin + 127) / 128, S), dim3(256), 0, st, Mpix,
                     H, W, Cin, Cout, (const bf16_t*)x, (const bf16_t*)dy, kchunk, partial);
}
template void asr_conv_wgrad_tiled<Taps33>(const void*, const void*, int, int, int, int, int, int, int, float*, hipStream_t);

void asr_conv_slab_sum(const float* partial, int S, size_t total, float* dw, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(conv_slab_sum_kernel, dim3(grid_for(total)), dim3(256), 0, st, partial, S, total, dw, accumulate);
}

extern "C" int asr_colsum(asr_handle* h, int dtype, const void* a, int M, int N, int lda, float* out, asr_stream s);

// weight + bias gradient of the tiled kernels
template <typename TP>
static int conv_wgrad_launch(asr_handle* h, const char* what, const void* x, const void* dy, int N, int H, int W, int Cin,
                             int Cout, float* dw, float* dbias, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!x || !dy || !dw || N < 1 || H < 1 || W < 1) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "%s: bad args", what);
  if (Cin % 8 != 0 || Cout % 8 != 0)
    ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "%s: Cin=%d, Cout=%d must be multiples of 8", what, Cin, Cout);
  const long long mp = (long long)N * H * W;
  if (mp >= (1ll << 31) - 128) ASR_FAIL(h, ASR_ERR_UNSUPPORTED, "%s: %lld pixels", what, mp);
  const int Mpix = (int)mp, M = TP::N * Cin;
  int S, kchunk;
  const int rc = asr_conv_wgrad_plan(h, what, Mpix, ((M + 127) / 128) * ((Cout + 127) / 128),
                                     (size_t)M * Cout * sizeof(float), INT_MAX, &S, &kchunk);
  if (rc != ASR_OK) return rc;
  float* partial = (float*)h->scratch;
  asr_conv_wgrad_tiled<TP>(x, dy, Mpix, H, W, Cin, Cout, S, kchunk, partial, (hipStream_t)s);
  asr_conv_slab_sum(partial, S, (size_t)M * Cout, dw, 0, (hipStream_t)s);
  ASR_CHECK_LAUNCH(h, what);
  if (dbias) return asr_colsum(h, ASR_BF16, dy, Mpix, Cout, Cout, dbias, s);
  return ASR_OK;
}

static const ConvGate kNoGate = {nullptr, 1.f, 0, 0, 0};

// ---- cnn_zhang: 3x5
extern "C" int asr_conv3x5_prep_weights(asr_handle* h, const float* w_hwio, int Cin, int Cout, void* wt_fwd, void* wt_bwd,
                                        asr_stream s) {
  return asr_conv_prep(h, "asr_conv3x5_prep_weights", 15, w_hwio, Cin, Cout, wt_fwd, wt_bwd, s);
}

extern "C" int asr_conv3x5_fwd(asr_handle* h, const void* x, int N, int H, int W, int Cin, const void* wt_fwd,
                               const float* bias, int Cout, int relu, void* out, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  return asr_conv_nt<Taps35>(h, "asr_conv3x5_fwd", x, N, H, W, Cin, wt_fwd, bias, Cout, relu ? 1 : 0, kNoGate, false, out, s);
}

extern "C" int asr_conv3x5_fwd_drop(asr_handle* h, const void* x, int N, int H, int W, int Cin, const void* wt_fwd,
                                    const float* bias, int Cout, float keep_prob, uint64_t seed, uint64_t offset, void* out,
                                    asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!(keep_prob > 0.f && keep_prob <= 1.f)) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_conv3x5_fwd_drop: keep_prob %g", keep_prob);
  const ConvGate g = {nullptr, keep_prob, seed, offset, 1};
  return asr_conv_nt<Taps35>(h, "asr_conv3x5_fwd_drop", x, N, H, W, Cin, wt_fwd, bias, Cout, 3, g, false, out, s);
}

extern "C" int asr_conv3x5_bwd_data(asr_handle* h, const void* dy, int N, int H, int W, int Cout, const void* wt_bwd,
                                    int Cin, float* dx, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  return asr_conv_nt<Taps35>(h, "asr_conv3x5_bwd_data", dy, N, H, W, Cout, wt_bwd, nullptr, Cin, 0, kNoGate, true, dx, s);
}

extern "C" int asr_conv3x5_bwd_data_relu(asr_handle* h, const void* dy, int N, int H, int W, int Cout, const void* wt_bwd,
                                         int Cin, const void* act_below, float keep_prob, uint64_t seed, uint64_t offset,
                                         int use_drop, void* dpre_below, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!act_below || use_drop < 0 || use_drop > 2 || (use_drop && !(keep_prob > 0.f && keep_prob <= 1.f)))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_conv3x5_bwd_data_relu: bad args");
  const ConvGate g = {(const bf16_t*)act_below, keep_prob, seed, offset, use_drop};
  return asr_conv_nt<Taps35>(h, "asr_conv3x5_bwd_data_relu", dy, N, H, W, Cout, wt_bwd, nullptr, Cin, 2, g, false, dpre_below, s);
}

extern "C" int asr_conv3x5_bwd_weight_bias(asr_handle* h, const void* x, const void* dy, int N, int H, int W, int Cin,
                                           int Cout, float* dw, float* dbias, asr_stream s) {
  return conv_wgrad_launch<Taps35>(h, "asr_conv3x5_bwd_weight_bias", x, dy, N, H, W, Cin, Cout, dw, dbias, s);
}

extern "C" int asr_maxpool3x1_fwd(asr_handle* h, int dtype, const void* in, int N, int H, int W, int C, void* out,
                                  uint8_t* argmax, float keep_prob, uint64_t seed, uint64_t offset, int use_drop,
                                  asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!asr_dtype_ok(dtype) || !in || !out || !argmax || N < 1 || H < 1 || W < 1 || C < 4 || C % 4 != 0 ||
      (use_drop && !(keep_prob > 0.f && keep_prob <= 1.f)))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_maxpool3x1_fwd: bad args");
  const size_t total = (size_t)N * ((H + 2) / 3) * W * (C / 4);
  if (dtype == ASR_F32)
    hipLaunchKernelGGL(maxpool3x1_fwd_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s, (const float*)in,
                       N, H, W, C, (float*)out, argmax, keep_prob, seed, offset, use_drop);
  else
    hipLaunchKernelGGL(maxpool3x1_fwd_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s,
                       (const bf16_t*)in, N, H, W, C, (bf16_t*)out, argmax, keep_prob, seed, offset, use_drop);
  ASR_CHECK_LAUNCH(h, "asr_maxpool3x1_fwd");
  return ASR_OK;
}

extern "C" int asr_maxpool3x1_bwd(asr_handle* h, int dtype, const void* dout, const uint8_t* argmax, int N, int H, int W,
                                  int C, void* din, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!asr_dtype_ok(dtype) || !dout || !argmax || !din || N < 1 || H < 1 || W < 1 || C < 1)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_maxpool3x1_bwd: bad args");
  const size_t total = (size_t)N * H * W * C;
  if (dtype == ASR_F32)
    hipLaunchKernelGGL(maxpool3x1_bwd_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s,
                       (const float*)dout, argmax, N, H, W, C, (float*)din);
  else
    hipLaunchKernelGGL(maxpool3x1_bwd_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s,
                       (const bf16_t*)dout, argmax, N, H, W, C, (bf16_t*)din);
  ASR_CHECK_LAUNCH(h, "asr_maxpool3x1_bwd");
  return ASR_OK;
}

// ---- the 3x4 SAME convolution of the student CNNs (CNN2, models/encoders/core/student_cnn_ctc.py:111-117)
extern "C" int asr_conv3x4_prep_weights(asr_handle* h, const float* w_hwio, int Cin, int Cout, void* wt_fwd, void* wt_bwd,
                                        asr_stream s) {
  return asr_conv_prep(h, "asr_conv3x4_prep_weights", 12, w_hwio, Cin, Cout, wt_fwd, wt_bwd, s);
}

extern "C" int asr_conv3x4_fwd(asr_handle* h, const void* x, int N, int H, int W, int Cin, const void* wt_fwd,
                               const float* bias, int Cout, int relu, int out_f32, void* out, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  return asr_conv_nt<Taps34f>(h, "asr_conv3x4_fwd", x, N, H, W, Cin, wt_fwd, bias, Cout, relu ? 1 : 0, kNoGate, out_f32 != 0,
                              out, s);
}

extern "C" int asr_conv3x4_bwd_data(asr_handle* h, const void* dy, int N, int H, int W, int Cout, const void* wt_bwd,
                                    int Cin, float* dx, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  return asr_conv_nt<Taps34b>(h, "asr_conv3x4_bwd_data", dy, N, H, W, Cout, wt_bwd, nullptr, Cin, 0, kNoGate, true, dx, s);
}

extern "C" int asr_conv3x4_bwd_weight_bias(asr_handle* h, const void* x, const void* dy, int N, int H, int W, int Cin,
                                           int Cout, float* dw, float* dbias, asr_stream s) {
  return conv_wgrad_launch<Taps34f>(h, "asr_conv3x4_bwd_weight_bias", x, dy, N, H, W, Cin, Cout, dw, dbias, s);
}
