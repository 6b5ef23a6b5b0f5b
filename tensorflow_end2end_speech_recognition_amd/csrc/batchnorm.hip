// Batch normalization of the student CNNs (models/encoders/core/cnn_util.py:87-149, batch_normalization with its
// defaults: eps 1e-3, momentum 0.9, non-fused) over NHWC activations viewed as [M rows = N H W, C channels], C % 64 == 0.
//
//   statistics   tf.nn.moments over all rows: mean and the biased (population) variance.  Each thread keeps sums of
//                (x - shift_c) over its rows (shift_c = row 0's value of the channel, so the sums stay near zero whatever
//                the data's offset) and turns them into (count, mean, M2); the 16 row lanes of a block and then the G
//                blocks are merged with Chan's pairwise formula, always in index order: bitwise reproducible.  The
//                finalize also forms the moving-average update avg * momentum + stat * (1 - momentum) (the UPDATE_OPS
//                of cnn_util.py:138-145) into a pending buffer that the training step commits on the device.
//   apply        tf.nn.batch_normalization: inv = rsqrt(var + eps) * gamma, y = x * inv + (beta - mean * inv), fused
//                with the following max_pool [3,1] / [3,1] SAME over H (argmax kept, first of equal values) or with the
//                identity pool [1,1]; writes the next layer's operand (fp32 or bf16).
//   backward     gather-form pool backward, then sum(dy) and sum(dy * xhat) per channel (same fixed-order two-level
//                reduction; these ARE dbeta and dgamma and are written into the gradient buffer), then
//                dx = gamma rstd (dy - sum(dy) / M - xhat sum(dy xhat) / M), gated by the ReLU in front of the layer
//                (x > 0, x = the ReLU output the statistics were taken over).
#include "common.h"

namespace {

constexpr int BN_LANES = 16;      // row lanes per block; 16 channel quads (64 channels) across a block of 256 threads
constexpr int BN_MAXG = 512;      // row blocks

// number of row blocks: a function of M only, so the reduction order never depends on anything but the shape
static inline int bn_groups(long long M) {
  long long g = (M + 255) / 256;
  if (g > BN_MAXG) g = BN_MAXG;
  return (int)(g < 1 ? 1 : g);
}

struct Moments {
  float n, mean, m2;
};

__device__ __forceinline__ Moments chan_merge(Moments a, Moments b) {
  const float n = a.n + b.n;
  if (b.n == 0.f) return a;
  if (a.n == 0.f) return b;
  const float d = b.mean - a.mean, fb = b.n / n;
  Moments r;
  r.n = n;
  r.mean = a.mean + d * fb;
  r.m2 = a.m2 + b.m2 + d * d * a.n * fb;
  return r;
}

// grid (G, C / 64), 256 threads: lane (r, q) sums rows r, r + 16, ... of this block's row range for channels
// 64 blockIdx.y + 4 q .. + 3.  ws: [G][3][C] = count, mean, M2.
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, long long M, int C, int rows_per,
                                                       float* __restrict__ ws) {
  const int q = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int c = blockIdx.y * 64 + q * 4;
  const long long r0 = (long long)blockIdx.x * rows_per;
  const long long r1 = min(M, r0 + rows_per);
  const f32x4_t shift = *reinterpret_cast<const f32x4_t*>(x + c);
  float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
  float cnt = 0.f;
  for (long long row = r0 + r; row < r1; row += BN_LANES) {
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + row * C + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = v[j] - shift[j];
      s[j] += d;
      ss[j] = fmaf(d, d, ss[j]);
    }
    cnt += 1.f;
  }
  __shared__ float sh[3][BN_LANES][64];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float m = cnt > 0.f ? s[j] / cnt : 0.f;
    sh[0][r][q * 4 + j] = cnt;
    sh[1][r][q * 4 + j] = m + shift[j];
    sh[2][r][q * 4 + j] = cnt > 0.f ? fmaxf(ss[j] - s[j] * m, 0.f) : 0.f;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int cc = threadIdx.x;
    Moments a = {sh[0][0][cc], sh[1][0][cc], sh[2][0][cc]};
    for (int k = 1; k < BN_LANES; ++k) a = chan_merge(a, Moments{sh[0][k][cc], sh[1][k][cc], sh[2][k][cc]});
    float* w = ws + (size_t)blockIdx.x * 3 * C + blockIdx.y * 64 + cc;
    w[0] = a.n;
    w[C] = a.mean;
    w[2 * C] = a.m2;
  }
}

// one thread per channel: merge the G partials in order (double), then mean, var, rstd and the pending moving averages.
// stats: [5][C] = mean, var, rstd, pending avg_mean, pending avg_variance
__global__ void bn_stats_finalize_kernel(const float* __restrict__ ws, int G, int C, float eps, float momentum,
                                         const float* __restrict__ avg_mean, const float* __restrict__ avg_var,
                                         float* __restrict__ stats) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int g = 0; g < G; ++g) {
    const double nb = ws[(size_t)g * 3 * C + c];
    if (nb == 0.0) continue;
    const double mb = ws[(size_t)g * 3 * C + C + c], m2b = ws[(size_t)g * 3 * C + 2 * C + c];
    const double nn = n + nb, d = mb - mean;
    mean += d * (nb / nn);
    m2 += m2b + d * d * n * (nb / nn);
    n = nn;
  }
  const float fm = (float)mean, fv = (float)(n > 0.0 ? m2 / n : 0.0);
  stats[c] = fm;
  stats[C + c] = fv;
  stats[2 * C + c] = 1.f / sqrtf(fv + eps);
  if (avg_mean && avg_var) {
    stats[3 * C + c] = avg_mean[c] * momentum + fm * (1.f - momentum);
    stats[4 * C + c] = avg_var[c] * momentum + fv * (1.f - momentum);
  }
}

// y = x * inv + (beta - mean * inv), inv = rsqrt(var + eps) * gamma (tf.nn.batch_normalization), then the pool.
// pool 0: identity ([1,1] / [1,1]); pool 1: max over rows 3 ho - pt .. 3 ho - pt + 2 of H (SAME, pt = (3 Ho - H) / 2).
template <typename TO>
__global__ void bn_apply_kernel(const float* __restrict__ x, int N, int H, int W, int C, const float* __restrict__ mean,
                                const float* __restrict__ var, const float* __restrict__ gamma,
                                const float* __restrict__ beta, float eps, int pool, TO* __restrict__ out,
                                uint8_t* __restrict__ arg) {
  const int Ho = pool ? (H + 2) / 3 : H, pt = pool ? (3 * Ho - H) / 2 : 0, C4 = C / 4;
  const size_t total = (size_t)N * Ho * W * C4;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C4) * 4;
    const size_t q = idx / C4;
    const int w = (int)(q % W);
    const size_t q2 = q / W;
    const int ho = (int)(q2 % Ho);
    const size_t n = q2 / Ho;
    float inv[4], off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      inv[j] = (1.f / sqrtf(var[c + j] + eps)) * gamma[c + j];
      off[j] = beta[c + j] - mean[c + j] * inv[j];
    }
    float best[4];
    int bi[4] = {0, 0, 0, 0};
    if (!pool) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + ((n * H + ho) * W + w) * C + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) best[j] = fmaf(v[j], inv[j], off[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) best[j] = -INFINITY;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int h = 3 * ho - pt + k;
        if (h < 0 || h >= H) continue;
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + ((n * H + h) * W + w) * C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float y = fmaf(v[j], inv[j], off[j]);
          if (y > best[j]) { best[j] = y; bi[j] = k; }
        }
      }
    }
    const size_t e = idx * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out[e + j] = Elem<TO>::from_f32(best[j]);
      if (pool) arg[e + j] = (uint8_t)bi[j];
    }
  }
}

// the gradient at BN output row `row` (input geometry [N, H, W]) for channels c .. c + 3: dz itself, or gathered from the
// pooled gradient where this row was its window's maximum
__device__ __forceinline__ f32x4_t bn_dy(const float* __restrict__ dz, const uint8_t* __restrict__ arg, int pool,
                                         long long row, int H, int W, int C, int c) {
  if (!pool) return *reinterpret_cast<const f32x4_t*>(dz + row * C + c);
  const int Ho = (H + 2) / 3, pt = (3 * Ho - H) / 2;
  const long long hw = (long long)H * W;
  const long long n = row / hw;
  const int rem = (int)(row - n * hw), h = rem / W, w = rem - h * W;
  const int ho = (h + pt) / 3, k = (h + pt) - 3 * ho;
  const size_t o = (size_t)((n * Ho + ho) * W + w) * C + c;
  const f32x4_t g = *reinterpret_cast<const f32x4_t*>(dz + o);
  const uint32_t a = *reinterpret_cast<const uint32_t*>(arg + o);
  f32x4_t r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = ((a >> (8 * j)) & 0xffu) == (uint32_t)k ? g[j] : 0.f;
  return r;
}

// ws: [G][2][C] = partial sum(dy), sum(dy xhat)
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ dz, const uint8_t* __restrict__ arg,
                                                            int pool, const float* __restrict__ x, long long M, int H,
                                                            int W, int C, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, int rows_per,
                                                            float* __restrict__ ws) {
  const int q = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int c = blockIdx.y * 64 + q * 4;
  const long long r0 = (long long)blockIdx.x * rows_per;
  const long long r1 = min(M, r0 + rows_per);
  float mu[4], rs[4], s[4] = {0.f, 0.f, 0.f, 0.f}, sx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) { mu[j] = mean[c + j]; rs[j] = rstd[c + j]; }
  for (long long row = r0 + r; row < r1; row += BN_LANES) {
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + row * C + c);
    const f32x4_t g = bn_dy(dz, arg, pool, row, H, W, C, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] += g[j];
      sx[j] = fmaf(g[j], (v[j] - mu[j]) * rs[j], sx[j]);
    }
  }
  __shared__ float sh[2][BN_LANES][64];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sh[0][r][q * 4 + j] = s[j];
    sh[1][r][q * 4 + j] = sx[j];
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int cc = threadIdx.x;
    float a = 0.f, b = 0.f;
    for (int k = 0; k < BN_LANES; ++k) { a += sh[0][k][cc]; b += sh[1][k][cc]; }
    float* w = ws + (size_t)blockIdx.x * 2 * C + blockIdx.y * 64 + cc;
    w[0] = a;
    w[C] = b;
  }
}

__global__ void bn_bwd_finalize_kernel(const float* __restrict__ ws, int G, int C, float* __restrict__ dgamma,
                                       float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int g = 0; g < G; ++g) {
    a += ws[(size_t)g * 2 * C + c];
    b += ws[(size_t)g * 2 * C + C + c];
  }
  dbeta[c] = (float)a;
  dgamma[c] = (float)b;
}

template <typename TO>
__global__ void bn_bwd_dx_kernel(const float* __restrict__ dz, const uint8_t* __restrict__ arg, int pool,
                                 const float* __restrict__ x, long long M, int H, int W, int C,
                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                 const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                 const float* __restrict__ dbeta, int relu_gate, TO* __restrict__ dx) {
  const int C4 = C / 4;
  const float invM = 1.f / (float)M;
  const size_t total = (size_t)M * C4;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C4) * 4;
    const long long row = (long long)(idx / C4);
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + row * C + c);
    const f32x4_t g = bn_dy(dz, arg, pool, row, H, W, C, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float rs = rstd[c + j];
      const float xh = (v[j] - mean[c + j]) * rs;
      float d = gamma[c + j] * rs * (g[j] - dbeta[c + j] * invM - xh * (dgamma[c + j] * invM));
      if (relu_gate && !(v[j] > 0.f)) d = 0.f;
      dx[(size_t)row * C + c + j] = Elem<TO>::from_f32(d);
    }
  }
}

static inline int bn_grid(size_t total) {
  const size_t b = (total + 255) / 256;
  return (int)(b < 16384 ? (b ? b : 1) : 16384);
}

}  // namespace

extern "C" size_t asr_bn_workspace_bytes(long long M, int C) {
  return (size_t)bn_groups(M) * 3 * (size_t)(C > 0 ? C : 0) * sizeof(float);
}

extern "C" int asr_bn_stats(asr_handle* h, const float* x, long long M, int C, float eps, float momentum,
                            const float* avg_mean, const float* avg_var, float* stats, void* ws, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!x || !stats || !ws || M < 1 || C < 64 || C % 64 != 0 || !(eps > 0.f))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_bn_stats: bad args (M=%lld, C=%d)", M, C);
  const int G = bn_groups(M);
  const int rows_per = (int)((M + G - 1) / G);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(bn_stats_kernel, dim3(G, C / 64), dim3(256), 0, st, x, M, C, rows_per, (float*)ws);
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, st, (const float*)ws, G, C, eps,
                     momentum, avg_mean, avg_var, stats);
  ASR_CHECK_LAUNCH(h, "asr_bn_stats");
  return ASR_OK;
}

extern "C" int asr_bn_apply(asr_handle* h, int out_dtype, const float* x, int N, int H, int W, int C, const float* mean,
                            const float* var, const float* gamma, const float* beta, float eps, int pool, void* out,
                            uint8_t* argmax, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!asr_dtype_ok(out_dtype) || !x || !mean || !var || !gamma || !beta || !out || N < 1 || H < 1 || W < 1 || C < 4 ||
      C % 4 != 0 || (pool != 0 && pool != 1) || (pool && !argmax))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_bn_apply: bad args");
  const int Ho = pool ? (H + 2) / 3 : H;
  const size_t total = (size_t)N * Ho * W * (C / 4);
  hipStream_t st = (hipStream_t)s;
  if (out_dtype == ASR_F32)
    hipLaunchKernelGGL(bn_apply_kernel<float>, dim3(bn_grid(total)), dim3(256), 0, st, x, N, H, W, C, mean, var, gamma,
                       beta, eps, pool, (float*)out, argmax);
  else
    hipLaunchKernelGGL(bn_apply_kernel<bf16_t>, dim3(bn_grid(total)), dim3(256), 0, st, x, N, H, W, C, mean, var, gamma,
                       beta, eps, pool, (bf16_t*)out, argmax);
  ASR_CHECK_LAUNCH(h, "asr_bn_apply");
  return ASR_OK;
}

extern "C" int asr_bn_bwd(asr_handle* h, int out_dtype, const float* dz, const uint8_t* argmax, int pool, const float* x,
                          int N, int H, int W, int C, const float* stats, const float* gamma, int relu_gate,
                          float* dgamma, float* dbeta, void* dx, void* ws, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!asr_dtype_ok(out_dtype) || !dz || !x || !stats || !gamma || !dgamma || !dbeta || !dx || !ws || N < 1 || H < 1 ||
      W < 1 || C < 64 || C % 64 != 0 || (pool != 0 && pool != 1) || (pool && !argmax))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_bn_bwd: bad args");
  const long long M = (long long)N * H * W;
  const int G = bn_groups(M);
  const int rows_per = (int)((M + G - 1) / G);
  const float* mean = stats;
  const float* rstd = stats + 2 * C;
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(G, C / 64), dim3(256), 0, st, dz, argmax, pool, x, M, H, W, C, mean, rstd,
                     rows_per, (float*)ws);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, st, (const float*)ws, G, C, dgamma, dbeta);
  const size_t total = (size_t)M * (C / 4);
  if (out_dtype == ASR_F32)
    hipLaunchKernelGGL(bn_bwd_dx_kernel<float>, dim3(bn_grid(total)), dim3(256), 0, st, dz, argmax, pool, x, M, H, W, C,
                       mean, rstd, gamma, dgamma, dbeta, relu_gate, (float*)dx);
  else
    hipLaunchKernelGGL(bn_bwd_dx_kernel<bf16_t>, dim3(bn_grid(total)), dim3(256), 0, st, dz, argmax, pool, x, M, H, W, C,
                       mean, rstd, gamma, dgamma, dbeta, relu_gate, (bf16_t*)dx);
  ASR_CHECK_LAUNCH(h, "asr_bn_bwd");
  return ASR_OK;
}

// ---- soft-target softmax cross-entropy (tf.nn.softmax_cross_entropy_with_logits, student_ctc.py:321-327): one block
// per row.  loss = sum_j p_j (lse - z_j), lse = max + log sum exp(z - max); gradient (TF's kernel) (softmax(z) - p) *
// grad_scale, whatever the sum of p.  Block reductions in a fixed tree order.
namespace {

__device__ __forceinline__ float block_reduce(float v, float* sh, bool is_max) {
  v = is_max ? wave_reduce_max(v) : wave_reduce_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  float r = sh[0];
  for (int k = 1; k < (int)(blockDim.x >> 6); ++k) r = is_max ? fmaxf(r, sh[k]) : r + sh[k];
  return r;
}

__global__ __launch_bounds__(256) void soft_xent_kernel(const float* __restrict__ z, const float* __restrict__ p, int C,
                                                        float grad_scale, float* __restrict__ loss,
                                                        float* __restrict__ dz) {
  __shared__ float sh[4];
  const size_t row = blockIdx.x;
  const float* zr = z + row * C;
  const float* pr = p + row * C;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < C; j += blockDim.x) m = fmaxf(m, zr[j]);
  m = block_reduce(m, sh, true);
  float se = 0.f, sp = 0.f, spz = 0.f;
  for (int j = threadIdx.x; j < C; j += blockDim.x) {
    const float d = zr[j] - m;
    se += expf(d);
    sp += pr[j];
    spz = fmaf(pr[j], d, spz);
  }
  se = block_reduce(se, sh, false);
  sp = block_reduce(sp, sh, false);
  spz = block_reduce(spz, sh, false);
  const float lse = logf(se);
  if (threadIdx.x == 0) loss[row] = lse * sp - spz;
  if (dz) {
    const float inv = 1.f / se;
    for (int j = threadIdx.x; j < C; j += blockDim.x) dz[row * C + j] = (expf(zr[j] - m) * inv - pr[j]) * grad_scale;
  }
}

}  // namespace

extern "C" int asr_softmax_xent_soft(asr_handle* h, const float* logits, const float* targets, int rows, int C,
                                     float grad_scale, float* row_loss, float* dlogits, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!logits || !targets || !row_loss || rows < 1 || C < 1)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_softmax_xent_soft: bad args");
  hipLaunchKernelGGL(soft_xent_kernel, dim3(rows), dim3(256), 0, (hipStream_t)s, logits, targets, C, grad_scale, row_loss,
                     dlogits);
  ASR_CHECK_LAUNCH(h, "asr_softmax_xent_soft");
  return ASR_OK;
}
