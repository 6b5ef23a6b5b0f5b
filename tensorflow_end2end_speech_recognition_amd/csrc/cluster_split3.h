// fp32 operands on the bf16 matrix pipe: the three-term split that the fp32 LSTM clusters (lstm_cluster_f32.hip, the *_f32s
// kernels) and both GRU cluster kernels (gru_cluster.hip) multiply with.
// The exact-fp32 cluster kernels are bound by v_mfma_f32_16x16x4_f32: 32 cycles per SIMD for K = 4, i.e. 256 cycles per
// K = 32 against 17 for one v_mfma_f32_16x16x32_bf16 (MI355X_MICROARCH.md) -- 2 048 of the ~4 000 cycles of a step at
// H = 128.  An fp32 value IS the sum of three bf16 values (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): 3 x 8
// significand bits; both subtractions are exact in fp32), so x.w = sum of the nine term products, of which the six with
// weight >= 2^-16 are kept: lo.hi + hi.lo + mid.mid + mid.hi + hi.mid + hi.hi -- every product of two bf16 values is exact
// in the MFMA's fp32 accumulator; the dropped terms (mid.lo, lo.mid, lo.lo) are below 2^-24 of the result.  6 bf16 MFMAs x 17
// cycles = 102 per K = 32: the matrix phase of a step drops from 2 048 to ~820 cycles.  W_h is split once per launch into
// registers; h (forward) / the gate gradients (BPTT) are split by the lane that writes them into three bf16 LDS images.
// Same exchange, same saved activations, same lane <-> (row, unit) mapping as the exact-fp32 kernels; results differ from
// theirs by accumulation rounding only (fp32 parity bounds unchanged, tests/test_gpu_ops.py).  ASR_LSTM_F32_SPLIT=0 keeps
// the exact-fp32 MFMA kernels.
#pragma once
#include "common.h"

namespace {
__device__ __forceinline__ void split3(float x, unsigned short (&t)[3]) {
  const __bf16 h = (__bf16)x;
  const float r1 = x - (float)h;
  const __bf16 m = (__bf16)r1;
  const float r2 = r1 - (float)m;
  t[0] = __builtin_bit_cast(unsigned short, h);
  t[1] = __builtin_bit_cast(unsigned short, m);
  t[2] = __builtin_bit_cast(unsigned short, (__bf16)r2);
}
// one K = 32 chunk of a 16 x 16 tile: a[term], b[term] bf16 fragments; smallest terms first
__device__ __forceinline__ f32x4_t mma_s3(const bf16x8_t (&a)[3], const bf16x8_t (&b)[3], f32x4_t c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
  return c;
}
// B fragment of chunk c (k = 32 c + 8 rg + j, j < 8) of one 16-column tile out of an fp32 fragment packing
// [frag16][64 lanes][4] (lane (n, rg') holds k = 16 frag16 + 4 rg' + e): two 16-byte loads, split into three bf16 terms
__device__ __forceinline__ void load_split_frag(const float* tile_base, int c, int rg, int n, bf16x8_t (&out)[3]) {
  const float* p = tile_base + (((size_t)(2 * c + (rg >> 1)) * 64 + ((rg & 1) * 2) * 16 + n) * 4);
  const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(p);
  const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(p + 16 * 4);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    unsigned short t[3];
    split3(j < 4 ? v0[j] : v1[j - 4], t);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k][j] = (short)t[k];
  }
}
}  // namespace
