// fp32 operands on the bf16 matrix pipe: the three-term split that the fp32 LSTM clusters (lstm_cluster_f32.hip, under the
// OpSplit3 operand policy at the end of this file) and both GRU cluster kernels (gru_cluster.hip) multiply with.
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

// ---------------------------------------------------------------- exact fp32 MFMA (v_mfma_f32_16x16x4_f32, four per k = 16)
__device__ __forceinline__ void mma_f32x2(const f32x4_t& a, const f32x4_t& b0, const f32x4_t& b1, f32x4_t& c0,
                                          f32x4_t& c1) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b0[e], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b1[e], c1, 0, 0, 0);
  }
}
__device__ __forceinline__ f32x4_t mma_f32(const f32x4_t& a, const f32x4_t& b, f32x4_t c) {
#pragma unroll
  for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], c, 0, 0, 0);
  return c;
}

// ---------------------------------------------------------------- operand policies of the fp32 LSTM cluster kernels
// How the operands of the recurrent product (h W_h forward, dG W_h^T in the BPTT) are held and multiplied -- everything else
// of lstm_fwd_cluster_f32_kernel / lstm_bwd_cluster_f32_kernel is the same text for both.  A policy gives
//   frag, K      what a lane holds of an A or B operand for one k-step of a 16 x 16 tile, and the k values it covers
//   elem, TERMS  the LDS image: TERMS images [16 rows][n + PAD] of elem, `plb` bytes apart; a lane's fragment is 16 bytes at
//                16-byte steps in both (PAD: 16 bytes per row -> an odd number of 16-byte slots, see lds_swz)
//   PARK         whether rows past their length fetch and save at ONE parked position (which stays in the L2) instead of
//                walking the padded frames.  Kept as found when the two forms were merged: the split kernels were written
//                with it, the exact ones without, and it has not been measured for the exact form.
//   load_b       B fragment c, counted from k = 16 f0, of a 16-column tile out of the standard fp32 packing w: [k / 16][64
//                lanes][4]; lane (n, rg)
//   store_a      four consecutive k values of one row into the image (BPTT: the gate gradients of a unit)
//   load_a, mma, mma2 (one A fragment against the fragments of two tiles)
// and for the forward all-gather, whose 8-byte granule carries one value of h with its step tag:
//   encode       value, epoch = step + 1 -> the granule's two words;  tagged: does a polled granule carry `epoch`;
//   stage        a granule's words -> the image (the publisher stages its own value with the same call)
struct OpF32 {      // exact: the fp32 MFMA on fp32 images
  typedef f32x4_t frag;
  typedef float elem;
  static constexpr int K = 16, TERMS = 1, PAD = 16 / sizeof(elem);
  static constexpr bool PARK = false;
  // (the lane's slot 16 rg + n summed in 32 bits: added part by part to the 64-bit index, the BPTT at H = 512 comes out with
  // its MFMA chains rescheduled, profiles/f32_operand_policy.md)
  static __device__ __forceinline__ void load_b(const float* w, size_t f0, int c, int rg, unsigned n, frag& out) {
    out = *reinterpret_cast<const f32x4_t*>(w + ((f0 + c) * 64 + (rg * 16 + (int)n)) * 4);
  }
  static __device__ __forceinline__ void store_a(char* img, int, unsigned off, f32x4_t v) {
    *reinterpret_cast<f32x4_t*>(img + off) = v;
  }
  static __device__ __forceinline__ void load_a(const char* p, int, frag& out) { out = *reinterpret_cast<const f32x4_t*>(p); }
  static __device__ __forceinline__ f32x4_t mma(const frag& a, const frag& b, f32x4_t c) { return mma_f32(a, b, c); }
  static __device__ __forceinline__ void mma2(const frag& a, const frag& b0, const frag& b1, f32x4_t& c0, f32x4_t& c1) {
    mma_f32x2(a, b0, b1, c0, c1);
  }
  // granule = {tag32, fp32}
  static __device__ __forceinline__ void encode(float v, unsigned epoch, unsigned& hi, unsigned& lo) {
    hi = epoch;
    lo = __float_as_uint(v);
  }
  static __device__ __forceinline__ bool tagged(unsigned long long v, unsigned epoch) { return (unsigned)(v >> 32) == epoch; }
  static __device__ __forceinline__ void stage(char* img, int, unsigned off, unsigned lo, unsigned) {
    *reinterpret_cast<unsigned*>(img + off) = lo;
  }
};
struct OpSplit3 {   // three bf16 terms per value on the bf16 MFMA (above)
  typedef bf16x8_t frag[3];
  typedef unsigned short elem;
  static constexpr int K = 32, TERMS = 3, PAD = 16 / sizeof(elem);
  static constexpr bool PARK = true;
  static __device__ __forceinline__ void load_b(const float* w, size_t f0, int c, int rg, unsigned n, frag& out) {
    load_split_frag(w + f0 * 256, c, rg, (int)n, out);
  }
  static __device__ __forceinline__ void store_a(char* img, int plb, unsigned off, f32x4_t v) {
    typedef __attribute__((ext_vector_type(4))) unsigned short us4_t;
    us4_t tq[3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned short t[3];
      split3(v[q], t);
#pragma unroll
      for (int k = 0; k < 3; ++k) tq[k][q] = t[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<us4_t*>(img + k * plb + off) = tq[k];
  }
  static __device__ __forceinline__ void load_a(const char* p, int plb, frag& out) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = *reinterpret_cast<const bf16x8_t*>(p + k * plb);
  }
  static __device__ __forceinline__ f32x4_t mma(const frag& a, const frag& b, f32x4_t c) { return mma_s3(a, b, c); }
  static __device__ __forceinline__ void mma2(const frag& a, const frag& b0, const frag& b1, f32x4_t& c0, f32x4_t& c1) {
    c0 = mma_s3(a, b0, c0);
    c1 = mma_s3(a, b1, c1);
  }
  // The all-gather carries the TERMS: granule = {hi | mid << 16, lo | tag16 << 16}, tag16 = epoch & 0xffff (T < 65536, checked
  // by the launcher) -- a value is split once, by the lane that produced it, and a consumer stages what it polled with three
  // 2-byte LDS stores and no arithmetic.
  static __device__ __forceinline__ void encode(float v, unsigned epoch, unsigned& hi, unsigned& lo) {
    unsigned short t3[3];
    split3(v, t3);
    lo = (unsigned)t3[0] | ((unsigned)t3[1] << 16);
    hi = ((unsigned)t3[2]) | (epoch << 16);
  }
  static __device__ __forceinline__ bool tagged(unsigned long long v, unsigned epoch) {
    return (unsigned)(v >> 48) == (epoch & 0xffffu);
  }
  static __device__ __forceinline__ void stage(char* img, int plb, unsigned off, unsigned lo, unsigned hi) {
    *reinterpret_cast<unsigned short*>(img + off) = (unsigned short)lo;
    *reinterpret_cast<unsigned short*>(img + plb + off) = (unsigned short)(lo >> 16);
    *reinterpret_cast<unsigned short*>(img + 2 * plb + off) = (unsigned short)hi;
  }
};
// geometry of the images [16 rows][n k-values] under a policy: elements per row, bytes of one term image, of all of them
template <class OP> constexpr int op_ld(int n) { return n + OP::PAD; }
template <class OP> constexpr int op_term_bytes(int n) { return 16 * op_ld<OP>(n) * (int)sizeof(typename OP::elem); }
template <class OP> constexpr int op_image_bytes(int n) { return OP::TERMS * op_term_bytes<OP>(n); }
}  // namespace
