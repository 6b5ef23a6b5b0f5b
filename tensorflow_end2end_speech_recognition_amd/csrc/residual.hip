// Skip connections between two recurrent layers (encoder_residual / encoder_dense_residual of the reference's
// config/ctc/encoders/residual_blstm_ctc.yml, dense_residual_blstm_ctc.yml and their attention twins; semantics:
// models/encoders/core/residual.py).  Forward: the layer's dropout and the sum with what came before it in one pass,
// out = round(m * h + skip), optionally the running sum of the dense form; backward: the un-masked gradient sum that has
// to travel further down, g = dx_raw + carry, and the masked one the layer's BPTT kernel takes, dout = m * g.  Both know
// the frame counts: a padded frame is never loaded (dx_raw is unwritten there) and every output is zero there.
// HBM-bound: grid-stride over 16-byte groups where the row width allows it (cdna guide G13), one element per lane
// otherwise.  Multiplies and adds are separate roundings: the numpy statement has no fma.  HIP's __fmul_rn / __fadd_rn are
// plain operators, which the default -ffp-contract=fast fuses (v_pk_fma_f32 in the 8-wide forward kernel), so build.py
// compiles this file with -ffp-contract=off.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

inline int grid_for(size_t n) {
  size_t blocks = (n + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  return (int)blocks;
}

// G consecutive elements as fp32: 16-byte accesses for G > 1 (fp32: G / 4 of them; bf16: G = 8), one element for G = 1
template <int G> __device__ __forceinline__ void load_g(const float* p, float* v) {
  if constexpr (G == 1) {
    v[0] = p[0];
  } else {
#pragma unroll
    for (int j = 0; j < G; j += 4) {
      const f32x4_t q = *reinterpret_cast<const f32x4_t*>(p + j);
      v[j] = q[0]; v[j + 1] = q[1]; v[j + 2] = q[2]; v[j + 3] = q[3];
    }
  }
}
template <int G> __device__ __forceinline__ void load_g(const bf16_t* p, float* v) {
  if constexpr (G == 1) {
    v[0] = bf16_to_f32(p[0]);
  } else {
    static_assert(G == 8, "bf16 groups are 8 wide");
    const u32x4_t q = *reinterpret_cast<const u32x4_t*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = __uint_as_float(q[j] << 16);
      v[2 * j + 1] = __uint_as_float(q[j] & 0xFFFF0000u);
    }
  }
}
// stores v rounded to the element type and leaves in v what was stored (the dense sum adds the STORED value)
template <int G> __device__ __forceinline__ void store_g(float* p, float* v) {
  if constexpr (G == 1) {
    p[0] = v[0];
  } else {
#pragma unroll
    for (int j = 0; j < G; j += 4) {
      f32x4_t q = {v[j], v[j + 1], v[j + 2], v[j + 3]};
      *reinterpret_cast<f32x4_t*>(p + j) = q;
    }
  }
}
template <int G> __device__ __forceinline__ void store_g(bf16_t* p, float* v) {
  if constexpr (G == 1) {
    const bf16_t r = f32_to_bf16(v[0]);
    p[0] = r;
    v[0] = bf16_to_f32(r);
  } else {
    static_assert(G == 8, "bf16 groups are 8 wide");
    u32x4_t q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t lo = f32_to_bf16(v[2 * j]), hi = f32_to_bf16(v[2 * j + 1]);
      q[j] = lo | (hi << 16);
      v[2 * j] = __uint_as_float(lo << 16);
      v[2 * j + 1] = __uint_as_float(hi << 16);
    }
    *reinterpret_cast<u32x4_t*>(p) = q;
  }
}

// the dropout multipliers of elements e0 .. e0 + G - 1 of the tensor: element e takes word e % 4 of the block at
// offset + e / 4 (asr_dropout_mask's layout; 64-bit throughout: layer offsets are li << 32 on top of calls << 40).
// G > 1: e0 % 4 == 0, an 8-wide group spans two blocks.  keep >= 1: no dropout, every multiplier is 1.
template <int G>
__device__ __forceinline__ void mask_g(uint64_t e0, float keep, float inv, uint64_t seed, uint64_t offset, float* m) {
  if (keep >= 1.f) {
#pragma unroll
    for (int j = 0; j < G; ++j) m[j] = 1.f;
    return;
  }
  if constexpr (G == 1) {
    float w[4];
    asr_dropout_words(offset + (e0 >> 2), seed, keep, inv, w);
    const int k = (int)(e0 & 3);
    m[0] = k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3];
  } else {
#pragma unroll
    for (int j = 0; j < G; j += 4) asr_dropout_words(offset + (e0 >> 2) + (uint64_t)(j >> 2), seed, keep, inv, m + j);
  }
}

__device__ __forceinline__ int frames_of(int len, int T) { return min(max(len, 0), T); }

// out[T,Bp,W] = round(m * h + skip) at t < len[b], zero elsewhere; sum_out (nullable, fp32) = skip + out as stored.
// sum_out may be skip itself (an fp32 running sum updated in place): a lane loads its group of skip before it stores,
// and no other lane touches that group -- hence no __restrict__ on the two.
template <typename T, typename TS, int G>
__global__ __launch_bounds__(256) void residual_fwd_kernel(const T* __restrict__ h, const TS* skip,
                                                           const int32_t* __restrict__ len, int T_, int Bp, int W,
                                                           float keep, uint64_t seed, uint64_t offset, T* out,
                                                           float* sum_out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const float inv = 1.f / keep;
  const int gpr = W / G;                                     // groups per row
  const size_t total = (size_t)T_ * Bp * gpr;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += stride) {
    const size_t r = i / gpr;
    const int b = (int)(r % Bp);
    const int t = (int)(r / Bp);
    const size_t e0 = i * G;                                 // = r * W + col
    float o[G], sm[G];
    if (t < frames_of(len[b], T_)) {
      float hv[G], sk[G], m[G];
      load_g<G>(h + e0, hv);
      load_g<G>(skip + e0, sk);
      mask_g<G>(e0, keep, inv, seed, offset, m);
#pragma unroll
      for (int j = 0; j < G; ++j) o[j] = __fadd_rn(__fmul_rn(m[j], hv[j]), sk[j]);
      store_g<G>(out + e0, o);
#pragma unroll
      for (int j = 0; j < G; ++j) sm[j] = __fadd_rn(sk[j], o[j]);
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j) o[j] = sm[j] = 0.f;
      store_g<G>(out + e0, o);
    }
    if (sum_out) store_g<G>(sum_out + e0, sm);
  }
}

// g = dx_raw + carry; dout = m * g; carry_out = g (residual) or g + carry (dense) at t < len[b]; zero elsewhere.
// dout may be dx_raw and carry_out may be carry (each lane loads its groups before it stores): no __restrict__.
template <int G>
__global__ __launch_bounds__(256) void residual_bwd_kernel(const float* dx_raw, const float* carry,
                                                           const int32_t* __restrict__ len, int T_, int Bp, int W,
                                                           float keep, uint64_t seed, uint64_t offset, int dense,
                                                           float* dout, float* carry_out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const float inv = 1.f / keep;
  const int gpr = W / G;
  const size_t total = (size_t)T_ * Bp * gpr;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += stride) {
    const size_t r = i / gpr;
    const int b = (int)(r % Bp);
    const int t = (int)(r / Bp);
    const size_t e0 = i * G;
    float d[G], c[G];
    if (t < frames_of(len[b], T_)) {
      float dx[G], m[G];
      load_g<G>(dx_raw + e0, dx);
      load_g<G>(carry + e0, c);
      mask_g<G>(e0, keep, inv, seed, offset, m);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const float g = __fadd_rn(dx[j], c[j]);
        d[j] = __fmul_rn(m[j], g);
        c[j] = dense ? __fadd_rn(g, c[j]) : g;
      }
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j) d[j] = c[j] = 0.f;
    }
    store_g<G>(dout + e0, d);
    store_g<G>(carry_out + e0, c);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T, typename TS>
void launch_fwd(bool vec, const void* h, const void* skip, const int32_t* len, int T_, int Bp, int W, float keep,
                uint64_t seed, uint64_t offset, void* out, float* sum_out, hipStream_t st) {
  constexpr int G = sizeof(T) == 2 ? 8 : 4;
  if (vec)
    hipLaunchKernelGGL((residual_fwd_kernel<T, TS, G>), dim3(grid_for((size_t)T_ * Bp * (W / G))), dim3(256), 0, st,
                       (const T*)h, (const TS*)skip, len, T_, Bp, W, keep, seed, offset, (T*)out, sum_out);
  else
    hipLaunchKernelGGL((residual_fwd_kernel<T, TS, 1>), dim3(grid_for((size_t)T_ * Bp * W)), dim3(256), 0, st,
                       (const T*)h, (const TS*)skip, len, T_, Bp, W, keep, seed, offset, (T*)out, sum_out);
}

}  // namespace

extern "C" int asr_residual_fwd(asr_handle* h, int dtype, int skip_dtype, const void* h_tb, const void* skip,
                                const int32_t* seq_len, int T, int Bp, int W, float keep_prob, uint64_t seed,
                                uint64_t offset, void* out, float* sum_out, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(asr_dtype_ok(dtype) && (skip_dtype == dtype || skip_dtype == ASR_F32),
           "asr_residual_fwd: dtype %d / skip dtype %d", dtype, skip_dtype);
  ASR_NEED(T >= 0 && Bp >= 0 && W > 0, "asr_residual_fwd: bad args (T %d, Bp %d, W %d)", T, Bp, W);
  ASR_NEED(keep_prob > 0.f && keep_prob <= 1.f, "asr_residual_fwd: keep_prob must be in (0,1]");
  ASR_NEED((size_t)T * (size_t)Bp * (size_t)W < ((size_t)1 << 40), "asr_residual_fwd: tensor too large");
  if (T == 0 || Bp == 0) return ASR_OK;
  ASR_NEED(h_tb && skip && seq_len && out, "asr_residual_fwd: null tensor");
  ASR_NEED(out != h_tb && out != skip, "asr_residual_fwd: out must not alias an input");
  ASR_NEED((const void*)sum_out != h_tb && (const void*)sum_out != out &&
               ((const void*)sum_out != skip || skip_dtype == ASR_F32),
           "asr_residual_fwd: sum_out may alias an fp32 skip only");
  hipStream_t st = (hipStream_t)s;
  const bool al = aligned16(h_tb) && aligned16(skip) && aligned16(out) && aligned16(sum_out);
  if (dtype == ASR_F32) {
    launch_fwd<float, float>(al && W % 4 == 0, h_tb, skip, seq_len, T, Bp, W, keep_prob, seed, offset, out, sum_out, st);
  } else if (skip_dtype == ASR_F32) {
    launch_fwd<bf16_t, float>(al && W % 8 == 0, h_tb, skip, seq_len, T, Bp, W, keep_prob, seed, offset, out, sum_out, st);
  } else {
    launch_fwd<bf16_t, bf16_t>(al && W % 8 == 0, h_tb, skip, seq_len, T, Bp, W, keep_prob, seed, offset, out, sum_out, st);
  }
  ASR_CHECK_LAUNCH(h, "asr_residual_fwd");
  return ASR_OK;
}

extern "C" int asr_residual_bwd(asr_handle* h, const float* dx_raw, const float* carry, const int32_t* seq_len, int T,
                                int Bp, int W, float keep_prob, uint64_t seed, uint64_t offset, int dense, float* dout,
                                float* carry_out, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(T >= 0 && Bp >= 0 && W > 0, "asr_residual_bwd: bad args (T %d, Bp %d, W %d)", T, Bp, W);
  ASR_NEED(keep_prob > 0.f && keep_prob <= 1.f, "asr_residual_bwd: keep_prob must be in (0,1]");
  ASR_NEED((size_t)T * (size_t)Bp * (size_t)W < ((size_t)1 << 40), "asr_residual_bwd: tensor too large");
  if (T == 0 || Bp == 0) return ASR_OK;
  ASR_NEED(dx_raw && carry && seq_len && dout && carry_out, "asr_residual_bwd: null tensor");
  ASR_NEED(dout != carry_out && dout != carry && carry_out != dx_raw,
           "asr_residual_bwd: dout may alias dx_raw and carry_out may alias carry, nothing else");
  hipStream_t st = (hipStream_t)s;
  if (W % 4 == 0 && aligned16(dx_raw) && aligned16(carry) && aligned16(dout) && aligned16(carry_out))
    hipLaunchKernelGGL((residual_bwd_kernel<4>), dim3(grid_for((size_t)T * Bp * (W / 4))), dim3(256), 0, st, dx_raw,
                       carry, seq_len, T, Bp, W, keep_prob, seed, offset, dense, dout, carry_out);
  else
    hipLaunchKernelGGL((residual_bwd_kernel<1>), dim3(grid_for((size_t)T * Bp * W)), dim3(256), 0, st, dx_raw, carry,
                       seq_len, T, Bp, W, keep_prob, seed, offset, dense, dout, carry_out);
  ASR_CHECK_LAUNCH(h, "asr_residual_bwd");
  return ASR_OK;
}
