// Time subsampling between two recurrent layers (subsample_list / subsample_type of the reference's recipes; the
// 'concat' form is what models/encoders/core/pyramidal_blstm.py:120-170 set out to build): a 2x reduction in time of the
// time-major output a recurrence wrote, handed to the next layer stack as the batch-major fp32 tensor its __call__ takes,
// and the exact transpose for the backward pass.  Pure data movement, HBM-bound: grid-stride over 16-byte groups where
// the row width allows it (cdna guide G13), one element per lane otherwise.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

inline int grid_for(size_t n) {
  size_t blocks = (n + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  return (int)blocks;
}

// G consecutive elements of T as fp32: one 16-byte load for (float, 4) and (bf16, 8), one element for G = 1
template <typename T, int G> struct Group;
template <typename T> struct Group<T, 1> {
  static __device__ __forceinline__ void load(const T* p, float* v) { v[0] = Elem<T>::to_f32(p[0]); }
};
template <> struct Group<float, 4> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const f32x4_t q = *reinterpret_cast<const f32x4_t*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  }
};
template <> struct Group<bf16_t, 8> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
    const u32x4_t q = *reinterpret_cast<const u32x4_t*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = __uint_as_float(q[j] << 16);
      v[2 * j + 1] = __uint_as_float(q[j] & 0xFFFF0000u);
    }
  }
};
template <int G> __device__ __forceinline__ void store_f32(float* p, const float* v) {
  if (G == 1) {
    p[0] = v[0];
  } else {
#pragma unroll
    for (int j = 0; j < G; j += 4) {
      f32x4_t q = {v[j], v[j + 1], v[j + 2], v[j + 3]};
      *reinterpret_cast<f32x4_t*>(p + j) = q;
    }
  }
}

__device__ __forceinline__ int half_len(int len, int T) { return min(max(len, 0), T) >> 1; }

// y[b, t', :] (fp32, batch-major, rows of Wo = W or 2W) from x[T, Bp, W]; groups of the OUTPUT enumerated in order.
// W % G == 0, so a group never straddles the two stacked frames of 'concat'.
template <typename T, int G, bool CONCAT>
__global__ __launch_bounds__(256) void subsample_fwd_kernel(const T* __restrict__ x, const int32_t* __restrict__ len_in,
                                                            int T_, int Bp, int B, int W, float* __restrict__ y,
                                                            int32_t* __restrict__ len_out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  for (size_t i = gid; i < (size_t)Bp; i += stride) len_out[i] = half_len(len_in[i], T_);
  const int T2 = T_ >> 1;
  const int Wo = CONCAT ? 2 * W : W;
  const int gpr = Wo / G;                                   // groups per output row
  const size_t total = (size_t)B * T2 * gpr;
  for (size_t i = gid; i < total; i += stride) {
    const int col = (int)(i % gpr) * G;
    const size_t r = i / gpr;
    const int t2 = (int)(r % T2);
    const int b = (int)(r / T2);
    float v[G];
    if (t2 < half_len(len_in[b], T_)) {                      // frames 2 t2, 2 t2 + 1 < 2 (len >> 1): never a padded one
      const int second = CONCAT ? (col >= W) : 1;
      const int c = CONCAT ? col - second * W : col;
      Group<T, G>::load(x + ((size_t)(2 * t2 + second) * Bp + b) * W + c, v);
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j) v[j] = 0.f;
    }
    store_f32<G>(y + r * Wo + col, v);
  }
}

// dx[T, Bp, W] from dy[T/2, Bp, Wo] (both fp32, time-major); groups of dx enumerated in order, every one written
template <int G, bool CONCAT>
__global__ __launch_bounds__(256) void subsample_bwd_kernel(const float* __restrict__ dy,
                                                            const int32_t* __restrict__ len_out, int T_, int Bp, int W,
                                                            float* __restrict__ dx) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const int T2 = T_ >> 1;
  const int Wo = CONCAT ? 2 * W : W;
  const int gpr = W / G;
  const size_t total = (size_t)T_ * Bp * gpr;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += stride) {
    const int col = (int)(i % gpr) * G;
    const size_t r = i / gpr;
    const int b = (int)(r % Bp);
    const int t = (int)(r / Bp);
    const int t2 = t >> 1, second = t & 1;
    float v[G];
    if (t2 < min(max(len_out[b], 0), T2) && (CONCAT || second)) {
      Group<float, G>::load(dy + ((size_t)t2 * Bp + b) * Wo + (CONCAT ? second * W : 0) + col, v);
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j) v[j] = 0.f;
    }
    store_f32<G>(dx + r * W + col, v);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T, int G>
void launch_fwd(int type, const void* x, const int32_t* len_in, int T_, int Bp, int B, int W, float* y,
                int32_t* len_out, hipStream_t st) {
  const size_t groups = (size_t)B * (T_ / 2) * ((type == ASR_SUBSAMPLE_CONCAT ? 2 * W : W) / G);
  const dim3 grid(grid_for(groups > (size_t)Bp ? groups : (size_t)Bp));
  if (type == ASR_SUBSAMPLE_CONCAT)
    hipLaunchKernelGGL((subsample_fwd_kernel<T, G, true>), grid, dim3(256), 0, st, (const T*)x, len_in, T_, Bp, B, W, y,
                       len_out);
  else
    hipLaunchKernelGGL((subsample_fwd_kernel<T, G, false>), grid, dim3(256), 0, st, (const T*)x, len_in, T_, Bp, B, W, y,
                       len_out);
}

template <int G>
void launch_bwd(int type, const float* dy, const int32_t* len_out, int T_, int Bp, int W, float* dx, hipStream_t st) {
  const dim3 grid(grid_for((size_t)T_ * Bp * (W / G)));
  if (type == ASR_SUBSAMPLE_CONCAT)
    hipLaunchKernelGGL((subsample_bwd_kernel<G, true>), grid, dim3(256), 0, st, dy, len_out, T_, Bp, W, dx);
  else
    hipLaunchKernelGGL((subsample_bwd_kernel<G, false>), grid, dim3(256), 0, st, dy, len_out, T_, Bp, W, dx);
}

}  // namespace

extern "C" int asr_time_subsample_fwd(asr_handle* h, int dtype, int type, const void* x_tb, const int32_t* len_in, int T,
                                      int Bp, int B, int W, float* y_bt, int32_t* len_out, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(asr_dtype_ok(dtype) && (type == ASR_SUBSAMPLE_DROP || type == ASR_SUBSAMPLE_CONCAT),
           "asr_time_subsample_fwd: dtype %d / type %d", dtype, type);
  ASR_NEED(len_in && len_out && T >= 0 && Bp >= 0 && B >= 0 && B <= Bp && W > 0,
           "asr_time_subsample_fwd: bad args (T %d, Bp %d, B %d, W %d)", T, Bp, B, W);
  ASR_NEED((size_t)T * (size_t)Bp * (size_t)W < ((size_t)1 << 40), "asr_time_subsample_fwd: tensor too large");
  const bool work = T / 2 > 0 && B > 0;
  ASR_NEED(!work || (x_tb && y_bt), "asr_time_subsample_fwd: null tensor");
  if (Bp == 0) return ASR_OK;                      // (T/2 == 0 or B == 0: only the lengths are written)
  hipStream_t st = (hipStream_t)s;
  const bool al = aligned16(x_tb) && aligned16(y_bt);
  if (dtype == ASR_F32) {
    if (al && W % 4 == 0) launch_fwd<float, 4>(type, x_tb, len_in, T, Bp, B, W, y_bt, len_out, st);
    else launch_fwd<float, 1>(type, x_tb, len_in, T, Bp, B, W, y_bt, len_out, st);
  } else {
    if (al && W % 8 == 0) launch_fwd<bf16_t, 8>(type, x_tb, len_in, T, Bp, B, W, y_bt, len_out, st);
    else launch_fwd<bf16_t, 1>(type, x_tb, len_in, T, Bp, B, W, y_bt, len_out, st);
  }
  ASR_CHECK_LAUNCH(h, "asr_time_subsample_fwd");
  return ASR_OK;
}

extern "C" int asr_time_subsample_bwd(asr_handle* h, int type, const float* dy_tb, const int32_t* len_out, int T, int Bp,
                                      int W, float* dx_tb, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(type == ASR_SUBSAMPLE_DROP || type == ASR_SUBSAMPLE_CONCAT, "asr_time_subsample_bwd: type %d", type);
  ASR_NEED(len_out && T >= 0 && Bp >= 0 && W > 0, "asr_time_subsample_bwd: bad args (T %d, Bp %d, W %d)", T, Bp, W);
  ASR_NEED((size_t)T * (size_t)Bp * (size_t)W < ((size_t)1 << 40), "asr_time_subsample_bwd: tensor too large");
  if (T == 0 || Bp == 0) return ASR_OK;
  ASR_NEED(dx_tb && (dy_tb || T / 2 == 0), "asr_time_subsample_bwd: null tensor");
  hipStream_t st = (hipStream_t)s;
  if (W % 4 == 0 && aligned16(dy_tb) && aligned16(dx_tb)) launch_bwd<4>(type, dy_tb, len_out, T, Bp, W, dx_tb, st);
  else launch_bwd<1>(type, dy_tb, len_out, T, Bp, W, dx_tb, st);
  ASR_CHECK_LAUNCH(h, "asr_time_subsample_bwd");
  return ASR_OK;
}
