// Gaussian weight noise (weight_noise_std of the reference's config/ctc/regularization/blstm_ctc_weight_noise.yml,
// config/attention/regularization/att_blstm_location_weight_noise.yml and att_baseline.yml -- keys none of its code reads;
// Graves 2011 / 2013): once per training step the flat parameter buffer is saved and perturbed in ONE pass,
// backup[i] = w[i], w[i] = w[i] + std * z[i], z = asr_normal_words of block offset + i / 4 (common.h).  The clean weights
// come back by a device-to-device copy of the backup; there is no kernel for that.
// HBM-bound by design, 12 bytes per element: grid-stride, one Philox block per lane = four elements = one 16-byte load and
// two 16-byte stores (cdna guide G13); the block that holds the n % 4 tail, and every block of a buffer that is not
// 16-byte aligned, goes element by element.  The product and the sum are separate roundings (the statement is
// w + fl(std * z)), so build.py compiles this file with -ffp-contract=off, like residual.hip.
#include "common.h"

namespace {

inline int grid_for(size_t n) {
  size_t blocks = (n + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  return (int)blocks;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// VEC: w and backup are 16-byte aligned.  The entry point rejects overlapping buffers.
template <bool VEC>
__global__ __launch_bounds__(256) void weight_noise_kernel(float* __restrict__ w, float* __restrict__ backup, size_t n,
                                                           float std, uint64_t seed, uint64_t offset) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t groups = (n + 3) >> 2;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < groups; q += stride) {
    const size_t e0 = q << 2;
    float z[4];
    asr_normal_words(offset + q, seed, z);
    if (VEC && e0 + 4 <= n) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(w + e0);
      *reinterpret_cast<f32x4_t*>(backup + e0) = v;
      f32x4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __fadd_rn(v[j], __fmul_rn(std, z[j]));
      *reinterpret_cast<f32x4_t*>(w + e0) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e0 + j < n) {
          const float v = w[e0 + j];
          backup[e0 + j] = v;
          w[e0 + j] = __fadd_rn(v, __fmul_rn(std, z[j]));
        }
      }
    }
  }
}

}  // namespace

extern "C" int asr_weight_noise_perturb(asr_handle* h, float* w, float* backup, size_t n, float std, uint64_t seed,
                                        uint64_t offset, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(std >= 0.f && std <= 3.0e38f, "asr_weight_noise_perturb: std must be finite and >= 0");
  ASR_NEED(n < ((size_t)1 << 40), "asr_weight_noise_perturb: buffer too large");
  if (n == 0) return ASR_OK;
  ASR_NEED(w && backup, "asr_weight_noise_perturb: null buffer");
  ASR_NEED(backup + n <= w || w + n <= backup, "asr_weight_noise_perturb: backup overlaps the weights");
  hipStream_t st = (hipStream_t)s;
  const bool vec = aligned16(w) && aligned16(backup);
  h->weight_noise_counts[0] += 1;
  h->weight_noise_counts[1] += n;
  if (std == 0.f) {
    // w + 0 * z would turn a -0 into +0: the weights stay bit for bit, only the backup is taken
    if (hipMemcpyAsync(backup, w, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
      ASR_FAIL(h, ASR_ERR_HIP, "asr_weight_noise_perturb: device copy failed");
    return ASR_OK;
  }
  const int grid = grid_for((n + 3) >> 2);
  if (vec) {
    h->weight_noise_counts[2] += 1;
    hipLaunchKernelGGL((weight_noise_kernel<true>), dim3(grid), dim3(256), 0, st, w, backup, n, std, seed, offset);
  } else {
    hipLaunchKernelGGL((weight_noise_kernel<false>), dim3(grid), dim3(256), 0, st, w, backup, n, std, seed, offset);
  }
  ASR_CHECK_LAUNCH(h, "asr_weight_noise_perturb");
  return ASR_OK;
}

ASR_DEFINE_COUNTS(weight_noise_counts, weight_noise_counts)
