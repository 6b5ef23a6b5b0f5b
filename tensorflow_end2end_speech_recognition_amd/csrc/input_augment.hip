// On-device input augmentation for one training step (EXTENSION: the reference declares _add_noise_to_inputs(inputs,
// stddev=0.075) at models/model_base.py:40-55 with its body commented out; frequency / time masking: Park et al. 2019):
// y = x with Gaussian noise on every valid element and up to 8 frequency and 8 time masks per utterance, in ONE pass over
// the batch-major [B,T,F] fp32 features.  The statement is in include/asr_hip.h; z = asr_normal_words, the mask draws
// are asr_philox_block (common.h).
// HBM-bound by design, 8 bytes per element.  A workgroup belongs to one utterance: its first 16 lanes draw the
// utterance's mask slots into LDS once, then every lane takes groups of four consecutive FLAT elements (one Philox block
// per group) -- one 16-byte load and one 16-byte store where both pointers are 16-byte aligned and the group lies inside
// the utterance's valid frames (or inside its padded ones: a plain copy), element by element otherwise (cdna guide G13).
// With F % 4 != 0 groups straddle rows, and with T·F % 4 != 0 utterances: the two workgroups that share such a group each
// write their own elements of it.  The Box-Muller work is skipped for a group whose elements are all masked or padded.
// The product and the sum are separate roundings (v = x + fl(std * z)), so build.py compiles this file with
// -ffp-contract=off, like weight_noise.hip.
#include "common.h"

namespace {

constexpr int MAX_MASKS = 8;

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct aug_args {
  int T, F, n_ch;
  float noise_std;
  int n_fmask, fmask_width, n_tmask, tmask_width;
  float tmask_ratio, mask_value;
  uint64_t seed, offset;
};

// VEC: x and y are 16-byte aligned.  The entry point rejects overlapping buffers.  Grid: B * nblk workgroups, workgroup
// b * nblk + k strides over utterance b's groups from k.
template <bool VEC>
__global__ __launch_bounds__(256) void input_augment_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            const int32_t* __restrict__ seq_len, int nblk, aug_args a) {
  // slot m: [0, 8) frequency {start, end}, [8, 16) time {start, end}; an unused slot is empty
  __shared__ int s_lo[2 * MAX_MASKS], s_hi[2 * MAX_MASKS];
  const int b = blockIdx.x / nblk, k = blockIdx.x - b * nblk;
  int len = seq_len[b];
  len = len < 0 ? 0 : (len > a.T ? a.T : len);
  if (threadIdx.x < 2 * MAX_MASKS) {
    const int slot = threadIdx.x;
    int lo = 0, hi = 0;
    const bool freq = slot < MAX_MASKS;
    if (freq ? slot < a.n_fmask : slot - MAX_MASKS < a.n_tmask) {
      uint32_t c[4];
      asr_philox_block(a.offset + ((uint64_t)1 << 39) + 16ull * (uint64_t)b + (uint64_t)slot, a.seed, c);
      int cap, span;
      if (freq) {
        cap = a.fmask_width < a.n_ch ? a.fmask_width : a.n_ch;
        span = a.n_ch;
      } else {
        const int r = (int)floorf(__fmul_rn(a.tmask_ratio, (float)len));
        cap = a.tmask_width < r ? a.tmask_width : r;
        span = len;
      }
      const int w = (int)__umulhi(c[0], (uint32_t)(cap + 1));
      lo = (int)__umulhi(c[1], (uint32_t)(span - w + 1));
      hi = lo + w;
    }
    s_lo[slot] = lo;
    s_hi[slot] = hi;
  }
  __syncthreads();

  const uint64_t TF = (uint64_t)a.T * (uint64_t)a.F;
  const uint64_t e_lo = (uint64_t)b * TF, e_hi = e_lo + TF;
  const uint64_t q_end = (e_hi + 3) >> 2;
  const bool small = TF < ((uint64_t)1 << 32);
  const bool noisy = a.noise_std > 0.f;
  for (uint64_t q = (e_lo >> 2) + (uint64_t)k * 256u + threadIdx.x; q < q_end; q += (uint64_t)nblk * 256u) {
    const uint64_t e0 = q << 2;
    // frame and column of the group's first element that belongs to this utterance
    const int j0 = e0 < e_lo ? (int)(e_lo - e0) : 0;
    const uint64_t rel = e0 + j0 - e_lo;
    int t, f;
    if (small) {
      t = (int)((uint32_t)rel / (uint32_t)a.F);
      f = (int)((uint32_t)rel - (uint32_t)t * (uint32_t)a.F);
    } else {
      t = (int)(rel / (uint64_t)a.F);
      f = (int)(rel - (uint64_t)t * (uint64_t)a.F);
    }
    int c = (int)((uint32_t)f % (uint32_t)a.n_ch);
    const bool whole = j0 == 0 && e0 + 4 <= e_hi;
    // frame and base channel of each element (-1: not this utterance's)
    int tj[4], cj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tj[j] = -1;
      cj[j] = 0;
      if (j < j0 || e0 + j >= e_hi) continue;
      tj[j] = t;
      cj[j] = c;
      ++f;
      ++c;
      if (f == a.F) {
        f = 0;
        c = 0;
        ++t;
      } else if (c == a.n_ch) {
        c = 0;
      }
    }
    // one pass over the slots: each bound is read from LDS once per group
    bool masked[4] = {false, false, false, false};
    for (int m = 0; m < a.n_fmask; ++m) {
      const int lo = s_lo[m], hi = s_hi[m];
#pragma unroll
      for (int j = 0; j < 4; ++j) masked[j] = masked[j] || (cj[j] >= lo && cj[j] < hi);
    }
    for (int m = 0; m < a.n_tmask; ++m) {
      const int lo = s_lo[MAX_MASKS + m], hi = s_hi[MAX_MASKS + m];
#pragma unroll
      for (int j = 0; j < 4; ++j) masked[j] = masked[j] || (tj[j] >= lo && tj[j] < hi);
    }
    // per element: 0 = not ours, 1 = copy (padded frame), 2 = masked, 3 = value (with noise)
    int kind[4];
    bool any_value = false, all_pad = true, all_valid = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      kind[j] = tj[j] < 0 ? 0 : (tj[j] >= len ? 1 : (masked[j] ? 2 : 3));
      any_value = any_value || kind[j] == 3;
      all_pad = all_pad && kind[j] == 1;
      all_valid = all_valid && kind[j] >= 2;
    }
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (noisy && any_value) asr_normal_words(a.offset + q, a.seed, z);
    if (VEC && whole && (all_pad || all_valid)) {
      // (a group inside a time mask is not read)
      const bool all_masked = kind[0] == 2 && kind[1] == 2 && kind[2] == 2 && kind[3] == 2;
      f32x4_t v = {0.f, 0.f, 0.f, 0.f};
      if (!all_masked) v = *reinterpret_cast<const f32x4_t*>(x + e0);
      f32x4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float r = v[j];
        if (kind[j] == 3 && noisy) r = __fadd_rn(r, __fmul_rn(a.noise_std, z[j]));
        if (kind[j] == 2) r = a.mask_value;
        o[j] = r;
      }
      *reinterpret_cast<f32x4_t*>(y + e0) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (kind[j] == 0) continue;
        float r = a.mask_value;
        if (kind[j] != 2) {
          r = x[e0 + j];
          if (kind[j] == 3 && noisy) r = __fadd_rn(r, __fmul_rn(a.noise_std, z[j]));
        }
        y[e0 + j] = r;
      }
    }
  }
}

}  // namespace

extern "C" int asr_input_augment(asr_handle* h, const float* x, float* y, const int32_t* seq_len, int B, int T, int F,
                                 int n_ch, float noise_std, int n_fmask, int fmask_width, int n_tmask, int tmask_width,
                                 float tmask_ratio, float mask_value, uint64_t seed, uint64_t offset, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  ASR_NEED(B >= 0 && T >= 0 && F >= 1, "asr_input_augment: B, T >= 0 and F >= 1");
  ASR_NEED(n_ch >= 1 && n_ch <= F && F % n_ch == 0, "asr_input_augment: n_ch must be in [1, F] and divide F");
  ASR_NEED(n_fmask >= 0 && n_fmask <= MAX_MASKS && n_tmask >= 0 && n_tmask <= MAX_MASKS,
           "asr_input_augment: mask counts must be in [0, 8]");
  ASR_NEED(fmask_width >= 0 && tmask_width >= 0, "asr_input_augment: mask widths must be >= 0");
  ASR_NEED(tmask_ratio >= 0.f && tmask_ratio <= 1.f, "asr_input_augment: tmask_ratio must be in [0, 1]");
  ASR_NEED(noise_std >= 0.f && noise_std <= 3.0e38f, "asr_input_augment: noise_std must be finite and >= 0");
  ASR_NEED(mask_value >= -3.4e38f && mask_value <= 3.4e38f, "asr_input_augment: mask_value must be finite");
  // (the noise counters of one call stay below 2^39 blocks)
  const unsigned __int128 n128 = (unsigned __int128)B * (unsigned __int128)T * (unsigned __int128)F;
  ASR_NEED(n128 < ((unsigned __int128)1 << 41), "asr_input_augment: B*T*F must be below 2^41");
  const size_t n = (size_t)n128;
  if (n == 0) return ASR_OK;
  ASR_NEED(x && y && seq_len, "asr_input_augment: null buffer");
  ASR_NEED(y + n <= x || x + n <= y, "asr_input_augment: y overlaps x");
  hipStream_t st = (hipStream_t)s;
  h->input_augment_counts[0] += 1;
  h->input_augment_counts[1] += n;
  if (fmask_width == 0) n_fmask = 0;
  if (tmask_width == 0 || tmask_ratio == 0.f) n_tmask = 0;
  if (noise_std == 0.f && n_fmask == 0 && n_tmask == 0) {
    if (hipMemcpyAsync(y, x, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
      ASR_FAIL(h, ASR_ERR_HIP, "asr_input_augment: device copy failed");
    return ASR_OK;
  }
  const size_t groups = ((size_t)T * (size_t)F + 3) / 4 + 1;   // per utterance, a straddling first group included
  size_t nblk = (groups + 255) / 256;
  const size_t cap = (size_t)B >= 2048 ? 1 : 2048 / (size_t)B;
  if (nblk > cap) nblk = cap;
  const aug_args a = {T, F, n_ch, noise_std, n_fmask, fmask_width, n_tmask, tmask_width, tmask_ratio, mask_value,
                      seed, offset};
  const dim3 grid((unsigned)((size_t)B * nblk));
  if (aligned16(x) && aligned16(y)) {
    h->input_augment_counts[2] += 1;
    hipLaunchKernelGGL((input_augment_kernel<true>), grid, dim3(256), 0, st, x, y, seq_len, (int)nblk, a);
  } else {
    hipLaunchKernelGGL((input_augment_kernel<false>), grid, dim3(256), 0, st, x, y, seq_len, (int)nblk, a);
  }
  ASR_CHECK_LAUNCH(h, "asr_input_augment");
  return ASR_OK;
}

ASR_DEFINE_COUNTS(input_augment_counts, input_augment_counts)
