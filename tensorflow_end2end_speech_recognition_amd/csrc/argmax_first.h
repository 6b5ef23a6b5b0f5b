// The first maximum of a row of floats, one statement for every kernel that needs it (asr_argmax_rows and the two
// token-selection kernels of the decoder loops), so that they agree on ties: the lower index wins.
#pragma once
#include "common.h"

// One wave over p[start], p[start + stride], ... below C: every lane returns the wave's (best, bi); bi stays 0x7fffffff
// when nothing compared greater than -inf.
__device__ __forceinline__ void argmax_first_wave(const float* __restrict__ p, int C, int start, int stride, float& best,
                                                  int& bi) {
  best = -INFINITY;
  bi = 0x7fffffff;
  for (int k = start; k < C; k += stride) {
    const float v = p[k];
    if (v > best || (v == best && k < bi)) { best = v; bi = k; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
}
// the index a caller emits: 0 where no element was found
__device__ __forceinline__ int argmax_first_id(int bi) { return bi == 0x7fffffff ? 0 : bi; }

// A workgroup of 256 threads (4 waves) over one row; every thread returns the id.  It holds a barrier: every thread
// calls it, under a condition that is uniform over the workgroup.
__device__ __forceinline__ int argmax_first_block256(const float* __restrict__ p, int C) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float best;
  int bi;
  argmax_first_wave(p, C, threadIdx.x, 256, best, bi);
  if (lane == 0) { sv[w] = best; si[w] = bi; }
  __syncthreads();
  best = sv[0]; bi = si[0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (sv[i] > best || (sv[i] == best && si[i] < bi)) { best = sv[i]; bi = si[i]; }
  return argmax_first_id(bi);
}
