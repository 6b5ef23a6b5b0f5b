// LDS image of the reduction-major ("TN") MFMA products and its transposing fragment read: gemm.hip's gemm_tn_bf16_kernel,
// conv3x3.hip's conv3x3_wgrad_tr_kernel and vgg.hip's small-channel weight gradient.  Tiles are copied into LDS as they
// lie in memory (one 16-byte vector = 8 columns of a k row), as 16-column subtiles [k][16], so that the 4 x 16 block a
// 16-lane group needs is 128 contiguous bytes; see gemm_tn_bf16_kernel for the layout.
#pragma once
#include "common.h"

constexpr int TN_SUB = 2048 + 32;                 // bytes from one 16-column subtile [64 k][16] to the next
constexpr int TN_OPER = 8 * TN_SUB;               // one operand tile: 128 columns
constexpr int TN_STAGE = 2 * TN_OPER;             // A tile | B tile
typedef __attribute__((ext_vector_type(4))) short bf16x4_t;
// one MFMA fragment = two ds_read_b64_tr_b16 (k 0-3 and 4-7 of the lane's eight, 4 k rows = 128 bytes apart): each lane
// passes the address of one 8-byte piece of the block and receives its COLUMN
__device__ __forceinline__ bf16x8_t tn_frag(const char* p) {
  typedef __attribute__((address_space(3))) bf16x4_t lds4_t;
  const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t*)(p));
  const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t*)(p + 128));
  return (bf16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
