// Device side of the cluster recurrences (lstm_cluster.hip, lstm_cluster_f32.hip, gru_cluster.hip): the placement-independent
// hand-off between the workgroups of a cluster -- 8-byte {tag, payload} granules and 4-byte self-tagged words, the data IS
// the flag (cdna_hip_programming.md G16 "R2") -- the cluster / XCD placement, the LDS swizzle and the DPP moves the kernels
// share.  Internal linkage: every unit that includes this gets its own copy, nothing here has state.
#pragma once
#include "common.h"

namespace {
typedef unsigned long long u64;
typedef __attribute__((ext_vector_type(4))) __bf16 cbf16x4_t;

constexpr int HS = 64;                 // units per CU
constexpr unsigned SPIN_LIMIT = 4000000u;

__device__ __forceinline__ float cfsig(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float cftanh(float x) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x));
}
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
  return __builtin_bit_cast(unsigned, (bf2){(__bf16)lo, (__bf16)hi});
}
__device__ __forceinline__ void gstore(u64* p, unsigned epoch, unsigned payload) {
  __hip_atomic_store(p, ((u64)epoch << 32) | payload, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 gload(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 16-byte exchange store of self-tagged words.  Same-XCD cluster: plain store (stays in the shared
// L2); otherwise sc1 (write-through), as the agent-scope atomics lower to.  Inline asm pins the store
// in program order (a plain C++ store could legally sink below the spin loop that follows).
__device__ __forceinline__ void xstore16(f32x4_t* ubase, unsigned voff, f32x4_t v, bool fast) {
  // uniform base in SGPRs + 32-bit per-lane byte offset: no 64-bit pointer registers per slot
  // (s_nop 4 in front: a base restored from a spill lane by v_readlane is a VALU-written SGPR, which a VMEM address may
  // only use 5 wait states later -- the compiler cannot see that hazard inside the block; see the XP publish)
  if (fast) asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(ubase) : "memory");
  else asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(ubase) : "memory");
}
// ---- forward exchange with 4-byte SELF-TAGGED words (XW) ----
// h = o * tanh(c) lies in [-1, 1], so the top exponent bit of its bf16 form (bit 14) is always 0: the two free bits of a
// packed {bf16, bf16} word (bits 14 and 30) carry a 2-bit step tag and the DATA IS THE FLAG at 4-byte granularity -- no
// separate tag word (half of every polled byte in the 8-byte {tag, payload} granules), tear-proof for any load / store
// width because every 4-byte word validates itself.  tag(s) = ((s >> 1) + 1) & 3 for the slot of parity s & 1: 1 on the
// first write into the zeroed area, a different value on each of the next three writes to the same word (a consumer is
// never more than one write behind, see the poll).  The publisher FORCES the two bits, so a NaN (exponent all ones)
// cannot forge a tag and stall the cluster.
constexpr unsigned XW_MASK = 0x40004000u;
__device__ __forceinline__ unsigned xw_tag(int s) {
  const unsigned t = (((unsigned)s >> 1) + 1u) & 3u;
  return ((t & 1u) << 14) | ((t & 2u) << 29);
}
typedef __attribute__((ext_vector_type(4))) unsigned xw4_t;
// uniform base + per-lane element offset (lets the backend use the SGPR-base addressing mode)
template <typename T>
__device__ __forceinline__ T* uoff(T* ubase, unsigned elem) {
  return ubase + elem;   // plain pointer arithmetic: an integer round trip would demote it to a flat pointer
}

// The exchange area is double-buffered ACROSS launches: launch n runs on area n % 2 and, as its first act, zeroes the
// part of the other area the previous launch dirtied (all workgroups of the grid help: < 3 stores per thread), so the
// next launch finds clean tags without a memset launch in front of every recurrence kernel (10 per training step,
// each ~6 us on the critical path).  The host side tracks the dirty extent of both areas (asr_handle::xch_dirty).
__device__ __forceinline__ void zero_next_area(u64* __restrict__ znext, unsigned zwords) {
  const unsigned nthreads = gridDim.x * blockDim.x;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < zwords; i += nthreads) znext[i] = 0;
}
constexpr int CT8 = 512;               // threads of an eight-wave workgroup
// LDS images [16 rows][...] read as MFMA A fragments with ds_read_b128: row stride = 33 x 16 B.  The
// hardware services a wave in lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... (rows 0-3,12-15
// of k-block q together with rows 4-11 of k-block q^1), so a plain row-major image always has one
// 2-way bank conflict per group; swapping the two 16-byte halves of every 32 B for rows 4-11 makes
// each group hit 16 distinct 16-byte slots.  Byte offset XOR applied by writers and readers alike.
__device__ __forceinline__ unsigned lds_swz(int row) { return (((row + 4) >> 3) & 1) ? 16u : 0u; }

__device__ __forceinline__ float dpp_ror8(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));
}
__device__ __forceinline__ float dpp_xor1(float v) {   // quad_perm [1,0,3,2]
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
}

// ---------------------------------------------------------------- cluster placement
// Cluster c = tile * ndir + dir.  Block b of the 1-D grid: XCD slot x = b % 8, q = b / 8,
// member g = q % G, round = q / G, cluster c = round * 8 + x.  grid = 8 * G * ceil(nclusters / 8).
// A launch covers the TILE RANGE [tile0, tile0 + ntl) of the batch (one launch: tile0 = 0, ntl = B / 16; a batch that needs
// more clusters than the chip has CUs for runs as several launches over consecutive ranges, see cluster_tile_plan).  c is
// LOCAL to the launch (tile - tile0) * ndir + dir: it picks the cluster's exchange slots and placement header -- handed out
// per launch -- and decides `valid`.  `tile` is the GLOBAL tile: everything in memory (B stays the batch stride of every
// tensor; seq_len, the final states, the per-tile peephole / bias partials) is indexed with it.
struct ClusterId { int c, g, d, tile; bool valid; };
template <int G>
__device__ __forceinline__ ClusterId cluster_id(int ndir, int tile0, int ntl) {
  const int b = blockIdx.x, x = b & 7, q = b >> 3;
  ClusterId r;
  r.g = q % G;
  r.c = (q / G) * 8 + x;
  r.valid = r.c < ndir * ntl;
  r.d = r.c % ndir;
  r.tile = tile0 + r.c / ndir;
  return r;
}
static inline unsigned cluster_grid(int G, int nclusters) { return 8u * G * ((nclusters + 7) / 8); }

constexpr int XHDR = 16;                  // header granules per cluster (XCC ids of the members)
constexpr unsigned XCC_EPOCH = 0x80000001u;

// Every member publishes the XCC (= XCD) id it runs on with the placement-independent granule
// protocol and reads all G of them: true iff the whole cluster shares one XCD, hence one L2.
// Same inputs -> same answer on every member.
template <int G>
__device__ __forceinline__ bool same_xcd(u64* hdr, int g, bool& timed_out) {
  const unsigned mine = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xFu;   // HW_REG_XCC_ID[3:0]
  if (threadIdx.x == 0) gstore(hdr + g, XCC_EPOCH, mine);
  bool same = true;
#pragma unroll
  for (int i = 0; i < G; ++i) {
    u64 v = gload(hdr + i);
    unsigned spins = 0;
    while ((unsigned)(v >> 32) != XCC_EPOCH) {
      if (++spins > SPIN_LIMIT) { timed_out = true; break; }
      v = gload(hdr + i);
    }
    same = same && ((unsigned)v == mine);
  }
  return same;
}
// Granule publish.  Same-XCD cluster: a PLAIN 8-byte store stays in the shared L2, where the
// consumers' L1-bypassing (sc1) polls find it after ~an L2 round trip; an sc1 store would drop the
// line from L2 and make every poll a fabric round trip (MI355X_MICROARCH.md, store-flavour row).
// Otherwise: the write-through agent-scope store, correct for any placement.
__device__ __forceinline__ void gpublish(u64* p, unsigned epoch, unsigned payload, bool fast) {
  const u64 v = ((u64)epoch << 32) | payload;
  if (fast) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // plain store, no wait
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// masked DPP: lanes whose bank (lane & 15) >> 2 is in `BANKS` take `src` of lane (i + 8) % 16 of
// their row, the others keep `old` -- the halves swap without any v_cndmask
template <int BANKS>
__device__ __forceinline__ float dpp_ror8_into(float old, float src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old),
                                                                 __builtin_bit_cast(int, src), 0x128, 0xF, BANKS, false));
}
}  // namespace
