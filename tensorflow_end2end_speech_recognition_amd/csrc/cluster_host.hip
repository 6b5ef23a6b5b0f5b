// Host side of the cluster recurrences (cluster_launch.h), everything that exists ONCE per process: the run-time flags and
// the CU budget the tests set, the cached environment switches, the exchange-area bookkeeping and tile-group planning, the
// handle's path / kernel counters, the sticky error word's entry points and the tear probe.
#include "cluster_launch.h"
#include <stdlib.h>

static int g_dflags = -1;
// bit 4 (16): force the placement-independent write-through exchange
// bit 5 (32): invert the default choice of the EARLY forward variant (A/B measurements)
// bit 7 (128): BPTT kernel requests the next iteration's saved activations ahead of the poll loop (the old place; A/B)
// bit 8 (256): fp32 BPTT kernel without the priority of the published tile's MFMAs (A/B)
// bit 9 (512): clusters of H/64 CUs x eight waves instead of H/32 CUs x four waves: bf16 H = 256 / 512 (H = 320 has only
//              that form), fp32 H = 128; fp32 H = 256 / 320 / 512 have no such form and fall to the single-CU kernels
// bit 10 (1024): forward all-gather with 8-byte {step, payload} granules instead of 4-byte self-tagged words (A/B, tests)
// bit 11 (2048): inverts the default choice of the BPTT reduce-scatter slot layout (consumer-major source pairs, XP) (A/B, tests)
// bit 12 (4096): fp32 operands on the exact-fp32 MFMA kernels instead of the three-term bf16 split (A/B, tests)
// bit 13 (8192): inverts the choice between the 16-CU and the 8-CU forward form at H = 256 (A/B, tests)
// bit 6 (64): TEST ONLY -- the last member of every cluster leaves right after the placement handshake and the
//             spin limit drops to 2000 polls, so every hand-off times out (tests/test_gpu_ops.py checks that the
//             error word is raised and surfaces as an exception)
int dbg_flags() {
  if (g_dflags < 0) { const char* e = getenv("ASR_LSTM_DFLAGS"); g_dflags = e ? atoi(e) : 0; }
  return g_dflags;
}
extern "C" int asr_debug_set_lstm_flags(int flags) { g_dflags = flags; return 0; }
int kernel_flags() {
  return ((dbg_flags() & 16) ? 1 : 0) | ((dbg_flags() & 64) ? 2 : 0) | ((dbg_flags() & 128) ? 4 : 0) |
         ((dbg_flags() & 256) ? 8 : 0);
}
// an environment switch that is on unless its value starts with 0; every switch that uses it reads its variable once
static bool env_on(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }
bool cluster_enabled() { static const bool on = env_on("ASR_LSTM_CLUSTER"); return on; }
// H = 320 (the width of most of the reference's recipes): five CUs per (direction, tile).  ASR_LSTM_CLUSTER_320=0
// keeps the single-CU kernels for that width (A/B).
bool cluster_320_enabled() { static const bool on = env_on("ASR_LSTM_CLUSTER_320"); return on; }

XchAreas xch_take(asr_handle* h, char* base, size_t need, hipStream_t st) {
  const int a = h->xch_next & 1, o = a ^ 1;
  char* area = base + 256 + (size_t)a * XCH_HALF;
  char* other = base + 256 + (size_t)o * XCH_HALF;
  if (h->xch_dirty[a]) {
    (void)hipMemsetAsync(area, 0, h->xch_dirty[a], st);
    h->xch_dirty[a] = 0;
  }
  XchAreas x;
  x.area = (u64*)area;
  x.znext = (u64*)other;
  x.zwords = (unsigned)(h->xch_dirty[o] / sizeof(u64));
  h->xch_dirty[o] = 0;
  h->xch_dirty[a] = (need + 7) & ~(size_t)7;
  h->xch_next = o;
  return x;
}

// ---------------------------------------------------------------- tile groups
// Every member of a launch must be resident at once (one workgroup per CU), so a launch holds at most
// 8 * floor(budget / (8 G)) clusters.  A batch with more (tile, direction) pairs runs as consecutive launches over tile
// ranges: clusters never talk to each other, so the ranges are independent and each launch is the same kernel with a
// first tile.  The plan is the minimal number of groups: full groups of `per` tiles and one partial group at the end.
static TilePlan cluster_tile_plan(int G, int ndir, int tiles, int budget) {
  TilePlan p = {0, 0};
  if (G < 1 || ndir < 1 || ndir > 8 || tiles < 1 || budget < 1) return p;
  const int per = (budget / (8 * G)) * 8 / ndir;          // largest m with cluster_grid(G, m * ndir) <= budget
  if (per < 1) return p;
  p.per = per < tiles ? per : tiles;
  p.n = (tiles + p.per - 1) / p.per;
  return p;
}
extern "C" int asr_cluster_tile_groups(int G, int ndir, int tiles, int cu_budget, int* first_tile, int* ntiles,
                                       int max_groups) {
  if (G < 1 || (ndir != 1 && ndir != 2) || tiles < 1 || cu_budget < 1 || max_groups < 0) return ASR_ERR_INVALID_ARG;
  const TilePlan p = cluster_tile_plan(G, ndir, tiles, cu_budget);
  for (int i = 0; i < p.n && i < max_groups; ++i) {
    if (first_tile) first_tile[i] = i * p.per;
    if (ntiles) ntiles[i] = (i + 1 < p.n) ? p.per : tiles - i * p.per;
  }
  return p.n;
}
// TEST ONLY: co-resident workgroups a cluster launch may use; 0 = the device's CU count.  Clamped to the CU count where it
// is used -- a grid larger than the chip would leave members spinning on peers that are not resident.  Process-wide and
// NOT thread-safe (a plain int every handle reads at launch time, like g_dflags): set it while no recurrence call runs.
static int g_cu_budget = 0;
extern "C" int asr_debug_set_cluster_cu_budget(int n) { g_cu_budget = n; return 0; }
static int cluster_cu_budget(const asr_handle* h) {
  return (g_cu_budget <= 0 || g_cu_budget > h->num_cu) ? h->num_cu : g_cu_budget;
}
// The plan of one launcher call: `grouped` false = exactly one launch or nothing (the shapes that fit keep their form and
// their single launch), true = any number of groups.  cl_bytes = exchange bytes per cluster: every group's slots must fit
// in one exchange area, so a grouped plan also shrinks its groups to what the area holds (a shape whose one launch fits the
// CUs but not the area is split too).
static TilePlan cluster_launch_plan(const asr_handle* h, int G, int ndir, int B, size_t cl_bytes, bool grouped) {
  const int tiles = B / 16;
  TilePlan p = cluster_tile_plan(G, ndir, tiles, cluster_cu_budget(h));
  const size_t area_tiles = XCH_HALF / ((size_t)ndir * cl_bytes);   // tiles whose clusters one area has slots for
  if (p.n && (size_t)p.per > area_tiles) {
    p.per = (int)area_tiles;
    p.n = p.per ? (tiles + p.per - 1) / p.per : 0;
  }
  if (p.n != 1 && !grouped) p.n = 0;
  return p;
}
ClusterCall cluster_call(const asr_handle* h, int G, int ndir, int B, size_t elems, size_t cl_bytes, bool grouped) {
  ClusterCall cc = {{0, 0}, nullptr};
  if (elems >= (1ull << 31) || h->scratch_bytes < XCH_BYTES) return cc;
  cc.plan = cluster_launch_plan(h, G, ndir, B, cl_bytes, grouped);   // every member of a launch must be resident at once
  cc.base = (char*)h->scratch + (h->scratch_bytes - XCH_BYTES);
  return cc;
}
void count_cluster_launches(asr_handle* h, int kind, int groups) {
  h->rec_counts[3 * kind + 0] += (unsigned long long)groups;
  if (groups > 1) h->rec_counts[3 * kind + 2] += 1;
}
ASR_DEFINE_COUNTS(recurrence_path_counts, rec_counts)
// the form each asr_lstm_fwd / asr_lstm_bwd(_ex) call on this handle ended in (host integers bumped where the form is
// chosen: the cluster launchers of lstm_cluster.hip and lstm_cluster_f32.hip, asr_lstm_fwd / lstm_bwd_impl for the single-CU kernels)
ASR_DEFINE_COUNTS_N(lstm_kernel_counts, lstm_counts)

// Units per CU of the H = 256 / 512 clusters: 32 (default since round 3: H/32 CUs with four waves each, one per SIMD) or
// 64 (H/64 CUs with eight waves; ASR_LSTM_HS=64, ASR_LSTM_FWD_HS / ASR_LSTM_BWD_HS for one pass only, or
// ASR_LSTM_DFLAGS bit 9 at run time -- the tests run both).  Measured (profiles/r03_cluster_hs32.md): forward
// 907 -> 866 us and BPTT 953 -> 929 us per launch at H = 256 (T = 778), 1791 -> 1374 and 2354 -> 1833 us at H = 512.
// The bf16 forward at H = 256 has a third form, 16 units per CU (lstm_fwd_cluster16_kernel: 16 CUs x four waves x 4 units).
// FWD_HS16_DEFAULT says whether it is the default there; ASR_LSTM_FWD_HS=16 / 32 / 64 picks a form, ASR_LSTM_DFLAGS bit 13
// inverts the choice between 16 and 32 at run time (tests, A/B).  Every other kernel reads 16 as 32.  Measured
// (profiles/r10_fwd_cu16.md): forward launch 694 -> 622 us at T = 745, B = 16, headline step 8.63 -> 8.34 ms, same bits.
static constexpr bool FWD_HS16_DEFAULT = true;
int units_per_cu(const char* specific, bool allow16) {
  if (dbg_flags() & 512) return 64;
  const char* e = getenv(specific);
  if (!e) e = getenv("ASR_LSTM_HS");
  const int v = e ? atoi(e) : 0;
  if (v == 64) return 64;
  if (!allow16) return 32;
  const bool cu16 = e ? v == 16 : FWD_HS16_DEFAULT;
  return (cu16 != ((dbg_flags() & 8192) != 0)) ? 16 : 32;
}
// forward all-gather word format: 4-byte self-tagged words unless ASR_LSTM_XW=0 or ASR_LSTM_DFLAGS bit 10 (run time, tests)
bool fwd_xw_enabled() { static const bool on = env_on("ASR_LSTM_XW"); return on && !(dbg_flags() & 1024); }
// BPTT reduce-scatter slot layout: consumer-major source pairs (XP) or one 16-byte slot per (source, tile).  Measured
// (round 4, us per BPTT launch, T = 778): H = 320 on five CUs x eight waves 1107 -> 1064 with XP, but H = 256 on eight CUs x
// four waves 851 -> 940 and H = 512 on sixteen 1520 -> 1790: with one wave per SIMD the doubled store count of the
// producers (two 8-byte stores per tile instead of one 16-byte store) sits on the chain between the MFMAs and the peers'
// polls and costs more than the halved poll count saves.  Default: XP only on the eight-wave clusters (units per CU 64);
// ASR_LSTM_XP=1 / 0 forces it on / off everywhere, ASR_LSTM_DFLAGS bit 11 inverts the choice at run time (tests, A/B).
bool bwd_xp_enabled(int hsu) {
  static const int env = [] { const char* e = getenv("ASR_LSTM_XP"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
  const bool def = env >= 0 ? env == 1 : hsu == 64;
  return def != ((dbg_flags() & 2048) != 0);
}

// fp32 operands (H = 128 / 256 / 320 / 512, see asr_cluster_fwd_f32_try) and the GRU clusters: ASR_LSTM_CLUSTER_F32=0 keeps
// the single-CU kernels (A/B).
bool cluster_f32_enabled() { static const bool on = env_on("ASR_LSTM_CLUSTER_F32"); return on && cluster_enabled(); }
// fp32 operands as three bf16 terms on the bf16 matrix pipe (H = 128 / 256, four waves per CU); ASR_LSTM_F32_SPLIT=0 or
// ASR_LSTM_DFLAGS bit 12 (run time, tests) keeps the exact-fp32 MFMA kernels
bool cluster_f32_split_enabled() { static const bool on = env_on("ASR_LSTM_F32_SPLIT"); return on && !(dbg_flags() & 4096); }
// fp32 operands: H = 128 / 256 / 320 / 512 on clusters of H/32 CUs x four waves (default), H = 128 also on two CUs x eight
// waves (ASR_LSTM_HS=64 / flag bit 9).  ASR_LSTM_CLUSTER_F32=0 keeps the single-CU kernels (A/B);
// ASR_LSTM_CLUSTER_F32_WIDE=0 keeps them for H > 128 only.
bool cluster_f32_wide_enabled() { static const bool on = env_on("ASR_LSTM_CLUSTER_F32_WIDE"); return on; }

// ---------------------------------------------------------------- debug: 16-byte exchange words, tear probe
// Would a lane's 16-byte store be seen whole by a 16-byte load of another CU?  The clusters' exchange uses 8-byte granules
// (one 64-bit store / load per lane: single-copy atomic by construction) or per-word tags; a 16-byte self-tagged word would
// halve the poll instructions but is only correct if the four dwords of one
// global_store_dwordx4 never appear torn.  Workgroup 0 writes {i, i, i, i} for i = 1 .. iters into one word per lane
// (plain stores when `wt` is 0, as a co-located cluster does, write-through sc1 stores otherwise); workgroup `peer`
// (8: same XCD as workgroup 0, 1: another XCD) polls the same words with L1-bypassing 16-byte loads and counts the loads
// whose four dwords differ.  out[3 lane .. + 2] = {loads, torn loads, distinct values seen}.
namespace {
__global__ __launch_bounds__(64) void tear_probe_kernel(unsigned* __restrict__ buf, unsigned iters, int peer, int wt,
                                                        unsigned long long* __restrict__ out) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
  const int lane = threadIdx.x;
  u32x4_t* word = reinterpret_cast<u32x4_t*>(buf) + lane;
  if (blockIdx.x == 0) {
    for (unsigned i = 1; i <= iters; ++i) {
      const u32x4_t v = {i, i, i, i};
      if (wt) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(word), "v"(v) : "memory");
      else asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(word), "v"(v) : "memory");
      if ((i & 63u) == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // bounded queue, stores in order
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return;
  }
  if ((int)blockIdx.x != peer) return;
  unsigned long long loads = 0, torn = 0, seen = 0;
  unsigned last = 0;
  for (unsigned long long spin = 0; spin < (1ull << 24); ++spin) {          // bounded: ~15 s even if nothing ever arrives
    u32x4_t v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(word) : "memory");
    ++loads;
    if (!(v[0] == v[1] && v[1] == v[2] && v[2] == v[3])) ++torn;
    if (v[0] != last) { ++seen; last = v[0]; }
    if (__all(v[0] >= iters && v[1] >= iters && v[2] >= iters && v[3] >= iters)) break;
  }
  out[3 * lane + 0] = loads;
  out[3 * lane + 1] = torn;
  out[3 * lane + 2] = seen;
}
}  // namespace
extern "C" int asr_debug_tear_probe(asr_handle* h, unsigned* buf, unsigned iters, int peer, int write_through,
                                    unsigned long long* out, asr_stream s) {
  if (!h || !buf || !out || iters < 1 || (peer != 1 && peer != 8) || ((uintptr_t)buf) % 16 != 0) return ASR_ERR_INVALID_ARG;
  if (hipMemsetAsync(buf, 0, 64 * 16, (hipStream_t)s) != hipSuccess) return ASR_ERR_HIP;
  hipLaunchKernelGGL(tear_probe_kernel, dim3(9), dim3(64), 0, (hipStream_t)s, buf, iters, peer, write_through, out);
  ASR_CHECK_LAUNCH(h, "asr_debug_tear_probe");
  return ASR_OK;
}

// Asynchronous read of the sticky error word: one 4-byte device->host copy on `st`, no synchronisation.
extern "C" int asr_peek_async_errors(asr_handle* h, unsigned* host_flags, asr_stream s) {
  hipStream_t st = (hipStream_t)s;
  if (!h || !host_flags) return ASR_ERR_INVALID_ARG;
  if (h->scratch_bytes < XCH_BYTES) { *host_flags = 0; return ASR_OK; }
  char* base = (char*)h->scratch + (h->scratch_bytes - XCH_BYTES);
  if (hipMemcpyAsync(host_flags, base, sizeof(unsigned), hipMemcpyDeviceToHost, st) != hipSuccess)
    ASR_FAIL(h, ASR_ERR_HIP, "asr_peek_async_errors: copy failed");
  return ASR_OK;
}
// Clears the sticky error word (after it has been reported) -- and, since a launch whose hand-off timed out leaves its
// exchange area in a state no later launch was written for (members that gave up at different steps, a header of a cluster
// that never completed its placement handshake), puts BOTH exchange areas and their bookkeeping back to what a fresh handle
// has: everything zero, nothing owed.  64 MiB of memset on the error path only.
extern "C" int asr_clear_async_errors(asr_handle* h, asr_stream s) {
  hipStream_t st = (hipStream_t)s;
  if (!h) return ASR_ERR_INVALID_ARG;
  if (h->scratch_bytes < XCH_BYTES) return ASR_OK;
  char* base = (char*)h->scratch + (h->scratch_bytes - XCH_BYTES);
  if (hipMemsetAsync(base, 0, XCH_BYTES, st) != hipSuccess) ASR_FAIL(h, ASR_ERR_HIP, "asr_clear_async_errors");
  h->xch_dirty[0] = h->xch_dirty[1] = 0;
  h->xch_next = 0;
  return ASR_OK;
}

// Synchronises the device and returns the sticky error word of the cluster kernels
// (bit 0: forward hand-off timed out, bit 1: backward); 0 = fine.
extern "C" int asr_check_async_errors(asr_handle* h, unsigned* flags_out) {
  if (!h) return ASR_ERR_INVALID_ARG;
  unsigned v = 0;
  char* base = (char*)h->scratch + (h->scratch_bytes - XCH_BYTES);
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(&v, base, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
    ASR_FAIL(h, ASR_ERR_HIP, "asr_check_async_errors: device error");
  if (flags_out) *flags_out = v;
  if (v & 3u) ASR_FAIL(h, ASR_ERR_HIP, "LSTM cluster hand-off timed out (flags 0x%x)", v);
  if (v) ASR_FAIL(h, ASR_ERR_HIP, "LSTM recurrence produced a non-finite hidden state (flags 0x%x)", v);
  return ASR_OK;
}
