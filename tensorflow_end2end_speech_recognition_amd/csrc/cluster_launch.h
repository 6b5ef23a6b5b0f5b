// Host side of the cluster recurrences: what the launchers of lstm_cluster.hip, lstm_cluster_f32.hip and gru_cluster.hip
// share.  Everything with state (the run-time flags, the CU budget, the cached environment switches) is defined once, in
// cluster_host.hip; this header declares it and holds the two small templates.
#pragma once
#include "cluster_xch.h"

#pragma GCC visibility push(hidden)   // calls between the units of the library, not part of its interface
static constexpr size_t XCH_BYTES = ASR_XCH_BYTES;
static constexpr size_t XCH_HALF = ((XCH_BYTES - 256) / 2) & ~(size_t)255;   // one of the two exchange areas

// ASR_LSTM_DFLAGS / asr_debug_set_lstm_flags (the bits: cluster_host.hip) and the part of them the kernels take
int dbg_flags();
int kernel_flags();
// environment switches, each read once (cluster_host.hip tells what they choose)
bool cluster_enabled();             // ASR_LSTM_CLUSTER
bool cluster_320_enabled();         // ASR_LSTM_CLUSTER_320
bool cluster_f32_enabled();         // ASR_LSTM_CLUSTER_F32 (and cluster_enabled)
bool cluster_f32_wide_enabled();    // ASR_LSTM_CLUSTER_F32_WIDE
bool cluster_f32_split_enabled();   // ASR_LSTM_F32_SPLIT, flag bit 12
bool fwd_xw_enabled();              // ASR_LSTM_XW, flag bit 10
bool bwd_xp_enabled(int hsu);       // ASR_LSTM_XP, flag bit 11
int units_per_cu(const char* specific, bool allow16 = false);
inline int fwd_units_per_cu() { return units_per_cu("ASR_LSTM_FWD_HS"); }
inline int fwd256_units_per_cu() { return units_per_cu("ASR_LSTM_FWD_HS", true); }
inline int bwd_units_per_cu() { return units_per_cu("ASR_LSTM_BWD_HS"); }

// The area this launch runs on (clean by construction; the memset is the fallback for a handle whose bookkeeping was
// reset) and the stretch of the other one it has to zero for its successor (zero_next_area).
struct XchAreas { u64* area; u64* znext; unsigned zwords; };
XchAreas xch_take(asr_handle* h, char* base, size_t need, hipStream_t st);

struct TilePlan { int per, n; };   // tiles per full group, number of groups (0: not even one tile fits)
// host counters of the path a recurrence call took (asr_recurrence_path_counts); kind 0 = LSTM, 1 = GRU
void count_cluster_launches(asr_handle* h, int kind, int groups);

// What every cluster launcher opens with.  elems = elements of the caller's largest [T, B, ndir, ...] array (the kernels
// index with 32 bits), G = CUs per cluster, cl_bytes = exchange bytes per cluster.  plan.n == 0: not applicable (too many
// elements, no exchange area in the scratch, or no plan: cluster_launch_plan in cluster_host.hip tells what `grouped`
// means); else base = the exchange area at the top of the scratch, the error word first.
struct ClusterCall { TilePlan plan; char* base; };
ClusterCall cluster_call(const asr_handle* h, int G, int ndir, int B, size_t elems, size_t cl_bytes, bool grouped);

// Runs launch(xa, ncl, t0, nt) once per tile group of the plan on `st`: an exchange area per launch (xch_take: each launch
// zeroes what its predecessor dirtied), ncl = clusters of the group, [t0, t0 + nt) its tiles.  kind as above.
template <typename F>
static void run_tile_groups(asr_handle* h, const ClusterCall& cc, int B, int ndir, size_t cl_bytes, hipStream_t st,
                            int kind, F launch) {
  for (int t0 = 0; t0 < B / 16; t0 += cc.plan.per) {
    const int nt = min(cc.plan.per, B / 16 - t0), ncl = nt * ndir;
    launch(xch_take(h, cc.base, ncl * cl_bytes, st), ncl, t0, nt);
  }
  count_cluster_launches(h, kind, cc.plan.n);
}
// attempt(grouped): first every form as ONE launch, in the order of preference; tile groups only when no form fits in one
template <typename F>
static bool one_launch_else_groups(F attempt) { return attempt(false) || attempt(true); }
#pragma GCC visibility pop
