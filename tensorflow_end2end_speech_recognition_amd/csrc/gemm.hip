// LDS-tiled MFMA GEMM for gfx950:  C[M,N] = op(A) * op(B) (+bias) (+C).
//   fp32 operands -> v_mfma_f32_16x16x4_f32   (exact fp32, the parity path)
//   bf16 operands -> v_mfma_f32_16x16x32_bf16 (fp32 accumulate)
// Used for every contraction that is not on the serial recurrence: the LSTM input
// projections x*W_x hoisted over all T (models/encoders/core/blstm.py:286-320), the
// bottleneck/output FC (models/ctc/ctc.py:198-233) and all dW / dX products of backward.
//
// Tile BM x BN x 128 bytes-of-K, 256 threads = 4 waves in a 2x2 grid, each wave owns a
// (BM/2)x(BN/2) block of 16x16 MFMA tiles.  Both operands are staged K-contiguous in
// LDS (As[m][k], Bs[n][k], row padded by 16 B so the 16 rows of a fragment read hit
// distinct banks); global loads are 16 B per lane along whichever dimension is
// contiguous in memory, register-staged so the next tile's loads fly during the MFMAs.
#include "common.h"
#include "mfma_tn.h"
#include <stdlib.h>

namespace {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE property of a kernel: "set once per process" leaves a
// second GPU of the same process without the LDS opt-in.  One bit per device ordinal.
static inline bool first_on_device(unsigned long long& mask) {
  int d = 0;
  (void)hipGetDevice(&d);
  const unsigned long long bit = 1ull << (d & 63);
  if (mask & bit) return false;
  mask |= bit;
  return true;
}

template <typename T> struct GT;
template <> struct GT<float> {
  static constexpr int BK = 32;   // 128 B of K per row
  static constexpr int VEC = 4;   // elements per 16 B
};
template <> struct GT<bf16_t> {
  static constexpr int BK = 64;
  static constexpr int VEC = 8;
};

template <typename T> struct Vec16 { T v[GT<T>::VEC]; } __attribute__((aligned(16)));

template <typename TO> __device__ __forceinline__ void store_out(TO* p, float v);
template <> __device__ __forceinline__ void store_out<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void store_out<bf16_t>(bf16_t* p, float v) { *p = f32_to_bf16(v); }
template <typename TO> __device__ __forceinline__ float load_out(const TO* p);
template <> __device__ __forceinline__ float load_out<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float load_out<bf16_t>(const bf16_t* p) { return bf16_to_f32(*p); }

// The k rows of a reduction-major product as frames of a time-major [T, Bp] batch (asr_gemm_tn_frames): row k is utterance
// k % Bp at frame frame0 + k / Bp, valid while that frame is below len[utterance].
struct TnFrames {
  const int32_t* len;           // [>= Bp] frames per utterance, device
  int Bp, frame0;
};
__device__ __forceinline__ bool tn_frame_valid(const TnFrames& fv, int k) {
  const int t = k / fv.Bp;
  return fv.frame0 + t < fv.len[k - t * fv.Bp];
}

// Stage one operand tile [ROWS x BK] (logical: row r, reduction index k) into registers.
// KCONT: memory is k-contiguous (elem(r,k) = p[r*ld + k]); else r-contiguous (p[k*ld + r]).
template <typename T, int ROWS, bool KCONT>
struct TileLoader {
  static constexpr int BK = GT<T>::BK, VEC = GT<T>::VEC;
  static constexpr int NVEC = ROWS * BK / VEC;
  static constexpr int PER_THREAD = NVEC / 256;
  static_assert(NVEC % 256 == 0, "tile must divide over 256 threads");
  Vec16<T> reg[PER_THREAD];

  // FR (reduction-major tiles only): a k row that is a padded frame of `fv` is not loaded, zeros take its place
  template <bool FR = false>
  __device__ __forceinline__ void load(const T* __restrict__ p, int ld, int r0, int k0, int R,
                                       int K, bool aligned, TnFrames fv = TnFrames{nullptr, 1, 0}) {
    static_assert(!FR || !KCONT, "frames: one k row per vector");
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      const int v = tid + i * 256;
      int r, k;
      size_t off;
      int nr, nk;  // extent of the vector in r and k
      if (KCONT) {
        r = v / (BK / VEC); k = (v % (BK / VEC)) * VEC;
        off = (size_t)(r0 + r) * ld + (k0 + k);
        nr = 1; nk = VEC;
      } else {
        k = v / (ROWS / VEC); r = (v % (ROWS / VEC)) * VEC;
        off = (size_t)(k0 + k) * ld + (r0 + r);
        nr = VEC; nk = 1;
      }
      if constexpr (FR) {
        if (k0 + k >= K || !tn_frame_valid(fv, k0 + k)) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) reg[i].v[j] = T(0);
          continue;
        }
      }
      const bool full = (r0 + r + nr <= R) && (k0 + k + nk <= K);
      if (full && aligned) {
        reg[i] = *reinterpret_cast<const Vec16<T>*>(p + off);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const int rr = r0 + r + (KCONT ? 0 : j), kk = k0 + k + (KCONT ? j : 0);
          T val = T(0);
          if (rr < R && kk < K) val = p[KCONT ? ((size_t)rr * ld + kk) : ((size_t)kk * ld + rr)];
          reg[i].v[j] = val;
        }
      }
    }
  }
  // LDS image: s[r][k], row stride LDS_LD elements
  __device__ __forceinline__ void store(T* s, int lds_ld) const {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      const int v = tid + i * 256;
      if (KCONT) {
        const int r = v / (BK / VEC), k = (v % (BK / VEC)) * VEC;
        *reinterpret_cast<Vec16<T>*>(s + r * lds_ld + k) = reg[i];
      } else {
        const int k = v / (ROWS / VEC), r = (v % (ROWS / VEC)) * VEC;
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[(r + j) * lds_ld + k] = reg[i].v[j];
      }
    }
  }
};

// FR (TA && !TB, asr_gemm_tn_frames): the k rows that are padded frames of `fv` are loaded from neither operand.
template <typename T, typename TO, int BM, int BN, bool TA, bool TB, bool FR = false>
__global__ __launch_bounds__(256) void gemm_kernel(int M, int N, int K, const T* __restrict__ A,
                                                   int lda, const T* __restrict__ B, int ldb,
                                                   TO* __restrict__ C, int ldc,
                                                   const float* __restrict__ bias, int accumulate,
                                                   int a_aligned, int b_aligned, int kchunk,
                                                   float* __restrict__ partial, int act, int c_vec,
                                                   TnFrames fv = TnFrames{nullptr, 1, 0}) {
  constexpr int BK = GT<T>::BK, VEC = GT<T>::VEC;
  constexpr int LDS_LD = BK + VEC;  // +16 B pad
  constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 16, TN = WN / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* As = reinterpret_cast<T*>(smem);
  T* Bs = As + BM * LDS_LD;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;

  // A tile: rows = m. memory k-contiguous iff !TA.  B tile: rows = n. k-contiguous iff TB.
  TileLoader<T, BM, !TA> la;
  TileLoader<T, BN, TB> lb;

  f32x4_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  // split-K: blockIdx.z owns the reduction range [kbeg, kend)
  const int kbeg = blockIdx.z * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int nkt = (kend - kbeg + BK - 1) / BK;
  // LDS is double-buffered: tile kt+1 is stored into the other buffer while nobody reads it, so
  // one barrier per k-tile orders everything (writers of buffer b at kt+1 have passed the
  // barrier of kt, which every reader of b reached only after finishing tile kt-1).
  constexpr int STAGE = (BM + BN) * LDS_LD;
  la.template load<FR>(A, lda, m0, kbeg, M, kend, a_aligned, fv);
  lb.template load<FR>(B, ldb, n0, kbeg, N, kend, b_aligned, fv);
  la.store(As, LDS_LD);
  lb.store(Bs, LDS_LD);
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    const T* Ac = As + (kt & 1) * STAGE;
    const T* Bc = Bs + (kt & 1) * STAGE;
    if (kt + 1 < nkt) {
      la.template load<FR>(A, lda, m0, kbeg + (kt + 1) * BK, M, kend, a_aligned, fv);
      lb.template load<FR>(B, ldb, n0, kbeg + (kt + 1) * BK, N, kend, b_aligned, fv);
    }
    const int fr = lane & 15, fq = lane >> 4;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int ks = 0; ks < BK / 32; ++ks) {
        bf16x8_t a[TM], b[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
          a[i] = *reinterpret_cast<const bf16x8_t*>(Ac + (wm * WM + i * 16 + fr) * LDS_LD + ks * 32 + fq * 8);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          b[j] = *reinterpret_cast<const bf16x8_t*>(Bc + (wn * WN + j * 16 + fr) * LDS_LD + ks * 32 + fq * 8);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < BK / 4; ++ks) {
        float a[TM], b[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i] = Ac[(wm * WM + i * 16 + fr) * LDS_LD + ks * 4 + fq];
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j] = Bc[(wn * WN + j * 16 + fr) * LDS_LD + ks * 4 + fq];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j], a[i], acc[i][j], 0, 0, 0);
      }
    }
    if (kt + 1 < nkt) {
      la.store(As + ((kt + 1) & 1) * STAGE, LDS_LD);
      lb.store(Bs + ((kt + 1) & 1) * STAGE, LDS_LD);
    }
    __syncthreads();
  }

  // epilogue.  The MFMAs above take (B fragment, A fragment), i.e. they produce the TRANSPOSED
  // tile: a lane holds C[m = lane&15][n = (lane>>4)*4 + 0..3] -- four consecutive columns of one
  // row -> one 16-byte (fp32) / 8-byte (bf16) store per tile instead of four scalar ones (the
  // scalar-store epilogue was store-issue bound and as long as the K loop at K = 512).
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int m = m0 + wm * WM + i * 16 + (lane & 15);
      const int nb = n0 + wn * WN + j * 16 + (lane >> 4) * 4;
      if (m >= M || nb >= N) continue;
      const bool full = nb + 3 < N;
      if (partial) {  // split-K partial slab [z][M][N]; bias / accumulate applied by the reducer
        float* pp = partial + ((size_t)blockIdx.z * M + m) * N + nb;
        if (full && (N & 3) == 0) *reinterpret_cast<f32x4_t*>(pp) = acc[i][j];
        else
          for (int r = 0; r < 4 && nb + r < N; ++r) pp[r] = acc[i][j][r];
        continue;
      }
      TO* cp = C + (size_t)m * ldc + nb;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] + ((bias && nb + r < N) ? bias[nb + r] : 0.f);
      if (full && c_vec) {
        if constexpr (sizeof(TO) == 4) {
          if (accumulate) {
            const f32x4_t o = *reinterpret_cast<const f32x4_t*>(cp);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += o[r];
          }
          if (act == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
          }
          *reinterpret_cast<f32x4_t*>(cp) = (f32x4_t){v[0], v[1], v[2], v[3]};
        } else {
          typedef __attribute__((ext_vector_type(4))) unsigned short us4_t;
          if (accumulate) {
            const us4_t o = *reinterpret_cast<const us4_t*>(cp);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += bf16_to_f32(o[r]);
          }
          if (act == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
          }
          *reinterpret_cast<us4_t*>(cp) = (us4_t){f32_to_bf16(v[0]), f32_to_bf16(v[1]), f32_to_bf16(v[2]), f32_to_bf16(v[3])};
        }
      } else {
        for (int r = 0; r < 4 && nb + r < N; ++r) {
          float w = v[r];
          if (accumulate) w += load_out<TO>(cp + r);
          if (act == 1) w = fmaxf(w, 0.f);
          store_out<TO>(cp + r, w);
        }
      }
    }
}

// LDS images [rows][64 + 8 bf16] read as MFMA fragments with ds_read_b128 (16 lanes = 16 rows of one 16-byte k-slot): the
// hardware serves a wave in lane groups that pair rows 0-3, 12-15 of k-slot q with rows 4-11 of k-slot q ^ 1
// (cluster_xch.h, lds_swz), so with plain padding those two sets collide on the 16 sixteen-byte bank groups --
// SQ_LDS_BANK_CONFLICT on 11-13 % of the CU cycles of these kernels (profiles/r03_pmc_util.md).  Swapping the two halves of
// every 32 bytes OF A ROW for rows 4-11 (mod 16), by writers and readers alike, makes every group hit 16 distinct slots
// (row stride 9 slots: 9 r + q mod 16 is a permutation of the 16 rows).
__device__ __forceinline__ unsigned nt_swz(int row) { return (((row + 4) >> 3) & 1) ? 8u : 0u; }   // in bf16 elements

// The tile a block of the NT kernels works on: block b runs on XCD b % 8, and XCD x gets a contiguous run of tiles, so that
// the N-tiles sharing an A row-panel fetch it into ONE L2.  The full products apply this when the tile count is a multiple
// of 8 (and take tile b otherwise).  ANY: for every count -- XCD x runs blocks x, x + 8, ..., total / 8 of them and one more
// on the first total % 8 XCDs, and gets that many consecutive tiles (the same tiles as the other rule where that one
// applies); the listed-row products use it, whose counts are rarely multiples of 8 (dx of the headline step: 204 tiles,
// 46.3 -> 42.8 us).
template <bool ANY> __device__ __forceinline__ int nt_tile_of_block(int b, int total) {
  if constexpr (ANY) {
    const int per = total >> 3, rem = total & 7, x = b & 7;
    return x * per + min(x, rem) + (b >> 3);
  } else {
    int t = b;
    if ((total & 7) == 0) t = (t & 7) * (total >> 3) + (t >> 3);
    return t;
  }
}

struct GemmDrop {               // dropout multiplier of the OUTPUT formed in the epilogue (element m*N + n of a contiguous
  float keep;                   // [M,N] tensor -> word (m*N + n) % 4 of Philox block offset + (m*N + n) / 4): asr_dropout_mask's
  uint64_t seed, offset;        // values without the mask tensor
  int use;
};

// ---------------------------------------------------------------- lean NT kernel (bf16)
// C[M,N] = A[M,K] * Bt[N,K]^T (+bias)(+C)(relu): both operands reduction-contiguous, K % 64 == 0,
// N % 128 == 0, 16-byte aligned rows.  This is the shape of every GEMM on the critical path of
// the BLSTM step (x W_x with W_x pre-transposed, dG W_x^T).  No bounds code in the loop: rows of
// the last M tile are clamped for the loads and masked at the store.  128x128x64 tiles, register
// staged global->LDS with the next tile's loads in flight during the MFMAs, double-buffered LDS
// (one barrier per k-tile), transposed accumulators (16-byte stores).  Tiles are mapped to blocks
// so that the N-tiles sharing an A row-panel run on ONE XCD (block b lands on XCD b % 8): the
// panel is then fetched into one L2 instead of eight.
// ROWS (the listed-row form, asr_gemm_rows): M counts the entries of `rows` (ascending row numbers of A / C / mul);
// product row i reads A[rows[i]] and is stored to C[rows[i]], the multiplier and the dropout counter are those of row
// rows[i] of the full tensor.  Same k-loop and accumulation order: a listed row gets the bits the full product gives it.
// (Measured and not kept: the listed-row form with the global loads of TWO k-tiles in flight -- two register sets, the
// loop unrolled by two, 144 + 64 registers, s_waitcnt vmcnt(15..8) in the loop.  dx of the headline step 42.8 -> 42.8 us,
// projection 32.4 -> 33.1 us, step within the run-to-run spread: the k-loop is not what these launches wait for.
// profiles/r08_valid_rows_ab.md.)
template <typename TO, bool ROWS = false>
__global__ __launch_bounds__(256) void gemm_nt_bf16_kernel(int M, int N, int K, const bf16_t* __restrict__ A,
                                                           int lda, const bf16_t* __restrict__ Bt, int ldb,
                                                           TO* __restrict__ C, int ldc,
                                                           const float* __restrict__ bias, int accumulate,
                                                           int act, const float* __restrict__ mul, int ldm,
                                                           GemmDrop drop, const int32_t* __restrict__ rows) {
  constexpr int BM = 128, BN = 128, BK = 64, LD = BK + 8;
  constexpr int STAGE = (BM + BN) * LD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* S = reinterpret_cast<bf16_t*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = N / BN, ntm = (M + BM - 1) / BM, total = ntn * ntm;
  const int t = nt_tile_of_block<ROWS>((int)blockIdx.x, total);
  const int m0 = (t / ntn) * BM, n0 = (t % ntn) * BN;

  // 4 A vectors + 4 B vectors of 16 B per thread per k-tile: vector v -> row v>>3, k-offset (v&7)*8
  const bf16_t* pa[4];
  const bf16_t* pb[4];
  unsigned so[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = tid + i * 256, r = v >> 3, kv = (v & 7) * 8;
    const int ar = min(m0 + r, M - 1);
    pa[i] = A + (size_t)(ROWS ? rows[ar] : ar) * lda + kv;
    pb[i] = Bt + (size_t)(n0 + r) * ldb + kv;
    so[i] = (unsigned)(r * LD) + ((unsigned)kv ^ nt_swz(r));
  }
  bf16x8_t ra[4], rb[4];
  auto gload = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const bf16x8_t*>(pa[i]);
      rb[i] = *reinterpret_cast<const bf16x8_t*>(pb[i]);
      pa[i] += BK;
      pb[i] += BK;
    }
  };
  auto sstore = [&](bf16_t* st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<bf16x8_t*>(st + so[i]) = ra[i];
      *reinterpret_cast<bf16x8_t*>(st + BM * LD + so[i]) = rb[i];
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int nkt = K / BK;
  gload();
  sstore(S);
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  const unsigned aoff = (unsigned)((wm * 64 + fr) * LD) + ((unsigned)(fq * 8) ^ nt_swz(fr));
  const unsigned boff = (unsigned)(BM * LD + (wn * 64 + fr) * LD) + ((unsigned)(fq * 8) ^ nt_swz(fr));
  for (int kt = 0; kt < nkt; ++kt) {
    const bf16_t* cur = S + (kt & 1) * STAGE;
    if (kt + 1 < nkt) gload();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(cur + aoff + i * 16 * LD + ks * 32);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(cur + boff + j * 16 * LD + ks * 32);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nkt) sstore(S + ((kt + 1) & 1) * STAGE);
    __syncthreads();
  }
  // lane holds C[m = fr][n = fq*4 .. +3] of each 16x16 tile
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int mi = m0 + wm * 64 + i * 16 + fr;
    if (mi >= M) continue;
    const int m = ROWS ? rows[mi] : mi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nb = n0 + wn * 64 + j * 16 + fq * 4;
      TO* cp = C + (size_t)m * ldc + nb;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r];
      if (bias) {
        const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(bias + nb);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bv[r];
      }
      if constexpr (sizeof(TO) == 4) {
        if (accumulate) {
          const f32x4_t o = *reinterpret_cast<const f32x4_t*>(cp);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += o[r];
        }
        if (act == 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if (mul) {                                         // e.g. the dropout mask of the tensor this gradient is of
          const f32x4_t mv = *reinterpret_cast<const f32x4_t*>(mul + (size_t)m * ldm + nb);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] *= mv[r];
        }
        if (drop.use) {                                    // the same mask from its Philox counter (N % 4 == 0)
          float mk[4];
          asr_dropout_words(drop.offset + ((size_t)m * N + nb) / 4, drop.seed, drop.keep, 1.f / drop.keep, mk);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] *= mk[r];
        }
        *reinterpret_cast<f32x4_t*>(cp) = (f32x4_t){v[0], v[1], v[2], v[3]};
      } else {
        typedef __attribute__((ext_vector_type(4))) unsigned short us4_t;
        if (accumulate) {
          const us4_t o = *reinterpret_cast<const us4_t*>(cp);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bf16_to_f32(o[r]);
        }
        if (act == 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        *reinterpret_cast<us4_t*>(cp) = (us4_t){f32_to_bf16(v[0]), f32_to_bf16(v[1]), f32_to_bf16(v[2]), f32_to_bf16(v[3])};
      }
    }
  }
}

// ---------------------------------------------------------------- NT kernel, large tiles (bf16)
// The 128 x 128 kernel above is bound by LDS traffic, not by the matrix pipes: a wave's 64 x 64 tile reads 8 KB of
// fragments per 16 MFMAs, eight waves per CU -> 128 KB read + 64 KB written per k-tile round = 1 536 LDS clocks against
// 1 024 MFMA clocks per SIMD (measured 0.62-0.64 PFLOP/s on the [105 600 x 1 024] x [1 024 x 4 096] projection of cfg C).
// This one gives a wave a (BM / WM) x (BN / WN) tile of a BM x BN block: 128 x 64 wave tiles read 12 KB per 32 MFMAs,
// 128 x 128 ones 16 KB per 64.  Measured on one MI355X (scripts/probe_matmul.py, fp32 output, TFLOP/s on the
// [12 448 x 512] x [512 x 2 048] / [51 136 x 1 024] x [1 024 x 4 096] / [105 600 x 1 024] x [1 024 x 4 096] projections):
//   128 x 128 block, four waves of 64 x 64, two blocks per CU (the kernel above)      509 / 578 / 643
//   256 x 256 block, EIGHT waves of 128 x 64 (two per SIMD, 244 VGPRs)                496 / 721 / 842   <- used from 512 tiles on
//   256 x 128 block, four waves of 128 x 64 (one per SIMD: nothing hides a stall)     321 / 491 / 512
//   256 x 256 block, four waves of 128 x 128: the 256 accumulators ARE the AGPR file; the allocator keeps half of them
//   in VGPRs and copies (433 v_accvgpr moves per k-tile, 94 spilled registers)        169 / 200 / 205
// (torch.matmul -> hipBLASLt with a bf16 result reaches 420 / 1 029 / 1 237 on the same operands.)  Same staging scheme (next k-tile's global loads in flight during the MFMAs, one barrier
// per k-tile), same transposed accumulators and epilogue; the staging loads are buffer loads (descriptor in SGPRs, a
// per-lane 32-bit byte offset that never changes, the k-tile's offset in one SGPR).
// (Round 5, measured: a PERSISTENT form -- 256 / 512 workgroups walking the tiles, the next tile's first k-tile requested
// before the epilogue's stores -- is 2 % SLOWER on every cfg C / D projection (1178 -> 1206 us, 493 -> 516 us): the
// dispatcher already replaces a finished workgroup faster than the epilogue drains.  scripts/bench_nt.py.)
// ROWS: the listed-row form, as in gemm_nt_bf16_kernel (the A descriptor then reaches to the last listed row).
template <typename TO, int BM, int BN, int WM, int WN, bool ROWS = false>
__global__ __launch_bounds__(WM * WN * 64, 1) void gemm_nt_bf16_big_kernel(int M, int N, int K, const bf16_t* __restrict__ A,
                                                                           int lda, const bf16_t* __restrict__ Bt, int ldb,
                                                                           TO* __restrict__ C, int ldc,
                                                                           const float* __restrict__ bias, int accumulate,
                                                                           int act, const float* __restrict__ mul, int ldm,
                                                                           GemmDrop drop, const int32_t* __restrict__ rows) {
  constexpr int BK = 64, LD = BK + 8, NT = WM * WN * 64;
  constexpr int STAGE = (BM + BN) * LD;
  constexpr int TM = BM / WM, TN = BN / WN, TI = TM / 16, TJ = TN / 16;
  constexpr int VA = BM * 8 / NT, VB = BN * 8 / NT, RSTEP = NT / 8;   // staging vectors per thread, rows between them
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* S = reinterpret_cast<bf16_t*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int ntn = N / BN, ntm = (M + BM - 1) / BM, total = ntn * ntm;
  const int t = nt_tile_of_block<ROWS>((int)blockIdx.x, total);
  const int m0 = (t / ntn) * BM, n0 = (t % ntn) * BN;

  // staging vector i of a thread: row (tid >> 3) + RSTEP i, k-offset (tid & 7) * 8; rows of A past M (last tile) are
  // clamped to row M - 1 and masked at the store
  const int r0 = tid >> 3, kv = (tid & 7) * 8;
  unsigned oa[VA], ob[VB];
#pragma unroll
  for (int i = 0; i < VA; ++i) {
    const int ar = min(m0 + r0 + RSTEP * i, M - 1);
    oa[i] = (unsigned)(((size_t)(ROWS ? rows[ar] : ar) * lda + kv) * sizeof(bf16_t));
  }
#pragma unroll
  for (int i = 0; i < VB; ++i) ob[i] = (unsigned)(((size_t)(n0 + r0 + RSTEP * i) * ldb + kv) * sizeof(bf16_t));
  const unsigned so0 = (unsigned)(r0 * LD) + ((unsigned)kv ^ nt_swz(r0));   // (a thread's rows are RSTEP = 32 k apart: same class)
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16_t*>(A), 0,
      (int)min((size_t)0xFFFFFFFFu, ((size_t)(ROWS ? rows[M - 1] : M - 1) * lda + K) * sizeof(bf16_t)), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16_t*>(Bt), 0, (int)min((size_t)0xFFFFFFFFu, ((size_t)(N - 1) * ldb + K) * sizeof(bf16_t)), 0x00020000);
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
  u32x4_t ra[VA], rb[VB];
  unsigned koff = 0;                                       // byte offset of the k-tile being fetched (uniform)
  auto gload = [&]() {
#pragma unroll
    for (int i = 0; i < VA; ++i) ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rsA, oa[i], koff, 0);
#pragma unroll
    for (int i = 0; i < VB; ++i) rb[i] = __builtin_amdgcn_raw_buffer_load_b128(rsB, ob[i], koff, 0);
    koff += BK * sizeof(bf16_t);
  };
  auto sstore = [&](bf16_t* st) {
#pragma unroll
    for (int i = 0; i < VA; ++i) *reinterpret_cast<u32x4_t*>(st + so0 + i * RSTEP * LD) = ra[i];
#pragma unroll
    for (int i = 0; i < VB; ++i) *reinterpret_cast<u32x4_t*>(st + BM * LD + so0 + i * RSTEP * LD) = rb[i];
  };

  f32x4_t acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int nkt = K / BK;
  gload();
  sstore(S);
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  const unsigned aoff = (unsigned)((wm * TM + fr) * LD) + ((unsigned)(fq * 8) ^ nt_swz(fr));
  const unsigned boff = (unsigned)(BM * LD + (wn * TN + fr) * LD) + ((unsigned)(fq * 8) ^ nt_swz(fr));
  for (int kt = 0; kt < nkt; ++kt) {
    const bf16_t* cur = S + (kt & 1) * STAGE;
    if (kt + 1 < nkt) gload();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t a[TI];
#pragma unroll
      for (int i = 0; i < TI; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(cur + aoff + i * 16 * LD + ks * 32);
#pragma unroll
      for (int jh = 0; jh < TJ; jh += 4) {                  // B fragments in runs of four (registers)
        bf16x8_t b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(cur + boff + (jh + j) * 16 * LD + ks * 32);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][jh + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][jh + j], 0, 0, 0);
      }
    }
    if (kt + 1 < nkt) sstore(S + ((kt + 1) & 1) * STAGE);
    __syncthreads();
  }
  // lane holds C[m = fr][n = fq*4 .. +3] of each 16x16 tile
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int mi = m0 + wm * TM + i * 16 + fr;
    if (mi >= M) continue;
    const int m = ROWS ? rows[mi] : mi;
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int nb = n0 + wn * TN + j * 16 + fq * 4;
      TO* cp = C + (size_t)m * ldc + nb;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r];
      if (bias) {
        const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(bias + nb);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bv[r];
      }
      if constexpr (sizeof(TO) == 4) {
        if (accumulate) {
          const f32x4_t o = *reinterpret_cast<const f32x4_t*>(cp);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += o[r];
        }
        if (act == 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if (mul) {
          const f32x4_t mv = *reinterpret_cast<const f32x4_t*>(mul + (size_t)m * ldm + nb);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] *= mv[r];
        }
        if (drop.use) {
          float mk[4];
          asr_dropout_words(drop.offset + ((size_t)m * N + nb) / 4, drop.seed, drop.keep, 1.f / drop.keep, mk);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] *= mk[r];
        }
        *reinterpret_cast<f32x4_t*>(cp) = (f32x4_t){v[0], v[1], v[2], v[3]};
      } else {
        typedef __attribute__((ext_vector_type(4))) unsigned short us4_t;
        if (accumulate) {
          const us4_t o = *reinterpret_cast<const us4_t*>(cp);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bf16_to_f32(o[r]);
        }
        if (act == 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        *reinterpret_cast<us4_t*>(cp) = (us4_t){f32_to_bf16(v[0]), f32_to_bf16(v[1]), f32_to_bf16(v[2]), f32_to_bf16(v[3])};
      }
    }
  }
}

template <typename TO, int BM, int BN, int WM, int WN, bool ROWS = false>
static void launch_gemm_nt_big(int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                               const float* bias, int accumulate, hipStream_t st, int act, const float* mul, int ldm,
                               GemmDrop drop, const int32_t* rows = nullptr) {
  const size_t lds = (size_t)2 * (BM + BN) * (64 + 8) * sizeof(bf16_t);
  static unsigned long long attr_done = 0;
  auto k = gemm_nt_bf16_big_kernel<TO, BM, BN, WM, WN, ROWS>;
  if (first_on_device(attr_done)) {
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  const long tiles = (long)(N / BN) * ((M + BM - 1) / BM);
  hipLaunchKernelGGL(k, dim3((unsigned)tiles), dim3(WM * WN * 64), lds, st, M, N, K, (const bf16_t*)A, lda,
                     (const bf16_t*)B, ldb, (TO*)C, ldc, bias, accumulate, act, mul, ldm, drop, rows);
}

// the listed-row launch of the 128 x 128 kernel (its own function: its own opt-in for the dynamic LDS)
static void launch_gemm_nt_rows128(int nrows, int N, int K, const void* A, int lda, const void* B, int ldb, float* C,
                                   int ldc, const float* bias, int accumulate, hipStream_t st, int act,
                                   const float* mul, int ldm, GemmDrop drop, const int32_t* rows) {
  const size_t lds = (size_t)2 * (128 + 128) * (64 + 8) * sizeof(bf16_t);
  static unsigned long long attr_done = 0;
  auto k = gemm_nt_bf16_kernel<float, true>;
  if (first_on_device(attr_done)) {
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  const int total = (N / 128) * ((nrows + 127) / 128);
  hipLaunchKernelGGL(k, dim3(total), dim3(256), lds, st, nrows, N, K, (const bf16_t*)A, lda, (const bf16_t*)B, ldb, C,
                     ldc, bias, accumulate, act, mul, ldm, drop, rows);
}

// rows / nrows (asr_gemm_rows, fp32 output): the product of the `nrows` (>= 1) listed rows only.  Whether the lean path
// applies is judged on the full M, as for the full product; which of the two kernels runs, on the listed count.
// counts: the handle's gemm_counts (listed-row launches by kernel).  used_big: set to whether the 256 x 256 kernel ran.
template <typename TO>
bool try_gemm_nt_bf16(int transA, int transB, int M, int N, int K, const void* A, int lda, const void* B,
                      int ldb, void* C, int ldc, const float* bias, int accumulate, hipStream_t st, int act,
                      const float* mul, int ldm, GemmDrop drop = GemmDrop{1.f, 0, 0, 0}, const int32_t* rows = nullptr,
                      int nrows = 0, unsigned long long* counts = nullptr, bool* used_big = nullptr) {
  if (transA || !transB || K % 64 != 0 || N % 128 != 0 || M < 1024) return false;
  if (drop.use && sizeof(TO) != 4) return false;
  if (mul && (sizeof(TO) != 4 || ldm % 4 != 0 || ((uintptr_t)mul) % 16 != 0)) return false;
  if (lda % 8 != 0 || ldb % 8 != 0 || ((uintptr_t)A) % 16 != 0 || ((uintptr_t)B) % 16 != 0) return false;
  if (ldc % 4 != 0 || ((uintptr_t)C) % (4 * sizeof(TO)) != 0 || (bias && ((uintptr_t)bias) % 16 != 0)) return false;
  if (rows && (sizeof(TO) != 4 || nrows < 1 || nrows > M)) return false;
  // large products (>= 512 tiles of 256 x 256, i.e. two full rounds of the chip): 256 x 256 blocks of eight waves, see
  // gemm_nt_bf16_big_kernel; ASR_GEMM_NT_BIG=0 keeps the 128 x 128 tiles (A/B), =2 takes the big ones from M >= 2048 on
  static const int big = [] { const char* e = getenv("ASR_GEMM_NT_BIG"); return e ? atoi(e) : 1; }();
  const bool fits32 = ((size_t)(M - 1) * lda + K) * sizeof(bf16_t) < 0xFFFFFFFFull && ((size_t)(N - 1) * ldb + K) * sizeof(bf16_t) < 0xFFFFFFFFull;
  const int Mk = rows ? nrows : M;                          // rows the launch computes
  const long tiles256 = (long)(N / 256) * ((Mk + 255) / 256);
  const bool use_big = big && fits32 && N % 256 == 0 && (big == 2 ? Mk >= 2048 : tiles256 >= 512);
  if (used_big) *used_big = use_big;
  if constexpr (sizeof(TO) == 4) {
    if (rows) {
      if (use_big)
        launch_gemm_nt_big<float, 256, 256, 2, 4, true>(Mk, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act, mul,
                                                         ldm, drop, rows);
      else
        launch_gemm_nt_rows128(Mk, N, K, A, lda, B, ldb, (float*)C, ldc, bias, accumulate, st, act, mul, ldm, drop, rows);
      if (counts) counts[use_big ? ASR_GEMMP_ROWS_256 : ASR_GEMMP_ROWS_128] += 1;
      return true;
    }
  }
  if (use_big) {
    launch_gemm_nt_big<TO, 256, 256, 2, 4>(M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act, mul, ldm, drop);
    return true;
  }
  const size_t lds = (size_t)2 * (128 + 128) * (64 + 8) * sizeof(bf16_t);
  static unsigned long long attr_done = 0;
  if (first_on_device(attr_done)) {
    (void)hipFuncSetAttribute((const void*)gemm_nt_bf16_kernel<TO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  const int total = (N / 128) * ((M + 127) / 128);
  hipLaunchKernelGGL(gemm_nt_bf16_kernel<TO>, dim3(total), dim3(256), lds, st, M, N, K, (const bf16_t*)A, lda,
                     (const bf16_t*)B, ldb, (TO*)C, ldc, bias, accumulate, act, mul, ldm, drop, (const int32_t*)nullptr);
  return true;
}

// Workgroup b of a 1-D grid runs on XCD b % 8 (asr_debug_placement).  Side-stream kernels leave the first `skip` XCDs
// -- where the recurrence clusters live -- alone: their workgroups there retire at once and the work is dealt over
// the others.  Returns the dense work index of this workgroup, -1 for a workgroup that has nothing to do.
__device__ __forceinline__ int xcd_work_index(int skip) {
  const int b = blockIdx.x, x = b & 7;
  if (x < skip) return -1;
  return (b >> 3) * (8 - skip) + (x - skip);
}
static inline unsigned xcd_grid(long work, int skip) {     // workgroups to launch for `work` work items
  const long per = 8 - skip;
  return (unsigned)((work + per - 1) / per * 8);
}

// ---------------------------------------------------------------- skinny fp32 kernel (M <= 32)
// C[M,N] = A[M,K] op(B) (+bias)(+C)(relu), fp32, M <= 32: the per-step products of the attention decoder (cell input
// 1600 -> 2048 and back, query 512 <-> 128 at B = 32 utterances, attention_decoder.py:142-229).  They are weight
// streaming -- 13 MB of W_cell per step against 0.2 GFLOP -- and sit on the decoder's serial chain, so what counts is
// how many CUs pull on the weights and how many bytes each has in flight.  One workgroup owns 16*NT output columns of
// ONE 16-row group (grid.y = row groups: the fp32 MFMA rate of the 64..100 column tiles alone is ~7 us per product,
// so the rows are spread over twice the CUs and B comes out of L2 for the second group); its eight waves split K in
// 64-element units (interleaved), and a wave issues the loads of its NEXT unit (4 float4 of A, NT x 4 float4 -- or
// NT x 16 row-segment words -- of B) before the MFMAs of the current one.  TRANSB reads a float4 of a B^T row per
// lane, the plain form reads full 128-byte lines (NT = 2).  The products are exact fp32 MFMAs (16x16x4) and the eight
// partial tiles meet in LDS in a fixed order (deterministic).
// Requires K % 64 == 0, N % (16 NT) == 0, 16-byte aligned rows.
constexpr int SK_WAVES = 8;
// CELL: the product is the decoder cell's pre-activation with the gate columns INTERLEAVED (column 4 u + g = gate g of unit
// u, asr_lstm_cell_gemm_prep) so that a workgroup's 32 columns are all four gates of 8 units, and the LSTM cell
// (cell_fwd_kernel of attention.hip, same arithmetic in the same order) runs in the epilogue on the reduced tile: one launch
// and one dependent round trip fewer per decoder step, the pre-activations never written.  The cell's own inputs are
// requested before the product's first load.
struct SkinnyCell {
  const float *c_prev, *h_prev, *peep, *live, *out_mask;
  float *gates, *c_raw, *c_out, *h_out, *h_raw, *cell_out, *h_out2, *cell_out2;
  int U, ld_h2, ld_c2;
  float fb, clip;
};
__device__ __forceinline__ float sk_sigf(float x) { return 1.0f / (1.0f + expf(-x)); }
// BH: the weights are bf16 (the activations stay fp32, the products are exact fp32 MFMAs of an fp32 value and a
// bf16-valued one): half the bytes of a launch that is weight streaming.  !TRANSB: Bm is the FRAGMENT image of
// asr_lstm_cell_gemm_prep_h -- per (32-column block, 64-row unit) the 64 lanes' 32 values each, contiguous, in the order
// the multiplies consume them: four 16-byte loads per lane and unit instead of 32 strided dword loads.  TRANSB: Bm is a
// bf16 [N, ldb] matrix of B^T rows; a lane takes 16 consecutive k of its row (two 16-byte loads) and the matching 16
// consecutive k of its A row -- MFMA slot rg carries k = kb + 16 rg + t at multiply t (any k-to-slot map is a valid dot
// product as long as both operands use it).
template <bool TRANSB, int NT, bool CELL = false, bool BH = false>
__global__ __launch_bounds__(64 * SK_WAVES) void gemm_skinny_f32_kernel(int M, int N, int K, const float* __restrict__ A,
                                                                        int lda, const float* __restrict__ Bm, int ldb,
                                                                        float* __restrict__ C, int ldc,
                                                                        const float* __restrict__ bias, int accumulate,
                                                                        int act, SkinnyCell cell) {
  constexpr int TN = 16 * NT;
  __shared__ float red[SK_WAVES][16][TN + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, rg = lane >> 4;
  const int n0 = blockIdx.x * TN, m0 = blockIdx.y * 16;
  // CELL: thread idx < 16 * TN / 4 owns (row m0 + idx / (TN/4), unit n0/4 + idx % (TN/4))
  float cl_cp = 0.f, cl_hp = 0.f, cl_lv = 0.f, cl_wci = 0.f, cl_wcf = 0.f, cl_wco = 0.f, cl_om = 1.f;
  const int cl_m = m0 + (int)threadIdx.x / (TN / 4), cl_u = n0 / 4 + (int)threadIdx.x % (TN / 4);
  const bool cl_on = CELL && (int)threadIdx.x < 16 * (TN / 4) && cl_m < M;
  if (CELL && cl_on) {
    const size_t ci = (size_t)cl_m * cell.U + cl_u;
    cl_cp = cell.c_prev[ci];
    cl_hp = cell.h_prev[ci];
    cl_lv = cell.live[cl_m];
    if (cell.peep) { cl_wci = cell.peep[cl_u]; cl_wcf = cell.peep[cell.U + cl_u]; cl_wco = cell.peep[2 * cell.U + cl_u]; }
    if (cell.out_mask) cl_om = cell.out_mask[ci];
  }
  typedef __attribute__((ext_vector_type(4))) unsigned skw4_t;
  static_assert(!BH || (TRANSB ? NT == 1 : NT == 2), "bf16 weights: NT = 2 fragment image / NT = 1 transposed rows");
  struct Frag {
    f32x4_t a[4], b[BH ? 1 : NT][BH ? 1 : 4];
    skw4_t w[BH ? (TRANSB ? 2 : 4) : 1];
    float keep;                 // 1 for a real unit, 0 for a round past the end (A is zeroed at the multiply)
  };
  f32x4_t acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  // rows past M read a valid row, masked at the store
  const float* ap = A + (size_t)min(m0 + col, M - 1) * lda + ((BH && TRANSB) ? rg * 16 : rg * 4);
  const int units = K / 64;
  const bf16_t* Bh = reinterpret_cast<const bf16_t*>(Bm);
  // round r of a wave is the 64-element unit wave + 8r; rounds past the end re-read the last unit with A zeroed, so
  // every wave runs the same (even) number of rounds and every prefetch below is consumed -- a prefetch whose use sits
  // behind a branch gets sunk below the multiplies by the compiler, which serialises load and multiply again
  auto load = [&](int round, Frag& f) {
    const int unit = wave + round * SK_WAVES;
    const bool valid = unit < units;
    const int kb = (valid ? unit : units - 1) * 64;
    f.keep = valid ? 1.f : 0.f;
    if constexpr (BH) {
      if constexpr (TRANSB) {
#pragma unroll
        for (int j = 0; j < 4; ++j) f.a[j] = *reinterpret_cast<const f32x4_t*>(ap + kb + j * 4);   // A[row][kb + 16rg + 4j + e]
        const bf16_t* bp = Bh + (size_t)(n0 + col) * ldb + kb + rg * 16;                           // Bt[n][kb + 16rg + 0..15]
        f.w[0] = *reinterpret_cast<const skw4_t*>(bp);
        f.w[1] = *reinterpret_cast<const skw4_t*>(bp + 8);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) f.a[j] = *reinterpret_cast<const f32x4_t*>(ap + kb + j * 16);
        const skw4_t* bp = reinterpret_cast<const skw4_t*>(Bh + (((size_t)blockIdx.x * units + (kb >> 6)) * 64 + lane) * 32);
#pragma unroll
        for (int j = 0; j < 4; ++j) f.w[j] = bp[j];       // word e of w[j]: {column n0 + col, column n0 + 16 + col} at k = kb + 16j + 4rg + e
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f.a[j] = *reinterpret_cast<const f32x4_t*>(ap + kb + j * 16);     // A[row][kb + 16j + 4rg + e]
#pragma unroll
      for (int n = 0; n < NT; ++n) {                                    // B[kb + 16j + 4rg + e][n0 + 16n + col]
        if (TRANSB) {
          f.b[n][j] = *reinterpret_cast<const f32x4_t*>(Bm + (size_t)(n0 + n * 16 + col) * ldb + kb + j * 16 + rg * 4);
        } else {
          const float* bp = Bm + (size_t)(kb + j * 16 + rg * 4) * ldb + n0 + n * 16 + col;
#pragma unroll
          for (int e = 0; e < 4; ++e) f.b[n][j][e] = bp[(size_t)e * ldb];
        }
      }
    }
  };
  auto mma = [&](const Frag& f) {
    if constexpr (BH) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if constexpr (TRANSB) {                           // multiply t = 4j + e: k = kb + 16rg + t
            const int t = 4 * j + e;
            const unsigned wd = f.w[t >> 3][(t & 7) >> 1];
            const float bv = __uint_as_float((t & 1) ? (wd & 0xffff0000u) : (wd << 16));
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[j][e] * f.keep, bv, acc[0], 0, 0, 0);
          } else {
            const unsigned wd = f.w[j][e];
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[j][e] * f.keep, __uint_as_float(wd << 16), acc[0], 0, 0, 0);
            acc[NT - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[j][e] * f.keep, __uint_as_float(wd & 0xffff0000u), acc[NT - 1], 0, 0, 0);
          }
        }
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[j][e] * f.keep, f.b[n][j][e], acc[n], 0, 0, 0);
  };
  // (Round 4, measured: with all four rounds of a K = 1600 / 2048 product requested before the first multiply -- four
  // Frags, 154 / 108 registers -- the cell launch takes 12.7 us against 11.4 and the 8-unit query product 5.9 against 4.9:
  // the launch is not a chain of weight trips, it is the fp32 matrix rate (128 16x16x4 multiplies of 32 cycles per wave,
  // two waves per SIMD: 3.4 us) plus launch and epilogue; bf16 weights alone therefore buy only ~1 %.)
  // (Round 5, measured: the activations split by the loading lane into hi + lo bf16 terms and multiplied as two
  // v_mfma_f32_16x16x32_bf16 per 32-wide chunk -- 8 x fewer matrix cycles, VERDICT r04 item 4(i) -- leaves both launches where
  // they were: cell product 11.3 -> 11.1 us, backward product 8.6 -> 8.6, cfg D step 69.0 -> 68.9 ms.  The fp32 multiplies
  // were already hidden under the weight trips: the attention kernels stream 69 MB between two steps, so the 6.5 MB of
  // W_cell come from the memory side every step and a launch is launch + two to four dependent ~2 us trips + the
  // eight-wave reduction.  Not kept: the exact products cost nothing.)
  Frag f0, f1;
  load(0, f0);
  if (units <= SK_WAVES) {                  // one round: nothing to overlap
    mma(f0);
  } else {
    const int rounds = ((units + SK_WAVES - 1) / SK_WAVES + 1) & ~1;
    for (int r = 0; r < rounds; r += 2) {   // the loads of one round are in flight under the MFMAs of the other
      load(r + 1, f1);
      __builtin_amdgcn_sched_barrier(0);
      mma(f0);
      __builtin_amdgcn_sched_barrier(0);
      load(r + 2, f0);
      __builtin_amdgcn_sched_barrier(0);
      mma(f1);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // lane holds C[m0 + rg*4 + r][n0 + n*16 + col]
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][rg * 4 + r][n * 16 + col] = acc[n][r];
  __syncthreads();
  if constexpr (CELL) {
    if (!cl_on) return;
    const int m = (int)threadIdx.x / (TN / 4), ul = (int)threadIdx.x % (TN / 4), U = cell.U;
    float p[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {                          // the plain epilogue's sum, in its order
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < SK_WAVES; ++w) v += red[w][m][ul * 4 + g];
      if (bias) v += bias[n0 + ul * 4 + g];
      p[g] = v;
    }
    // cell_fwd_kernel (attention.hip), expression for expression
    const float cp = cl_cp;
    const float i = sk_sigf(p[0] + cl_wci * cp);
    const float g = tanhf(p[1]);
    const float f = sk_sigf(p[2] + cell.fb + cl_wcf * cp);
    float cn = g * i + cp * f;
    if (cell.clip > 0.f) cn = fminf(fmaxf(cn, -cell.clip), cell.clip);
    const float o = sk_sigf(p[3] + cl_wco * cn);
    const float hn = tanhf(cn) * o;
    const size_t ci = (size_t)cl_m * U + cl_u;
    float* gp = cell.gates + (size_t)cl_m * 4 * U;
    gp[cl_u] = i; gp[U + cl_u] = g; gp[2 * U + cl_u] = f; gp[3 * U + cl_u] = o;
    cell.c_raw[ci] = cn;
    cell.h_raw[ci] = hn;
    cell.c_out[ci] = cl_lv > 0.f ? cn : cp;
    const float ho = cl_lv > 0.f ? hn : cl_hp;
    cell.h_out[ci] = ho;
    if (cell.h_out2) cell.h_out2[(size_t)cl_m * cell.ld_h2 + cl_u] = ho;
    const float co = cell.out_mask ? hn * cl_om : hn;
    if (cell.cell_out) cell.cell_out[ci] = co;
    if (cell.cell_out2) cell.cell_out2[(size_t)cl_m * cell.ld_c2 + cl_u] = co;
    return;
  }
  for (int idx = threadIdx.x; idx < 16 * TN; idx += 64 * SK_WAVES) {
    const int m = idx / TN, n = idx % TN;
    if (m0 + m >= M) continue;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < SK_WAVES; ++w) v += red[w][m][n];
    if (bias) v += bias[n0 + n];
    float* cp = C + (size_t)(m0 + m) * ldc + n0 + n;
    if (accumulate) v += *cp;
    if (act == 1) v = fmaxf(v, 0.f);
    *cp = v;
  }
}

// Returns the ASR_GEMMP_SKINNY_* counter of the instantiation it launched, -1 where the skinny path does not apply.
static int try_gemm_skinny_f32(int transA, int transB, int M, int N, int K, const void* A, int lda, const void* B,
                               int ldb, void* C, int ldc, const float* bias, int accumulate, hipStream_t st, int act) {
  if (transA || M < 1 || M > 32 || K % 64 != 0 || N % 16 != 0 || K < 64) return -1;
  if (lda % 4 != 0 || ((uintptr_t)A) % 16 != 0 || ((uintptr_t)B) % 16 != 0) return -1;
  if (transB && ldb % 4 != 0) return -1;
  // full 128-byte lines of a row-major B need 32 columns per workgroup; B^T rows are contiguous in k, so the narrow
  // tile (twice the workgroups) is used until the launch is wide enough anyway
  const bool wide = (N % 32 == 0) && (!transB || N >= 32 * 192);
  const unsigned gy = (unsigned)((M + 15) / 16);
#define ASR_SKINNY(TB, NT_)                                                                                             \
  hipLaunchKernelGGL((gemm_skinny_f32_kernel<TB, NT_>), dim3(N / (16 * NT_), gy), dim3(64 * SK_WAVES), 0, st, M, N, K, \
                     (const float*)A, lda, (const float*)B, ldb, (float*)C, ldc, bias, accumulate, act, SkinnyCell{})
  if (transB) {
    if (wide) ASR_SKINNY(true, 2); else ASR_SKINNY(true, 1);
  } else {
    if (wide) ASR_SKINNY(false, 2); else ASR_SKINNY(false, 1);
  }
#undef ASR_SKINNY
  return transB ? (wide ? ASR_GEMMP_SKINNY_NT32 : ASR_GEMMP_SKINNY_NT16) : (wide ? ASR_GEMMP_SKINNY_NN32 : ASR_GEMMP_SKINNY_NN16);
}

// ---------------------------------------------------------------- lean TN kernel (bf16)
// C[M,N] = A^T B with A [K,M] and B [K,N] both REDUCTION-MAJOR (row = one k): the weight-gradient
// products X^T dG with K = T*B.  The MFMA fragments want 8 consecutive k per lane while memory has 8 consecutive m.
// gfx950 transposes on the LDS READ side: the tiles are copied into LDS as they come (one 16-byte vector = 8 columns
// of a k row per ds_write_b128), laid out as 16-column subtiles [128/16][64 k][16] so that the 4 x 16 block a
// 16-lane group needs is 128 contiguous bytes, and a fragment is two ds_read_b64_tr_b16 (k 0-3 and 4-7 of the lane's
// eight): each lane passes the address of one 8-byte piece of the block and receives its COLUMN.  Subtiles are
// 2080 bytes apart (2048 + 32) so the sixteen vectors of a k row land in sixteen different bank groups (TN_SUB and
// tn_frag: mfma_tn.h).
// (The first form of this kernel transposed on the WRITE side -- sixteen 32-bit LDS stores per thread and tile into
// a swizzled [m][k] image -- and ran the 5 x 512 weight gradients at ~200 TFLOP/s.)
// Split-K over slabs (summed in a fixed order by splitk_reduce_kernel), 128x128x64 tiles, double-buffered LDS.
// Requires M % 8 == 0, N % 8 == 0, lda/ldb % 8 == 0, 16-byte aligned bases.
// FRAMES (asr_gemm_tn_frames): the k rows are frames of a time-major [T, Bp] batch -- row k is utterance k % Bp at frame
// frame0 + k / Bp -- and B holds exact zeros in the rows of padded frames (t >= len[b]: the BPTT kernels' dgates).  Such a
// row is not requested from either operand; zeros go to LDS as for k >= kend.  Same tiles, same MFMA sequence, same slabs:
// a product 0 * a it drops added +-0 to an accumulator that is never -0, so the bits are those of the plain kernel.
// Where Bp divides 64 (kbeg and the k-tile step are multiples of 64) a thread's row kr0 + 16 q is one utterance in every
// k-tile, and "valid" is one more upper bound on k per q: the predicate costs the loop a compare against a register.
template <bool FRAMES>
__global__ __launch_bounds__(256) void gemm_tn_bf16_kernel(int M, int N, int K, const bf16_t* __restrict__ A,
                                                           int lda, const bf16_t* __restrict__ Bm, int ldb,
                                                           int kchunk, float* __restrict__ partial, int tn, int tm,
                                                           int nslab, int xcd_skip, TnFrames fv) {
  constexpr int BM = 128, BN = 128, BK = 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // 1-D grid; workgroup b runs on XCD b % 8 and the first xcd_skip XCDs are left to the recurrence clusters
  const int widx = xcd_work_index(xcd_skip);
  if (widx < 0 || widx >= tn * tm * nslab) return;
  const int bx = widx % tn, by = (widx / tn) % tm, bz = widx / (tn * tm);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = by * BM, n0 = bx * BN;
  const int kbeg = bz * kchunk, kend = min(K, kbeg + kchunk);
  const int nkt = (kend - kbeg + BK - 1) / BK;

  // four (k row, 8-column vector) items per operand per thread: vector mvec = tid & 15 of rows (tid >> 4) + 16 q
  const int mvec = tid & 15, kr0 = tid >> 4;
  const bool a_ok = m0 + mvec * 8 + 8 <= M, b_ok = n0 + mvec * 8 + 8 <= N;
  const bf16_t* pa = A + (size_t)(kbeg + kr0) * lda + m0 + mvec * 8;
  const bf16_t* pb = Bm + (size_t)(kbeg + kr0) * ldb + n0 + mvec * 8;
  const bf16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8_t ra[4], rb[4];
  // FRAMES: klim[q] = first k past the utterance's last valid frame, for the rows kr0 + 16 q (+ 64 kt) of this thread
  int klim[4] = {kend, kend, kend, kend};
  const bool per_q = FRAMES && (64 % fv.Bp) == 0;
  if constexpr (FRAMES) {
    if (per_q) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int b = (kr0 + 16 * q) % fv.Bp;
        const long lim = (long)max(fv.len[b] - fv.frame0, 0) * fv.Bp;
        klim[q] = (int)min((long)kend, lim);
      }
    }
  }
  auto gload = [&](int kt) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = kbeg + kt * BK + kr0 + 16 * q;
      const size_t ro = (size_t)(kt * BK + 16 * q);
      bool k_ok = k < klim[q];
      if constexpr (FRAMES) {
        if (!per_q && k_ok) {                              // any Bp: the row's utterance changes from k-tile to k-tile
          k_ok = tn_frame_valid(fv, k);
        }
      }
      ra[q] = (a_ok && k_ok) ? *reinterpret_cast<const bf16x8_t*>(pa + ro * lda) : zero;
      rb[q] = (b_ok && k_ok) ? *reinterpret_cast<const bf16x8_t*>(pb + ro * ldb) : zero;
    }
  };
  // image: subtile (mvec >> 1), row k (32 bytes), half (mvec & 1)
  const unsigned wbase = (unsigned)(mvec >> 1) * TN_SUB + (unsigned)kr0 * 32u + (unsigned)(mvec & 1) * 16u;
  auto sstore = [&](char* st) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<bf16x8_t*>(st + wbase + q * 16 * 32) = ra[q];
      *reinterpret_cast<bf16x8_t*>(st + TN_OPER + wbase + q * 16 * 32) = rb[q];
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  if (nkt > 0) {
    gload(0);
    sstore(smem);
  }
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  // lane's 8-byte piece of a 16-lane group's [4 k][16 col] block: row (fr >> 2), columns 4 (fr & 3) .. + 3; the
  // group fq takes k rows 8 fq .. 8 fq + 7 of the 32-row k-block (two reads, 4 rows = 128 bytes apart)
  const unsigned piece = (unsigned)(8 * fq + (fr >> 2)) * 32u + (unsigned)(fr & 3) * 8u;
  unsigned aoff[4], boff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    aoff[i] = (unsigned)(wm * 4 + i) * TN_SUB + piece;
    boff[i] = (unsigned)TN_OPER + (unsigned)(wn * 4 + i) * TN_SUB + piece;
  }
  for (int kt = 0; kt < nkt; ++kt) {
    const char* cur = smem + (kt & 1) * TN_STAGE;
    if (kt + 1 < nkt) gload(kt + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = tn_frag(cur + aoff[i] + ks * 32 * 32);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = tn_frag(cur + boff[j] + ks * 32 * 32);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nkt) sstore(smem + ((kt + 1) & 1) * TN_STAGE);
    __syncthreads();
  }
  // slab [z][M][N]; lane holds C[m = fr][n = fq*4 .. +3] of each 16x16 tile
  float* slab = partial + (size_t)bz * M * N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nb = n0 + wn * 64 + j * 16 + fq * 4;
      if (nb >= N) continue;                               // N % 8 == 0: a 4-group is all in or all out
      *reinterpret_cast<f32x4_t*>(slab + (size_t)m * N + nb) = acc[i][j];
    }
  }
}


// fixed-order sum of the split-K slabs -> deterministic
template <typename TO>
__global__ void splitk_reduce_kernel(const float* __restrict__ partial, int S, int M, int N,
                                     TO* __restrict__ C, int ldc, const float* __restrict__ bias,
                                     int accumulate, int act, int xcd_skip) {
  const size_t total = (size_t)M * N;
  const int widx = xcd_work_index(xcd_skip);
  if (widx < 0) return;
  const size_t nwork = (size_t)(gridDim.x >> 3) * (8 - xcd_skip) + max(0, (int)(gridDim.x & 7) - xcd_skip);
  for (size_t i = widx * (size_t)blockDim.x + threadIdx.x; i < total; i += nwork * blockDim.x) {
    const int m = i / N, n = i % N;
    float v = bias ? bias[n] : 0.f;
    // the slabs' values are requested eight at a time and added in slab order (round 6: one dependent load per addition
    // left this pass at the memory LATENCY per slab -- ~1 ms for 128 slabs where the bytes take 25 us; same sums, same order)
    int z = 0;
    for (; z + 8 <= S; z += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = partial[(size_t)(z + u) * total + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; z < S; ++z) v += partial[(size_t)z * total + i];
    TO* cp = C + (size_t)m * ldc + n;
    if (accumulate) v += load_out<TO>(cp);
    if (act == 1) v = fmaxf(v, 0.f);
    store_out<TO>(cp, v);
  }
}

// The lean TN path of a bf16 product (reduction-major operands: the weight-gradient products X^T dG), or false.
// fv.len != NULL: the frames form of the kernel (TnFrames); everything else -- tiles, kchunk, slabs, reducer -- is the same.
template <typename TO>
bool try_gemm_tn_bf16(asr_handle* h, int transA, int transB, int M, int N, int K, const void* A, int lda, const void* B,
                      int ldb, void* C, int ldc, const float* bias, int accumulate, hipStream_t st, int act,
                      TnFrames fv = TnFrames{nullptr, 1, 0}) {
  if (!(transA && !transB && K >= 2048 && M % 8 == 0 && N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 &&
        ((uintptr_t)A) % 16 == 0 && ((uintptr_t)B) % 16 == 0))
    return false;
  const int tm = (M + 127) / 128, tn = (N + 127) / 128;
  // workgroups (output tiles x split-K slabs) to aim at: ~2 per CU by default; a handle whose GEMMs run BESIDE a
  // recurrence kernel asks for few (asr_set_gemm_tn_workgroups): the slabs' write + re-read traffic is what stretches
  // the recurrence (BPTT launch 1340 / 1307 / 1285 / 1256 us with 1024 / 512 / 128 / 32 workgroups per GEMM)
  const int tn_wgs = h->tn_wgs > 0 ? h->tn_wgs : 512;
  int S = (tn_wgs + tm * tn - 1) / (tm * tn);
  const int maxS = (K + 255) / 256;
  if (S > maxS) S = maxS;
  if (S > 256) S = 256;
  while (S > 1 && (size_t)S * M * N * sizeof(float) > h->scratch_bytes - ASR_XCH_BYTES) --S;
  if ((size_t)S * M * N * sizeof(float) > h->scratch_bytes - ASR_XCH_BYTES) return false;
  int kchunk = (K + S - 1) / S;
  kchunk = (kchunk + 63) / 64 * 64;
  S = (K + kchunk - 1) / kchunk;
  const size_t lds = (size_t)2 * TN_STAGE;
  static unsigned long long attr_done = 0;
  if (first_on_device(attr_done)) {
    (void)hipFuncSetAttribute((const void*)gemm_tn_bf16_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void*)gemm_tn_bf16_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  float* partial = (float*)h->scratch;
  const int skip = h->xcd_skip;
  if (fv.len)
    hipLaunchKernelGGL(gemm_tn_bf16_kernel<true>, dim3(xcd_grid((long)tn * tm * S, skip)), dim3(256), lds, st, M, N, K,
                       (const bf16_t*)A, lda, (const bf16_t*)B, ldb, kchunk, partial, tn, tm, S, skip, fv);
  else
    hipLaunchKernelGGL(gemm_tn_bf16_kernel<false>, dim3(xcd_grid((long)tn * tm * S, skip)), dim3(256), lds, st, M, N, K,
                       (const bf16_t*)A, lda, (const bf16_t*)B, ldb, kchunk, partial, tn, tm, S, skip, fv);
  const size_t total = (size_t)M * N;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(splitk_reduce_kernel<TO>, dim3(xcd_grid(blocks, skip)), dim3(256), 0, st, partial, S, M, N,
                     (TO*)C, ldc, bias, accumulate, act, skip);
  return true;
}

template <typename T, typename TO, int BM, int BN>
int launch_layout(int transA, int transB, dim3 grid, size_t lds, hipStream_t st, int M, int N, int K,
                  const T* A, int lda, const T* B, int ldb, TO* C, int ldc, const float* bias,
                  int accumulate, int aa, int ba, int kchunk, float* partial, int act,
                  TnFrames fv = TnFrames{nullptr, 1, 0}) {
  // 4-column vector stores need the row starts of C aligned to 4 elements
  const int c_vec = (((uintptr_t)C) % (4 * sizeof(TO)) == 0) && (ldc % 4 == 0);
  if constexpr (sizeof(T) == 2 && sizeof(TO) == 4) {
    if (fv.len && transA && !transB) {                     // the frames form of the same kernel (asr_gemm_tn_frames)
      auto k = gemm_kernel<T, TO, BM, BN, true, false, true>;
      static unsigned long long attr_done = 0;             // (its own opt-in for the 128 x 128 tiles' 72 KB of LDS)
      if (first_on_device(attr_done))
        (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(k, grid, dim3(256), lds, st, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, aa, ba, kchunk,
                         partial, act, c_vec, fv);
      return 0;
    }
  }
#define ASR_GEMM_LAUNCH(TA_, TB_)                                                             \
  hipLaunchKernelGGL((gemm_kernel<T, TO, BM, BN, TA_, TB_>), grid, dim3(256), lds, st, M, N, K, A, \
                     lda, B, ldb, C, ldc, bias, accumulate, aa, ba, kchunk, partial, act, c_vec)
  if (!transA && !transB) ASR_GEMM_LAUNCH(false, false);
  else if (!transA && transB) ASR_GEMM_LAUNCH(false, true);
  else if (transA && !transB) ASR_GEMM_LAUNCH(true, false);
  else ASR_GEMM_LAUNCH(true, true);
#undef ASR_GEMM_LAUNCH
  return 0;
}

template <typename T, typename TO>
int launch_gemm(asr_handle* h, int transA, int transB, int M, int N, int K, const void* A, int lda,
                const void* B, int ldb, void* C, int ldc, const float* bias, int accumulate,
                hipStream_t st, int act, const float* mul = nullptr, int ldm = 0, bool* mul_done = nullptr,
                GemmDrop drop = GemmDrop{1.f, 0, 0, 0}, TnFrames fv = TnFrames{nullptr, 1, 0}) {
  constexpr int VEC = GT<T>::VEC, BK = GT<T>::BK;
  // every return below bumps the ASR_GEMMP_* counter of the kernel the product ended in (host integers on the handle)
  if constexpr (sizeof(T) == 4 && sizeof(TO) == 4) {
    const int sk = try_gemm_skinny_f32(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act);
    if (sk >= 0) {
      h->gemm_counts[sk] += 1;
      return 0;
    }
  }
  if constexpr (sizeof(T) == 2) {
    bool used_big = false;
    if (try_gemm_nt_bf16<TO>(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act, mul, ldm, drop,
                             nullptr, 0, nullptr, &used_big)) {
      if (mul_done) *mul_done = true;
      h->gemm_counts[used_big ? ASR_GEMMP_NT256 : ASR_GEMMP_NT128] += 1;
      return 0;
    }
    // reduction-major operands (X^T dG): lean TN kernel, always through split-K slabs
    if (try_gemm_tn_bf16<TO>(h, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act, fv)) {
      h->gemm_counts[ASR_GEMMP_TN_LEAN] += 1;
      return 0;
    }
  }
  const int aa = (((uintptr_t)A) % 16 == 0) && (lda % VEC == 0);
  const int ba = (((uintptr_t)B) % 16 == 0) && (ldb % VEC == 0);
  // big tiles only when they still fill the 256 CUs
  const long tiles128 = (long)((M + 127) / 128) * ((N + 127) / 128);
  if (tiles128 >= 320) {
    dim3 grid((N + 127) / 128, (M + 127) / 128);
    size_t lds = (size_t)2 * (128 + 128) * (BK + VEC) * sizeof(T);
    static unsigned long long attr_done = 0;   // 72 KB of dynamic LDS needs the opt-in
    if (first_on_device(attr_done)) {
      (void)hipFuncSetAttribute((const void*)gemm_kernel<T, TO, 128, 128, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      (void)hipFuncSetAttribute((const void*)gemm_kernel<T, TO, 128, 128, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      (void)hipFuncSetAttribute((const void*)gemm_kernel<T, TO, 128, 128, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      (void)hipFuncSetAttribute((const void*)gemm_kernel<T, TO, 128, 128, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    h->gemm_counts[ASR_GEMMP_GENERIC128] += 1;
    return launch_layout<T, TO, 128, 128>(transA, transB, grid, lds, st, M, N, K, (const T*)A, lda,
                                          (const T*)B, ldb, (TO*)C, ldc, bias, accumulate, aa, ba, K, nullptr, act, fv);
  }
  const long tiles64 = (long)((M + 63) / 64) * ((N + 63) / 64);
  // small output, long reduction (the dW = X^T dG products: K = T*B): split K over blockIdx.z so
  // the launch has >= ~2 workgroups per CU; slabs go to the handle's scratch and are summed in
  // a fixed order (deterministic, unlike fp32 atomics).
  int S = 1;
  if (tiles64 < 256 && K >= 16 * BK) {
    S = (int)((512 + tiles64 - 1) / tiles64);
    const int maxS = K / (4 * BK);
    if (S > maxS) S = maxS;
    if (S > 64) S = 64;
    while (S > 1 && (size_t)S * M * N * sizeof(float) > h->scratch_bytes - ASR_XCH_BYTES) --S;
  }
  size_t lds = (size_t)2 * (64 + 64) * (BK + VEC) * sizeof(T);
  if (S <= 1) {
    dim3 grid((N + 63) / 64, (M + 63) / 64);
    h->gemm_counts[ASR_GEMMP_GENERIC64] += 1;
    return launch_layout<T, TO, 64, 64>(transA, transB, grid, lds, st, M, N, K, (const T*)A, lda,
                                        (const T*)B, ldb, (TO*)C, ldc, bias, accumulate, aa, ba, K, nullptr, act, fv);
  }
  int kchunk = (K + S - 1) / S;
  kchunk = (kchunk + BK - 1) / BK * BK;
  S = (K + kchunk - 1) / kchunk;
  dim3 grid((N + 63) / 64, (M + 63) / 64, S);
  float* partial = (float*)h->scratch;
  h->gemm_counts[ASR_GEMMP_GENERIC64_SPLITK] += 1;
  launch_layout<T, TO, 64, 64>(transA, transB, grid, lds, st, M, N, K, (const T*)A, lda, (const T*)B, ldb,
                               (TO*)C, ldc, nullptr, 0, aa, ba, kchunk, partial, 0, fv);
  const size_t total = (size_t)M * N;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(splitk_reduce_kernel<TO>, dim3(blocks), dim3(256), 0, st, partial, S, M, N, (TO*)C, ldc,
                     bias, accumulate, act, 0);
  return 0;
}

// rows x [4, U] gate-major -> rows x [U, 4] (column 4 u + g <- column g U + u): the weight image of the CELL form of the
// skinny kernel; the bias is row `rows - 1` of the image when one is given
__global__ void interleave_gates_kernel(const float* __restrict__ W, const float* __restrict__ bias, int K, int U,
                                        float* __restrict__ out) {
  const size_t n = (size_t)(K + (bias ? 1 : 0)) * U;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t k = i / U;
    const int u = (int)(i % U);
    const float* src = k < (size_t)K ? W + k * 4 * U : bias;
    *reinterpret_cast<f32x4_t*>(out + k * 4 * U + (size_t)u * 4) = (f32x4_t){src[u], src[U + u], src[2 * U + u], src[3 * U + u]};
  }
}

// The bf16 images of a decoder cell's kernel W [K, 4U] (gate-major columns) for the BH forms of the skinny kernel:
//   frag [4U/32][K/64][64 lanes][32] bf16 -- gate-interleaved columns (4 u + g), fragment order (see the kernel): value
//        idx = (4j + e) * 2 + n of lane rg * 16 + col is W[unit * 64 + 16j + 4rg + e][column 32 nb + 16 n + col];
//   bias fp32 [4U], interleaved;   plain [K, 4U] bf16, W as it is (the backward product's B^T rows).
__global__ void cell_images_h_kernel(const float* __restrict__ W, const float* __restrict__ bias, int K, int U,
                                     bf16_t* __restrict__ frag, float* __restrict__ bias_il, bf16_t* __restrict__ plain) {
  const size_t n = (size_t)K * 4 * U;
  const int units = K / 64;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    plain[i] = f32_to_bf16(W[i]);
    // frag element i: decode (nb, unit, lane, idx)
    const int idx = (int)(i & 31), lane = (int)((i >> 5) & 63);
    const size_t bu = i >> 11;
    const int unit = (int)(bu % units), nb = (int)(bu / units);
    const int nn = idx & 1, je = idx >> 1, j = je >> 2, e = je & 3, rg = lane >> 4, col = lane & 15;
    const int k = unit * 64 + 16 * j + 4 * rg + e, c = nb * 32 + 16 * nn + col;      // interleaved column c = 4 u + g
    frag[i] = f32_to_bf16(W[(size_t)k * 4 * U + (size_t)(c & 3) * U + (c >> 2)]);
    if (i < (size_t)4 * U) bias_il[i] = bias ? bias[(i & 3) * U + (i >> 2)] : 0.f;
  }
}

}  // namespace

extern "C" int asr_gemm_act(asr_handle* h, int dtype, int out_dtype, int transA, int transB, int M,
                            int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                            int ldc, const float* bias, int accumulate, int act, asr_stream s);
extern "C" int asr_gemm(asr_handle* h, int dtype, int out_dtype, int transA, int transB, int M,
                        int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                        int ldc, const float* bias, int accumulate, asr_stream s) {
  return asr_gemm_act(h, dtype, out_dtype, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, 0, s);
}
extern "C" int asr_gemm_act(asr_handle* h, int dtype, int out_dtype, int transA, int transB, int M,
                            int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                            int ldc, const float* bias, int accumulate, int act, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!asr_dtype_ok(dtype) || !asr_dtype_ok(out_dtype))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_gemm: bad dtype %d/%d", dtype, out_dtype);
  if (act != 0 && act != 1) ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_gemm_act: act must be 0 (none) or 1 (relu)");
  if (M < 0 || N < 0 || K < 0 || !A || !B || !C)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_gemm: bad shape/pointer M=%d N=%d K=%d", M, N, K);
  if (lda < (transA ? M : K) || ldb < (transB ? K : N) || ldc < N)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_gemm: leading dimension too small (lda=%d ldb=%d ldc=%d)",
             lda, ldb, ldc);
  if (M == 0 || N == 0) return ASR_OK;
  hipStream_t st = (hipStream_t)s;
  if (dtype == ASR_F32 && out_dtype == ASR_F32)
    launch_gemm<float, float>(h, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act);
  else if (dtype == ASR_F32 && out_dtype == ASR_BF16)
    launch_gemm<float, bf16_t>(h, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act);
  else if (dtype == ASR_BF16 && out_dtype == ASR_F32)
    launch_gemm<bf16_t, float>(h, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act);
  else
    launch_gemm<bf16_t, bf16_t>(h, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act);
  ASR_CHECK_LAUNCH(h, "asr_gemm");
  return ASR_OK;
}

namespace {
__global__ void mul_rows_kernel(float* __restrict__ C, int ldc, const float* __restrict__ mul, int ldm, int M, int N) {
  const size_t total = (size_t)M * N;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i / N, n = i % N;
    C[m * ldc + n] *= mul[m * ldm + n];
  }
}
}  // namespace

// C = (op(A) op(B) + bias [+ C]) [relu] * mul, mul [M, N] fp32 with row stride ldmul: the multiplier is applied in the
// epilogue of the lean NT kernel (no second pass over C); other shapes run the plain GEMM and one multiply pass.
extern "C" int asr_gemm_mul(asr_handle* h, int dtype, int transA, int transB, int M, int N, int K, const void* A,
                            int lda, const void* B, int ldb, float* C, int ldc, const float* bias, int accumulate,
                            int act, const float* mul, int ldmul, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!mul) return asr_gemm_act(h, dtype, ASR_F32, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, act, s);
  if (!asr_dtype_ok(dtype) || (act != 0 && act != 1) || M < 0 || N < 0 || K < 0 || !A || !B || !C ||
      lda < (transA ? M : K) || ldb < (transB ? K : N) || ldc < N || ldmul < N)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_gemm_mul: bad args M=%d N=%d K=%d lda=%d ldb=%d ldc=%d ldmul=%d", M, N, K, lda,
             ldb, ldc, ldmul);
  if (M == 0 || N == 0) return ASR_OK;
  hipStream_t st = (hipStream_t)s;
  bool fused = false;
  if (dtype == ASR_F32)
    launch_gemm<float, float>(h, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act, mul, ldmul, &fused);
  else
    launch_gemm<bf16_t, float>(h, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act, mul, ldmul, &fused);
  ASR_CHECK_LAUNCH(h, "asr_gemm_mul");
  if (!fused) {
    const size_t total = (size_t)M * N;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(mul_rows_kernel, dim3(blocks), dim3(256), 0, st, C, ldc, mul, ldmul, M, N);
    h->gemm_counts[ASR_GEMMP_MUL_PASS] += 1;
    ASR_CHECK_LAUNCH(h, "asr_gemm_mul(multiply)");
  }
  return ASR_OK;
}

// C (fp32, CONTIGUOUS rows: ldc == N) = (op(A) op(B) + bias [+ C]) [relu] * dropout mask(seed, offset) of a [M,N] tensor
// -- asr_gemm_mul with the mask of asr_dropout_mask(M*N, keep, seed, offset) formed in the epilogue instead of read
// from memory (the lean NT kernel); other shapes run the plain GEMM and asr_dropout_apply in place.
extern "C" int asr_dropout_apply(asr_handle* h, int dtype, const void* in, void* out, size_t n, float keep_prob,
                                 uint64_t seed, uint64_t offset, asr_stream s);
extern "C" int asr_gemm_drop(asr_handle* h, int dtype, int transA, int transB, int M, int N, int K, const void* A,
                             int lda, const void* B, int ldb, float* C, int ldc, const float* bias, int accumulate,
                             int act, float keep_prob, uint64_t seed, uint64_t offset, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!asr_dtype_ok(dtype) || (act != 0 && act != 1) || M < 0 || N < 0 || K < 0 || !A || !B || !C ||
      lda < (transA ? M : K) || ldb < (transB ? K : N) || ldc != N || N % 4 != 0 || !(keep_prob > 0.f && keep_prob <= 1.f))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_gemm_drop: bad args M=%d N=%d K=%d ldc=%d (ldc == N, N %% 4 == 0)", M, N, K, ldc);
  if (M == 0 || N == 0) return ASR_OK;
  hipStream_t st = (hipStream_t)s;
  bool fused = false;
  const GemmDrop drop = {keep_prob, seed, offset, 1};
  if (dtype == ASR_F32)
    launch_gemm<float, float>(h, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act, nullptr, 0, &fused, drop);
  else
    launch_gemm<bf16_t, float>(h, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, st, act, nullptr, 0, &fused, drop);
  ASR_CHECK_LAUNCH(h, "asr_gemm_drop");
  if (!fused) {
    h->gemm_counts[ASR_GEMMP_DROP_PASS] += 1;
    return asr_dropout_apply(h, ASR_F32, C, C, (size_t)M * N, keep_prob, seed, offset, s);
  }
  return ASR_OK;
}

// asr_gemm_act / asr_gemm_mul / asr_gemm_drop (fp32 output) on the `num_rows` rows of the product that `rows` lists: the
// lean NT kernels in their listed-row form where the full product would take them (bf16 operands, NT, K % 64 == 0,
// N % 128 == 0, M >= 1024 ...); anywhere else the full product, exactly as the entry point without a list runs it.
extern "C" int asr_gemm_rows(asr_handle* h, int dtype, int transA, int transB, int M, int N, int K, const void* A,
                             int lda, const void* B, int ldb, float* C, int ldc, const float* bias, int accumulate,
                             int act, const float* mul, int ldmul, float keep_prob, uint64_t seed, uint64_t offset,
                             const int32_t* rows, int num_rows, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  const bool use_drop = keep_prob != 0.f;
  if (!rows || num_rows < 0 || num_rows > M || (mul && use_drop))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_gemm_rows: bad row list (rows=%p num_rows=%d M=%d) or both mul and dropout",
             (const void*)rows, num_rows, M);
  if (!asr_dtype_ok(dtype) || (act != 0 && act != 1) || M < 0 || N < 0 || K < 0 || !A || !B || !C ||
      lda < (transA ? M : K) || ldb < (transB ? K : N) || ldc < N || (mul && ldmul < N) ||
      (use_drop && (ldc != N || N % 4 != 0 || !(keep_prob > 0.f && keep_prob <= 1.f))))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_gemm_rows: bad args M=%d N=%d K=%d lda=%d ldb=%d ldc=%d ldmul=%d keep_prob=%g",
             M, N, K, lda, ldb, ldc, ldmul, (double)keep_prob);
  if (M == 0 || N == 0 || num_rows == 0) return ASR_OK;
  if (dtype == ASR_BF16) {
    const GemmDrop drop = {use_drop ? keep_prob : 1.f, seed, offset, use_drop ? 1 : 0};
    if (try_gemm_nt_bf16<float>(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, (hipStream_t)s, act,
                                mul, ldmul, drop, rows, num_rows, h->gemm_counts)) {
      ASR_CHECK_LAUNCH(h, "asr_gemm_rows");
      return ASR_OK;
    }
  }
  h->gemm_counts[ASR_GEMMP_ROWS_FULL] += 1;
  if (use_drop)
    return asr_gemm_drop(h, dtype, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, act, keep_prob, seed,
                         offset, s);
  return asr_gemm_mul(h, dtype, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate, act, mul, ldmul, s);
}

// C [M,N] fp32 (+= with accumulate) = A^T B on bf16 operands whose k rows are frames (see TnFrames above): the plain TN
// product's bits wherever B is zero in the rows of padded frames, without the loads of those rows from A or B -- on the
// lean TN kernel where asr_gemm takes it, on the generic kernel (the kernel asr_gemm runs for the shape) elsewhere.
extern "C" int asr_gemm_tn_frames(asr_handle* h, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                                  float* C, int ldc, int accumulate, const int32_t* seq_len, int Bp, int frame0,
                                  asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (M < 0 || N < 0 || K < 0 || !A || !B || !C || lda < M || ldb < N || ldc < N || !seq_len || Bp < 1 || frame0 < 0 ||
      K % Bp != 0)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_gemm_tn_frames: bad args M=%d N=%d K=%d lda=%d ldb=%d ldc=%d Bp=%d frame0=%d "
             "(K %% Bp == 0)", M, N, K, lda, ldb, ldc, Bp, frame0);
  if (M == 0 || N == 0) return ASR_OK;
  if (try_gemm_tn_bf16<float>(h, 1, 0, M, N, K, A, lda, B, ldb, C, ldc, nullptr, accumulate, (hipStream_t)s, 0,
                              TnFrames{seq_len, Bp, frame0})) {
    h->gemm_counts[ASR_GEMMP_TN_FRAMES] += 1;
    ASR_CHECK_LAUNCH(h, "asr_gemm_tn_frames");
    return ASR_OK;
  }
  // shapes outside the lean TN path: the generic kernel asr_gemm runs for them, in its frames form
  h->gemm_counts[ASR_GEMMP_TN_FRAMES_GENERIC] += 1;
  launch_gemm<bf16_t, float>(h, 1, 0, M, N, K, A, lda, B, ldb, C, ldc, nullptr, accumulate, (hipStream_t)s, 0, nullptr, 0,
                             nullptr, GemmDrop{1.f, 0, 0, 0}, TnFrames{seq_len, Bp, frame0});
  ASR_CHECK_LAUNCH(h, "asr_gemm_tn_frames");
  return ASR_OK;
}

// d(encoder output) [M, E] fp32 of a CTC head: dl [M, Kp] (the bf16 image of dlogits, asr_ctc_loss_ex) times Wp [E, Kp]^T
// (asr_ctc_head_prep), times the top layer's dropout mask (keep_prob != 0: asr_gemm_drop's epilogue), on the rows that
// `rows` lists (or all, rows == NULL): asr_gemm_rows' contract and kernels under counters of its own.
extern "C" int asr_ctc_head_bwd(asr_handle* h, int M, int E, int Kp, const void* dl, const void* Wp, float* denc,
                                float keep_prob, uint64_t seed, uint64_t offset, const int32_t* rows, int num_rows,
                                asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  const bool use_drop = keep_prob != 0.f;
  if (M < 0 || E < 1 || Kp < 1 || !dl || !Wp || !denc || E % 4 != 0 || (rows && (num_rows < 0 || num_rows > M)) ||
      (use_drop && !(keep_prob > 0.f && keep_prob <= 1.f)))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_ctc_head_bwd: bad args M=%d E=%d Kp=%d num_rows=%d keep_prob=%g (E %% 4 == 0)", M, E,
             Kp, num_rows, (double)keep_prob);
  if (M == 0 || (rows && num_rows == 0)) return ASR_OK;
  const GemmDrop drop = {use_drop ? keep_prob : 1.f, seed, offset, use_drop ? 1 : 0};
  if (try_gemm_nt_bf16<float>(0, 1, M, E, Kp, dl, Kp, Wp, Kp, denc, E, nullptr, 0, (hipStream_t)s, 0, nullptr, 0, drop, rows,
                              rows ? num_rows : 0, nullptr)) {
    h->gemm_counts[ASR_GEMMP_HEAD_BWD_LEAN] += 1;
    ASR_CHECK_LAUNCH(h, "asr_ctc_head_bwd");
    return ASR_OK;
  }
  h->gemm_counts[ASR_GEMMP_HEAD_BWD_FULL] += 1;
  if (use_drop)
    return asr_gemm_drop(h, ASR_BF16, 0, 1, M, E, Kp, dl, Kp, Wp, Kp, denc, E, nullptr, 0, 0, keep_prob, seed, offset, s);
  return asr_gemm_act(h, ASR_BF16, ASR_F32, 0, 1, M, E, Kp, dl, Kp, Wp, Kp, denc, E, nullptr, 0, 0, s);
}

ASR_DEFINE_COUNTS_N(gemm_path_counts, gemm_counts)

// ---------------------------------------------------------------- decoder cell: product + LSTM cell in one launch
extern "C" int asr_lstm_cell_gemm_prep(asr_handle* h, const float* W, const float* bias, int K, int U, float* W_il,
                                       asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!W || !W_il || K < 1 || U < 1 || ((uintptr_t)W_il) % 16 != 0)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_lstm_cell_gemm_prep: bad args");
  const size_t n = (size_t)(K + (bias ? 1 : 0)) * U;
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(interleave_gates_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, W, bias, K, U, W_il);
  ASR_CHECK_LAUNCH(h, "asr_lstm_cell_gemm_prep");
  return ASR_OK;
}
extern "C" int asr_lstm_cell_gemm_ok(int B, int K, int U, int ldx) {
  return B >= 1 && B <= 32 && K >= 64 && K % 64 == 0 && U >= 8 && U % 8 == 0 && ldx % 4 == 0 && ldx >= K;
}
extern "C" int asr_lstm_cell_gemm_fwd(asr_handle* h, const float* x, int ldx, int K, const float* W_il, int has_bias,
                                      const float* c_prev, const float* h_prev, const float* peep, const float* live,
                                      int B, int U, float forget_bias, float cell_clip, float* gates, float* c_raw,
                                      float* c_out, float* h_out, float* h_raw, const float* out_mask, float* cell_out,
                                      float* h_out2, int ld_h2, float* cell_out2, int ld_c2, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!x || !W_il || !c_prev || !h_prev || !live || !gates || !c_raw || !c_out || !h_out || !h_raw ||
      !asr_lstm_cell_gemm_ok(B, K, U, ldx) || ((uintptr_t)x) % 16 != 0 || ((uintptr_t)W_il) % 16 != 0 ||
      (h_out2 && ld_h2 < U) || (cell_out2 && ld_c2 < U))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_lstm_cell_gemm_fwd: bad args (B <= 32, K %% 64 == 0, U %% 8 == 0, 16-byte aligned rows)");
  SkinnyCell c;
  c.c_prev = c_prev; c.h_prev = h_prev; c.peep = peep; c.live = live; c.out_mask = out_mask;
  c.gates = gates; c.c_raw = c_raw; c.c_out = c_out; c.h_out = h_out; c.h_raw = h_raw;
  c.cell_out = cell_out; c.h_out2 = h_out2; c.cell_out2 = cell_out2;
  c.U = U; c.ld_h2 = ld_h2; c.ld_c2 = ld_c2; c.fb = forget_bias; c.clip = cell_clip;
  const int N = 4 * U;
  hipLaunchKernelGGL((gemm_skinny_f32_kernel<false, 2, true>), dim3(N / 32, (unsigned)((B + 15) / 16)), dim3(64 * SK_WAVES), 0,
                     (hipStream_t)s, B, N, K, x, ldx, W_il, N, (float*)nullptr, N, has_bias ? W_il + (size_t)K * N : nullptr,
                     0, 0, c);
  ASR_CHECK_LAUNCH(h, "asr_lstm_cell_gemm_fwd");
  return ASR_OK;
}

// ---- the same with bf16 weight images (bf16-operand models)
extern "C" size_t asr_lstm_cell_gemm_h_bytes(int K, int U) {
  return (size_t)K * 4 * U * 2 * 2 + (size_t)4 * U * 4;     // fragment image | interleaved fp32 bias | plain bf16 copy
}
static inline float* cell_h_bias(void* img, int K, int U) { return reinterpret_cast<float*>((char*)img + (size_t)K * 4 * U * 2); }
static inline bf16_t* cell_h_plain(void* img, int K, int U) {
  return reinterpret_cast<bf16_t*>((char*)img + (size_t)K * 4 * U * 2 + (size_t)4 * U * 4);
}
extern "C" int asr_lstm_cell_gemm_prep_h(asr_handle* h, const float* W, const float* bias, int K, int U, void* img,
                                         asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!W || !img || K < 64 || K % 64 != 0 || U < 8 || U % 8 != 0 || ((uintptr_t)img) % 16 != 0)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_lstm_cell_gemm_prep_h: bad args");
  const size_t n = (size_t)K * 4 * U;
  size_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(cell_images_h_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, W, bias, K, U,
                     (bf16_t*)img, cell_h_bias(img, K, U), cell_h_plain(img, K, U));
  ASR_CHECK_LAUNCH(h, "asr_lstm_cell_gemm_prep_h");
  return ASR_OK;
}
extern "C" int asr_lstm_cell_gemm_fwd_h(asr_handle* h, const float* x, int ldx, int K, const void* img,
                                        const float* c_prev, const float* h_prev, const float* peep, const float* live,
                                        int B, int U, float forget_bias, float cell_clip, float* gates, float* c_raw,
                                        float* c_out, float* h_out, float* h_raw, const float* out_mask, float* cell_out,
                                        float* h_out2, int ld_h2, float* cell_out2, int ld_c2, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!x || !img || !c_prev || !h_prev || !live || !gates || !c_raw || !c_out || !h_out || !h_raw ||
      !asr_lstm_cell_gemm_ok(B, K, U, ldx) || ((uintptr_t)x) % 16 != 0 || ((uintptr_t)img) % 16 != 0 ||
      (h_out2 && ld_h2 < U) || (cell_out2 && ld_c2 < U))
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_lstm_cell_gemm_fwd_h: bad args (B <= 32, K %% 64 == 0, U %% 8 == 0, 16-byte aligned rows)");
  SkinnyCell c;
  c.c_prev = c_prev; c.h_prev = h_prev; c.peep = peep; c.live = live; c.out_mask = out_mask;
  c.gates = gates; c.c_raw = c_raw; c.c_out = c_out; c.h_out = h_out; c.h_raw = h_raw;
  c.cell_out = cell_out; c.h_out2 = h_out2; c.cell_out2 = cell_out2;
  c.U = U; c.ld_h2 = ld_h2; c.ld_c2 = ld_c2; c.fb = forget_bias; c.clip = cell_clip;
  const int N = 4 * U;
  hipLaunchKernelGGL((gemm_skinny_f32_kernel<false, 2, true, true>), dim3(N / 32, (unsigned)((B + 15) / 16)),
                     dim3(64 * SK_WAVES), 0, (hipStream_t)s, B, N, K, x, ldx, (const float*)img, N, (float*)nullptr, N,
                     cell_h_bias(const_cast<void*>(img), K, U), 0, 0, c);
  ASR_CHECK_LAUNCH(h, "asr_lstm_cell_gemm_fwd_h");
  return ASR_OK;
}
// dx [B, K] = dpre [B, 4U] W^T on the plain bf16 copy inside the image (the decoder step's backward product)
extern "C" int asr_lstm_cell_gemm_bwd_h(asr_handle* h, const float* dpre, int B, int K, int U, const void* img, float* dx,
                                        int lddx, asr_stream s) {
  if (!h) return ASR_ERR_INVALID_ARG;
  if (!dpre || !img || !dx || B < 1 || B > 32 || K < 16 || K % 16 != 0 || U < 16 || U % 16 != 0 || lddx < K ||
      ((uintptr_t)dpre) % 16 != 0 || ((uintptr_t)img) % 16 != 0)
    ASR_FAIL(h, ASR_ERR_INVALID_ARG, "asr_lstm_cell_gemm_bwd_h: bad args (B <= 32, K %% 16 == 0, U %% 16 == 0)");
  hipLaunchKernelGGL((gemm_skinny_f32_kernel<true, 1, false, true>), dim3(K / 16, (unsigned)((B + 15) / 16)),
                     dim3(64 * SK_WAVES), 0, (hipStream_t)s, B, K, 4 * U, dpre, 4 * U,
                     (const float*)cell_h_plain(const_cast<void*>(img), K, U), 4 * U, dx, lddx, (const float*)nullptr, 0, 0,
                     SkinnyCell{});
  ASR_CHECK_LAUNCH(h, "asr_lstm_cell_gemm_bwd_h");
  return ASR_OK;
}
