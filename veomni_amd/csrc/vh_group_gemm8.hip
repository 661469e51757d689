// 256x256 grouped GEMMs for gfx950 (bf16, fp32 accumulate): the 8-phase
// nk8 (below), the register-staged mn8 ring and the persistent XCD-scheduled
// nk256s (fwd, and dgrad straight from the stored weights) / wgd256s (wgrad
// straight from the token-major operands). Retired variants are at commits
// 49b7734 and 2f18dcb; what they measured is in DESIGN.md.
//
// nk8: the deep-pipelined variant of vh_group_gemm.hip's same-NK kernel, built on
// the guide's 256-square 8-phase recipe (cdna_hip_programming.md §5 "The 256²
// 8-phase template" + T3/T4/T5): counted vmcnt (loads stay in flight across
// barriers), raw s_barrier (never __syncthreads — it would drain the LDS-DMA
// queue), s_setprio around each MFMA cluster.
//
// Geometry:
//   tile 256x256, K consumed in 32-deep k-subs; 512 threads = 8 waves in a
//   2(M) x 4(N) grid, 128x64 per wave = 8x4 16x16 fragments (128 acc VGPRs).
//   LDS = 4-deep ring of k-sub slots x {A, B}, slot = [256 rows][32 k] bf16
//   (16 KiB) -> 128 KiB total, 1 block/CU, 2 waves/SIMD.
//   Per k-sub: 2 phases x {8 ds_read_b128 + 16 MFMA + raw barrier}.
//   Staging: 2 glds (A) + a register-transposed B slot issued at phase 0 of
//   each k-sub for slot s+3; vmcnt(6) then admits slot s while 3 slots stay
//   in flight.
//
// Dispatched by vh_group_gemm_nk_bf16 (vh_group_gemm.hip) for the large
// B [K, N] (!trans_b) shapes that nk256s_kn does not take (K % 64 == 32,
// G > 4096).

#include "vh_common.h"

#include <type_traits>

namespace {

constexpr int BM8 = 256, BN8 = 256, KSUB = 32;
constexpr int THREADS8 = 512;

using bf16frag = __attribute__((ext_vector_type(8))) __bf16;

__device__ __forceinline__ void glds16(const bf16_t* g, bf16_t* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)g,
      (__attribute__((address_space(3))) unsigned int*)l, 16, 0, 0);
}

// swizzle for the [256][32] k-sub slot (row = 64 B): 4 16-B slots per row;
// bank row = 256 B = 4 tile rows, so rows r, r+4, r+8, r+12 share a bank
// phase -> slot = (row>>2)&3 makes each mod-4 class conflict-free over the
// 16 consecutive rows a ds_read_b128 lane group touches.
__device__ __forceinline__ int swz32(int row, int colb) {
  return colb ^ (((row >> 2) & 3) << 4);
}

__device__ __forceinline__ void raw_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

#define VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

// K-contiguous staging of one [256][32] slot via glds (2 instructions of
// 8 KiB; per-lane source carries the inverse swizzle).
struct KStage8 {
  const bf16_t* src[2];
  int lds_base[2];

  template <typename RowFn>
  __device__ __forceinline__ void init(const bf16_t* s, int64_t ld_elems,
                                       RowFn row_of, int tid) {
    const int lane = tid & 63;
    const int wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int base = i * 8192 + wave * 1024;
      int o = base + lane * 16;
      int row = o >> 6;           // 64 B per row
      int colb = o & 63;
      src[i] = s + row_of(row) * ld_elems + (swz32(row, colb) >> 1);
      lds_base[i] = base;
    }
  }

  __device__ __forceinline__ void stage(bf16_t* slot, int64_t k0) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) glds16(src[i] + k0, slot + (lds_base[i] >> 1));
  }
};

// Transposed staging of one [256 out][32 k] slot from a [k][out] source.
// Thread t: o0 = (t&31)*8, kp = (t>>5)*2 -> 2 x 16-B loads (8 consecutive
// outs, k and k+1; 32 lanes x 16 B = 512 B coalesced), 8 x ds_write_b32
// (the (k, k+1) pair is contiguous in the [out][k] image).
struct TStage8 {
  const bf16_t* base;
  int64_t ld;
  bool out_ok;
  int64_t gout_left;
  int o0, kp;

  __device__ __forceinline__ void init(const bf16_t* s, int64_t ld_elems,
                                       int out0, int out_max, int tid) {
    o0 = (tid & 31) * 8;
    kp = (tid >> 5) * 2;
    int64_t gout = (int64_t)out0 + o0;
    gout_left = out_max - gout;
    out_ok = gout_left >= 8;
    base = s + gout;
    ld = ld_elems;
  }

  __device__ __forceinline__ void stage(bf16_t* slot, int64_t k0) const {
    bf16x8 v[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int64_t k = k0 + kp + i;
      if (out_ok) {
        v[i] = *reinterpret_cast<const bf16x8*>(base + k * ld);
      } else if (gout_left > 0) {
        const bf16_t* p = base + k * ld;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i].v[j] = (j < gout_left) ? p[j] : bf16_t(0);
      } else {
        v[i] = bf16x8{};
      }
    }
    const int colb = kp * 2;  // 4-B aligned pair position
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int row = o0 + j;
      ushort2 pk = {v[0].v[j], v[1].v[j]};
      *reinterpret_cast<uint32_t*>(&slot[(row * 64 + swz32(row, colb & ~15) + (colb & 15)) >> 1]) =
          *reinterpret_cast<uint32_t*>(&pk);
    }
  }
};

__device__ __forceinline__ bf16frag frag_read8(const bf16_t* slot, int row0,
                                               int lane) {
  int row = row0 + (lane & 15);
  int colb = ((lane >> 4) << 3) * 2;  // k position within the 32-k slot
  int off_b = row * 64 + swz32(row, colb);
  return *reinterpret_cast<const bf16frag*>(
      reinterpret_cast<const char*>(slot) + off_b);
}

// C_g = A_g @ B_g with B [K, N]: A rows K-contiguous via glds (wrapped past
// the group's end), B transposed-staged through registers.
__global__ __launch_bounds__(THREADS8, 2) void k_group_gemm_nk8(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
    bf16_t* __restrict__ C, const int64_t* __restrict__ cumsum, int G,
    int64_t N, int64_t K, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* sm = reinterpret_cast<bf16_t*>(smem);
  auto slotA = [&](int s) { return sm + (s & 3) * 8192; };          // 4 x 16 KiB
  auto slotB = [&](int s) { return sm + 32768 + (s & 3) * 8192; };  // 4 x 16 KiB

  const int gid = blockIdx.y;
  const int64_t row_start = (gid > 0) ? cumsum[gid - 1] : 0;
  const int64_t m_size = cumsum[gid] - row_start;
  const int bm = blockIdx.x / tiles_n;
  const int bn = blockIdx.x % tiles_n;
  if ((int64_t)bm * BM8 >= m_size) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;  // 2x4 wave grid; 128x64 per wave

  const bf16_t* Ag = A + row_start * K;
  const bf16_t* Bg = B + (int64_t)gid * N * K;
  bf16_t* Cg = C + row_start * N;

  KStage8 sa;
  sa.init(Ag, K, [&](int r) -> int64_t {
    int64_t gm = (int64_t)bm * BM8 + r;
    return gm % m_size;
  }, tid);
  TStage8 sb;
  sb.init(Bg, N, bn * BN8, (int)N, tid);

  auto stage = [&](int s, int64_t k0) {
    sa.stage(slotA(s), k0);
    sb.stage(slotB(s), k0);
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int nsub = (int)(K / KSUB);
  // prologue: slots 0..2 in flight
  stage(0, 0);
  stage(1, KSUB);
  if (nsub > 2) stage(2, 2 * KSUB);
  for (int s = 0; s < nsub; ++s) {
    // phase 0: issue next staging, admit slot s, compute fragment half 0
    if (s + 3 < nsub) stage(s + 3, (int64_t)(s + 3) * KSUB);
    // counted wait: slot s must have landed; younger slots stay in flight.
    // glds per in-flight slot: 2 (A only — B is synchronous ds_writes).
    // Tail k-subs have fewer in flight.
    {
      const int rem = nsub - s;  // slots still live: s .. min(s+3, nsub-1)
      if (rem >= 4) VMCNT(6);
      else if (rem == 3) VMCNT(4);
      else if (rem == 2) VMCNT(2);
      else VMCNT(0);
    }
    raw_barrier();
    {
      const bf16_t* TA = slotA(s);
      const bf16_t* TB = slotB(s);
      bf16frag af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag_read8(TA, wr * 128 + i * 16, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = frag_read8(TB, wc * 64 + j * 16, lane);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      raw_barrier();
      // phase 1: fragment half 1 (rows 64..127 of this wave's panel)
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag_read8(TA, wr * 128 + 64 + i * 16, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = frag_read8(TB, wc * 64 + j * 16, lane);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i + 4][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i + 4][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    raw_barrier();
  }

  const int col_in = lane & 15;
  const int row_base_in = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        int64_t m = (int64_t)bm * BM8 + wr * 128 + (i & 3) * 16 + (i >> 2) * 64 +
                    row_base_in + rr;
        int64_t n = (int64_t)bn * BN8 + wc * 64 + j * 16 + col_in;
        if (m < m_size && n < N) Cg[m * N + n] = f2bf(acc[i][j][rr]);
      }
}

}  // namespace

extern "C" int vh_group_gemm_nk8_bf16(const uint16_t* A, const uint16_t* B,
                                      uint16_t* C, const int64_t* cumsum,
                                      int G, int64_t N, int64_t K,
                                      int64_t total_rows, int trans_b,
                                      void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(K % KSUB == 0 && K / KSUB >= 2, "K must be a multiple of 32, >= 64");
  VH_CHECK(N % 16 == 0, "N %% 16 != 0");
  VH_CHECK(trans_b == 0, "trans_b != 0 (B [N, K] goes to nk256s / 128x128)");
  int tiles_m = (int)((total_rows + BM8 - 1) / BM8);
  if (tiles_m < 1) tiles_m = 1;
  int tiles_n = (int)((N + BN8 - 1) / BN8);
  dim3 grid(tiles_m * tiles_n, G);
  hipLaunchKernelGGL(k_group_gemm_nk8, grid, dim3(THREADS8), 131072, s,
                     reinterpret_cast<const bf16_t*>(A),
                     reinterpret_cast<const bf16_t*>(B),
                     reinterpret_cast<bf16_t*>(C), cumsum, G, N, K, tiles_m,
                     tiles_n);
  VH_HIP(hipGetLastError());
  return 0;
}

// ============================================================================
// Register-staged 256x256 ring kernel (no glds — every load is
// compiler-visible, so hipcc emits counted waits and the T14 split pipelines
// cleanly; mixing glds with ordinary loads makes the compiler drain vmcnt(0)
// at every ds_write — the §5 "Three .s-level traps" (b) case).
//
//   k_group_gemm_mn8: C[g] = A_g^T @ B_g, both operands transposed-staged,
//       per-group ragged K (row count).
//
// Ring: 4 k-sub slots x {A, B} (16 KiB each, 128 KiB LDS, 1 block/CU,
// 8 waves). Per k-sub: load slot s+3's registers, two 16-MFMA phases on slot
// s, flush slot s+2's ds_writes, one barrier.
// ============================================================================

namespace {

// Transposed register staging with split load/flush and optional k clamp.
template <bool CLAMP>
struct TRegStage8 {
  const bf16_t* base;
  int64_t ld, kmax;
  bool out_ok;
  int64_t gout_left;
  int o0, kp;

  __device__ __forceinline__ void init(const bf16_t* s, int64_t ld_elems,
                                       int64_t kmax_, int out0, int out_max,
                                       int tid) {
    o0 = (tid & 31) * 8;
    kp = (tid >> 5) * 2;
    int64_t gout = (int64_t)out0 + o0;
    gout_left = out_max - gout;
    out_ok = gout_left >= 8;
    base = s + gout;
    ld = ld_elems;
    kmax = kmax_;
  }

  __device__ __forceinline__ void load(bf16x8 (&v)[2], int64_t k0) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int64_t k = k0 + kp + i;
      bool kok = !CLAMP || k < kmax;
      if (kok && out_ok) {
        v[i] = *reinterpret_cast<const bf16x8*>(base + k * ld);
      } else if (kok && gout_left > 0) {
        const bf16_t* p = base + k * ld;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i].v[j] = (j < gout_left) ? p[j] : bf16_t(0);
      } else {
        v[i] = bf16x8{};
      }
    }
  }

  __device__ __forceinline__ void flush(bf16_t* slot, const bf16x8 (&v)[2]) const {
    const int colb = kp * 2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int row = o0 + j;
      ushort2 pk = {v[0].v[j], v[1].v[j]};
      *reinterpret_cast<uint32_t*>(&slot[(row * 64 + swz32(row, colb & ~15) + (colb & 15)) >> 1]) =
          *reinterpret_cast<uint32_t*>(&pk);
    }
  }
};

#define VH_MFMA_PHASE8(TA_, TB_, ROWOFF, ACCOFF)                               \
  {                                                                            \
    bf16frag af[4], bfr[4];                                                    \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                              \
        af[i] = frag_read8(TA_, wr * 128 + (ROWOFF) + i * 16, lane);           \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                              \
        bfr[j] = frag_read8(TB_, wc * 64 + j * 16, lane);                      \
    __builtin_amdgcn_s_setprio(1);                                             \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                              \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                          \
            acc[i + (ACCOFF)][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(    \
                af[i], bfr[j], acc[i + (ACCOFF)][j], 0, 0, 0);                 \
    __builtin_amdgcn_s_setprio(0);                                             \
  }

// ring skeleton. Two pending register sets: slot
// s+3's loads issue at k-sub s and flush at the END of k-sub s+1 — the
// load->flush gap spans TWO 32-MFMA blocks (~2k cycles) so HBM/L3 latency
// is fully covered.
#define VH_RING_LOOP(SA, SB, NSUB)                                             \
  {                                                                            \
    bf16x8 va0[2], vb0[2];                                                     \
    SA.load(va0, 0);                                                           \
    SB.load(vb0, 0);                                                           \
    SA.flush(slotA(0), va0);                                                   \
    SB.flush(slotB(0), vb0);                                                   \
    if ((NSUB) > 1) {                                                          \
      SA.load(va0, KSUB);                                                      \
      SB.load(vb0, KSUB);                                                      \
      SA.flush(slotA(1), va0);                                                 \
      SB.flush(slotB(1), vb0);                                                 \
    }                                                                          \
    bf16x8 vap[2], vbp[2], van[2], vbn[2];                                     \
    if ((NSUB) > 2) {                                                          \
      SA.load(vap, 2 * KSUB);                                                  \
      SB.load(vbp, 2 * KSUB);                                                  \
    }                                                                          \
    __syncthreads();                                                           \
    for (int s = 0; s < (NSUB); ++s) {                                         \
      const bool more = s + 3 < (NSUB);                                        \
      if (more) {                                                              \
        SA.load(van, (int64_t)(s + 3) * KSUB);                                 \
        SB.load(vbn, (int64_t)(s + 3) * KSUB);                                 \
      }                                                                        \
      {                                                                        \
        const bf16_t* TA = slotA(s);                                           \
        const bf16_t* TB = slotB(s);                                           \
        VH_MFMA_PHASE8(TA, TB, 0, 0)                                           \
        VH_MFMA_PHASE8(TA, TB, 64, 4)                                          \
      }                                                                        \
      if (s + 2 < (NSUB)) {                                                    \
        SA.flush(slotA(s + 2), vap);                                           \
        SB.flush(slotB(s + 2), vbp);                                           \
      }                                                                        \
      _Pragma("unroll") for (int q = 0; q < 2; ++q) {                          \
        vap[q] = van[q];                                                       \
        vbp[q] = vbn[q];                                                       \
      }                                                                        \
      __syncthreads();                                                         \
    }                                                                          \
  }

__global__ __launch_bounds__(THREADS8, 2) void k_group_gemm_mn8(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
    bf16_t* __restrict__ C, const int64_t* __restrict__ cumsum, int G,
    int64_t M, int64_t N, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* sm = reinterpret_cast<bf16_t*>(smem);
  auto slotA = [&](int s) { return sm + (s & 3) * 8192; };
  auto slotB = [&](int s) { return sm + 32768 + (s & 3) * 8192; };

  const int gid = blockIdx.y;
  const int64_t row_start = (gid > 0) ? cumsum[gid - 1] : 0;
  const int64_t kcount = cumsum[gid] - row_start;
  const int bm = blockIdx.x / tiles_n;
  const int bn = blockIdx.x % tiles_n;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;

  bf16_t* Cg = C + (int64_t)gid * M * N;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  if (kcount > 0) {
    const bf16_t* Ag = A + row_start * M;
    const bf16_t* Bg = B + row_start * N;
    TRegStage8<true> sa, sb;
    sa.init(Ag, M, kcount, bm * BM8, (int)M, tid);
    sb.init(Bg, N, kcount, bn * BN8, (int)N, tid);
    const int nsub = (int)((kcount + KSUB - 1) / KSUB);
    VH_RING_LOOP(sa, sb, nsub)
  }

  const int col_in = lane & 15;
  const int row_base_in = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        int64_t m = (int64_t)bm * BM8 + wr * 128 + (i & 3) * 16 + (i >> 2) * 64 +
                    row_base_in + rr;
        int64_t n = (int64_t)bn * BN8 + wc * 64 + j * 16 + col_in;
        if (m < M && n < N) Cg[m * N + n] = f2bf(acc[i][j][rr]);
      }
}

}  // namespace

extern "C" int vh_group_gemm_mn8_bf16(const uint16_t* A, const uint16_t* B,
                                      uint16_t* C, const int64_t* cumsum,
                                      int G, int64_t M, int64_t N,
                                      void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int tiles_m = (int)((M + BM8 - 1) / BM8);
  int tiles_n = (int)((N + BN8 - 1) / BN8);
  dim3 grid(tiles_m * tiles_n, G);
  hipLaunchKernelGGL(k_group_gemm_mn8, grid, dim3(THREADS8), 131072, s,
                     reinterpret_cast<const bf16_t*>(A),
                     reinterpret_cast<const bf16_t*>(B),
                     reinterpret_cast<bf16_t*>(C), cumsum, G, M, N, tiles_m,
                     tiles_n);
  VH_HIP(hipGetLastError());
  return 0;
}

// ============================================================================
// 256x256 x BK=64 double-buffered glds structure (shared by nk256s and
// wgd256s below): the 128x128 2-phase structure scaled to a 256-square tile —
// 2x the MFMA work per staged byte and per barrier drain, with the proven
// conflict-free 128-B-row swizzle.
// 8 waves (2x4), per wave 128x64; LDS = 2 x (A 32K + B 32K) = 128 KiB.
// ============================================================================

namespace {

constexpr int BK64 = 64;

// conflict-free slot map for 128-B rows (see vh_group_gemm.hip swz comment)
__device__ __forceinline__ int swz64(int row, int colb) {
  return colb ^ ((((row >> 1) ^ (row >> 3)) & 7) << 4);
}

struct KStage64 {  // [256][64] tile via 4 glds of 8 KiB (512 threads)
  const bf16_t* src[4];
  int lds_base[4];

  template <typename RowFn>
  __device__ __forceinline__ void init(const bf16_t* s, int64_t ld_elems,
                                       RowFn row_of, int tid) {
    const int lane = tid & 63;
    const int wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int base = i * 8192 + wave * 1024;
      int o = base + lane * 16;
      int row = o >> 7;  // 128 B per row
      int colb = o & 127;
      src[i] = s + row_of(row) * ld_elems + (swz64(row, colb) >> 1);
      lds_base[i] = base;
    }
  }

  __device__ __forceinline__ void stage(bf16_t* tile, int64_t k0) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(src[i] + k0, tile + (lds_base[i] >> 1));
  }
};

__device__ __forceinline__ bf16frag frag_read64(const bf16_t* tile, int row0,
                                                int ks, int lane) {
  int row = row0 + (lane & 15);
  int colb = (ks * 32 + ((lane >> 4) << 3)) * 2;
  int off_b = row * 128 + swz64(row, colb);
  return *reinterpret_cast<const bf16frag*>(
      reinterpret_cast<const char*>(tile) + off_b);
}

// ----------------------------------------------------------------------------
// "Reduction-slow" tiles: a [64 k][256 out] bf16 tile (32 KiB, the footprint
// of the [256][64] tile above) of an operand whose reduction index is the
// SLOW one in memory — both wgrad operands ([rows, M] / [rows, N], k = row)
// and the stored weights W[g][K][N] for dgrad. No transposed copy is made:
// the tile is staged as it lies in memory and the MFMA fragments are read
// with the CDNA4 transposing LDS read (ds_read_b64_tr_b16).
//
// Image: k-row r occupies bytes [512 r, 512 r + 512); inside the row the
// sixteen 32-B segments (16 outs each) are permuted,
//     off(r, seg) = 512 r + 32 (seg ^ h(r)),   h(r) = (r & 3) | ((r >> 3) & 1) << 2.
// Why this h. A transposed read hands each 16-lane group a block of 4 k-rows
// x 16 outs (lane 4q+p: row q, outs 4p..4p+3, 8 B). For the 16x16x32 operand,
// group g of the wave takes k = 32 ks + 8 g + {0..3} (first read) and
// + {4..7} (second read), all groups in the same 16 outs, i.e. the same seg.
// Banks are counted per 32-lane half, 64 banks = 256 B: a half holds groups
// {0,1} or {2,3}, so 8 k-rows {b..b+3} u {b+8..b+11} with b % 4 == 0, each
// contributing one 32-B segment (8 banks). Rows are 512 B = 2 bank rows, so
// without the XOR all 8 land on the same 8 banks (8-way). Over those 8 rows
// r & 3 takes 0..3 and bit 3 of r takes both values, so h(r) takes all of
// 0..7 and (seg ^ h) & 7 — the segment's 32-B position in the bank row — is
// distinct for the 8 rows: 8 x 8 banks = all 64, conflict-free. h ignores
// bit 2, so the second read (+4 rows) is the first one 2048 B further on.
// Every lane address is 512 r + 32 x + 8 p: 8-byte aligned.
// Fill: glds writes LDS lane-linearly (wave w, instruction i, lane l -> byte
// 8192 i + 1024 w + 16 l: always conflict-free); the permutation is carried
// by the per-lane SOURCE column, and since h(16 i + 2 w + (l >> 5)) does not
// depend on i, one column offset per lane serves all four instructions. A
// wave instruction fetches two whole 512-B k-rows: fully coalesced.
// The transposed reads need EXEC all ones (the gather crosses lanes): they
// are only ever issued from wave-uniform control flow; tails are handled by
// padding the tile (clamped source row, zeroed LDS rows), never by masking.
// ----------------------------------------------------------------------------
__device__ __forceinline__ int tswz64(int k) {
  return (k & 3) | (((k >> 3) & 1) << 2);
}

struct TStage64 {  // [64 k][256 out] tile via 4 glds of 8 KiB (512 threads)
  const bf16_t* src;  // operand base + this lane's (permuted) column
  int64_t ld;
  int krow;           // this lane's k-row within each 16-row glds: 2 w + (l >> 5)
  int wave;           // wave-uniform (SGPR)

  // col_of(c): source column of tile column c (c a 16-multiple; wrap/clamp
  // partial tiles there so every staged address stays in bounds)
  template <typename ColFn>
  __device__ __forceinline__ void init(const bf16_t* s, int64_t ld_elems,
                                       ColFn col_of, int tid) {
    const int lane = tid & 63;
    wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    krow = wave * 2 + (lane >> 5);
    const int pb = (lane & 31) * 16;  // byte within the 512-B LDS row
    const int seg = (pb >> 5) ^ tswz64(krow);
    src = s + col_of(seg * 16) + ((pb & 31) >> 1);
    ld = ld_elems;
  }

  // row_of(k): source row of tile k-row k0 + k' (a functor, so a row-index
  // indirection can be folded in later)
  template <typename RowFn>
  __device__ __forceinline__ void stage(bf16_t* tile, int k0, RowFn row_of) const {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      glds16(src + (int64_t)row_of(k0 + i * 16 + krow) * ld,
             tile + ((i * 8192 + wave * 1024) >> 1));
  }

  // Zero the k-rows >= rem that THIS wave staged (call after vmcnt(0), before
  // the barrier that publishes the tile). Wave-uniform branches; a row is
  // one 64-lane x 8-B store.
  __device__ __forceinline__ void zero_tail(bf16_t* tile, int rem, int lane) const {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int k = i * 16 + wave * 2 + b;
        if (k >= rem)
          *reinterpret_cast<uint2*>(reinterpret_cast<char*>(tile) + k * 512 +
                                    lane * 8) = uint2{0u, 0u};
      }
  }
};

// 16x16x32 fragments (out = out0 + (lane & 15), k = 32 ks + 8 (lane >> 4) +
// 0..7: the k-to-lane map of frag_read64) from a [64 k][256 out] tile, as two
// transposed reads of 4 k each.
// The reads are inline asm on purpose: through the builtin the compiler
// cannot tell them from the tile the LDS-DMA is filling and puts
// s_waitcnt vmcnt(0) in front of the first read, which serialises the
// prefetch of the next k-tile with the MFMAs of this one. The asm is opaque
// to the compiler's counters, so tr_wait ties the destination registers to
// an explicit s_waitcnt lgkmcnt(0): nothing can use (or copy) them earlier.
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
struct TrFrag { u32x2 lo, hi; };

__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(size_t)(const __attribute__((address_space(3))) char*)p;
}

// this lane's byte offset in the tile for the fragment at outs out0..out0+15
__device__ __forceinline__ int tr_lane_off(int out0, int lane) {
  const int k = ((lane >> 4) << 3) + ((lane >> 2) & 3);
  return k * 512 + (((out0 >> 4) ^ tswz64(k)) << 5) + (lane & 3) * 8;
}

// addr = LDS byte address of the tile + tr_lane_off; KS = 32-k half (0/1)
template <int KS>
__device__ __forceinline__ void tr_issue(TrFrag& f, uint32_t addr) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2 offset:%3\n\t"
      "ds_read_b64_tr_b16 %1, %2 offset:%4"
      : "=&v"(f.lo), "=&v"(f.hi)
      : "v"(addr), "n"(KS * 16384), "n"(KS * 16384 + 2048)
      : "memory");
}

__device__ __forceinline__ void tr_wait(TrFrag (&f)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(f[0].lo), "+v"(f[0].hi), "+v"(f[1].lo), "+v"(f[1].hi),
                 "+v"(f[2].lo), "+v"(f[2].hi), "+v"(f[3].lo), "+v"(f[3].hi)
               :
               : "memory");
}

__device__ __forceinline__ bf16frag tr_frag(const TrFrag& f) {
  u32x4 u{f.lo.x, f.lo.y, f.hi.x, f.hi.y};
  return __builtin_bit_cast(bf16frag, u);
}

// ============================================================================
// nk256s: the inner loop above under a DEVICE-BUILT tile schedule with
// XCD-clustered persistent blocks.
//
// Why (PMC, profiles/r02_groupgemm_pmc.txt): a plain (tiles x G) grid
// dispatches consecutive blocks round-robin across the 8 XCDs, so blocks
// sharing a group's A/B tiles land on DIFFERENT L2s — zero reuse. At the
// bench shapes every 256x256 tile streams ~2 MB from HBM (~6.5 TB/s:
// HBM-bound at 20% MFMA-busy, vs the Tensile reference's 82%). The grid is
// also sized for worst-case skew (ceil(total/256) m-tiles for EVERY group):
// at G=128 that is ~786k blocks, 99% of which exit immediately.
//
// Structure:
//   - k_gg_sched (1 tiny launch) turns cumsum into a per-group tile prefix
//     sum in a device workspace: group g owns tiles_m_g x tiles_n tiles,
//     enumerated bm-inner (consecutive tiles share the B n-slab).
//   - the GEMM launches a FIXED grid of 256 persistent blocks (1/CU at
//     128 KiB LDS). Block b runs on XCD b%8 (dispatch affinity);
//     it walks the CONTIGUOUS tile range [X*L, (X+1)*L) of the global list
//     with stride 32, so the ~32 concurrently-resident blocks of an XCD
//     process consecutive tiles of the SAME group — the group's B n-slab
//     (~1 MB) and the shared A m-tiles stay hot in that XCD's 4 MB L2.
//   - zero-count groups occupy no schedule slots; per-tile group lookup is
//     a binary search over the prefix (G<=4096).
// ============================================================================

__global__ void k_gg_sched(const int64_t* __restrict__ cumsum, int G,
                           int tiles_n, int* __restrict__ ws) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int total = 0;
    int64_t prev = 0;
    for (int g = 0; g < G; ++g) {
      int64_t m = cumsum[g] - prev;
      prev = cumsum[g];
      ws[1 + g] = total;
      total += (int)((m + BM8 - 1) / BM8) * tiles_n;
    }
    ws[1 + G] = total;
    ws[0] = total;
  }
}

// BKN = false: B [G, N, K] (trans_b), staged K-contiguous like A.
// BKN = true:  B [G, K, N] as stored (dgrad straight from the weights): the
// B tile is a "reduction-slow" [64 k][256 n] tile (TStage64 / tr_issue).
// The k-to-lane map of the fragments is the same in both, so both feed the
// MFMAs identical operands in identical order.
template <bool BKN>
__global__ __launch_bounds__(THREADS8, 2) void k_group_gemm_nk256s(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
    bf16_t* __restrict__ C, const int64_t* __restrict__ cumsum, int G,
    int64_t N, int64_t K, int tiles_n, const int* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* sm = reinterpret_cast<bf16_t*>(smem);
  auto ta = [&](int buf) { return sm + buf * 32768; };          // 2 x 32 KiB
  auto tb = [&](int buf) { return sm + 16384 + buf * 32768; };  // 2 x 32 KiB

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;

  const int total_tiles = ws[0];
  const int X = blockIdx.x & 7;        // this block's XCD (dispatch affinity)
  const int slot = blockIdx.x >> 3;    // 0..31 within the XCD
  const int L = (total_tiles + 7) / 8; // contiguous tile range per XCD
  const int t_end = min((X + 1) * L, total_tiles);
  const int nk = (int)(K / BK64);

  for (int t = X * L + slot; t < t_end; t += 32) {
    // group lookup: largest g with ws[1+g] <= t
    int lo = 0, hi = G - 1;
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (ws[1 + mid] <= t) lo = mid;
      else hi = mid - 1;
    }
    const int gid = lo;
    const int local = t - ws[1 + gid];
    const int tiles_m_g = (ws[2 + gid] - ws[1 + gid]) / tiles_n;
    const int bm = local % tiles_m_g;   // bm-inner: consecutive t share bn
    const int bn = local / tiles_m_g;

    const int64_t row_start = (gid > 0) ? cumsum[gid - 1] : 0;
    const int64_t m_size = cumsum[gid] - row_start;
    const bf16_t* Ag = A + row_start * K;
    const bf16_t* Bg = B + (int64_t)gid * N * K;
    bf16_t* Cg = C + row_start * N;

    KStage64 sa, sb;
    TStage64 sbt;
    sa.init(Ag, K, [&](int r) -> int64_t {
      int64_t gm = (int64_t)bm * BM8 + r;
      return gm % m_size;
    }, tid);
    if constexpr (BKN) {
      sbt.init(Bg, N, [&](int c) -> int64_t {
        return ((int64_t)bn * BN8 + c) % N;
      }, tid);
    } else {
      sb.init(Bg, K, [&](int r) -> int64_t {
        int64_t gn = (int64_t)bn * BN8 + r;
        return gn % N;
      }, tid);
    }
    auto stage_b = [&](bf16_t* tile, int kt) {
      if constexpr (BKN) sbt.stage(tile, kt * BK64, [](int k) { return k; });
      else sb.stage(tile, (int64_t)kt * BK64);
    };
    int btr_off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) btr_off[j] = tr_lane_off(wc * 64 + j * 16, lane);

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    sa.stage(ta(0), 0);
    stage_b(tb(0), 0);
    if constexpr (BKN) VMCNT(0);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) {
        sa.stage(ta(cur ^ 1), (int64_t)(kt + 1) * BK64);
        stage_b(tb(cur ^ 1), kt + 1);
      }
      // fragments of one 32-k half; the MFMA clusters are the same for both
      // B layouts
      auto ks_step = [&](auto ks_c) {
        constexpr int ks = decltype(ks_c)::value;
        bf16frag af[4], bfr[4];
        TrFrag tf[4];
        const uint32_t b0 = lds_addr(tb(cur));
#pragma unroll
        for (int j = 0; j < 4; ++j) tr_issue<ks>(tf[j], b0 + btr_off[j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = frag_read64(ta(cur), wr * 128 + i * 16, ks, lane);
        tr_wait(tf);
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = tr_frag(tf[j]);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = frag_read64(ta(cur), wr * 128 + 64 + i * 16, ks, lane);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i + 4][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i + 4][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      };
      if constexpr (BKN) {
        ks_step(std::integral_constant<int, 0>{});
        ks_step(std::integral_constant<int, 1>{});
      } else {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16frag af[4], bfr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = frag_read64(tb(cur), wc * 64 + j * 16, ks, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = frag_read64(ta(cur), wr * 128 + i * 16, ks, lane);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = frag_read64(ta(cur), wr * 128 + 64 + i * 16, ks, lane);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i + 4][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i + 4][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
      }
      if constexpr (BKN) VMCNT(0);
      __syncthreads();
      cur ^= 1;
    }

    const int col_in = lane & 15;
    const int row_base_in = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          int64_t m = (int64_t)bm * BM8 + wr * 128 + (i & 3) * 16 + (i >> 2) * 64 +
                      row_base_in + rr;
          int64_t n = (int64_t)bn * BN8 + wc * 64 + j * 16 + col_in;
          if (m < m_size && n < N) Cg[m * N + n] = f2bf(acc[i][j][rr]);
        }
  }
}

}  // namespace

// lazily-allocated device workspace for the tile schedule (ws[0] = total,
// ws[1..G+1] = per-group tile prefix). Single compute stream per process;
// calls on one stream serialize, so one buffer suffices.
static int* vh_gg_sched_ws = nullptr;
static constexpr int VH_GG_SCHED_MAX_G = 4096;

static int vh_launch_nk256s(bool b_kn, const uint16_t* A, const uint16_t* B,
                            uint16_t* C, const int64_t* cumsum, int G,
                            int64_t N, int64_t K, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(K % BK64 == 0, "K %% 64 != 0");
  VH_CHECK(N % 16 == 0, "N %% 16 != 0");
  VH_CHECK(G <= VH_GG_SCHED_MAX_G, "G > %d", VH_GG_SCHED_MAX_G);
  if (vh_gg_sched_ws == nullptr) {
    VH_HIP(hipMalloc(&vh_gg_sched_ws, (VH_GG_SCHED_MAX_G + 2) * sizeof(int)));
  }
  int tiles_n = (int)((N + BN8 - 1) / BN8);
  hipLaunchKernelGGL(k_gg_sched, dim3(1), dim3(64), 0, s, cumsum, G, tiles_n,
                     vh_gg_sched_ws);
  VH_HIP(hipGetLastError());
  auto kern = b_kn ? k_group_gemm_nk256s<true> : k_group_gemm_nk256s<false>;
  hipLaunchKernelGGL(kern, dim3(256), dim3(THREADS8), 131072, s,
                     reinterpret_cast<const bf16_t*>(A),
                     reinterpret_cast<const bf16_t*>(B),
                     reinterpret_cast<bf16_t*>(C), cumsum, G, N, K, tiles_n,
                     vh_gg_sched_ws);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_group_gemm_nk256s_bf16(const uint16_t* A, const uint16_t* B,
                                         uint16_t* C, const int64_t* cumsum,
                                         int G, int64_t N, int64_t K,
                                         int64_t total_rows, void* stream) {
  (void)total_rows;
  return vh_launch_nk256s(false, A, B, C, cumsum, G, N, K, stream);
}

extern "C" int vh_group_gemm_nk256s_kn_bf16(const uint16_t* A, const uint16_t* B,
                                            uint16_t* C, const int64_t* cumsum,
                                            int G, int64_t N, int64_t K,
                                            int64_t total_rows, void* stream) {
  (void)total_rows;
  return vh_launch_nk256s(true, A, B, C, cumsum, G, N, K, stream);
}

// ============================================================================
// wgd256s: the direct wgrad. C[g] (M x N) = A_g^T @ B_g with A [rows, M] and
// B [rows, N] token-major exactly as autograd hands them over; group g owns
// rows [cumsum[g-1], cumsum[g]). The reduction index (the token row) is the
// slow one of BOTH operands, so both are staged as [64 k][256 out] tiles
// (TStage64) and read with transposing LDS reads: no transposed/padded
// copies, no temporaries, no helper launches.
//
// Same compute structure as k_group_gemm_nk256s under the same XCD-clustered
// persistent schedule: every group owns the same tiles_m x tiles_n output
// tiles (weight-shaped C), so the schedule needs no device prefix — block b
// (XCD b%8) walks the contiguous tile range [X*L, (X+1)*L) with stride 32,
// bm-inner, keeping a group's B k-slab hot in its XCD's L2.
//
// K range: ceil(count/64) tiles from the group's first row, whatever its
// alignment. In the last tile the rows at or past the group's end are loaded
// from the group's own last row (clamped: nothing is read outside the group)
// and then zeroed in LDS in BOTH operands, so they contribute exactly 0
// whatever the neighbouring rows hold (0 * NaN would be NaN). Each wave
// zeroes the rows it staged itself, after its own vmcnt(0) and before the
// barrier that publishes the tile — no extra barrier, wave-uniform branches.
// Partial m/n tiles wrap their columns (M, N are 16-multiples, so a 16-out
// segment never straddles the edge); the surplus is dropped at the store.
// ============================================================================

namespace {

__global__ __launch_bounds__(THREADS8, 2) void k_group_gemm_wgd256s(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
    bf16_t* __restrict__ C, const int64_t* __restrict__ cumsum, int G,
    int64_t M, int64_t N, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* sm = reinterpret_cast<bf16_t*>(smem);
  auto ta = [&](int buf) { return sm + buf * 32768; };
  auto tb = [&](int buf) { return sm + 16384 + buf * 32768; };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;

  const int tpg = tiles_m * tiles_n;
  const int total = G * tpg;
  const int X = blockIdx.x & 7;
  const int slot = blockIdx.x >> 3;
  const int L = (total + 7) / 8;
  const int t_end = min((X + 1) * L, total);

  for (int t = X * L + slot; t < t_end; t += 32) {
    const int gid = t / tpg;
    const int local = t - gid * tpg;
    const int bm = local % tiles_m;   // bm-inner: consecutive t share bn
    const int bn = local / tiles_m;

    const int64_t row_start = (gid > 0) ? cumsum[gid - 1] : 0;
    const int cnt = (int)(cumsum[gid] - row_start);
    bf16_t* Cg = C + (int64_t)gid * M * N;

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    if (cnt > 0) {
      TStage64 sa, sb;
      sa.init(A + row_start * M, M, [&](int c) -> int64_t {
        return ((int64_t)bm * BM8 + c) % M;
      }, tid);
      sb.init(B + row_start * N, N, [&](int c) -> int64_t {
        return ((int64_t)bn * BN8 + c) % N;
      }, tid);
      // clamp to the group's last row: in bounds for every k of every tile
      auto row_of = [&](int k) { return min(k, cnt - 1); };

      const int nk = (cnt + BK64 - 1) / BK64;
      const int rem = cnt - (nk - 1) * BK64;  // valid k-rows of the last tile
      // stage k-tile kt; the group's last tile gets its tail rows zeroed
      auto stage = [&](int buf, int kt) {
        sa.stage(ta(buf), kt * BK64, row_of);
        sb.stage(tb(buf), kt * BK64, row_of);
      };
      auto zero_tail = [&](int buf) {
        VMCNT(0);
        sa.zero_tail(ta(buf), rem, lane);
        sb.zero_tail(tb(buf), rem, lane);
      };

      int atr_off[8], btr_off[4];
#pragma unroll
      for (int i = 0; i < 8; ++i) atr_off[i] = tr_lane_off(wr * 128 + i * 16, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) btr_off[j] = tr_lane_off(wc * 64 + j * 16, lane);

      stage(0, 0);
      if (nk == 1 && rem < BK64) zero_tail(0);
      VMCNT(0);
      __syncthreads();
      int cur = 0;
      for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
        const uint32_t a0 = lds_addr(ta(cur)), b0 = lds_addr(tb(cur));
        auto ks_step = [&](auto ks_c) {
          constexpr int ks = decltype(ks_c)::value;
          TrFrag tb4[4], ta4[4], ta4h[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) tr_issue<ks>(tb4[j], b0 + btr_off[j]);
#pragma unroll
          for (int i = 0; i < 4; ++i) tr_issue<ks>(ta4[i], a0 + atr_off[i]);
          tr_wait(tb4);
          tr_wait(ta4);
          // the second 64 rows' fragments land under the first MFMA cluster
#pragma unroll
          for (int i = 0; i < 4; ++i) tr_issue<ks>(ta4h[i], a0 + atr_off[4 + i]);
          bf16frag af[4], bfr[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) bfr[j] = tr_frag(tb4[j]);
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = tr_frag(ta4[i]);
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
          __builtin_amdgcn_s_setprio(0);
          tr_wait(ta4h);
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = tr_frag(ta4h[i]);
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[i + 4][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i + 4][j], 0, 0, 0);
          __builtin_amdgcn_s_setprio(0);
        };
        ks_step(std::integral_constant<int, 0>{});
        ks_step(std::integral_constant<int, 1>{});
        if (kt + 2 == nk && rem < BK64) zero_tail(cur ^ 1);
        VMCNT(0);
        __syncthreads();
        cur ^= 1;
      }
    }

    const int col_in = lane & 15;
    const int row_base_in = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          int64_t m = (int64_t)bm * BM8 + wr * 128 + (i & 3) * 16 + (i >> 2) * 64 +
                      row_base_in + rr;
          int64_t n = (int64_t)bn * BN8 + wc * 64 + j * 16 + col_in;
          if (m < M && n < N) Cg[m * N + n] = f2bf(acc[i][j][rr]);
        }
  }
}

}  // namespace

extern "C" int vh_group_gemm_wgd_bf16(const uint16_t* A, const uint16_t* B,
                                      uint16_t* C, const int64_t* cumsum, int G,
                                      int64_t M, int64_t N, int64_t total_rows,
                                      void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  (void)total_rows;
  VH_CHECK(M % 16 == 0 && N % 16 == 0, "M/N %% 16 != 0");
  VH_CHECK(G >= 1, "G < 1");
  int tiles_m = (int)((M + BM8 - 1) / BM8);
  int tiles_n = (int)((N + BN8 - 1) / BN8);
  hipLaunchKernelGGL(k_group_gemm_wgd256s, dim3(256), dim3(THREADS8), 131072, s,
                     reinterpret_cast<const bf16_t*>(A),
                     reinterpret_cast<const bf16_t*>(B),
                     reinterpret_cast<bf16_t*>(C), cumsum, G, M, N, tiles_m,
                     tiles_n);
  VH_HIP(hipGetLastError());
  return 0;
}
