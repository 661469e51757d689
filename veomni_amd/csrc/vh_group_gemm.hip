// Grouped GEMM on gfx950 MFMA (bf16 in, fp32 accumulate).
//
// Semantics anchors (restated, not copied):
//   group_gemm_same_nk — ref kernel/group_gemm.py:66-234: G per-expert GEMMs,
//     rows of A/C partitioned by an inclusive cumsum; shared N,K; out-of-range
//     row loads wrapped modulo the group's row count and stores masked.
//   group_gemm_same_mn — ref kernel/group_gemm.py:252-397: per-group wgrad
//     C[g] = A_g^T @ B_g with per-group K = row count; zero-count groups are
//     zero-filled.
//
// MI355X design (guide cdna_hip_programming.md §5):
//   * v_mfma_f32_16x16x32_bf16; 128x128x64 tile; 256 threads = 4 waves in a
//     2x2 wave grid, 64x64 per wave (4x4 fragments, f32x4 accumulators).
//   * K-contiguous operands staged via global_load_lds width 16 into a
//     lane-linear LDS image; the T2 XOR swizzle ((row&7)<<4) is applied on the
//     per-lane SOURCE address and on the ds_read address (rule 21).
//   * Per-lane stage addresses (incl. the reference's modulo row wrap) are
//     hoisted OUT of the K-loop — the loop only adds k0 (int64 div/mod per
//     stage was VALU-bound).
//   * K-strided operands (dgrad's B, wgrad's A and B) staged through
//     registers: per-lane column loads are coalesced ACROSS lanes (consecutive
//     out-dim per lane), written as 16-B ds_writes into the transposed image.
//   * 2-phase double buffer: stage tile t+1, compute tile t, one
//     __syncthreads per K-step (guide T3 "minimum 2-phase" recipe).

#include "vh_common.h"
#include "../../include/veomni_hip.h"  // the 256x256 entries dispatched to

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int THREADS = 256;

using bf16frag = __attribute__((ext_vector_type(8))) __bf16;

__device__ __forceinline__ void glds16(const bf16_t* g, bf16_t* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)g,
      (__attribute__((address_space(3))) unsigned int*)l, 16, 0, 0);
}

// byte-offset XOR swizzle within a 128-B row (8 x 16-B slots).
// ds_read_b128 lane groups read 16 CONSECUTIVE tile rows at one col range;
// the bank row is 256 B, so tile rows alternate half-banks (+0 / +32 dwords).
// slot = ((row>>1) ^ (row>>3)) & 7:
//   * reads: over 16 consecutive rows each parity class hits 8 DISTINCT
//     slots -> all 16 (slot, half-bank) pairs distinct -> conflict-free;
//   * transposed-staging writes (ds_write_b64, rows 8m+j at one k-col):
//     slots over m = 0..7 are the distinct set m ^ 4(m&1) -> only the m+8
//     repeat collides -> 2-way (vs 8-way with a (row>>1)-only slot map).
__device__ __forceinline__ int swz(int row, int colb) {
  return colb ^ ((((row >> 1) ^ (row >> 3)) & 7) << 4);
}

// Per-lane staging context for a [128][BK] K-contiguous tile via glds:
// 4 pre-swizzled per-lane source pointers (advance by k each stage) + the
// wave-uniform LDS byte bases.
struct KStage {
  const bf16_t* src[4];
  int lds_base[4];

  template <typename RowFn>
  __device__ __forceinline__ void init(const bf16_t* s, int64_t ld_elems,
                                       RowFn row_of, int tid) {
    const int lane = tid & 63;
    const int wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int base = i * 4096 + wave * 1024;
      int o = base + lane * 16;
      int row = o >> 7;
      int colb = o & 127;
      src[i] = s + row_of(row) * ld_elems + (swz(row, colb) >> 1);
      lds_base[i] = base;
    }
  }

  __device__ __forceinline__ void stage(bf16_t* lds_tile, int64_t k0) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(src[i] + k0, lds_tile + (lds_base[i] >> 1));
  }
};

// Transposed register staging: element (out, k) read from src[k*ld + out].
// Thread t owns a [4k][8out] sub-block: o0 = (t&15)*8, ks0 = (t>>4)*4.
// Loads: 4 x 16-B bf16x8 (8 consecutive `out` at one k) — lanes 0..15 read
// 256 contiguous bytes (fully coalesced). Writes: 8 x ds_write_b64 (4
// consecutive k at one out — k IS contiguous in the [out][k] image).
// CLAMP guards ragged k (zero fill); ragged out takes a per-element path.
template <bool CLAMP>
struct TStage {
  const bf16_t* base;   // src + out0 + o0 (this thread's out chunk)
  int64_t ld;
  int64_t kmax;
  bool out_ok;          // whole 8-out chunk in range
  int64_t gout_left;    // number of valid outs in this chunk (ragged tiles)
  int o0, ks0;

  __device__ __forceinline__ void init(const bf16_t* s, int64_t ld_elems,
                                       int64_t kmax_, int out0, int out_max,
                                       int tid) {
    o0 = (tid & 15) * 8;
    ks0 = (tid >> 4) * 4;
    int64_t gout = (int64_t)out0 + o0;
    gout_left = out_max - gout;  // may be <= 0
    out_ok = gout_left >= 8;
    base = s + gout;
    ld = ld_elems;
    kmax = kmax_;
  }

  // T14 split (guide G15): issue the global loads EARLY (before the MFMA
  // phase that covers their latency), write to LDS LATE (after it).
  __device__ __forceinline__ void load(bf16x8 (&v)[4], int64_t k0) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int64_t k = k0 + ks0 + i;
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

  __device__ __forceinline__ void flush(bf16_t* lds_tile, const bf16x8 (&v)[4]) const {
    const int colb = ks0 * 2;  // 8-B aligned; swz flips only bits 4-6
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int row = o0 + j;
      ushort2 lo = {v[0].v[j], v[1].v[j]};
      ushort2 hi = {v[2].v[j], v[3].v[j]};
      uint2 pack = {*reinterpret_cast<const uint32_t*>(&lo),
                    *reinterpret_cast<const uint32_t*>(&hi)};
      *reinterpret_cast<uint2*>(&lds_tile[(row * 128 + swz(row, colb)) >> 1]) = pack;
    }
  }

  __device__ __forceinline__ void stage(bf16_t* lds_tile, int64_t k0) const {
    bf16x8 v[4];
    load(v, k0);
    flush(lds_tile, v);
  }
};

// read one 16x32 MFMA A/B fragment from the swizzled [row][64] bf16 image
__device__ __forceinline__ bf16frag frag_read(const bf16_t* lds_tile, int row0,
                                              int ks, int lane) {
  int row = row0 + (lane & 15);
  int colb = (ks * 32 + ((lane >> 4) << 3)) * 2;
  int off_b = row * 128 + swz(row, colb);
  return *reinterpret_cast<const bf16frag*>(
      reinterpret_cast<const char*>(lds_tile) + off_b);
}

__device__ __forceinline__ float maybe_act(float x, int ACT) {
  return ACT == 1 ? siluf(x) : x;
}

// shared MFMA inner step over both K-sub-tiles of one staged K-step
#define VH_MFMA_STEP(TA_, TB_)                                                 \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                           \
    bf16frag af[4], bfr[4];                                                    \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                              \
        af[i] = frag_read(TA_, wr * 64 + i * 16, ks, lane);                    \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                              \
        bfr[j] = frag_read(TB_, wc * 64 + j * 16, ks, lane);                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                              \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                          \
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(               \
                af[i], bfr[j], acc[i][j], 0, 0, 0);                            \
  }

// ---------------------------------------------------------------- same_nk
template <bool TRANS_B, bool ACCUM, int ACT>
__global__ __launch_bounds__(THREADS, 2) void k_group_gemm_nk(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
    bf16_t* __restrict__ C, const int64_t* __restrict__ cumsum, int G,
    int64_t N, int64_t K, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* sm = reinterpret_cast<bf16_t*>(smem);
  auto ta = [&](int buf) { return sm + buf * 16384; };
  auto tb = [&](int buf) { return sm + 8192 + buf * 16384; };

  const int gid = blockIdx.y;
  const int64_t row_start = (gid > 0) ? cumsum[gid - 1] : 0;
  const int64_t row_end = cumsum[gid];
  const int64_t m_size = row_end - row_start;
  const int bm = blockIdx.x / tiles_n;
  const int bn = blockIdx.x % tiles_n;
  if ((int64_t)bm * BM >= m_size) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;  // 2x2 wave grid

  const bf16_t* Ag = A + row_start * K;
  const bf16_t* Bg = B + (int64_t)gid * N * K;
  bf16_t* Cg = C + row_start * N;

  KStage sa;
  sa.init(Ag, K, [&](int r) -> int64_t {
    int64_t gm = (int64_t)bm * BM + r;
    return gm % m_size;  // wrap like the reference; stores are masked
  }, tid);

  KStage sb_k;          // TRANS_B path
  TStage<false> sb_t;   // !TRANS_B path (K % 64 == 0 asserted by the wrapper)
  if (TRANS_B) {
    sb_k.init(Bg, K, [&](int r) -> int64_t {
      int64_t gn = (int64_t)bn * BN + r;
      return gn % N;
    }, tid);
  } else {
    sb_t.init(Bg, N, K, bn * BN, (int)N, tid);
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int nk = (int)(K / BK);
  sa.stage(ta(0), 0);
  if (TRANS_B) sb_k.stage(tb(0), 0);
  else sb_t.stage(tb(0), 0);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < nk; ++t) {
    bf16x8 vb[4];
    const bool more = t + 1 < nk;
    const int64_t k1 = (int64_t)(t + 1) * BK;
    if (more) {
      sa.stage(ta(cur ^ 1), k1);           // glds: async fire-and-forget
      if (TRANS_B) sb_k.stage(tb(cur ^ 1), k1);
      else sb_t.load(vb, k1);              // T14: issue loads before MFMA
    }
    {
      const bf16_t* TA = ta(cur);
      const bf16_t* TB = tb(cur);
      VH_MFMA_STEP(TA, TB)
    }
    if (more && !TRANS_B) sb_t.flush(tb(cur ^ 1), vb);  // write late
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: C row = (lane>>4)*4 + reg, col = lane&15 within each 16x16 frag
  const int col_in = lane & 15;
  const int row_base_in = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        int64_t m = (int64_t)bm * BM + wr * 64 + i * 16 + row_base_in + rr;
        int64_t n = (int64_t)bn * BN + wc * 64 + j * 16 + col_in;
        if (m < m_size && n < N) {
          float v = acc[i][j][rr];
          if (ACCUM) v += bf2f(Cg[m * N + n]);
          Cg[m * N + n] = f2bf(maybe_act(v, ACT));
        }
      }
    }
  }
}

// ---------------------------------------------------------------- same_mn
// C[g, M, N] = A_g^T @ B_g ; A [rows, M], B [rows, N]; k = group row count.
__global__ __launch_bounds__(THREADS, 2) void k_group_gemm_mn(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
    bf16_t* __restrict__ C, const int64_t* __restrict__ cumsum, int G,
    int64_t M, int64_t N, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* sm = reinterpret_cast<bf16_t*>(smem);
  auto ta = [&](int buf) { return sm + buf * 16384; };
  auto tb = [&](int buf) { return sm + 8192 + buf * 16384; };

  const int gid = blockIdx.y;
  const int64_t row_start = (gid > 0) ? cumsum[gid - 1] : 0;
  const int64_t row_end = cumsum[gid];
  const int64_t kcount = row_end - row_start;
  const int bm = blockIdx.x / tiles_n;
  const int bn = blockIdx.x % tiles_n;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  bf16_t* Cg = C + (int64_t)gid * M * N;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  if (kcount > 0) {
    const bf16_t* Ag = A + row_start * M;
    const bf16_t* Bg = B + row_start * N;
    const int nk = (int)((kcount + BK - 1) / BK);
    TStage<true> sta, stb;
    sta.init(Ag, M, kcount, bm * BM, (int)M, tid);
    stb.init(Bg, N, kcount, bn * BN, (int)N, tid);
    sta.stage(ta(0), 0);
    stb.stage(tb(0), 0);
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < nk; ++t) {
      bf16x8 va[4], vb[4];
      const bool more = t + 1 < nk;
      const int64_t k1 = (int64_t)(t + 1) * BK;
      if (more) {  // T14 split: loads before the MFMA phase, writes after
        sta.load(va, k1);
        stb.load(vb, k1);
      }
      {
        const bf16_t* TA = ta(cur);
        const bf16_t* TB = tb(cur);
        VH_MFMA_STEP(TA, TB)
      }
      if (more) {
        sta.flush(ta(cur ^ 1), va);
        stb.flush(tb(cur ^ 1), vb);
      }
      __syncthreads();
      cur ^= 1;
    }
  }

  const int col_in = lane & 15;
  const int row_base_in = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        int64_t m = (int64_t)bm * BM + wr * 64 + i * 16 + row_base_in + rr;
        int64_t n = (int64_t)bn * BN + wc * 64 + j * 16 + col_in;
        if (m < M && n < N) Cg[m * N + n] = f2bf(acc[i][j][rr]);
      }
}

}  // namespace

extern "C" int vh_group_gemm_nk_bf16(const uint16_t* A, const uint16_t* B,
                                     uint16_t* C, const int64_t* cumsum, int G,
                                     int64_t N, int64_t K, int64_t total_rows,
                                     int trans_b, int accumulate,
                                     int activation, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // Per-shape dispatch from measured data (profiles/r01_groupgemm_microbench,
  // profiles/gg_direct_operands_ab.md):
  //   large, either B layout -> nk256s (256-sq double-buffered glds, persistent
  //                      XCD-clustered schedule; B [G,K,N] is staged as it is
  //                      stored and read with transposing LDS reads)
  //   !trans_b wide, K % 64 == 32 or G > 4096 -> nk8 (glds A + transposed B ring)
  //   everything else -> the 128x128 2-phase kernel
  if (!accumulate && activation == 0 && K % 64 == 0 && N >= 256 &&
      total_rows >= (int64_t)G * 256 && G <= 4096) {
    // nk256s: device-built tile schedule + XCD-clustered persistent blocks
    // (L2 reuse; no skew-sized null-block grid) — see vh_group_gemm8.hip
    if (trans_b)
      return vh_group_gemm_nk256s_bf16(A, B, C, cumsum, G, N, K, total_rows,
                                       stream);
    return vh_group_gemm_nk256s_kn_bf16(A, B, C, cumsum, G, N, K, total_rows,
                                        stream);
  }
  if (!accumulate && activation == 0 && !trans_b && K % 32 == 0 && K >= 1024 &&
      N >= 1024 && total_rows >= 16 * G * 16) {
    return vh_group_gemm_nk8_bf16(A, B, C, cumsum, G, N, K, total_rows, 0,
                                  stream);
  }
  VH_CHECK(K % BK == 0, "K %% 64 != 0 (K=%lld)", (long long)K);
  VH_CHECK(N % 16 == 0, "N %% 16 != 0 (N=%lld)", (long long)N);
  VH_CHECK(G >= 1, "G < 1");
  int tiles_m = (int)((total_rows + BM - 1) / BM);
  if (tiles_m < 1) tiles_m = 1;
  int tiles_n = (int)((N + BN - 1) / BN);
  dim3 grid(tiles_m * tiles_n, G);
  size_t lds = 65536;

#define VH_DISPATCH(TB, AC, ACT_)                                              \
  hipLaunchKernelGGL((k_group_gemm_nk<TB, AC, ACT_>), grid, dim3(THREADS),     \
                     lds, s, reinterpret_cast<const bf16_t*>(A),               \
                     reinterpret_cast<const bf16_t*>(B),                       \
                     reinterpret_cast<bf16_t*>(C), cumsum, G, N, K, tiles_m,   \
                     tiles_n)

  if (trans_b) {
    if (accumulate) VH_DISPATCH(true, true, 0);
    else if (activation == 1) VH_DISPATCH(true, false, 1);
    else VH_DISPATCH(true, false, 0);
  } else {
    if (accumulate) VH_DISPATCH(false, true, 0);
    else if (activation == 1) VH_DISPATCH(false, false, 1);
    else VH_DISPATCH(false, false, 0);
  }
#undef VH_DISPATCH
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_group_gemm_mn_bf16(const uint16_t* A, const uint16_t* B,
                                     uint16_t* C, const int64_t* cumsum, int G,
                                     int64_t M, int64_t N, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(M % 16 == 0 && N % 16 == 0, "M/N %% 16 != 0");
  if (M >= 1024 && N >= 1024) {  // measured: mn8 wins only at wide M,N
    return vh_group_gemm_mn8_bf16(A, B, C, cumsum, G, M, N, stream);
  }
  int tiles_m = (int)((M + BM - 1) / BM);
  int tiles_n = (int)((N + BN - 1) / BN);
  dim3 grid(tiles_m * tiles_n, G);
  hipLaunchKernelGGL(k_group_gemm_mn, grid, dim3(THREADS), 65536, s,
                     reinterpret_cast<const bf16_t*>(A),
                     reinterpret_cast<const bf16_t*>(B),
                     reinterpret_cast<bf16_t*>(C), cumsum, G, M, N, tiles_m,
                     tiles_n);
  VH_HIP(hipGetLastError());
  return 0;
}
