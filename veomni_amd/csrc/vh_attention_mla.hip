// Flash attention forward/backward for gfx950, multi-head latent attention
// as it is trained (DeepSeek-V2/V3, Kimi-K2): q/k heads 192 wide (128 "nope"
// + 64 "rope"), v heads 128 wide. bf16, causal, GQA, packed-varlen /
// key-window bounds, no sinks. Contract: include/veomni_hip.h, "MLA flash
// pair"; numerics are those of the D = 128 and D = 64 pairs. V is never
// padded: P.V, dP = dO V^T and dV run 128 wide, only QK^T and dQ / dK are 192.
//
// What changes at 192 / 128. Per 32-key subtile QK^T is 12 MFMA
// (mfma_f32_32x32x16_bf16) and P.V is 8, against 8 + 8 at D = 128, for the
// same 16 exponents per lane; the backward kernels run 40 (dK/dV) and 32 (dQ)
// MFMA per 16 exponents. All three kernels are therefore bound by the matrix
// pipe, and the design spends registers, not occupancy, on keeping it fed:
// every kernel is a 4-wave block with a 512-register budget per lane (256
// VGPRs + AGPRs), one wave per SIMD. A wave holds its whole accumulator set
// (forward 64, dQ 96, dK/dV 160 registers) plus the tile-invariant operand
// fragments, so a subtile is unbroken MFMA chains around one softmax / dS
// section, and the 20..40 : 16 MFMA-to-exponent ratio, not a second wave,
// keeps the pipe busy. With 8 waves and 256 registers the forward spilled
// 100-330 B per lane to scratch, and dK/dV with its K / V fragments in
// registers spilled too; neither form is kept.
//   * forward: on interior kv tiles both QK^T chains of the tile are issued
//     before the first softmax, so the second chain runs under the exponent
//     stream of the first; tiles on the diagonal or a bound go subtile by
//     subtile behind wave-uniform live / cut tests.
//   * dK/dV: each wave accumulates its 32 kv rows x (192 + 128) columns; the
//     strip's K and V sit in LDS as one tile set for the whole kernel and are
//     read as B-fragments with the same conflict-free b128 reads as the
//     Q / dO A-fragments.
//   * dQ: one image set per kv tile serves the b128 A-fragment reads of
//     S^T = K Q^T and dP^T = V dO^T and the tr16 B-fragment reads of
//     dQ += dS^T K.
//
// LDS images. A 192-wide row (384 B) is 1.5 bank lines, so every Q / K tile
// is staged as two images and each keeps the map, and the bank argument, of
// the file it comes from:
//   N image (d 0..127; also V and dO): 256-B rows, the L16 latin square of
//     vh_attention.hip:
//       off(row, p) = row*256 + ((row&15) ^ P(p))*16,  p = d>>3,
//       P(p) = ((p&3)<<2) | (p>>2).
//     One row is one bank line of 16 slots. b128 reads (16 consecutive rows,
//     one p): slot = (row&15) ^ const, a bijection of the 16 rows -> 16
//     distinct slots. tr16 reads (rows R..R+3, R%4 == 0, chunks p = 4*dblk+0..3
//     in 8-byte halves): P(p) = (p&3)<<2 | dblk, so the four chunks differ in
//     slot bits 2..3 and the four rows in bits 0..1 -> 16 distinct slots.
//     Filled by global_load_lds: a wave's 1 KiB window is 4 rows, lane i
//     lands on (row = 4*win + i/16, slot i%16) and fetches chunk
//     P(slot ^ (row&15)) (P is an involution).
//   R image (d 128..191): 128-B rows, the map of vh_attention64.hip:
//       off(row, p) = row*128 + (p ^ g(row))*16,  p = (d-128)>>3,
//       g(row) = ((y&1)<<2) | (y>>1),  y = (row>>1)&7;
//     two rows per bank line, conflict-free for the same two read kinds by
//     the argument in that file's header. A window is 8 rows, lane i lands on
//     (row = 8*win + i/8, slot i%8) and fetches chunk (i%8) ^ g(row).
//   The 12 k-steps of QK^T walk the 8 chunk pairs of the N image and the 4 of
//   the R image; the 6 column blocks of dQ / dK are 4 tr16 blocks of the N
//   image and 2 of the R image. Adding a multiple of 16 rows leaves both maps
//   unchanged, so subtiles and 16-row chunks are immediate offsets.
//
// Kernels, LDS, waves, occupancy (registers: profiles/attn_mla_microbench.md):
//   (grids are ceil(S / block); S % 256 != 0 launches the TAIL instantiations:
//   same tiling, reads of rows >= S redirected to row S-1, stores guarded)
//   k_mla_fwd      grid (S/128, B*Hq), 4 waves x 32 q rows, Q fragments (48
//                  VGPRs) in registers, 64-row kv tiles: K 16 + 8 KiB, V
//                  16 KiB, double buffered: 80 KiB. One block = 4 waves per
//                  CU (more than 256 registers per lane).
//   k_mla_bwd_dkv  grid (S/64, B*Hkv), 4 waves = 2 kv slices x 2 q subtiles of
//                  a 64-row q tile, loops the GQA head group; K / V strip
//                  40 KiB, then Q 16 + 8 KiB, dO 16 KiB and 768 B of row
//                  scalars, double buffered: 121.5 KiB. One block per CU.
//   k_mla_bwd_dq   grid (S/128, B*Hq), 4 waves x 32 q rows, Q / dO fragments
//                  (80 VGPRs) and the 128x192 fp32 dQ (96) in registers,
//                  64-row kv tiles as the forward, double buffered: 80 KiB.
//                  One block per CU (324-331 registers per lane).
//   vh_attn_mla_bwd_pre_bf16 is the D = 128 preprocess (O and dO are 128
//   wide, head-major, any row count): it calls vh_attn_bwd_pre_bf16.
// Nothing is accumulated in global memory and there are no atomics: dQ, dK
// and dV are written once and are bit-identical from run to run.
//
// Masking contract (include/veomni_hip.h): lo[q] first visible key of row q,
// hi[j] one past the last row that sees key j, both monotone, indexed by row
// within the sequence.

#include "vh_common.h"

#include <type_traits>

extern "C" int vh_attn_bwd_pre_bf16(const uint16_t* dO, const uint16_t* O,
                                    const float* LSE, float* delta,
                                    float* lse2, int64_t rows, void* stream);

namespace {

constexpr int DQK = 192;   // q / k head dim: 128 nope + 64 rope
constexpr int DN = 128;    // nope part; also the v head dim
constexpr int DV = 128;
constexpr int QB = 128;    // forward, dQ: q rows per block
constexpr int WQ = 32;     // q rows per wave
constexpr int KB = 64;     // kv rows per tile (forward, dQ); q rows (dK/dV)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float DEFER_THR = 8.0f;  // defer-max threshold (exp2 domain)

// one staged tile set of 64 rows: N image, R image, 128-wide image
constexpr int IMG_N = 0;
constexpr int IMG_R = 16384;
constexpr int IMG_V = 24576;
constexpr int TILE_BYTES = 40960;
constexpr int DKV_STAGE = TILE_BYTES + 768;   // + lse2 / delta / lo of 64 rows
constexpr int DKV_LDS = TILE_BYTES + 2 * DKV_STAGE;  // K / V strip + 2 stages

using bf16frag = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4t = __attribute__((ext_vector_type(4))) __bf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef __attribute__((address_space(3))) const char* lds_cptr;

__device__ __forceinline__ void glds16a(const bf16_t* g, void* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)g,
      (__attribute__((address_space(3))) unsigned int*)l, 16, 0, 0);
}
// one dword per lane: lane i lands at l + i
__device__ __forceinline__ void glds4(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)g,
      (__attribute__((address_space(3))) unsigned int*)l, 4, 0, 0);
}

// N image: P(p) and the byte offset of 16-B chunk p of `row`
__device__ __forceinline__ int nperm(int p) { return ((p & 3) << 2) | (p >> 2); }
__device__ __forceinline__ int nimg_off(int row, int p) {
  return row * 256 + (((row & 15) ^ nperm(p)) << 4);
}
// R image: g(row) and the byte offset of 16-B chunk p of `row`
__device__ __forceinline__ int rperm(int row) {
  const int y = (row >> 1) & 7;
  return ((y & 1) << 2) | (y >> 1);
}
__device__ __forceinline__ int rimg_off(int row, int p) {
  return row * 128 + ((p ^ rperm(row)) << 4);
}

// Element offsets, from the tile's first row, of what lane `lane` fetches for
// 1 KiB window `win` of an image; `rs` is the row stride of the global tensor
// in elements. Source rows past rmax (the tile-local index of row S-1; 63 on
// every full tile) fetch row rmax; the chunk permutation stays the destination
// row's, so the image keeps its layout.
__device__ __forceinline__ uint32_t nimg_src(int win, int lane, int rs, int rmax) {
  const int row = win * 4 + (lane >> 4);
  const int pg = nperm((lane & 15) ^ (row & 15));
  return (uint32_t)(min(row, rmax) * rs + pg * 8);
}
__device__ __forceinline__ uint32_t rimg_src(int win, int lane, int rmax) {
  const int row = win * 8 + (lane >> 3);
  return (uint32_t)(min(row, rmax) * DQK + DN + (((lane & 7) ^ rperm(row)) << 3));
}

// Stage one 64-row tile set with NW waves: a 192-wide tensor `a` (rows at a0)
// into the N and R images and a 128-wide tensor `b` into the third image.
template <int NW>
__device__ __forceinline__ void stage_tiles(const bf16_t* a0, const bf16_t* b0,
                                            char* sb, int wave, int lane,
                                            int rmax) {
  constexpr int PN = 16 / NW, PR = 8 / NW;
#pragma unroll
  for (int u = 0; u < PN; ++u) {
    const int win = wave * PN + u;
    glds16a(a0 + nimg_src(win, lane, DQK, rmax), sb + IMG_N + win * 1024);
    glds16a(b0 + nimg_src(win, lane, DV, rmax), sb + IMG_V + win * 1024);
  }
#pragma unroll
  for (int u = 0; u < PR; ++u) {
    const int win = wave * PR + u;
    glds16a(a0 + rimg_src(win, lane, rmax), sb + IMG_R + win * 1024);
  }
}

__device__ __forceinline__ uint32_t swap32_u(uint32_t v, int half) {
  auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return half ? (uint32_t)r[0] : (uint32_t)r[1];
}
__device__ __forceinline__ float xor32h(float v, int half) {
  return __builtin_bit_cast(float, swap32_u(__builtin_bit_cast(uint32_t, v), half));
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) float f32x2t;
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2t;
  return __builtin_bit_cast(uint32_t,
                            __builtin_convertvector(f32x2t{lo, hi}, bf16x2t));
}
// one v_max3_f32 (see vh_attention.hip: maximumnum needs no canonicalise)
__device__ __forceinline__ float max3f(float a, float b, float c) {
  return __builtin_fmaximum_numf(__builtin_fmaximum_numf(a, b), c);
}
// partner-quad exchange of packed bf16 pairs into an MFMA A fragment (see
// vh_attention.hip)
__device__ __forceinline__ bf16frag quad_exchange(uint32_t a0, uint32_t a1,
                                                  uint32_t c0, uint32_t c1) {
  auto r0 = __builtin_amdgcn_permlane32_swap(a0, c0, false, false);
  auto r1 = __builtin_amdgcn_permlane32_swap(a1, c1, false, false);
  uint4 u{(uint32_t)r0[0], (uint32_t)r1[0], (uint32_t)r0[1], (uint32_t)r1[1]};
  return __builtin_bit_cast(bf16frag, u);
}
__device__ __forceinline__ bf16frag lds_frag(lds_cptr p) {
  return *(__attribute__((address_space(3))) const bf16frag*)p;
}
// B fragment of 8 k-rows: two 4-row hardware-transpose reads
__device__ __forceinline__ bf16frag lds_tr_frag(lds_cptr a0, lds_cptr a1) {
  typedef __attribute__((address_space(3))) bf16x4t as3b4;
  bf16x4t r0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((as3b4*)a0);
  bf16x4t r1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((as3b4*)a1);
  return __builtin_shufflevector(r0, r1, 0, 1, 2, 3, 4, 5, 6, 7);
}
// Per-lane byte offsets of the tr16 reads of 32-column block `dblk` of an
// image (N: dblk 0..3, R: dblk 0..1): the lane supplies (row = half*8 + m/4
// [+4], 8-byte slot c_r) of a 16-row chunk and receives column
// dblk*32 + lane%32 of its 8 rows.
template <bool NIMG>
__device__ __forceinline__ void tr_offsets(int lane, int dblk, int& a0, int& a1) {
  const int m_ = lane & 15;
  const int row = (lane >> 5) * 8 + (m_ >> 2);
  const int c_r = dblk * 8 + ((lane >> 4) & 1) * 4 + (m_ & 3);
  if (NIMG) {
    a0 = nimg_off(row, c_r >> 1) + (c_r & 1) * 8;
    a1 = nimg_off(row + 4, c_r >> 1) + (c_r & 1) * 8;
  } else {
    a0 = rimg_off(row, c_r >> 1) + (c_r & 1) * 8;
    a1 = rimg_off(row + 4, c_r >> 1) + (c_r & 1) * 8;
  }
}
// Byte offset, inside a tile set, of the b128 A-fragment of k-step c (0..11)
// for image row `row`: steps 0..7 walk the N image, 8..11 the R image. The
// 32-row subtile adds sub*8192 (N) or sub*4096 (R).
__device__ __forceinline__ int afrag_off(int row, int c, int half) {
  return c < 8 ? IMG_N + nimg_off(row, c * 2 + half)
               : IMG_R + rimg_off(row, (c - 8) * 2 + half);
}
__device__ __forceinline__ int sub_step(int c) { return c < 8 ? 8192 : 4096; }

// ============================================================================
// Forward
// ============================================================================
// TAIL (S % 256 != 0, every kernel of this file): the grid is ceil(S / block)
// and a lane whose row is >= S reads, and is masked as, row S-1; its results
// are not stored. The kv loop ends at the tile that holds row S-1, whose
// staging sources are clamped the same way: its keys >= S are copies of key
// S-1 and lie above the diagonal of every row, so the masked body hides them.
template <bool DOC, bool TAIL>
__global__ __launch_bounds__(256, 1) void k_mla_fwd(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, bf16_t* __restrict__ O,
    float* __restrict__ LSE, const int* __restrict__ lo, int B, int Hq,
    int Hkv, int64_t S, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int qb = blockIdx.x;
  const int bh = blockIdx.y;           // b * Hq + hq
  const int b = bh / Hq;
  const int hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int col = lane & 31;

  const bf16_t* Qb = Q + (((int64_t)b * Hq + hq) * S) * DQK;
  const bf16_t* Kb = K + (((int64_t)b * Hkv + hkv) * S) * DQK;
  const bf16_t* Vb = V + (((int64_t)b * Hkv + hkv) * S) * DV;
  bf16_t* Ob = O + (((int64_t)b * Hq + hq) * S) * DV;
  float* Lb = LSE + ((int64_t)b * Hq + hq) * S;

  const int w0r = qb * QB + wave * WQ;         // the wave's first q row
  const int sm1 = (int)S - 1;
  // rows the wave and the lane compute (TAIL: clamped to S-1)
  const int w0 = TAIL ? min(w0r, sm1) : w0r;
  const int w1 = TAIL ? min(w0r + WQ - 1, sm1) : w0r + WQ - 1;
  const int q_row = TAIL ? min(w0r + col, sm1) : w0r + col;
  const float scale2 = scale * LOG2E;

  // bounds: this lane's, and the wave's smallest / largest (lo is monotone)
  int lo_l = 0, lo_w0 = 0, lo_w1 = 0, t0 = 0;
  if (DOC) {
    lo_l = lo[q_row];
    lo_w0 = __builtin_amdgcn_readfirstlane(lo[w0]);
    lo_w1 = __builtin_amdgcn_readfirstlane(lo[w1]);
    t0 = lo[qb * QB] / KB;
  }

  // Q fragments (tile-invariant): chunk c = Q[q_row][c*16 + half*8 .. +8)
  bf16frag qreg[12];
#pragma unroll
  for (int c = 0; c < 12; ++c)
    qreg[c] = *reinterpret_cast<const bf16frag*>(
        Qb + (int64_t)q_row * DQK + c * 16 + half * 8);

  const int t_tail = sm1 / KB;
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
    const int rmax = (TAIL && t == t_tail) ? sm1 - t_tail * KB : KB - 1;
    stage_tiles<4>(Kb + (int64_t)t * KB * DQK, Vb + (int64_t)t * KB * DV,
                   smem + buf * TILE_BYTES, wave, lane, rmax);
  };

  f32x16 oacc[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) oacc[d] = f32x16{};
  float m_run = -1e30f;
  float l_run = 0.f;

  // per-lane LDS read offsets inside a tile set
  int kaddr[12], vaddr[4][2];
#pragma unroll
  for (int c = 0; c < 12; ++c) kaddr[c] = afrag_off(col, c, half);
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    tr_offsets<true>(lane, d, vaddr[d][0], vaddr[d][1]);
    vaddr[d][0] += IMG_V;
    vaddr[d][1] += IMG_V;
  }

  // inclusive; TAIL: no tile past the one that holds row S-1
  const int t_max = TAIL ? min((qb * QB + QB - 1) / KB, t_tail)
                         : (qb * QB + QB - 1) / KB;
  stage(t0, 0);
  __syncthreads();

  int cur = 0;
  for (int t = t0; t <= t_max; ++t) {
    if (t < t_max) stage(t + 1, cur ^ 1);
    const int k0t = t * KB;
    lds_cptr tb = (lds_cptr)(smem + cur * TILE_BYTES);

    // S^T = K Q^T of one 32-key subtile: lane owns q column col, 16 scores
    auto qk = [&](const int sub) __attribute__((always_inline)) {
      f32x16 sacc = f32x16{};
#pragma unroll
      for (int c = 0; c < 12; ++c)
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            lds_frag(tb + kaddr[c] + sub * sub_step(c)), qreg[c], sacc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      return sacc;
    };

    // online softmax + PV of one subtile. MASK is a compile-time tag: the
    // masked body applies the causal and lower-bound select per score.
    auto softmax_pv = [&](auto mask_tag, const int sub, const f32x16 sacc)
                          __attribute__((always_inline)) {
      constexpr bool MASK = decltype(mask_tag)::value;
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) p[r] = sacc[r] * scale2;
      if (MASK) {
        const int kv_lim = q_row - k0t - sub * 32 - 4 * half;
        const int lo_lim = DOC ? lo_l - k0t - sub * 32 - 4 * half : 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int idx = (r & 3) + 8 * (r >> 2);
          if (idx > kv_lim) p[r] = -INFINITY;
          if (DOC && idx < lo_lim) p[r] = -INFINITY;
        }
      }
      float m5[5];
#pragma unroll
      for (int i = 0; i < 5; ++i)
        m5[i] = max3f(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
      float mt = max3f(max3f(m5[0], m5[1], m5[2]), max3f(m5[3], m5[4], p[15]),
                       -INFINITY);
      mt = max3f(mt, xor32h(mt, half), -INFINITY);

      // defer-max: rescale only when some lane's max moved past the threshold
      const bool need = mt > m_run + DEFER_THR;
      if (__builtin_amdgcn_ballot_w64(need) != 0ull) {
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qr = (r & 3) + 8 * (r >> 2) + 4 * half;
          const float a_r = __shfl(alpha, qr, 32);
#pragma unroll
          for (int d = 0; d < 4; ++d) oacc[d][r] *= a_r;
        }
      }

      // raw v_exp_f32 (flushes below 2^-126: under half an ulp of any row sum
      // >= 1 and of every bf16 P entry)
      float s8[8];
      uint32_t pk[8];
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const float e0 = __builtin_amdgcn_exp2f(p[r] - m_run);
        const float e1 = __builtin_amdgcn_exp2f(p[r + 1] - m_run);
        s8[r >> 1] = e0 + e1;
        pk[r >> 1] = pack_bf16x2(e0, e1);
      }
      float psum = ((s8[0] + s8[1]) + (s8[2] + s8[3])) +
                   ((s8[4] + s8[5]) + (s8[6] + s8[7]));
      psum += xor32h(psum, half);
      l_run += psum;

      // O += P^T V: A = packed P, B = V^T through the tr16 reads
#pragma unroll
      for (int mch = 0; mch < 2; ++mch) {
        const bf16frag pa = quad_exchange(pk[4 * mch], pk[4 * mch + 1],
                                          pk[4 * mch + 2], pk[4 * mch + 3]);
        const int off = (sub * 32 + mch * 16) * 256;
#pragma unroll
        for (int d = 0; d < 4; ++d)
          oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa, lds_tr_frag(tb + vaddr[d][0] + off, tb + vaddr[d][1] + off),
              oacc[d], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    };

    // wave-uniform: the whole tile lies below the wave's diagonal and above
    // every lower bound of its rows
    const bool interior = (k0t + KB - 1 <= w0) && (!DOC || k0t >= lo_w1);
    if (interior) {
      // both QK^T chains go to the matrix pipe before the first softmax
      const f32x16 s_a = qk(0);
      const f32x16 s_b = qk(1);
      softmax_pv(std::false_type{}, 0, s_a);
      softmax_pv(std::false_type{}, 1, s_b);
    } else {
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int k0 = k0t + sub * 32;
        // skip: every key past every row of the wave, or before every bound
        const bool live = (k0 <= w1) && (!DOC || k0 + 32 > lo_w0);
        if (live) {
          const bool cut = (k0 + 31 > w0) || (DOC && k0 < lo_w1);
          const f32x16 s = qk(sub);
          if (cut) softmax_pv(std::true_type{}, sub, s);
          else softmax_pv(std::false_type{}, sub, s);
        }
      }
    }

    __syncthreads();
    cur ^= 1;
  }

  // epilogue: O / l, bf16 store, LSE
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * half;
    const float inv = 1.0f / __shfl(l_run, qr, 32);
    const int64_t qg = (int64_t)w0r + qr;
    if (!TAIL || qg < S) {
#pragma unroll
      for (int d = 0; d < 4; ++d)
        Ob[qg * DV + d * 32 + col] = f2bf(oacc[d][r] * inv);
    }
  }
  if (half == 0 && (!TAIL || w0r + col < S))
    Lb[w0r + col] = 0.6931471805599453f * (m_run + __log2f(l_run));
}

// ============================================================================
// dK/dV, GQA-folded: a block owns a 64-row kv strip of one KV head and loops
// the query-head group and the 64-row q tiles from the diagonal to hi.
// 4 waves = (kv slice of 32 rows) x (q subtile of 32 rows): a wave runs one
// 32x32 quadrant per tile and keeps dK (32x192) and dV (32x128) of its slice
// in registers; the two q subtiles are summed through LDS at the end. The
// strip's K / V tile set is staged once at the start of LDS. Stage
// (DKV_STAGE): Q as N + R images, dO as the 128-wide image, lse2 / delta / lo
// of the 64 rows.
// ============================================================================
// TAIL: strip rows >= S read K / V row S-1 and are not stored; the q tile
// that holds row S-1 is staged with clamped sources (Q, dO, lse2, delta, lo)
// and its rows >= S get P = dS = 0 through a row < S term in the masked body,
// which every quadrant that reaches S takes.
template <bool DOC, bool TAIL>
__global__ __launch_bounds__(256, 1) void k_mla_bwd_dkv(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
    const float* __restrict__ delta, const float* __restrict__ lse2,
    bf16_t* __restrict__ dK, bf16_t* __restrict__ dV,
    const int* __restrict__ lo, const int* __restrict__ hi, int B, int Hq,
    int Hkv, int64_t S, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);   // epilogue reuse, <= 48 KiB

  const int kvb = blockIdx.x;          // 64-row kv strip
  const int bkh = blockIdx.y;          // b * Hkv + hkv
  const int b = bkh / Hkv;
  const int hkv = bkh % Hkv;
  const int rep = Hq / Hkv;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kvslice = wave & 1;
  const int qsub = wave >> 1;
  const int half = lane >> 5;
  const int col = lane & 31;

  const int kv0 = kvb * 64;
  const int kvs0 = kv0 + kvslice * 32;          // the wave's first kv row
  const int64_t kvrow0 = ((int64_t)b * Hkv + hkv) * S;
  const int sm1 = (int)S - 1;

  // the strip's K / V tile set, staged once at smem + 0 (TAIL: rows >= S are
  // copies of row S-1); the q stages follow it
  stage_tiles<4>(K + (kvrow0 + kv0) * DQK, V + (kvrow0 + kv0) * DV, smem, wave,
                 lane, TAIL ? min(sm1 - kv0, 63) : 63);
  char* stages = smem + TILE_BYTES;
  lds_cptr kvt = (lds_cptr)smem;

  f32x16 dv_acc[4], dk_acc[6];
#pragma unroll
  for (int d = 0; d < 4; ++d) dv_acc[d] = f32x16{};
#pragma unroll
  for (int d = 0; d < 6; ++d) dk_acc[d] = f32x16{};

  const float scale2 = scale * LOG2E;
  const int qt0 = kvb;                 // 64-row q tiles
  int qtn = (int)((S + (TAIL ? 63 : 0)) / 64);
  int hi_w = 0;
  if (DOC) {
    const int j_b = TAIL ? min(kv0 + 63, sm1) : kv0 + 63;
    const int j_w = TAIL ? min(kvs0 + 31, sm1) : kvs0 + 31;
    qtn = (hi[j_b] + 63) / 64;                                  // block end
    hi_w = __builtin_amdgcn_readfirstlane(hi[j_w]);             // wave end
  }
  const int ntiles = qtn - qt0;
  const int itn = rep * ntiles;

  const int qt_tail = sm1 / 64;
  // stage (head g, q tile) number `it` into buffer `buf`
  auto stage = [&](int it, int buf) __attribute__((always_inline)) {
    const int g = it / ntiles;
    const int qt = qt0 + (it - g * ntiles);
    const int64_t rowbase = ((int64_t)b * Hq + hkv * rep + g) * S + (int64_t)qt * 64;
    char* sb = stages + buf * DKV_STAGE;
    const int rmax = (TAIL && qt == qt_tail) ? sm1 - qt_tail * 64 : 63;
    stage_tiles<4>(Q + rowbase * DQK, dO + rowbase * DV, sb, wave, lane, rmax);
    float* st = reinterpret_cast<float*>(sb + TILE_BYTES);
    const uint32_t s0 = (uint32_t)min(lane, rmax);
    if (wave == 0) glds4(lse2 + rowbase + s0, st);
    else if (wave == 1) glds4(delta + rowbase + s0, st + 64);
    else if (DOC && wave == 2) glds4(lo + qt * 64 + s0, st + 128);
  };

  // per-lane image offsets of the wave's quadrant (image rows qsub*32 ..)
  const int rl0 = qsub * 32;
  int aoff[12], trn[4][2], trr[2][2];
#pragma unroll
  for (int c = 0; c < 12; ++c) aoff[c] = afrag_off(col, c, half);
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    tr_offsets<true>(lane, d, trn[d][0], trn[d][1]);
    trn[d][0] += rl0 * 256;
    trn[d][1] += rl0 * 256;
  }
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    tr_offsets<false>(lane, d, trr[d][0], trr[d][1]);
    trr[d][0] += IMG_R + rl0 * 128;
    trr[d][1] += IMG_R + rl0 * 128;
  }

  if (itn > 0) stage(0, 0);
  __syncthreads();
  int cur = 0;
  for (int it = 0; it < itn; ++it) {
    if (it + 1 < itn) stage(it + 1, cur ^ 1);
    const int qt = qt0 + it % ntiles;
    lds_cptr tb = (lds_cptr)(stages + cur * DKV_STAGE);
    const float* stat = reinterpret_cast<const float*>(stages + cur * DKV_STAGE + TILE_BYTES);

    const int q0 = qt * 64 + rl0;
    const bool live = (q0 + 31 >= kvs0) && (!DOC || q0 < hi_w) &&
                      (!TAIL || q0 <= sm1);
    if (live) {
      bool cut = q0 < kvs0 + 31;
      if (TAIL) cut = cut || (q0 + 31 > sm1);
      if (DOC)
        cut = cut || __builtin_amdgcn_readfirstlane(
                         reinterpret_cast<const int*>(stat)[128 + rl0 + 31]) > kvs0;

      // S = Q K^T and dP = dO V^T of the quadrant: lane owns kv column col
      f32x16 s2 = f32x16{}, dp2 = f32x16{};
#pragma unroll
      for (int c = 0; c < 12; ++c)
        s2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            lds_frag(tb + aoff[c] + qsub * sub_step(c)),
            lds_frag(kvt + aoff[c] + kvslice * sub_step(c)), s2, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < 8; ++c)
        dp2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            lds_frag(tb + IMG_V + aoff[c] + qsub * 8192),
            lds_frag(kvt + IMG_V + aoff[c] + kvslice * 8192), dp2, 0, 0, 0);

      // P and dS packed to bf16 pairs; score r belongs to q row
      // (r&3) + 8*(r>>2) + 4*half of the quadrant: four runs of four rows,
      // one b128 broadcast read per run and quantity
      uint32_t pk2[8], dg2[8];
      auto pds_pack = [&](auto mask_tag) __attribute__((always_inline)) {
        constexpr bool MASK = decltype(mask_tag)::value;
        // kv row kvs0 + col is masked for q row q0 + idx + 4*half when it lies
        // past that row or before the row's lower bound
        const int c_lim = (kvs0 + col) - q0 - 4 * half;
        const int kv_abs = kvs0 + col;
        // TAIL: q row q0 + idx + 4*half is >= S
        const int r_lim = (int)S - q0 - 4 * half;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int qr4 = rl0 + 8 * jj + 4 * half;
          const float4 l4 = *reinterpret_cast<const float4*>(stat + qr4);
          const float4 d4 = *reinterpret_cast<const float4*>(stat + 64 + qr4);
          const float lse_q[4] = {l4.x, l4.y, l4.z, l4.w};
          const float del_q[4] = {d4.x, d4.y, d4.z, d4.w};
          int lo_q[4] = {0, 0, 0, 0};
          if (MASK && DOC) {
            const int4 s4 = *reinterpret_cast<const int4*>(
                reinterpret_cast<const int*>(stat) + 128 + qr4);
            lo_q[0] = s4.x, lo_q[1] = s4.y, lo_q[2] = s4.z, lo_q[3] = s4.w;
          }
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2) {
            float pv[2], gv[2];
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
              const int i = 2 * h2 + rr;
              const int r2 = 4 * jj + i;
              float pp = __builtin_amdgcn_exp2f(
                  __builtin_fmaf(s2[r2], scale2, -lse_q[i]));
              if (MASK) {
                bool masked = (i + 8 * jj) < c_lim;
                if (DOC) masked = masked || (kv_abs < lo_q[i]);
                if (TAIL) masked = masked || ((i + 8 * jj) >= r_lim);
                pp = masked ? 0.f : pp;
              }
              pv[rr] = pp;
              gv[rr] = pp * (dp2[r2] - del_q[i]) * scale;
            }
            pk2[2 * jj + h2] = pack_bf16x2(pv[0], pv[1]);
            dg2[2 * jj + h2] = pack_bf16x2(gv[0], gv[1]);
          }
        }
      };
      __builtin_amdgcn_sched_barrier(0);
      if (cut) pds_pack(std::true_type{});
      else pds_pack(std::false_type{});
      __builtin_amdgcn_sched_barrier(0);

      // dV += P^T dO, dK += dS^T Q: B fragments by tr16 reads of the images
#pragma unroll
      for (int mch = 0; mch < 2; ++mch) {
        const bf16frag pa = quad_exchange(pk2[4 * mch], pk2[4 * mch + 1],
                                          pk2[4 * mch + 2], pk2[4 * mch + 3]);
        const bf16frag da = quad_exchange(dg2[4 * mch], dg2[4 * mch + 1],
                                          dg2[4 * mch + 2], dg2[4 * mch + 3]);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          dv_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa, lds_tr_frag(tb + IMG_V + mch * 4096 + trn[d][0],
                              tb + IMG_V + mch * 4096 + trn[d][1]),
              dv_acc[d], 0, 0, 0);
          dk_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              da, lds_tr_frag(tb + IMG_N + mch * 4096 + trn[d][0],
                              tb + IMG_N + mch * 4096 + trn[d][1]),
              dk_acc[d], 0, 0, 0);
        }
#pragma unroll
        for (int d = 0; d < 2; ++d)
          dk_acc[4 + d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              da, lds_tr_frag(tb + mch * 2048 + trr[d][0],
                              tb + mch * 2048 + trr[d][1]),
              dk_acc[4 + d], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // sum the two q subtiles per kv slice through LDS (red: [slice][lane][ND*16]
  // floats, over the images: every wave is past the last barrier) and store.
  // Spelled out per accumulator: a pointer into the accumulator arrays would
  // send them to scratch.
#define VH_MLA_DKV_COMBINE(ACC, DST, ND, RS)                                  \
  {                                                                           \
    float* slot = red + (kvslice * 64 + lane) * (ND * 16);                    \
    if (qsub == 1) {                                                          \
      _Pragma("unroll") for (int d = 0; d < ND; ++d)                          \
          _Pragma("unroll") for (int r = 0; r < 16; r += 4)                   \
              *reinterpret_cast<float4*>(slot + d * 16 + r) = float4{         \
                  ACC[d][r], ACC[d][r + 1], ACC[d][r + 2], ACC[d][r + 3]};    \
    }                                                                         \
    __syncthreads();                                                          \
    if (qsub == 0) {                                                          \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                        \
        const int kvr = (r & 3) + 8 * (r >> 2) + 4 * half;                    \
        const int64_t o = (kvrow0 + kvs0 + kvr) * RS + col;                   \
        if (!TAIL || kvs0 + kvr < S) {                                        \
          _Pragma("unroll") for (int d = 0; d < ND; ++d)                      \
              DST[o + d * 32] = f2bf(ACC[d][r] + slot[d * 16 + r]);           \
        }                                                                     \
      }                                                                       \
    }                                                                         \
    __syncthreads();                                                          \
  }
  VH_MLA_DKV_COMBINE(dv_acc, dV, 4, DV)
  VH_MLA_DKV_COMBINE(dk_acc, dK, 6, DQK)
#undef VH_MLA_DKV_COMBINE
}

// ============================================================================
// dQ: a block owns 128 q rows (wave = 32-row slice) of one query head; the
// wave's Q / dO fragments, lse2 and delta stay in registers, dQ (32x192 fp32
// per wave) too, stored once as bf16. 64-row kv tiles (K as N + R images, V
// as the 128-wide image) are double buffered, one barrier per tile; the K
// images feed both S^T = K Q^T (b128 A-fragments) and dQ += dS^T K (tr16
// B-fragments). Each 32-key subtile has its own wave-uniform live / cut test.
// ============================================================================
// TAIL: as the forward: rows >= S compute row S-1 and are not stored, the kv
// loop ends at the tile that holds row S-1, staged with clamped sources.
template <bool DOC, bool TAIL>
__global__ __launch_bounds__(256, 1) void k_mla_bwd_dq(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
    const float* __restrict__ delta, const float* __restrict__ lse2,
    bf16_t* __restrict__ dQ, const int* __restrict__ lo, int B, int Hq,
    int Hkv, int64_t S, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int qb = blockIdx.x;           // q block of 128 rows
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int col = lane & 31;

  const int64_t qbase = ((int64_t)b * Hq + hq) * S;
  const bf16_t* Kb = K + (((int64_t)b * Hkv + hkv) * S) * DQK;
  const bf16_t* Vb = V + (((int64_t)b * Hkv + hkv) * S) * DV;

  const int q0b = qb * 128;
  const int w0r = q0b + wave * 32;     // the wave's first q row
  const int sm1 = (int)S - 1;
  // rows the wave and the lane compute (TAIL: clamped to S-1)
  const int w0 = TAIL ? min(w0r, sm1) : w0r;
  const int w1 = TAIL ? min(w0r + 31, sm1) : w0r + 31;
  const int q_l = TAIL ? min(w0r + col, sm1) : w0r + col;

  bf16frag qrow[12], dorow[8];
#pragma unroll
  for (int c = 0; c < 12; ++c)
    qrow[c] = *reinterpret_cast<const bf16frag*>(
        Q + (qbase + q_l) * DQK + c * 16 + half * 8);
#pragma unroll
  for (int c = 0; c < 8; ++c)
    dorow[c] = *reinterpret_cast<const bf16frag*>(
        dO + (qbase + q_l) * DV + c * 16 + half * 8);
  const float lse_l = lse2[qbase + q_l];
  const float del_l = delta[qbase + q_l];
  const float scale2 = scale * LOG2E;

  int lo_l = 0, lo_w0 = 0, lo_w1 = 0, kvt_begin = 0;
  if (DOC) {
    lo_l = lo[q_l];
    lo_w0 = __builtin_amdgcn_readfirstlane(lo[w0]);
    lo_w1 = __builtin_amdgcn_readfirstlane(lo[w1]);
    kvt_begin = lo[q0b] / KB;
  }

  f32x16 dq2[6];
#pragma unroll
  for (int d = 0; d < 6; ++d) dq2[d] = f32x16{};

  const int kt_tail = sm1 / KB;
  auto stage = [&](int kvt, int buf) __attribute__((always_inline)) {
    const int rmax = (TAIL && kvt == kt_tail) ? sm1 - kt_tail * KB : KB - 1;
    stage_tiles<4>(Kb + (int64_t)kvt * KB * DQK, Vb + (int64_t)kvt * KB * DV,
                   smem + buf * TILE_BYTES, wave, lane, rmax);
  };
  int aoff[12], trn[4][2], trr[2][2];
#pragma unroll
  for (int c = 0; c < 12; ++c) aoff[c] = afrag_off(col, c, half);
#pragma unroll
  for (int d = 0; d < 4; ++d) tr_offsets<true>(lane, d, trn[d][0], trn[d][1]);
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    tr_offsets<false>(lane, d, trr[d][0], trr[d][1]);
    trr[d][0] += IMG_R;
    trr[d][1] += IMG_R;
  }

  // exclusive; TAIL: no tile past the one that holds row S-1
  const int kvtn = TAIL ? min((q0b + 128) / KB, kt_tail + 1) : (q0b + 128) / KB;
  stage(kvt_begin, 0);
  __syncthreads();
  int cur = 0;
  for (int kvt = kvt_begin; kvt < kvtn; ++kvt) {
    if (kvt + 1 < kvtn) stage(kvt + 1, cur ^ 1);
    lds_cptr tb = (lds_cptr)(smem + cur * TILE_BYTES);

#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int k0 = kvt * KB + sub * 32;
      const bool live = (k0 <= w1) && (!DOC || k0 + 32 > lo_w0);
      if (!live) continue;
      const bool cut = (k0 + 31 > w0) || (DOC && k0 < lo_w1);

      // S^T = K Q^T, dP^T = V dO^T: lane owns q column col, 16 kv rows
      f32x16 s1 = f32x16{}, dp1 = f32x16{};
#pragma unroll
      for (int c = 0; c < 12; ++c)
        s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            lds_frag(tb + aoff[c] + sub * sub_step(c)), qrow[c], s1, 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 8; ++c)
        dp1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            lds_frag(tb + (IMG_V - IMG_N) + aoff[c] + sub * 8192), dorow[c],
            dp1, 0, 0, 0);

      uint32_t dg1[8];
      auto ds_pack = [&](auto mask_tag) __attribute__((always_inline)) {
        constexpr bool MASK = decltype(mask_tag)::value;
        const int c_lim = q_l - k0 - 4 * half;
        const int lo_lim = DOC ? lo_l - k0 - 4 * half : 0;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          float g[2];
#pragma unroll
          for (int rr = 0; rr < 2; ++rr) {
            const int r2 = r + rr;
            float pp = __builtin_amdgcn_exp2f(
                __builtin_fmaf(s1[r2], scale2, -lse_l));
            if (MASK) {
              const int idx = (r2 & 3) + 8 * (r2 >> 2);
              bool masked = idx > c_lim;
              if (DOC) masked = masked || (idx < lo_lim);
              pp = masked ? 0.f : pp;
            }
            g[rr] = pp * (dp1[r2] - del_l) * scale;
          }
          dg1[r >> 1] = pack_bf16x2(g[0], g[1]);
        }
      };
      if (cut) ds_pack(std::true_type{});
      else ds_pack(std::false_type{});

      // dQ += dS^T K: B fragments by tr16 reads of the K images
#pragma unroll
      for (int mch = 0; mch < 2; ++mch) {
        const bf16frag da = quad_exchange(dg1[4 * mch], dg1[4 * mch + 1],
                                          dg1[4 * mch + 2], dg1[4 * mch + 3]);
        const int rows = sub * 32 + mch * 16;
#pragma unroll
        for (int d = 0; d < 4; ++d)
          dq2[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              da, lds_tr_frag(tb + rows * 256 + trn[d][0],
                              tb + rows * 256 + trn[d][1]),
              dq2[d], 0, 0, 0);
#pragma unroll
        for (int d = 0; d < 2; ++d)
          dq2[4 + d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              da, lds_tr_frag(tb + rows * 128 + trr[d][0],
                              tb + rows * 128 + trr[d][1]),
              dq2[4 + d], 0, 0, 0);
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // single-contributor store
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * half;
    const int64_t o = (qbase + w0r + qr) * DQK + col;
    if (!TAIL || w0r + qr < S) {
#pragma unroll
      for (int d = 0; d < 6; ++d) dQ[o + d * 32] = f2bf(dq2[d][r]);
    }
  }
}

// shared argument checks
int check_common(int B, int Hq, int Hkv, int64_t S, float scale) {
  VH_CHECK(B > 0 && Hq > 0 && Hkv > 0, "B, Hq, Hkv must be > 0");
  VH_CHECK(S > 0, "S must be > 0");
  VH_CHECK(S * DQK < (1ll << 31), "S too large for 32-bit tile offsets");
  VH_CHECK((int64_t)B * Hq < 65536, "B * Hq must be < 65536 (grid y)");
  VH_CHECK(Hq % Hkv == 0, "Hq %% Hkv != 0");
  VH_CHECK(scale > 0, "scale must be > 0 (got %g)", (double)scale);
  return 0;
}

}  // namespace

extern "C" int vh_attn_mla_fwd_bf16(const uint16_t* Q, const uint16_t* K,
                                    const uint16_t* V, uint16_t* O, float* LSE,
                                    int B, int Hq, int Hkv, int64_t S,
                                    float scale, const int32_t* lo,
                                    void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = check_common(B, Hq, Hkv, S, scale)) return rc;
  dim3 grid((uint32_t)((S + QB - 1) / QB), (uint32_t)(B * Hq));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 2 * TILE_BYTES, s, Q, K, V, O,
                       LSE, lo, B, Hq, Hkv, S, scale);
  };
  if (S % 256 == 0) {
    if (lo) launch(k_mla_fwd<true, false>);
    else launch(k_mla_fwd<false, false>);
  } else {
    if (lo) launch(k_mla_fwd<true, true>);
    else launch(k_mla_fwd<false, true>);
  }
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_attn_mla_bwd_pre_bf16(const uint16_t* dO, const uint16_t* O,
                                        const float* LSE, float* delta,
                                        float* lse2, int B, int Hq, int64_t S,
                                        void* stream) {
  VH_CHECK(S > 0, "S must be > 0");
  VH_CHECK(B > 0 && Hq > 0, "B, Hq must be > 0");
  // O and dO are [B,Hq,S,128] head-major: the D = 128 preprocess as it is
  return vh_attn_bwd_pre_bf16(dO, O, LSE, delta, lse2, (int64_t)B * Hq * S,
                              stream);
}

extern "C" int vh_attn_mla_bwd2_bf16(const uint16_t* Q, const uint16_t* K,
                                     const uint16_t* V, const uint16_t* dO,
                                     const float* delta, const float* lse2,
                                     uint16_t* dQ, uint16_t* dK, uint16_t* dV,
                                     int B, int Hq, int Hkv, int64_t S,
                                     float scale, const int32_t* lo,
                                     const int32_t* hi, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = check_common(B, Hq, Hkv, S, scale)) return rc;
  VH_CHECK((lo == nullptr) == (hi == nullptr), "lo/hi must be passed together");
  dim3 grid_kv((uint32_t)((S + 63) / 64), (uint32_t)(B * Hkv));
  dim3 grid_q((uint32_t)((S + 127) / 128), (uint32_t)(B * Hq));
  auto launch_dkv = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid_kv, dim3(256), DKV_LDS, s, Q, K, V, dO,
                       delta, lse2, dK, dV, lo, hi, B, Hq, Hkv, S, scale);
  };
  auto launch_dq = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid_q, dim3(256), 2 * TILE_BYTES, s, Q, K, V, dO,
                       delta, lse2, dQ, lo, B, Hq, Hkv, S, scale);
  };
  const bool tail = S % 256 != 0;
  if (tail) {
    if (lo) launch_dkv(k_mla_bwd_dkv<true, true>);
    else launch_dkv(k_mla_bwd_dkv<false, true>);
  } else {
    if (lo) launch_dkv(k_mla_bwd_dkv<true, false>);
    else launch_dkv(k_mla_bwd_dkv<false, false>);
  }
  VH_HIP(hipGetLastError());
  if (tail) {
    if (lo) launch_dq(k_mla_bwd_dq<true, true>);
    else launch_dq(k_mla_bwd_dq<false, true>);
  } else {
    if (lo) launch_dq(k_mla_bwd_dq<true, false>);
    else launch_dq(k_mla_bwd_dq<false, false>);
  }
  VH_HIP(hipGetLastError());
  return 0;
}
