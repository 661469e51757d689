// Flash attention forward/backward for gfx950, head_dim 64 (bf16, causal, GQA,
// packed-varlen / key-window bounds, attention sinks). The D = 128 pair lives
// in vh_attention.hip; this file shares its contract (include/veomni_hip.h)
// and its numerics, not its layouts.
//
// What changes at D = 64. Per 32-key subtile QK^T and PV are 4 MFMA
// (mfma_f32_32x32x16_bf16) each instead of 8, while the softmax VALU stream
// (16 scores per lane: scale, max tree, v_exp_f32, pack, exchange) is the
// same, so all three kernels are bound by the VALU / transcendental stream
// and the design spends the freed registers on keeping the matrix pipe fed
// underneath it:
//   * forward: on interior kv tiles (no diagonal, no bound) the QK^T chain of
//     subtile i+1 is issued before the softmax of subtile i (two score
//     accumulators live: 32 VGPRs, paid for by Q 8 -> 4 and O 64 -> 32
//     registers), so the matrix pipe runs under the exponent stream. Tiles
//     that touch the diagonal or a bound run subtile by subtile instead, each
//     behind a wave-uniform live test, with the masked body only where the
//     subtile itself is cut.
//   * dK/dV: the block's K and V strip fragments are kept in registers for
//     the whole kernel (32 VGPRs) instead of LDS; LDS holds only the Q / dO
//     images, double buffered, one barrier per 128-row q tile.
//   * dQ: one K image serves both the b128 A-fragment reads of S = K Q^T and
//     the tr16 B-fragment reads of dQ += dS^T K (the D = 128 kernel stages K
//     twice), 64-row kv tiles, double buffered.
//
// LDS image (all tiles, every kernel): rows are 128 bytes = 8 chunks of 16 B.
//   off(row, p) = row*128 + (p ^ g(row))*16,  p = d>>3,
//   g(row) = ((y&1)<<2) | (y>>1),  y = (row>>1) & 7.
// Two rows share one 256-byte bank line, so the bank slot of (row, p) is
// (row&1)*8 + (p ^ g(row)).  b128 reads (16 consecutive rows, one p): y runs
// over 8 values and g is a bijection of them, row&1 gives the 9th..16th ->
// 16 distinct slots.  tr16 reads (4 consecutive rows R..R+3, R%4 == 0, four
// chunks p = 4*dblk + 0..3): g's low bits are the same for the four rows, its
// bit 2 is (row>>1)&1, so the two rows of one parity land in the two different
// aligned groups of four slots -> 16 distinct slots.  One map, conflict-free
// for both, filled by global_load_lds straight into LDS: a wave's 1 KiB
// window covers 8 rows, lane i lands on (row = 8*win + i/8, slot i%8) and
// fetches chunk (i%8) ^ g(row) of that row. No staging registers, no ds_write.
//
// Kernels, LDS, waves, occupancy (registers: profiles/attn_d64_microbench.md):
//   (grids are ceil(S / block); S % 256 != 0 launches the TAIL instantiations:
//   same tiling, reads of rows >= S redirected to row S-1, stores guarded)
//   k_attn64_fwd      grid (S/256, B*Hq), 8 waves x 32 q rows, 128-row kv
//                     tiles, K and V 16 KiB each, double buffered: 64 KiB.
//                     LDS would admit 2 blocks per CU; the two live score
//                     accumulators put the kernel at 168-206 VGPRs, so it runs
//                     one block = 8 waves per CU (2 per SIMD), as the D = 128
//                     forward does. Capped at 128 VGPRs it spills.
//   k_attn64_bwd_dkv  grid (S/64, B*Hkv), 4 waves = 2 kv slices x 2 q halves
//                     of a 128-row q tile, loops the GQA head group; Q and dO
//                     images 16 KiB each + 1.5 KiB row scalars, double
//                     buffered: 67 KiB, 2 blocks = 8 waves per CU.
//   k_attn64_bwd_dq   grid (S/128, B*Hq), 4 waves x 32 q rows, 64-row kv
//                     tiles, K and V 8 KiB each, double buffered: 32 KiB,
//                     140 VGPRs: 3 blocks = 12 waves per CU.
//   k_attn64_bwd_pre  delta, lse2 and the per-block dsinks partials;
//   k_attn64_dsinks   sums the partials in a fixed order.
// Nothing is accumulated in global memory and there are no atomics: dQ, dK
// and dV are written once, dsinks is bit-identical from run to run.
//
// Masking contract (include/veomni_hip.h, "Sliding-window attention and
// attention sinks"): lo[q] first visible key of row q, hi[j] one past the
// last row that sees key j, both monotone, indexed by row within the
// sequence. Sinks: the online softmax starts from m = sinks[hq]*log2e, l = 1;
// LSE includes the sink and is all the backward needs.

#include "vh_common.h"

#include <type_traits>

namespace {

constexpr int DH = 64;     // head dim
constexpr int QB = 256;    // forward: q rows per block
constexpr int WQ = 32;     // q rows per wave
constexpr int KB = 128;    // forward: kv rows per tile
constexpr float LOG2E = 1.4426950408889634f;
constexpr float DEFER_THR = 8.0f;  // defer-max threshold (exp2 domain)

using bf16frag = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4t = __attribute__((ext_vector_type(4))) __bf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef __attribute__((address_space(3))) const char* lds_cptr;

__device__ __forceinline__ void glds16a(const bf16_t* g, bf16_t* l) {
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

// 128-B rows: the slot permutation g(row) of the file header
__device__ __forceinline__ int rperm(int row) {
  const int y = (row >> 1) & 7;
  return ((y & 1) << 2) | (y >> 1);
}
// byte offset of 16-B chunk p of `row` in an image
__device__ __forceinline__ int img_off(int row, int p) {
  return row * 128 + ((p ^ rperm(row)) << 4);
}
// element offset, from the tile's first row, of what lane `lane` fetches for
// the 1 KiB window `win` (rows 8*win .. 8*win+7) of an image
__device__ __forceinline__ uint32_t img_src(int win, int lane) {
  const int row = win * 8 + (lane >> 3);
  return (uint32_t)(row * DH + (((lane & 7) ^ rperm(row)) << 3));
}

// img_src for the tile that holds row S-1: rows past `rmax` (the tile-local
// index of row S-1) fetch row rmax instead; the chunk permutation stays the
// destination row's, so the image keeps its layout
__device__ __forceinline__ uint32_t img_src_tail(int win, int lane, int rmax) {
  const int row = win * 8 + (lane >> 3);
  return (uint32_t)(min(row, rmax) * DH + (((lane & 7) ^ rperm(row)) << 3));
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
// per-lane byte offsets of the tr16 reads of d block `dblk` (32 columns): the
// lane supplies (row = half*8 + m/4 [+4], 8-byte slot c_r) of a 16-row chunk
// and receives column dblk*32 + lane%32 of its 8 rows
__device__ __forceinline__ void tr_offsets(int lane, int dblk, int& a0, int& a1) {
  const int m_ = lane & 15;
  const int row = (lane >> 5) * 8 + (m_ >> 2);
  const int c_r = dblk * 8 + ((lane >> 4) & 1) * 4 + (m_ & 3);
  a0 = img_off(row, c_r >> 1) + (c_r & 1) * 8;
  a1 = img_off(row + 4, c_r >> 1) + (c_r & 1) * 8;
}

// ============================================================================
// Forward
// ============================================================================
// TAIL (S % 256 != 0, every kernel of this file): the grid is ceil(S / block)
// and a lane whose row is >= S reads, and is masked as, row S-1; its results
// are not stored. The kv loop ends at the tile that holds row S-1, whose
// staging sources are clamped the same way (img_src_tail): its keys >= S are
// copies of key S-1 and lie above the diagonal of every row, so the masked
// body hides them. DESIGN.md, "Ragged tails in the causal pairs".
template <bool DOC, bool SINK, bool TAIL>
__global__ __launch_bounds__(512, 2) void k_attn64_fwd(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, bf16_t* __restrict__ O,
    float* __restrict__ LSE, const int* __restrict__ lo, int B, int Hq,
    int Hkv, int64_t S, float scale, const float* __restrict__ sinks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // K buffers at 0 / 16 KiB, V buffers at 32 / 48 KiB
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

  const bf16_t* Qb = Q + (((int64_t)b * Hq + hq) * S) * DH;
  const bf16_t* Kb = K + (((int64_t)b * Hkv + hkv) * S) * DH;
  const bf16_t* Vb = V + (((int64_t)b * Hkv + hkv) * S) * DH;
  bf16_t* Ob = O + (((int64_t)b * Hq + hq) * S) * DH;
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
  bf16frag qreg[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
    qreg[c] = *reinterpret_cast<const bf16frag*>(
        Qb + (int64_t)q_row * DH + c * 16 + half * 8);

  // staging: the wave fills windows 2*wave, 2*wave+1 of both images
  uint32_t ssrc[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) ssrc[u] = img_src(wave * 2 + u, lane);
  // TAIL: the lane offsets of the tile that holds row S-1
  const int t_tail = TAIL ? sm1 / KB : 0;
  uint32_t ssrc_t[2] = {0, 0};
  if (TAIL) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
      ssrc_t[u] = img_src_tail(wave * 2 + u, lane, sm1 - t_tail * KB);
  }
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
    const bf16_t* kg = Kb + (int64_t)t * KB * DH;
    const bf16_t* vg = Vb + (int64_t)t * KB * DH;
    bf16_t* kl = reinterpret_cast<bf16_t*>(smem + buf * 16384);
    bf16_t* vl = reinterpret_cast<bf16_t*>(smem + 32768 + buf * 16384);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t so = (TAIL && t == t_tail) ? ssrc_t[u] : ssrc[u];
      glds16a(kg + so, kl + (wave * 2 + u) * 512);
      glds16a(vg + so, vl + (wave * 2 + u) * 512);
    }
  };

  f32x16 oacc[2];
  oacc[0] = f32x16{};
  oacc[1] = f32x16{};
  float m_run = -1e30f;
  float l_run = 0.f;
  if (SINK) {
    m_run = sinks[hq] * LOG2E;
    l_run = 1.f;
  }

  // per-lane LDS read addresses of the current buffer, flipped once per tile;
  // subtile and 16-row chunk select by immediate offsets (g(row) does not
  // change when a multiple of 16 is added to the row)
  lds_cptr kaddr[4], vaddr[2][2];
  {
    lds_cptr kt0 = (lds_cptr)smem, vt0 = (lds_cptr)(smem + 32768);
#pragma unroll
    for (int c = 0; c < 4; ++c) kaddr[c] = kt0 + img_off(col, c * 2 + half);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      int a0, a1;
      tr_offsets(lane, d, a0, a1);
      vaddr[d][0] = vt0 + a0;
      vaddr[d][1] = vt0 + a1;
    }
  }
  int flip = 16384;

  // inclusive; TAIL: no tile past the one that holds row S-1
  const int t_max = TAIL ? min((qb * QB + QB - 1) / KB, t_tail)
                         : (qb * QB + QB - 1) / KB;
  stage(t0, 0);
  __syncthreads();

  // S^T = K Q^T of one 32-key subtile: lane owns q column col, 16 scores
  auto qk = [&](const int sub) __attribute__((always_inline)) {
    f32x16 sacc = f32x16{};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          lds_frag(kaddr[c] + sub * 4096), qreg[c], sacc, 0, 0, 0);
    return sacc;
  };

  int cur = 0;
  for (int t = t0; t <= t_max; ++t) {
    if (t < t_max) stage(t + 1, cur ^ 1);
    const int k0t = t * KB;

    // online softmax + PV of one subtile. MASK is a compile-time tag: the
    // masked body applies the causal and lower-bound select per score.
    auto softmax_pv = [&](auto mask_tag, const int sub, const f32x16 sacc)
                          __attribute__((always_inline)) {
      constexpr bool MASK = decltype(mask_tag)::value;
      // scale into the exp2 domain; the product is rounded before the
      // max-subtract (two roundings per score, as in the D = 128 kernel)
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
          oacc[0][r] *= a_r;
          oacc[1][r] *= a_r;
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
        const int off = (sub * 32 + mch * 16) * 128;
#pragma unroll
        for (int d = 0; d < 2; ++d)
          oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa, lds_tr_frag(vaddr[d][0] + off, vaddr[d][1] + off), oacc[d],
              0, 0, 0);
      }
    };

    // wave-uniform: the whole tile lies below the wave's diagonal and above
    // every lower bound of its rows
    const bool interior = (k0t + KB - 1 <= w0) && (!DOC || k0t >= lo_w1);
    if (interior) {
      // software pipeline: QK^T of subtile i+1 goes to the matrix pipe before
      // the softmax VALU stream of subtile i starts
      f32x16 s_cur = qk(0);
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        f32x16 s_nxt = s_cur;
        if (sub < 3) {
          s_nxt = qk(sub + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        softmax_pv(std::false_type{}, sub, s_cur);
        s_cur = s_nxt;
      }
    } else {
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
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
#pragma unroll
    for (int c = 0; c < 4; ++c) kaddr[c] += flip;
#pragma unroll
    for (int d = 0; d < 2; ++d) vaddr[d][0] += flip, vaddr[d][1] += flip;
    flip = -flip;
  }

  // epilogue: O / l, bf16 store, LSE
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * half;
    const float inv = 1.0f / __shfl(l_run, qr, 32);
    const int64_t qg = (int64_t)w0r + qr;
    if (!TAIL || qg < S) {
      Ob[qg * DH + col] = f2bf(oacc[0][r] * inv);
      Ob[qg * DH + 32 + col] = f2bf(oacc[1][r] * inv);
    }
  }
  if (half == 0 && (!TAIL || w0r + col < S))
    Lb[w0r + col] = 0.6931471805599453f * (m_run + __log2f(l_run));
}

// ============================================================================
// Backward preprocess: delta = rowsum(dO*O), lse2 = LSE*log2e and, with SINK,
//   part[bh*nblk + blk] = -sum_{rows of the block} exp(sink - LSE) * delta.
// Grid (S/256, B*Hq), 4 waves; a row is 8 lanes x 16 B, a wave takes 8 rows
// per pass. Every sum runs in a fixed order. TAIL: grid ceil(S/256); a row
// >= S reads row S-1, stores nothing and adds 0 to the partial.
// ============================================================================
template <bool SINK, bool TAIL>
__global__ __launch_bounds__(256) void k_attn64_bwd_pre(
    const bf16_t* __restrict__ dO, const bf16_t* __restrict__ O,
    const float* __restrict__ LSE, const float* __restrict__ sinks,
    float* __restrict__ delta, float* __restrict__ lse2,
    float* __restrict__ part, int64_t S, int Hq) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int grp = lane >> 3;
  const int cl = lane & 7;
  const int64_t bh = blockIdx.y;
  const float sink = SINK ? sinks[bh % Hq] : 0.f;
  float gacc = 0.f;   // this 8-lane group's share, the same in its lanes
  for (int it = 0; it < 8; ++it) {
    const int64_t sr = (int64_t)blockIdx.x * 256 + it * 32 + wave * 8 + grp;
    const bool ok = !TAIL || sr < S;
    const int64_t r = bh * S + (TAIL ? min(sr, S - 1) : sr);
    const bf16x8 a = reinterpret_cast<const bf16x8*>(dO + r * DH)[cl];
    const bf16x8 o = reinterpret_cast<const bf16x8*>(O + r * DH)[cl];
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += bf2f(a.v[j]) * bf2f(o.v[j]);
#pragma unroll
    for (int x = 4; x > 0; x >>= 1) acc += __shfl_xor(acc, x, kWave);
    const float lse = LSE[r];
    if (cl == 0 && ok) {
      delta[r] = acc;
      lse2[r] = lse * LOG2E;
    }
    if (SINK) gacc += ok ? expf(sink - lse) * acc : 0.f;
  }
  if (SINK) {
    float g[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = __shfl(gacc, i * 8, kWave);
    if (lane == 0)
      red[wave] = ((g[0] + g[1]) + (g[2] + g[3])) + ((g[4] + g[5]) + (g[6] + g[7]));
    __syncthreads();
    if (threadIdx.x == 0)
      part[bh * gridDim.x + blockIdx.x] =
          -((red[0] + red[1]) + (red[2] + red[3]));
  }
}

// dsinks[h] = sum over b, then blocks, of part[(b*Hq + h)*nblk + blk]
__global__ void k_attn64_dsinks(const float* __restrict__ part,
                                float* __restrict__ dsinks, int B, int Hq,
                                int nblk) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= Hq) return;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* p = part + ((int64_t)b * Hq + h) * nblk;
    for (int i = 0; i < nblk; ++i) acc += p[i];
  }
  dsinks[h] = acc;
}

// ============================================================================
// dK/dV, GQA-folded: a block owns a 64-row kv strip of one KV head and loops
// the query-head group and the 128-row q tiles from the diagonal to hi.
// 4 waves = (kv slice of 32 rows) x (q half of 64 rows); a wave runs the two
// 32x32 quadrants of its q half per tile and keeps dK/dV of its slice in
// registers; the two q halves are summed through LDS at the end. The K/V
// fragments of the slice stay in registers. Stage (34304 B): Q image 16 KiB,
// dO image 16 KiB, lse2 / delta / lo of the 128 rows 3 x 512 B.
// ============================================================================
constexpr int DKV_STAGE = 32768 + 1536;

// TAIL: strip rows >= S read K / V row S-1 and are not stored; the q tile
// that holds row S-1 is staged with clamped sources (Q, dO, lse2, delta, lo)
// and its rows >= S get P = dS = 0 through a row < S term in the masked body,
// which every quadrant that reaches S takes.
template <bool DOC, bool TAIL>
__global__ __launch_bounds__(256, 2) void k_attn64_bwd_dkv(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
    const float* __restrict__ delta, const float* __restrict__ lse2,
    bf16_t* __restrict__ dK, bf16_t* __restrict__ dV,
    const int* __restrict__ lo, const int* __restrict__ hi, int B, int Hq,
    int Hkv, int64_t S, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);   // epilogue reuse, 16 KiB

  const int kvb = blockIdx.x;          // 64-row kv strip
  const int bkh = blockIdx.y;          // b * Hkv + hkv
  const int b = bkh / Hkv;
  const int hkv = bkh % Hkv;
  const int rep = Hq / Hkv;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kvslice = wave & 1;
  const int qh = wave >> 1;
  const int half = lane >> 5;
  const int col = lane & 31;

  const int kv0 = kvb * 64;
  const int kvs0 = kv0 + kvslice * 32;          // the wave's first kv row
  const int64_t kvbase = (((int64_t)b * Hkv + hkv) * S) * DH;
  const int sm1 = (int)S - 1;

  // the slice's K / V B-fragments: row kvs0 + col, chunk c*16 + half*8
  bf16frag kf[4], vf[4];
  const int kv_ld = TAIL ? min(kvs0 + col, sm1) : kvs0 + col;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t o = kvbase + (int64_t)kv_ld * DH + c * 16 + half * 8;
    kf[c] = *reinterpret_cast<const bf16frag*>(K + o);
    vf[c] = *reinterpret_cast<const bf16frag*>(V + o);
  }

  f32x16 dv_acc[2], dk_acc[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) dv_acc[d] = f32x16{}, dk_acc[d] = f32x16{};

  const float scale2 = scale * LOG2E;
  const int qt0 = kv0 / 128;           // 128-row q tiles
  int qtn = (int)((S + (TAIL ? 127 : 0)) / 128);
  int hi_w = 0;
  if (DOC) {
    const int j_b = TAIL ? min(kv0 + 63, sm1) : kv0 + 63;
    const int j_w = TAIL ? min(kvs0 + 31, sm1) : kvs0 + 31;
    qtn = (hi[j_b] + 127) / 128;                                // block end
    hi_w = __builtin_amdgcn_readfirstlane(hi[j_w]);             // wave end
  }
  const int ntiles = qtn - qt0;
  const int itn = rep * ntiles;

  uint32_t ssrc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) ssrc[u] = img_src(wave * 4 + u, lane);
  // TAIL: the lane offsets of the q tile that holds row S-1
  const int qt_tail = TAIL ? sm1 / 128 : 0;
  uint32_t ssrc_t[4] = {0, 0, 0, 0};
  uint32_t st_t[2] = {0, 0};
  if (TAIL) {
    const int rmax = sm1 - qt_tail * 128;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      ssrc_t[u] = img_src_tail(wave * 4 + u, lane, rmax);
    st_t[0] = (uint32_t)min(lane, rmax);
    st_t[1] = (uint32_t)min(64 + lane, rmax);
  }
  // stage (head g, q tile) number `it` into buffer `buf`
  auto stage = [&](int it, int buf) __attribute__((always_inline)) {
    const int g = it / ntiles;
    const int qt = qt0 + (it - g * ntiles);
    const int64_t rowbase = ((int64_t)b * Hq + hkv * rep + g) * S + (int64_t)qt * 128;
    char* sb = smem + buf * DKV_STAGE;
    const bool tl = TAIL && qt == qt_tail;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t so = tl ? ssrc_t[u] : ssrc[u];
      glds16a(Q + rowbase * DH + so,
              reinterpret_cast<bf16_t*>(sb) + (wave * 4 + u) * 512);
      glds16a(dO + rowbase * DH + so,
              reinterpret_cast<bf16_t*>(sb + 16384) + (wave * 4 + u) * 512);
    }
    float* st = reinterpret_cast<float*>(sb + 32768);
    const uint32_t s0 = tl ? st_t[0] : (uint32_t)lane;
    const uint32_t s1 = tl ? st_t[1] : 64 + (uint32_t)lane;
    if (wave == 0) {
      glds4(lse2 + rowbase + s0, st);
      glds4(lse2 + rowbase + s1, st + 64);
    } else if (wave == 1) {
      glds4(delta + rowbase + s0, st + 128);
      glds4(delta + rowbase + s1, st + 192);
    } else if (DOC && wave == 2) {
      glds4(lo + qt * 128 + s0, st + 256);
      glds4(lo + qt * 128 + s1, st + 320);
    }
  };

  // per-lane image offsets: A-fragment rows (b128) and tr16 B-fragments; the
  // quadrant and 16-row chunk add multiples of 16 rows, which leave g(row)
  int aoff[4], troff[2][2];
#pragma unroll
  for (int c = 0; c < 4; ++c) aoff[c] = img_off(col, c * 2 + half);
#pragma unroll
  for (int d = 0; d < 2; ++d) tr_offsets(lane, d, troff[d][0], troff[d][1]);

  stage(0, 0);
  __syncthreads();
  int cur = 0;
  for (int it = 0; it < itn; ++it) {
    if (it + 1 < itn) stage(it + 1, cur ^ 1);
    const int qt = qt0 + it % ntiles;
    lds_cptr qimg = (lds_cptr)(smem + cur * DKV_STAGE);
    lds_cptr doimg = qimg + 16384;
    const float* stat = reinterpret_cast<const float*>(smem + cur * DKV_STAGE + 32768);

#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int rl0 = qh * 64 + j * 32;        // quadrant's first image row
      const int q0 = qt * 128 + rl0;
      const bool live = (q0 + 31 >= kvs0) && (!DOC || q0 < hi_w) &&
                        (!TAIL || q0 <= sm1);
      if (!live) continue;
      bool cut = q0 < kvs0 + 31;
      if (TAIL) cut = cut || (q0 + 31 > sm1);
      if (DOC)
        cut = cut || __builtin_amdgcn_readfirstlane(
                         reinterpret_cast<const int*>(stat)[256 + rl0 + 31]) > kvs0;

      // S = Q K^T and dP = dO V^T of the quadrant: lane owns kv column col
      f32x16 s2 = f32x16{}, dp2 = f32x16{};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            lds_frag(qimg + rl0 * 128 + aoff[c]), kf[c], s2, 0, 0, 0);
        dp2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            lds_frag(doimg + rl0 * 128 + aoff[c]), vf[c], dp2, 0, 0, 0);
      }
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
          const float4 d4 = *reinterpret_cast<const float4*>(stat + 128 + qr4);
          const float lse_q[4] = {l4.x, l4.y, l4.z, l4.w};
          const float del_q[4] = {d4.x, d4.y, d4.z, d4.w};
          int lo_q[4] = {0, 0, 0, 0};
          if (MASK && DOC) {
            const int4 s4 = *reinterpret_cast<const int4*>(
                reinterpret_cast<const int*>(stat) + 256 + qr4);
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
      if (cut) pds_pack(std::true_type{});
      else pds_pack(std::false_type{});

      // dV += P^T dO, dK += dS^T Q: B fragments by tr16 reads of the images
#pragma unroll
      for (int mch = 0; mch < 2; ++mch) {
        const bf16frag pa = quad_exchange(pk2[4 * mch], pk2[4 * mch + 1],
                                          pk2[4 * mch + 2], pk2[4 * mch + 3]);
        const bf16frag da = quad_exchange(dg2[4 * mch], dg2[4 * mch + 1],
                                          dg2[4 * mch + 2], dg2[4 * mch + 3]);
        const int off = (rl0 + mch * 16) * 128;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          dv_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa, lds_tr_frag(doimg + off + troff[d][0], doimg + off + troff[d][1]),
              dv_acc[d], 0, 0, 0);
          dk_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              da, lds_tr_frag(qimg + off + troff[d][0], qimg + off + troff[d][1]),
              dk_acc[d], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // sum the two q halves per kv slice through LDS (red: [slice][lane][32]
  // floats = 16 KiB, over the images: every wave is past the last barrier)
  // and store. Spelled out per accumulator: a pointer into the accumulator
  // arrays would send them to scratch.
#define VH_DKV64_COMBINE(ACC, DST)                                            \
  {                                                                           \
    float* slot = red + (kvslice * 64 + lane) * 32;                           \
    if (qh == 1) {                                                            \
      _Pragma("unroll") for (int d = 0; d < 2; ++d)                           \
          _Pragma("unroll") for (int r = 0; r < 16; r += 4)                   \
              *reinterpret_cast<float4*>(slot + d * 16 + r) = float4{         \
                  ACC[d][r], ACC[d][r + 1], ACC[d][r + 2], ACC[d][r + 3]};    \
    }                                                                         \
    __syncthreads();                                                          \
    if (qh == 0) {                                                            \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                        \
        const int kvr = (r & 3) + 8 * (r >> 2) + 4 * half;                    \
        const int64_t o = kvbase + (int64_t)(kvs0 + kvr) * DH + col;          \
        if (!TAIL || kvs0 + kvr < S) {                                        \
          DST[o] = f2bf(ACC[0][r] + slot[r]);                                 \
          DST[o + 32] = f2bf(ACC[1][r] + slot[16 + r]);                       \
        }                                                                     \
      }                                                                       \
    }                                                                         \
    __syncthreads();                                                          \
  }
  VH_DKV64_COMBINE(dv_acc, dV)
  VH_DKV64_COMBINE(dk_acc, dK)
#undef VH_DKV64_COMBINE
}

// ============================================================================
// dQ: a block owns 128 q rows (wave = 32-row slice) of one query head; the
// wave's Q / dO fragments, lse2 and delta stay in registers. 64-row kv tiles
// of K and V (8 KiB images each) are double buffered, one barrier per tile;
// the K image feeds both S = K Q^T (b128 A-fragments) and dQ += dS^T K (tr16
// B-fragments). Each 32-key subtile has its own wave-uniform live / cut test.
// ============================================================================
// TAIL: as the forward: rows >= S compute row S-1 and are not stored, the kv
// loop ends at the tile that holds row S-1, staged with clamped sources.
template <bool DOC, bool TAIL>
__global__ __launch_bounds__(256, 3) void k_attn64_bwd_dq(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
    const float* __restrict__ delta, const float* __restrict__ lse2,
    bf16_t* __restrict__ dQ, const int* __restrict__ lo, int B, int Hq,
    int Hkv, int64_t S, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // two stages of 16 KiB: K image at +0, V image at +8192

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
  const bf16_t* Kb = K + (((int64_t)b * Hkv + hkv) * S) * DH;
  const bf16_t* Vb = V + (((int64_t)b * Hkv + hkv) * S) * DH;

  const int q0b = qb * 128;
  const int w0r = q0b + wave * 32;     // the wave's first q row
  const int sm1 = (int)S - 1;
  // rows the wave and the lane compute (TAIL: clamped to S-1)
  const int w0 = TAIL ? min(w0r, sm1) : w0r;
  const int w1 = TAIL ? min(w0r + 31, sm1) : w0r + 31;
  const int q_l = TAIL ? min(w0r + col, sm1) : w0r + col;

  bf16frag qrow[4], dorow[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t o = (qbase + q_l) * DH + c * 16 + half * 8;
    qrow[c] = *reinterpret_cast<const bf16frag*>(Q + o);
    dorow[c] = *reinterpret_cast<const bf16frag*>(dO + o);
  }
  const float lse_l = lse2[qbase + q_l];
  const float del_l = delta[qbase + q_l];
  const float scale2 = scale * LOG2E;

  int lo_l = 0, lo_w0 = 0, lo_w1 = 0, kvt_begin = 0;
  if (DOC) {
    lo_l = lo[q_l];
    lo_w0 = __builtin_amdgcn_readfirstlane(lo[w0]);
    lo_w1 = __builtin_amdgcn_readfirstlane(lo[w1]);
    kvt_begin = lo[q0b] / 64;
  }

  f32x16 dq2[2];
  dq2[0] = f32x16{};
  dq2[1] = f32x16{};

  uint32_t ssrc[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) ssrc[u] = img_src(wave * 2 + u, lane);
  // TAIL: the lane offsets of the kv tile that holds row S-1
  const int kt_tail = TAIL ? sm1 / 64 : 0;
  uint32_t ssrc_t[2] = {0, 0};
  if (TAIL) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
      ssrc_t[u] = img_src_tail(wave * 2 + u, lane, sm1 - kt_tail * 64);
  }
  auto stage = [&](int kvt, int buf) __attribute__((always_inline)) {
    char* sb = smem + buf * 16384;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t so = (TAIL && kvt == kt_tail) ? ssrc_t[u] : ssrc[u];
      glds16a(Kb + (int64_t)kvt * 64 * DH + so,
              reinterpret_cast<bf16_t*>(sb) + (wave * 2 + u) * 512);
      glds16a(Vb + (int64_t)kvt * 64 * DH + so,
              reinterpret_cast<bf16_t*>(sb + 8192) + (wave * 2 + u) * 512);
    }
  };
  int aoff[4], troff[2][2];
#pragma unroll
  for (int c = 0; c < 4; ++c) aoff[c] = img_off(col, c * 2 + half);
#pragma unroll
  for (int d = 0; d < 2; ++d) tr_offsets(lane, d, troff[d][0], troff[d][1]);

  // exclusive; TAIL: no tile past the one that holds row S-1
  const int kvtn = TAIL ? min((q0b + 128) / 64, kt_tail + 1) : (q0b + 128) / 64;
  stage(kvt_begin, 0);
  __syncthreads();
  int cur = 0;
  for (int kvt = kvt_begin; kvt < kvtn; ++kvt) {
    if (kvt + 1 < kvtn) stage(kvt + 1, cur ^ 1);
    lds_cptr kimg = (lds_cptr)(smem + cur * 16384);
    lds_cptr vimg = kimg + 8192;

#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int k0 = kvt * 64 + sub * 32;
      const bool live = (k0 <= w1) && (!DOC || k0 + 32 > lo_w0);
      if (!live) continue;
      const bool cut = (k0 + 31 > w0) || (DOC && k0 < lo_w1);

      // S^T = K Q^T, dP^T = V dO^T: lane owns q column col, 16 kv rows
      f32x16 s1 = f32x16{}, dp1 = f32x16{};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            lds_frag(kimg + sub * 4096 + aoff[c]), qrow[c], s1, 0, 0, 0);
        dp1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            lds_frag(vimg + sub * 4096 + aoff[c]), dorow[c], dp1, 0, 0, 0);
      }
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

      // dQ += dS^T K: B fragments by tr16 reads of the K image
#pragma unroll
      for (int mch = 0; mch < 2; ++mch) {
        const bf16frag da = quad_exchange(dg1[4 * mch], dg1[4 * mch + 1],
                                          dg1[4 * mch + 2], dg1[4 * mch + 3]);
        const int off = (sub * 32 + mch * 16) * 128;
#pragma unroll
        for (int d = 0; d < 2; ++d)
          dq2[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              da, lds_tr_frag(kimg + off + troff[d][0], kimg + off + troff[d][1]),
              dq2[d], 0, 0, 0);
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // single-contributor store
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * half;
    const int64_t o = (qbase + w0r + qr) * DH + col;
    if (!TAIL || w0r + qr < S) {
      dQ[o] = f2bf(dq2[0][r]);
      dQ[o + 32] = f2bf(dq2[1][r]);
    }
  }
}

// shared argument checks
int check_common(int B, int Hq, int Hkv, int64_t S, float scale) {
  VH_CHECK(B > 0 && Hq > 0 && Hkv > 0, "B, Hq, Hkv must be > 0");
  VH_CHECK(S > 0, "S must be > 0");
  VH_CHECK(S * DH < (1ll << 31), "S too large for 32-bit tile offsets");
  VH_CHECK(Hq % Hkv == 0, "Hq %% Hkv != 0");
  VH_CHECK(scale > 0, "scale must be > 0 (got %g)", (double)scale);
  return 0;
}

}  // namespace

extern "C" int vh_attn64_fwd_bf16(const uint16_t* Q, const uint16_t* K,
                                  const uint16_t* V, uint16_t* O, float* LSE,
                                  int B, int Hq, int Hkv, int64_t S,
                                  float scale, const int32_t* lo,
                                  const float* sinks, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = check_common(B, Hq, Hkv, S, scale)) return rc;
  dim3 grid((uint32_t)((S + QB - 1) / QB), (uint32_t)(B * Hq));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(512), 65536, s, Q, K, V, O, LSE, lo, B,
                       Hq, Hkv, S, scale, sinks);
  };
  if (S % 256 == 0) {
    if (sinks) {
      if (lo) launch(k_attn64_fwd<true, true, false>);
      else launch(k_attn64_fwd<false, true, false>);
    } else {
      if (lo) launch(k_attn64_fwd<true, false, false>);
      else launch(k_attn64_fwd<false, false, false>);
    }
  } else {
    if (sinks) {
      if (lo) launch(k_attn64_fwd<true, true, true>);
      else launch(k_attn64_fwd<false, true, true>);
    } else {
      if (lo) launch(k_attn64_fwd<true, false, true>);
      else launch(k_attn64_fwd<false, false, true>);
    }
  }
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_attn64_bwd_pre_bf16(const uint16_t* dO, const uint16_t* O,
                                      const float* LSE, const float* sinks,
                                      float* delta, float* lse2, float* dsinks,
                                      float* partials, int B, int Hq,
                                      int64_t S, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(S > 0, "S must be > 0");
  VH_CHECK(B > 0 && Hq > 0, "B, Hq must be > 0");
  VH_CHECK(sinks == nullptr || (dsinks != nullptr && partials != nullptr),
           "sinks need the dsinks output and the partials workspace");
  const int nblk = (int)((S + 255) / 256);
  dim3 grid((uint32_t)nblk, (uint32_t)(B * Hq));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, dO, O, LSE, sinks, delta,
                       lse2, partials, S, Hq);
  };
  if (sinks) {
    if (S % 256 == 0) launch(k_attn64_bwd_pre<true, false>);
    else launch(k_attn64_bwd_pre<true, true>);
    VH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_attn64_dsinks, dim3((Hq + 63) / 64), dim3(64), 0, s,
                       partials, dsinks, B, Hq, nblk);
  } else {
    if (S % 256 == 0) launch(k_attn64_bwd_pre<false, false>);
    else launch(k_attn64_bwd_pre<false, true>);
  }
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_attn64_bwd2_bf16(const uint16_t* Q, const uint16_t* K,
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
    hipLaunchKernelGGL(kern, grid_kv, dim3(256), 2 * DKV_STAGE, s, Q, K, V, dO,
                       delta, lse2, dK, dV, lo, hi, B, Hq, Hkv, S, scale);
  };
  auto launch_dq = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid_q, dim3(256), 32768, s, Q, K, V, dO, delta,
                       lse2, dQ, lo, B, Hq, Hkv, S, scale);
  };
  const bool tail = S % 256 != 0;
  if (tail) {
    if (lo) launch_dkv(k_attn64_bwd_dkv<true, true>);
    else launch_dkv(k_attn64_bwd_dkv<false, true>);
  } else {
    if (lo) launch_dkv(k_attn64_bwd_dkv<true, false>);
    else launch_dkv(k_attn64_bwd_dkv<false, false>);
  }
  VH_HIP(hipGetLastError());
  if (tail) {
    if (lo) launch_dq(k_attn64_bwd_dq<true, true>);
    else launch_dq(k_attn64_bwd_dq<false, true>);
  } else {
    if (lo) launch_dq(k_attn64_bwd_dq<true, false>);
    else launch_dq(k_attn64_bwd_dq<false, false>);
  }
  VH_HIP(hipGetLastError());
  return 0;
}
