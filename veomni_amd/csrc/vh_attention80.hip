// Flash attention forward/backward for gfx950, head_dim 80 (bf16, NON-causal,
// block-diagonal segments, Hq == Hkv, token-major strided operands): the
// attention of the Qwen2.5-VL vision tower. The D = 128 and D = 64 pairs live
// in vh_attention.hip / vh_attention64.hip; this file shares their numerics
// (exp2 domain, the scale product rounded before the max-subtract, P and dS
// rounded to bf16, fp32 accumulation), not their tiling or layouts.
//
// Operands. Q, K, V, dO are [S, H, 80] with a runtime row stride each (in
// elements, a multiple of 8) and the head stride fixed at 80, so the v slice
// of the [S, 3, H, 80] qkv projection is read in place. O, dQ, dK, dV are
// written [S, H, 80] contiguous; LSE, delta and lse2 are [H, S] fp32.
// seg_lo / seg_hi (int32 [S], monotone, both or neither): row i sees key j iff
// seg_lo[i] <= j < seg_hi[i]; for a block-diagonal mask the rows that see key
// j are [seg_lo[j], seg_hi[j]), so the one pair serves all three kernels.
// Null bounds mean one segment [0, S).
//
// Matrix instructions. 80 = 5 * 16, so everything runs on the 16x16 MFMAs:
//   * the two D-reductions (S^T = K Q^T, dP^T = V dO^T, and S = Q K^T,
//     dP = dO V^T in the dK/dV kernel) are two v_mfma_f32_16x16x32_bf16 plus
//     one v_mfma_f32_16x16x16_bf16 for d = 64..79 (2 x 32 + 16 = 80): 20
//     passes per 16x16 block of scores against 24 for a zero-padded third
//     16x16x32, and no padded LDS image. The three products are independent
//     (C = 0) and summed on the VALU (dot80 below says why). The padded form
//     was not built, so no measured figure for it is claimed
//     (profiles/attn_vit_d80_microbench.md).
//   * the products whose output width is D (O^T = V^T P^T, dQ^T = K^T dS^T,
//     dV^T = dO^T P, dK^T = Q^T dS) are five 16-row blocks of 16x16x32.
// The kernels compute the TRANSPOSED products on purpose: the 16x16 C layout
// gives lane (g = lane/16, n = lane%16) the entries [4g .. 4g+3][n]. With
// S^T = K Q^T a lane holds four keys of ONE q row (n), so m, l, lse and delta
// are plain per-lane scalars, replicated over the four g groups; a row max is
// two permlane swaps. And two 16-key C blocks X, Y side by side ARE the B
// operand of the next 16x16x32 (k index 8g+j = key 4g+j of X for j < 4, of Y
// for j >= 4) once rounded to bf16: no cross-lane exchange between the two
// GEMMs. The A operand of that product is the matching transposed read of
// the V (K, Q, dO) image: two ds_read_b64_tr_b16, rows 4g..4g+3 of X and of Y.
//
// LDS image: 64 rows of 160 bytes, NO padding, 10 chunks of 16 B per row:
//   off(row, p) = row*160 + ((p ^ ((row>>3)&1)) << 4),   p = d >> 3.
// 160 B = 40 banks, so row r starts at bank 40 r mod 64 = 0,40,16,56,32,8,48,
// 24 for r = 0..7: eight distinct multiples of 8 banks, repeating with period
// 8. The reads the kernels issue:
//   * tr16 b64 (A^T fragments): a 32-lane phase reads rows R..R+7 (R % 8 == 0),
//     32 contiguous bytes = 8 banks each (the chunk pair 2*dblk, 2*dblk+1;
//     the XOR only swaps the pair, and is constant over the 8 rows): 8 rows x
//     8 banks on distinct multiples of 8 -> all 64 banks, conflict-free.
//   * b128 (A fragments of the D-reductions): 16 lanes read rows R..R+15
//     (R % 16 == 0) at one chunk p. Plain 160-B rows would put rows r and r+8
//     on the same 16-B slot (10*8 = 80 = 0 mod 16); rows 0..7 fill the eight
//     slots of p's parity, and the XOR sends rows 8..15 to the other parity:
//     16 distinct slots of the 256-B bank line, conflict-free.
//   * b64 of the d = 64..79 tail (chunk 8 or 9, either half): a 32-lane phase
//     is rows R..R+15 x both halves of one chunk -> the b128 case.
// A 16-row step leaves (row>>3)&1 unchanged, so subtiles are immediate
// offsets. Images are filled by global_load_lds, 16 B per lane: a wave's
// 1 KiB window is LDS chunks 64j .. 64j+63 of the image (640 chunks = 10
// windows, dealt round-robin to the four waves); lane i lands on chunk
// c = 64j+i = (row c/10, slot c%10) and fetches source chunk slot^((row>>3)&1)
// of global row min(tile_row0 + row, S-1). That clamp is all the tail handling
// the loads need: rows past S are copies of row S-1 and are masked, because a
// tile that reaches past seg_hi (<= S) of its rows always runs the masked
// body (dK/dV: q rows >= seg_hi[key] get P = dS = 0; nothing is zeroed in
// LDS). Stores are predicated on row < S.
//
// Work split. One body serves both regimes; tiles start AT the segment edge,
// not at a multiple of the tile size (per-lane source addresses make that
// free), so a q tile of 64-token windows touches exactly its windows' keys:
//   k_attn80_fwd      grid (ceil(S/128), H), 4 waves x 32 q rows (two 16-row
//                     MFMA columns). Keys [seg_lo[first row], seg_hi[last
//                     row)) in 64-key tiles, K and V images 10 KiB each,
//                     double buffered: 40 KiB. Each wave tests each tile
//                     against its own 32 rows: dead -> skipped, inside every
//                     row's segment -> unmasked body, else masked body.
//   k_attn80_bwd_dq   the same split and staging; Q, dO, lse2, delta of the
//                     wave's rows in registers.
//   k_attn80_bwd_dkv  grid (ceil(S/128), H), 4 waves x 32 keys; the wave's K
//                     and V fragments stay in registers, 64-row Q and dO
//                     images plus lse2 / delta of the tile (512 B) are double
//                     buffered: 42 KiB. No split over q, so no reduction.
//   k_attn80_bwd_pre  delta = rowsum(dO * O), lse2 = LSE * log2e.
// No atomics, no fp32 global accumulators, every output element is written
// once: results are bit-identical from run to run.

#include "vh_common.h"

#include <type_traits>

namespace {

constexpr int DH = 80;
constexpr int ROWB = 160;            // LDS row bytes
constexpr int TILE = 64;             // rows per LDS image
constexpr int IMG = TILE * ROWB;     // 10240 B
constexpr int QB = 128;              // rows per block (4 waves x 32)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float DEFER_THR = 8.0f;    // defer-max threshold (exp2 domain)

using bf16x4v = __attribute__((ext_vector_type(4))) __bf16;
typedef __attribute__((address_space(3))) const char* lds_cptr;

__device__ __forceinline__ void glds16(const bf16_t* g, void* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)g,
      (__attribute__((address_space(3))) unsigned int*)l, 16, 0, 0);
}
__device__ __forceinline__ void glds4(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)g,
      (__attribute__((address_space(3))) unsigned int*)l, 4, 0, 0);
}

__device__ __forceinline__ int img_off(int row, int p) {
  return row * ROWB + ((p ^ ((row >> 3) & 1)) << 4);
}

// fill one 64-row image from rows [r0, r0+64) (clamped to S-1) of an operand
// whose head offset is folded into `base`
__device__ __forceinline__ void stage_img(const bf16_t* base, int64_t rs,
                                          int r0, int last, char* img,
                                          int wave, int lane) {
  for (int j = wave; j < 10; j += 4) {
    const int c = j * 64 + lane;
    const int row = c / 10;
    const int p = (c - row * 10) ^ ((row >> 3) & 1);
    const int gr = min(r0 + row, last);
    glds16(base + (int64_t)gr * rs + p * 8, img + j * 1024);
  }
}

// max / sum over the four 16-lane groups (the replicas of one row): after a
// permlane swap of v with itself the two results hold the two partners' values
__device__ __forceinline__ float max4g(float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float t = __builtin_fmaximum_numf(__builtin_bit_cast(float, (uint32_t)a[0]),
                                          __builtin_bit_cast(float, (uint32_t)a[1]));
  const uint32_t tu = __builtin_bit_cast(uint32_t, t);
  auto b = __builtin_amdgcn_permlane32_swap(tu, tu, false, false);
  return __builtin_fmaximum_numf(__builtin_bit_cast(float, (uint32_t)b[0]),
                                 __builtin_bit_cast(float, (uint32_t)b[1]));
}
__device__ __forceinline__ float sum4g(float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float t = __builtin_bit_cast(float, (uint32_t)a[0]) +
                  __builtin_bit_cast(float, (uint32_t)a[1]);
  const uint32_t tu = __builtin_bit_cast(uint32_t, t);
  auto b = __builtin_amdgcn_permlane32_swap(tu, tu, false, false);
  return __builtin_bit_cast(float, (uint32_t)b[0]) +
         __builtin_bit_cast(float, (uint32_t)b[1]);
}

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) float f32x2t;
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2t;
  return __builtin_bit_cast(uint32_t,
                            __builtin_convertvector(f32x2t{lo, hi}, bf16x2t));
}
// B operand of a 16x16x32 from two C blocks: k = 8g+j is x[j], then y[j-4]
__device__ __forceinline__ bf16v8 pack_b(const f32x4 x, const f32x4 y) {
  uint4 u{pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]),
          pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3])};
  return __builtin_bit_cast(bf16v8, u);
}

__device__ __forceinline__ bf16v8 lds_b128(lds_cptr p) {
  return *(__attribute__((address_space(3))) const bf16v8*)p;
}
__device__ __forceinline__ bf16x4v lds_b64(lds_cptr p) {
  return *(__attribute__((address_space(3))) const bf16x4v*)p;
}
// A^T fragment: rows 4g..4g+3 of block X (a0) and of block Y (a1), column
// lane%16 of the 16-column block the address points into
__device__ __forceinline__ bf16v8 lds_tr(lds_cptr a0, lds_cptr a1) {
  typedef __attribute__((address_space(3))) bf16x4v as3b4;
  bf16x4v r0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((as3b4*)a0);
  bf16x4v r1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((as3b4*)a1);
  return __builtin_shufflevector(r0, r1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// per-lane image offsets, rows relative to a 16-row block:
//   a[c]  b128 A fragment of d = 32c + 8g .. +8 (row m),
//   at    b64 A fragment of d = 64 + 4g .. +4 (row m),
//   tr    tr16 source: row 4g + m/4, d = 4*(m%4) .. +4 of d block 0; d block
//         dblk adds 32 B, block Y adds 16 rows
struct LaneOffs { int a[2], at, tr; };
__device__ __forceinline__ LaneOffs lane_offs(int lane) {
  const int g = lane >> 4, m = lane & 15;
  LaneOffs o;
  o.a[0] = img_off(m, g);
  o.a[1] = img_off(m, 4 + g);
  o.at = img_off(m, 8 + (g >> 1)) + (g & 1) * 8;
  o.tr = img_off(4 * g + (m >> 2), (m & 3) >> 1) + (m & 1) * 8;
  return o;
}

__device__ __forceinline__ f32x4 mfma32(const bf16v8 a, const bf16v8 b, const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// the D-reduction of one 16x16 block: K = 80 as 32 + 32 + 16
__device__ __forceinline__ f32x4 dot80(const bf16v8 a0, const bf16v8 a1,
                                       const bf16x4v at, const bf16v8 b0,
                                       const bf16v8 b1, const bf16x4v bt) {
  // Three independent products summed on the VALU, not one dependent chain:
  // chained (16x16x32 -> 16x16x32 -> 16x16x16 through the C operand, the
  // compiler placing each result on other registers) the kernels returned
  // wrong scores in part of a block on the MI355X; see DESIGN.md.
  const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 c0 = mfma32(a0, b0, z);
  const f32x4 c1 = mfma32(a1, b1, z);
  const f32x4 ct = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(at, bt, z, 0, 0, 0);
  return (c0 + c1) + ct;
}

// a row's (or key's) 80 values as B fragments, from global memory
struct RowFrag { bf16v8 f[2]; bf16x4v t; };
__device__ __forceinline__ RowFrag load_row(const bf16_t* p, int g) {
  RowFrag r;
  r.f[0] = *reinterpret_cast<const bf16v8*>(p + 8 * g);
  r.f[1] = *reinterpret_cast<const bf16v8*>(p + 32 + 8 * g);
  r.t = *reinterpret_cast<const bf16x4v*>(p + 64 + 4 * g);
  return r;
}

// store a transposed accumulator (lane: d = 16*dblk + 4g + i of row `row`)
__device__ __forceinline__ void store_t(bf16_t* dst, const f32x4 (&acc)[5],
                                        float mul, int g) {
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    uint2 u{pack_bf16x2(acc[d][0] * mul, acc[d][1] * mul),
            pack_bf16x2(acc[d][2] * mul, acc[d][3] * mul)};
    *reinterpret_cast<uint2*>(dst + d * 16 + 4 * g) = u;
  }
}

// ============================================================================
// Forward
// ============================================================================
__global__ __launch_bounds__(256, 2) void k_attn80_fwd(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, bf16_t* __restrict__ O,
    float* __restrict__ LSE, const int* __restrict__ seg_lo,
    const int* __restrict__ seg_hi, int H, int S, int64_t q_rs, int64_t k_rs,
    int64_t v_rs, float scale) {
  __shared__ __attribute__((aligned(16))) char smem[4 * IMG];
  // stage b: K image at b*2*IMG, V image at b*2*IMG + IMG
  const int h = blockIdx.y;
  const int q0b = blockIdx.x * QB;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, m = lane & 15;
  const int last = S - 1;
  const int w0 = q0b + wave * 32;
  const float scale2 = scale * LOG2E;

  auto lo_at = [&](int r) { return seg_lo ? seg_lo[r] : 0; };
  auto hi_at = [&](int r) { return seg_hi ? seg_hi[r] : S; };

  int qr[2], lo_l[2], hi_l[2];
  RowFrag qf[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    qr[b] = min(w0 + b * 16 + m, last);
    lo_l[b] = lo_at(qr[b]);
    hi_l[b] = hi_at(qr[b]);
    qf[b] = load_row(Q + (int64_t)qr[b] * q_rs + h * DH, g);
  }
  const int wa = min(w0, last), wb = min(w0 + 31, last);
  const int lo_w0 = __builtin_amdgcn_readfirstlane(lo_at(wa));
  const int hi_w0 = __builtin_amdgcn_readfirstlane(hi_at(wa));
  const int lo_w1 = __builtin_amdgcn_readfirstlane(lo_at(wb));
  const int hi_w1 = __builtin_amdgcn_readfirstlane(hi_at(wb));
  const int kbeg = __builtin_amdgcn_readfirstlane(lo_at(q0b));
  const int kend = __builtin_amdgcn_readfirstlane(hi_at(min(q0b + QB - 1, last)));
  const int ntiles = (kend - kbeg + TILE - 1) / TILE;

  const bf16_t* Kh = K + h * DH;
  const bf16_t* Vh = V + h * DH;
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
    char* sb = smem + buf * 2 * IMG;
    stage_img(Kh, k_rs, kbeg + t * TILE, last, sb, wave, lane);
    stage_img(Vh, v_rs, kbeg + t * TILE, last, sb + IMG, wave, lane);
  };
  const LaneOffs lo_ = lane_offs(lane);

  f32x4 oacc[2][5];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int d = 0; d < 5; ++d) oacc[b][d] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {-1e30f, -1e30f};
  float l_part[2] = {0.f, 0.f};   // this lane's share of the row sum

  stage(0, 0);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) stage(t + 1, cur ^ 1);
    const int k0 = kbeg + t * TILE;
    lds_cptr kimg = (lds_cptr)(smem + cur * 2 * IMG);
    lds_cptr vimg = kimg + IMG;

    auto body = [&](auto mask_tag) __attribute__((always_inline)) {
      constexpr bool MASK = decltype(mask_tag)::value;
      // S^T = K Q^T: lane holds keys k0 + 16kb + 4g + i of rows qr[0], qr[1]
      f32x4 s[2][4];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const int ro = kb * 16 * ROWB;
        const bf16v8 a0 = lds_b128(kimg + ro + lo_.a[0]);
        const bf16v8 a1 = lds_b128(kimg + ro + lo_.a[1]);
        const bf16x4v at = lds_b64(kimg + ro + lo_.at);
#pragma unroll
        for (int b = 0; b < 2; ++b)
          s[b][kb] = dot80(a0, a1, at, qf[b].f[0], qf[b].f[1], qf[b].t);
      }
      bf16v8 pb[2][2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        // scale into the exp2 domain; the product is rounded before the
        // max-subtract (two roundings per score, as in the other pairs)
        float mt = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float p = s[b][kb][i] * scale2;
            if (MASK) {
              const int key = k0 + kb * 16 + 4 * g + i;
              if (key < lo_l[b] || key >= hi_l[b]) p = -INFINITY;
            }
            s[b][kb][i] = p;
            mt = __builtin_fmaximum_numf(mt, p);
          }
        mt = max4g(mt);
        // defer-max: rescale only when some row's max moved past the threshold
        if (__builtin_amdgcn_ballot_w64(mt > m_run[b] + DEFER_THR) != 0ull) {
          const float m_new = fmaxf(m_run[b], mt);
          const float alpha = __builtin_amdgcn_exp2f(m_run[b] - m_new);
          m_run[b] = m_new;
          l_part[b] *= alpha;
#pragma unroll
          for (int d = 0; d < 5; ++d) oacc[b][d] *= alpha;
        }
        float ps = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float e = __builtin_amdgcn_exp2f(s[b][kb][i] - m_run[b]);
            s[b][kb][i] = e;
            ps += e;
          }
        l_part[b] += ps;
        pb[b][0] = pack_b(s[b][0], s[b][1]);
        pb[b][1] = pack_b(s[b][2], s[b][3]);
      }
      // O^T += V^T P^T
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int d = 0; d < 5; ++d) {
          lds_cptr a = vimg + j * 32 * ROWB + d * 32 + lo_.tr;
          const bf16v8 vt = lds_tr(a, a + 16 * ROWB);
#pragma unroll
          for (int b = 0; b < 2; ++b)
            oacc[b][d] = mfma32(vt, pb[b][j], oacc[b][d]);
        }
    };

    // wave-uniform: some row of the wave sees some key of the tile; every
    // row of the wave sees every key of the tile
    if (k0 < hi_w1 && k0 + TILE > lo_w0) {
      if (k0 >= lo_w1 && k0 + TILE <= hi_w0) body(std::false_type{});
      else body(std::true_type{});
    }
    __syncthreads();
    cur ^= 1;
  }

#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const float l = sum4g(l_part[b]);
    const int row = w0 + b * 16 + m;
    if (row < S) {
      store_t(O + ((int64_t)row * H + h) * DH, oacc[b], 1.0f / l, g);
      if (g == 0)
        LSE[(int64_t)h * S + row] = 0.6931471805599453f * (m_run[b] + __log2f(l));
    }
  }
}

// ============================================================================
// Backward preprocess: delta = rowsum(dO * O), lse2 = LSE * log2e. 16 lanes per
// (row, head), ten of them with a 16-B chunk; fixed-order sums.
// ============================================================================
__global__ __launch_bounds__(256) void k_attn80_bwd_pre(
    const bf16_t* __restrict__ dO, const bf16_t* __restrict__ O,
    const float* __restrict__ LSE, float* __restrict__ delta,
    float* __restrict__ lse2, int H, int S, int64_t do_rs) {
  const int64_t n = (int64_t)S * H;
  const int64_t rh = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int64_t rc = rh < n ? rh : n - 1;
  const int sub = threadIdx.x & 15;
  const int s = (int)(rc / H), h = (int)(rc % H);
  float acc = 0.f;
  if (sub < 10) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(dO + (int64_t)s * do_rs + h * DH + sub * 8);
    const bf16x8 o = *reinterpret_cast<const bf16x8*>(O + rc * DH + sub * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += bf2f(a.v[j]) * bf2f(o.v[j]);
  }
#pragma unroll
  for (int x = 8; x > 0; x >>= 1) acc += __shfl_xor(acc, x, 16);
  if (sub == 0 && rh < n) {
    const int64_t i = (int64_t)h * S + s;
    delta[i] = acc;
    lse2[i] = LSE[i] * LOG2E;
  }
}

// ============================================================================
// dQ: the forward's split. dS^T = P^T o (dP^T - delta) * scale per 64-key
// tile, dQ^T += K^T dS^T with K^T read transposed from the same K image that
// feeds S^T = K Q^T.
// ============================================================================
__global__ __launch_bounds__(256, 2) void k_attn80_bwd_dq(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
    const float* __restrict__ delta, const float* __restrict__ lse2,
    bf16_t* __restrict__ dQ, const int* __restrict__ seg_lo,
    const int* __restrict__ seg_hi, int H, int S, int64_t q_rs, int64_t k_rs,
    int64_t v_rs, int64_t do_rs, float scale) {
  __shared__ __attribute__((aligned(16))) char smem[4 * IMG];
  const int h = blockIdx.y;
  const int q0b = blockIdx.x * QB;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, m = lane & 15;
  const int last = S - 1;
  const int w0 = q0b + wave * 32;
  const float scale2 = scale * LOG2E;

  auto lo_at = [&](int r) { return seg_lo ? seg_lo[r] : 0; };
  auto hi_at = [&](int r) { return seg_hi ? seg_hi[r] : S; };

  int lo_l[2], hi_l[2];
  float lse_l[2], del_l[2];
  RowFrag qf[2], dof[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int r = min(w0 + b * 16 + m, last);
    lo_l[b] = lo_at(r);
    hi_l[b] = hi_at(r);
    lse_l[b] = lse2[(int64_t)h * S + r];
    del_l[b] = delta[(int64_t)h * S + r];
    qf[b] = load_row(Q + (int64_t)r * q_rs + h * DH, g);
    dof[b] = load_row(dO + (int64_t)r * do_rs + h * DH, g);
  }
  const int wa = min(w0, last), wb = min(w0 + 31, last);
  const int lo_w0 = __builtin_amdgcn_readfirstlane(lo_at(wa));
  const int hi_w0 = __builtin_amdgcn_readfirstlane(hi_at(wa));
  const int lo_w1 = __builtin_amdgcn_readfirstlane(lo_at(wb));
  const int hi_w1 = __builtin_amdgcn_readfirstlane(hi_at(wb));
  const int kbeg = __builtin_amdgcn_readfirstlane(lo_at(q0b));
  const int kend = __builtin_amdgcn_readfirstlane(hi_at(min(q0b + QB - 1, last)));
  const int ntiles = (kend - kbeg + TILE - 1) / TILE;

  const bf16_t* Kh = K + h * DH;
  const bf16_t* Vh = V + h * DH;
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
    char* sb = smem + buf * 2 * IMG;
    stage_img(Kh, k_rs, kbeg + t * TILE, last, sb, wave, lane);
    stage_img(Vh, v_rs, kbeg + t * TILE, last, sb + IMG, wave, lane);
  };
  const LaneOffs lo_ = lane_offs(lane);

  f32x4 dq[2][5];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int d = 0; d < 5; ++d) dq[b][d] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) stage(t + 1, cur ^ 1);
    const int k0 = kbeg + t * TILE;
    lds_cptr kimg = (lds_cptr)(smem + cur * 2 * IMG);
    lds_cptr vimg = kimg + IMG;

    auto body = [&](auto mask_tag) __attribute__((always_inline)) {
      constexpr bool MASK = decltype(mask_tag)::value;
      // two 32-key halves, so that only 2 x 2 score blocks per row group and
      // quantity are live at a time
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x4 ds[2][2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int ro = (j * 2 + kk) * 16 * ROWB;
          const bf16v8 a0 = lds_b128(kimg + ro + lo_.a[0]);
          const bf16v8 a1 = lds_b128(kimg + ro + lo_.a[1]);
          const bf16x4v at = lds_b64(kimg + ro + lo_.at);
          const bf16v8 v0 = lds_b128(vimg + ro + lo_.a[0]);
          const bf16v8 v1 = lds_b128(vimg + ro + lo_.a[1]);
          const bf16x4v vt = lds_b64(vimg + ro + lo_.at);
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const f32x4 s = dot80(a0, a1, at, qf[b].f[0], qf[b].f[1], qf[b].t);
            const f32x4 dp = dot80(v0, v1, vt, dof[b].f[0], dof[b].f[1], dof[b].t);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float pp = __builtin_amdgcn_exp2f(
                  __builtin_fmaf(s[i], scale2, -lse_l[b]));
              if (MASK) {
                const int key = k0 + (j * 2 + kk) * 16 + 4 * g + i;
                pp = (key < lo_l[b] || key >= hi_l[b]) ? 0.f : pp;
              }
              ds[b][kk][i] = pp * (dp[i] - del_l[b]) * scale;
            }
          }
        }
        const bf16v8 db0 = pack_b(ds[0][0], ds[0][1]);
        const bf16v8 db1 = pack_b(ds[1][0], ds[1][1]);
        // dQ^T += K^T dS^T
#pragma unroll
        for (int d = 0; d < 5; ++d) {
          lds_cptr a = kimg + j * 32 * ROWB + d * 32 + lo_.tr;
          const bf16v8 kt = lds_tr(a, a + 16 * ROWB);
          dq[0][d] = mfma32(kt, db0, dq[0][d]);
          dq[1][d] = mfma32(kt, db1, dq[1][d]);
        }
      }
    };

    if (k0 < hi_w1 && k0 + TILE > lo_w0) {
      if (k0 >= lo_w1 && k0 + TILE <= hi_w0) body(std::false_type{});
      else body(std::true_type{});
    }
    __syncthreads();
    cur ^= 1;
  }

#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int row = w0 + b * 16 + m;
    if (row < S) store_t(dQ + ((int64_t)row * H + h) * DH, dq[b], 1.0f, g);
  }
}

// ============================================================================
// dK/dV: a block owns 128 keys of one head, a wave 32 of them (two 16-key
// MFMA columns, K and V fragments in registers), and loops over the 64-row q
// tiles of [seg_lo[first key], seg_hi[last key]). Per 32 q rows:
// S = Q K^T and dP = dO V^T (lane: q rows 4g+i, key lane%16), P and dS packed
// straight into B operands, dV^T += dO^T P, dK^T += Q^T dS with dO^T / Q^T
// read transposed from the images.
// Stage: Q image, dO image, lse2 and delta of the 64 rows.
// ============================================================================
constexpr int DKV_STAGE = 2 * IMG + 512;

__global__ __launch_bounds__(256, 2) void k_attn80_bwd_dkv(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
    const float* __restrict__ delta, const float* __restrict__ lse2,
    bf16_t* __restrict__ dK, bf16_t* __restrict__ dV,
    const int* __restrict__ seg_lo, const int* __restrict__ seg_hi, int H,
    int S, int64_t q_rs, int64_t k_rs, int64_t v_rs, int64_t do_rs,
    float scale) {
  __shared__ __attribute__((aligned(16))) char smem[2 * DKV_STAGE];
  const int h = blockIdx.y;
  const int k0b = blockIdx.x * QB;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, m = lane & 15;
  const int last = S - 1;
  const int kvs = k0b + wave * 32;
  const float scale2 = scale * LOG2E;

  auto lo_at = [&](int r) { return seg_lo ? seg_lo[r] : 0; };
  auto hi_at = [&](int r) { return seg_hi ? seg_hi[r] : S; };

  int lo_k[2], hi_k[2];
  RowFrag kf[2], vf[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int r = min(kvs + b * 16 + m, last);
    lo_k[b] = lo_at(r);
    hi_k[b] = hi_at(r);
    kf[b] = load_row(K + (int64_t)r * k_rs + h * DH, g);
    vf[b] = load_row(V + (int64_t)r * v_rs + h * DH, g);
  }
  const bool wave_on = kvs < S;
  const int wa = min(kvs, last), wb = min(kvs + 31, last);
  const int lo_w0 = __builtin_amdgcn_readfirstlane(lo_at(wa));
  const int hi_w0 = __builtin_amdgcn_readfirstlane(hi_at(wa));
  const int lo_w1 = __builtin_amdgcn_readfirstlane(lo_at(wb));
  const int hi_w1 = __builtin_amdgcn_readfirstlane(hi_at(wb));
  const int qbeg = __builtin_amdgcn_readfirstlane(lo_at(k0b));
  const int qend = __builtin_amdgcn_readfirstlane(hi_at(min(k0b + QB - 1, last)));
  const int ntiles = (qend - qbeg + TILE - 1) / TILE;

  const bf16_t* Qh = Q + h * DH;
  const bf16_t* dOh = dO + h * DH;
  const float* lse_h = lse2 + (int64_t)h * S;
  const float* del_h = delta + (int64_t)h * S;
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
    char* sb = smem + buf * DKV_STAGE;
    const int r0 = qbeg + t * TILE;
    stage_img(Qh, q_rs, r0, last, sb, wave, lane);
    stage_img(dOh, do_rs, r0, last, sb + IMG, wave, lane);
    // waves 2 and 3 carry two image windows, waves 0 and 1 three
    if (wave == 2) glds4(lse_h + min(r0 + lane, last), sb + 2 * IMG);
    if (wave == 3) glds4(del_h + min(r0 + lane, last), sb + 2 * IMG + 256);
  };
  const LaneOffs lo_ = lane_offs(lane);

  f32x4 dv[2][5], dk[2][5];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int d = 0; d < 5; ++d)
      dv[b][d] = f32x4{0.f, 0.f, 0.f, 0.f}, dk[b][d] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) stage(t + 1, cur ^ 1);
    lds_cptr qimg = (lds_cptr)(smem + cur * DKV_STAGE);
    lds_cptr doimg = qimg + IMG;
    const float* stat = reinterpret_cast<const float*>(smem + cur * DKV_STAGE + 2 * IMG);

#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const int q0 = qbeg + t * TILE + pr * 32;
      auto body = [&](auto mask_tag) __attribute__((always_inline)) {
        constexpr bool MASK = decltype(mask_tag)::value;
        // P and dS as packed bf16 pairs, [q block][key block]
        uint32_t pk[2][2][2], dg[2][2][2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          const int rl = pr * 32 + qb * 16;
          const int ro = rl * ROWB;
          const bf16v8 a0 = lds_b128(qimg + ro + lo_.a[0]);
          const bf16v8 a1 = lds_b128(qimg + ro + lo_.a[1]);
          const bf16x4v at = lds_b64(qimg + ro + lo_.at);
          const bf16v8 o0 = lds_b128(doimg + ro + lo_.a[0]);
          const bf16v8 o1 = lds_b128(doimg + ro + lo_.a[1]);
          const bf16x4v ot = lds_b64(doimg + ro + lo_.at);
          const float4 l4 = *reinterpret_cast<const float4*>(stat + rl + 4 * g);
          const float4 d4 = *reinterpret_cast<const float4*>(stat + 64 + rl + 4 * g);
          const float lse_q[4] = {l4.x, l4.y, l4.z, l4.w};
          const float del_q[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const f32x4 s = dot80(a0, a1, at, kf[b].f[0], kf[b].f[1], kf[b].t);
            const f32x4 dp = dot80(o0, o1, ot, vf[b].f[0], vf[b].f[1], vf[b].t);
            float pv[4], gv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float pp = __builtin_amdgcn_exp2f(
                  __builtin_fmaf(s[i], scale2, -lse_q[i]));
              if (MASK) {
                const int qrow = q0 + qb * 16 + 4 * g + i;
                pp = (qrow < lo_k[b] || qrow >= hi_k[b]) ? 0.f : pp;
              }
              pv[i] = pp;
              gv[i] = pp * (dp[i] - del_q[i]) * scale;
            }
            pk[qb][b][0] = pack_bf16x2(pv[0], pv[1]);
            pk[qb][b][1] = pack_bf16x2(pv[2], pv[3]);
            dg[qb][b][0] = pack_bf16x2(gv[0], gv[1]);
            dg[qb][b][1] = pack_bf16x2(gv[2], gv[3]);
          }
        }
        // B operands: k = 8g+j is q row 4g+j of the first q block for j < 4,
        // of the second for j >= 4
        auto bop = [](const uint32_t (&x)[2], const uint32_t (&y)[2]) {
          return __builtin_bit_cast(bf16v8, uint4{x[0], x[1], y[0], y[1]});
        };
        const bf16v8 pb0 = bop(pk[0][0], pk[1][0]);
        const bf16v8 pb1 = bop(pk[0][1], pk[1][1]);
        const bf16v8 db0 = bop(dg[0][0], dg[1][0]);
        const bf16v8 db1 = bop(dg[0][1], dg[1][1]);
#pragma unroll
        for (int d = 0; d < 5; ++d) {
          const int o = pr * 32 * ROWB + d * 32 + lo_.tr;
          const bf16v8 dot_ = lds_tr(doimg + o, doimg + o + 16 * ROWB);
          const bf16v8 qt_ = lds_tr(qimg + o, qimg + o + 16 * ROWB);
          dv[0][d] = mfma32(dot_, pb0, dv[0][d]);
          dv[1][d] = mfma32(dot_, pb1, dv[1][d]);
          dk[0][d] = mfma32(qt_, db0, dk[0][d]);
          dk[1][d] = mfma32(qt_, db1, dk[1][d]);
        }
      };
      // wave-uniform: some key of the wave is seen by some of the 32 rows;
      // every key of the wave is seen by all of them (rows past S lie past
      // every seg_hi, so they always take the masked body)
      if (wave_on && q0 < hi_w1 && q0 + 32 > lo_w0) {
        if (q0 >= lo_w1 && q0 + 32 <= hi_w0) body(std::false_type{});
        else body(std::true_type{});
      }
    }
    __syncthreads();
    cur ^= 1;
  }

#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int row = kvs + b * 16 + m;
    if (row < S) {
      store_t(dV + ((int64_t)row * H + h) * DH, dv[b], 1.0f, g);
      store_t(dK + ((int64_t)row * H + h) * DH, dk[b], 1.0f, g);
    }
  }
}

int check_common(const void* seg_lo, const void* seg_hi, int H, int64_t S,
                 float scale) {
  VH_CHECK(H > 0 && H <= 65535, "H must be in 1..65535 (got %d)", H);
  VH_CHECK(S >= 1 && S < (1ll << 31) - 2 * QB, "S must be in 1..2^31-257");
  VH_CHECK(scale > 0, "scale must be > 0 (got %g)", (double)scale);
  VH_CHECK((seg_lo == nullptr) == (seg_hi == nullptr),
           "seg_lo / seg_hi must be passed together");
  return 0;
}
int check_stride(const char* what, const void* p, int H, int64_t rs) {
  VH_CHECK(rs >= (int64_t)H * DH && rs % 8 == 0,
           "%s row stride %lld: need a multiple of 8 elements >= H*80", what,
           (long long)rs);
  VH_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "%s is not 16-byte aligned", what);
  return 0;
}

}  // namespace

extern "C" int vh_attn80_fwd_bf16(const uint16_t* Q, const uint16_t* K,
                                  const uint16_t* V, uint16_t* O, float* LSE,
                                  int H, int64_t S, int64_t q_rs, int64_t k_rs,
                                  int64_t v_rs, float scale,
                                  const int32_t* seg_lo, const int32_t* seg_hi,
                                  void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = check_common(seg_lo, seg_hi, H, S, scale)) return rc;
  if (int rc = check_stride("Q", Q, H, q_rs)) return rc;
  if (int rc = check_stride("K", K, H, k_rs)) return rc;
  if (int rc = check_stride("V", V, H, v_rs)) return rc;
  if (int rc = check_stride("O", O, H, (int64_t)H * DH)) return rc;
  dim3 grid((uint32_t)((S + QB - 1) / QB), (uint32_t)H);
  hipLaunchKernelGGL(k_attn80_fwd, grid, dim3(256), 0, s, Q, K, V, O, LSE,
                     seg_lo, seg_hi, H, (int)S, q_rs, k_rs, v_rs, scale);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_attn80_bwd_pre_bf16(const uint16_t* dO, const uint16_t* O,
                                      const float* LSE, float* delta,
                                      float* lse2, int H, int64_t S,
                                      int64_t do_rs, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = check_common(nullptr, nullptr, H, S, 1.0f)) return rc;
  if (int rc = check_stride("dO", dO, H, do_rs)) return rc;
  if (int rc = check_stride("O", O, H, (int64_t)H * DH)) return rc;
  const int64_t nblk = (S * H + 15) / 16;
  VH_CHECK(nblk < (1ll << 31), "S*H too large");
  hipLaunchKernelGGL(k_attn80_bwd_pre, dim3((uint32_t)nblk), dim3(256), 0, s,
                     dO, O, LSE, delta, lse2, H, (int)S, do_rs);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_attn80_bwd2_bf16(const uint16_t* Q, const uint16_t* K,
                                   const uint16_t* V, const uint16_t* dO,
                                   const float* delta, const float* lse2,
                                   uint16_t* dQ, uint16_t* dK, uint16_t* dV,
                                   int H, int64_t S, int64_t q_rs,
                                   int64_t k_rs, int64_t v_rs, int64_t do_rs,
                                   float scale, const int32_t* seg_lo,
                                   const int32_t* seg_hi, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = check_common(seg_lo, seg_hi, H, S, scale)) return rc;
  if (int rc = check_stride("Q", Q, H, q_rs)) return rc;
  if (int rc = check_stride("K", K, H, k_rs)) return rc;
  if (int rc = check_stride("V", V, H, v_rs)) return rc;
  if (int rc = check_stride("dO", dO, H, do_rs)) return rc;
  if (int rc = check_stride("dQ", dQ, H, (int64_t)H * DH)) return rc;
  if (int rc = check_stride("dK", dK, H, (int64_t)H * DH)) return rc;
  if (int rc = check_stride("dV", dV, H, (int64_t)H * DH)) return rc;
  dim3 grid((uint32_t)((S + QB - 1) / QB), (uint32_t)H);
  hipLaunchKernelGGL(k_attn80_bwd_dkv, grid, dim3(256), 0, s, Q, K, V, dO,
                     delta, lse2, dK, dV, seg_lo, seg_hi, H, (int)S, q_rs, k_rs,
                     v_rs, do_rs, scale);
  VH_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_attn80_bwd_dq, grid, dim3(256), 0, s, Q, K, V, dO, delta,
                     lse2, dQ, seg_lo, seg_hi, H, (int)S, q_rs, k_rs, v_rs,
                     do_rs, scale);
  VH_HIP(hipGetLastError());
  return 0;
}
