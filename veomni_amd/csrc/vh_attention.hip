// Flash attention forward for gfx950 (bf16, causal, GQA, D=128).
//
// Replaces the external flash_attn wheel the reference delegates to
// (ref ops/kernels/attention/flash.py:153-301) for the packed causal path.
//
// Structure (guide cdna_hip_programming.md Appendix B, swapped-QK^T design):
//   grid (S/256, B*Hq); block = 8 waves (512 thr), wave w owns 32 q rows.
//   Q fragments live in registers (tile-invariant); K and V tiles
//   ([64 kv][128 d]) are double-buffered and both filled by glds straight
//   into LDS, issued before the tile's MFMA phase (T14): K with a
//   lane-swizzled source (kswz), V as the L16 latin-square image (per-lane
//   permuted sources) that the PV B-fragments read with the CDNA4 tr16
//   hardware transpose. Earlier V staging went through registers and
//   transposing ds_writes; the glds image drops both (DESIGN.md, round-2
//   outcomes). Per 32-kv subtile:
//     S^T = mfma_32x32x16(A=K, B=Q): lane owns col q = lane&31, 16 f32
//       scores (the kv rows split across the lane pair);
//     online softmax per q-col (running m, l lane scalars; cross-half
//       reduce = one v_permlane32_swap): scores scaled into the exp2
//       domain, row maximum by a v_max3 tree, P = exp2(s*scale2 - m) with
//       the raw v_exp_f32; defer-max (T13, THR=8) skips the
//       O-rescale when the wave's max is stable;
//     P packed to bf16 pairs (one v_cvt_pk each), partner-quad exchange by
//       two v_permlane32_swap whose both outputs are used -> A-fragment;
//     O += mfma(A=P^T, B=V^T (tr16 reads)).
//   The subtile body exists twice, with and without the causal / document
//   compare+select per score; a wave-uniform test per kv tile (does the tile
//   touch the wave's diagonal; varlen: always) picks one. The LDS read
//   addresses (8 K bases, 8 V bases) are per-lane values carried across the
//   loop and flipped between the two buffers once per tile; subtile and
//   16-row chunk select by immediate offsets. Staging sources are a
//   wave-uniform tile base plus a 32-bit lane offset.
//   Epilogue: O / l via lane broadcasts; LSE = m + log(l) saved for bwd.
//   Measurements: profiles/attn_valu_ab.md.
//
// LDS: 2x(K 16 + V 16) = 64 KiB.

#include "vh_common.h"

#include <type_traits>

namespace {

constexpr int QB = 256;   // q rows per block
constexpr int WQ = 32;    // q rows per wave
constexpr int KB = 64;    // kv rows per tile
constexpr int DH = 128;   // head dim
constexpr float DEFER_THR = 8.0f;  // T13 defer-max threshold

using bf16frag = __attribute__((ext_vector_type(8))) __bf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

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

// 256-B rows (K, Q tiles): conflict-free slot map for b128 reads
__device__ __forceinline__ int kswz(int row, int colb) {
  return colb ^ ((row & 15) << 4);
}

// 32-lane-distance exchange via v_permlane32_swap (1 VALU op) instead of
// __shfl_xor's ds_bpermute (~50-cycle LDS round trip) — guide T12.
__device__ __forceinline__ uint32_t swap32_u(uint32_t v, int half) {
  auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return half ? (uint32_t)r[0] : (uint32_t)r[1];
}

__device__ __forceinline__ float xor32h(float v, int half) {
  return __builtin_bit_cast(float, swap32_u(__builtin_bit_cast(uint32_t, v), half));
}

// Two f32 -> one packed bf16 pair (RNE) in a single v_cvt_pk_bf16_f32;
// converting the halves one by one costs two converts, a shift and an or.
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) float f32x2t;
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2t;
  return __builtin_bit_cast(uint32_t,
                            __builtin_convertvector(f32x2t{lo, hi}, bf16x2t));
}

// max of three as one v_max3_f32. fmaxf on raw MFMA outputs makes the
// compiler put a canonicalising v_max_f32 v,v,v in front of every operand;
// maximumnum has the hardware's own NaN behaviour and needs none. (Not inline
// asm: the wait states between an MFMA and a VALU read of its result are the
// compiler's to insert, and it does not look into asm operands; an asm
// v_max3_f32 here read stale accumulators.)
__device__ __forceinline__ float max3f(float a, float b, float c) {
  return __builtin_fmaximum_numf(__builtin_fmaximum_numf(a, b), c);
}

// Partner-quad exchange of packed bf16 pairs into an MFMA A/B fragment.
// In: this lane's pairs for kv (or q) rows +0..3 (a0, a1) and +8..11 (c0, c1)
// of a 16-row chunk; its lane+32 partner holds rows +4..7 and +12..15. Out:
// 8 consecutive rows, +0..7 in the lower and +8..15 in the upper half-wave.
// v_permlane32_swap(vdst, src) swaps lanes 32-63 of vdst with lanes 0-31 of
// src, so swap(a, c) leaves [own a | partner's c] in vdst and [partner's a |
// own c] in src: both outputs are used and no half-wave select is needed.
__device__ __forceinline__ bf16frag quad_exchange(uint32_t a0, uint32_t a1,
                                                  uint32_t c0, uint32_t c1) {
  auto r0 = __builtin_amdgcn_permlane32_swap(a0, c0, false, false);
  auto r1 = __builtin_amdgcn_permlane32_swap(a1, c1, false, false);
  uint4 u{(uint32_t)r0[0], (uint32_t)r1[0], (uint32_t)r0[1], (uint32_t)r1[1]};
  return __builtin_bit_cast(bf16frag, u);
}

// Where O (forward) and dO (backward) live: element strides of the batch,
// head and row indices, D contiguous. Head-major [B,Hq,S,D] is {Hq*S*DH,
// S*DH, DH}; token-major [B,S,Hq,D] (what o_proj reads as [B,S,Hq*D] without
// a copy) is {S*Hq*DH, DH, Hq*DH}. Runtime values, not a template parameter:
// tile bases stay wave-uniform, lane offsets 32-bit, and the kernels keep
// one instantiation per DOC. Q, K, V, dQ, dK, dV and the per-row statistics
// are head-major always.
struct OStrides {
  int64_t sb, sh, sr;
};
__host__ inline OStrides head_major(int Hq, int64_t S) {
  return OStrides{(int64_t)Hq * S * DH, S * DH, DH};
}

// DOC: packed-varlen (block-diagonal causal) masking via per-token document
// start indices (doc_start[t] = cu_seqlens[i] for t in document i; B == 1).
// Replaces the reference's flash-attn varlen cu_seqlens path
// (ops/kernels/attention/flash.py:61-91, kwargs from data_collator.py:50).
// V image: natural [64 kv][128 d] layout, off(kv,d) = kv*256 + L16*16 +
// (d&7)*2, L16 = (kv&15) ^ (((p&3)<<2)|(p>>2)), p = d>>3 (the same image
// k_attn_bwd_dkv_g stages Q/dO in).
// The bounds need not come from documents: the kernel only assumes that
// doc_start is monotone non-decreasing and indexes it by row within the
// sequence, never by batch, so a causal window of W keys is the same array
// with max(doc_start[q], q-W+1) in it (vh_attn_fwd_win_sink_bf16).
// SINK: attention sinks (gpt-oss). Row q of head hq has one more softmax
// column, with the logit sinks[hq] (fp32, natural-log domain, not multiplied
// by scale) and a zero value vector. The online softmax simply starts from
// that column, m_run = sinks[hq]*log2e and l_run = 1, instead of from the
// empty row (-1e30, 0): the defer-max rescale then treats it like any score
// seen earlier, so a dominant sink cannot overflow (every later exponent is
// <= DEFER_THR) and a negligible one is scaled away by the first rescale.
// LSE includes the sink, which is all the backward kernels need: their
// P = exp2(s*scale2 - lse2) is then the sink-inclusive probability.
template <bool DOC, bool SINK>
__global__ __launch_bounds__(512, 2) void k_attn_fwd(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, bf16_t* __restrict__ O,
    float* __restrict__ LSE, const int* __restrict__ doc_start, int B, int Hq,
    int Hkv, int64_t S, float scale, OStrides os,
    const float* __restrict__ sinks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto kt = [&](int buf) {                                   // 2 x 16 KiB
    return reinterpret_cast<bf16_t*>(smem + buf * 16384);
  };
  auto vt = [&](int buf) {                                   // 2 x 16 KiB
    return reinterpret_cast<bf16_t*>(smem + 32768 + buf * 16384);
  };

  const int qb = blockIdx.x;
  const int bh = blockIdx.y;           // b * Hq + hq
  const int b = bh / Hq;
  const int hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int half = lane >> 5;
  const int col = lane & 31;           // q within the wave for S; d%32 for O

  const bf16_t* Qb = Q + (((int64_t)b * Hq + hq) * S) * DH;
  const bf16_t* Kb = K + (((int64_t)b * Hkv + hkv) * S) * DH;
  const bf16_t* Vb = V + (((int64_t)b * Hkv + hkv) * S) * DH;
  bf16_t* Ob = O + b * os.sb + hq * os.sh;
  float* Lb = LSE + ((int64_t)b * Hq + hq) * S;

  const int64_t q_global = (int64_t)qb * QB + wave * WQ + col;
  const float scale2 = scale * 1.4426950408889634f;  // log2(e)

  // varlen: this lane's document start, and the wave/block minima (doc_start
  // is monotone non-decreasing, so the first row's value is the minimum)
  int ds_l = 0, ds_wave = 0, t0 = 0;
  if (DOC) {
    ds_l = doc_start[q_global];
    ds_wave = doc_start[(int64_t)qb * QB + wave * WQ];
    t0 = doc_start[(int64_t)qb * QB] / KB;
  }

  // ---- Q fragments straight into registers (tile-invariant: chunk c =
  // Q[q = col][c*16 + half*8 .. +8))
  bf16frag qreg[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    qreg[c] = *reinterpret_cast<const bf16frag*>(
        Qb + q_global * DH + c * 16 + half * 8);
  }

  // ---- persistent staging addresses: 32-bit lane offsets, added to the
  // tile's wave-uniform base (scalar-base global addressing: no 64-bit
  // per-lane pointers live across the loop)
  uint32_t ksrc[2];
  int klds[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int base = i * 8192 + wave * 1024;
    int o = base + lane * 16;
    int row = o >> 8;
    int colb = o & 255;
    ksrc[i] = (uint32_t)(row * DH + (kswz(row, colb) >> 1));
    klds[i] = base >> 1;
  }
  f32x16 oacc[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) oacc[d] = f32x16{};
  float m_run = -1e30f;
  float l_run = 0.f;
  if (SINK) {
    m_run = sinks[hq] * 1.4426950408889634f;
    l_run = 1.f;
  }

  const int t_max = (int)(((int64_t)qb * QB + QB - 1) / KB);  // inclusive

  // ---- per-lane LDS read addresses of the current buffer, carried across
  // the loop and flipped to the other buffer once per tile; sub / mch select
  // by immediate offsets. K b128 reads: the kswz slot of d-chunk c depends
  // on the lane's row (col & 15), not on sub -> 8 bases. V tr16 reads: the
  // L16 slot depends on (kv & 15), which neither sub (32 rows) nor mch (16
  // rows) changes -> one base per d block and 4-row half.
  typedef __attribute__((address_space(3))) const char* lds_cptr;
  lds_cptr kaddr[8], vaddr[4][2];
  {
    lds_cptr kt0 = (lds_cptr)kt(0), vt0 = (lds_cptr)vt(0);
#pragma unroll
    for (int c = 0; c < 8; ++c)
      kaddr[c] = kt0 + col * 256 + kswz(col, (c * 16 + half * 8) * 2);
    const int m_ = lane & 15;
    const int colhi_ = (lane >> 4) & 1;
    const int kvb0 = half * 8 + (m_ >> 2);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int c_r = d * 8 + colhi_ * 4 + (m_ & 3);
      const int perm_ = (((c_r >> 1) & 3) << 2) | (c_r >> 3);
      vaddr[d][0] = vt0 + kvb0 * 256 + ((kvb0 & 15) ^ perm_) * 16 + (c_r & 1) * 8;
      vaddr[d][1] = vt0 + (kvb0 + 4) * 256 + (((kvb0 + 4) & 15) ^ perm_) * 16 +
                    (c_r & 1) * 8;
    }
  }
  int flip = 16384;  // byte distance to the other buffer

  // prologue: stage tile t0 synchronously
  {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      glds16a(Kb + (int64_t)t0 * KB * DH + ksrc[i], kt(0) + klds[i]);
    // glds fill of the L16 V image: window win = wave*2+u covers 4 kv rows
    // (1024 B, lane-linear dest); lane sources pair p = P(slot ^ (kv&15))
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int win = wave * 2 + u;
      const int kvr = win * 4 + (lane >> 4);
      const int pp0 = (lane & 15) ^ (kvr & 15);
      const int pg = ((pp0 & 3) << 2) | (pp0 >> 2);
      glds16a(Vb + (int64_t)t0 * KB * DH + (uint32_t)(kvr * DH + pg * 8),
              vt(0) + win * 512);
    }
  }
  __syncthreads();

  int cur = 0;
  for (int t = t0; t <= t_max; ++t) {
    // ---- T14: issue next tile's loads before this tile's MFMAs
    if (t < t_max) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        glds16a(Kb + (int64_t)(t + 1) * KB * DH + ksrc[i],
                kt(cur ^ 1) + klds[i]);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int win = wave * 2 + u;
        const int kvr = win * 4 + (lane >> 4);
        const int pp0 = (lane & 15) ^ (kvr & 15);
        const int pg = ((pp0 & 3) << 2) | (pp0 >> 2);
        glds16a(Vb + (int64_t)(t + 1) * KB * DH +
                    (uint32_t)(kvr * DH + pg * 8),
                vt(cur ^ 1) + win * 512);
      }
    }

    const bool diag = ((int64_t)(t + 1) * KB) > ((int64_t)qb * QB + wave * WQ);
    // causal skip: every kv in this tile is beyond every q of this wave
    // (varlen adds: or before every document of this wave)
    const bool live =
        ((int64_t)t * KB <= (int64_t)qb * QB + wave * WQ + (WQ - 1)) &&
        (!DOC || (int64_t)(t + 1) * KB > ds_wave);

    // One 32-kv subtile. MASK is a compile-time tag: the masked body applies
    // the causal (and, for DOC, the document lower-bound) compare+select per
    // score, the unmasked body has neither. For kv tiles fully below the
    // diagonal the causal compare never fires, so both bodies compute the
    // same values there.
    auto subtile = [&](auto mask_tag, const int sub)
                       __attribute__((always_inline)) {
      constexpr bool MASK = decltype(mask_tag)::value;
      // ---- S^T = K·Q^T over 8 d-chunks
      f32x16 sacc = f32x16{};
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        typedef __attribute__((address_space(3))) const bf16frag* lds_frag;
        bf16frag kf = *(lds_frag)(kaddr[c] + sub * 8192);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qreg[c], sacc, 0, 0, 0);
      }

      // ---- scale (+ mask) in the exp2 domain (scale2 = scale*log2e folded
      // into the score multiply; v_exp_f32 IS 2^x). The product is rounded
      // before the max-subtract below, two roundings per score: folding them
      // into one fma is 16 VALU cheaper per subtile but moves O and LSE in
      // the last bit, which the flagship model amplifies to percents of its
      // grad norm within one step (profiles/attn_valu_ab.md), so the
      // roundings stay what they were.
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) p[r] = sacc[r] * scale2;
      if (MASK) {
        const int kv_lim =
            (int)(q_global - (int64_t)t * KB) - sub * 32 - 4 * half;
        const int lo_lim =
            DOC ? ds_l - (int)((int64_t)t * KB) - sub * 32 - 4 * half : 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int idx = (r & 3) + 8 * (r >> 2);
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

      // ---- defer-max (T13): rescale only when some lane's max moved past
      // the threshold (wave-uniform decision via ballot)
      bool need = mt > m_run + DEFER_THR;
      if (__builtin_amdgcn_ballot_w64(need) != 0ull) {
        float m_new = fmaxf(m_run, mt);
        float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int qr = (r & 3) + 8 * (r >> 2) + 4 * half;
          float a_r = __shfl(alpha, qr, 32);
#pragma unroll
          for (int d = 0; d < 4; ++d) oacc[d][r] *= a_r;
        }
      }

      // ---- exponentiate + pack pairs + tree row sum. Raw v_exp_f32: it
      // returns 0 where the result would be an f32 denormal (< 2^-126);
      // such a probability is below half an ulp of any row sum >= 1 and of
      // every bf16 P entry, so the flush cannot reach the output.
      float s8[8];
      uint32_t pk[8];
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        float e0 = __builtin_amdgcn_exp2f(p[r] - m_run);
        float e1 = __builtin_amdgcn_exp2f(p[r + 1] - m_run);
        s8[r >> 1] = e0 + e1;
        pk[r >> 1] = pack_bf16x2(e0, e1);
      }
      float s4a = (s8[0] + s8[1]) + (s8[2] + s8[3]);
      float s4b = (s8[4] + s8[5]) + (s8[6] + s8[7]);
      float psum = s4a + s4b;
      psum += xor32h(psum, half);
      l_run += psum;

      // ---- partner-quad exchange -> P^T A-fragments
      bf16frag pa[2];
#pragma unroll
      for (int mch = 0; mch < 2; ++mch)
        pa[mch] = quad_exchange(pk[4 * mch], pk[4 * mch + 1], pk[4 * mch + 2],
                                pk[4 * mch + 3]);

      // ---- O += P^T · V (B-frags: two 4-kv tr16 reads of the L16 image)
#pragma unroll
      for (int mch = 0; mch < 2; ++mch) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int off = (sub * 32 + mch * 16) * 256;
          typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4t;
          typedef __attribute__((address_space(3))) bf16x4t as3b4;
          bf16x4t r0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (as3b4*)(vaddr[d][0] + off));
          bf16x4t r1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (as3b4*)(vaddr[d][1] + off));
          bf16frag vf =
              __builtin_shufflevector(r0, r1, 0, 1, 2, 3, 4, 5, 6, 7);
          oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[mch], vf, oacc[d], 0, 0, 0);
        }
      }
    };

    // wave-uniform body choice: varlen always masks (its lower bound can
    // cut any tile); plain causal masks only on tiles that touch the diagonal
    if (live) {
      if (DOC || diag) {
        subtile(std::true_type{}, 0);
        subtile(std::true_type{}, 1);
      } else {
        subtile(std::false_type{}, 0);
        subtile(std::false_type{}, 1);
      }
    }

    __syncthreads();
    cur ^= 1;
#pragma unroll
    for (int c = 0; c < 8; ++c) kaddr[c] += flip;
#pragma unroll
    for (int d = 0; d < 4; ++d) vaddr[d][0] += flip, vaddr[d][1] += flip;
    flip = -flip;
  }

  // ---- epilogue: O / l; bf16 store; LSE
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int qr = (r & 3) + 8 * (r >> 2) + 4 * half;
    float l_r = __shfl(l_run, qr, 32);
    float inv = 1.0f / l_r;
    int64_t qg = (int64_t)qb * QB + wave * WQ + qr;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      Ob[qg * os.sr + d * 32 + col] = f2bf(oacc[d][r] * inv);
    }
  }
  if (half == 0) {
    // back to the natural-log domain: LSE = ln2 * (m2 + log2(l))
    Lb[q_global] = 0.6931471805599453f * (m_run + __log2f(l_run));
  }
}

}  // namespace

// strides the kernels can address: 16 B aligned rows (dO is read in b128
// fragments) and a row stride whose in-tile lane offsets fit 32 bits
static int check_ostrides(const void* base, int64_t sb, int64_t sh, int64_t sr) {
  VH_CHECK((reinterpret_cast<uintptr_t>(base) & 15) == 0, "O/dO base not 16 B aligned");
  VH_CHECK(sb >= 0 && sh >= 0 && sr >= DH, "O/dO strides must be >= 0, row >= 128");
  VH_CHECK(sb % 8 == 0 && sh % 8 == 0 && sr % 8 == 0, "O/dO strides %% 8 != 0");
  VH_CHECK(sr <= (1 << 20), "O/dO row stride too large (%lld)", (long long)sr);
  return 0;
}

static int attn_fwd_launch(const uint16_t* Q, const uint16_t* K,
                           const uint16_t* V, uint16_t* O, float* LSE, int B,
                           int Hq, int Hkv, int64_t S, float scale,
                           const int32_t* doc_start, OStrides os,
                           void* stream, const float* sinks = nullptr,
                           bool shared_bounds = false) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(S % QB == 0, "S %% 256 != 0 (pad the sequence)");
  VH_CHECK(Hq % Hkv == 0, "Hq %% Hkv != 0");
  VH_CHECK(doc_start == nullptr || B == 1 || shared_bounds,
           "varlen requires packed B == 1");
  // a softmax scale is positive; zero or negative is a caller's mistake
  VH_CHECK(scale > 0, "scale must be > 0 (got %g)", (double)scale);
  dim3 grid((uint32_t)(S / QB), (uint32_t)(B * Hq));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(512), 65536, s,
                       reinterpret_cast<const bf16_t*>(Q),
                       reinterpret_cast<const bf16_t*>(K),
                       reinterpret_cast<const bf16_t*>(V),
                       reinterpret_cast<bf16_t*>(O), LSE, doc_start, B, Hq,
                       Hkv, S, scale, os, sinks);
  };
  if (sinks) {
    if (doc_start) launch(k_attn_fwd<true, true>);
    else launch(k_attn_fwd<false, true>);
  } else {
    if (doc_start) launch(k_attn_fwd<true, false>);
    else launch(k_attn_fwd<false, false>);
  }
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_attn_fwd_bf16(const uint16_t* Q, const uint16_t* K,
                                const uint16_t* V, uint16_t* O, float* LSE,
                                int B, int Hq, int Hkv, int64_t S, float scale,
                                const int32_t* doc_start, void* stream) {
  return attn_fwd_launch(Q, K, V, O, LSE, B, Hq, Hkv, S, scale, doc_start,
                         head_major(Hq, S), stream);
}

/* vh_attn_fwd_bf16 with O addressed as O + b*o_sb + hq*o_sh + row*o_sr
 * (element strides, D contiguous); LSE stays [B,Hq,S]. */
extern "C" int vh_attn_fwd_ostrided_bf16(
    const uint16_t* Q, const uint16_t* K, const uint16_t* V, uint16_t* O,
    float* LSE, int B, int Hq, int Hkv, int64_t S, float scale,
    const int32_t* doc_start, int64_t o_sb, int64_t o_sh, int64_t o_sr,
    void* stream) {
  if (int rc = check_ostrides(O, o_sb, o_sh, o_sr)) return rc;
  return attn_fwd_launch(Q, K, V, O, LSE, B, Hq, Hkv, S, scale, doc_start,
                         OStrides{o_sb, o_sh, o_sr}, stream);
}

/* vh_attn_fwd_ostrided_bf16 with a key window and attention sinks.
 * lo (nullable): int32 [S], the first visible key of every row, applied to
 * every batch row (B > 1 allowed); monotone non-decreasing, lo[q] <= q.
 * sinks (nullable): fp32 [Hq], one more softmax column per row whose value
 * vector is zero; LSE includes it. */
extern "C" int vh_attn_fwd_win_sink_bf16(
    const uint16_t* Q, const uint16_t* K, const uint16_t* V, uint16_t* O,
    float* LSE, int B, int Hq, int Hkv, int64_t S, float scale,
    const int32_t* lo, const float* sinks, int64_t o_sb, int64_t o_sh,
    int64_t o_sr, void* stream) {
  if (int rc = check_ostrides(O, o_sb, o_sh, o_sr)) return rc;
  return attn_fwd_launch(Q, K, V, O, LSE, B, Hq, Hkv, S, scale, lo,
                         OStrides{o_sb, o_sh, o_sr}, stream, sinks,
                         /*shared_bounds=*/true);
}

// ============================================================================
// Flash attention backward (bf16, causal, GQA, D = 128): split into two
// kernels that keep every accumulator in registers, with no atomics and no
// cross-block reduction.
//   k_attn_bwd_pre   — delta = rowsum(dO*O), lse2 = LSE*log2e.
//   k_attn_bwd_pre4_sink + k_attn_dsinks_finish — the same plus the
//     attention-sink gradient; with a sink-inclusive LSE the two kernels
//     below need no change for sinks, and a key window is their doc_start /
//     doc_end bounds (vh_attn_bwd2_win_bf16).
//   k_attn_bwd_dkv_g — block owns a 64-row kv strip of one KV head, loops the
//     GQA head group and the q tiles from the diagonal; dK/dV in registers.
//   k_attn_bwd_dq    — block owns 128 q rows (wave = 32-q slice), loops kv
//     tiles up to the diagonal; dQ in registers, written once as bf16 (this
//     block is the only contributor).
// Scores are recomputed in both kernels: P = exp2(fma(S, scale2, -lse2[q]))
// with the raw v_exp_f32, dS = P * (dP - delta[q]) * scale. In both, the
// P/dS section between the two MFMA chains exists twice, with and without
// the per-score mask select (tile-local 32-bit compares), picked per tile by
// a wave-uniform diagonal test (varlen: always masked); the MFMA chains are
// shared (profiles/attn_valu_ab.md). A single kernel that shared the scores
// needed a cross-wave dQ reduction through LDS + global atomics, which
// measured 2-4 ms of pure overhead per call (DESIGN.md, round-1 and round-2
// attention results; the retired variants are at commit 49b7734).
// ============================================================================

namespace {

__global__ void k_attn_bwd_pre(const bf16_t* __restrict__ dO,
                               const bf16_t* __restrict__ O,
                               const float* __restrict__ LSE,
                               float* __restrict__ delta,
                               float* __restrict__ lse2, int64_t rows) {
  int wave = (blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  int lane = threadIdx.x & (kWave - 1);
  int num_waves = (gridDim.x * blockDim.x) / kWave;
  for (int64_t r = wave; r < rows; r += num_waves) {
    const bf16x8* d8 = reinterpret_cast<const bf16x8*>(dO + r * DH);
    const bf16x8* o8 = reinterpret_cast<const bf16x8*>(O + r * DH);
    float acc = 0.f;
    if (lane < 16) {
      bf16x8 a = d8[lane], b = o8[lane];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += bf2f(a.v[j]) * bf2f(b.v[j]);
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
    if (lane == 0) {
      delta[r] = acc;
      lse2[r] = LSE[r] * 1.4426950408889634f;
    }
  }
}

// k_attn_bwd_pre with 4 rows per wave (16-lane groups) and strided O/dO.
// The xor butterfly over offsets 8, 4, 2, 1 gives every lane of a group the
// sum lane 0 gets from the __shfl_down chain above (same tree; a + b == b + a),
// so delta is bit-equal. r walks the head-major statistics [B,Hq,S].
__global__ __launch_bounds__(256) void k_attn_bwd_pre4(
    const bf16_t* __restrict__ dO, const bf16_t* __restrict__ O,
    const float* __restrict__ LSE, float* __restrict__ delta,
    float* __restrict__ lse2, int64_t rows, int64_t S, int Hq, OStrides os) {
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane >> 4;
  const int cl = lane & 15;
  const int64_t gw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t r0 = gw * 4; r0 < rows; r0 += nw * 4) {
    const int64_t r = r0 + sub;
    const bool ok = r < rows;
    float acc = 0.f;
    if (ok) {
      const int64_t s = r % S;
      const int64_t bh = r / S;
      const int64_t off = (bh / Hq) * os.sb + (bh % Hq) * os.sh + s * os.sr;
      bf16x8 a = reinterpret_cast<const bf16x8*>(dO + off)[cl];
      bf16x8 b = reinterpret_cast<const bf16x8*>(O + off)[cl];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += bf2f(a.v[j]) * bf2f(b.v[j]);
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
    if (ok && cl == 0) {
      delta[r] = acc;
      lse2[r] = LSE[r] * 1.4426950408889634f;
    }
  }
}

// k_attn_bwd_pre4 plus the gradient of the attention sinks,
//   dsinks[h] = -sum_{b,s} exp(sinks[h] - LSE[b,h,s]) * delta[b,h,s]
// (the sink column's probability times -delta; its dP is 0 because its value
// vector is zero). Grid (S/256, B*Hq): a block owns 256 rows of one (b, h),
// wave w and 16-lane group g take row it*16 + w*4 + g of them in pass it, so
// delta is k_attn_bwd_pre4's bit for bit. Every block writes one partial
// (part[bh*nblk + blk]); the sums inside a block and in k_attn_dsinks_finish
// run in a fixed order and use no atomics, so dsinks is the same from run to
// run and for every O/dO layout.
__global__ __launch_bounds__(256) void k_attn_bwd_pre4_sink(
    const bf16_t* __restrict__ dO, const bf16_t* __restrict__ O,
    const float* __restrict__ LSE, const float* __restrict__ sinks,
    float* __restrict__ delta, float* __restrict__ lse2,
    float* __restrict__ part, int64_t S, int Hq, OStrides os) {
  __shared__ float red[4];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> 4;
  const int cl = lane & 15;
  const int64_t bh = blockIdx.y;
  const int hq = (int)(bh % Hq);
  const int64_t base = (bh / Hq) * os.sb + hq * os.sh;
  const float sink = sinks[hq];
  float gacc = 0.f;   // this 16-lane group's share, the same in its lanes
  for (int it = 0; it < 16; ++it) {
    const int64_t s = (int64_t)blockIdx.x * 256 + it * 16 + wave * 4 + sub;
    const int64_t r = bh * S + s;
    const int64_t off = base + s * os.sr;
    bf16x8 a = reinterpret_cast<const bf16x8*>(dO + off)[cl];
    bf16x8 b = reinterpret_cast<const bf16x8*>(O + off)[cl];
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += bf2f(a.v[j]) * bf2f(b.v[j]);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
    const float lse = LSE[r];
    if (cl == 0) {
      delta[r] = acc;
      lse2[r] = lse * 1.4426950408889634f;
    }
    gacc += expf(sink - lse) * acc;
  }
  const float g0 = __shfl(gacc, 0, kWave), g1 = __shfl(gacc, 16, kWave);
  const float g2 = __shfl(gacc, 32, kWave), g3 = __shfl(gacc, 48, kWave);
  if (lane == 0) red[wave] = (g0 + g1) + (g2 + g3);
  __syncthreads();
  if (threadIdx.x == 0)
    part[bh * gridDim.x + blockIdx.x] = -((red[0] + red[1]) + (red[2] + red[3]));
}

// dsinks[h] = sum over b, then blocks, of part[(b*Hq + h)*nblk + blk], in
// that order: one thread per head.
__global__ void k_attn_dsinks_finish(const float* __restrict__ part,
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

// dK/dV: GQA-folded on the 64-kv-strip geometry.
//   - grid (S/64, B*Hkv): a block owns a 64-row kv strip of ONE KV head and
//     loops the whole GQA head group (rep = Hq/Hkv) — dK/dV are written ONCE
//     to the [B,Hkv,S,D] buffers (no per-Q-head intermediates, no host group
//     sum) and the K/V staging amortizes over the group. The strip split
//     keeps the grid at >= 2 blocks/CU even at B = 1: folding on 128-kv
//     blocks (256 blocks at the llama microbench shape) measured ~2.45 ms
//     from half-empty wave slots vs 1.78 ms unfolded — occupancy beat
//     traffic.
//   - 4 waves = (2 kv slices) x (2 q subtiles of a 64-row staged q tile):
//     each wave owns a distinct 32x32 quadrant; barrier cadence halves per
//     unit of work vs 32-row q tiles.
//   - DOC: packed-varlen block-diagonal causal via doc_start/doc_end
//     (per-token document bounds; see k_attn_fwd).
//   - Staging: the Q/dO tiles sit in LDS in natural [64 q][128 d] layout as
//     the L16 latin-square image
//       off(q,d) = q*256 + L16*16 + (d&7)*2,
//       L16 = (q&15) ^ (((p&3)<<2)|(p>>2)), p = d>>3,
//     filled by global_load_lds straight into LDS (lane-linear destination,
//     per-lane permuted sources: no staging VGPRs, no ds_writes). The image
//     is conflict-free for both the CDNA4 ds_read_b64_tr_b16 hardware-
//     transpose reads that feed the dV/dK B-fragments (guide T10) and the
//     plain b128 reads of the Q/dO A-fragments, so nothing re-reads global.
//     Why this scheme: on the previous scalar-transpose staging SQ_WAIT_ANY
//     was 66% of wave cycles, waves parked at the per-tile barrier pair
//     draining the staging loads (profiles/r02_dkv_pmc_sq.csv); this one
//     measured -47% cumulative and is bit-identical (DESIGN.md, round-2
//     outcomes). Register prefetch and register double-buffering of the
//     staging were measured and lost; see DESIGN.md.
//   - Per tile the 64 lse2 / delta (varlen: doc_start) values of the q tile
//     are dropped into LDS by one-dword glds next to the images; a lane
//     fetches the 16 rows its scores belong to with four b128 broadcast
//     reads per quantity (earlier: two ds_bpermute per score).
//   - The quadrant body exists twice, chosen per tile by the wave-uniform
//     `diag`: with and without the per-score mask select.
// LDS 64.75 KB: K/V strips 2x16 K + Q/dO tiles 2x16 K + 768 B of per-row
// scalars -> still 2 blocks/CU (160 KiB).
template <bool DOC>
__global__ __launch_bounds__(256, 2) void k_attn_bwd_dkv_g(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
    const float* __restrict__ delta, const float* __restrict__ lse2,
    bf16_t* __restrict__ dK, bf16_t* __restrict__ dV,
    const int* __restrict__ doc_start, const int* __restrict__ doc_end, int B,
    int Hq, int Hkv, int64_t S, float scale, OStrides dos) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* krow = reinterpret_cast<bf16_t*>(smem);            // [64][128] 16 K
  bf16_t* vrow = reinterpret_cast<bf16_t*>(smem + 16384);    // [64][128] 16 K
  bf16_t* qtr = reinterpret_cast<bf16_t*>(smem + 32768);     // [64][128] L16 16 K
  bf16_t* dotr = reinterpret_cast<bf16_t*>(smem + 49152);    // [64][128] L16 16 K
  float* stat = reinterpret_cast<float*>(smem + 65536);      // 3 x [64] dwords
  float* red = reinterpret_cast<float*>(smem);               // epilogue reuse

  const int kvb = blockIdx.x;          // 64-row kv strip
  const int bkh = blockIdx.y;          // b * Hkv + hkv
  const int b = bkh / Hkv;
  const int hkv = bkh % Hkv;
  const int rep = Hq / Hkv;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int kvslice = wave & 1;        // 32-kv slice within the strip
  const int qsub = wave >> 1;          // 32-q subtile within the 64-q tile
  const int half = lane >> 5;
  const int col = lane & 31;

  const bf16_t* Kb = K + (((int64_t)b * Hkv + hkv) * S) * DH;
  const bf16_t* Vb = V + (((int64_t)b * Hkv + hkv) * S) * DH;
  bf16_t* dKb = dK + (((int64_t)b * Hkv + hkv) * S) * DH;
  bf16_t* dVb = dV + (((int64_t)b * Hkv + hkv) * S) * DH;

  const int64_t kv0 = (int64_t)kvb * 64;
  const int kvrow_l = kvslice * 32 + col;

  // stage the strip's 64 K/V rows once (256 thr: 4 passes of 4 KiB each)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int o = i * 4096 + tid * 16;
    int row = o >> 8;
    int colb = o & 255;
    *reinterpret_cast<bf16x8*>(
        reinterpret_cast<char*>(krow) + row * 256 + kswz(row, colb)) =
        *reinterpret_cast<const bf16x8*>(Kb + (kv0 + row) * DH + (colb >> 1));
    *reinterpret_cast<bf16x8*>(
        reinterpret_cast<char*>(vrow) + row * 256 + kswz(row, colb)) =
        *reinterpret_cast<const bf16x8*>(Vb + (kv0 + row) * DH + (colb >> 1));
  }

  f32x16 dv_acc[4], dk_acc[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    dv_acc[d] = f32x16{};
    dk_acc[d] = f32x16{};
  }

  const float scale2 = scale * 1.4426950408889634f;
  const int qt0 = (int)(kv0 / 64);     // 64-row q tiles
  int qtn = (int)(S / 64);
  int de_wave = 0;
  if (DOC) {
    qtn = (doc_end[kv0 + 63] + 63) / 64;          // block-uniform end
    de_wave = doc_end[kv0 + kvslice * 32 + 31];   // wave-live bound
  }

  // single flattened loop over (head g, q tile): one live address chain —
  // a nested g/qt loop form kept per-head pointer sets alive across the
  // whole accumulator section and spilled ~190 extra bytes/lane
  const int ntiles = qtn - qt0;
  const int itn = rep * ntiles;
  for (int it = 0; it < itn; ++it) {
    const int g = it / ntiles;
    const int qt = qt0 + (it - g * ntiles);
    {
      const int hq = hkv * rep + g;
      const bf16_t* Qb = Q + (((int64_t)b * Hq + hq) * S) * DH;
      const bf16_t* dOb = dO + b * dos.sb + hq * dos.sh;
      const float* delb = delta + ((int64_t)b * Hq + hq) * S;
      const float* lseb = lse2 + ((int64_t)b * Hq + hq) * S;
      const int64_t q0t = (int64_t)qt * 64;
      const int64_t q0 = q0t + qsub * 32;   // this wave's 32-q subtile
      // stage the Q / dO tiles [64 q][128 d]: glds fill of the L16 image.
      // Window win = wave*4+u covers 4 q rows (1024 B, lane-linear dest);
      // lane sources pair p = P(slot ^ (q&15)) — zero VGPR staging, zero
      // ds_writes
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int win = wave * 4 + u;
        const int qrow = win * 4 + (lane >> 4);
        const int pp0 = (lane & 15) ^ (qrow & 15);
        const int pg = ((pp0 & 3) << 2) | (pp0 >> 2);
        // uniform tile base + 32-bit lane offset (scalar-base addressing)
        const uint32_t loff = (uint32_t)(qrow * DH + pg * 8);
        glds16a(Qb + q0t * DH + loff, qtr + win * 512);
      }
      // dO rows are dos.sr elements apart, so its lane offsets are its own.
      // They are rebuilt per tile behind an opaque move and issued after the
      // Q loads: sharing the loop with Q, or letting them hoist, costs VGPRs
      // the accumulator section does not have (scratch 0 -> 8..64 B/lane).
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int win = wave * 4 + u;
        uint32_t qrow = win * 4 + (lane >> 4);
        asm volatile("" : "+v"(qrow));
        const uint32_t pp0 = (lane & 15) ^ (qrow & 15);
        const uint32_t pg = ((pp0 & 3) << 2) | (pp0 >> 2);
        glds16a(dOb + q0t * dos.sr + (uint32_t)(qrow * (uint32_t)dos.sr + pg * 8),
                dotr + win * 512);
      }
      // the tile's 64 lse2 / delta (and, varlen, doc_start) values go to LDS
      // next to the images: one dword per lane, waves 0 / 1 / 2
      if (wave == 0) glds4(lseb + q0t + (uint32_t)lane, stat);
      else if (wave == 1) glds4(delb + q0t + (uint32_t)lane, stat + 64);
      else if (DOC && wave == 2)
        glds4(doc_start + q0t + (uint32_t)lane, stat + 128);
      __syncthreads();

      const bool live = ((q0 + 31) >= (kv0 + kvslice * 32)) &&
                        (!DOC || q0 < de_wave);
      const bool diag = (q0 < kv0 + 64);
      if (live) {
        f32x16 s2 = f32x16{}, dp2 = f32x16{};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          int colb = (c * 16 + half * 8) * 2;
          // A-frags from the staged L16 image (conflict-free b128):
          // chunk pair p = c*2 + half, row q0+col
          const int pp = c * 2 + half;
          const int rl = qsub * 32 + col;  // local image row
          const int l16 = (rl & 15) ^ (((pp & 3) << 2) | (pp >> 2));
          bf16frag dc = *reinterpret_cast<const bf16frag*>(
              reinterpret_cast<const char*>(dotr) + rl * 256 + l16 * 16);
          bf16frag qc = *reinterpret_cast<const bf16frag*>(
              reinterpret_cast<const char*>(qtr) + rl * 256 + l16 * 16);
          bf16frag kf = *reinterpret_cast<const bf16frag*>(
              reinterpret_cast<const char*>(krow) + kvrow_l * 256 + kswz(kvrow_l, colb));
          bf16frag vf = *reinterpret_cast<const bf16frag*>(
              reinterpret_cast<const char*>(vrow) + kvrow_l * 256 + kswz(kvrow_l, colb));
          s2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qc, kf, s2, 0, 0, 0);
          dp2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dc, vf, dp2, 0, 0, 0);
        }
        // P and dS of the quadrant, packed to bf16 pairs. MASK is a
        // compile-time tag: the masked body applies the causal (and, for
        // DOC, the document lower-bound) select per score with tile-local
        // 32-bit indices, the unmasked body has none. Below the diagonal the
        // causal compare never fires, so both bodies compute the same values
        // there. Only this section exists twice; the MFMA chains around it
        // are shared (whole-quadrant duplicates spilled ~120 dwords/lane).
        uint32_t pk2[8], dg2[8];
        auto pds_pack = [&](auto mask_tag) __attribute__((always_inline)) {
          constexpr bool MASK = decltype(mask_tag)::value;
          // tile-local mask bounds: kv row kvl of the strip is masked for q row
          // idx + 4*half of the subtile when kvl > (q0 - kv0) + idx + 4*half
          const int kvl = kvslice * 32 + col;
          const int c_lim = kvl - (int)(q0 - kv0) - 4 * half;
          const int kv_abs = (int)kv0 + kvl;
          // per-score softmax scalars: score r belongs to q row
          // (r&3) + 8*(r>>2) + 4*half of the subtile, i.e. four runs of four
          // consecutive rows -> one b128 broadcast read per run and quantity.
          // The runs are kept apart (sched_barrier) so that at most one run's
          // scalars are live next to the 128 accumulator registers.
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int qr4 = qsub * 32 + 8 * j + 4 * half;
            const float4 l4 = *reinterpret_cast<const float4*>(stat + qr4);
            const float4 d4 = *reinterpret_cast<const float4*>(stat + 64 + qr4);
            const float lse_q[4] = {l4.x, l4.y, l4.z, l4.w};
            const float del_q[4] = {d4.x, d4.y, d4.z, d4.w};
            int ds_q[4] = {0, 0, 0, 0};
            if (MASK && DOC) {
              const int4 s4 = *reinterpret_cast<const int4*>(
                  reinterpret_cast<const int*>(stat) + 128 + qr4);
              ds_q[0] = s4.x, ds_q[1] = s4.y, ds_q[2] = s4.z, ds_q[3] = s4.w;
            }
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
              float pv[2], gv[2];
#pragma unroll
              for (int rr = 0; rr < 2; ++rr) {
                const int i = 2 * h2 + rr;
                const int r2 = 4 * j + i;
                // raw v_exp_f32: flushes results below 2^-126 to 0, which is
                // below the bf16 rounding of every P and dS entry they feed
                float pp = __builtin_amdgcn_exp2f(
                    __builtin_fmaf(s2[r2], scale2, -lse_q[i]));
                if (MASK) {
                  const int idx = i + 8 * j;
                  bool masked = idx < c_lim;
                  if (DOC) masked = masked || (kv_abs < ds_q[i]);
                  pp = masked ? 0.f : pp;
                }
                pv[rr] = pp;
                gv[rr] = pp * (dp2[r2] - del_q[i]) * scale;
              }
              pk2[2 * j + h2] = pack_bf16x2(pv[0], pv[1]);
              dg2[2 * j + h2] = pack_bf16x2(gv[0], gv[1]);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        };
        // wave-uniform choice (varlen always masks: its lower bound can cut
        // any tile)
        if (DOC || diag) pds_pack(std::true_type{});
        else pds_pack(std::false_type{});
        bf16frag pa2[2], da2[2];
#pragma unroll
        for (int mch = 0; mch < 2; ++mch) {
          pa2[mch] = quad_exchange(pk2[4 * mch], pk2[4 * mch + 1],
                                   pk2[4 * mch + 2], pk2[4 * mch + 3]);
          da2[mch] = quad_exchange(dg2[4 * mch], dg2[4 * mch + 1],
                                   dg2[4 * mch + 2], dg2[4 * mch + 3]);
        }
        // B-frags: two 4-q hardware-transpose reads per frag from this wave's
        // half of the 64-row image; lane m of each 16-lane group supplies
        // (q = qr_+(m>>2), 8-B slot c_r) and receives (q = qr_+0..3,
        // d = dblk*32 + lane%16 (+16))
#pragma unroll
        for (int mch = 0; mch < 2; ++mch) {
#pragma unroll
          for (int dblk = 0; dblk < 4; ++dblk) {
            const int m_ = lane & 15;
            const int colhi_ = (lane >> 4) & 1;
            const int qr_ = qsub * 32 + mch * 16 + half * 8 + (m_ >> 2);
            const int c_r = dblk * 8 + colhi_ * 4 + (m_ & 3);
            const int perm_c = (((c_r >> 1) & 3) << 2) | (c_r >> 3);
            const int l16a = (qr_ & 15) ^ perm_c;
            const int l16b = ((qr_ + 4) & 15) ^ perm_c;  // q&15 changes at +4
            const int a0 = qr_ * 256 + l16a * 16 + (c_r & 1) * 8;
            const int a1 = (qr_ + 4) * 256 + l16b * 16 + (c_r & 1) * 8;
            auto* dob3 = (__attribute__((address_space(3))) char*)dotr;
            auto* qb3 = (__attribute__((address_space(3))) char*)qtr;
            typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4t;
            typedef __attribute__((address_space(3))) bf16x4t as3b4;
            bf16x4t d0v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (as3b4*)(dob3 + a0));
            bf16x4t d1v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (as3b4*)(dob3 + a1));
            bf16x4t q0v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (as3b4*)(qb3 + a0));
            bf16x4t q1v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (as3b4*)(qb3 + a1));
            bf16frag dof =
                __builtin_shufflevector(d0v, d1v, 0, 1, 2, 3, 4, 5, 6, 7);
            bf16frag qf =
                __builtin_shufflevector(q0v, q1v, 0, 1, 2, 3, 4, 5, 6, 7);
            dv_acc[dblk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa2[mch], dof, dv_acc[dblk], 0, 0, 0);
            dk_acc[dblk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da2[mch], qf, dk_acc[dblk], 0, 0, 0);
          }
        }
      }
      __syncthreads();
    }
  }

  // combine the two q-subtile partials per kv slice through LDS, then store.
  // red layout: [slice 2][lane 64][64 floats] = 32 KB (reuses K/V space —
  // every wave has passed the loop-final barrier). Written out directly per
  // accumulator (no pointer indirection: an f32x16* into the accumulator
  // arrays sent all 128 accumulator VGPRs to scratch).
#define VH_DKVG_COMBINE(ACC, DST)                                             \
  {                                                                           \
    if (qsub == 1) {                                                          \
      float* out = red + (kvslice * 64 + lane) * 64;                          \
      _Pragma("unroll") for (int d = 0; d < 4; ++d)                           \
          _Pragma("unroll") for (int r = 0; r < 16; r += 4)                   \
              *reinterpret_cast<float4*>(out + d * 16 + r) = float4{          \
                  ACC[d][r], ACC[d][r + 1], ACC[d][r + 2], ACC[d][r + 3]};    \
    }                                                                         \
    __syncthreads();                                                          \
    if (qsub == 0) {                                                          \
      const float* in = red + (kvslice * 64 + lane) * 64;                     \
      _Pragma("unroll") for (int d = 0; d < 4; ++d)                           \
          _Pragma("unroll") for (int r = 0; r < 16; ++r) ACC[d][r] +=         \
          in[d * 16 + r];                                                     \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                        \
        int kvr = (r & 3) + 8 * (r >> 2) + 4 * half;                          \
        int64_t kvg = kv0 + kvslice * 32 + kvr;                               \
        _Pragma("unroll") for (int d = 0; d < 4; ++d) DST[kvg * DH + d * 32 + \
                                                          col] =             \
            f2bf(ACC[d][r]);                                                  \
      }                                                                       \
    }                                                                         \
    __syncthreads();                                                          \
  }
  VH_DKVG_COMBINE(dv_acc, dVb)
  VH_DKVG_COMBINE(dk_acc, dKb)
#undef VH_DKVG_COMBINE
}

// dQ: block owns 128 q rows (wave = 32-q slice) of one Q head; the wave's
// Q/dO rows, lse and delta stay in registers for the whole kernel.
// Per 32-row kv tile the stage is three glds-filled images: K and V rows in
// the kswz layout (A-frags of S = K·Q^T and dP = V·dO^T) and K again as the
// L16 latin-square image (see k_attn_bwd_dkv_g) whose tr16 hardware-
// transpose reads supply the K^T B-frags of dQ += dS^T·K. The three images
// are DOUBLE buffered (2 x 24 KiB) and filled one kv tile ahead with a
// single barrier per tile, so the staging drain is off the barrier path
// (measurements in DESIGN.md, round-2 outcomes). Per tile: S/dP chain (16
// MFMA), the dS section (masked or unmasked, see the section header above),
// pack + partner-quad exchange, dQ chain (8 MFMA). The K/V/K^T read
// addresses stay base-plus-tile-offset adds: with one 32-row tile per
// iteration a carried, flipped address costs the same one add per base.
template <bool DOC>
__global__ __launch_bounds__(256, 2) void k_attn_bwd_dq(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
    const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
    const float* __restrict__ delta, const float* __restrict__ lse2,
    bf16_t* __restrict__ dQ, const int* __restrict__ doc_start, int B, int Hq,
    int Hkv, int64_t S, float scale, OStrides dos) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // two buffer sets of 24 KiB (the launch carves 48 KiB), each:
  //   +0     krow [32][128] kswz  8 K
  //   +8192  vrow [32][128] kswz  8 K
  //   +16384 ktr  [32][128] L16   8 K

  const int qb = blockIdx.x;           // q block of 128 rows
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;           // 32-row q slice
  const int half = lane >> 5;
  const int col = lane & 31;

  const bf16_t* Qb = Q + (((int64_t)b * Hq + hq) * S) * DH;
  const bf16_t* Kb = K + (((int64_t)b * Hkv + hkv) * S) * DH;
  const bf16_t* Vb = V + (((int64_t)b * Hkv + hkv) * S) * DH;
  const bf16_t* dOb = dO + b * dos.sb + hq * dos.sh;
  const float* delb = delta + ((int64_t)b * Hq + hq) * S;
  const float* lseb = lse2 + ((int64_t)b * Hq + hq) * S;
  bf16_t* dQb = dQ + (((int64_t)b * Hq + hq) * S) * DH;

  const int64_t q0b = (int64_t)qb * 128;
  const int64_t q_l = q0b + wave * 32 + col;   // this lane's q row

  // the wave's Q/dO rows and lse/delta are fixed for the whole kernel
  bf16frag qrow[8], dorow[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    qrow[c] = *reinterpret_cast<const bf16frag*>(Qb + q_l * DH + c * 16 + half * 8);
    dorow[c] = *reinterpret_cast<const bf16frag*>(dOb + q_l * dos.sr + c * 16 + half * 8);
  }
  const float lse_l = lseb[q_l];
  const float del_l = delb[q_l];
  const float scale2 = scale * 1.4426950408889634f;

  int ds_l = 0, ds_wave = 0, kvt_begin = 0;
  if (DOC) {
    ds_l = doc_start[q_l];
    ds_wave = doc_start[q0b + wave * 32];
    kvt_begin = doc_start[q0b] / 32;
  }

  f32x16 dq4[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) dq4[d] = f32x16{};

  const int kvtn = (int)((q0b + 128) / 32);
  // glds one whole tile set (krow/vrow kswz + ktr L16) into buffer BF
#define VH_DQ_STAGE(KVT2, BF)                                                  \
  {                                                                            \
    const int64_t kv0_ = (int64_t)(KVT2) * 32;                                 \
    char* kb_ = reinterpret_cast<char*>(smem) + (BF) * 24576;                  \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                            \
      const int win_ = wave * 2 + u;                                           \
      const int row_ = win_ * 4 + (lane >> 4);                                 \
      const int c16_ = (lane & 15) ^ (row_ & 15);                              \
      const int pg_ = (((c16_ & 3) << 2) | (c16_ >> 2));                       \
      /* uniform tile base + 32-bit lane offset (scalar-base addressing) */    \
      const uint32_t lo_ = (uint32_t)(row_ * DH + c16_ * 8);                   \
      const uint32_t lp_ = (uint32_t)(row_ * DH + pg_ * 8);                    \
      glds16a(Kb + kv0_ * DH + lo_,                                            \
              reinterpret_cast<bf16_t*>(kb_) + win_ * 512);                    \
      glds16a(Vb + kv0_ * DH + lo_,                                            \
              reinterpret_cast<bf16_t*>(kb_ + 8192) + win_ * 512);             \
      glds16a(Kb + kv0_ * DH + lp_,                                            \
              reinterpret_cast<bf16_t*>(kb_ + 16384) + win_ * 512);            \
    }                                                                          \
  }
  int cur = 0;
  if (kvt_begin < kvtn) VH_DQ_STAGE(kvt_begin, 0);
  __syncthreads();
  for (int kvt = kvt_begin; kvt < kvtn; ++kvt) {
    const int64_t kvt0 = (int64_t)kvt * 32;
    char* base_ = reinterpret_cast<char*>(smem) + cur * 24576;
    const bf16_t* krow = reinterpret_cast<bf16_t*>(base_);
    const bf16_t* vrow = reinterpret_cast<bf16_t*>(base_ + 8192);
    const bf16_t* ktr = reinterpret_cast<bf16_t*>(base_ + 16384);
    if (kvt + 1 < kvtn) VH_DQ_STAGE(kvt + 1, cur ^ 1);

    const bool live = (kvt0 <= q0b + wave * 32 + 31) &&
                      (!DOC || kvt0 + 31 >= ds_wave);
    const bool diag = (kvt0 + 31 >= q0b + wave * 32);

    if (live) {
      // or1: C = [kv regs][q lanes]; s1 = mfma(K, Q)
      f32x16 s1 = f32x16{}, dp1 = f32x16{};
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        int colb = (c * 16 + half * 8) * 2;
        bf16frag kf = *reinterpret_cast<const bf16frag*>(
            reinterpret_cast<const char*>(krow) + col * 256 + kswz(col, colb));
        bf16frag vf = *reinterpret_cast<const bf16frag*>(
            reinterpret_cast<const char*>(vrow) + col * 256 + kswz(col, colb));
        s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qrow[c], s1, 0, 0, 0);
        dp1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dorow[c], dp1, 0, 0, 0);
      }
      // dS of the tile, packed to bf16 pairs. MASK is a compile-time tag:
      // the masked body applies the causal (and, for DOC, the document
      // lower-bound) select per score with tile-local 32-bit indices, the
      // unmasked body has none. Below the diagonal the causal compare never
      // fires, so both bodies compute the same values there. Only this
      // section exists twice; the MFMA chains around it are shared (whole-
      // tile duplicates spilled the resident Q/dO fragments).
      uint32_t dg1[8];
      auto ds_pack = [&](auto mask_tag) __attribute__((always_inline)) {
        constexpr bool MASK = decltype(mask_tag)::value;
        // tile-local mask bounds: kv row idx + 4*half of the tile is masked
        // when it lies past this lane's q row or before its document
        const int c_lim = (int)(q_l - kvt0) - 4 * half;
        const int lo_lim = DOC ? ds_l - (int)kvt0 - 4 * half : 0;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          float g[2];
#pragma unroll
          for (int rr = 0; rr < 2; ++rr) {
            int r2 = r + rr;
            // raw v_exp_f32: flushes results below 2^-126 to 0, which is
            // below the bf16 rounding of every dS entry they feed
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
      // wave-uniform choice (varlen always masks: its lower bound can cut
      // any tile)
      if (DOC || diag) ds_pack(std::true_type{});
      else ds_pack(std::false_type{});
      bf16frag da1[2];
#pragma unroll
      for (int mch = 0; mch < 2; ++mch) {
        da1[mch] = quad_exchange(dg1[4 * mch], dg1[4 * mch + 1],
                                 dg1[4 * mch + 2], dg1[4 * mch + 3]);
      }
      // dQ[q][d] += dS1^T(pack) x K^T-tile
#pragma unroll
      for (int dblk = 0; dblk < 4; ++dblk) {
#pragma unroll
        for (int mch = 0; mch < 2; ++mch) {
          const int m_ = lane & 15;
          const int colhi_ = (lane >> 4) & 1;
          const int kvb0 = mch * 16 + half * 8 + (m_ >> 2);
          const int c_r = dblk * 8 + colhi_ * 4 + (m_ & 3);
          const int perm_ = (((c_r >> 1) & 3) << 2) | (c_r >> 3);
          const int a0 =
              kvb0 * 256 + ((kvb0 & 15) ^ perm_) * 16 + (c_r & 1) * 8;
          const int a1 = (kvb0 + 4) * 256 +
                         (((kvb0 + 4) & 15) ^ perm_) * 16 + (c_r & 1) * 8;
          auto* kb3 = (__attribute__((address_space(3))) char*)ktr;
          typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4t;
          typedef __attribute__((address_space(3))) bf16x4t as3b4;
          bf16x4t r0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (as3b4*)(kb3 + a0));
          bf16x4t r1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (as3b4*)(kb3 + a1));
          bf16frag ktf =
              __builtin_shufflevector(r0, r1, 0, 1, 2, 3, 4, 5, 6, 7);
          dq4[dblk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da1[mch], ktf, dq4[dblk], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }
#undef VH_DQ_STAGE

  // single-contributor store: this block covers every kv for its q rows
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int qr = (r & 3) + 8 * (r >> 2) + 4 * half;
    int64_t qg = q0b + wave * 32 + qr;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      dQb[qg * DH + d * 32 + col] = f2bf(dq4[d][r]);
    }
  }
}

}  // namespace

extern "C" int vh_attn_bwd_pre_bf16(const uint16_t* dO, const uint16_t* O,
                                    const float* LSE, float* delta,
                                    float* lse2, int64_t rows, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int blocks = (int)((rows + 3) / 4);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_attn_bwd_pre, dim3(blocks), dim3(256), 0, s,
                     reinterpret_cast<const bf16_t*>(dO),
                     reinterpret_cast<const bf16_t*>(O), LSE, delta, lse2, rows);
  VH_HIP(hipGetLastError());
  return 0;
}

/* vh_attn_bwd_pre_bf16 over O and dO addressed as base + b*sb + hq*sh +
 * row*sr (one layout for both); delta and lse2 stay [B,Hq,S]. */
extern "C" int vh_attn_bwd_pre_ostrided_bf16(
    const uint16_t* dO, const uint16_t* O, const float* LSE, float* delta,
    float* lse2, int B, int Hq, int64_t S, int64_t o_sb, int64_t o_sh,
    int64_t o_sr, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = check_ostrides(dO, o_sb, o_sh, o_sr)) return rc;
  if (int rc = check_ostrides(O, o_sb, o_sh, o_sr)) return rc;
  int64_t rows = (int64_t)B * Hq * S;
  int blocks = (int)((rows + 15) / 16);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_attn_bwd_pre4, dim3(blocks), dim3(256), 0, s,
                     reinterpret_cast<const bf16_t*>(dO),
                     reinterpret_cast<const bf16_t*>(O), LSE, delta, lse2, rows,
                     S, Hq, OStrides{o_sb, o_sh, o_sr});
  VH_HIP(hipGetLastError());
  return 0;
}

/* vh_attn_bwd_pre_ostrided_bf16 that also returns the attention-sink
 * gradient. sinks (nullable, fp32 [Hq]): with it, dsinks (fp32 [Hq]) is
 * written and partials (fp32 [B*Hq*S/256], workspace) is used; LSE must be
 * the sink-inclusive one of vh_attn_fwd_win_sink_bf16. Without it the call
 * is vh_attn_bwd_pre_ostrided_bf16. S % 256 == 0. */
extern "C" int vh_attn_bwd_pre_sink_bf16(
    const uint16_t* dO, const uint16_t* O, const float* LSE,
    const float* sinks, float* delta, float* lse2, float* dsinks,
    float* partials, int B, int Hq, int64_t S, int64_t o_sb, int64_t o_sh,
    int64_t o_sr, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(S > 0 && S % 256 == 0, "S %% 256 != 0 (pad the sequence)");
  VH_CHECK(B > 0 && Hq > 0, "B, Hq must be > 0");
  if (sinks == nullptr)
    return vh_attn_bwd_pre_ostrided_bf16(dO, O, LSE, delta, lse2, B, Hq, S,
                                         o_sb, o_sh, o_sr, stream);
  VH_CHECK(dsinks != nullptr && partials != nullptr,
           "sinks need the dsinks output and the partials workspace");
  if (int rc = check_ostrides(dO, o_sb, o_sh, o_sr)) return rc;
  if (int rc = check_ostrides(O, o_sb, o_sh, o_sr)) return rc;
  const int nblk = (int)(S / 256);
  hipLaunchKernelGGL(k_attn_bwd_pre4_sink, dim3(nblk, (uint32_t)(B * Hq)),
                     dim3(256), 0, s, reinterpret_cast<const bf16_t*>(dO),
                     reinterpret_cast<const bf16_t*>(O), LSE, sinks, delta,
                     lse2, partials, S, Hq, OStrides{o_sb, o_sh, o_sr});
  VH_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_attn_dsinks_finish, dim3((Hq + 63) / 64), dim3(64), 0,
                     s, partials, dsinks, B, Hq, nblk);
  VH_HIP(hipGetLastError());
  return 0;
}

static int attn_bwd2_launch(const uint16_t* Q, const uint16_t* K,
                            const uint16_t* V, const uint16_t* dO,
                            const float* delta, const float* lse2,
                            uint16_t* dQ, uint16_t* dK, uint16_t* dV, int B,
                            int Hq, int Hkv, int64_t S, float scale,
                            const int32_t* doc_start, const int32_t* doc_end,
                            OStrides dos, void* stream,
                            bool shared_bounds = false) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(S % 128 == 0, "S %% 128 != 0");
  VH_CHECK(Hq % Hkv == 0, "Hq %% Hkv != 0");
  VH_CHECK((doc_start == nullptr) == (doc_end == nullptr),
           "doc_start/doc_end must be passed together");
  VH_CHECK(doc_start == nullptr || B == 1 || shared_bounds,
           "varlen requires packed B == 1");
  dim3 grid_kv((uint32_t)(S / 64), (uint32_t)(B * Hkv));
  dim3 grid_q((uint32_t)(S / 128), (uint32_t)(B * Hq));
  auto launch_dkv = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid_kv, dim3(256), 65536 + 768, s,
                       reinterpret_cast<const bf16_t*>(Q),
                       reinterpret_cast<const bf16_t*>(K),
                       reinterpret_cast<const bf16_t*>(V),
                       reinterpret_cast<const bf16_t*>(dO), delta, lse2,
                       reinterpret_cast<bf16_t*>(dK),
                       reinterpret_cast<bf16_t*>(dV), doc_start, doc_end, B,
                       Hq, Hkv, S, scale, dos);
  };
  auto launch_dq = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid_q, dim3(256), 49152, s,
                       reinterpret_cast<const bf16_t*>(Q),
                       reinterpret_cast<const bf16_t*>(K),
                       reinterpret_cast<const bf16_t*>(V),
                       reinterpret_cast<const bf16_t*>(dO), delta, lse2,
                       reinterpret_cast<bf16_t*>(dQ), doc_start, B, Hq, Hkv,
                       S, scale, dos);
  };
  if (doc_start) launch_dkv(k_attn_bwd_dkv_g<true>);
  else launch_dkv(k_attn_bwd_dkv_g<false>);
  VH_HIP(hipGetLastError());
  if (doc_start) launch_dq(k_attn_bwd_dq<true>);
  else launch_dq(k_attn_bwd_dq<false>);
  VH_HIP(hipGetLastError());
  return 0;
}

/* Split backward: GQA-folded dkv (dK/dV [B,Hkv,S,D] written once — no
 * per-Q-head intermediates, no host group sum) + per-Q-head dq.
 * doc_start/doc_end (nullable, B == 1) select the packed-varlen
 * block-diagonal causal mask. */
extern "C" int vh_attn_bwd2_bf16(const uint16_t* Q, const uint16_t* K,
                                 const uint16_t* V, const uint16_t* dO,
                                 const float* delta, const float* lse2,
                                 uint16_t* dQ, uint16_t* dK, uint16_t* dV,
                                 int B, int Hq, int Hkv, int64_t S, float scale,
                                 const int32_t* doc_start,
                                 const int32_t* doc_end, void* stream) {
  return attn_bwd2_launch(Q, K, V, dO, delta, lse2, dQ, dK, dV, B, Hq, Hkv, S,
                          scale, doc_start, doc_end, head_major(Hq, S), stream);
}

/* vh_attn_bwd2_bf16 with dO addressed as dO + b*do_sb + hq*do_sh + row*do_sr
 * (element strides, D contiguous). */
extern "C" int vh_attn_bwd2_ostrided_bf16(
    const uint16_t* Q, const uint16_t* K, const uint16_t* V, const uint16_t* dO,
    const float* delta, const float* lse2, uint16_t* dQ, uint16_t* dK,
    uint16_t* dV, int B, int Hq, int Hkv, int64_t S, float scale,
    const int32_t* doc_start, const int32_t* doc_end, int64_t do_sb,
    int64_t do_sh, int64_t do_sr, void* stream) {
  if (int rc = check_ostrides(dO, do_sb, do_sh, do_sr)) return rc;
  return attn_bwd2_launch(Q, K, V, dO, delta, lse2, dQ, dK, dV, B, Hq, Hkv, S,
                          scale, doc_start, doc_end,
                          OStrides{do_sb, do_sh, do_sr}, stream);
}

/* vh_attn_bwd2_ostrided_bf16 with key-window bounds shared by the batch.
 * lo / hi (nullable together): int32 [S]; lo[q] is the first key row q sees,
 * hi[j] the exclusive end of the rows that see key j, both monotone
 * non-decreasing with lo[q] <= q < hi[q] <= S; B > 1 allowed. delta and lse2
 * come from vh_attn_bwd_pre_sink_bf16: with a sink-inclusive LSE the two
 * kernels need nothing else for sinks. S % 256 == 0. */
extern "C" int vh_attn_bwd2_win_bf16(
    const uint16_t* Q, const uint16_t* K, const uint16_t* V, const uint16_t* dO,
    const float* delta, const float* lse2, uint16_t* dQ, uint16_t* dK,
    uint16_t* dV, int B, int Hq, int Hkv, int64_t S, float scale,
    const int32_t* lo, const int32_t* hi, int64_t do_sb, int64_t do_sh,
    int64_t do_sr, void* stream) {
  VH_CHECK(S % 256 == 0, "S %% 256 != 0 (pad the sequence)");
  VH_CHECK(scale > 0, "scale must be > 0 (got %g)", (double)scale);
  if (int rc = check_ostrides(dO, do_sb, do_sh, do_sr)) return rc;
  return attn_bwd2_launch(Q, K, V, dO, delta, lse2, dQ, dK, dV, B, Hq, Hkv, S,
                          scale, lo, hi, OStrides{do_sb, do_sh, do_sr}, stream,
                          /*shared_bounds=*/true);
}
