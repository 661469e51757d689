// Fused MoE load-balancing (Switch aux) loss, forward + backward (gfx950,
// HBM-bound).
//
// Semantics anchor: the reference's load_balancing_loss provider
// (ref load_balancing_loss/eager.py:28-114; fused twin triton.py:280-354):
// per row fp32 upcast + max-subtracted softmax, prob_sum += w*p, each of the
// top_k selected experts gets count += w, and
//   loss = dot(count, prob_sum) * E / total_w^2   (0 when total_w == 0).
//
// Selection rule (the spec of this kernel): the top_k LARGEST LOGITS of the
// row after the fp32 upcast, ties going to the LOWEST expert index. Softmax
// is monotone, so this is the reference's top-k of the probabilities
// wherever that top-k is unambiguous, and unlike a selection on in-kernel
// exp results it does not depend on the exp implementation. -inf logits are
// allowed (p = 0); NaN logits and all--inf rows are outside the contract.
//
// Layout: a sub-group of G lanes (G = pow2 >= ceil(E/8), G <= 32) owns one
// row, each lane 8 consecutive expert columns. When E == 8*G and the base is
// 16-B aligned a lane reads its columns with 16-B loads; every other E takes
// the same code with scalar, bounds-checked loads and -inf padding columns.
// Row max / sum / arg-max stay inside the sub-group, as a butterfly of DPP
// lane exchanges (quad_perm, row_half_mirror, row_mirror; only the 32-lane
// step goes through __shfl_xor). Top-k is top_k rounds of arg-max over
// order-preserving integer keys that carry the expert index in their low
// bits (value, then lower index, in ONE unsigned max: 32-bit keys for bf16
// logits, 64-bit for fp32); the winner's key is zeroed, and the zeroed keys
// are the row's selection. Forward: each lane keeps fp32 accumulators for its 8 columns
// over all rows it sees; at block end lanes owning the same columns are
// combined by wave shuffles, then across waves through LDS, and the block
// writes its own row of `partial` -- no atomics, bit-reproducible. A finish
// pass reduces all partial rows in fixed order in double precision (counts
// stay exact past 2^24) and forms loss and coef on device.
//
// Backward recomputes the row softmax:
//   grad[t,j] = grad_out*coef*w_t * p_j * (count_j - sum_i p_i count_i).

#include "vh_common.h"

#include <cmath>
#include <type_traits>

namespace {

constexpr int kLblFwdThreads = 1024;
constexpr int kLblBwdThreads = 256;
constexpr int kLblMaxE = 256;

// ------------------------------------------------------ sub-group exchange
// lbl_xchg<S>(v): each lane's value from its butterfly partner at step S
// (S = 1, 2, 4, 8, 16; steps must be taken in ascending order). Steps 1 and
// 2 are lane-xor inside a quad; steps 4 and 8 mirror the 8- and 16-lane row,
// which pairs the two halves just like xor once every smaller block already
// holds one common value. All 64 lanes are active at every call site.
template <int S>
__device__ __forceinline__ uint32_t lbl_xchg(uint32_t v) {
  if constexpr (S == 1)
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);
  else if constexpr (S == 2)
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);
  else if constexpr (S == 4)  // row_half_mirror
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);
  else if constexpr (S == 8)  // row_mirror
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true);
  else
    return (uint32_t)__shfl_xor((int)v, 16, kWave);
}
template <int S>
__device__ __forceinline__ float lbl_xchg(float v) {
  return __uint_as_float(lbl_xchg<S>(__float_as_uint(v)));
}
template <int S>
__device__ __forceinline__ uint64_t lbl_xchg(uint64_t v) {
  return ((uint64_t)lbl_xchg<S>((uint32_t)(v >> 32)) << 32) |
         lbl_xchg<S>((uint32_t)v);
}

struct LblMax {
  template <typename V>
  __device__ __forceinline__ V operator()(V a, V b) const { return a > b ? a : b; }
};
struct LblAdd {
  __device__ __forceinline__ float operator()(float a, float b) const { return a + b; }
};

// All-reduce over the G-lane sub-group; every lane ends with the same bits
// (both partners of a step combine the same two values with a commutative op).
template <int G, typename V, typename Op>
__device__ __forceinline__ V lbl_group_reduce(V v, Op op) {
  if constexpr (G >= 2) v = op(v, lbl_xchg<1>(v));
  if constexpr (G >= 4) v = op(v, lbl_xchg<2>(v));
  if constexpr (G >= 8) v = op(v, lbl_xchg<4>(v));
  if constexpr (G >= 16) v = op(v, lbl_xchg<8>(v));
  if constexpr (G >= 32) v = op(v, lbl_xchg<16>(v));
  return v;
}

// Selection key of logit x at expert column col: unsigned order == (larger x
// first, then lower col); -0.0 keys as +0.0 (they compare equal as floats).
// Every live key is > 0 (x = -inf included); 0 marks "not a candidate".
template <int MODE>
using lbl_key_t = typename std::conditional<(MODE & 1) != 0, uint64_t, uint32_t>::type;

template <int MODE>
__device__ __forceinline__ lbl_key_t<MODE> lbl_key(float x, int col) {
  uint32_t u = __float_as_uint(x + 0.0f);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  if constexpr (MODE & 1)
    return ((uint64_t)u << 32) | (uint64_t)(0xffffffffu - (uint32_t)col);
  else  // bf16 logits: the low 16 value bits carry nothing
    return (u & 0xffff0000u) | (0xffffu - (uint32_t)col);
}

// MODE bit0: fp32 logits (else bf16); bit1: scalar bounds-checked access.
template <int MODE>
__device__ __forceinline__ void lbl_load8(const void* base, int64_t off,
                                          int c0, int E, bool valid,
                                          float (&x)[8]) {
  if (!valid) {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = 0.f;
    return;
  }
  if constexpr (MODE == 0) {
    uint4 u = *reinterpret_cast<const uint4*>(
        reinterpret_cast<const bf16_t*>(base) + off);
    uint32_t wds[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = __uint_as_float(wds[j] << 16);
      x[2 * j + 1] = __uint_as_float(wds[j] & 0xffff0000u);
    }
  } else if constexpr (MODE == 1) {
    const float4* p = reinterpret_cast<const float4*>(
        reinterpret_cast<const float*>(base) + off);
    float4 a = p[0], b = p[1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = -INFINITY;
      if (c0 + j < E) {
        if constexpr (MODE & 1)
          v = reinterpret_cast<const float*>(base)[off + j];
        else
          v = bf2f(reinterpret_cast<const bf16_t*>(base)[off + j]);
      }
      x[j] = v;
    }
  }
}

template <int MODE>
__device__ __forceinline__ void lbl_store8(void* base, int64_t off, int c0,
                                           int E, const float (&g)[8]) {
  if constexpr (MODE == 0) {
    uint4 u;
    u.x = (uint32_t)f2bf(g[0]) | ((uint32_t)f2bf(g[1]) << 16);
    u.y = (uint32_t)f2bf(g[2]) | ((uint32_t)f2bf(g[3]) << 16);
    u.z = (uint32_t)f2bf(g[4]) | ((uint32_t)f2bf(g[5]) << 16);
    u.w = (uint32_t)f2bf(g[6]) | ((uint32_t)f2bf(g[7]) << 16);
    *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(base) + off) = u;
  } else if constexpr (MODE == 1) {
    float4* p = reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + off);
    p[0] = make_float4(g[0], g[1], g[2], g[3]);
    p[1] = make_float4(g[4], g[5], g[6], g[7]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (c0 + j < E) {
        if constexpr (MODE & 1)
          reinterpret_cast<float*>(base)[off + j] = g[j];
        else
          reinterpret_cast<bf16_t*>(base)[off + j] = f2bf(g[j]);
      }
    }
  }
}

// Row softmax over the sub-group: x -> p (padding columns give p = 0).
template <int G>
__device__ __forceinline__ void lbl_softmax(const float (&x)[8],
                                            float (&p)[8]) {
  float m = x[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) m = fmaxf(m, x[j]);
  m = lbl_group_reduce<G>(m, LblMax());
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    p[j] = __expf(x[j] - m);
    s += p[j];
  }
  s = lbl_group_reduce<G>(s, LblAdd());
  float inv = 1.0f / s;
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] *= inv;
}

template <int G, int MODE>
__global__ void __launch_bounds__(kLblFwdThreads)
k_lbl_fwd(const void* __restrict__ logits, const float* __restrict__ mask_w,
          int64_t T, int E, int top_k, float* __restrict__ partial) {
  constexpr int kWaves = kLblFwdThreads / kWave;
  constexpr int R = kLblFwdThreads / G;  // rows per block pass
  __shared__ float red[kWaves][2][G * 8];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  const int sub = tid % G;
  const int c0 = sub * 8;

  float cnt[8], ps[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { cnt[j] = 0.f; ps[j] = 0.f; }

  // block-uniform trip count: every lane reaches every shuffle
  for (int64_t base = (int64_t)blockIdx.x * R; base < T;
       base += (int64_t)gridDim.x * R) {
    const int64_t row = base + tid / G;
    const bool valid = row < T;
    float x[8], p[8];
    lbl_load8<MODE>(logits, row * E + c0, c0, E, valid, x);
    const float w = valid ? (mask_w != nullptr ? mask_w[row] : 1.0f) : 0.f;
    lbl_softmax<G>(x, p);
#pragma unroll
    for (int j = 0; j < 8; ++j) ps[j] += (w != 0.f) ? w * p[j] : 0.f;

    // top_k rounds of arg-max over the selection keys; keys are unique in a
    // row, so zeroing "my key == the winner" removes exactly the winner.
    lbl_key_t<MODE> key[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      key[j] = (MODE < 2 || c0 + j < E) ? lbl_key<MODE>(x[j], c0 + j) : 0;
    for (int r = 0; r < top_k; ++r) {
      lbl_key_t<MODE> a0 = LblMax()(key[0], key[1]), a1 = LblMax()(key[2], key[3]);
      lbl_key_t<MODE> a2 = LblMax()(key[4], key[5]), a3 = LblMax()(key[6], key[7]);
      lbl_key_t<MODE> best = LblMax()(LblMax()(a0, a1), LblMax()(a2, a3));
      best = lbl_group_reduce<G>(best, LblMax());
#pragma unroll
      for (int j = 0; j < 8; ++j) key[j] = (key[j] == best) ? 0 : key[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      cnt[j] += (key[j] == 0 && (MODE < 2 || c0 + j < E)) ? w : 0.f;
  }

  // lanes with the same `sub` own the same columns: combine inside the wave
#pragma unroll
  for (int off = G; off < kWave; off <<= 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      cnt[j] += __shfl_xor(cnt[j], off, kWave);
      ps[j] += __shfl_xor(ps[j], off, kWave);
    }
  }
  if (lane < G) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[wave][0][c0 + j] = cnt[j];
      red[wave][1][c0 + j] = ps[j];
    }
  }
  __syncthreads();
  float* out = partial + (int64_t)blockIdx.x * 2 * E;
  for (int i = tid; i < 2 * E; i += kLblFwdThreads) {
    const int s = i / E, e = i - s * E;
    float acc = 0.f;
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv) acc += red[wv][s][e];
    out[i] = acc;
  }
}

template <int G, int MODE>
__global__ void __launch_bounds__(kLblBwdThreads)
k_lbl_bwd(const void* __restrict__ logits, const float* __restrict__ mask_w,
          const float* __restrict__ count, const float* __restrict__ coef,
          const float* __restrict__ grad_out, void* __restrict__ grad,
          int64_t T, int E) {
  constexpr int R = kLblBwdThreads / G;
  const int tid = threadIdx.x;
  const int c0 = (tid % G) * 8;
  float c[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) c[j] = (c0 + j < E) ? count[c0 + j] : 0.f;
  const float sc = grad_out[0] * coef[0];

  for (int64_t base = (int64_t)blockIdx.x * R; base < T;
       base += (int64_t)gridDim.x * R) {
    const int64_t row = base + tid / G;
    const bool valid = row < T;
    float x[8], p[8], g[8];
    lbl_load8<MODE>(logits, row * E + c0, c0, E, valid, x);
    const float w = valid ? (mask_w != nullptr ? mask_w[row] : 1.0f) : 0.f;
    lbl_softmax<G>(x, p);
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) d += p[j] * c[j];
    d = lbl_group_reduce<G>(d, LblAdd());
    const float gw = sc * w;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      g[j] = (w != 0.f) ? gw * p[j] * (c[j] - d) : 0.f;
    if (valid) lbl_store8<MODE>(grad, row * E + c0, c0, E, g);
  }
}

// Column sums of partial [P_total, 2E] in fixed row order, double
// accumulation. Block = kRedCols columns (one 64-B segment of each row) x
// kRedSlices row slices; slice s takes rows s, s + kRedSlices, ...
constexpr int kRedCols = 16;
constexpr int kRedSlices = 64;

__global__ void __launch_bounds__(kRedCols * kRedSlices)
k_lbl_reduce(const float* __restrict__ partial, int64_t P_total, int E,
             float* __restrict__ count, float* __restrict__ prob_sum) {
  __shared__ double red[kRedSlices][kRedCols + 1];
  const int cl = threadIdx.x % kRedCols, slice = threadIdx.x / kRedCols;
  const int col = blockIdx.x * kRedCols + cl;
  const int W = 2 * E;
  double acc = 0.0;
  if (col < W) {
    for (int64_t r = slice; r < P_total; r += kRedSlices)
      acc += (double)partial[r * W + col];
  }
  red[slice][cl] = acc;
  __syncthreads();
  if (slice == 0 && col < W) {
    double t = 0.0;
#pragma unroll
    for (int s = 0; s < kRedSlices; ++s) t += red[s][cl];
    if (col < E) count[col] = (float)t;
    else prob_sum[col - E] = (float)t;
  }
}

__global__ void __launch_bounds__(kLblMaxE)
k_lbl_loss(const float* __restrict__ count, const float* __restrict__ prob_sum,
           const float* __restrict__ total_w, int E, float* __restrict__ out) {
  __shared__ double red[kLblMaxE];
  const int tid = threadIdx.x;
  red[tid] = (tid < E) ? (double)count[tid] * (double)prob_sum[tid] : 0.0;
  __syncthreads();
#pragma unroll
  for (int off = kLblMaxE / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    const double tw = (double)total_w[0];
    if (tw == 0.0) {
      out[0] = 0.f;
      out[1] = 0.f;
    } else {
      const double coef = (double)E / (tw * tw);
      out[0] = (float)(red[0] * coef);
      out[1] = (float)coef;
    }
  }
}

inline int lbl_group(int E) {
  int ng = (E + 7) / 8, G = 1;
  while (G < ng) G <<= 1;
  return G;
}

inline bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

}  // namespace

#define LBL_DISPATCH_MODE(KERNEL, GG, MODE, ...)                               \
  switch (MODE) {                                                              \
    case 0: KERNEL<GG, 0> __VA_ARGS__; break;                                  \
    case 1: KERNEL<GG, 1> __VA_ARGS__; break;                                  \
    case 2: KERNEL<GG, 2> __VA_ARGS__; break;                                  \
    default: KERNEL<GG, 3> __VA_ARGS__; break;                                 \
  }

#define LBL_DISPATCH(KERNEL, G, MODE, ...)                                     \
  switch (G) {                                                                 \
    case 1: LBL_DISPATCH_MODE(KERNEL, 1, MODE, __VA_ARGS__) break;             \
    case 2: LBL_DISPATCH_MODE(KERNEL, 2, MODE, __VA_ARGS__) break;             \
    case 4: LBL_DISPATCH_MODE(KERNEL, 4, MODE, __VA_ARGS__) break;             \
    case 8: LBL_DISPATCH_MODE(KERNEL, 8, MODE, __VA_ARGS__) break;             \
    case 16: LBL_DISPATCH_MODE(KERNEL, 16, MODE, __VA_ARGS__) break;           \
    default: LBL_DISPATCH_MODE(KERNEL, 32, MODE, __VA_ARGS__) break;           \
  }

extern "C" int vh_lbl_fwd(const void* logits, int dtype, const float* mask_w,
                          int64_t T, int E, int top_k, float* partial, int P,
                          void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(dtype == 0 || dtype == 1, "lbl_fwd: dtype %d (0 = bf16, 1 = fp32)", dtype);
  VH_CHECK(E >= 1 && E <= kLblMaxE, "lbl_fwd: E=%d outside [1, %d]", E, kLblMaxE);
  VH_CHECK(top_k >= 1 && top_k <= E, "lbl_fwd: top_k=%d outside [1, E=%d]", top_k, E);
  VH_CHECK(T >= 1, "lbl_fwd: T=%lld < 1", (long long)T);
  VH_CHECK(P >= 1, "lbl_fwd: P=%d < 1", P);
  const int G = lbl_group(E);
  const bool vec = (E == G * 8) && aligned16(logits);
  const int mode = dtype | (vec ? 0 : 2);
  LBL_DISPATCH(k_lbl_fwd, G, mode,
               <<<dim3((uint32_t)P), dim3(kLblFwdThreads), 0, s>>>(
                   logits, mask_w, T, E, top_k, partial));
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_lbl_finish(const float* partial, int64_t P_total, int E,
                             const float* total_w, float* count,
                             float* prob_sum, float* out, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(E >= 1 && E <= kLblMaxE, "lbl_finish: E=%d outside [1, %d]", E, kLblMaxE);
  VH_CHECK(P_total >= 1, "lbl_finish: P_total=%lld < 1", (long long)P_total);
  const int blocks = (2 * E + kRedCols - 1) / kRedCols;
  k_lbl_reduce<<<dim3(blocks), dim3(kRedCols * kRedSlices), 0, s>>>(
      partial, P_total, E, count, prob_sum);
  VH_HIP(hipGetLastError());
  k_lbl_loss<<<dim3(1), dim3(kLblMaxE), 0, s>>>(count, prob_sum, total_w, E, out);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_lbl_bwd(const void* logits, int dtype, const float* mask_w,
                          const float* count, const float* coef,
                          const float* grad_out, void* grad_logits, int64_t T,
                          int E, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(dtype == 0 || dtype == 1, "lbl_bwd: dtype %d (0 = bf16, 1 = fp32)", dtype);
  VH_CHECK(E >= 1 && E <= kLblMaxE, "lbl_bwd: E=%d outside [1, %d]", E, kLblMaxE);
  VH_CHECK(T >= 1, "lbl_bwd: T=%lld < 1", (long long)T);
  const int G = lbl_group(E);
  const bool vec = (E == G * 8) && aligned16(logits) && aligned16(grad_logits);
  const int mode = dtype | (vec ? 0 : 2);
  const int R = kLblBwdThreads / G;
  int64_t blocks = (T + R - 1) / R;
  if (blocks > 2048) blocks = 2048;
  LBL_DISPATCH(k_lbl_bwd, G, mode,
               <<<dim3((uint32_t)blocks), dim3(kLblBwdThreads), 0, s>>>(
                   logits, mask_w, count, coef, grad_out, grad_logits, T, E));
  VH_HIP(hipGetLastError());
  return 0;
}
