// gpt-oss experts: the streaming kernels around the grouped GEMMs, gfx950.
//
// Replaces (semantics, not code): the per-expert Python loop of the
// reference's GptOssExperts (bias add, interleaved clamped GLU, bias add,
// routing weight) and the bias-gradient reductions of its fused gpt-oss
// expert function. The grouped GEMMs write RAW products; everything that
// depends on the expert of a row (the two biases) is applied here:
//
//   glu:        g_raw = fc1[r,2j] + b[e,2j]      u_raw = fc1[r,2j+1] + b[e,2j+1]
//               g = min(g_raw, L)                u = min(max(u_raw, -L), L)
//               out[r,j] = (u + 1) * g * sigmoid(alpha * g)
//   bias_scale: out[r,:] = (x[r,:] + b[e,:]) * w[r]
//   colsum:     out[g,n] = sum over the rows of expert g of x[r,n]   (bias grads)
//
// gate and up are INTERLEAVED along the last dim ([..., ::2] gate, [..., 1::2]
// up): one 32-bit word holds a (gate, up) pair, so the de-interleave is a
// shift and a mask in registers. Row r belongs to expert e iff
// cumsum[e-1] <= r < cumsum[e]; every row kernel gives one wave to a row, so
// the expert is found once per row by a wave-uniform binary search of cumsum
// (scalar loads, no host read, empty experts anywhere are skipped over).
// Both directions recompute clamp and mask from the raw fc1 and the bias;
// fc1 + bias is never rounded to bf16. Bounds are inclusive, NaN gets a zero
// gradient, L arrives already rounded to bf16 (see vh_moe_swiglu_limit.hip).

#include "vh_common.h"

#include <cmath>

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// a (gate, up) pair as it lies in memory: element 2j in the low half
__device__ __forceinline__ float lo_f(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi_f(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// two fp32 -> one packed bf16 pair (a in the low half), round-to-nearest-even
// through the gfx950 conversion instruction (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack_bf2(float a, float b) {
  union { bf16x2_t v; uint32_t u; } c;
  f32x2_t f = {a, b};
  c.v = __builtin_convertvector(f, bf16x2_t);
  return c.u;
}

__device__ __forceinline__ float clamp_gate(float g, float L) {
  return g > L ? L : g;
}
__device__ __forceinline__ float clamp_up(float u, float L) {
  return u < -L ? -L : (u > L ? L : u);
}

// 1 / (1 + exp(-x)) with the hardware exp2 and reciprocal (1 ulp each): the
// IEEE division costs ~10 VALU instructions per element in kernels that are
// issue-bound before they are HBM-bound
__device__ __forceinline__ float sigmoid_fast(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}

// smallest e with cumsum[e] > r, clamped to G-1 (so a row past the last
// cumsum entry still reads a bias that exists). r is wave-uniform.
__device__ __forceinline__ int expert_of_row(const int64_t* __restrict__ cumsum,
                                             int G, int64_t r) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (cumsum[mid] > r) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ int wave_id() {
  return __builtin_amdgcn_readfirstlane(
      (int)(blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave));
}

constexpr int kRowBlock = 256;                     // 4 waves = 4 rows per block
constexpr int kRowWaves = kRowBlock / kWave;
constexpr int64_t kRowMaxBlocks = 2048;            // 8192 rows per pass

__device__ __forceinline__ float glu_one(float g_raw, float u_raw, float alpha, float L) {
  float g = clamp_gate(g_raw, L), u = clamp_up(u_raw, L);
  return (u + 1.0f) * g * sigmoid_fast(alpha * g);
}

// One lane: two adjacent 16-byte loads = 8 (gate, up) pairs -> one 16-byte store.
__global__ __launch_bounds__(kRowBlock) void k_gptoss_glu(
    const uint4* __restrict__ fc1, const uint4* __restrict__ bias,
    const int64_t* __restrict__ cumsum, uint4* __restrict__ out, int64_t rows,
    int64_t Iv, int G, float alpha, float L) {
  const int lane = threadIdx.x & (kWave - 1);
  const int num_waves = gridDim.x * kRowWaves;
  for (int64_t r = wave_id(); r < rows; r += num_waves) {
    const int e = expert_of_row(cumsum, G, r);
    const uint4* x = fc1 + r * 2 * Iv;
    const uint4* b = bias + (int64_t)e * 2 * Iv;
    for (int64_t c = lane; c < Iv; c += kWave) {
      uint4 x0 = x[2 * c], x1 = x[2 * c + 1];
      uint4 b0 = b[2 * c], b1 = b[2 * c + 1];
      const uint32_t xw[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
      const uint32_t bw[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = glu_one(lo_f(xw[j]) + lo_f(bw[j]), hi_f(xw[j]) + hi_f(bw[j]), alpha, L);
      uint4 ov;
      ov.x = pack_bf2(o[0], o[1]);
      ov.y = pack_bf2(o[2], o[3]);
      ov.z = pack_bf2(o[4], o[5]);
      ov.w = pack_bf2(o[6], o[7]);
      out[r * Iv + c] = ov;
    }
  }
}

__global__ __launch_bounds__(kRowBlock) void k_gptoss_glu_bwd(
    const uint4* __restrict__ dy, const uint4* __restrict__ fc1,
    const uint4* __restrict__ bias, const int64_t* __restrict__ cumsum,
    uint4* __restrict__ dfc1, int64_t rows, int64_t Iv, int G, float alpha,
    float L) {
  const int lane = threadIdx.x & (kWave - 1);
  const int num_waves = gridDim.x * kRowWaves;
  for (int64_t r = wave_id(); r < rows; r += num_waves) {
    const int e = expert_of_row(cumsum, G, r);
    const uint4* x = fc1 + r * 2 * Iv;
    const uint4* b = bias + (int64_t)e * 2 * Iv;
    uint4* dx = dfc1 + r * 2 * Iv;
    for (int64_t c = lane; c < Iv; c += kWave) {
      uint4 x0 = x[2 * c], x1 = x[2 * c + 1];
      uint4 b0 = b[2 * c], b1 = b[2 * c + 1];
      uint4 d = dy[r * Iv + c];
      const uint32_t xw[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
      const uint32_t bw[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
      uint32_t ow[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float g_raw = lo_f(xw[j]) + lo_f(bw[j]);
        float u_raw = hi_f(xw[j]) + hi_f(bw[j]);
        float dj = (j & 1) ? hi_f(dw[j >> 1]) : lo_f(dw[j >> 1]);
        float g = clamp_gate(g_raw, L), u = clamp_up(u_raw, L);
        float s = sigmoid_fast(alpha * g);
        float gs = g * s;
        // d/dg [g * s(alpha g)] = s + alpha * g * s * (1 - s)
        float dg = dj * (u + 1.0f) * (s + alpha * gs * (1.0f - s));
        float du = dj * gs;
        dg = g_raw <= L ? dg : 0.f;
        du = (u_raw >= -L && u_raw <= L) ? du : 0.f;
        ow[j] = pack_bf2(dg, du);
      }
      dx[2 * c] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
      dx[2 * c + 1] = make_uint4(ow[4], ow[5], ow[6], ow[7]);
    }
  }
}

// out[r,:] = (x[r,:] + bias[e,:]) * w[r]
template <bool HAS_W>
__global__ __launch_bounds__(kRowBlock) void k_expert_bias_scale(
    const uint4* __restrict__ x, const uint4* __restrict__ bias,
    const int64_t* __restrict__ cumsum, const bf16_t* __restrict__ w_row,
    uint4* __restrict__ out, int64_t rows, int64_t Nv, int G) {
  const int lane = threadIdx.x & (kWave - 1);
  const int num_waves = gridDim.x * kRowWaves;
  for (int64_t r = wave_id(); r < rows; r += num_waves) {
    const int e = expert_of_row(cumsum, G, r);
    const float w = HAS_W ? bf2f(w_row[r]) : 1.0f;
    const uint4* xr = x + r * Nv;
    const uint4* b = bias + (int64_t)e * Nv;
    for (int64_t c = lane; c < Nv; c += kWave) {
      uint4 xv = xr[c], bv = b[c];
      const uint32_t xw[4] = {xv.x, xv.y, xv.z, xv.w};
      const uint32_t bw[4] = {bv.x, bv.y, bv.z, bv.w};
      uint32_t ow[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        ow[j] = pack_bf2((lo_f(xw[j]) + lo_f(bw[j])) * w,
                         (hi_f(xw[j]) + hi_f(bw[j])) * w);
      out[r * Nv + c] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
  }
}

// dx = dy * w[r];  dw_row[r] = sum_n (x + bias) * dy. The row reduce stays in
// the wave and lane 0 STORES it: dw_row needs no zero fill, no atomics.
template <bool HAS_W>
__global__ __launch_bounds__(kRowBlock) void k_expert_bias_scale_bwd(
    const uint4* __restrict__ dy, const uint4* __restrict__ x,
    const uint4* __restrict__ bias, const int64_t* __restrict__ cumsum,
    const bf16_t* __restrict__ w_row, uint4* __restrict__ dx,
    float* __restrict__ dw_row, int64_t rows, int64_t Nv, int G) {
  const int lane = threadIdx.x & (kWave - 1);
  const int num_waves = gridDim.x * kRowWaves;
  for (int64_t r = wave_id(); r < rows; r += num_waves) {
    if (!HAS_W) {
      // factor 1: the gradient passes through unchanged
      for (int64_t c = lane; c < Nv; c += kWave) dx[r * Nv + c] = dy[r * Nv + c];
      continue;
    }
    const int e = expert_of_row(cumsum, G, r);
    const float w = bf2f(w_row[r]);
    const uint4* b = bias + (int64_t)e * Nv;
    float acc = 0.f;
    for (int64_t c = lane; c < Nv; c += kWave) {
      uint4 dv = dy[r * Nv + c], xv = x[r * Nv + c], bv = b[c];
      const uint32_t dwd[4] = {dv.x, dv.y, dv.z, dv.w};
      const uint32_t xw[4] = {xv.x, xv.y, xv.z, xv.w};
      const uint32_t bw[4] = {bv.x, bv.y, bv.z, bv.w};
      uint32_t ow[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float d0 = lo_f(dwd[j]), d1 = hi_f(dwd[j]);
        acc += (lo_f(xw[j]) + lo_f(bw[j])) * d0;
        acc += (hi_f(xw[j]) + hi_f(bw[j])) * d1;
        ow[j] = pack_bf2(d0 * w, d1 * w);
      }
      dx[r * Nv + c] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
      acc += __shfl_down(acc, off, kWave);
    if (lane == 0) dw_row[r] = acc;
  }
}

// Segment column sum. A block owns one expert x one slab of 256 columns. Its
// 16 waves split into 32 half-wave row slots (32 lanes x 8 columns = the
// slab); slot s adds rows start+s, start+s+32, ... of the expert in that
// order, then column t of the slab is the sum of the 32 slot partials in slot
// order through LDS. No atomics, one fixed order: bit-reproducible. An empty
// expert adds nothing and writes exact zeros.
constexpr int kCsBlock = 1024;
constexpr int kCsSlots = kCsBlock / 32;            // 32 row slots
constexpr int kCsCols = 256;                       // columns per slab

__global__ __launch_bounds__(kCsBlock) void k_segment_colsum(
    const uint4* __restrict__ x, const int64_t* __restrict__ cumsum,
    float* __restrict__ out, int64_t rows, int64_t N) {
  __shared__ float red[kCsSlots][kCsCols];
  const int g = blockIdx.y;
  const int64_t Nv = N / 8;
  const int slot = threadIdx.x >> 5;
  const int sub = threadIdx.x & 31;
  const int64_t cv = (int64_t)blockIdx.x * 32 + sub;
  int64_t start = g == 0 ? 0 : cumsum[g - 1];
  int64_t end = cumsum[g];
  // a cumsum that runs past the buffer must not turn into reads past it
  if (start < 0) start = 0;
  if (end > rows) end = rows;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (cv < Nv) {
#pragma unroll 4
    for (int64_t r = start + slot; r < end; r += kCsSlots) {
      uint4 v = x[r * Nv + cv];
      acc[0] += lo_f(v.x); acc[1] += hi_f(v.x);
      acc[2] += lo_f(v.y); acc[3] += hi_f(v.y);
      acc[4] += lo_f(v.z); acc[5] += hi_f(v.z);
      acc[6] += lo_f(v.w); acc[7] += hi_f(v.w);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[slot][sub * 8 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < kCsCols) {
    const int64_t col = (int64_t)blockIdx.x * kCsCols + threadIdx.x;
    if (col < N) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < kCsSlots; ++k) s += red[k][threadIdx.x];
      out[(int64_t)g * N + col] = s;
    }
  }
}

int64_t row_blocks(int64_t rows) {
  int64_t blocks = (rows + kRowWaves - 1) / kRowWaves;
  return blocks > kRowMaxBlocks ? kRowMaxBlocks : blocks;
}

}  // namespace

#define VH_GPTOSS_CHECK_GLU()                                                  \
  VH_CHECK(I > 0 && I % 8 == 0, "I %% 8 != 0 (I=%lld)", (long long)I);         \
  VH_CHECK(G > 0, "G <= 0 (G=%d)", G);                                         \
  VH_CHECK(std::isfinite(limit) && limit > 0.f,                                \
           "swiglu limit must be finite and > 0 (got %g)", (double)limit);     \
  VH_CHECK(std::isfinite(alpha), "swiglu alpha must be finite (got %g)",       \
           (double)alpha);                                                     \
  VH_CHECK(rows >= 0, "rows < 0")

extern "C" int vh_moe_gptoss_glu_bf16(const uint16_t* fc1, const uint16_t* bias,
                                      const int64_t* cumsum, uint16_t* out,
                                      int64_t rows, int64_t I, int G,
                                      float alpha, float limit, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_GPTOSS_CHECK_GLU();
  if (rows == 0) return 0;
  hipLaunchKernelGGL(k_gptoss_glu, dim3((uint32_t)row_blocks(rows)),
                     dim3(kRowBlock), 0, s,
                     reinterpret_cast<const uint4*>(fc1),
                     reinterpret_cast<const uint4*>(bias), cumsum,
                     reinterpret_cast<uint4*>(out), rows, I / 8, G, alpha, limit);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_moe_gptoss_glu_bwd_bf16(const uint16_t* dy, const uint16_t* fc1,
                                          const uint16_t* bias,
                                          const int64_t* cumsum, uint16_t* dfc1,
                                          int64_t rows, int64_t I, int G,
                                          float alpha, float limit, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_GPTOSS_CHECK_GLU();
  if (rows == 0) return 0;
  hipLaunchKernelGGL(k_gptoss_glu_bwd, dim3((uint32_t)row_blocks(rows)),
                     dim3(kRowBlock), 0, s, reinterpret_cast<const uint4*>(dy),
                     reinterpret_cast<const uint4*>(fc1),
                     reinterpret_cast<const uint4*>(bias), cumsum,
                     reinterpret_cast<uint4*>(dfc1), rows, I / 8, G, alpha, limit);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_moe_expert_bias_scale_bf16(const uint16_t* x, const uint16_t* bias,
                                             const int64_t* cumsum,
                                             const uint16_t* w_row, uint16_t* out,
                                             int64_t rows, int64_t N, int G,
                                             void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(N > 0 && N % 8 == 0, "N %% 8 != 0 (N=%lld)", (long long)N);
  VH_CHECK(G > 0, "G <= 0 (G=%d)", G);
  VH_CHECK(rows >= 0, "rows < 0");
  if (rows == 0) return 0;
  auto kern = w_row != nullptr ? k_expert_bias_scale<true>
                               : k_expert_bias_scale<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)row_blocks(rows)), dim3(kRowBlock), 0,
                     s, reinterpret_cast<const uint4*>(x),
                     reinterpret_cast<const uint4*>(bias), cumsum,
                     reinterpret_cast<const bf16_t*>(w_row),
                     reinterpret_cast<uint4*>(out), rows, N / 8, G);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_moe_expert_bias_scale_bwd_bf16(
    const uint16_t* dy, const uint16_t* x, const uint16_t* bias,
    const int64_t* cumsum, const uint16_t* w_row, uint16_t* dx, float* dw_row,
    int64_t rows, int64_t N, int G, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(N > 0 && N % 8 == 0, "N %% 8 != 0 (N=%lld)", (long long)N);
  VH_CHECK(G > 0, "G <= 0 (G=%d)", G);
  VH_CHECK(rows >= 0, "rows < 0");
  VH_CHECK(w_row == nullptr || dw_row != nullptr, "w_row without dw_row");
  if (rows == 0) return 0;
  auto kern = w_row != nullptr ? k_expert_bias_scale_bwd<true>
                               : k_expert_bias_scale_bwd<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)row_blocks(rows)), dim3(kRowBlock), 0,
                     s, reinterpret_cast<const uint4*>(dy),
                     reinterpret_cast<const uint4*>(x),
                     reinterpret_cast<const uint4*>(bias), cumsum,
                     reinterpret_cast<const bf16_t*>(w_row),
                     reinterpret_cast<uint4*>(dx), dw_row, rows, N / 8, G);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_moe_segment_colsum_bf16(const uint16_t* x, const int64_t* cumsum,
                                          float* out, int64_t rows, int64_t N,
                                          int G, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(N > 0 && N % 8 == 0, "N %% 8 != 0 (N=%lld)", (long long)N);
  VH_CHECK(G > 0 && G <= 65535, "G out of range (G=%d)", G);
  VH_CHECK(rows >= 0, "rows < 0");
  // rows == 0 still launches: every element of out is written (zeros)
  const int64_t slabs = (N + kCsCols - 1) / kCsCols;
  hipLaunchKernelGGL(k_segment_colsum, dim3((uint32_t)slabs, (uint32_t)G),
                     dim3(kCsBlock), 0, s, reinterpret_cast<const uint4*>(x),
                     cumsum, out, rows, N);
  VH_HIP(hipGetLastError());
  return 0;
}
