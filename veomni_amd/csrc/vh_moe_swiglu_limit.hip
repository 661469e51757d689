// Clamped SwiGLU expert epilogue (gpt-oss / DeepSeek-V4 `swiglu_limit`),
// streaming kernels for gfx950.
//
// Replaces (semantics, not code): ref group_gemm.py:24-42 (_apply_swiglu_limit
// + mask-zeroed gradients) fused into the silu*up*weight epilogue pair of
// vh_moe_ops.hip. The reference writes two clamped copies of the fc1 halves
// and two [rows, I] boolean masks and saves them for backward; here both
// directions read the RAW merged pre-activation and recompute clamp and mask
// in registers, so the clamped pair moves exactly the bytes of the unclamped
// pair and saves nothing extra.
//
//   g = min(g_raw, L)            u = min(max(u_raw, -L), L)
//   dg = (g_raw <= L)            ? dact * u * silu'(g) : 0
//   du = (-L <= u_raw <= L)      ? dact * silu(g)      : 0
//
// Bounds are inclusive (a value exactly at +-L passes its gradient, like
// torch.clamp autograd); NaN propagates through the clamp and gets a zero
// gradient. L is used as received: the caller rounds it to bf16 so that it
// compares the way the reference's bf16 clamp / `<=` against a scalar do.

#include "vh_common.h"

#include <cmath>

namespace {

// fp32 -> bf16, round-to-nearest-even, through the gfx950 conversion
// instruction (v_cvt_pk_bf16_f32) instead of vh_common.h's integer sequence
// with its NaN branch: the same bits for every non-NaN value, ~8 VALU
// instructions less per conversion. These epilogues issue ~80 VALU
// instructions per element and are issue-bound before they are HBM-bound,
// so this pays for the clamp compares.
__device__ __forceinline__ bf16_t f2bf_hw(float f) {
  union { __bf16 b; bf16_t u; } c;
  c.b = static_cast<__bf16>(f);
  return c.u;
}

__device__ __forceinline__ float clamp_gate(float g, float L) {
  return g > L ? L : g;
}
__device__ __forceinline__ float clamp_up(float u, float L) {
  return u < -L ? -L : (u > L ? L : u);
}

// Grid-stride over the rows*Iv output vectors. (row, col) of a lane's first
// vector cost one division; every later vector is reached by stepping with
// the constant (stride / Iv, stride % Iv), so the loop holds no division.
template <bool HAS_W>
__global__ void k_silu_mul_clamp_weighted(const bf16x8* __restrict__ fc1,
                                          const bf16_t* __restrict__ w_row,
                                          bf16x8* __restrict__ out,
                                          int64_t rows, int64_t Iv, float L) {
  const int64_t total = rows * Iv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= total) return;
  int64_t r = i / Iv, c = i - r * Iv;
  const int64_t step_r = stride / Iv, step_c = stride - step_r * Iv;
  for (; i < total; i += stride) {
    const bf16x8* row = fc1 + r * 2 * Iv;
    bf16x8 g = row[c];
    bf16x8 u = row[Iv + c];
    float w = HAS_W ? bf2f(w_row[r]) : 1.0f;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // same rounding chain as k_silu_mul_weighted, on the clamped values
      float a = bf2f(f2bf_hw(siluf(clamp_gate(bf2f(g.v[j]), L))));
      float b = bf2f(f2bf_hw(a * clamp_up(bf2f(u.v[j]), L)));
      o.v[j] = f2bf_hw(b * w);
    }
    out[r * Iv + c] = o;
    r += step_r;
    c += step_c;
    if (c >= Iv) {
      c -= Iv;
      ++r;
    }
  }
}

// One wave owns a row (waves stride the rows), so the per-row dw reduce stays
// in-wave and lane 0 STORES the sum: dw_row needs no zero fill, no atomics.
// With the row-weight path the conversion instruction lengthens live ranges
// to 88 VGPRs (5 waves/SIMD); that instance keeps the integer f2bf, which
// holds it at the unclamped kernel's 6 waves/SIMD.
template <bool HAS_W>
__global__ void k_silu_mul_clamp_weighted_bwd(const bf16x8* __restrict__ dy,
                                              const bf16x8* __restrict__ fc1,
                                              const bf16_t* __restrict__ w_row,
                                              bf16x8* __restrict__ dfc1,
                                              float* __restrict__ dw_row,
                                              int64_t rows, int64_t Iv,
                                              float L) {
  int wave = (blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  int lane = threadIdx.x & (kWave - 1);
  int num_waves = (gridDim.x * blockDim.x) / kWave;
  for (int64_t r = wave; r < rows; r += num_waves) {
    float w = HAS_W ? bf2f(w_row[r]) : 1.0f;
    float dw_acc = 0.f;
    for (int64_t c = lane; c < Iv; c += kWave) {
      bf16x8 g8 = fc1[r * 2 * Iv + c];
      bf16x8 u8 = fc1[r * 2 * Iv + Iv + c];
      bf16x8 d8 = dy[r * Iv + c];
      bf16x8 dg8, du8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float g_raw = bf2f(g8.v[j]), u_raw = bf2f(u8.v[j]), d = bf2f(d8.v[j]);
        float g = clamp_gate(g_raw, L), u = clamp_up(u_raw, L);
        float sg = siluf(g);
        float dact = d * w;           // grad wrt silu(g)*up
        float dg = dact * u * dsiluf(g);
        float du = dact * sg;
        dg = g_raw <= L ? dg : 0.f;
        du = (u_raw >= -L && u_raw <= L) ? du : 0.f;
        dg8.v[j] = HAS_W ? f2bf(dg) : f2bf_hw(dg);
        du8.v[j] = HAS_W ? f2bf(du) : f2bf_hw(du);
        dw_acc += d * sg * u;
      }
      dfc1[r * 2 * Iv + c] = dg8;
      dfc1[r * 2 * Iv + Iv + c] = du8;
    }
    if (HAS_W && dw_row != nullptr) {
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1)
        dw_acc += __shfl_down(dw_acc, off, kWave);
      if (lane == 0) dw_row[r] = dw_acc;
    }
  }
}

}  // namespace

extern "C" int vh_moe_silu_mul_clamp_weighted_bf16(
    const uint16_t* fc1, const uint16_t* w_row, uint16_t* out, int64_t rows,
    int64_t I, int has_w, float limit, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(I > 0 && I % 8 == 0, "I %% 8 != 0 (I=%lld)", (long long)I);
  VH_CHECK(std::isfinite(limit) && limit > 0.f,
           "swiglu limit must be finite and > 0 (got %g)", (double)limit);
  VH_CHECK(rows >= 0, "rows < 0");
  if (rows == 0) return 0;
  int64_t Iv = I / 8;
  int64_t total = rows * Iv;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  auto kern = has_w ? k_silu_mul_clamp_weighted<true>
                    : k_silu_mul_clamp_weighted<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, s,
                     reinterpret_cast<const bf16x8*>(fc1),
                     reinterpret_cast<const bf16_t*>(w_row),
                     reinterpret_cast<bf16x8*>(out), rows, Iv, limit);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_moe_silu_mul_clamp_weighted_bwd_bf16(
    const uint16_t* dy, const uint16_t* fc1, const uint16_t* w_row,
    uint16_t* dfc1, float* dw_row, int64_t rows, int64_t I, int has_w,
    float limit, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(I > 0 && I % 8 == 0, "I %% 8 != 0 (I=%lld)", (long long)I);
  VH_CHECK(std::isfinite(limit) && limit > 0.f,
           "swiglu limit must be finite and > 0 (got %g)", (double)limit);
  VH_CHECK(rows >= 0, "rows < 0");
  if (rows == 0) return 0;
  int64_t Iv = I / 8;
  // 4 waves (rows) per 256-thread block, at most 2048 blocks = 8192 waves
  int64_t blocks = (rows + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  auto kern = has_w ? k_silu_mul_clamp_weighted_bwd<true>
                    : k_silu_mul_clamp_weighted_bwd<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, s,
                     reinterpret_cast<const bf16x8*>(dy),
                     reinterpret_cast<const bf16x8*>(fc1),
                     reinterpret_cast<const bf16_t*>(w_row),
                     reinterpret_cast<bf16x8*>(dfc1), dw_row, rows, Iv, limit);
  VH_HIP(hipGetLastError());
  return 0;
}
