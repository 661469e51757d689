// Per-token log-probability and softmax entropy over a bf16 logits chunk
// (gfx950, HBM-bound), with the matching single-pass gradient.
//
// Semantics anchor: the reference's chunk_logprobs (ref chunk_logprobs.py:
// 165-189 forward, :214-263 backward): fp32 math on the bf16 logits,
//   log_probs[r] = f_y - lse,   entropy[r] = lse - sum_j p_j f_j,
// both exactly 0 where labels[r] == ignore_index. The reference builds
// softmax / probs*logits / logsumexp (and in backward log_softmax + one-hot)
// as fp32 [chunk, V] tensors; here each row is read once.
//
// Forward, per row, online over the row maximum m with d_j = f_j - m:
//   s = sum e^{d_j},  u = sum e^{d_j} d_j   (u <= 0)
//   lse = m + ln s,   H = ln s - u / s.
// Carrying d_j instead of f_j keeps H a sum of two non-negative terms, so a
// peaked row (H ~ 1e-7) or a row sitting at +-80 loses nothing to
// cancellation against |m|.
//
// Backward, per row, with p_j = e^{f_j - lse}:
//   dlogits[j] = dlp (1[j==y] - p_j) - dent p_j ((f_j - lse) + H),
// rounded once to bf16, then scaled by the temperature in bf16.
//
// Temperature follows the reference's rounding boundaries: the bf16 logits
// are scaled by 1/T in bf16 before the fp32 upcast, dlogits is rounded to
// bf16 and then scaled by 1/T in bf16. The scale is a multiply by the fp32
// reciprocal, as ATen's bf16 true-divide by a scalar evaluates it.
//
// One 256-thread block per row, 16-B loads, two in flight per lane; wave
// shuffles then a 4-entry LDS combine in fixed order. No atomics:
// bit-identical run to run.

#include "vh_common.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr float kNegBig = -3.0e38f;

template <bool SCALE>
__device__ __forceinline__ float lp_load(bf16_t x, float inv_t) {
  float f = bf2f(x);
  if (SCALE) f = bf2f(f2bf(f * inv_t));
  return f;
}

// Online (m, s, u) state: s = sum e^{f-m}, u = sum e^{f-m} (f-m).
struct Msu { float m, s, u; };

// Move a state to a new (not smaller) maximum mn.
__device__ __forceinline__ void lp_rebase(Msu& a, float mn) {
  // s == 0 marks a lane that saw no column: keep (.., 0, 0) free of 0 * inf
  float d = (a.s == 0.f) ? 0.f : a.m - mn;
  float e = __expf(d);
  a.u = e * (a.u + d * a.s);
  a.s = e * a.s;
  a.m = mn;
}

__device__ __forceinline__ Msu lp_merge(Msu a, Msu b) {
  float mn = fmaxf(a.m, b.m);
  lp_rebase(a, mn);
  lp_rebase(b, mn);
  a.s += b.s;
  a.u += b.u;
  return a;
}

template <bool SCALE>
__device__ __forceinline__ void lp_accum(Msu& a, const bf16x8& v, float inv_t) {
  float f[8];
  float mx = kNegBig;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f[j] = lp_load<SCALE>(v.v[j], inv_t);
    mx = fmaxf(mx, f[j]);
  }
  if (mx > a.m) lp_rebase(a, mx);
  // the vector's 8 terms are summed as a tree before they join the running
  // sums: the per-lane addition chain is V/2048 + 3 long, not V/256
  float e[8], w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float d = f[j] - a.m;
    e[j] = __expf(d);
    w[j] = e[j] * d;
  }
  a.s += ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
  a.u += ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]));
}

template <bool SCALE>
__global__ __launch_bounds__(kThreads) void k_logprob_fwd(
    const bf16_t* __restrict__ logits, const int64_t* __restrict__ labels,
    float* __restrict__ log_probs, float* __restrict__ entropy,
    float* __restrict__ lse_out, float* __restrict__ ent_raw, int64_t Vv,
    int64_t V, float inv_t, int64_t ignore_index) {
  __shared__ Msu red[kWaves];
  int64_t r = blockIdx.x;
  int64_t label = labels[r];
  if (label == ignore_index) {  // block-uniform: the row is never read
    if (threadIdx.x == 0) {
      log_probs[r] = 0.f;
      entropy[r] = 0.f;
      if (lse_out != nullptr) lse_out[r] = 0.f;
      if (ent_raw != nullptr) ent_raw[r] = 0.f;
    }
    return;
  }
  const bf16x8* row = reinterpret_cast<const bf16x8*>(logits + r * V);
  int lane = threadIdx.x & (kWave - 1);
  int wave = threadIdx.x / kWave;

  Msu a = {kNegBig, 0.f, 0.f};
  for (int64_t c = threadIdx.x; c < Vv; c += 2 * kThreads) {
    bool two = c + kThreads < Vv;
    bf16x8 v0 = row[c];
    bf16x8 v1 = two ? row[c + kThreads] : v0;
    lp_accum<SCALE>(a, v0, inv_t);
    if (two) lp_accum<SCALE>(a, v1, inv_t);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    Msu b;
    b.m = __shfl_down(a.m, off, kWave);
    b.s = __shfl_down(a.s, off, kWave);
    b.u = __shfl_down(a.u, off, kWave);
    a = lp_merge(a, b);
  }
  if (lane == 0) red[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0];
    for (int wv = 1; wv < kWaves; ++wv) a = lp_merge(a, red[wv]);
    float ln_s = logf(a.s);
    float lse = a.m + ln_s;
    float H = ln_s - a.u / a.s;
    // a label outside [0, V) is outside the contract; it is never
    // dereferenced and yields NaN rather than a plausible number
    float lp = NAN;
    if (label >= 0 && label < V)
      lp = lp_load<SCALE>(logits[r * V + label], inv_t) - lse;
    log_probs[r] = lp;
    entropy[r] = H;
    if (lse_out != nullptr) lse_out[r] = lse;
    if (ent_raw != nullptr) ent_raw[r] = H;
  }
}

template <bool SCALE>
__device__ __forceinline__ bf16x8 lp_grad(const bf16x8& v, int64_t col0,
                                          int64_t label, float lse, float H,
                                          float dlp, float dent, float inv_t) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float ld = lp_load<SCALE>(v.v[j], inv_t) - lse;  // log p_j
    float p = __expf(ld);
    float onehot = (col0 + j == label) ? 1.0f : 0.0f;
    float g = dlp * (onehot - p) - dent * p * (ld + H);
    bf16_t gb = f2bf(g);
    if (SCALE) gb = f2bf(bf2f(gb) * inv_t);
    o.v[j] = gb;
  }
  return o;
}

template <bool SCALE>
__global__ __launch_bounds__(kThreads) void k_logprob_bwd(
    const bf16_t* __restrict__ logits, const int64_t* __restrict__ labels,
    const float* __restrict__ lse_in, const float* __restrict__ ent_raw,
    const float* __restrict__ dlog_probs, const float* __restrict__ dentropy,
    bf16_t* __restrict__ dlogits, int64_t Vv, int64_t V, float inv_t,
    int64_t ignore_index) {
  int64_t r = blockIdx.x;
  int64_t label = labels[r];
  const bf16x8* row = reinterpret_cast<const bf16x8*>(logits + r * V);
  bf16x8* drow = reinterpret_cast<bf16x8*>(dlogits + r * V);
  if (label == ignore_index) {  // block-uniform
    bf16x8 z = {};
    for (int64_t c = threadIdx.x; c < Vv; c += kThreads) drow[c] = z;
    return;
  }
  float lse = lse_in[r];
  float H = ent_raw[r];
  float dlp = (dlog_probs != nullptr) ? dlog_probs[r] : 0.f;
  float dent = (dentropy != nullptr) ? dentropy[r] : 0.f;
  for (int64_t c = threadIdx.x; c < Vv; c += 2 * kThreads) {
    bool two = c + kThreads < Vv;
    bf16x8 v0 = row[c];
    bf16x8 v1 = two ? row[c + kThreads] : v0;
    drow[c] = lp_grad<SCALE>(v0, c * 8, label, lse, H, dlp, dent, inv_t);
    if (two)
      drow[c + kThreads] = lp_grad<SCALE>(v1, (c + kThreads) * 8, label, lse,
                                          H, dlp, dent, inv_t);
  }
}


// ---------------------------------------------------------------------------
// Top-k forward-KL distillation on the same chunk (ref chunk_topk_distill.py:
// 165-193 forward, :284-311 backward). Per valid row, ids i_k and teacher
// log-probs t_k (k < K), s_k = f[i_k] - lse:
//   student_mass = sum e^{s_k},  teacher_mass = sum e^{t_k}   (unclamped)
//   distill      = sum e^{t'_k} (t'_k - s'_k),  x' = max(x, clamp)
// and in backward, with w_k = e^{t'_k} [s_k >= clamp], M = sum w_k,
//   dlogits[j] += ddist (M p_j - sum_{k: i_k == j} w_k).
// The reference scatters the teacher into a dense fp32 [chunk, V] row; here
// the K columns are gathered, and the sparse term is folded into the element
// before its single bf16 rounding.

constexpr int kMaxTopk = 1024;

// clamp_min that keeps a NaN (fmaxf would drop it)
__device__ __forceinline__ float tk_floor(float x, bool has_clamp, float c) {
  return (has_clamp && x < c) ? c : x;
}

// One wave per row: lanes stride over K, shuffles combine in fixed order.
template <bool SCALE>
__global__ __launch_bounds__(kWave) void k_topk_kl_fwd(
    const bf16_t* __restrict__ logits, const int64_t* __restrict__ labels,
    const float* __restrict__ lse_in, const int64_t* __restrict__ ids,
    const float* __restrict__ tlp, float* __restrict__ distill,
    float* __restrict__ student_mass, float* __restrict__ teacher_mass,
    int64_t V, int K, float inv_t, bool has_clamp, float clamp,
    int64_t ignore_index) {
  int64_t r = blockIdx.x;
  if (labels[r] == ignore_index) {  // wave-uniform: ids / tlp are never read
    if (threadIdx.x == 0) {
      distill[r] = 0.f;
      student_mass[r] = 0.f;
      teacher_mass[r] = 0.f;
    }
    return;
  }
  float lse = lse_in[r];
  const int64_t* rid = ids + r * K;
  const float* rt = tlp + r * K;
  float kl = 0.f, sm = 0.f, tm = 0.f;
  for (int k = threadIdx.x; k < K; k += kWave) {
    int64_t id = rid[k];
    float t = rt[k];
    // an id outside [0, V) is outside the contract: never dereferenced,
    // NaN in distill and student_mass rather than a plausible number
    float s = NAN;
    if (id >= 0 && id < V) s = lp_load<SCALE>(logits[r * V + id], inv_t) - lse;
    // K terms per row: the accurate expf costs nothing next to the row read
    sm += expf(s);
    tm += expf(t);
    float tc = tk_floor(t, has_clamp, clamp);
    float sc = tk_floor(s, has_clamp, clamp);
    kl += expf(tc) * (tc - sc);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    kl += __shfl_down(kl, off, kWave);
    sm += __shfl_down(sm, off, kWave);
    tm += __shfl_down(tm, off, kWave);
  }
  if (threadIdx.x == 0) {
    distill[r] = kl;
    student_mass[r] = sm;
    teacher_mass[r] = tm;
  }
}

// The log-prob / entropy part of an element, evaluated the way k_logprob_bwd
// evaluates it (three products, one subtraction, nothing contracted), so a
// zero distillation term leaves exactly that kernel's bits.
__device__ __forceinline__ float tk_dense(float ld, float p, float onehot,
                                          float H, float dlp, float dent) {
#pragma clang fp contract(off)
  return dlp * (onehot - p) - dent * p * (ld + H);
}

// lp_grad with the dense part of the distillation term, ddM = ddist * M.
template <bool SCALE>
__device__ __forceinline__ bf16x8 tk_grad(const bf16x8& v, int64_t col0,
                                          int64_t label, float lse, float H,
                                          float dlp, float dent, float ddM,
                                          float inv_t) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float ld = lp_load<SCALE>(v.v[j], inv_t) - lse;  // log p_j
    float p = __expf(ld);
    float onehot = (col0 + j == label) ? 1.0f : 0.0f;
    float g = tk_dense(ld, p, onehot, H, dlp, dent) + ddM * p;
    bf16_t gb = f2bf(g);
    if (SCALE) gb = f2bf(bf2f(gb) * inv_t);
    o.v[j] = gb;
  }
  return o;
}

// One 256-thread block per row. Prologue: (i_k, w_k) parked in LDS, M reduced
// in fixed order. Streaming pass: as k_logprob_bwd plus ddist M p_j. Fix-up:
// thread k recomputes column i_k in full, sparse term included, and
// overwrites that one element; duplicates of a column write the same bits.
template <bool SCALE>
__global__ __launch_bounds__(kThreads) void k_topk_distill_bwd(
    const bf16_t* __restrict__ logits, const int64_t* __restrict__ labels,
    const float* __restrict__ lse_in, const float* __restrict__ ent_raw,
    const int64_t* __restrict__ ids, const float* __restrict__ tlp,
    const float* __restrict__ dlog_probs, const float* __restrict__ dentropy,
    const float* __restrict__ ddistill, bf16_t* __restrict__ dlogits,
    int64_t Vv, int64_t V, int K, float inv_t, bool has_clamp, float clamp,
    int64_t ignore_index) {
  __shared__ int s_id[kMaxTopk];    // column, or -1 for an id outside [0, V)
  __shared__ float s_w[kMaxTopk];
  __shared__ float s_red[kWaves];
  int64_t r = blockIdx.x;
  int64_t label = labels[r];
  const bf16_t* frow = logits + r * V;
  const bf16x8* row = reinterpret_cast<const bf16x8*>(frow);
  bf16x8* drow = reinterpret_cast<bf16x8*>(dlogits + r * V);
  if (label == ignore_index) {  // block-uniform: ids / tlp are never read
    bf16x8 z = {};
    for (int64_t c = threadIdx.x; c < Vv; c += kThreads) drow[c] = z;
    return;
  }
  float lse = lse_in[r];
  float H = ent_raw[r];
  float dlp = (dlog_probs != nullptr) ? dlog_probs[r] : 0.f;
  float dent = (dentropy != nullptr) ? dentropy[r] : 0.f;
  float dd = ddistill[r];

  const int64_t* rid = ids + r * K;
  const float* rt = tlp + r * K;
  float msum = 0.f;
  for (int k = threadIdx.x; k < K; k += kThreads) {
    int64_t id = rid[k];
    bool ok = id >= 0 && id < V;  // checked before any address is formed
    float w = 0.f;
    if (ok) {
      float s = lp_load<SCALE>(frow[id], inv_t) - lse;
      // a clamp that binds on the student side carries no gradient
      if (!has_clamp || s >= clamp) w = expf(tk_floor(rt[k], has_clamp, clamp));
    }
    s_id[k] = ok ? (int)id : -1;
    s_w[k] = w;
    msum += w;
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
    msum += __shfl_down(msum, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) s_red[threadIdx.x / kWave] = msum;
  __syncthreads();
  float M = s_red[0];
  for (int wv = 1; wv < kWaves; ++wv) M += s_red[wv];
  float ddM = dd * M;

  for (int64_t c = threadIdx.x; c < Vv; c += 2 * kThreads) {
    bool two = c + kThreads < Vv;
    bf16x8 v0 = row[c];
    bf16x8 v1 = two ? row[c + kThreads] : v0;
    drow[c] = tk_grad<SCALE>(v0, c * 8, label, lse, H, dlp, dent, ddM, inv_t);
    if (two)
      drow[c + kThreads] = tk_grad<SCALE>(v1, (c + kThreads) * 8, label, lse,
                                          H, dlp, dent, ddM, inv_t);
  }
  // The barrier orders the vector stores above against the element stores
  // below at workgroup scope but waits for no counter: drain this wave's
  // stores first, so none is still queued when another wave overwrites an
  // element of it.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  bf16_t* dst = dlogits + r * V;
  for (int k = threadIdx.x; k < K; k += kThreads) {
    int id = s_id[k];
    if (id < 0) continue;
    float sparse = 0.f;
    for (int q = 0; q < K; ++q)  // ascending: duplicates get identical sums
      if (s_id[q] == id) sparse += s_w[q];
    float ld = lp_load<SCALE>(frow[id], inv_t) - lse;
    float p = __expf(ld);
    float onehot = (id == label) ? 1.0f : 0.0f;
    float g = tk_dense(ld, p, onehot, H, dlp, dent) + dd * (M * p - sparse);
    bf16_t gb = f2bf(g);
    if (SCALE) gb = f2bf(bf2f(gb) * inv_t);
    dst[id] = gb;
  }
}

}  // namespace

extern "C" int vh_logprob_fwd_bf16(const uint16_t* logits,
                                   const int64_t* labels, float* log_probs,
                                   float* entropy, float* lse, float* ent_raw,
                                   int64_t rows, int64_t V,
                                   float inv_temperature, int64_t ignore_index,
                                   void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(V > 0 && V % 8 == 0, "V %% 8 != 0 (V=%lld)", (long long)V);
  VH_CHECK(rows >= 0 && rows <= 0x7fffffffLL, "rows out of range (%lld)",
           (long long)rows);
  VH_CHECK(inv_temperature > 0.f, "inv_temperature must be > 0 (%g)",
           (double)inv_temperature);
  if (rows == 0) return 0;
  auto kern = (inv_temperature != 1.0f) ? k_logprob_fwd<true>
                                        : k_logprob_fwd<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)rows), dim3(kThreads), 0, s, logits,
                     labels, log_probs, entropy, lse, ent_raw, V / 8, V,
                     inv_temperature, ignore_index);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_logprob_bwd_bf16(const uint16_t* logits,
                                   const int64_t* labels, const float* lse,
                                   const float* ent_raw,
                                   const float* dlog_probs,
                                   const float* dentropy, uint16_t* dlogits,
                                   int64_t rows, int64_t V,
                                   float inv_temperature, int64_t ignore_index,
                                   void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(V > 0 && V % 8 == 0, "V %% 8 != 0 (V=%lld)", (long long)V);
  VH_CHECK(rows >= 0 && rows <= 0x7fffffffLL, "rows out of range (%lld)",
           (long long)rows);
  VH_CHECK(inv_temperature > 0.f, "inv_temperature must be > 0 (%g)",
           (double)inv_temperature);
  VH_CHECK(lse != nullptr && ent_raw != nullptr,
           "backward needs the forward's lse / ent_raw statistics");
  if (rows == 0) return 0;
  auto kern = (inv_temperature != 1.0f) ? k_logprob_bwd<true>
                                        : k_logprob_bwd<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)rows), dim3(kThreads), 0, s, logits,
                     labels, lse, ent_raw, dlog_probs, dentropy, dlogits,
                     V / 8, V, inv_temperature, ignore_index);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_topk_kl_fwd_bf16(const uint16_t* logits,
                                   const int64_t* labels, const float* lse,
                                   const int64_t* ids, const float* tlp,
                                   float* distill, float* student_mass,
                                   float* teacher_mass, int64_t rows,
                                   int64_t V, int64_t K, float inv_temperature,
                                   int has_clamp, float clamp,
                                   int64_t ignore_index, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(V > 0 && V % 8 == 0, "V %% 8 != 0 (V=%lld)", (long long)V);
  VH_CHECK(rows >= 0 && rows <= 0x7fffffffLL, "rows out of range (%lld)",
           (long long)rows);
  VH_CHECK(K >= 1 && K <= kMaxTopk, "K out of range [1, %d] (K=%lld)",
           kMaxTopk, (long long)K);
  VH_CHECK(inv_temperature > 0.f, "inv_temperature must be > 0 (%g)",
           (double)inv_temperature);
  VH_CHECK(lse != nullptr, "needs the forward's lse statistic");
  if (rows == 0) return 0;
  auto kern = (inv_temperature != 1.0f) ? k_topk_kl_fwd<true>
                                        : k_topk_kl_fwd<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)rows), dim3(kWave), 0, s, logits,
                     labels, lse, ids, tlp, distill, student_mass,
                     teacher_mass, V, (int)K, inv_temperature, has_clamp != 0,
                     clamp, ignore_index);
  VH_HIP(hipGetLastError());
  return 0;
}

extern "C" int vh_topk_distill_bwd_bf16(
    const uint16_t* logits, const int64_t* labels, const float* lse,
    const float* ent_raw, const int64_t* ids, const float* tlp,
    const float* dlog_probs, const float* dentropy, const float* ddistill,
    uint16_t* dlogits, int64_t rows, int64_t V, int64_t K,
    float inv_temperature, int has_clamp, float clamp, int64_t ignore_index,
    void* stream) {
  // without the distillation gradient this is the log-probs backward itself
  if (ddistill == nullptr)
    return vh_logprob_bwd_bf16(logits, labels, lse, ent_raw, dlog_probs,
                               dentropy, dlogits, rows, V, inv_temperature,
                               ignore_index, stream);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  VH_CHECK(V > 0 && V % 8 == 0 && V <= 0x7fffffffLL,
           "V %% 8 != 0 or V >= 2^31 (V=%lld)", (long long)V);
  VH_CHECK(rows >= 0 && rows <= 0x7fffffffLL, "rows out of range (%lld)",
           (long long)rows);
  VH_CHECK(K >= 1 && K <= kMaxTopk, "K out of range [1, %d] (K=%lld)",
           kMaxTopk, (long long)K);
  VH_CHECK(inv_temperature > 0.f, "inv_temperature must be > 0 (%g)",
           (double)inv_temperature);
  VH_CHECK(lse != nullptr && ent_raw != nullptr,
           "backward needs the forward's lse / ent_raw statistics");
  VH_CHECK(ids != nullptr && tlp != nullptr,
           "ddistill given without teacher ids / log-probs");
  if (rows == 0) return 0;
  auto kern = (inv_temperature != 1.0f) ? k_topk_distill_bwd<true>
                                        : k_topk_distill_bwd<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)rows), dim3(kThreads), 0, s, logits,
                     labels, lse, ent_raw, ids, tlp, dlog_probs, dentropy,
                     ddistill, dlogits, V / 8, V, (int)K, inv_temperature,
                     has_clamp != 0, clamp, ignore_index);
  VH_HIP(hipGetLastError());
  return 0;
}
