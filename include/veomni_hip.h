/* veomni_hip.h — C ABI of libveomni_hip.so (gfx950 / MI355X hot-path kernels).
 *
 * This is the drop-in boundary under the Python operator API.
 * Each entry replaces one reference kernel (anchor cited per function).
 * Conventions:
 *   - caller owns every buffer (device pointers from torch tensors);
 *   - all entries are stream-ordered on the passed hipStream_t (as void*);
 *   - return 0 on success, nonzero error code otherwise; vh_last_error()
 *     returns a thread-local message for the last failure;
 *   - no threads are spawned inside; no allocation except where stated;
 *   - bf16 buffers are passed as uint16_t*.
 */
#ifndef VEOMNI_HIP_H
#define VEOMNI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Last error message (thread-local). */
const char* vh_last_error(void);

/* Build tag: returns a static string identifying arch + version. */
const char* vh_build_info(void);

/* ---- MoE token bookkeeping --------------------------------------------- */

/* Histogram of expert ids. Bit-exact.
 * Replaces: veomni/ops/kernels/moe/_kernels/kernel/moe.py:29-82.
 * expert_index: int64 [n]; out: int32 [num_experts] (pre-zeroed NOT required;
 * kernel zeroes it). */
int vh_expert_histogram(const int64_t* expert_index, int64_t n,
                        int num_experts, int32_t* out, void* stream);

/* Row scatter: out[index[i]] = x[i / topk]'s row — i.e. for each token row t
 * and slot k, out[index[t*topk+k]] = x[t]. bf16 rows.
 * Replaces: kernel/moe.py:253-333 (_moe_scatter_kernel).
 * x: [M, N] bf16; index: int32 [M*topk]; out: [M*topk, N] bf16. */
int vh_moe_scatter_bf16(const uint16_t* x, const int32_t* index, uint16_t* out,
                        int64_t M, int64_t N, int topk, void* stream);

/* Row gather with fp32 accumulation over topk:
 * out[t] = sum_k x[index[t*topk+k]].
 * Replaces: kernel/moe.py:87-159 (_moe_gather_kernel).
 * x: [M*topk, N] bf16; out: [M, N] bf16. */
int vh_moe_gather_bf16(const uint16_t* x, const int32_t* index, uint16_t* out,
                       int64_t M, int64_t N, int topk, void* stream);

/* ---- Grouped GEMM (MFMA bf16, fp32 accumulate) ------------------------- */

/* Per-group GEMM, shared N,K; group g owns rows [cumsum[g-1], cumsum[g]) of
 * A and C.  trans_b!=0: B is [G,N,K] and C_g = A_g @ B_g^T;
 * trans_b==0: B is [G,K,N] and C_g = A_g @ B_g.
 * activation: 0 none; 1 fused SiLU on the output (bf16 rounding after).
 * accumulate!=0: C += result (C read as bf16).
 * cumsum: int64 device [G], inclusive.
 * Replaces: kernel/group_gemm.py:66-234 (group_gemm_same_nk_kernel).
 * Constraints (v1): N % 16 == 0, K % 64 == 0. */
int vh_group_gemm_nk_bf16(const uint16_t* A, const uint16_t* B, uint16_t* C,
                          const int64_t* cumsum, int G, int64_t N, int64_t K,
                          int64_t total_rows, int trans_b, int accumulate,
                          int activation, void* stream);

/* The 256x256 kernels below are what vh_group_gemm_nk_bf16 /
 * vh_group_gemm_mn_bf16 dispatch to for large shapes; they are exported for
 * direct benchmarking. Everything else runs the 128x128 kernels. */

/* Deep-pipelined 256x256 kernel for trans_b == 0 (B [G,K,N]), no
 * accumulate/activation. vh_group_gemm_nk_bf16 dispatches to it for
 * !trans_b, K % 32 == 0, K >= 1024, N >= 1024, total_rows >= 256*G where
 * nk256s_kn does not apply (K % 64 == 32 or G > 4096).
 * K % 32 == 0, K >= 64, N % 16 == 0. trans_b != 0 is an error (that layout
 * is served by nk256s). */
int vh_group_gemm_nk8_bf16(const uint16_t* A, const uint16_t* B, uint16_t* C,
                           const int64_t* cumsum, int G, int64_t N, int64_t K,
                           int64_t total_rows, int trans_b, void* stream);

/* 256-square double-buffered glds kernel (trans_b semantics, B [G,N,K])
 * under a device-built tile schedule with XCD-clustered persistent blocks
 * (L2 reuse of the per-group A/B tiles; no skew-sized null-block grid).
 * vh_group_gemm_nk_bf16 dispatches to it for trans_b, K % 64 == 0,
 * N >= 256, total_rows >= 256*G, G <= 4096. NOTE: on first use this entry
 * hipMallocs one small (~16 KB) schedule workspace that lives for the
 * process (the single exception to the no-allocation convention; calls on
 * one stream serialize on it). */
int vh_group_gemm_nk256s_bf16(const uint16_t* A, const uint16_t* B,
                              uint16_t* C, const int64_t* cumsum, int G,
                              int64_t N, int64_t K, int64_t total_rows,
                              void* stream);

/* The same kernel for trans_b == 0 (B [G,K,N] as stored — dgrad straight
 * from the expert weights, no transposed copy): the B tile is staged
 * [64 k][256 n] and its MFMA fragments are read with transposing LDS reads.
 * Same constraints, dispatch conditions and schedule workspace as above;
 * feeds the MFMAs the operands vh_group_gemm_nk256s_bf16 would get from
 * the transposed weights, in the same order (bit-equal results). */
int vh_group_gemm_nk256s_kn_bf16(const uint16_t* A, const uint16_t* B,
                                 uint16_t* C, const int64_t* cumsum, int G,
                                 int64_t N, int64_t K, int64_t total_rows,
                                 void* stream);

/* Register-staged 256-square ring kernel with wgrad (A^T B) semantics;
 * vh_group_gemm_mn_bf16 dispatches to it for M >= 1024 and N >= 1024. */
int vh_group_gemm_mn8_bf16(const uint16_t* A, const uint16_t* B, uint16_t* C,
                           const int64_t* cumsum, int G, int64_t M, int64_t N,
                           void* stream);

/* Per-group wgrad: C[g] = A_g^T @ B_g with per-group row count (k) from
 * cumsum; A: [rows, M], B: [rows, N], C: [G, M, N] bf16 (fp32 accum).
 * Groups with zero rows are zero-filled.
 * Replaces: kernel/group_gemm.py:252-397 (group_gemm_same_mn_kernel,
 * transpose_a=True, transpose_b=False — the only variant on the path). */
int vh_group_gemm_mn_bf16(const uint16_t* A, const uint16_t* B, uint16_t* C,
                          const int64_t* cumsum, int G, int64_t M, int64_t N,
                          void* stream);

/* Batched expert-weight transpose [E, M, N] -> [E, N, M] bf16 (dgrad W^T;
 * M, N 64-multiples). */
int vh_wtranspose_bf16(const uint16_t* src, uint16_t* dst, int E, int64_t M,
                       int64_t N, void* stream);

/* Direct wgrad for large shapes: C[g] (M x N) = A_g^T @ B_g with A [rows, M]
 * and B [rows, N] token-major as autograd hands them over (no transposed or
 * padded copies, no temporaries); group g owns rows [cumsum[g-1], cumsum[g])
 * at any alignment. 256x256 tiles, persistent XCD-clustered schedule, both
 * operands staged [64 k][256 out] and read with transposing LDS reads. Rows
 * outside a group never contribute (the last k-tile's tail is zeroed in
 * LDS), zero-count groups are zero-filled. M % 16 == 0, N % 16 == 0. */
int vh_group_gemm_wgd_bf16(const uint16_t* A, const uint16_t* B, uint16_t* C,
                           const int64_t* cumsum, int G, int64_t M, int64_t N,
                           int64_t total_rows, void* stream);

/* ---- Fused MoE elementwise --------------------------------------------- */

/* Fused epilogue: act = silu(gate) * up * w_row, where gate/up are the two
 * halves of fc1 [rows, 2I] and w_row is the per-row routing weight.
 * Saves nothing; backward recomputes silu (ref moe_layer.py:328).
 * fc1: [rows, 2I] bf16; w: fp32-or-bf16 per-row [rows]; out: [rows, I] bf16. */
int vh_moe_silu_mul_weighted_bf16(const uint16_t* fc1, const uint16_t* w_row,
                                  uint16_t* out, int64_t rows, int64_t I,
                                  int has_w, void* stream);

/* Backward of the fused epilogue:
 * given dy [rows, I], fc1 [rows,2I] (pre-activation, saved), w_row,
 * produce dfc1 [rows, 2I] and (optional) dw_row [rows] fp32
 * (dw_row[t] = sum_i silu(g)*u * dy — the routing-weight grad numerator). */
int vh_moe_silu_mul_weighted_bwd_bf16(const uint16_t* dy, const uint16_t* fc1,
                                      const uint16_t* w_row, uint16_t* dfc1,
                                      float* dw_row, int64_t rows, int64_t I,
                                      int has_w, void* stream);

/* Clamped SwiGLU (`swiglu_limit`, gpt-oss / DeepSeek-V4) variants of the two
 * entries above; same buffers, plus the limit L before the stream.
 * Replaces: ops/kernels/moe/group_gemm.py:24-42 and its uses at :357-363,
 * :477-480 (clamp + two boolean masks, saved for backward).
 * With g_raw/u_raw the raw halves of fc1:
 *   g = min(g_raw, L);  u = min(max(u_raw, -L), L);
 *   forward : act = silu(g) * u * w_row, the rounding chain of the unclamped
 *             entry (silu -> bf16, *u -> bf16, *w -> bf16);
 *   backward: dg = (g_raw <= L)        ? dy*w*u*silu'(g) : 0
 *             du = (-L <= u_raw <= L)  ? dy*w*silu(g)    : 0
 *             dw_row[t] = sum_i dy*silu(g)*u  (clamped g, u).
 * Bounds are inclusive: a value exactly at +-L passes its gradient, as
 * torch.clamp autograd does. Backward takes the RAW fc1 and recomputes clamp
 * and mask; no mask or clamped copy is ever written. dw_row is STORED (one
 * wave owns a row), so it needs no zero fill. rows == 0 is a no-op returning
 * 0. Nonzero return if I % 8 != 0 or L is not finite and > 0.
 * L is used as received. bf16 callers pass the limit rounded to bf16
 * (round-to-nearest-even): that is the value the reference's bf16 `clamp` and
 * `<=` against a Python scalar effectively use — e.g. bf16 x = 7.125 with
 * limit 7.12 has x <= limit true, clamp(max=limit) = 7.125 and the gradient
 * passes. hip_lib does this rounding. */
int vh_moe_silu_mul_clamp_weighted_bf16(const uint16_t* fc1,
                                        const uint16_t* w_row, uint16_t* out,
                                        int64_t rows, int64_t I, int has_w,
                                        float limit, void* stream);

int vh_moe_silu_mul_clamp_weighted_bwd_bf16(const uint16_t* dy,
                                            const uint16_t* fc1,
                                            const uint16_t* w_row,
                                            uint16_t* dfc1, float* dw_row,
                                            int64_t rows, int64_t I, int has_w,
                                            float limit, void* stream);

/* ---- gpt-oss experts (vh_moe_gpt_oss.hip) ------------------------------ */
/* Streaming kernels around the grouped GEMMs of the gpt-oss expert bank
 * (interleaved gate/up, per-expert biases, routing weight after down_proj).
 * Replaces the per-expert loop of the reference's GptOssExperts.forward and
 * the elementwise/bias-gradient steps of its fused gpt-oss expert function.
 * Common: bf16 tensors, fp32 math. cumsum: int64 [G] inclusive row cumsum on
 * the device; row r belongs to expert e iff cumsum[e-1] <= r < cumsum[e]
 * (found on the device; empty experts are legal anywhere). I % 8 == 0,
 * N % 8 == 0, rows >= 0 (rows == 0 returns at once except for the column
 * sum, which still writes its zeros). */

/* Forward GLU on the RAW fc1 (no bias in it), gate/up interleaved:
 *   g_raw = fc1[r,2j] + bias[e,2j];   u_raw = fc1[r,2j+1] + bias[e,2j+1]
 *   g = min(g_raw, L);  u = min(max(u_raw, -L), L)
 *   out[r,j] = bf16((u + 1) * g * sigmoid(alpha * g))
 * fc1 [rows, 2I], bias [G, 2I], out [rows, I]. limit: finite, > 0, already
 * rounded to bf16 by the caller; alpha finite. */
int vh_moe_gptoss_glu_bf16(const uint16_t* fc1, const uint16_t* bias,
                           const int64_t* cumsum, uint16_t* out, int64_t rows,
                           int64_t I, int G, float alpha, float limit,
                           void* stream);

/* Backward of the above from the same raw fc1 and bias (nothing else saved):
 *   s  = sigmoid(alpha*g)
 *   dg = g_raw <= L       ? dy*(u+1)*(s + alpha*g*s*(1-s)) : 0
 *   du = -L <= u_raw <= L ? dy*g*s                          : 0
 * dfc1 [rows, 2I] interleaved; inclusive bounds; NaN gets a zero gradient. */
int vh_moe_gptoss_glu_bwd_bf16(const uint16_t* dy, const uint16_t* fc1,
                               const uint16_t* bias, const int64_t* cumsum,
                               uint16_t* dfc1, int64_t rows, int64_t I, int G,
                               float alpha, float limit, void* stream);

/* out[r,:] = bf16((x[r,:] + bias[e,:]) * w_row[r]); w_row NULL = factor 1.
 * x, out [rows, N]; bias [G, N]; w_row bf16 [rows]. */
int vh_moe_expert_bias_scale_bf16(const uint16_t* x, const uint16_t* bias,
                                  const int64_t* cumsum, const uint16_t* w_row,
                                  uint16_t* out, int64_t rows, int64_t N, int G,
                                  void* stream);

/* dx = bf16(dy * w_row[r]); dw_row[r] = sum_n (x + bias) * dy in fp32, stored
 * (not accumulated: no zero fill needed). w_row NULL: dx = dy, dw_row
 * untouched. */
int vh_moe_expert_bias_scale_bwd_bf16(const uint16_t* dy, const uint16_t* x,
                                      const uint16_t* bias,
                                      const int64_t* cumsum,
                                      const uint16_t* w_row, uint16_t* dx,
                                      float* dw_row, int64_t rows, int64_t N,
                                      int G, void* stream);

/* out[g,n] = sum over the rows of expert g of x[r,n]; x bf16 [rows, N], out
 * fp32 [G, N]. Every element is written (empty experts: exact zeros). Fixed
 * summation order, no atomics: bit-reproducible. Serves both bias grads. */
int vh_moe_segment_colsum_bf16(const uint16_t* x, const int64_t* cumsum,
                               float* out, int64_t rows, int64_t N, int G,
                               void* stream);

/* ---- RMSNorm------------------------------------------------------------ */

/* y = w * cast_bf16(x_f32 * rsqrt(mean(x^2)+eps)); saves rstd fp32 [T].
 * Replaces the Liger RMSNorm slot (ref ops/liger/__init__.py:28-60); math
 * order matches eager Qwen3MoeRMSNorm (patched modeling :380-400). */
int vh_rmsnorm_fwd_bf16(const uint16_t* x, const uint16_t* w, uint16_t* y,
                        float* rstd, int64_t T, int64_t H, float eps,
                        void* stream);

/* Backward: dx bf16 [T,H]; dw accumulated fp32 [H] (caller zeroes dw). */
int vh_rmsnorm_bwd_bf16(const uint16_t* dy, const uint16_t* x,
                        const uint16_t* w, const float* rstd, uint16_t* dx,
                        float* dw, int64_t T, int64_t H, void* stream);

/* Per-head (H == 128) RMSNorm over strided rows. Every tensor operand is
 * addressed as base + b*sb + s*ss + head*sh (element strides, multiples of
 * 8, D contiguous, 16 B aligned base), so x can be the q or k slice of the
 * fused [B,S,hq+2*hkv,128] qkv projection and y the head-major [B,h,S,128]
 * tensor RoPE and attention take. rstd fp32 [B*S*h] is indexed by the
 * logical row (b*S + s)*h + head, as vh_rmsnorm_fwd_bf16 indexes it on a
 * contiguous [B,S,h,128] copy; y and rstd are bit-equal to that call. */
int vh_rmsnorm128_fwd_strided_bf16(const uint16_t* x, const uint16_t* w,
                                   uint16_t* y, float* rstd, int64_t B,
                                   int64_t S, int64_t h, int64_t x_sb,
                                   int64_t x_ss, int64_t x_sh, int64_t y_sb,
                                   int64_t y_ss, int64_t y_sh, float eps,
                                   void* stream);

/* Backward of the above: dy, x and dx each with their own strides (dx may be
 * a slice of a qkv-gradient buffer; nothing outside the slice is written).
 * dx is bit-equal to vh_rmsnorm_bwd_bf16 on contiguous copies and dw (fp32
 * [128], caller zeroes) gets the same per-wave partials. */
int vh_rmsnorm128_bwd_strided_bf16(const uint16_t* dy, const uint16_t* x,
                                   const uint16_t* w, const float* rstd,
                                   uint16_t* dx, float* dw, int64_t B,
                                   int64_t S, int64_t h, int64_t dy_sb,
                                   int64_t dy_ss, int64_t dy_sh, int64_t x_sb,
                                   int64_t x_ss, int64_t x_sh, int64_t dx_sb,
                                   int64_t dx_ss, int64_t dx_sh, void* stream);

/* ---- RoPE --------------------------------------------------------------- */

/* In-place-capable rotate-half RoPE on [B, h, S, D] q and k with cos/sin
 * [B, S, D] (halves duplicated). backward = same call with negated sin
 * (host passes sign=-1). Replaces Liger RoPE slot (liger/__init__.py:115-126);
 * math matches patched modeling :94-111. */
int vh_rope_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* cos_t,
                 const uint16_t* sin_t, uint16_t* q_out, uint16_t* k_out,
                 int64_t B, int64_t hq, int64_t hk, int64_t S, int64_t D,
                 int negate_sin, void* stream);

/* ---- SwiGLU ------------------------------------------------------------- */

/* out = silu(gate) * up  (bf16; fp32 internal).
 * Replaces LigerSiLUMulFunction slot (liger/__init__.py:130-141). */
int vh_silu_mul_bf16(const uint16_t* gate, const uint16_t* up, uint16_t* out,
                     int64_t n, void* stream);

/* dgate = dy * up * silu'(gate); dup = dy * silu(gate). */
int vh_silu_mul_bwd_bf16(const uint16_t* dy, const uint16_t* gate,
                         const uint16_t* up, uint16_t* dgate, uint16_t* dup,
                         int64_t n, void* stream);

/* ---- Flash attention (causal, GQA, D = 128) ----------------------------- */

/* Forward: O [B,Hq,S,128] bf16, LSE [B,Hq,S] fp32; S % 256 == 0.
 * Replaces the external flash_attn wheel behind the reference's attention
 * slot (attention/flash.py:153-301) for the packed causal path.
 * doc_start (nullable, requires B == 1): int32 [S] per-token document start
 * indices (doc_start[t] = cu_seqlens[i] for t in document i) selecting the
 * packed-varlen block-diagonal causal mask — the reference's flash-attn
 * varlen cu_seqlens path (flash.py:61-91, data_collator.py:50). */
int vh_attn_fwd_bf16(const uint16_t* Q, const uint16_t* K, const uint16_t* V,
                     uint16_t* O, float* LSE, int B, int Hq, int Hkv,
                     int64_t S, float scale, const int32_t* doc_start,
                     void* stream);

/* Backward preprocess: delta[r] = rowsum(dO[r] * O[r]), lse2[r] = LSE[r]*log2e
 * over rows = B*Hq*S flattened. */
int vh_attn_bwd_pre_bf16(const uint16_t* dO, const uint16_t* O,
                         const float* LSE, float* delta, float* lse2,
                         int64_t rows, void* stream);

/* Backward: GQA-folded dk/dv kernel (block owns a 64-row kv strip of one KV
 * head and loops the whole Hq/Hkv head group — dK/dV are [B,Hkv,S,128] bf16
 * written once, no per-Q-head intermediates) + dq kernel (block owns 128 q
 * rows, dQ [B,Hq,S,128] bf16 written once — no atomics, no fp32
 * accumulator). delta/lse2 from the preprocess; S % 128 == 0.
 * doc_start/doc_end (nullable together,
 * require B == 1): int32 [S] per-token document bounds for the packed-varlen
 * block-diagonal causal mask (see vh_attn_fwd_bf16). */
int vh_attn_bwd2_bf16(const uint16_t* Q, const uint16_t* K, const uint16_t* V,
                      const uint16_t* dO, const float* delta,
                      const float* lse2, uint16_t* dQ, uint16_t* dK,
                      uint16_t* dV, int B, int Hq, int Hkv, int64_t S,
                      float scale, const int32_t* doc_start,
                      const int32_t* doc_end, void* stream);

/* The three calls above with O (forward, preprocess) and dO (preprocess,
 * backward) addressed as base + b*sb + hq*sh + row*sr: element strides,
 * multiples of 8, 128 <= sr <= 2^20, D contiguous, 16 B aligned base.
 * Token-major [B,S,Hq,128] is {S*Hq*128, 128, Hq*128}, which o_proj reads
 * as [B,S,Hq*128] without a copy. Q, K, V, dQ, dK, dV, LSE, delta and lse2
 * keep their head-major layouts; results are bit-equal to the head-major
 * calls. The preprocess takes one layout for both O and dO. */
int vh_attn_fwd_ostrided_bf16(const uint16_t* Q, const uint16_t* K,
                              const uint16_t* V, uint16_t* O, float* LSE,
                              int B, int Hq, int Hkv, int64_t S, float scale,
                              const int32_t* doc_start, int64_t o_sb,
                              int64_t o_sh, int64_t o_sr, void* stream);

int vh_attn_bwd_pre_ostrided_bf16(const uint16_t* dO, const uint16_t* O,
                                  const float* LSE, float* delta, float* lse2,
                                  int B, int Hq, int64_t S, int64_t o_sb,
                                  int64_t o_sh, int64_t o_sr, void* stream);

int vh_attn_bwd2_ostrided_bf16(const uint16_t* Q, const uint16_t* K,
                               const uint16_t* V, const uint16_t* dO,
                               const float* delta, const float* lse2,
                               uint16_t* dQ, uint16_t* dK, uint16_t* dV, int B,
                               int Hq, int Hkv, int64_t S, float scale,
                               const int32_t* doc_start,
                               const int32_t* doc_end, int64_t do_sb,
                               int64_t do_sh, int64_t do_sr, void* stream);

/* Sliding-window attention and attention sinks (the reference forwards
 * sliding_window and s_aux to its flash kernels, attention/flash.py:249-288).
 * The strided calls above with
 *   lo, hi  (nullable; bwd2 takes both or neither) int32 [S] key-window
 *           bounds shared by every batch row, so B > 1 is allowed: row q sees
 *           keys lo[q] .. q, and key j is seen by rows j .. hi[j]-1. For a
 *           causal window of W keys inside documents [doc_start, doc_end):
 *           lo[q] = max(doc_start[q], q-W+1), hi[j] = min(doc_end[j], j+W).
 *           Both must be monotone non-decreasing with lo[q] <= q < hi[q] <= S
 *           (the kernels skip whole tiles from them); a packed batch still
 *           means B == 1, which the caller enforces.
 *   sinks   (nullable) fp32 [Hq]: one more softmax column per row of head h
 *           with the logit sinks[h] (natural-log domain, not multiplied by
 *           scale) and a zero value vector. LSE includes it. The preprocess
 *           then also writes dsinks[h] = -sum_{b,s} exp(sinks[h] - LSE) *
 *           delta (fp32 [Hq]) through partials (fp32 [B*Hq*S/256] workspace),
 *           summed in a fixed order without atomics; with sinks == NULL it is
 *           vh_attn_bwd_pre_ostrided_bf16. bwd2 needs only the sink-inclusive
 *           lse2.
 * All three: S % 256 == 0, scale > 0, the stride rules above. */
int vh_attn_fwd_win_sink_bf16(const uint16_t* Q, const uint16_t* K,
                              const uint16_t* V, uint16_t* O, float* LSE,
                              int B, int Hq, int Hkv, int64_t S, float scale,
                              const int32_t* lo, const float* sinks,
                              int64_t o_sb, int64_t o_sh, int64_t o_sr,
                              void* stream);

int vh_attn_bwd_pre_sink_bf16(const uint16_t* dO, const uint16_t* O,
                              const float* LSE, const float* sinks,
                              float* delta, float* lse2, float* dsinks,
                              float* partials, int B, int Hq, int64_t S,
                              int64_t o_sb, int64_t o_sh, int64_t o_sr,
                              void* stream);

int vh_attn_bwd2_win_bf16(const uint16_t* Q, const uint16_t* K,
                          const uint16_t* V, const uint16_t* dO,
                          const float* delta, const float* lse2, uint16_t* dQ,
                          uint16_t* dK, uint16_t* dV, int B, int Hq, int Hkv,
                          int64_t S, float scale, const int32_t* lo,
                          const int32_t* hi, int64_t do_sb, int64_t do_sh,
                          int64_t do_sr, void* stream);

/* ---- Fused optimizer ----------------------------------------------------- */

/* One-sweep AdamW over a device pointer table (torch semantics: decoupled
 * weight decay, bias correction; fp32 math, bf16 p/g/m/v storage). prefix is
 * the inclusive element prefix sum [T+1] (all sizes 8-multiples); grad_scale
 * (nullable fp32) divides grads in-register (grad-clip fold). */
int vh_adamw_bf16(const uint64_t* p_ptrs, const uint64_t* g_ptrs,
                  const uint64_t* m_ptrs, const uint64_t* v_ptrs,
                  const int64_t* prefix, int T, int64_t total, float lr,
                  float beta1, float beta2, float eps, float weight_decay,
                  int step, const float* grad_scale, void* stream);

/* ---- Fused chunked cross-entropy ---------------------------------------- */

/* Per-row softmax CE over a bf16 logits chunk:
 *   loss_rows[r]  = is_valid * (logsumexp(logits[r]) - logits[r][label]);
 *   dlogits[r][v] = is_valid * (softmax - onehot) * grad_scale.
 * fp32 online logsumexp; ignored rows (label == ignore_index) produce 0.
 * Replaces the inner loop of chunk_loss (ref chunk_loss.py:109-127 +
 * transformers fixed_cross_entropy). */
int vh_ce_fwd_bf16(const uint16_t* logits, const int64_t* labels,
                   float* loss_rows, uint16_t* dlogits, int64_t rows,
                   int64_t V, float grad_scale, int64_t ignore_index,
                   void* stream);

/* ---- Fused per-token log-probs and entropy ------------------------------- */

/* Per-row log p(label) and softmax entropy over a bf16 logits chunk
 * [rows, V] (row-contiguous, V % 8 == 0), fp32 math, one read of each row:
 *   log_probs[r] = f_y - lse,  entropy[r] = lse - sum_j p_j f_j,
 * both exactly 0 where labels[r] == ignore_index (such rows are not read).
 * f = logits scaled by inv_temperature in bf16 (skipped when it is 1.0f):
 * f = bf16(float(x) * inv_temperature). lse / ent_raw (the row statistics
 * vh_logprob_bwd_bf16 needs; 0 on ignored rows) may be null. No atomics:
 * bit-reproducible run to run. Labels outside [0, V) other than
 * ignore_index are never dereferenced and give log_probs = NaN.
 * Replaces the fp32 [chunk, V] softmax / logsumexp / gather chain of the
 * reference's chunk_logprobs forward (ref chunk_logprobs.py:165-189). */
int vh_logprob_fwd_bf16(const uint16_t* logits, const int64_t* labels,
                        float* log_probs, float* entropy, float* lse,
                        float* ent_raw, int64_t rows, int64_t V,
                        float inv_temperature, int64_t ignore_index,
                        void* stream);

/* Gradient of the above w.r.t. the (unscaled) logits, one pass:
 *   p_j = exp(f_j - lse),
 *   dlogits[r,j] = dlp_r (1[j==y_r] - p_j) - dent_r p_j ((f_j - lse_r) + H_r),
 * rounded once to bf16 and then scaled by inv_temperature in bf16 (skipped
 * when it is 1.0f). dlog_probs / dentropy may each be null (term dropped);
 * ignored rows write zeros. lse / ent_raw: the forward's statistics.
 * Replaces ref chunk_logprobs.py:225-263. */
int vh_logprob_bwd_bf16(const uint16_t* logits, const int64_t* labels,
                        const float* lse, const float* ent_raw,
                        const float* dlog_probs, const float* dentropy,
                        uint16_t* dlogits, int64_t rows, int64_t V,
                        float inv_temperature, int64_t ignore_index,
                        void* stream);

/* ---- Fused top-k forward-KL distillation --------------------------------- */

/* Per-row top-k forward KL against a teacher given as K ids (int64
 * [rows, K]) and K log-probs (fp32 [rows, K]), on the same bf16 logits chunk
 * and with the lse that vh_logprob_fwd_bf16 wrote. With f as above and
 * s_k = f[ids[r,k]] - lse[r], t_k = tlp[r,k]:
 *   student_mass[r] = sum_k exp(s_k),  teacher_mass[r] = sum_k exp(t_k),
 *   distill[r]      = sum_k exp(t'_k) (t'_k - s'_k),
 * x' = max(x, clamp) when has_clamp != 0, else x; the masses are taken
 * before the clamp. 1 <= K <= 1024. Rows with labels[r] == ignore_index write
 * three zeros and read neither ids nor tlp. Every id is range-checked before
 * it forms an address: one outside [0, V) gives NaN in distill and
 * student_mass of its row. No atomics: bit-reproducible run to run.
 * Replaces the fp32 [chunk, V] log_softmax + gather of the reference's
 * chunk_topk_distill forward (ref chunk_topk_distill.py:170-193). */
int vh_topk_kl_fwd_bf16(const uint16_t* logits, const int64_t* labels,
                        const float* lse, const int64_t* ids, const float* tlp,
                        float* distill, float* student_mass,
                        float* teacher_mass, int64_t rows, int64_t V,
                        int64_t K, float inv_temperature, int has_clamp,
                        float clamp, int64_t ignore_index, void* stream);

/* vh_logprob_bwd_bf16 plus the distillation term, one pass over the row:
 *   w_k = exp(t'_k) * (has_clamp ? s_k >= clamp : 1),  M = sum_k w_k,
 *   dlogits[r,j] = dlp_r (1[j==y_r] - p_j) - dent_r p_j ((f_j - lse_r) + H_r)
 *                + ddist_r (M p_j - sum_{k: ids[r,k]==j} w_k),
 * summed in fp32, rounded once to bf16, then scaled by inv_temperature in
 * bf16. Duplicate ids add up; an id may equal the label; ids outside [0, V)
 * are skipped. Each of the three upstream gradients may be null; with
 * ddistill null this is vh_logprob_bwd_bf16 (ids / tlp unused). Ignored rows
 * write zeros and read neither ids nor tlp. No atomics. V < 2^31,
 * 1 <= K <= 1024. Replaces the dense scatter_add / softmax chain of ref
 * chunk_topk_distill.py:252-311. */
int vh_topk_distill_bwd_bf16(const uint16_t* logits, const int64_t* labels,
                             const float* lse, const float* ent_raw,
                             const int64_t* ids, const float* tlp,
                             const float* dlog_probs, const float* dentropy,
                             const float* ddistill, uint16_t* dlogits,
                             int64_t rows, int64_t V, int64_t K,
                             float inv_temperature, int has_clamp, float clamp,
                             int64_t ignore_index, void* stream);

/* ---- Fused MoE load-balancing (aux) loss --------------------------------- */

/* Switch-transformer aux loss over per-layer router logits [T, E] with
 * contiguous rows; dtype: 0 = bf16, 1 = fp32; 1 <= top_k <= E <= 256.
 * Replaces the reference's fused provider
 * (load_balancing_loss/triton.py:280-354; semantics eager.py:28-114).
 * Per row: fp32 upcast, max-subtracted softmax p, prob_sum += w*p, and each
 * of the top_k selected experts gets count += w (w = mask_w[t], or 1 when
 * mask_w is null).
 * SELECTION RULE: the top_k largest LOGITS of the row after the upcast, ties
 * to the LOWEST expert index -- equal to the reference's top-k of the
 * probabilities wherever that is unambiguous, and independent of the exp
 * implementation. -inf logits are allowed (p = 0); NaN logits and all--inf
 * rows are outside the contract.
 *
 * Forward, stage 1: launches exactly P blocks that grid-stride over rows;
 * block b writes partial[b,0,:] = weighted expert counts and partial[b,1,:]
 * = weighted probability sums of its rows (zeros if it had none). No
 * atomics: bit-reproducible run to run. partial: fp32 [P, 2, E]. */
int vh_lbl_fwd(const void* logits, int dtype, const float* mask_w, int64_t T,
               int E, int top_k, float* partial, int P, void* stream);

/* Forward, stage 2: reduces the P_total partial rows of all layers in fixed
 * row order (double accumulation: counts stay exact past 2^24; results
 * stored fp32) into count [E] / prob_sum [E], then out[1] = coef =
 * E / total_w^2 and out[0] = loss = dot(count, prob_sum) * coef; both are 0
 * when total_w == 0 (the reference's early return, without a host sync).
 * total_w: device fp32 [1]. */
int vh_lbl_finish(const float* partial, int64_t P_total, int E,
                  const float* total_w, float* count, float* prob_sum,
                  float* out, void* stream);

/* Backward for one layer (recomputes the row softmax):
 *   grad[t,j] = grad_out*coef*w_t * p_j * (count_j - sum_i p_i count_i),
 * evaluated in fp32 and rounded once to the logits dtype; rows with
 * w_t == 0 get zeros. coef / grad_out: device fp32 [1]; grad_logits [T, E]
 * in the logits dtype.
 * Replaces triton.py's backward kernel (same formula). */
int vh_lbl_bwd(const void* logits, int dtype, const float* mask_w,
               const float* count, const float* coef, const float* grad_out,
               void* grad_logits, int64_t T, int E, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VEOMNI_HIP_H */
