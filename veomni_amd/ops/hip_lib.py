"""ctypes binding of libveomni_hip.so (the C ABI in include/veomni_hip.h).

The product path calls HIP kernels ONLY through here. There is no fallback:
if the library is missing on a machine with a GPU, `get_lib()` raises — the
"hip" kernel registrations must never silently degrade to eager/torch.
"""

from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

_LIB: Optional[ctypes.CDLL] = None

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO_PATH = os.path.join(_PKG_DIR, "libveomni_hip.so")

c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_f32 = ctypes.c_float
c_p = ctypes.c_void_p


def _sig(lib: ctypes.CDLL, name: str, *argtypes) -> None:
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int
    fn.argtypes = list(argtypes)


def get_lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f"libveomni_hip.so not found at {SO_PATH}. Build it with "
            "`python veomni_amd/csrc/build.py` (or __graft_entry__.build()). "
            "The HIP op path has NO fallback by design."
        )
    lib = ctypes.CDLL(SO_PATH)
    lib.vh_last_error.restype = ctypes.c_char_p
    lib.vh_build_info.restype = ctypes.c_char_p
    _sig(lib, "vh_expert_histogram", c_p, c_i64, c_int, c_p, c_p)
    _sig(lib, "vh_moe_scatter_bf16", c_p, c_p, c_p, c_i64, c_i64, c_int, c_p)
    _sig(lib, "vh_moe_gather_bf16", c_p, c_p, c_p, c_i64, c_i64, c_int, c_p)
    _sig(lib, "vh_group_gemm_nk_bf16", c_p, c_p, c_p, c_p, c_int, c_i64, c_i64,
         c_i64, c_int, c_int, c_int, c_p)
    _sig(lib, "vh_group_gemm_nk8_bf16", c_p, c_p, c_p, c_p, c_int, c_i64, c_i64,
         c_i64, c_int, c_p)
    _sig(lib, "vh_group_gemm_nk256s_bf16", c_p, c_p, c_p, c_p, c_int, c_i64,
         c_i64, c_i64, c_p)
    _sig(lib, "vh_group_gemm_nk256s_kn_bf16", c_p, c_p, c_p, c_p, c_int, c_i64,
         c_i64, c_i64, c_p)
    _sig(lib, "vh_group_gemm_mn_bf16", c_p, c_p, c_p, c_p, c_int, c_i64, c_i64, c_p)
    _sig(lib, "vh_wtranspose_bf16", c_p, c_p, c_int, c_i64, c_i64, c_p)
    _sig(lib, "vh_group_gemm_wgd_bf16", c_p, c_p, c_p, c_p, c_int, c_i64,
         c_i64, c_i64, c_p)
    _sig(lib, "vh_moe_silu_mul_weighted_bf16", c_p, c_p, c_p, c_i64, c_i64, c_int, c_p)
    _sig(lib, "vh_moe_silu_mul_weighted_bwd_bf16", c_p, c_p, c_p, c_p, c_p,
         c_i64, c_i64, c_int, c_p)
    _sig(lib, "vh_moe_silu_mul_clamp_weighted_bf16", c_p, c_p, c_p, c_i64, c_i64,
         c_int, c_f32, c_p)
    _sig(lib, "vh_moe_silu_mul_clamp_weighted_bwd_bf16", c_p, c_p, c_p, c_p, c_p,
         c_i64, c_i64, c_int, c_f32, c_p)
    _sig(lib, "vh_moe_gptoss_glu_bf16", c_p, c_p, c_p, c_p, c_i64, c_i64, c_int,
         c_f32, c_f32, c_p)
    _sig(lib, "vh_moe_gptoss_glu_bwd_bf16", c_p, c_p, c_p, c_p, c_p, c_i64,
         c_i64, c_int, c_f32, c_f32, c_p)
    _sig(lib, "vh_moe_expert_bias_scale_bf16", c_p, c_p, c_p, c_p, c_p, c_i64,
         c_i64, c_int, c_p)
    _sig(lib, "vh_moe_expert_bias_scale_bwd_bf16", c_p, c_p, c_p, c_p, c_p, c_p,
         c_p, c_i64, c_i64, c_int, c_p)
    _sig(lib, "vh_moe_segment_colsum_bf16", c_p, c_p, c_p, c_i64, c_i64, c_int,
         c_p)
    _sig(lib, "vh_rmsnorm_fwd_bf16", c_p, c_p, c_p, c_p, c_i64, c_i64, c_f32, c_p)
    _sig(lib, "vh_rmsnorm_bwd_bf16", c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_i64, c_p)
    _sig(lib, "vh_rmsnorm128_fwd_strided_bf16", c_p, c_p, c_p, c_p, c_i64, c_i64,
         c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_f32, c_p)
    _sig(lib, "vh_rmsnorm128_bwd_strided_bf16", c_p, c_p, c_p, c_p, c_p, c_p,
         c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64,
         c_i64, c_i64, c_p)
    _sig(lib, "vh_rope_bf16", c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64,
         c_i64, c_i64, c_int, c_p)
    _sig(lib, "vh_silu_mul_bf16", c_p, c_p, c_p, c_i64, c_p)
    _sig(lib, "vh_silu_mul_bwd_bf16", c_p, c_p, c_p, c_p, c_p, c_i64, c_p)
    _sig(lib, "vh_ce_fwd_bf16", c_p, c_p, c_p, c_p, c_i64, c_i64, c_f32, c_i64, c_p)
    _sig(lib, "vh_logprob_fwd_bf16", c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_i64,
         c_f32, c_i64, c_p)
    _sig(lib, "vh_logprob_bwd_bf16", c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i64,
         c_i64, c_f32, c_i64, c_p)
    _sig(lib, "vh_topk_kl_fwd_bf16", c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
         c_i64, c_i64, c_i64, c_f32, c_int, c_f32, c_i64, c_p)
    _sig(lib, "vh_topk_distill_bwd_bf16", c_p, c_p, c_p, c_p, c_p, c_p, c_p,
         c_p, c_p, c_p, c_i64, c_i64, c_i64, c_f32, c_int, c_f32, c_i64, c_p)
    _sig(lib, "vh_adamw_bf16", c_p, c_p, c_p, c_p, c_p, c_int, c_i64, c_f32,
         c_f32, c_f32, c_f32, c_f32, c_int, c_p, c_p)
    _sig(lib, "vh_attn_fwd_bf16", c_p, c_p, c_p, c_p, c_p, c_int, c_int, c_int,
         c_i64, c_f32, c_p, c_p)
    _sig(lib, "vh_attn_bwd_pre_bf16", c_p, c_p, c_p, c_p, c_p, c_i64, c_p)
    _sig(lib, "vh_attn_bwd2_bf16", c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
         c_int, c_int, c_int, c_i64, c_f32, c_p, c_p, c_p)
    _sig(lib, "vh_attn_fwd_ostrided_bf16", c_p, c_p, c_p, c_p, c_p, c_int, c_int,
         c_int, c_i64, c_f32, c_p, c_i64, c_i64, c_i64, c_p)
    _sig(lib, "vh_attn_bwd_pre_ostrided_bf16", c_p, c_p, c_p, c_p, c_p, c_int,
         c_int, c_i64, c_i64, c_i64, c_i64, c_p)
    _sig(lib, "vh_attn_bwd2_ostrided_bf16", c_p, c_p, c_p, c_p, c_p, c_p, c_p,
         c_p, c_p, c_int, c_int, c_int, c_i64, c_f32, c_p, c_p, c_i64, c_i64,
         c_i64, c_p)
    _sig(lib, "vh_attn_fwd_win_sink_bf16", c_p, c_p, c_p, c_p, c_p, c_int, c_int,
         c_int, c_i64, c_f32, c_p, c_p, c_i64, c_i64, c_i64, c_p)
    _sig(lib, "vh_attn_bwd_pre_sink_bf16", c_p, c_p, c_p, c_p, c_p, c_p, c_p,
         c_p, c_int, c_int, c_i64, c_i64, c_i64, c_i64, c_p)
    _sig(lib, "vh_attn_bwd2_win_bf16", c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
         c_p, c_int, c_int, c_int, c_i64, c_f32, c_p, c_p, c_i64, c_i64, c_i64,
         c_p)
    _sig(lib, "vh_lbl_fwd", c_p, c_int, c_p, c_i64, c_int, c_int, c_p, c_int, c_p)
    _sig(lib, "vh_lbl_finish", c_p, c_i64, c_int, c_p, c_p, c_p, c_p, c_p)
    _sig(lib, "vh_lbl_bwd", c_p, c_int, c_p, c_p, c_p, c_p, c_p, c_i64, c_int, c_p)
    _LIB = lib
    return lib


def cur_stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------- event profiling
# bench.py's roofline leg: when enabled, each wrapped kernel call records a
# (start, end) HIP event pair on ITS launch stream plus the call's
# algorithmic work, so average per-launch durations can be read back.
_PROFILE = False
_PROF_EVENTS: dict = {}


def profile_enable(on: bool = True) -> None:
    global _PROFILE
    _PROFILE = on
    if on:
        _PROF_EVENTS.clear()


def profile_events() -> dict:
    return _PROF_EVENTS


def profile_summary() -> dict:
    """{name: {"count": n, "ms_avg": per-launch ms, "work": [payloads]}}."""
    torch.cuda.synchronize()
    out = {}
    for name, recs in _PROF_EVENTS.items():
        times = [s.elapsed_time(e) for s, e, _ in recs]
        out[name] = {
            "count": len(recs),
            "ms_avg": sum(times) / max(len(times), 1),
            "ms_total": sum(times),
            "work": [w for _, _, w in recs],
        }
    return out


class _prof:
    def __init__(self, name: str, work=None):
        self.name = name
        self.work = work

    def __enter__(self):
        if _PROFILE:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *a):
        if _PROFILE:
            self.e.record()
            _PROF_EVENTS.setdefault(self.name, []).append((self.s, self.e, self.work))


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {get_lib().vh_last_error().decode()}")


def dptr(t: torch.Tensor) -> int:
    return t.data_ptr()


# ------------------------------------------------------------- typed wrappers
def expert_histogram(expert_index: torch.Tensor, num_experts: int) -> torch.Tensor:
    assert expert_index.dtype == torch.int64
    flat = expert_index.flatten().contiguous()
    out = torch.empty(num_experts, dtype=torch.int32, device=flat.device)
    check(get_lib().vh_expert_histogram(dptr(flat), flat.numel(), num_experts,
                                        dptr(out), cur_stream()), "vh_expert_histogram")
    return out


def moe_scatter(x: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    M, N = x.shape
    topk = index.shape[1] if index.dim() == 2 else 1
    idx = index.reshape(-1).to(torch.int32).contiguous()
    out = torch.empty(M * topk, N, dtype=x.dtype, device=x.device)
    check(get_lib().vh_moe_scatter_bf16(dptr(x.contiguous()), dptr(idx), dptr(out),
                                        M, N, topk, cur_stream()), "vh_moe_scatter")
    return out


def moe_gather(x: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    M, topk = index.shape
    N = x.shape[1]
    idx = index.reshape(-1).to(torch.int32).contiguous()
    out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    check(get_lib().vh_moe_gather_bf16(dptr(x.contiguous()), dptr(idx), dptr(out),
                                       M, N, topk, cur_stream()), "vh_moe_gather")
    return out


def group_gemm_nk(a: torch.Tensor, b: torch.Tensor, cumsum: torch.Tensor,
                  trans_b: bool, c: torch.Tensor | None = None,
                  activation: int = 0) -> torch.Tensor:
    """C_g = A_g @ (B_g^T if trans_b else B_g); rows partitioned by cumsum."""
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16
    G = b.shape[0]
    N = b.shape[1] if trans_b else b.shape[2]
    K = b.shape[2] if trans_b else b.shape[1]
    assert a.shape[1] == K, (a.shape, b.shape, trans_b)
    if K % 64 != 0:
        # zero-pad the reduction dim to the kernel's BK multiple (only test
        # shapes hit this; every production K — H, I, 2I — is a 64-multiple)
        pad = 64 - K % 64
        a = torch.nn.functional.pad(a, (0, pad))
        b = torch.nn.functional.pad(b, (0, pad) if trans_b else (0, 0, 0, pad))
        K = K + pad
    accumulate = c is not None
    if c is None:
        c = torch.empty(a.shape[0], N, dtype=a.dtype, device=a.device)
    cs = cumsum.to(torch.int64).contiguous()
    # algorithmic flops = 2 * total_rows * N * K (every A row belongs to one group)
    with _prof("group_gemm_nk", 2.0 * a.shape[0] * N * K):
        check(get_lib().vh_group_gemm_nk_bf16(
            dptr(a.contiguous()), dptr(b.contiguous()), dptr(c), dptr(cs), G, N, K,
            a.shape[0], int(trans_b), int(accumulate), activation, cur_stream()),
            "vh_group_gemm_nk")
    return c


def group_gemm_mn(a: torch.Tensor, b: torch.Tensor, cumsum: torch.Tensor,
                  G: int) -> torch.Tensor:
    """C[g] = A_g^T @ B_g; A [rows, M], B [rows, N] -> C [G, M, N].

    Large shapes take the direct wgrad kernel: both operands are read
    token-major as they are (no transposed/padded copies, no temporaries);
    the kernel stages [64 k][256 out] tiles and transposes in the LDS read."""
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16
    rows = a.shape[0]
    M, N = a.shape[1], b.shape[1]
    c = torch.empty(G, M, N, dtype=a.dtype, device=a.device)
    cs = cumsum.to(torch.int64).contiguous()
    if M >= 512 and N >= 512 and rows >= 2048:
        with _prof("group_gemm_mn", 2.0 * rows * M * N):
            check(get_lib().vh_group_gemm_wgd_bf16(
                dptr(a.contiguous()), dptr(b.contiguous()), dptr(c), dptr(cs), G,
                M, N, rows, cur_stream()), "vh_group_gemm_wgd")
        return c
    with _prof("group_gemm_mn", 2.0 * rows * M * N):
        check(get_lib().vh_group_gemm_mn_bf16(
            dptr(a.contiguous()), dptr(b.contiguous()), dptr(c), dptr(cs), G, M, N,
            cur_stream()), "vh_group_gemm_mn")
    return c


def weight_transpose(b: torch.Tensor) -> torch.Tensor:
    """[E, M, N] -> [E, N, M] contiguous. HIP tile kernel for 64-multiple
    shapes; torch copy otherwise. The MoE dgrad no longer needs it (it reads
    the stored weights with trans_b=False); kept as a utility."""
    E, M, N = b.shape
    if M % 64 or N % 64 or b.dtype != torch.bfloat16:
        return b.transpose(1, 2).contiguous()
    out = torch.empty(E, N, M, dtype=b.dtype, device=b.device)
    with _prof("wtranspose", 2.0 * E * M * N * 2):
        check(get_lib().vh_wtranspose_bf16(dptr(b.contiguous()), dptr(out), E,
                                           M, N, cur_stream()), "vh_wtranspose")
    return out


def swiglu_limit_bf16(limit: float) -> float:
    """The limit as the clamped kernels receive it: rounded to bf16
    (round-to-nearest-even). A bf16 `clamp` / `<=` against a Python scalar
    behaves as if the scalar had this value (bf16 7.125 <= 7.12 is True)."""
    return float(torch.tensor(limit, dtype=torch.bfloat16))


def silu_mul_weighted(fc1: torch.Tensor, w_row: torch.Tensor | None,
                      limit: float | None = None) -> torch.Tensor:
    """silu(gate) * up * w_row over merged fc1 [rows, 2I]; with `limit` the
    clamped-SwiGLU entry (gate <= L, -L <= up <= L, L = bf16(limit))."""
    rows, twoI = fc1.shape
    I = twoI // 2
    out = torch.empty(rows, I, dtype=fc1.dtype, device=fc1.device)
    has_w = w_row is not None
    if limit is not None:
        check(get_lib().vh_moe_silu_mul_clamp_weighted_bf16(
            dptr(fc1.contiguous()), dptr(w_row.contiguous()) if has_w else None,
            dptr(out), rows, I, int(has_w), swiglu_limit_bf16(limit),
            cur_stream()), "vh_moe_silu_mul_clamp_weighted")
        return out
    check(get_lib().vh_moe_silu_mul_weighted_bf16(
        dptr(fc1.contiguous()), dptr(w_row.contiguous()) if has_w else None,
        dptr(out), rows, I, int(has_w), cur_stream()), "vh_moe_silu_mul_weighted")
    return out


def silu_mul_weighted_bwd(dy: torch.Tensor, fc1: torch.Tensor,
                          w_row: torch.Tensor | None,
                          limit: float | None = None):
    """Backward of silu_mul_weighted from the RAW saved fc1: (dfc1, dw_row).
    With `limit`, clamp and gradient mask are recomputed in the kernel and
    dw_row is stored, not accumulated, so it is allocated uninitialised."""
    rows, twoI = fc1.shape
    I = twoI // 2
    dfc1 = torch.empty_like(fc1)
    has_w = w_row is not None
    if limit is not None:
        dw_row = torch.empty(rows, dtype=torch.float32, device=fc1.device) if has_w else None
        check(get_lib().vh_moe_silu_mul_clamp_weighted_bwd_bf16(
            dptr(dy.contiguous()), dptr(fc1.contiguous()),
            dptr(w_row.contiguous()) if has_w else None, dptr(dfc1),
            dptr(dw_row) if has_w else None, rows, I, int(has_w),
            swiglu_limit_bf16(limit), cur_stream()),
            "vh_moe_silu_mul_clamp_weighted_bwd")
        return dfc1, dw_row
    dw_row = torch.zeros(rows, dtype=torch.float32, device=fc1.device) if has_w else None
    check(get_lib().vh_moe_silu_mul_weighted_bwd_bf16(
        dptr(dy.contiguous()), dptr(fc1.contiguous()),
        dptr(w_row.contiguous()) if has_w else None, dptr(dfc1),
        dptr(dw_row) if has_w else None, rows, I, int(has_w), cur_stream()),
        "vh_moe_silu_mul_weighted_bwd")
    return dfc1, dw_row


# ---- gpt-oss experts (vh_moe_gpt_oss.hip) ----------------------------------
def _cumsum_i64(cumsum: torch.Tensor, G: int | None = None) -> torch.Tensor:
    assert G is None or cumsum.numel() == G, (cumsum.shape, G)
    return cumsum.to(torch.int64).contiguous()


def gptoss_glu(fc1: torch.Tensor, bias: torch.Tensor, cumsum: torch.Tensor,
               alpha: float, limit: float) -> torch.Tensor:
    """(up + 1) * gate * sigmoid(alpha * gate) on the clamped, biased,
    INTERLEAVED pre-activation: fc1 [rows, 2I] is the raw grouped-GEMM output,
    bias [G, 2I] is added per expert in the kernel (L = bf16(limit))."""
    assert fc1.dtype == torch.bfloat16 and bias.dtype == torch.bfloat16
    rows, twoI = fc1.shape
    I = twoI // 2
    assert bias.shape[1] == twoI, (fc1.shape, bias.shape)
    G = bias.shape[0]
    out = torch.empty(rows, I, dtype=fc1.dtype, device=fc1.device)
    with _prof("gptoss_glu", 2.0 * rows * 3 * I):
        check(get_lib().vh_moe_gptoss_glu_bf16(
            dptr(fc1.contiguous()), dptr(bias.contiguous()),
            dptr(_cumsum_i64(cumsum, G)), dptr(out), rows, I, G, float(alpha),
            swiglu_limit_bf16(limit), cur_stream()), "vh_moe_gptoss_glu")
    return out


def gptoss_glu_bwd(dy: torch.Tensor, fc1: torch.Tensor, bias: torch.Tensor,
                   cumsum: torch.Tensor, alpha: float,
                   limit: float) -> torch.Tensor:
    """dfc1 [rows, 2I] (interleaved) of gptoss_glu, recomputed from the raw
    fc1 and the bias; zero outside the inclusive clamp bounds."""
    assert fc1.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16
    rows, twoI = fc1.shape
    I = twoI // 2
    assert dy.shape == (rows, I) and bias.shape[1] == twoI
    G = bias.shape[0]
    dfc1 = torch.empty_like(fc1)
    with _prof("gptoss_glu_bwd", 2.0 * rows * 5 * I):
        check(get_lib().vh_moe_gptoss_glu_bwd_bf16(
            dptr(dy.contiguous()), dptr(fc1.contiguous()),
            dptr(bias.contiguous()), dptr(_cumsum_i64(cumsum, G)), dptr(dfc1), rows,
            I, G, float(alpha), swiglu_limit_bf16(limit), cur_stream()),
            "vh_moe_gptoss_glu_bwd")
    return dfc1


def expert_bias_scale(x: torch.Tensor, bias: torch.Tensor, cumsum: torch.Tensor,
                      w_row: torch.Tensor | None) -> torch.Tensor:
    """(x[r] + bias[expert(r)]) * w_row[r]; w_row None is a factor of 1."""
    assert x.dtype == torch.bfloat16 and bias.dtype == torch.bfloat16
    rows, N = x.shape
    assert bias.shape[1] == N, (x.shape, bias.shape)
    if w_row is not None:
        assert w_row.dtype == torch.bfloat16 and w_row.numel() == rows
    out = torch.empty_like(x)
    with _prof("expert_bias_scale", 2.0 * rows * 2 * N):
        check(get_lib().vh_moe_expert_bias_scale_bf16(
            dptr(x.contiguous()), dptr(bias.contiguous()),
            dptr(_cumsum_i64(cumsum, bias.shape[0])),
            dptr(w_row.contiguous()) if w_row is not None else None, dptr(out),
            rows, N, bias.shape[0], cur_stream()), "vh_moe_expert_bias_scale")
    return out


def expert_bias_scale_bwd(dy: torch.Tensor, x: torch.Tensor, bias: torch.Tensor,
                          cumsum: torch.Tensor, w_row: torch.Tensor | None):
    """(dx, dw_row) of expert_bias_scale: dx = dy * w_row[r] and
    dw_row[r] = sum_n (x + bias) * dy (fp32, stored by the kernel, so the
    buffer is allocated uninitialised). w_row None: (a copy of dy, None)."""
    assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
    rows, N = x.shape
    assert dy.shape == x.shape and bias.shape[1] == N
    has_w = w_row is not None
    dx = torch.empty_like(x)
    dw_row = torch.empty(rows, dtype=torch.float32, device=x.device) if has_w else None
    with _prof("expert_bias_scale_bwd", 2.0 * rows * 3 * N):
        check(get_lib().vh_moe_expert_bias_scale_bwd_bf16(
            dptr(dy.contiguous()), dptr(x.contiguous()), dptr(bias.contiguous()),
            dptr(_cumsum_i64(cumsum, bias.shape[0])),
            dptr(w_row.contiguous()) if has_w else None, dptr(dx),
            dptr(dw_row) if has_w else None, rows, N, bias.shape[0],
            cur_stream()), "vh_moe_expert_bias_scale_bwd")
    return dx, dw_row


def segment_colsum(x: torch.Tensor, cumsum: torch.Tensor,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [G, N] column sums of x [rows, N] over each expert's row segment;
    fixed summation order (bit-reproducible), every element written."""
    assert x.dtype == torch.bfloat16
    rows, N = x.shape
    G = cumsum.numel()
    if out is None:
        out = torch.empty(G, N, dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.shape == (G, N) and out.is_contiguous()
    with _prof("segment_colsum", 2.0 * rows * N):
        check(get_lib().vh_moe_segment_colsum_bf16(
            dptr(x.contiguous()), dptr(_cumsum_i64(cumsum)), dptr(out), rows, N,
            G, cur_stream()), "vh_moe_segment_colsum")
    return out


def rmsnorm_fwd(x: torch.Tensor, w: torch.Tensor, eps: float):
    T = x.numel() // x.shape[-1]
    H = x.shape[-1]
    y = torch.empty_like(x)
    rstd = torch.empty(T, dtype=torch.float32, device=x.device)
    with _prof("rmsnorm_fwd", 2.0 * T * H * 2 + T * H * 2):
        check(get_lib().vh_rmsnorm_fwd_bf16(dptr(x.contiguous()), dptr(w.contiguous()),
                                            dptr(y), dptr(rstd), T, H, eps,
                                            cur_stream()), "vh_rmsnorm_fwd")
    return y, rstd


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                rstd: torch.Tensor):
    T = x.numel() // x.shape[-1]
    H = x.shape[-1]
    dx = torch.empty_like(x)
    dw = torch.zeros(H, dtype=torch.float32, device=x.device)
    check(get_lib().vh_rmsnorm_bwd_bf16(dptr(dy.contiguous()), dptr(x.contiguous()),
                                        dptr(w.contiguous()), dptr(rstd), dptr(dx),
                                        dptr(dw), T, H, cur_stream()), "vh_rmsnorm_bwd")
    return dx, dw


def _bsh_strides(t: torch.Tensor):
    """(batch, token, head) element strides of a logical [B,S,h,128] bf16
    tensor whose last dim is contiguous — any view the strided kernels take."""
    assert t.dim() == 4 and t.shape[-1] == 128 and t.dtype == torch.bfloat16, \
        (t.shape, t.dtype)
    assert t.stride(3) == 1 or t.shape[3] == 1, t.stride()
    return t.stride(0), t.stride(1), t.stride(2)


def rmsnorm128_fwd_strided(x: torch.Tensor, w: torch.Tensor, eps: float,
                           y: torch.Tensor | None = None):
    """Per-head RMSNorm of a logical [B,S,h,128] view x (e.g. the q slice of
    the qkv projection), no copy. y is a logical [B,S,h,128] view as well;
    by default the transpose of a fresh head-major [B,h,S,128] buffer.
    Returns (y, rstd fp32 [B*S*h] in (b, s, head) row order)."""
    B, S, h, D = x.shape
    if y is None:
        y = torch.empty(B, h, S, D, dtype=x.dtype, device=x.device).transpose(1, 2)
    assert y.shape == x.shape
    rstd = torch.empty(B * S * h, dtype=torch.float32, device=x.device)
    with _prof("rmsnorm_fwd", 2.0 * B * S * h * D * 2 + B * S * h * D * 2):
        check(get_lib().vh_rmsnorm128_fwd_strided_bf16(
            dptr(x), dptr(w.contiguous()), dptr(y), dptr(rstd), B, S, h,
            *_bsh_strides(x), *_bsh_strides(y), eps, cur_stream()),
            "vh_rmsnorm128_fwd_strided")
    return y, rstd


def rmsnorm128_bwd_strided(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                           rstd: torch.Tensor, dx: torch.Tensor):
    """Backward of rmsnorm128_fwd_strided: dy, x and dx are logical
    [B,S,h,128] views; dx (e.g. a slice of the qkv gradient) is written in
    place and nothing around it is touched. Returns dw fp32 [128]."""
    B, S, h, D = x.shape
    assert dy.shape == x.shape and dx.shape == x.shape
    assert rstd.dtype == torch.float32 and rstd.numel() == B * S * h \
        and rstd.is_contiguous()
    dw = torch.zeros(D, dtype=torch.float32, device=x.device)
    check(get_lib().vh_rmsnorm128_bwd_strided_bf16(
        dptr(dy), dptr(x), dptr(w.contiguous()), dptr(rstd), dptr(dx), dptr(dw),
        B, S, h, *_bsh_strides(dy), *_bsh_strides(x), *_bsh_strides(dx),
        cur_stream()), "vh_rmsnorm128_bwd_strided")
    return dw


def rope(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
         negate_sin: bool = False):
    B, hq, S, D = q.shape
    hk = k.shape[1]
    qo = torch.empty_like(q)
    ko = torch.empty_like(k)
    check(get_lib().vh_rope_bf16(dptr(q.contiguous()), dptr(k.contiguous()),
                                 dptr(cos.contiguous()), dptr(sin.contiguous()),
                                 dptr(qo), dptr(ko), B, hq, hk, S, D,
                                 int(negate_sin), cur_stream()), "vh_rope")
    return qo, ko


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(gate)
    with _prof("silu_mul", 3.0 * gate.numel() * 2):
        check(get_lib().vh_silu_mul_bf16(dptr(gate.contiguous()), dptr(up.contiguous()),
                                         dptr(out), gate.numel(), cur_stream()),
              "vh_silu_mul")
    return out


def silu_mul_bwd(dy: torch.Tensor, gate: torch.Tensor, up: torch.Tensor):
    dg = torch.empty_like(gate)
    du = torch.empty_like(up)
    check(get_lib().vh_silu_mul_bwd_bf16(dptr(dy.contiguous()), dptr(gate.contiguous()),
                                         dptr(up.contiguous()), dptr(dg), dptr(du),
                                         gate.numel(), cur_stream()), "vh_silu_mul_bwd")
    return dg, du


def ce_fwd(logits: torch.Tensor, labels: torch.Tensor, grad_scale: float,
           ignore_index: int = -100, dlogits_out: torch.Tensor | None = None):
    rows, V = logits.shape
    loss_rows = torch.zeros(rows, dtype=torch.float32, device=logits.device)
    dlogits = dlogits_out if dlogits_out is not None else torch.empty_like(logits)
    assert dlogits.is_contiguous() and dlogits.shape == logits.shape
    with _prof("ce_fwd", 3.0 * rows * V * 2):
        check(get_lib().vh_ce_fwd_bf16(dptr(logits.contiguous()),
                                       dptr(labels.to(torch.int64).contiguous()),
                                       dptr(loss_rows), dptr(dlogits), rows, V,
                                       grad_scale, ignore_index, cur_stream()),
              "vh_ce_fwd")
    return loss_rows, dlogits


def inv_temperature(temperature: float) -> float:
    """fp32(1) / fp32(T): the factor ATen's bf16 true-divide by a Python
    scalar multiplies with; exactly 1.0 for T == 1.0 (kernel skips the scale)."""
    one = torch.ones((), dtype=torch.float32)
    return float(one / torch.tensor(float(temperature), dtype=torch.float32))


def _check_logprob_args(logits: torch.Tensor, labels: torch.Tensor) -> None:
    assert logits.dim() == 2 and logits.dtype == torch.bfloat16, \
        "logprob kernels take bf16 logits [rows, V]"
    assert logits.is_contiguous(), "logits must be row-contiguous"
    assert labels.shape == (logits.shape[0],), (labels.shape, logits.shape)
    assert labels.dtype == torch.int64 and labels.is_contiguous()


def logprob_fwd(logits: torch.Tensor, labels: torch.Tensor,
                temperature: float = 1.0, ignore_index: int = -100,
                want_stats: bool = True):
    """Per-row (log_probs, entropy, lse, ent_raw), all fp32 [rows]; lse and
    ent_raw (the statistics logprob_bwd needs) are None without want_stats."""
    _check_logprob_args(logits, labels)
    rows, V = logits.shape
    dev = logits.device
    log_probs = torch.empty(rows, dtype=torch.float32, device=dev)
    entropy = torch.empty(rows, dtype=torch.float32, device=dev)
    lse = torch.empty(rows, dtype=torch.float32, device=dev) if want_stats else None
    ent_raw = torch.empty(rows, dtype=torch.float32, device=dev) if want_stats else None
    with _prof("logprob_fwd", 2.0 * rows * V):
        check(get_lib().vh_logprob_fwd_bf16(
            dptr(logits), dptr(labels), dptr(log_probs), dptr(entropy),
            dptr(lse) if want_stats else None,
            dptr(ent_raw) if want_stats else None,
            rows, V, inv_temperature(temperature), ignore_index, cur_stream()),
            "vh_logprob_fwd")
    return log_probs, entropy, lse, ent_raw


def logprob_bwd(logits: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor,
                ent_raw: torch.Tensor, dlp: torch.Tensor | None,
                dent: torch.Tensor | None, temperature: float = 1.0,
                ignore_index: int = -100,
                dlogits_out: torch.Tensor | None = None) -> torch.Tensor:
    """dlogits (bf16, [rows, V]) from the per-row upstream gradients; a None
    upstream drops its term."""
    _check_logprob_args(logits, labels)
    rows, V = logits.shape
    for t in (lse, ent_raw, dlp, dent):
        assert t is None or (t.dtype == torch.float32 and t.shape == (rows,)
                             and t.is_contiguous())
    assert lse is not None and ent_raw is not None
    dlogits = dlogits_out if dlogits_out is not None else torch.empty_like(logits)
    assert dlogits.is_contiguous() and dlogits.shape == logits.shape \
        and dlogits.dtype == logits.dtype
    with _prof("logprob_bwd", 4.0 * rows * V):
        check(get_lib().vh_logprob_bwd_bf16(
            dptr(logits), dptr(labels), dptr(lse), dptr(ent_raw),
            dptr(dlp) if dlp is not None else None,
            dptr(dent) if dent is not None else None,
            dptr(dlogits), rows, V, inv_temperature(temperature), ignore_index,
            cur_stream()), "vh_logprob_bwd")
    return dlogits


TOPK_MAX = 1024   # kMaxTopk in vh_logprob.hip: the backward parks K (id, w) pairs in LDS


def _check_topk_args(logits: torch.Tensor, ids: torch.Tensor,
                     tlp: torch.Tensor) -> int:
    rows = logits.shape[0]
    assert ids.dim() == 2 and ids.shape[0] == rows, (ids.shape, logits.shape)
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    assert tlp.shape == ids.shape and tlp.dtype == torch.float32 \
        and tlp.is_contiguous(), (tlp.shape, tlp.dtype)
    K = ids.shape[1]
    assert 1 <= K <= TOPK_MAX, f"K = {K} outside [1, {TOPK_MAX}]"
    return K


def topk_kl_fwd(logits: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor,
                ids: torch.Tensor, tlp: torch.Tensor, temperature: float = 1.0,
                log_prob_min_clamp: float | None = None,
                ignore_index: int = -100):
    """Per-row (distill, student_mass, teacher_mass), fp32 [rows], from the
    teacher's top-k ids (int64 [rows, K]) and log-probs (fp32 [rows, K]) and
    the lse logprob_fwd wrote for the same logits and temperature."""
    _check_logprob_args(logits, labels)
    K = _check_topk_args(logits, ids, tlp)
    rows, V = logits.shape
    assert lse.dtype == torch.float32 and lse.shape == (rows,) and lse.is_contiguous()
    dev = logits.device
    distill = torch.empty(rows, dtype=torch.float32, device=dev)
    student_mass = torch.empty(rows, dtype=torch.float32, device=dev)
    teacher_mass = torch.empty(rows, dtype=torch.float32, device=dev)
    has_clamp = log_prob_min_clamp is not None
    with _prof("topk_kl_fwd", rows * (14.0 * K + 24.0)):
        check(get_lib().vh_topk_kl_fwd_bf16(
            dptr(logits), dptr(labels), dptr(lse), dptr(ids), dptr(tlp),
            dptr(distill), dptr(student_mass), dptr(teacher_mass), rows, V, K,
            inv_temperature(temperature), int(has_clamp),
            float(log_prob_min_clamp) if has_clamp else 0.0, ignore_index,
            cur_stream()), "vh_topk_kl_fwd")
    return distill, student_mass, teacher_mass


def topk_distill_bwd(logits: torch.Tensor, labels: torch.Tensor,
                     lse: torch.Tensor, ent_raw: torch.Tensor,
                     ids: torch.Tensor, tlp: torch.Tensor,
                     dlp: torch.Tensor | None, dent: torch.Tensor | None,
                     ddist: torch.Tensor | None, temperature: float = 1.0,
                     log_prob_min_clamp: float | None = None,
                     ignore_index: int = -100,
                     dlogits_out: torch.Tensor | None = None) -> torch.Tensor:
    """logprob_bwd plus the top-k distillation term, one pass; a None
    upstream drops its term, and ddist=None is logprob_bwd bit for bit."""
    _check_logprob_args(logits, labels)
    K = _check_topk_args(logits, ids, tlp)
    rows, V = logits.shape
    for t in (lse, ent_raw, dlp, dent, ddist):
        assert t is None or (t.dtype == torch.float32 and t.shape == (rows,)
                             and t.is_contiguous())
    assert lse is not None and ent_raw is not None
    dlogits = dlogits_out if dlogits_out is not None else torch.empty_like(logits)
    assert dlogits.is_contiguous() and dlogits.shape == logits.shape \
        and dlogits.dtype == logits.dtype
    has_clamp = log_prob_min_clamp is not None
    with _prof("topk_distill_bwd", 4.0 * rows * V + 18.0 * rows * K):
        check(get_lib().vh_topk_distill_bwd_bf16(
            dptr(logits), dptr(labels), dptr(lse), dptr(ent_raw), dptr(ids),
            dptr(tlp),
            dptr(dlp) if dlp is not None else None,
            dptr(dent) if dent is not None else None,
            dptr(ddist) if ddist is not None else None,
            dptr(dlogits), rows, V, K, inv_temperature(temperature),
            int(has_clamp), float(log_prob_min_clamp) if has_clamp else 0.0,
            ignore_index, cur_stream()), "vh_topk_distill_bwd")
    return dlogits


def attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float,
             doc_start: torch.Tensor | None = None):
    """Causal GQA flash attention forward: q [B,Hq,S,128] bf16 contiguous,
    k/v [B,Hkv,S,128]. Returns (o, lse). doc_start (int32 [S], B == 1)
    selects the packed-varlen block-diagonal mask (reference cu_seqlens
    path, attention/flash.py:61-91)."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    assert D == 128 and S % 256 == 0, (S, D)
    if doc_start is not None:
        assert B == 1 and doc_start.dtype == torch.int32 and doc_start.numel() == S
    o = torch.empty_like(q)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
    with _prof("attn_fwd", 2.0 * 2 * S * S * Hq * D * 0.5 * B):
        check(get_lib().vh_attn_fwd_bf16(dptr(q), dptr(k), dptr(v), dptr(o),
                                         dptr(lse), B, Hq, Hkv, S, scale,
                                         dptr(doc_start) if doc_start is not None else None,
                                         cur_stream()), "vh_attn_fwd")
    return o, lse


def attn_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
             o: torch.Tensor, lse: torch.Tensor, do: torch.Tensor,
             scale: float, doc_start: torch.Tensor | None = None,
             doc_end: torch.Tensor | None = None):
    """Backward for attn_fwd. Returns (dq bf16 [B,Hq,S,D], dk/dv bf16
    [B,Hkv,S,D] — the GQA head group is folded inside the dkv kernel)."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    rows = B * Hq * S
    do = do.contiguous()
    delta = torch.empty(rows, dtype=torch.float32, device=q.device)
    lse2 = torch.empty(rows, dtype=torch.float32, device=q.device)
    assert (doc_start is None) == (doc_end is None)
    lib = get_lib()
    with _prof("attn_bwd", 3.0 * 2 * 2 * S * S * Hq * D * 0.5 * B):
        check(lib.vh_attn_bwd_pre_bf16(dptr(do), dptr(o), dptr(lse.contiguous()),
                                       dptr(delta), dptr(lse2), rows,
                                       cur_stream()), "vh_attn_bwd_pre")
        dq = torch.empty(B, Hq, S, D, dtype=torch.bfloat16, device=q.device)
        dk = torch.empty(B, Hkv, S, D, dtype=torch.bfloat16, device=q.device)
        dv = torch.empty(B, Hkv, S, D, dtype=torch.bfloat16, device=q.device)
        check(lib.vh_attn_bwd2_bf16(dptr(q), dptr(k), dptr(v), dptr(do),
                                    dptr(delta), dptr(lse2), dptr(dq),
                                    dptr(dk), dptr(dv), B, Hq, Hkv, S, scale,
                                    dptr(doc_start) if doc_start is not None else None,
                                    dptr(doc_end) if doc_end is not None else None,
                                    cur_stream()), "vh_attn_bwd2")
    return dq, dk, dv


def _bhs_strides(t: torch.Tensor):
    """(batch, head, row) element strides of a logical [B,Hq,S,128] view."""
    assert t.dim() == 4 and t.shape[-1] == 128 and t.stride(3) == 1 \
        and t.dtype == torch.bfloat16, (t.shape, t.stride(), t.dtype)
    return t.stride(0), t.stride(1), t.stride(2)


def attn_fwd_token_major(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                         scale: float, doc_start: torch.Tensor | None = None):
    """attn_fwd writing O token-major: returns (o [B,S,Hq,128] contiguous,
    lse [B,Hq,S]). q/k/v as for attn_fwd; the values are attn_fwd's, bit for
    bit."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    assert D == 128 and S % 256 == 0, (S, D)
    if doc_start is not None:
        assert B == 1 and doc_start.dtype == torch.int32 and doc_start.numel() == S
    o = torch.empty(B, S, Hq, D, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
    with _prof("attn_fwd", 2.0 * 2 * S * S * Hq * D * 0.5 * B):
        check(get_lib().vh_attn_fwd_ostrided_bf16(
            dptr(q), dptr(k), dptr(v), dptr(o), dptr(lse), B, Hq, Hkv, S, scale,
            dptr(doc_start) if doc_start is not None else None,
            *_bhs_strides(o.transpose(1, 2)), cur_stream()), "vh_attn_fwd_ostrided")
    return o, lse


def attn_bwd_token_major(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                         o: torch.Tensor, lse: torch.Tensor, do: torch.Tensor,
                         scale: float, doc_start: torch.Tensor | None = None,
                         doc_end: torch.Tensor | None = None):
    """attn_bwd with o and do token-major [B,S,Hq,128] (read in place, no
    head-major copies). Returns head-major (dq, dk, dv), attn_bwd's bits."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    assert o.shape == (B, S, Hq, D) and o.is_contiguous(), (o.shape, o.stride())
    assert do.shape == o.shape
    do = do.contiguous()
    rows = B * Hq * S
    delta = torch.empty(rows, dtype=torch.float32, device=q.device)
    lse2 = torch.empty(rows, dtype=torch.float32, device=q.device)
    assert (doc_start is None) == (doc_end is None)
    strides = _bhs_strides(o.transpose(1, 2))
    lib = get_lib()
    with _prof("attn_bwd", 3.0 * 2 * 2 * S * S * Hq * D * 0.5 * B):
        check(lib.vh_attn_bwd_pre_ostrided_bf16(
            dptr(do), dptr(o), dptr(lse.contiguous()), dptr(delta), dptr(lse2),
            B, Hq, S, *strides, cur_stream()), "vh_attn_bwd_pre_ostrided")
        dq = torch.empty(B, Hq, S, D, dtype=torch.bfloat16, device=q.device)
        dk = torch.empty(B, Hkv, S, D, dtype=torch.bfloat16, device=q.device)
        dv = torch.empty(B, Hkv, S, D, dtype=torch.bfloat16, device=q.device)
        check(lib.vh_attn_bwd2_ostrided_bf16(
            dptr(q), dptr(k), dptr(v), dptr(do), dptr(delta), dptr(lse2),
            dptr(dq), dptr(dk), dptr(dv), B, Hq, Hkv, S, scale,
            dptr(doc_start) if doc_start is not None else None,
            dptr(doc_end) if doc_end is not None else None,
            *strides, cur_stream()), "vh_attn_bwd2_ostrided")
    return dq, dk, dv


def _check_window_sinks(B, Hq, S, D, device, lo, hi, sinks):
    assert D == 128 and S % 256 == 0, (S, D)
    for t in (lo, hi):
        assert t is None or (t.dtype == torch.int32 and t.shape == (S,)
                             and t.is_contiguous() and t.device == device), \
            "window bounds: int32 [S], contiguous, on the inputs' device"
    assert sinks is None or (sinks.dtype == torch.float32
                             and sinks.shape == (Hq,) and sinks.is_contiguous()
                             and sinks.device == device), \
        "sinks: fp32 [Hq], contiguous, on the inputs' device"


def attn_fwd_win_sink(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                      scale: float, lo: torch.Tensor | None = None,
                      sinks: torch.Tensor | None = None,
                      token_major: bool = False):
    """attn_fwd / attn_fwd_token_major with a key window and attention sinks
    (vh_attn_fwd_win_sink_bf16). lo: int32 [S] first visible key per row,
    shared by the batch (ops.kernels.attention.window_bounds); sinks: fp32
    [Hq] logits of the extra softmax column. Returns (o, lse); lse includes
    the sink."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    _check_window_sinks(B, Hq, S, D, q.device, lo, None, sinks)
    if token_major:
        o = torch.empty(B, S, Hq, D, dtype=q.dtype, device=q.device)
        strides = _bhs_strides(o.transpose(1, 2))
    else:
        o = torch.empty_like(q)
        strides = _bhs_strides(o)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
    with _prof("attn_fwd", 2.0 * 2 * S * S * Hq * D * 0.5 * B):
        check(get_lib().vh_attn_fwd_win_sink_bf16(
            dptr(q), dptr(k), dptr(v), dptr(o), dptr(lse), B, Hq, Hkv, S, scale,
            dptr(lo) if lo is not None else None,
            dptr(sinks) if sinks is not None else None,
            *strides, cur_stream()), "vh_attn_fwd_win_sink")
    return o, lse


def attn_bwd_win_sink(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                      o: torch.Tensor, lse: torch.Tensor, do: torch.Tensor,
                      scale: float, lo: torch.Tensor | None = None,
                      hi: torch.Tensor | None = None,
                      sinks: torch.Tensor | None = None,
                      token_major: bool = False):
    """Backward for attn_fwd_win_sink. Returns head-major (dq, dk, dv) and
    dsinks (fp32 [Hq], None without sinks). dsinks is summed in a fixed order
    (no atomics): the same bits from run to run and for both layouts."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    _check_window_sinks(B, Hq, S, D, q.device, lo, hi, sinks)
    assert (lo is None) == (hi is None)
    if token_major:
        assert o.shape == (B, S, Hq, D) and o.is_contiguous(), (o.shape, o.stride())
        strides = _bhs_strides(o.transpose(1, 2))
    else:
        assert o.shape == (B, Hq, S, D) and o.is_contiguous(), (o.shape, o.stride())
        strides = _bhs_strides(o)
    assert do.shape == o.shape
    do = do.contiguous()
    rows = B * Hq * S
    dev = q.device
    delta = torch.empty(rows, dtype=torch.float32, device=dev)
    lse2 = torch.empty(rows, dtype=torch.float32, device=dev)
    dsinks = part = None
    if sinks is not None:
        dsinks = torch.empty(Hq, dtype=torch.float32, device=dev)
        part = torch.empty(B * Hq * (S // 256), dtype=torch.float32, device=dev)
    lib = get_lib()
    with _prof("attn_bwd", 3.0 * 2 * 2 * S * S * Hq * D * 0.5 * B):
        check(lib.vh_attn_bwd_pre_sink_bf16(
            dptr(do), dptr(o), dptr(lse.contiguous()),
            dptr(sinks) if sinks is not None else None,
            dptr(delta), dptr(lse2),
            dptr(dsinks) if dsinks is not None else None,
            dptr(part) if part is not None else None,
            B, Hq, S, *strides, cur_stream()), "vh_attn_bwd_pre_sink")
        dq = torch.empty(B, Hq, S, D, dtype=torch.bfloat16, device=dev)
        dk = torch.empty(B, Hkv, S, D, dtype=torch.bfloat16, device=dev)
        dv = torch.empty(B, Hkv, S, D, dtype=torch.bfloat16, device=dev)
        check(lib.vh_attn_bwd2_win_bf16(
            dptr(q), dptr(k), dptr(v), dptr(do), dptr(delta), dptr(lse2),
            dptr(dq), dptr(dk), dptr(dv), B, Hq, Hkv, S, scale,
            dptr(lo) if lo is not None else None,
            dptr(hi) if hi is not None else None,
            *strides, cur_stream()), "vh_attn_bwd2_win")
    return dq, dk, dv, dsinks


# ---------------------------------------------------- load-balancing loss
# vh_lbl_fwd geometry: 1024-thread blocks, a sub-group of G lanes per row
# (G = pow2 >= ceil(E/8)), so one block pass covers 1024/G rows. At most
# LBL_MAX_BLOCKS blocks per layer (one per CU) grid-stride over the rows; the
# cap also bounds the partial rows the finish pass has to read.
LBL_FWD_THREADS = 1024
LBL_MAX_BLOCKS = 256
_LBL_DTYPES = {torch.bfloat16: 0, torch.float32: 1}


def lbl_rows_per_block(num_experts: int) -> int:
    groups, g = (num_experts + 7) // 8, 1
    while g < groups:
        g *= 2
    return max(LBL_FWD_THREADS // g, 1)


def lbl_num_blocks(rows: int, num_experts: int) -> int:
    rpb = lbl_rows_per_block(num_experts)
    return min((rows + rpb - 1) // rpb, LBL_MAX_BLOCKS)


def _lbl_dtype(t: torch.Tensor) -> int:
    if t.dtype not in _LBL_DTYPES:
        raise TypeError(f"load_balancing_loss: logits dtype {t.dtype} "
                        "(bf16 and fp32 are supported)")
    return _LBL_DTYPES[t.dtype]


def lbl_fwd(layers, top_k: int, mask_w: torch.Tensor | None,
            total_w: torch.Tensor | None = None):
    """Aux-loss forward over per-layer router logits [T_l, E] (contiguous,
    one dtype, one device). mask_w: fp32 [T] per-row weights shared by every
    layer, or None. total_w: device fp32 [1] normaliser (default: the summed
    row weights). Returns (loss 0-dim, count [E], prob_sum [E], coef [1]),
    all fp32. One vh_lbl_fwd per non-empty layer into its slice of a shared
    partial buffer, then one vh_lbl_finish; the layers are never
    concatenated."""
    layers = [l for l in layers if l.shape[0] > 0]  # 0-row layers are skipped
    assert layers, "lbl_fwd needs at least one non-empty layer"
    dev = layers[0].device
    E = layers[0].shape[1]
    blocks = [lbl_num_blocks(l.shape[0], E) for l in layers]
    p_total = sum(blocks)
    partial = torch.empty(p_total, 2, E, dtype=torch.float32, device=dev)
    count = torch.empty(E, dtype=torch.float32, device=dev)
    prob_sum = torch.empty(E, dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    if total_w is None:
        if mask_w is not None:
            total_w = (mask_w.sum() * len(layers)).reshape(1)
        else:
            total_w = torch.full((1,), float(sum(l.shape[0] for l in layers)),
                                 dtype=torch.float32, device=dev)
    lib = get_lib()
    stream = cur_stream()
    nbytes = sum(l.numel() * l.element_size() for l in layers)
    with _prof("lbl_fwd", float(nbytes)):
        row0 = 0
        for l, P in zip(layers, blocks):
            T = l.shape[0]
            assert l.is_contiguous() and l.shape[1] == E
            if mask_w is not None:
                assert mask_w.numel() == T, (mask_w.numel(), T)
            check(lib.vh_lbl_fwd(dptr(l), _lbl_dtype(l),
                                 dptr(mask_w) if mask_w is not None else None,
                                 T, E, top_k, dptr(partial[row0]), P, stream),
                  "vh_lbl_fwd")
            row0 += P
        check(lib.vh_lbl_finish(dptr(partial), p_total, E, dptr(total_w),
                                dptr(count), dptr(prob_sum), dptr(out), stream),
              "vh_lbl_finish")
    return out[0], count, prob_sum, out[1:2]


def lbl_bwd(layer: torch.Tensor, mask_w: torch.Tensor | None,
            count: torch.Tensor, coef: torch.Tensor,
            grad_out: torch.Tensor) -> torch.Tensor:
    """Gradient of the aux loss w.r.t. one layer's logits (same dtype).
    coef / grad_out are device fp32 scalars (no host sync)."""
    grad = torch.empty_like(layer)
    T, E = layer.shape
    if T == 0:
        return grad
    assert layer.is_contiguous() and grad.is_contiguous()
    with _prof("lbl_bwd", 2.0 * layer.numel() * layer.element_size()):
        check(get_lib().vh_lbl_bwd(dptr(layer), _lbl_dtype(layer),
                                   dptr(mask_w) if mask_w is not None else None,
                                   dptr(count), dptr(coef), dptr(grad_out),
                                   dptr(grad), T, E, cur_stream()),
              "vh_lbl_bwd")
    return grad
