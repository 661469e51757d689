"""q/k norms on the fused qkv projection without slice copies (HIP path).

The fused qkv projection leaves [B, S, hq + 2*hkv, 128]. Through the rms_norm
slot each of the q and k norms first copies its slice contiguous (and saves
the copy), its backward copies dy contiguous, and autograd's slice-backward
zero-fills one qkv-sized buffer per slice, copies the slice gradient in and
adds the buffers. `hip_qk_norm` is one autograd node for both norms instead:

  forward   vh_rmsnorm128_fwd_strided reads each slice of qkv in place and
            writes the contiguous [B, S, h, 128] tensor the slot returned.
  backward  vh_rmsnorm128_bwd_strided reads dy in whatever layout it arrives
            (RoPE's backward hands it transposed) and x from the saved qkv,
            and writes dx straight into the q / k slices of one qkv
            gradient whose v slice is zeroed (v keeps autograd's own slice
            path, so its gradient is still added in).

Outputs, saved statistics and gradients are the slot path's bit for bit (the
norm weight gradient up to the unordered atomic combine in k_dw_reduce, as
between two runs of the slot path): the kernels differ from the contiguous
ones in addressing only, and everything downstream receives tensors of the
same values, shapes and strides. `fused_path_applies` is the dispatch rule;
Attention.qkv_layout = "slots" forces the per-op path for A/B runs.
"""

from __future__ import annotations

import torch

from .. import hip_lib
from . import attention as _attention
from . import norms as _norms


class HipQkNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, wq, wk, nh, nkv, eps_q, eps_k):
        # qkv: [B, S, nh + 2*nkv, 128] (a view of the projection output)
        assert qkv.dtype == torch.bfloat16 and qkv.shape[-1] == 128
        assert qkv.shape[2] == nh + 2 * nkv, (qkv.shape, nh, nkv)
        B, S, _, D = qkv.shape
        yq = torch.empty(B, S, nh, D, dtype=qkv.dtype, device=qkv.device)
        yk = torch.empty(B, S, nkv, D, dtype=qkv.dtype, device=qkv.device)
        _, rstd_q = hip_lib.rmsnorm128_fwd_strided(qkv[:, :, :nh], wq, eps_q, yq)
        _, rstd_k = hip_lib.rmsnorm128_fwd_strided(qkv[:, :, nh:nh + nkv], wk,
                                                   eps_k, yk)
        ctx.save_for_backward(qkv, wq, wk, rstd_q, rstd_k)
        ctx.heads = (nh, nkv)
        return yq, yk

    @staticmethod
    def backward(ctx, dyq, dyk):
        qkv, wq, wk, rstd_q, rstd_k = ctx.saved_tensors
        nh, nkv = ctx.heads
        if dyq.stride(3) != 1:
            dyq = dyq.contiguous()
        if dyk.stride(3) != 1:
            dyk = dyk.contiguous()
        dqkv = torch.empty_like(qkv)
        dqkv[:, :, nh + nkv:].zero_()   # v's gradient is added by autograd
        dwq = hip_lib.rmsnorm128_bwd_strided(
            dyq, qkv[:, :, :nh], wq, rstd_q, dqkv[:, :, :nh])
        dwk = hip_lib.rmsnorm128_bwd_strided(
            dyk, qkv[:, :, nh:nh + nkv], wk, rstd_k, dqkv[:, :, nh:nh + nkv])
        return dqkv, dwq.to(wq.dtype), dwk.to(wk.dtype), None, None, None, None


def hip_qk_norm(qkv, q_norm_weight, k_norm_weight, num_heads, num_kv_heads,
                eps_q, eps_k):
    """[B,S,nh+2*nkv,128] projection output -> normed (q [B,S,nh,128],
    k [B,S,nkv,128]), both contiguous."""
    return HipQkNorm.apply(qkv, q_norm_weight, k_norm_weight, num_heads,
                           num_kv_heads, eps_q, eps_k)


def fused_path_applies(rms_slot, rope_slot, attn_slot, *, qk_norm, dtype,
                       head_dim, seq_len, ulysses, attn_kwargs) -> bool:
    """True when the per-op path would run hip RMSNorm, hip RoPE and the
    hip_flash core on these shapes, so hip_qk_norm and the token-major
    attention output compute the same thing. Everything else keeps the
    per-op path."""
    if not qk_norm or ulysses:
        return False
    if dtype != torch.bfloat16 or head_dim != 128 or seq_len % 256 != 0:
        return False
    if rms_slot.bound_kernel() is not _norms.hip_rms_norm:
        return False
    if rope_slot.bound_kernel() is not _norms.hip_rotary_pos_emb:
        return False
    if attn_slot.bound_kernel() is not _attention.hip_attention_forward:
        return False
    return attn_kwargs.get("core", _attention._DEFAULT_CORE) == "hip_flash"
