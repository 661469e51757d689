"""Attention with Ulysses SP (impl name "hip").

Parity target: flash_attention_forward + prepare/restore Ulysses exchange
(ops/kernels/attention/flash.py:153-301, attention/ulysses.py:27-91):
seq-sharded/full-heads -> (a2a) -> full-seq/head-sharded -> kernel ->
(a2a back); GQA KV head repeat when sp > kv heads.

Core kernel (round 2+): the in-repo CDNA4 flash pair (vh_attn_fwd_bf16 /
vh_attn_bwd2_bf16) including the packed-varlen cu_seqlens path; torch SDPA
(CK/AOTriton) remains as the A/B comparison core. The Ulysses layout
exchanges are the §8a items and are implemented here.
"""

from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn.functional as F

from ...distributed.parallel_state import get_parallel_state
from ...distributed.sequence_parallel import (
    gather_heads_scatter_seq,
    gather_seq_scatter_heads,
)
from ..kernel_registry import KERNEL_REGISTRY, HardwareRequirement, KernelSpec

# core attention engine for the "hip" slot: "hip_flash" (the in-repo CDNA4
# kernel pair — the default since round 2) or "sdpa" (torch's CK/AOTriton
# flash, kept as the A/B comparison core). Overridable per call via core= or
# VEOMNI_ATTN_CORE.
import os
_DEFAULT_CORE = os.environ.get("VEOMNI_ATTN_CORE", "hip_flash")


def docs_from_cu_seqlens(cu: torch.Tensor, seq_len: int):
    """Per-token document bounds from cu_seqlens (the reference's varlen
    contract, attention/flash.py:61-91 + data_collator.py:50): doc_start[t] =
    cu[i], doc_end[t] = cu[i+1] for t in document i. Returns (None, None)
    when the batch is a single document (plain causal covers it)."""
    cu = cu.to(torch.int32).flatten()
    if cu.numel() <= 2:
        return None, None
    assert int(cu[-1]) == seq_len, (
        f"cu_seqlens must cover the padded sequence (tail-coalesced): "
        f"cu[-1]={int(cu[-1])} != S={seq_len}")
    lens = (cu[1:] - cu[:-1]).to(torch.long)
    doc_start = torch.repeat_interleave(cu[:-1], lens)
    doc_end = torch.repeat_interleave(cu[1:], lens)
    return doc_start.contiguous(), doc_end.contiguous()


def prepare_ulysses_qkv(query, key, value, *, group, ulysses_size):
    """[B, S/sp, h, D] -> [B, S, h/sp, D] for q/k/v (ref attention/ulysses.py:27-65)."""
    q_heads = query.shape[2]
    kv_heads = key.shape[2]
    assert q_heads % ulysses_size == 0
    if ulysses_size > kv_heads:
        assert ulysses_size % kv_heads == 0
        rep = ulysses_size // kv_heads
        key = torch.repeat_interleave(key, dim=2, repeats=rep)
        value = torch.repeat_interleave(value, dim=2, repeats=rep)
    else:
        assert kv_heads % ulysses_size == 0
    if query.ndim == 4 and query.size(0) == 1:
        q, k, v = query.squeeze(0), key.squeeze(0), value.squeeze(0)
        q = gather_seq_scatter_heads(q, seq_dim=0, head_dim=1, group=group)
        k = gather_seq_scatter_heads(k, seq_dim=0, head_dim=1, group=group)
        v = gather_seq_scatter_heads(v, seq_dim=0, head_dim=1, group=group)
        return q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), q_heads
    q = gather_seq_scatter_heads(query, seq_dim=1, head_dim=2, group=group)
    k = gather_seq_scatter_heads(key, seq_dim=1, head_dim=2, group=group)
    v = gather_seq_scatter_heads(value, seq_dim=1, head_dim=2, group=group)
    return q, k, v, q_heads


def restore_ulysses_output(output, *, group):
    """[B, S, h/sp, D] -> [B, S/sp, h, D] (ref attention/ulysses.py:83-91)."""
    if output.ndim == 4 and output.size(0) == 1:
        out = output.squeeze(0)
        out = gather_heads_scatter_seq(out, seq_dim=0, head_dim=1, group=group)
        return out.unsqueeze(0)
    return gather_heads_scatter_seq(output, seq_dim=1, head_dim=2, group=group)


def _repeat_kv(x, n_rep):
    b, h, s, d = x.shape
    if n_rep == 1:
        return x
    return x[:, :, None, :, :].expand(b, h, n_rep, s, d).reshape(b, h * n_rep, s, d)


class _HipFlashAttention(torch.autograd.Function):
    """In-repo CDNA4 flash kernel pair (vh_attn_fwd_bf16 / vh_attn_bwd2_bf16;
    csrc/vh_attention.hip). Causal, GQA, D=128, S % 256 == 0, bf16; optional
    packed-varlen block-diagonal masking via per-token document bounds
    (the reference's flash-attn cu_seqlens path, attention/flash.py:61-91).

    Parity-tested against torch autograd (tests/test_gpu_kernels.py). The
    attention slot dispatches this pair by default since round 2 (the GQA-
    folded dkv kernel closed the backward gap to AOTriton); core="sdpa"
    keeps the torch CK/AOTriton comparison path.
    """

    @staticmethod
    def forward(ctx, q, k, v, scale, doc_start, doc_end, token_major=False):
        from .. import hip_lib
        # token_major: O is written, saved and differentiated as [B,S,h,D]
        # (vh_attn_*_ostrided); same values, no layout copies around the call
        fwd = hip_lib.attn_fwd_token_major if token_major else hip_lib.attn_fwd
        o, lse = fwd(q.contiguous(), k.contiguous(), v.contiguous(), scale,
                     doc_start)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        ctx.docs = (doc_start, doc_end)
        ctx.token_major = token_major
        return o

    @staticmethod
    def backward(ctx, do):
        from .. import hip_lib
        q, k, v, o, lse = ctx.saved_tensors
        bwd = hip_lib.attn_bwd_token_major if ctx.token_major else hip_lib.attn_bwd
        dq, dk, dv = bwd(q, k, v, o, lse, do, ctx.scale, *ctx.docs)
        return dq, dk, dv, None, None, None, None


def hip_flash_attention(q, k, v, scale, doc_start=None, doc_end=None,
                        token_major=False):
    """[B, h, S, D] bf16 causal attention through the in-repo HIP kernels;
    the output is [B, h, S, D], or [B, S, h, D] with token_major."""
    return _HipFlashAttention.apply(q, k, v, scale, doc_start, doc_end,
                                    token_major)


def hip_attention_forward(module, query, key, value, attention_mask,
                          dropout=0.0, scaling=None, sliding_window=None,
                          softcap=None, skip_ulysses=False,
                          token_major_out=False, **kwargs):
    """Slot signature parity: flash.py:153-165. Inputs [B, h, S, D]
    (pre-transpose, HF convention); returns ([B, S_local, h, D] reshaped by
    the caller, None)."""
    ps = get_parallel_state()
    ulysses = ps.ulysses_enabled and not skip_ulysses
    # FA kernels take [B, S, h, D]
    query = query.transpose(1, 2)
    key = key.transpose(1, 2)
    value = value.transpose(1, 2)
    if ulysses:
        group = ps.ulysses_group
        query, key, value, _ = prepare_ulysses_qkv(
            query, key, value, group=group, ulysses_size=ps.ulysses_size
        )
    # core attention (in-repo HIP flash pair; "sdpa" = torch CK/AOTriton A/B)
    q = query.transpose(1, 2)
    k = key.transpose(1, 2)
    v = value.transpose(1, 2)
    # packed-varlen document bounds: precomputed doc_start/doc_end kwargs, or
    # derived from the collator's cu_seq_lens (ref data_collator.py:50).
    doc_start = kwargs.get("doc_start")
    doc_end = kwargs.get("doc_end")
    if doc_start is None and kwargs.get("cu_seq_lens_q") is not None:
        doc_start, doc_end = docs_from_cu_seqlens(kwargs["cu_seq_lens_q"],
                                                  q.shape[2])
    core = kwargs.get("core", _DEFAULT_CORE)
    if core == "hip_flash" and (q.shape[-1] != 128 or q.shape[2] % 256 != 0
                                or q.dtype != torch.bfloat16):
        # the in-repo pair covers the BASELINE shapes (D=128, S%256, bf16);
        # toy/unit shapes take the torch core (a dispatch policy, not a
        # missing-extension fallback)
        core = "sdpa"
    if core == "hip_flash":
        if scaling is None:
            scaling = q.shape[-1] ** -0.5
        out = hip_flash_attention(q, k, v, scaling, doc_start, doc_end,
                                  token_major=token_major_out)
    else:
        n_rep = q.shape[1] // k.shape[1]
        k = _repeat_kv(k, n_rep)
        v = _repeat_kv(v, n_rep)
        if doc_start is not None:
            # explicit block-diagonal causal mask — never silently
            # cross-attend on packed batches
            S = q.shape[2]
            assert doc_start.numel() == S, (doc_start.numel(), S)
            ar = torch.arange(S, device=q.device)
            ds = doc_start.to(device=q.device, dtype=torch.long)
            allowed = (ar[None, :] <= ar[:, None]) & (ar[None, :] >= ds[:, None])
            out = F.scaled_dot_product_attention(q, k, v, attn_mask=allowed,
                                                 dropout_p=dropout,
                                                 scale=scaling, is_causal=False)
        else:
            out = F.scaled_dot_product_attention(q, k, v, attn_mask=None,
                                                 dropout_p=dropout,
                                                 scale=scaling, is_causal=True)
    if token_major_out:
        # the caller (Attention.forward) asks for this only where the
        # hip_flash core runs without Ulysses: out is [B, S, h, D] already
        assert core == "hip_flash" and not ulysses
    else:
        out = out.transpose(1, 2)  # [B, S, h, D]
    if ulysses:
        out = restore_ulysses_output(out, group=ps.ulysses_group)
    return out, None


KERNEL_REGISTRY.register(
    KernelSpec(
        name="hip", op_name="attention", variant="sdpa_with_sp",
        factory=lambda: hip_attention_forward,
        hardware=HardwareRequirement(device_type="gpu"),
        description="Ulysses SP exchange + in-repo CDNA4 flash pair incl. varlen (VEOMNI_ATTN_CORE=sdpa selects the torch CK/AOTriton A/B core)",
    )
)

KERNEL_REGISTRY.register(
    KernelSpec(
        name="hip_flash", op_name="attention", variant="hip_flash_pair",
        factory=lambda: (lambda *a, **kw: hip_attention_forward(*a, core="hip_flash", **kw)),
        hardware=HardwareRequirement(device_type="gpu"),
        description="Ulysses SP exchange + in-repo CDNA4 flash fwd/bwd kernels",
    )
)

# the reference exposes the same callable under this name in HF's
# ALL_ATTENTION_FUNCTIONS; keep the alias for drop-in callers.
veomni_flash_attention_2_with_sp = hip_attention_forward
