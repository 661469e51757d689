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


def check_sliding_window(sliding_window):
    """None, or an int > 0 (returned as int); else ValueError."""
    if sliding_window is None:
        return None
    if isinstance(sliding_window, bool) or not isinstance(sliding_window, int) \
            or sliding_window <= 0:
        raise ValueError(
            f"sliding_window must be an int > 0 or None, got {sliding_window!r}")
    return int(sliding_window)


# (S, W, id(doc_start), id(doc_end), device) -> (doc_start, doc_end, lo, hi).
# The model hands every layer of a forward (and its recompute) the same
# doc_start / doc_end tensors, so the bounds are built once per forward; the
# entry holds on to the two tensors, which keeps their ids from being reused.
_WINDOW_BOUNDS_CACHE: dict = {}
_WINDOW_BOUNDS_CACHE_MAX = 8


def window_bounds(S, W, doc_start=None, doc_end=None, device=None):
    """Key-window bounds for the HIP flash pair (int32 [S] each): row q sees
    keys lo[q] .. q, key j is seen by rows j .. hi[j]-1. Window semantics are
    the reference's and HF's: key j is visible to query i iff j <= i and
    j > i - W, inside i's document. With documents, lo = max(doc_start,
    q-W+1) and hi = min(doc_end, j+W); both stay monotone non-decreasing,
    which is what the kernels' tile skipping assumes. W = None returns the
    document bounds as they are; W >= S without documents returns (None,
    None), plain causal (HF applies the window only when key_length >
    sliding_window). Built with torch ops on `device`, no host sync."""
    W = check_sliding_window(W)
    assert (doc_start is None) == (doc_end is None)
    if W is None:
        return doc_start, doc_end
    if doc_start is None and W >= S:
        return None, None
    if device is None:
        device = doc_start.device if doc_start is not None else "cpu"
    device = torch.device(device)
    key = (S, W, id(doc_start), id(doc_end), device)
    hit = _WINDOW_BOUNDS_CACHE.get(key)
    if hit is not None and hit[0] is doc_start and hit[1] is doc_end:
        return hit[2], hit[3]
    ar = torch.arange(S, dtype=torch.int32, device=device)
    lo = (ar - (W - 1)).clamp_(min=0)
    hi = (ar + W).clamp_(max=S)
    if doc_start is not None:
        assert doc_start.numel() == S and doc_end.numel() == S, \
            (doc_start.numel(), doc_end.numel(), S)
        lo = torch.maximum(lo, doc_start.to(device=device, dtype=torch.int32).flatten())
        hi = torch.minimum(hi, doc_end.to(device=device, dtype=torch.int32).flatten())
    lo, hi = lo.contiguous(), hi.contiguous()
    if len(_WINDOW_BOUNDS_CACHE) >= _WINDOW_BOUNDS_CACHE_MAX:
        _WINDOW_BOUNDS_CACHE.pop(next(iter(_WINDOW_BOUNDS_CACHE)))
    _WINDOW_BOUNDS_CACHE[key] = (doc_start, doc_end, lo, hi)
    return lo, hi


def slice_ulysses_sinks(s_aux, *, query_head_count, local_query_head_count,
                        group):
    """This Ulysses rank's head slice of a global 1-D [num_heads] auxiliary
    (ref attention/ulysses.py:68-80 slice_ulysses_head_auxiliary)."""
    if s_aux is None or s_aux.ndim != 1 or s_aux.numel() != query_head_count:
        return s_aux
    head_start = dist.get_rank(group) * local_query_head_count
    return s_aux.narrow(0, head_start, local_query_head_count).contiguous()


def eager_window_sink_attention(q, k, v, scaling, lo=None, sinks=None,
                                dropout=0.0, training=False):
    """Explicit-mask attention with an optional sink column on [B,h,S,D]; the
    torch twin of the reference's gpt-oss eager_attention_forward
    (patched_modeling_gpt_oss_gpu.py:281-309): additive mask, sink logit
    sinks[h] appended as one more column (not scaled), max-subtracted softmax
    over the S+1 columns, sink column dropped before P·V. lo (int [S], None =
    plain causal) is the first visible key of every row (window_bounds).
    Returns [B,h,S,D]."""
    n_rep = q.shape[1] // k.shape[1]
    k = _repeat_kv(k, n_rep)
    v = _repeat_kv(v, n_rep)
    S = q.shape[2]
    w = torch.matmul(q, k.transpose(2, 3)) * scaling
    ar = torch.arange(S, device=q.device)
    allowed = ar[None, :] <= ar[:, None]
    if lo is not None:
        assert lo.numel() == S, (lo.numel(), S)
        allowed = allowed & (ar[None, :] >= lo.to(device=q.device, dtype=torch.long)[:, None])
    mask = torch.zeros(S, S, dtype=w.dtype, device=q.device).masked_fill(
        ~allowed, torch.finfo(w.dtype).min)
    w = w + mask
    if sinks is not None:
        assert sinks.ndim == 1 and sinks.numel() == q.shape[1], \
            (tuple(sinks.shape), q.shape[1])
        sk = sinks.to(w.dtype).reshape(1, -1, 1, 1).expand(q.shape[0], -1, S, -1)
        w = torch.cat([w, sk], dim=-1)
        w = w - w.max(dim=-1, keepdim=True).values
        p = F.softmax(w, dim=-1, dtype=w.dtype)[..., :-1]
    else:
        p = F.softmax(w, dim=-1, dtype=w.dtype)
    p = F.dropout(p, p=dropout, training=training).to(v.dtype)
    return torch.matmul(p, v)


class _HipFlashAttention(torch.autograd.Function):
    """In-repo CDNA4 flash kernel pair (vh_attn_fwd_bf16 / vh_attn_bwd2_bf16;
    csrc/vh_attention.hip). Causal, GQA, D=128, S % 256 == 0, bf16; optional
    packed-varlen block-diagonal masking via per-token document bounds
    (the reference's flash-attn cu_seqlens path, attention/flash.py:61-91).
    sinks (fp32 [Hq], differentiable) and shared_bounds (doc_start / doc_end
    are key-window bounds shared by the batch, B > 1 allowed) go through the
    vh_attn_*_win_sink entry points; without either the calls are the ones
    above, unchanged.

    Parity-tested against torch autograd (tests/test_gpu_kernels.py). The
    attention slot dispatches this pair by default since round 2 (the GQA-
    folded dkv kernel closed the backward gap to AOTriton); core="sdpa"
    keeps the torch CK/AOTriton comparison path.
    """

    @staticmethod
    def forward(ctx, q, k, v, scale, doc_start, doc_end, token_major=False,
                sinks=None, shared_bounds=False):
        from .. import hip_lib
        ctx.win_sink = sinks is not None or shared_bounds
        if ctx.win_sink:
            assert (doc_start is None) == (doc_end is None)
            sk = sinks.detach().contiguous() if sinks is not None else None
            # the backward reads q / k / v through raw pointers: save what
            # the forward read, not the caller's (possibly transposed) views
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
            o, lse = hip_lib.attn_fwd_win_sink(q, k, v, scale, doc_start, sk,
                                               token_major)
            ctx.save_for_backward(q, k, v, o, lse, sk)
            ctx.scale = scale
            ctx.docs = (doc_start, doc_end)
            ctx.token_major = token_major
            return o
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
        if ctx.win_sink:
            q, k, v, o, lse, sk = ctx.saved_tensors
            dq, dk, dv, dsinks = hip_lib.attn_bwd_win_sink(
                q, k, v, o, lse, do, ctx.scale, *ctx.docs, sk, ctx.token_major)
            return dq, dk, dv, None, None, None, None, dsinks, None
        q, k, v, o, lse = ctx.saved_tensors
        bwd = hip_lib.attn_bwd_token_major if ctx.token_major else hip_lib.attn_bwd
        dq, dk, dv = bwd(q, k, v, o, lse, do, ctx.scale, *ctx.docs)
        return dq, dk, dv, None, None, None, None, None, None


def hip_flash_attention(q, k, v, scale, doc_start=None, doc_end=None,
                        token_major=False, sinks=None, sliding_window=None,
                        shared_bounds=False):
    """[B, h, S, D] bf16 causal attention through the in-repo HIP kernels;
    the output is [B, h, S, D], or [B, S, h, D] with token_major.
    doc_start / doc_end: packed-varlen document bounds (B == 1).
    sliding_window: causal window of W keys (window_bounds), inside the
    documents if there are any; B > 1 is fine without documents.
    sinks: [h] attention-sink logits, differentiable.
    shared_bounds: doc_start / doc_end already are window bounds shared by
    the batch (what sliding_window builds)."""
    S = q.shape[2]
    if doc_start is not None and not shared_bounds:
        assert q.shape[0] == 1, "packed varlen requires B == 1"
    if check_sliding_window(sliding_window) is not None:
        lo, hi = window_bounds(S, sliding_window, doc_start, doc_end, q.device)
        if lo is not None:
            doc_start, doc_end, shared_bounds = lo, hi, True
    if sinks is not None:
        sinks = sinks.float()
    if sinks is None and not shared_bounds:
        return _HipFlashAttention.apply(q, k, v, scale, doc_start, doc_end,
                                        token_major)
    return _HipFlashAttention.apply(q, k, v, scale, doc_start, doc_end,
                                    token_major, sinks, shared_bounds)


def hip_attention_forward(module, query, key, value, attention_mask,
                          dropout=0.0, scaling=None, sliding_window=None,
                          softcap=None, skip_ulysses=False,
                          token_major_out=False, **kwargs):
    """Slot signature parity: flash.py:153-165. Inputs [B, h, S, D]
    (pre-transpose, HF convention); returns ([B, S_local, h, D] reshaped by
    the caller, None)."""
    if softcap not in (None, 0):
        raise NotImplementedError(
            f"softcap={softcap!r}: logit soft-capping is not implemented in "
            "either attention core")
    sliding_window = check_sliding_window(sliding_window)
    s_aux = kwargs.get("s_aux")
    ps = get_parallel_state()
    ulysses = ps.ulysses_enabled and not skip_ulysses
    q_heads = query.shape[1]
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
    if ulysses:
        # after the all-to-all this rank holds q_heads / sp of the heads
        # (ref flash.py:249-255)
        s_aux = slice_ulysses_sinks(
            s_aux, query_head_count=q_heads,
            local_query_head_count=q.shape[1], group=ps.ulysses_group)
    if s_aux is not None and (s_aux.ndim != 1 or s_aux.numel() != q.shape[1]):
        raise ValueError(
            f"s_aux must be 1-D [num_heads={q.shape[1]}], got {tuple(s_aux.shape)}")
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
                                  token_major=token_major_out, sinks=s_aux,
                                  sliding_window=sliding_window)
    elif sliding_window is not None or s_aux is not None:
        # explicit window / document mask plus the sink column. This is the
        # core that D != 128, S % 256 != 0 and fp32 take, gpt-oss's
        # head_dim = 64 included.
        if scaling is None:
            scaling = q.shape[-1] ** -0.5
        lo, _ = window_bounds(q.shape[2], sliding_window, doc_start, doc_end,
                              q.device)
        out = eager_window_sink_attention(
            q, k, v, scaling, lo, s_aux, dropout=dropout,
            training=getattr(module, "training", False))
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
