"""HIP fused-MoE kernels: grouped-GEMM expert MLP, non-EP and EP variants.

Parity targets:
  - math order of the reference's merged-fc1 fused path (routing weights
    applied BEFORE fc2): ops/kernels/moe/group_gemm.py:320-520
    (MergedFc1TritonFusedMoeExpertFunction) and the EP merged variant
    distributed/moe/moe_layer.py:414-567 (EPMergedFc1GroupGemm);
  - module pointer + patch entry: ops/kernels/moe/__init__.py:27-118
    (`_fused_moe_forward`, `fused_moe_forward`, `apply_veomni_fused_moe_patch`);
  - OpSlot adapter contract: ops/kernels/moe/__init__.py:126-161;
  - scatter-index helper kept plain torch ON PURPOSE, like the reference
    (_scatter.py:30-33: "plain-torch helper on purpose").

Device work: vh_expert_histogram / vh_moe_scatter / vh_group_gemm_nk /
vh_moe_silu_mul_weighted / vh_group_gemm_mn / vh_moe_gather (C ABI).

Clamped SwiGLU (`swiglu_limit`; ref group_gemm.py:24-42, :357-363, :477-480):
every expert path takes an optional limit and hands it to the epilogue pair,
which then runs vh_moe_silu_mul_clamp_weighted(_bwd). The saved tensor is
still the RAW fc1 — clamp and gradient mask are recomputed in the backward
kernel, nothing extra is saved. With limit None every path issues exactly the
calls it issued before the limit existed.

gpt-oss experts (OpSlot moe_experts/gpt_oss; ref GptOssExperts and its fused
gpt-oss expert function): a second provider further down, for the module
with interleaved gate/up, per-expert biases and the routing weight after
down_proj. Same grouped GEMMs on the stored [E,H,2I] / [E,I,H] layouts, with
vh_moe_gptoss_glu(_bwd) / vh_moe_expert_bias_scale(_bwd) /
vh_moe_segment_colsum around them.
"""

from __future__ import annotations

import functools
import math

import torch

from ...distributed.moe import dispatch_to_ep_class
from ...distributed.parallel_state import get_parallel_state
from .. import hip_lib
from ..kernel_registry import KERNEL_REGISTRY, HardwareRequirement, KernelSpec

_fused_moe_forward = None


def compute_expert_scatter_index(expert_index: torch.Tensor):
    """One stable sort + O(N) inverse permutation (ref _scatter.py:40-79)."""
    flat = expert_index.flatten()
    sorted_order = flat.argsort(stable=True)
    inv = torch.empty_like(sorted_order)
    inv[sorted_order] = torch.arange(sorted_order.numel(), dtype=sorted_order.dtype,
                                     device=sorted_order.device)
    return sorted_order, inv.to(torch.int32).view(expert_index.shape)


class HipFusedMoeFunction(torch.autograd.Function):
    """Non-EP merged-fc1 fused MoE (parity: MergedFc1TritonFusedMoeExpertFunction)."""

    @staticmethod
    def forward(ctx, num_experts, gate_weights, expert_index, hidden_states,
                fc1_1_2_weight, fc2_weight, swiglu_limit=None):
        T, H = hidden_states.shape
        splits = hip_lib.expert_histogram(expert_index, num_experts)
        _, scatter_index = compute_expert_scatter_index(expert_index)
        scatter_output = hip_lib.moe_scatter(hidden_states, scatter_index)
        cumsum_t = torch.cumsum(splits, dim=0)

        fc1 = hip_lib.group_gemm_nk(scatter_output, fc1_1_2_weight, cumsum_t, trans_b=True)

        w = gate_weights.reshape(-1)
        scattered_w = torch.empty_like(w)
        scattered_w[scatter_index.flatten().to(torch.int64)] = w
        weighted = hip_lib.silu_mul_weighted(fc1, scattered_w, swiglu_limit)

        fc2 = hip_lib.group_gemm_nk(weighted, fc2_weight, cumsum_t, trans_b=True)
        out = hip_lib.moe_gather(fc2, scatter_index)

        ctx.num_experts = num_experts
        ctx.swiglu_limit = swiglu_limit
        ctx.save_for_backward(gate_weights, fc1_1_2_weight, fc2_weight,
                              scatter_index, scatter_output, cumsum_t, fc1,
                              scattered_w, weighted)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        (gate_weights, fc1_1_2_weight, fc2_weight, scatter_index,
         scatter_output, cumsum_t, fc1, scattered_w, weighted) = ctx.saved_tensors
        G = fc2_weight.shape[0]
        grad_output = grad_output.view(-1, grad_output.shape[-1]).contiguous()

        grad_fc2_out = hip_lib.moe_scatter(grad_output, scatter_index)
        # dgrad through fc2 straight from the stored [G, H, I] weights: the
        # !trans_b nk256s kernel stages W[g] as it lies and transposes in the
        # LDS read (no transposed copy; profiles/gg_direct_operands_ab.md)
        d_weighted = hip_lib.group_gemm_nk(
            grad_fc2_out, fc2_weight, cumsum_t, trans_b=False)
        # wgrad fc2: [G, H, I]
        d_fc2_w = hip_lib.group_gemm_mn(grad_fc2_out, weighted, cumsum_t, G)

        # fused epilogue backward (silu — and, with a limit, clamp + mask —
        # recomputed from the saved raw pre-activation)
        d_fc1, dw_rows = hip_lib.silu_mul_weighted_bwd(d_weighted, fc1, scattered_w,
                                                       ctx.swiglu_limit)
        grad_gate = dw_rows[scatter_index.flatten().to(torch.int64)]
        grad_gate = grad_gate.reshape(gate_weights.shape).to(gate_weights.dtype)

        # dgrad + wgrad through merged fc1 (stored weights, as above)
        d_scatter = hip_lib.group_gemm_nk(
            d_fc1, fc1_1_2_weight, cumsum_t, trans_b=False)
        d_fc1_w = hip_lib.group_gemm_mn(d_fc1, scatter_output, cumsum_t, G)

        grad_hidden = hip_lib.moe_gather(d_scatter, scatter_index)
        return None, grad_gate, None, grad_hidden, d_fc1_w, d_fc2_w, None


class EPMergedFc1HipGroupGemm(torch.autograd.Function):
    """EP expert-MLP (parity: EPMergedFc1GroupGemm, moe_layer.py:414-567);
    routing weights applied later by `unpermute` in tokens_post_all2all.
    Kept for the plain dispatch path; the DISPATCHED EP path is
    EPMergedFc1HipGroupGemmA2A below (owns the dispatch a2a for the
    wgrad/a2a backward overlap)."""

    @staticmethod
    def forward(ctx, permute_tokens, cumsum, fc1_1_2_weight, fc2_weight,
                swiglu_limit=None):
        fc1 = hip_lib.group_gemm_nk(permute_tokens, fc1_1_2_weight, cumsum, trans_b=True)
        act = hip_lib.silu_mul_weighted(fc1, None, swiglu_limit)
        fc2 = hip_lib.group_gemm_nk(act, fc2_weight, cumsum, trans_b=True)
        ctx.swiglu_limit = swiglu_limit
        ctx.save_for_backward(permute_tokens, cumsum, fc1_1_2_weight, fc2_weight, fc1, act)
        return fc2

    @staticmethod
    def backward(ctx, grad_output):
        permute_tokens, cumsum, fc1_1_2_weight, fc2_weight, fc1, act = ctx.saved_tensors
        G = fc2_weight.shape[0]
        grad_output = grad_output.contiguous()
        d_act = hip_lib.group_gemm_nk(grad_output, fc2_weight, cumsum, trans_b=False)
        d_fc2_w = hip_lib.group_gemm_mn(grad_output, act, cumsum, G)
        d_fc1, _ = hip_lib.silu_mul_weighted_bwd(d_act, fc1, None, ctx.swiglu_limit)
        d_tokens = hip_lib.group_gemm_nk(d_fc1, fc1_1_2_weight, cumsum, trans_b=False)
        d_fc1_w = hip_lib.group_gemm_mn(d_fc1, permute_tokens, cumsum, G)
        return d_tokens, None, d_fc1_w, d_fc2_w, None


# ---- overlapped EP class: dispatch a2a owned by the autograd node so its
# backward launches the return exchange before the wgrad GEMMs ------------

def _ep_mlp_fwd(tokens, cumsum, fc1_1_2_weight, fc2_weight, swiglu_limit=None):
    fc1 = hip_lib.group_gemm_nk(tokens, fc1_1_2_weight, cumsum, trans_b=True)
    act = hip_lib.silu_mul_weighted(fc1, None, swiglu_limit)
    fc2 = hip_lib.group_gemm_nk(act, fc2_weight, cumsum, trans_b=True)
    return fc2, (tokens, fc1_1_2_weight, fc2_weight, fc1, act)


def _ep_mlp_bwd_dgrad(dY, cumsum, saved, swiglu_limit=None):
    _, w1, w2, fc1, _ = saved
    d_act = hip_lib.group_gemm_nk(dY, w2, cumsum, trans_b=False)
    d_fc1, _ = hip_lib.silu_mul_weighted_bwd(d_act, fc1, None, swiglu_limit)
    d_tokens = hip_lib.group_gemm_nk(d_fc1, w1, cumsum, trans_b=False)
    return d_tokens, (dY, d_fc1)


def _ep_mlp_bwd_wgrad(cumsum, saved, stash):
    tokens, _, w2, _, act = saved
    dY, d_fc1 = stash
    G = w2.shape[0]
    d_fc2_w = hip_lib.group_gemm_mn(dY, act, cumsum, G)
    d_fc1_w = hip_lib.group_gemm_mn(d_fc1, tokens, cumsum, G)
    return (d_fc1_w, d_fc2_w)


def _make_ep_a2a(swiglu_limit=None):
    from ...distributed.moe import make_ep_a2a_class

    if swiglu_limit is None:
        return make_ep_a2a_class(_ep_mlp_fwd, _ep_mlp_bwd_dgrad, _ep_mlp_bwd_wgrad)
    # the class takes closures, so the limit rides in them (the wgrad leg
    # never sees the activation and needs none)
    return make_ep_a2a_class(
        functools.partial(_ep_mlp_fwd, swiglu_limit=swiglu_limit),
        functools.partial(_ep_mlp_bwd_dgrad, swiglu_limit=swiglu_limit),
        _ep_mlp_bwd_wgrad)


EPMergedFc1HipGroupGemmA2A = _make_ep_a2a()


@functools.lru_cache(maxsize=None)
def ep_a2a_class_for_limit(swiglu_limit=None):
    """The overlapped EP class for a given swiglu_limit, built once per
    value. None is the module-level EPMergedFc1HipGroupGemmA2A itself."""
    if swiglu_limit is None:
        return EPMergedFc1HipGroupGemmA2A
    return _make_ep_a2a(float(swiglu_limit))


def check_swiglu_limit(swiglu_limit):
    """None, or a finite number > 0 (returned as float); else ValueError."""
    if swiglu_limit is None:
        return None
    try:
        ok = not isinstance(swiglu_limit, bool) and math.isfinite(swiglu_limit) \
            and swiglu_limit > 0
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(
            f"swiglu_limit must be a finite number > 0 or None, got {swiglu_limit!r}")
    return float(swiglu_limit)


def hip_fused_moe_forward(num_experts, routing_weights, selected_experts,
                          hidden_states, fc1_1_weight, fc1_2_weight, fc2_weight,
                          fc1_1_2_weight=None, swiglu_limit=None):
    """Signature parity: group_gemm_fused_moe_forward (group_gemm.py:523-603).

    Merged fc1 is the native layout (our models and the reference's v5
    experts use it); split weights are concatenated and take the same path.
    swiglu_limit (clamped SwiGLU: gate <= L, -L <= up <= L, gradients zeroed
    outside) is validated here, before any device work, and handed to the
    expert class; None keeps the unclamped kernels."""
    swiglu_limit = check_swiglu_limit(swiglu_limit)
    if fc1_1_2_weight is None:
        if fc1_1_weight is None or fc1_2_weight is None:
            raise ValueError("need merged fc1_1_2_weight or both split weights")
        fc1_1_2_weight = torch.cat([fc1_1_weight, fc1_2_weight], dim=1).contiguous()
    hs = hidden_states.reshape(-1, hidden_states.shape[-1])
    if get_parallel_state().ep_enabled:
        from ...distributed.moe import dispatch_to_ep_a2a_class

        out = dispatch_to_ep_a2a_class(
            ep_a2a_class_for_limit(swiglu_limit), num_experts, routing_weights,
            selected_experts, hs, fc1_1_2_weight, fc2_weight,
        )
    else:
        out = HipFusedMoeFunction.apply(
            num_experts, routing_weights, selected_experts, hs,
            fc1_1_2_weight, fc2_weight, swiglu_limit,
        )
    return out.reshape(hidden_states.shape)


# ---- gpt-oss experts (OpSlot moe_experts/gpt_oss) ------------------------
# A different module from the bank above (ref GptOssExperts): gate_up_proj
# [E, H, 2I] with gate / up INTERLEAVED along the last dim, down_proj
# [E, I, H], per-expert biases on both, (up + 1) * gate * sigmoid(alpha *
# gate) on the clamped values, routing weight applied AFTER down_proj + bias.
# Both weights are [G, K, N] for their forward GEMM, so every GEMM below reads
# them as they are stored (trans_b=False forward, True for the dgrads) and
# the wgrad kernel writes [G, M, N] = their stored layout: no weight copies.
# The grouped GEMMs produce RAW products; the kernels of vh_moe_gpt_oss.hip
# add the biases, so the saved fc1 / fc2 are bias-free and the backward
# recomputes clamp and mask from them (parity: the reference's
# GptOssQuackFusedMoeExpertFunction, quack_gemm_interleave_gate_up.py).

GPT_OSS_ALPHA = 1.702
GPT_OSS_LIMIT = 7.0


def _bias_grad(d_rows, cumsum, like):
    """Per-expert bias gradient: fp32 segment column sum, cast to the
    parameter's dtype."""
    return hip_lib.segment_colsum(d_rows, cumsum).to(like.dtype)


class HipGptOssFusedMoeFunction(torch.autograd.Function):
    """Non-EP gpt-oss experts. The row-to-expert lookup happens on the device
    (cumsum search in the kernels): no host read of the splits."""

    @staticmethod
    def forward(ctx, num_experts, gate_weights, expert_index, hidden_states,
                gate_up_proj, gate_up_proj_bias, down_proj, down_proj_bias,
                alpha, limit):
        splits = hip_lib.expert_histogram(expert_index, num_experts)
        _, scatter_index = compute_expert_scatter_index(expert_index)
        x_s = hip_lib.moe_scatter(hidden_states, scatter_index)
        cumsum_t = torch.cumsum(splits, dim=0)

        fc1 = hip_lib.group_gemm_nk(x_s, gate_up_proj, cumsum_t, trans_b=False)
        act = hip_lib.gptoss_glu(fc1, gate_up_proj_bias, cumsum_t, alpha, limit)
        fc2 = hip_lib.group_gemm_nk(act, down_proj, cumsum_t, trans_b=False)

        w = gate_weights.reshape(-1)
        scattered_w = torch.empty_like(w)
        scattered_w[scatter_index.flatten().to(torch.int64)] = w
        y = hip_lib.expert_bias_scale(fc2, down_proj_bias, cumsum_t, scattered_w)
        out = hip_lib.moe_gather(y, scatter_index)

        ctx.alpha, ctx.limit = alpha, limit
        ctx.save_for_backward(gate_weights, gate_up_proj, gate_up_proj_bias,
                              down_proj, down_proj_bias, scatter_index,
                              cumsum_t, x_s, fc1, act, fc2, scattered_w)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        (gate_weights, gate_up_proj, gate_up_proj_bias, down_proj,
         down_proj_bias, scatter_index, cumsum_t, x_s, fc1, act, fc2,
         scattered_w) = ctx.saved_tensors
        G = down_proj.shape[0]
        grad_output = grad_output.view(-1, grad_output.shape[-1]).contiguous()

        dy_rows = hip_lib.moe_scatter(grad_output, scatter_index)
        d_fc2, dw_rows = hip_lib.expert_bias_scale_bwd(
            dy_rows, fc2, down_proj_bias, cumsum_t, scattered_w)
        grad_gate = dw_rows[scatter_index.flatten().to(torch.int64)]
        grad_gate = grad_gate.reshape(gate_weights.shape).to(gate_weights.dtype)
        d_down_bias = _bias_grad(d_fc2, cumsum_t, down_proj_bias)

        d_act = hip_lib.group_gemm_nk(d_fc2, down_proj, cumsum_t, trans_b=True)
        d_down = hip_lib.group_gemm_mn(act, d_fc2, cumsum_t, G)          # [G, I, H]

        d_fc1 = hip_lib.gptoss_glu_bwd(d_act, fc1, gate_up_proj_bias, cumsum_t,
                                       ctx.alpha, ctx.limit)
        d_gate_up_bias = _bias_grad(d_fc1, cumsum_t, gate_up_proj_bias)
        d_x_s = hip_lib.group_gemm_nk(d_fc1, gate_up_proj, cumsum_t, trans_b=True)
        d_gate_up = hip_lib.group_gemm_mn(x_s, d_fc1, cumsum_t, G)       # [G, H, 2I]

        grad_hidden = hip_lib.moe_gather(d_x_s, scatter_index)
        return (None, grad_gate, None, grad_hidden, d_gate_up, d_gate_up_bias,
                d_down, d_down_bias, None, None)


def _gpt_oss_ep_fwd(tokens, cumsum, gate_up_proj, gate_up_proj_bias, down_proj,
                    down_proj_bias, *, alpha, limit):
    fc1 = hip_lib.group_gemm_nk(tokens, gate_up_proj, cumsum, trans_b=False)
    act = hip_lib.gptoss_glu(fc1, gate_up_proj_bias, cumsum, alpha, limit)
    fc2 = hip_lib.group_gemm_nk(act, down_proj, cumsum, trans_b=False)
    # routing weights are applied later by tokens_post_all2all's unpermute
    y = hip_lib.expert_bias_scale(fc2, down_proj_bias, cumsum, None)
    return y, (tokens, gate_up_proj, gate_up_proj_bias, down_proj,
               down_proj_bias, fc1, act)


def _gpt_oss_ep_bwd_dgrad(dY, cumsum, saved, *, alpha, limit):
    _, gate_up_proj, gate_up_proj_bias, down_proj, _, fc1, _ = saved
    # w_row=None forward: d_fc2 is dY itself
    d_act = hip_lib.group_gemm_nk(dY, down_proj, cumsum, trans_b=True)
    d_fc1 = hip_lib.gptoss_glu_bwd(d_act, fc1, gate_up_proj_bias, cumsum,
                                   alpha, limit)
    d_tokens = hip_lib.group_gemm_nk(d_fc1, gate_up_proj, cumsum, trans_b=True)
    return d_tokens, (dY, d_fc1)


def _gpt_oss_ep_bwd_wgrad(cumsum, saved, stash):
    tokens, _, gate_up_proj_bias, down_proj, down_proj_bias, _, act = saved
    dY, d_fc1 = stash
    G = down_proj.shape[0]
    d_gate_up = hip_lib.group_gemm_mn(tokens, d_fc1, cumsum, G)
    d_gate_up_bias = _bias_grad(d_fc1, cumsum, gate_up_proj_bias)
    d_down = hip_lib.group_gemm_mn(act, dY, cumsum, G)
    d_down_bias = _bias_grad(dY, cumsum, down_proj_bias)
    return (d_gate_up, d_gate_up_bias, d_down, d_down_bias)


@functools.lru_cache(maxsize=None)
def gpt_oss_ep_a2a_class(alpha=GPT_OSS_ALPHA, limit=GPT_OSS_LIMIT):
    """The overlapped gpt-oss EP class (weights: gate_up_proj,
    gate_up_proj_bias, down_proj, down_proj_bias), built once per
    (alpha, limit). Both bias column sums run in the wgrad leg, under the
    return all-to-all."""
    from ...distributed.moe import make_ep_a2a_class

    alpha, limit = float(alpha), float(limit)
    return make_ep_a2a_class(
        functools.partial(_gpt_oss_ep_fwd, alpha=alpha, limit=limit),
        functools.partial(_gpt_oss_ep_bwd_dgrad, alpha=alpha, limit=limit),
        _gpt_oss_ep_bwd_wgrad)


def check_gpt_oss_args(hidden_size, gate_up_proj, gate_up_proj_bias, down_proj,
                       down_proj_bias, alpha, limit):
    """Validate the gpt-oss expert arguments; returns (alpha, limit) as
    floats. ValueError on a bad limit / alpha or on shapes that do not fit
    [E,H,2I] / [E,2I] / [E,I,H] / [E,H]."""
    if limit is None:
        raise ValueError("swiglu_limit must be a finite number > 0 for the "
                         "gpt-oss experts (they always clamp), got None")
    limit = check_swiglu_limit(limit)
    try:
        ok = not isinstance(alpha, bool) and math.isfinite(alpha)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"alpha must be a finite number, got {alpha!r}")
    if gate_up_proj.dim() != 3 or down_proj.dim() != 3:
        raise ValueError(
            "gate_up_proj must be [E, H, 2I] and down_proj [E, I, H], got "
            f"{tuple(gate_up_proj.shape)} and {tuple(down_proj.shape)}")
    E, H, twoI = gate_up_proj.shape
    want = {"gate_up_proj": (E, hidden_size, twoI),
            "gate_up_proj_bias": (E, twoI),
            "down_proj": (E, twoI // 2, H),
            "down_proj_bias": (E, H)}
    got = {"gate_up_proj": gate_up_proj, "gate_up_proj_bias": gate_up_proj_bias,
           "down_proj": down_proj, "down_proj_bias": down_proj_bias}
    if twoI % 2:
        raise ValueError(f"gate_up_proj last dim must be even (2I), got {twoI}")
    for name, shape in want.items():
        if tuple(got[name].shape) != shape:
            raise ValueError(
                f"{name} must be {list(shape)} ([E,H,2I] / [E,2I] / [E,I,H] / "
                f"[E,H] layout), got {list(got[name].shape)}")
    return float(alpha), limit


def hip_gpt_oss_fused_moe_forward(num_experts, routing_weights, selected_experts,
                                  hidden_states, gate_up_proj, gate_up_proj_bias,
                                  down_proj, down_proj_bias,
                                  alpha=GPT_OSS_ALPHA, limit=GPT_OSS_LIMIT):
    """Signature parity: the reference's quack_gemm_gpt_oss_fused_moe_forward.
    Everything is validated here, before any device work."""
    alpha, limit = check_gpt_oss_args(
        hidden_states.shape[-1], gate_up_proj, gate_up_proj_bias, down_proj,
        down_proj_bias, alpha, limit)
    hs = hidden_states.reshape(-1, hidden_states.shape[-1])
    if get_parallel_state().ep_enabled:
        from ...distributed.moe import dispatch_to_ep_a2a_class

        out = dispatch_to_ep_a2a_class(
            gpt_oss_ep_a2a_class(alpha, limit), num_experts, routing_weights,
            selected_experts, hs, gate_up_proj, gate_up_proj_bias, down_proj,
            down_proj_bias)
    else:
        if gate_up_proj.shape[0] != num_experts:
            raise ValueError(
                f"gate_up_proj holds {gate_up_proj.shape[0]} experts, "
                f"num_experts is {num_experts}")
        out = HipGptOssFusedMoeFunction.apply(
            num_experts, routing_weights, selected_experts, hs, gate_up_proj,
            gate_up_proj_bias, down_proj, down_proj_bias, alpha, limit)
    return out.reshape(hidden_states.shape)


def fused_moe_forward(num_experts, routing_weights, selected_experts,
                      hidden_states, fc1_1_weight, fc1_2_weight, fc2_weight,
                      fc1_1_2_weight=None, swiglu_limit=None):
    """Module-pointer shim (parity: ops/kernels/moe/__init__.py:30-61)."""
    if _fused_moe_forward is None:
        raise NotImplementedError("No fused MoE kernel bound. Call apply_veomni_fused_moe_patch('hip').")
    assert routing_weights.dtype in (torch.bfloat16, torch.float16)
    assert hidden_states.dtype in (torch.bfloat16, torch.float16)
    return _fused_moe_forward(num_experts, routing_weights, selected_experts,
                              hidden_states, fc1_1_weight, fc1_2_weight,
                              fc2_weight, fc1_1_2_weight, swiglu_limit=swiglu_limit)


def apply_veomni_fused_moe_patch(fused_moe_kernel: str = "hip") -> None:
    """Bind the global `_fused_moe_forward` pointer (parity:
    ops/kernels/moe/__init__.py:64-118). Only "hip" exists on MI355X."""
    global _fused_moe_forward
    if fused_moe_kernel != "hip":
        raise ValueError(f"Invalid fused_moe_kernel: {fused_moe_kernel!r}; MI355X build provides 'hip'.")
    _fused_moe_forward = hip_fused_moe_forward


def _make_moe_experts_adapter(raw_forward):
    """OpSlot adapter (parity: ops/kernels/moe/__init__.py:126-161): pull
    num_experts / gate_up_proj / down_proj off the experts module."""

    def adapter(self, hidden_states, top_k_index, top_k_weights):
        return raw_forward(
            num_experts=self.num_experts,
            routing_weights=top_k_weights.to(hidden_states.dtype),
            selected_experts=top_k_index,
            hidden_states=hidden_states,
            fc1_1_weight=None,
            fc1_2_weight=None,
            fc2_weight=self.down_proj,
            fc1_1_2_weight=self.gate_up_proj,
            swiglu_limit=getattr(self, "limit", None),
        )

    return adapter


def _hip_moe_experts_factory():
    apply_veomni_fused_moe_patch("hip")
    return _make_moe_experts_adapter(fused_moe_forward)


KERNEL_REGISTRY.register(
    KernelSpec(
        name="hip", op_name="moe_experts", variant="standard",
        factory=_hip_moe_experts_factory,
        hardware=HardwareRequirement(device_type="gpu"),
        description="gfx950 grouped-GEMM fused MoE (vh_group_gemm_*)",
    )
)


def _make_gpt_oss_moe_experts_adapter(raw_forward):
    """OpSlot adapter for the gpt-oss experts module: pull num_experts, the
    two weights, the two biases, alpha and limit off it."""

    def adapter(self, hidden_states, router_indices, routing_weights):
        return raw_forward(
            num_experts=self.num_experts,
            routing_weights=routing_weights.to(hidden_states.dtype),
            selected_experts=router_indices,
            hidden_states=hidden_states,
            gate_up_proj=self.gate_up_proj,
            gate_up_proj_bias=self.gate_up_proj_bias,
            down_proj=self.down_proj,
            down_proj_bias=self.down_proj_bias,
            alpha=self.alpha,
            limit=self.limit,
        )

    return adapter


def _hip_gpt_oss_moe_experts_factory():
    return _make_gpt_oss_moe_experts_adapter(hip_gpt_oss_fused_moe_forward)


KERNEL_REGISTRY.register(
    KernelSpec(
        name="hip", op_name="moe_experts", variant="gpt_oss",
        factory=_hip_gpt_oss_moe_experts_factory,
        hardware=HardwareRequirement(device_type="gpu"),
        description="gfx950 gpt-oss experts: grouped GEMMs on the stored "
                    "layouts + vh_moe_gptoss_* / vh_moe_expert_bias_scale / "
                    "vh_moe_segment_colsum",
    )
)
