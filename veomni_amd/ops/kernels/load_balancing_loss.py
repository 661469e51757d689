"""HIP fused MoE load-balancing (aux) loss (impl name "hip").

Parity targets:
  - provider signature and mask validation:
    ops/kernels/load_balancing_loss/triton.py:280-354;
  - semantics (fp32 softmax, top-k counts, dot(count, prob_sum) * E / total^2):
    ops/kernels/load_balancing_loss/eager.py:28-114.

Unlike the reference's fused provider the per-layer logits are never
concatenated: vh_lbl_fwd runs once per layer into a shared partial buffer and
vh_lbl_finish reduces it (C ABI, include/veomni_hip.h). Expert selection is
top-k on the upcast logits with ties to the lowest expert index. The
total_weight == 0 early return happens on device, without a host sync.
"""

from __future__ import annotations

import torch

from .. import hip_lib
from ..kernel_registry import KERNEL_REGISTRY, HardwareRequirement, KernelSpec


class HipLoadBalancingLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, top_k, mask_w, total_w, *layers):
        loss, count, _, coef = hip_lib.lbl_fwd(layers, top_k, mask_w, total_w)
        ctx.save_for_backward(count, coef, *layers)
        ctx.mask_w = mask_w
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        count, coef, *layers = ctx.saved_tensors
        g = grad_out.to(torch.float32).reshape(1).contiguous()
        grads = [
            hip_lib.lbl_bwd(layer, ctx.mask_w, count, coef, g)
            if ctx.needs_input_grad[3 + i] else None
            for i, layer in enumerate(layers)
        ]
        return (None, None, None, *grads)


def hip_load_balancing_loss(gate_logits, num_experts=None, top_k=2,
                            attention_mask=None):
    """Reference-shaped entry: tuple of per-layer [B*S, E] router logits ->
    fp32 scalar loss (0 when gate_logits is None or not a tuple)."""
    if gate_logits is None or not isinstance(gate_logits, tuple):
        return 0
    dev, dtype = gate_logits[0].device, gate_logits[0].dtype
    for l in gate_logits:
        assert l.device == dev and l.dtype == dtype, \
            "gate_logits layers must share one device and dtype"
        assert l.dim() == 2 and l.shape[1] == num_experts, \
            f"gate_logits last dim ({tuple(l.shape)}) != num_experts ({num_experts})"
    layers = tuple(l.contiguous() for l in gate_logits)
    N = sum(l.shape[0] for l in layers)
    if attention_mask is not None:
        batch_size, sequence_length = attention_mask.shape
        expected = len(layers) * batch_size * sequence_length
        if N != expected or any(l.shape[0] * len(layers) != N for l in layers):
            raise ValueError(
                f"Mismatch between gate_logits total tokens ({N}) and "
                f"attention_mask shape. Expected {len(layers)} * {batch_size} * "
                f"{sequence_length} = {expected} tokens, but got {N}."
            )
        mask_w = attention_mask.to(dev).reshape(-1).float().contiguous()
        total_w = (mask_w.sum() * len(layers)).reshape(1)
    else:
        mask_w = None
        total_w = torch.full((1,), float(N), dtype=torch.float32, device=dev)
    if N == 0:
        return torch.zeros((), dtype=torch.float32, device=dev)
    return HipLoadBalancingLoss.apply(top_k, mask_w, total_w, *layers)


KERNEL_REGISTRY.register(
    KernelSpec(
        name="hip", op_name="load_balancing_loss", variant="standard",
        factory=lambda: hip_load_balancing_loss,
        hardware=HardwareRequirement(device_type="gpu"),
        description="gfx950 fused softmax/top-k aux loss, fwd+bwd (vh_lbl_*)",
    )
)
