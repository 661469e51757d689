#!/usr/bin/env python3
"""Generate the gpt-oss experts / router golden by RUNNING THE REFERENCE (build
container only), the way make_attn_window_sinks_golden.py does.

Executes the reference's GptOssExperts (eager per-expert loop, slot bound to
"eager") and GptOssTopKRouter (ref models/transformers/gpt_oss/generated/
patched_modeling_gpt_oss_gpu.py) on CPU in fp32 on seeded inputs and records
inputs, outputs and autograd gradients, so tests/test_gpt_oss_moe_cpu.py never
needs the reference at run time.

Usage:  python tests/golden/make_gpt_oss_moe_golden.py <path-to-reference-checkout>
        # writes tests/golden/gpt_oss_moe_golden.pt

Shapes: T 40, H 64, I 32, E 4, top-2; generator seed 11. gate_up ~ 0.25 N,
gate_up_bias ~ 0.5 N, down ~ 0.25 N, down_bias ~ 0.5 N, hidden ~ N(0, 1).
The router bias of expert 2 is -inf, so its logits are -inf and it receives
no token. Two cases on the same tensors: experts.limit = 1.5 (a good share
of gate and up pre-activations saturates) and the default 7.0 (essentially
none does).
"""

import os
import sys
import types

import torch

assert len(sys.argv) == 2 and os.path.isdir(sys.argv[1]), __doc__
sys.path.insert(0, sys.argv[1])

# No GPU in the build container; the reference probes the device at import
# time (see make_golden.py). Only a config-file path prefix depends on it.
torch.cuda.get_device_capability = lambda *a, **k: (8, 0)
torch.cuda.get_device_name = lambda *a, **k: "cpu-golden"
torch.cpu.get_device_name = lambda *a, **k: "cpu-golden"

from veomni.models.transformers.gpt_oss.generated import (  # noqa: E402
    patched_modeling_gpt_oss_gpu as ref,
)

ref.veomni_moe_experts_forward.bind("eager")

T, H, I, E, TOPK = 40, 64, 32, 4, 2
EMPTY_EXPERT = 2
CASES = [("limit_1p5", 1.5), ("limit_default", 7.0)]

cfg = types.SimpleNamespace(hidden_size=H, intermediate_size=I,
                            num_local_experts=E, num_experts_per_tok=TOPK)
g = torch.Generator().manual_seed(11)
out = {
    "in/gate_up_proj": torch.randn(E, H, 2 * I, generator=g) * 0.25,
    "in/gate_up_proj_bias": torch.randn(E, 2 * I, generator=g) * 0.5,
    "in/down_proj": torch.randn(E, I, H, generator=g) * 0.25,
    "in/down_proj_bias": torch.randn(E, H, generator=g) * 0.5,
    "in/hidden": torch.randn(T, H, generator=g),
    "in/router_weight": torch.randn(E, H, generator=g) * 0.25,
    "in/router_bias": torch.randn(E, generator=g) * 0.5,
    "in/dy": torch.randn(T, H, generator=g),
}
out["in/router_bias"][EMPTY_EXPERT] = float("-inf")

router = ref.GptOssTopKRouter(cfg)
with torch.no_grad():
    router.weight.copy_(out["in/router_weight"])
    router.bias.copy_(out["in/router_bias"])
    logits, scores, indices = router(out["in/hidden"])
assert (indices == EMPTY_EXPERT).sum() == 0
out["router/logits"], out["router/scores"], out["router/indices"] = logits, scores, indices

for name, limit in CASES:
    experts = ref.GptOssExperts(cfg)
    assert experts.alpha == 1.702 and experts.limit == 7.0
    experts.limit = limit
    with torch.no_grad():
        for p in ("gate_up_proj", "gate_up_proj_bias", "down_proj", "down_proj_bias"):
            getattr(experts, p).copy_(out[f"in/{p}"])
    hidden = out["in/hidden"].clone().requires_grad_(True)
    rw = scores.clone().requires_grad_(True)
    y = experts(hidden, indices, rw)
    assert y.shape == (T, H) and y.dtype == torch.float32
    y.backward(out["in/dy"])
    # saturation shares of the routed pre-activations
    sat_g = sat_u = n = 0
    with torch.no_grad():
        for k in range(TOPK):
            e = indices[:, k]
            gu = torch.einsum("th,thf->tf", out["in/hidden"], out["in/gate_up_proj"][e]) \
                + out["in/gate_up_proj_bias"][e]
            sat_g += (gu[:, ::2] > limit).sum().item()
            sat_u += (gu[:, 1::2].abs() > limit).sum().item()
            n += gu[:, ::2].numel()
    print(f"{name}: gate saturated {sat_g / n:.3f}, up saturated {sat_u / n:.3f}")
    out[f"case/{name}/limit"] = torch.tensor(limit, dtype=torch.float64)
    out[f"case/{name}/alpha"] = torch.tensor(experts.alpha, dtype=torch.float64)
    out[f"case/{name}/out"] = y.detach()
    out[f"case/{name}/d_hidden"] = hidden.grad
    out[f"case/{name}/d_routing_weights"] = rw.grad
    for p in ("gate_up_proj", "gate_up_proj_bias", "down_proj", "down_proj_bias"):
        out[f"case/{name}/d_{p}"] = getattr(experts, p).grad

dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                   "gpt_oss_moe_golden.pt")
torch.save(out, dst)
print(f"wrote {dst}: {os.path.getsize(dst)} bytes, {len(out)} entries")
