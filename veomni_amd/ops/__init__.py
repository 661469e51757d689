"""Operator API (drop-in mirror of the reference's `veomni.ops`).

Importing this package registers every MI355X kernel under impl name "hip"
in KERNEL_REGISTRY. `HIP_OPS_CONFIG` is the per-op implementation map the
bench/tests bind (the OpsImplementationConfig analog)."""

import os

from .dispatch import OpSlot  # noqa: F401
from .kernel_registry import (  # noqa: F401
    KERNEL_REGISTRY,
    HardwareRequirement,
    KernelSpec,
)
from . import kernels  # noqa: F401  (registrations run at import)

# Per-op implementation selection for the MI355X hot path. The aux
# load-balancing loss has a fused HIP provider (ops/kernels/
# load_balancing_loss.py, vh_lbl_*) that is opt-in: the default binding stays
# "eager" (the model's own torch code), and VEOMNI_LBL_IMPL=eager|hip, read
# once here, overrides that one entry (A/B numbers: profiles/lbl_microbench.md).
_LBL_IMPL = os.environ.get("VEOMNI_LBL_IMPL", "eager")
if _LBL_IMPL not in ("eager", "hip"):
    raise ValueError(
        f"VEOMNI_LBL_IMPL={_LBL_IMPL!r}: expected 'eager' or 'hip'"
    )

HIP_OPS_CONFIG = {
    "rms_norm": "hip",
    "rotary_pos_emb": "hip",
    "swiglu_mlp": "hip",
    "moe_experts": "hip",
    "cross_entropy_loss": "hip",
    "load_balancing_loss": _LBL_IMPL,
    "attention": "hip",
}
