"""Auxiliary model outputs (no torch.nn dependency).

Parity target: the reference's FusedLinearAuxOutput, the payload in the third
slot of the ForCausalLMLoss 3-tuple (ref cross_entropy/__init__.py:104, :177).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch


@dataclass
class FusedLinearAuxOutput:
    """Per-token tensors of a fused lm_head pass that never builds [T, V].

    log_probs / entropy: fp32, shape of the labels, exactly 0 at ignored
    positions. distillation_losses / student_mass / teacher_mass: the top-k
    forward KL against a teacher and the probability mass either side puts
    on the teacher's top-k ids, same shape and masking; filled only when
    teacher_topk_ids and teacher_topk_log_probs are given, else None. The
    two masses are metrics (requires_grad=False).
    """

    log_probs: Optional[torch.Tensor] = None
    entropy: Optional[torch.Tensor] = None
    distillation_losses: Optional[torch.Tensor] = None
    student_mass: Optional[torch.Tensor] = None
    teacher_mass: Optional[torch.Tensor] = None
