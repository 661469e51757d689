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
    positions. The three distillation fields belong to the top-k
    distillation path, which this project does not implement; they stay None.
    """

    log_probs: Optional[torch.Tensor] = None
    entropy: Optional[torch.Tensor] = None
    distillation_losses: Optional[torch.Tensor] = None
    student_mass: Optional[torch.Tensor] = None
    teacher_mass: Optional[torch.Tensor] = None
