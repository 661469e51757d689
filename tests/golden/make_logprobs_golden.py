#!/usr/bin/env python3
"""Generate the per-token log-probs / entropy golden by RUNNING THE REFERENCE
(build container only), the way make_golden.py does.

Executes the reference's chunk_logprobs_function (ref ops/kernels/
cross_entropy/chunk_logprobs.py:276-356) on CPU on seeded inputs and records
inputs, both outputs and both gradients, so tests/test_logprobs_cpu.py never
needs the reference at run time.

Usage:  python tests/golden/make_logprobs_golden.py <path-to-reference-checkout>
        # writes tests/golden/logprobs_golden.pt

Shape: B 2, L 19, H 32, V 200, chunk_size 8 (five chunks, the last ragged).
Labels carry ignore_index inside a row and over a row's end. Cases: fp32 and
bf16 at temperature 1.0 and 0.7, plus one bf16 case with explicit
shift_labels. Inputs are stored once per dtype; the bf16 inputs are the fp32
ones rounded.
"""

import os
import sys

import torch

assert len(sys.argv) == 2 and os.path.isdir(sys.argv[1]), __doc__
sys.path.insert(0, sys.argv[1])

# No GPU in the build container; the reference probes the device at import
# time (see make_golden.py). Only a config-file path prefix depends on it.
torch.cuda.get_device_capability = lambda *a, **k: (8, 0)
torch.cuda.get_device_name = lambda *a, **k: "cpu-golden"
torch.cpu.get_device_name = lambda *a, **k: "cpu-golden"

from veomni.ops.kernels.cross_entropy.chunk_logprobs import (  # noqa: E402
    chunk_logprobs_function,
)

B, L, H, V, CHUNK, IGN = 2, 19, 32, 200, 8, -100

g = torch.Generator().manual_seed(20260)
hidden = torch.randn(B, L, H, generator=g)
weight = torch.randn(V, H, generator=g) * 0.5
labels = torch.randint(0, V, (B, L), generator=g)
labels[0, 4:7] = IGN        # inside a row
labels[0, 12] = IGN
labels[1, 15:] = IGN        # a row's end
labels[0, 1] = 0            # first and last vocabulary entry
labels[1, 2] = V - 1
shift = torch.randint(0, V, (B, L), generator=g)
shift[0, 0] = IGN
shift[1, 9:12] = IGN
shift[1, L - 1] = IGN
dlp = torch.randn(B, L, generator=g)
dent = torch.randn(B, L, generator=g)

out = {
    "meta/chunk_size": torch.tensor(CHUNK),
    "meta/ignore_index": torch.tensor(IGN),
    "in/labels": labels,
    "in/shift_labels": shift,
    "in/dlog_probs": dlp,
    "in/dentropy": dent,
}
for dt_name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
    out[f"in/{dt_name}/hidden"] = hidden.to(dt)
    out[f"in/{dt_name}/weight"] = weight.to(dt)

CASES = [
    ("fp32_t1", "fp32", 1.0, False),
    ("fp32_t07", "fp32", 0.7, False),
    ("bf16_t1", "bf16", 1.0, False),
    ("bf16_t07", "bf16", 0.7, False),
    ("bf16_t07_shift", "bf16", 0.7, True),
]
for name, dt_name, temp, use_shift in CASES:
    h = out[f"in/{dt_name}/hidden"].clone().requires_grad_(True)
    w = out[f"in/{dt_name}/weight"].clone().requires_grad_(True)
    lp, ent = chunk_logprobs_function(
        h, w, labels, chunk_size=CHUNK, ignore_index=IGN,
        shift_labels=shift if use_shift else None, temperature=temp)
    assert lp.shape == labels.shape and lp.dtype == torch.float32
    torch.autograd.backward([lp, ent], [dlp, dent])
    out[f"case/{name}/temperature"] = torch.tensor(temp, dtype=torch.float64)
    out[f"case/{name}/use_shift"] = torch.tensor(use_shift)
    out[f"case/{name}/log_probs"] = lp.detach()
    out[f"case/{name}/entropy"] = ent.detach()
    out[f"case/{name}/dhidden"] = h.grad
    out[f"case/{name}/dweight"] = w.grad

dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "logprobs_golden.pt")
torch.save(out, dst)
print(f"wrote {dst}: {os.path.getsize(dst)} bytes, {len(out)} entries")
