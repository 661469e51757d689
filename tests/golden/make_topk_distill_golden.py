#!/usr/bin/env python3
"""Generate the top-k forward-KL distillation golden by RUNNING THE REFERENCE
(build container only), the way make_logprobs_golden.py does.

Executes the reference's chunk_topk_distill_function (ref ops/kernels/
cross_entropy/chunk_topk_distill.py:334-421) on CPU on seeded inputs and
records inputs, the five outputs and both gradients, so
tests/test_topk_distill_cpu.py never needs the reference at run time.

Usage:  python tests/golden/make_topk_distill_golden.py <path-to-reference-checkout>
        # writes tests/golden/topk_distill_golden.pt

Shape: B 2, L 19, H 32, V 200, K 6, chunk_size 8 (five chunks, the last
ragged). Labels carry ignore_index inside a row and over a row's end. The
teacher is the top-K of log_softmax(student fp32 logits + noise) at the
position whose hidden state predicts the slot, so student_mass is not
vanishing; one valid slot has a duplicated id and one has an id equal to its
label. Two teachers are stored: one aligned for the default mode (slot t
pairs with hidden t-1) and one for explicit shift_labels (slot t pairs with
hidden t).

Cases: fp32 and bf16 at temperature 1.0 and 0.7 without a clamp, fp32 and
bf16 at 0.7 with log_prob_min_clamp = CLAMP, one bf16 case with explicit
shift_labels, one bf16 case with bf16 teacher log-probs (clamped). CLAMP must
bind on the student side for between 1/4 and 3/4 of the valid (row, k)
entries and on the teacher side for some but not all of them: asserted below
for every clamped case, since a clamp that binds almost everywhere leaves a
backward of zeros that shows nothing.
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

from veomni.ops.kernels.cross_entropy.chunk_topk_distill import (  # noqa: E402
    chunk_topk_distill_function,
)

B, L, H, V, K, CHUNK, IGN = 2, 19, 32, 200, 6, 8, -100
CLAMP = -3.0

g = torch.Generator().manual_seed(20261)
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


def teacher_for(predicting_hidden, targets):
    """Top-K of log_softmax(student logits + noise); slot (b, t) is built
    from predicting_hidden[b, t]. Then the two forced entries."""
    noisy = (predicting_hidden @ weight.t()
             + torch.randn(B, L, V, generator=g)).log_softmax(-1)
    lp, ids = noisy.topk(K, dim=-1)
    ids, lp = ids.clone(), lp.clone()
    assert targets[0, 9] != IGN and targets[1, 5] != IGN
    ids[0, 9, 4] = ids[0, 9, 1]                 # a duplicated id
    ids[1, 5, 2] = targets[1, 5]                # an id equal to the label
    return ids, lp


# default mode: slot t (t >= 1) is predicted by hidden t-1; slot 0 is dropped
prev_hidden = torch.cat([hidden[:, :1], hidden[:, :-1]], dim=1)
t_ids, t_lp = teacher_for(prev_hidden, labels)
t_ids_shift, t_lp_shift = teacher_for(hidden, shift)

dlp = torch.randn(B, L, generator=g)
dent = torch.randn(B, L, generator=g)
ddist = torch.randn(B, L, generator=g)

out = {
    "meta/chunk_size": torch.tensor(CHUNK),
    "meta/ignore_index": torch.tensor(IGN),
    "meta/clamp": torch.tensor(CLAMP, dtype=torch.float64),
    "in/labels": labels,
    "in/shift_labels": shift,
    "in/teacher_ids": t_ids,
    "in/teacher_lp": t_lp,
    "in/teacher_ids_shift": t_ids_shift,
    "in/teacher_lp_shift": t_lp_shift,
    "in/dlog_probs": dlp,
    "in/dentropy": dent,
    "in/ddistill": ddist,
}
for dt_name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
    out[f"in/{dt_name}/hidden"] = hidden.to(dt)
    out[f"in/{dt_name}/weight"] = weight.to(dt)


def clamp_binding(h, w, temp, tgt, ids, tlp):
    """Fractions of the valid (row, k) entries on which CLAMP binds, student
    side and teacher side, on aligned inputs."""
    logits = (h @ w.t())
    if temp != 1.0:
        logits = logits / temp
    s_k = logits.float().log_softmax(-1).gather(-1, ids)
    valid = (tgt != IGN).unsqueeze(-1).expand_as(s_k)
    return (float((s_k < CLAMP)[valid].float().mean()),
            float((tlp.float() < CLAMP)[valid].float().mean()))


# name, dtype, temperature, clamp, explicit shift, bf16 teacher log-probs
CASES = [
    ("fp32_t1", "fp32", 1.0, False, False, False),
    ("fp32_t07", "fp32", 0.7, False, False, False),
    ("bf16_t1", "bf16", 1.0, False, False, False),
    ("bf16_t07", "bf16", 0.7, False, False, False),
    ("fp32_t07_clamp", "fp32", 0.7, True, False, False),
    ("bf16_t07_clamp", "bf16", 0.7, True, False, False),
    ("bf16_t07_shift", "bf16", 0.7, False, True, False),
    ("bf16_t07_clamp_tlpbf16", "bf16", 0.7, True, False, True),
]
for name, dt_name, temp, use_clamp, use_shift, tlp_bf16 in CASES:
    h = out[f"in/{dt_name}/hidden"].clone().requires_grad_(True)
    w = out[f"in/{dt_name}/weight"].clone().requires_grad_(True)
    ids = t_ids_shift if use_shift else t_ids
    tlp = t_lp_shift if use_shift else t_lp
    if tlp_bf16:
        tlp = tlp.to(torch.bfloat16)
    if use_clamp:
        assert not use_shift
        fs, ft = clamp_binding(h.detach()[:, :-1], w.detach(), temp,
                               labels[:, 1:], ids[:, 1:], tlp[:, 1:])
        print(f"{name}: clamp {CLAMP} binds on {fs:.2f} of the student and "
              f"{ft:.2f} of the teacher entries")
        assert 0.25 <= fs <= 0.75, fs
        assert 0.0 < ft < 1.0, ft
    outs = chunk_topk_distill_function(
        h, w, labels, ids, tlp, chunk_size=CHUNK, ignore_index=IGN,
        shift_labels=shift if use_shift else None, temperature=temp,
        log_prob_min_clamp=CLAMP if use_clamp else None)
    lp, ent, dist, sm, tm = outs
    assert all(t.shape == labels.shape and t.dtype == torch.float32 for t in outs)
    torch.autograd.backward([lp, ent, dist], [dlp, dent, ddist])
    out[f"case/{name}/temperature"] = torch.tensor(temp, dtype=torch.float64)
    out[f"case/{name}/use_clamp"] = torch.tensor(use_clamp)
    out[f"case/{name}/use_shift"] = torch.tensor(use_shift)
    out[f"case/{name}/tlp_bf16"] = torch.tensor(tlp_bf16)
    for key, t in zip(("log_probs", "entropy", "distill", "student_mass",
                       "teacher_mass"), outs):
        out[f"case/{name}/{key}"] = t.detach()
    out[f"case/{name}/dhidden"] = h.grad
    out[f"case/{name}/dweight"] = w.grad

dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                   "topk_distill_golden.pt")
torch.save(out, dst)
print(f"wrote {dst}: {os.path.getsize(dst)} bytes, {len(out)} entries")
