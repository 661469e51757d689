#!/usr/bin/env python3
"""Generate the sliding-window / attention-sink golden by RUNNING THE
REFERENCE (build container only), the way make_logprobs_golden.py does.

Executes the reference's gpt-oss eager_attention_forward (ref models/
transformers/gpt_oss/generated/patched_modeling_gpt_oss_gpu.py:281-309) on CPU
in fp32 on seeded inputs, with additive masks built here from the window and
document rule, and records inputs, outputs and autograd gradients (dsinks
included), so tests/test_attn_window_sinks_cpu.py never needs the reference
at run time.

Usage:  python tests/golden/make_attn_window_sinks_golden.py <path-to-reference-checkout>
        # writes tests/golden/attn_window_sinks_golden.pt

Mask rule (the reference's and HF's sliding window): key j is visible to
query i iff j <= i and j > i - W, and j lies in i's document. Masked entries
carry finfo(fp32).min, visible ones 0, as HF's mask builders do.

The reference function always appends the sink column. Cases without sinks
use a sink logit of -inf: exp(-inf) = 0 drops the column exactly.

Shapes: B 1, Hq 4, Hkv 2 (GQA 2:1); D 16 at S 48 and D 128 at S 32. Cases:
window only, sinks only, both, both plus two packed documents, W = 1. The
inputs (q, k, v, do, sinks) are drawn once per D and shared by its cases,
which keeps the file within the size limit for committed files.
"""

import math
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

from veomni.models.transformers.gpt_oss.generated.patched_modeling_gpt_oss_gpu import (  # noqa: E402
    eager_attention_forward,
)

HQ, HKV = 4, 2

B = 1
SEQ = {16: 48, 128: 32}
# name, D, W, sinks?, cu_seqlens
CASES = [
    ("window_d16", 16, 7, False, None),
    ("sinks_d16", 16, None, True, None),
    ("both_d16", 16, 7, True, None),
    ("both_docs_d16", 16, 7, True, [0, 19, 48]),
    ("w1_d16", 16, 1, True, None),
    ("both_d128", 128, 10, True, None),
    ("both_docs_d128", 128, 10, True, [0, 13, 32]),
]


def additive_mask(S, W, cu):
    i = torch.arange(S)[:, None]
    j = torch.arange(S)[None, :]
    allowed = j <= i
    if W is not None:
        allowed &= j > i - W
    if cu is not None:
        doc = torch.zeros(S, dtype=torch.long)
        for n, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
            doc[a:b] = n
        allowed &= doc[:, None] == doc[None, :]
    m = torch.zeros(S, S).masked_fill(~allowed, torch.finfo(torch.float32).min)
    return m[None, None]


g = torch.Generator().manual_seed(20261)
out = {}
for D, S in SEQ.items():
    out[f"in/d{D}/q"] = torch.randn(B, HQ, S, D, generator=g)
    out[f"in/d{D}/k"] = torch.randn(B, HKV, S, D, generator=g)
    out[f"in/d{D}/v"] = torch.randn(B, HKV, S, D, generator=g)
    out[f"in/d{D}/do"] = torch.randn(B, S, HQ, D, generator=g)   # [B, S, Hq, D]
    out[f"in/d{D}/sinks"] = torch.randn(HQ, generator=g)

for name, D, W, use_sinks, cu in CASES:
    S = SEQ[D]
    q = out[f"in/d{D}/q"].clone().requires_grad_(True)
    k = out[f"in/d{D}/k"].clone().requires_grad_(True)
    v = out[f"in/d{D}/v"].clone().requires_grad_(True)
    do = out[f"in/d{D}/do"]
    if use_sinks:
        sinks = out[f"in/d{D}/sinks"].clone().requires_grad_(True)
    else:
        sinks = torch.full((HQ,), float("-inf"))
    module = types.SimpleNamespace(num_key_value_groups=HQ // HKV, sinks=sinks,
                                   training=False)
    scaling = 1.0 / math.sqrt(D)
    o, _ = eager_attention_forward(module, q, k, v, additive_mask(S, W, cu),
                                   scaling=scaling, dropout=0.0)
    assert o.shape == (B, S, HQ, D) and o.dtype == torch.float32
    o.backward(do)
    out[f"case/{name}/D"] = torch.tensor(D)
    out[f"case/{name}/W"] = torch.tensor(-1 if W is None else W)
    out[f"case/{name}/use_sinks"] = torch.tensor(use_sinks)
    out[f"case/{name}/scaling"] = torch.tensor(scaling, dtype=torch.float64)
    if cu is not None:
        out[f"case/{name}/cu_seqlens"] = torch.tensor(cu, dtype=torch.int32)
    out[f"case/{name}/out"] = o.detach()        # [B, S, Hq, D]
    out[f"case/{name}/dq"] = q.grad
    out[f"case/{name}/dk"] = k.grad
    out[f"case/{name}/dv"] = v.grad
    if use_sinks:
        out[f"case/{name}/dsinks"] = sinks.grad

dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                   "attn_window_sinks_golden.pt")
torch.save(out, dst)
print(f"wrote {dst}: {os.path.getsize(dst)} bytes, {len(out)} entries")
