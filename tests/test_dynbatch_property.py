"""Parity: our dynamic batching vs the REFERENCE's on 160 random sample
streams drawn from the ranges the property test used (stream lengths 20..120
of samples 2..300 tokens, budgets/caps 64..1024, buffers 1..12, 1..3
micro-batches, 3..20 steps, three warmup schedules; the range ends pinned).
The reference's selections were recorded by RUNNING it
(tests/golden/make_property_golden.py -> golden/dynbatch_property.json), so
the test needs nothing outside this repository."""

import json
import os

import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden", "dynbatch_property.json")


def _stream(lens):
    out = []
    for i, L in enumerate(lens):
        out.append({"input_ids": torch.full((L,), i, dtype=torch.int64),
                    "attention_mask": torch.ones(L, dtype=torch.int64),
                    "sid": i})
    return out


def _run(mod_strategy, mod_loader, lens, budget, buffer_size, nmb, length,
         cap, wsteps=0, winit=200):
    strat = mod_strategy(token_micro_bsz=budget, buffer_size=buffer_size,
                         physical_token_cap=cap, bsz_warmup_steps=wsteps,
                         bsz_warmup_init_mbtoken=winit)
    loader = mod_loader(_stream(lens), strat, collate_fn=None,
                        num_micro_batch=nmb, length=length, drop_last=True)
    steps = []
    for group in loader:
        steps.append([[int(s["sid"]) for s in mb] for mb in group])
        if len(steps) >= 30:
            break
    return steps


def test_selection_matches_reference():
    from veomni_amd.data import DynamicBatchDataLoader, TextBatchingStrategy

    cases = json.load(open(GOLD))
    assert len(cases) == 160
    assert any(c["cap"] is None for c in cases) and any(c["cap"] for c in cases)
    assert {tuple(c["warmup"]) for c in cases} == {(0, 200), (5, 64), (12, 128)}
    for i, c in enumerate(cases):
        wsteps, winit = c["warmup"]
        ours = _run(TextBatchingStrategy, DynamicBatchDataLoader, c["lens"],
                    c["budget"], c["buffer_size"], c["nmb"], c["length"],
                    c["cap"], wsteps, winit)
        assert ours == c["steps"], (i, {k: v for k, v in c.items()
                                        if k not in ("lens", "steps")})
