#!/usr/bin/env python3
"""Record reference outputs for the parity tests that used to import the
reference tree at test time, so the suite needs nothing outside this repo.

Usage: python tests/golden/make_property_golden.py <path-to-reference-checkout>

RUNS the reference's torch-only helpers on fixed, seeded cases and stores the
case parameters next to what the reference returned:

  fa_kwargs.json          prepare_fa_kwargs_from_position_ids + tail coalescing
  ep_permute.pt           moe_utils permute/unpermute/weights_idx/sort_chunks
  spcollate_grid.pt       SequenceParallelCollator pad+slice, every L in 2..97
                          x sp_size in {2,4,8}, every rank
  dynbatch_property.json  dynamic batching selections on 160 random streams
                          drawn from the ranges the property test used
"""

import importlib
import importlib.util
import json
import os
import random
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_file(ref, name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, *rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- fa kwargs
def make_fa_kwargs(ref_root):
    ref = _load_file(ref_root, "ref_seqlen", "veomni", "utils",
                     "seqlen_pos_transform_utils.py")
    rng = random.Random(5)
    cases = []
    for _ in range(50):
        nseq = rng.randint(1, 6)
        lens = [rng.randint(1, 40) for _ in range(nseq)]
        tail = rng.choice([0, 0, rng.randint(1, 8)])
        pos = torch.cat([torch.arange(L) for L in lens]
                        + ([torch.zeros(tail, dtype=torch.int64)] if tail else []))
        pos = pos[None]
        (cu_ref, _), (ml_ref, _) = ref.prepare_fa_kwargs_from_position_ids(pos)
        if tail:
            cu_ref = ref.coalesce_tail_padding_cu_seqlens(cu_ref, tail)
            sl = cu_ref[1:] - cu_ref[:-1]
            ml_ref = int(sl.max()) if sl.numel() else 0
        cases.append({"lens": lens, "tail": tail,
                      "cu_seqlens": [int(x) for x in cu_ref],
                      "max_length": int(ml_ref)})
    with open(os.path.join(HERE, "fa_kwargs.json"), "w") as f:
        json.dump(cases, f)
    return len(cases)


# --------------------------------------------------------------- ep permute
def make_ep_permute(ref_root):
    ref = _load_file(ref_root, "ref_moe_utils", "veomni", "distributed", "moe",
                     "moe_utils.py")
    rng = random.Random(9)
    cases = []
    for case in range(20):
        T, E, topk, H = (rng.randint(3, 40), rng.choice([4, 8, 16]),
                         rng.choice([1, 2, 4]), 16)
        g = torch.Generator().manual_seed(case)
        tokens = torch.randn(T, H, generator=g)
        sel = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)])
        w = torch.softmax(torch.randn(T, topk, generator=g), dim=-1)
        routing_map = torch.nn.functional.one_hot(sel, num_classes=E).permute(2, 1, 0).sum(1)
        rpt, rmap = ref.permute(tokens, routing_map)
        rwidx = ref.generate_weights_idx(w, sel, E)
        rout = ref.unpermute(rpt, rwidx, tokens.shape, rmap, routing_map)
        splits = routing_map.sum(1)
        order = list(torch.randperm(E, generator=g))
        rsorted = ref.sort_chunks_by_idxs(rpt, splits, order)
        cases.append({"E": E, "tokens": tokens, "sel": sel, "w": w,
                      "order": torch.stack(order),
                      "permuted": rpt, "mapping": rmap, "weights_idx": rwidx,
                      "unpermuted": rout, "sorted": rsorted})
    torch.save(cases, os.path.join(HERE, "ep_permute.pt"))
    return len(cases)


# --------------------------------------------------------------- sp collate
def _ref_collator_cls(ref_root):
    sys.path.insert(0, ref_root)
    torch.cuda.get_device_capability = lambda *a, **k: (8, 0)
    torch.cuda.get_device_name = lambda *a, **k: "cpu-x"
    torch.cpu.get_device_name = lambda *a, **k: "cpu-x"
    if "torchdata" not in sys.modules:
        from torch.utils.data import DataLoader as _DL
        from torch.utils.data.distributed import DistributedSampler as _DS

        td = types.ModuleType("torchdata")
        sd = types.ModuleType("torchdata.stateful_dataloader")
        sd.__path__ = []
        samp = types.ModuleType("torchdata.stateful_dataloader.sampler")
        sd.StatefulDataLoader = _DL
        samp.StatefulDistributedSampler = _DS
        td.stateful_dataloader = sd
        sys.modules["torchdata"] = td
        sys.modules["torchdata.stateful_dataloader"] = sd
        sys.modules["torchdata.stateful_dataloader.sampler"] = samp
    if "veomni.data" not in sys.modules:
        pkg = types.ModuleType("veomni.data")
        pkg.__path__ = [os.path.join(ref_root, "veomni", "data")]
        sys.modules["veomni.data"] = pkg
    return importlib.import_module(
        "veomni.data.data_collator").SequenceParallelCollator


def make_spcollate(ref_root):
    cls = _ref_collator_cls(ref_root)
    cases = []
    for L in range(2, 98):
        for sp_size in (2, 4, 8):
            seed = 131 * L + sp_size
            g = torch.Generator().manual_seed(seed)
            ids = torch.randint(0, 1000, (1, L), generator=g)
            labels = ids.clone()
            ref_ids, ref_lab = [], []
            for rank in range(sp_size):
                col = object.__new__(cls)
                col.sp_size = sp_size
                col.sp_rank = rank
                shifted = torch.nn.functional.pad(labels[..., 1:], (0, 1),
                                                  "constant", -100)
                ref_lab.append(col.sp_slice(
                    "labels", col.sp_padding("labels", shifted, dim=-1,
                                             pad_value=-100), dim=-1))
                ref_ids.append(col.sp_slice(
                    "input_ids", col.sp_padding("input_ids", ids, dim=-1,
                                                pad_value=0), dim=-1))
            # ranks hold equal-length slices: stack to [sp_size, 1, L/sp];
            # token ids < 1000 and -100 fit int16
            cases.append({"L": L, "sp_size": sp_size, "seed": seed,
                          "input_ids": torch.stack(ref_ids).to(torch.int16),
                          "labels": torch.stack(ref_lab).to(torch.int16)})
    torch.save(cases, os.path.join(HERE, "spcollate_grid.pt"))
    return len(cases)


# ----------------------------------------------------- dynbatch (property)
def _stream(lens):
    return [{"input_ids": torch.full((L,), i, dtype=torch.int64),
             "attention_mask": torch.ones(L, dtype=torch.int64),
             "sid": i} for i, L in enumerate(lens)]


def make_dynbatch_property(ref_root):
    import make_dynbatch_golden

    make_dynbatch_golden.REF = ref_root
    mod = make_dynbatch_golden._load_ref_dynbatch()
    rng = random.Random(20)
    cases = []
    for i in range(160):
        # same ranges as the property test drew from (min length 2: both
        # implementations DROP length-1 samples, and an all-dropped stream
        # spins the epoch wrap forever); the first cases pin the range ends
        n = rng.randint(20, 120)
        lens = [rng.randint(2, 300) for _ in range(n)]
        budget = rng.randint(64, 1024)
        buffer_size = rng.randint(1, 12)
        nmb = rng.randint(1, 3)
        length = rng.randint(3, 20)
        cap = rng.choice([None, rng.randint(64, 1024)])
        wsteps, winit = rng.choice([(0, 200), (5, 64), (12, 128)])
        if i == 0:
            lens, budget, buffer_size, nmb, length, cap = [2] * 20, 64, 1, 1, 3, 64
        elif i == 1:
            lens, budget, buffer_size, nmb, length, cap = [300] * 120, 1024, 12, 3, 20, 1024
        elif i == 2:
            budget, cap = 64, None      # every sample exceeds the budget
        elif i == 3:
            budget, cap = 1024, 64      # the physical cap binds, not the budget
        strat = mod.TextBatchingStrategy(
            token_micro_bsz=budget, buffer_size=buffer_size,
            physical_token_cap=cap, bsz_warmup_steps=wsteps,
            bsz_warmup_init_mbtoken=winit)
        loader = mod.DynamicBatchSizeDataLoader(
            _stream(lens), strat, collate_fn=None, num_micro_batch=nmb,
            length=length, drop_last=True)
        steps = []
        for group in loader:
            steps.append([[int(s["sid"]) for s in mb] for mb in group])
            if len(steps) >= 30:
                break
        cases.append({"lens": lens, "budget": budget, "buffer_size": buffer_size,
                      "nmb": nmb, "length": length, "cap": cap,
                      "warmup": [wsteps, winit], "steps": steps})
    with open(os.path.join(HERE, "dynbatch_property.json"), "w") as f:
        json.dump(cases, f, separators=(",", ":"))
    return len(cases)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "veomni")):
        sys.exit(__doc__)
    ref_root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, HERE)
    print("fa_kwargs", make_fa_kwargs(ref_root))
    print("ep_permute", make_ep_permute(ref_root))
    print("dynbatch_property", make_dynbatch_property(ref_root))
    print("spcollate_grid", make_spcollate(ref_root))


if __name__ == "__main__":
    main()
