"""Parity: our sp_collate (shift/pad/slice) vs the reference's
SequenceParallelCollator methods, on every length 2..97 x sp size {2,4,8} x
rank. The reference's slices were recorded by RUNNING it
(tests/golden/make_property_golden.py -> golden/spcollate_grid.pt), so the
test needs nothing outside this repository."""

import os

import torch

GRID = os.path.join(os.path.dirname(__file__), "golden", "spcollate_grid.pt")


def test_shift_pad_slice_matches_reference():
    from veomni_amd.data import sp_collate

    cases = torch.load(GRID, weights_only=False)
    # the whole grid the property test sampled from
    assert {(c["L"], c["sp_size"]) for c in cases} == {
        (L, sp) for L in range(2, 98) for sp in (2, 4, 8)}
    for c in cases:
        L, sp_size = c["L"], c["sp_size"]
        g = torch.Generator().manual_seed(c["seed"])
        ids = torch.randint(0, 1000, (1, L), generator=g)
        labels = ids.clone()
        assert c["input_ids"].shape[0] == sp_size
        for rank in range(sp_size):
            ref_ids = c["input_ids"][rank].to(torch.int64)
            ref_lab = c["labels"][rank].to(torch.int64)
            ours = sp_collate({"input_ids": ids, "labels": labels.clone()},
                              sp_size=sp_size, sp_rank=rank)
            assert torch.equal(ours["input_ids"], ref_ids), (L, sp_size, rank)
            assert torch.equal(ours["labels"], ref_lab), (L, sp_size, rank)
