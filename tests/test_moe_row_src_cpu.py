"""row_src, the index the grouped GEMMs read token rows through (CPU):
row_src[r] is the token whose copy lies at sorted row r, i.e. the inverse of
scatter_index folded to tokens."""

import pytest
import torch

from veomni_amd.ops.kernels.moe import (compute_expert_row_src,
                                        compute_expert_scatter_index)


def _routing(T, topk, E, seed, live_experts=None):
    g = torch.Generator().manual_seed(seed)
    scores = torch.rand(T, E, generator=g)
    if live_experts is not None:  # the other experts get no token
        scores[:, live_experts:] = -1.0
    return torch.topk(scores, topk, dim=-1).indices


@pytest.mark.parametrize("T,topk,E,live", [
    (37, 1, 8, None),
    (300, 4, 16, None),
    (300, 4, 128, 40),   # 128 experts, 88 of them empty
])
def test_row_src_inverts_scatter_index(T, topk, E, live):
    expert_index = _routing(T, topk, E, seed=7, live_experts=live)
    if live is not None:
        assert torch.bincount(expert_index.flatten(), minlength=E).eq(0).sum() >= E - live
    sorted_order, scatter_index = compute_expert_scatter_index(expert_index)
    row_src = compute_expert_row_src(sorted_order, topk)

    assert row_src.dtype == torch.int32
    assert row_src.shape == (T * topk,)
    tokens = torch.arange(T, dtype=torch.int32)[:, None].expand(T, topk)
    assert torch.equal(row_src[scatter_index.to(torch.int64)], tokens)
    # rows are in expert order: the experts read through row_src are sorted
    flat = expert_index.flatten()
    assert torch.equal(flat[sorted_order], flat.sort(stable=True).values)
