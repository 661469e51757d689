"""Grouped GEMMs that read token rows through an index (pytest -m gpu):
nk256s with A = x[row_src] (both B layouts) and the direct wgrad with an
indexed A or B, against the same wrappers on the materialised gather. The
indexed kernels stage the same bytes into the same LDS image and share tile
walk, MFMA order and epilogue with the plain ones, so every comparison is
torch.equal. Everything goes through the hip_lib wrappers."""

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from veomni_amd.ops import hip_lib

    return hip_lib


def bf(x):
    return x.to(torch.bfloat16)


def _arbitrary_index(rows, n_src, seed):
    """Non-monotone, with repeats, and only every other source row used."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n_src // 2, (rows,), generator=g) * 2
    return idx.to(torch.int32).cuda()


def _routing_index(T, topk, E, seed):
    from veomni_amd.ops.kernels.moe import (compute_expert_row_src,
                                            compute_expert_scatter_index)

    g = torch.Generator().manual_seed(seed)
    expert_index = torch.topk(torch.rand(T, E, generator=g), topk, -1).indices.cuda()
    sorted_order, _ = compute_expert_scatter_index(expert_index)
    counts = torch.bincount(expert_index.flatten(), minlength=E)
    return compute_expert_row_src(sorted_order, topk), counts.cumsum(0)


def _cumsum(counts):
    return torch.tensor(counts).cumsum(0).cuda()


# ---------------------------------------------------------------------- nk
NK_COUNTS = [
    # an empty group, a group shorter than a tile, unaligned starts
    [1000, 0, 1500, 37, 1559],
    # more than 8 groups: every XCD range of the schedule holds tiles of
    # several groups
    [256] * 9 + [300, 17, 700],
]
NK_SHAPES = [(128, 256), (256, 528)]  # (K, N); N 528: a partial n-tile


def _nk_case(lib, row_src, cumsum, n_src, K, N, trans_b, seed):
    G, rows = cumsum.numel(), row_src.numel()
    assert lib.get_lib().vh_group_gemm_nk_takes_index(G, N, K, rows), \
        "shape must reach the indexed kernel"
    torch.manual_seed(seed)
    x = bf(torch.randn(n_src, K) * 0.3).cuda()
    w = bf(torch.randn(*((G, N, K) if trans_b else (G, K, N))) * 0.3).cuda()
    indexed = lib.group_gemm_nk(x, w, cumsum, trans_b=trans_b, a_rows=row_src)
    plain = lib.group_gemm_nk(x[row_src.long()], w, cumsum, trans_b=trans_b)
    assert torch.equal(indexed, plain)


@pytest.mark.parametrize("trans_b", [True, False])
@pytest.mark.parametrize("K,N", NK_SHAPES)
@pytest.mark.parametrize("counts", NK_COUNTS, ids=["ragged", "12groups"])
def test_nk_indexed_arbitrary_index(lib, counts, K, N, trans_b):
    n_src = 1500
    row_src = _arbitrary_index(sum(counts), n_src, seed=31)
    _nk_case(lib, row_src, _cumsum(counts), n_src, K, N, trans_b, seed=32)


@pytest.mark.parametrize("trans_b", [True, False])
@pytest.mark.parametrize("K,N", NK_SHAPES)
def test_nk_indexed_topk_routing(lib, K, N, trans_b):
    T, topk, E = 700, 4, 8
    row_src, cumsum = _routing_index(T, topk, E, seed=33)
    _nk_case(lib, row_src, cumsum, T, K, N, trans_b, seed=34)


# --------------------------------------------------------------------- wgd
WGD_CASES = [
    # k-tile boundaries from both sides, both double-buffer parities, an
    # empty group; 8 x 48 = 384 output tiles > 256 persistent blocks
    ([1, 63, 64, 65, 128, 129, 0, 1700], 1536, 2048),
    # partial last m- and n-tiles
    ([700, 900, 0, 600], 528, 784),
]


def _wgd_case(lib, counts, M, N, index_b, seed):
    rows, G = sum(counts), len(counts)
    assert lib.get_lib().vh_group_gemm_mn_takes_wgd(M, N, rows)
    n_src = 1200
    row_src = _arbitrary_index(rows, n_src, seed=seed)
    cumsum = _cumsum(counts)
    torch.manual_seed(seed + 1)
    if index_b:
        a = bf(torch.randn(rows, M) * 0.3).cuda()
        b = bf(torch.randn(n_src, N) * 0.3).cuda()
        indexed = lib.group_gemm_mn(a, b, cumsum, G, b_rows=row_src)
        plain = lib.group_gemm_mn(a, b[row_src.long()], cumsum, G)
    else:
        a = bf(torch.randn(n_src, M) * 0.3).cuda()
        b = bf(torch.randn(rows, N) * 0.3).cuda()
        indexed = lib.group_gemm_mn(a, b, cumsum, G, a_rows=row_src)
        plain = lib.group_gemm_mn(a[row_src.long()], b, cumsum, G)
    assert torch.equal(indexed, plain)
    for g, c in enumerate(counts):
        if c == 0:
            assert torch.all(indexed[g] == 0), f"group {g} not zero-filled"


@pytest.mark.parametrize("index_b", [False, True], ids=["idxA", "idxB"])
@pytest.mark.parametrize("counts,M,N", WGD_CASES, ids=["ktile-edges", "partial-mn"])
def test_wgd_indexed(lib, counts, M, N, index_b):
    _wgd_case(lib, counts, M, N, index_b, seed=41)


@pytest.mark.parametrize("index_b", [False, True], ids=["idxA", "idxB"])
def test_wgd_indexed_topk_routing(lib, index_b):
    T, topk, E = 700, 4, 8
    row_src, cumsum = _routing_index(T, topk, E, seed=43)
    M, N = 512, 768
    torch.manual_seed(44)
    rows = T * topk
    a = bf(torch.randn(rows if index_b else T, M) * 0.3).cuda()
    b = bf(torch.randn(T if index_b else rows, N) * 0.3).cuda()
    if index_b:
        indexed = lib.group_gemm_mn(a, b, cumsum, E, b_rows=row_src)
        plain = lib.group_gemm_mn(a, b[row_src.long()], cumsum, E)
    else:
        indexed = lib.group_gemm_mn(a, b, cumsum, E, a_rows=row_src)
        plain = lib.group_gemm_mn(a[row_src.long()], b, cumsum, E)
    assert torch.equal(indexed, plain)


# ------------------------------------------------------------------ poison
def _poisoned_source(clean, row_src):
    """The source as a view into a larger all-NaN allocation, with every row
    that no index entry references NaN as well."""
    n_src, width = clean.shape
    pad = 64
    big = torch.full((n_src + 2 * pad, width), float("nan"),
                     dtype=torch.bfloat16, device="cuda")
    view = big[pad:pad + n_src]
    used = torch.zeros(n_src, dtype=torch.bool, device="cuda")
    used[row_src.long()] = True
    assert not bool(used.all()), "the case needs unreferenced rows"
    view[used] = clean[used]
    return view


@pytest.mark.parametrize("trans_b", [True, False])
def test_nk_indexed_poison(lib, trans_b):
    counts, K, N, n_src = [1000, 0, 1500, 37, 1559], 256, 528, 1500
    row_src = _arbitrary_index(sum(counts), n_src, seed=51)
    cumsum = _cumsum(counts)
    torch.manual_seed(52)
    x = bf(torch.randn(n_src, K) * 0.3).cuda()
    G = len(counts)
    w = bf(torch.randn(*((G, N, K) if trans_b else (G, K, N))) * 0.3).cuda()
    clean = lib.group_gemm_nk(x, w, cumsum, trans_b=trans_b, a_rows=row_src)
    assert not bool(torch.isnan(clean).any())
    poisoned = lib.group_gemm_nk(_poisoned_source(x, row_src), w, cumsum,
                                 trans_b=trans_b, a_rows=row_src)
    assert torch.equal(poisoned, clean)


@pytest.mark.parametrize("index_b", [False, True], ids=["idxA", "idxB"])
def test_wgd_indexed_poison(lib, index_b):
    counts, M, N, n_src = [1, 63, 64, 65, 128, 129, 0, 1700], 528, 784, 1200
    rows, G = sum(counts), len(counts)
    row_src = _arbitrary_index(rows, n_src, seed=53)
    cumsum = _cumsum(counts)
    torch.manual_seed(54)
    a = bf(torch.randn(rows if index_b else n_src, M) * 0.3).cuda()
    b = bf(torch.randn(n_src if index_b else rows, N) * 0.3).cuda()
    kw = dict(b_rows=row_src) if index_b else dict(a_rows=row_src)
    clean = lib.group_gemm_mn(a, b, cumsum, G, **kw)
    assert not bool(torch.isnan(clean).any())
    if index_b:
        poisoned = lib.group_gemm_mn(a, _poisoned_source(b, row_src), cumsum, G, **kw)
    else:
        poisoned = lib.group_gemm_mn(_poisoned_source(a, row_src), b, cumsum, G, **kw)
    assert torch.equal(poisoned, clean)


# ---------------------------------------------------------- function level
def _parent_formulation(lib, E, gate_w, expert_index, hidden, w1, w2, dy):
    """HipFusedMoeFunction forward + backward as it was before the index:
    moe_scatter copies of hidden and dy feeding the unindexed wrappers."""
    from veomni_amd.ops.kernels.moe import compute_expert_scatter_index

    splits = lib.expert_histogram(expert_index, E)
    _, sidx = compute_expert_scatter_index(expert_index)
    pos = sidx.flatten().to(torch.int64)
    scatter_output = lib.moe_scatter(hidden, sidx)
    cs = torch.cumsum(splits, dim=0)
    fc1 = lib.group_gemm_nk(scatter_output, w1, cs, trans_b=True)
    w = gate_w.reshape(-1)
    scattered_w = torch.empty_like(w)
    scattered_w[pos] = w
    weighted = lib.silu_mul_weighted(fc1, scattered_w, None)
    fc2 = lib.group_gemm_nk(weighted, w2, cs, trans_b=True)
    out = lib.moe_gather(fc2, sidx)

    grad_fc2_out = lib.moe_scatter(dy, sidx)
    d_weighted = lib.group_gemm_nk(grad_fc2_out, w2, cs, trans_b=False)
    d_fc2_w = lib.group_gemm_mn(grad_fc2_out, weighted, cs, E)
    d_fc1, dw_rows = lib.silu_mul_weighted_bwd(d_weighted, fc1, scattered_w, None)
    grad_gate = dw_rows[pos].reshape(gate_w.shape).to(gate_w.dtype)
    d_scatter = lib.group_gemm_nk(d_fc1, w1, cs, trans_b=False)
    d_fc1_w = lib.group_gemm_mn(d_fc1, scatter_output, cs, E)
    grad_hidden = lib.moe_gather(d_scatter, sidx)
    return out, grad_hidden, d_fc1_w, d_fc2_w, grad_gate


# T 1024 / I 256: fc1, fc2 dgrad and the fc1 wgrad take the indexed kernels;
# the fc2 wgrad (M = H = 512, N = I = 256 < 512) is below the direct wgrad's
# shape predicate and runs on materialised rows. I 512 puts all four on the
# indexed kernels. T 64: the fallback everywhere, no indexed kernel runs.
@pytest.mark.parametrize("T,I", [(1024, 256), (1024, 512), (64, 256)])
def test_fused_moe_equals_parent_formulation(lib, T, I):
    from veomni_amd.ops.kernels.moe import HipFusedMoeFunction

    topk, E, H = 4, 8, 512
    g = torch.Generator().manual_seed(61)
    hidden = bf(torch.randn(T, H, generator=g) * 0.5).cuda()
    w1 = bf(torch.randn(E, 2 * I, H, generator=g) * 0.05).cuda()
    w2 = bf(torch.randn(E, H, I, generator=g) * 0.05).cuda()
    top_w, top_i = torch.topk(torch.softmax(torch.randn(T, E, generator=g), -1), topk, -1)
    gate_w = bf(top_w / top_w.sum(-1, keepdim=True)).cuda()
    top_i = top_i.cuda()
    dy = bf(torch.randn(T, H, generator=g) * 0.1).cuda()

    h = hidden.clone().requires_grad_(True)
    gw = gate_w.clone().requires_grad_(True)
    a1 = w1.clone().requires_grad_(True)
    a2 = w2.clone().requires_grad_(True)
    out = HipFusedMoeFunction.apply(E, gw, top_i, h, a1, a2)
    out.backward(dy)

    p1 = _parent_formulation(lib, E, gate_w, top_i, hidden, w1, w2, dy)
    p2 = _parent_formulation(lib, E, gate_w, top_i, hidden, w1, w2, dy)

    assert torch.equal(out.detach(), p1[0])
    assert torch.equal(h.grad, p1[1])
    assert torch.equal(a1.grad, p1[2])
    assert torch.equal(a2.grad, p1[3])
    # dw_row is summed with fp32 atomics: allow what the parent formulation
    # itself moves by between two runs, measured here
    spread = (p1[4].float() - p2[4].float()).abs().max().item()
    diff = (gw.grad.float() - p1[4].float()).abs().max().item()
    print(f"grad_gate: parent run-to-run spread {spread:.3e}, indexed vs parent {diff:.3e}")
    assert diff <= spread
