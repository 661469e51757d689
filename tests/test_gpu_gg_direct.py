"""Grouped GEMMs that read their operands as autograd hands them over
(pytest -m gpu): the direct wgrad kernel (token-major A and B, no
transpose-padded copies) and the !trans_b dgrad through nk256s (stored
[G, K, N] weights, no transposed copy). Everything goes through the hip_lib
wrappers, i.e. what the model runs. Reference: per-group fp32 matmul on the
device; tolerance: the one tests/test_gpu_kernels.py uses for these paths
(rtol = atol = 3e-2 on randn * 0.3 data)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = dict(rtol=3e-2, atol=3e-2)


@pytest.fixture(scope="module")
def lib():
    from veomni_amd.ops import hip_lib

    return hip_lib


def bf(x):
    return x.to(torch.bfloat16)


def _ranges(counts):
    out, start = [], 0
    for c in counts:
        out.append((start, start + c))
        start += c
    return out


def _wgrad_inputs(counts, M, N, seed):
    torch.manual_seed(seed)
    rows = sum(counts)
    a = bf(torch.randn(rows, M) * 0.3).cuda()
    b = bf(torch.randn(rows, N) * 0.3).cuda()
    cumsum = torch.tensor(counts).cumsum(0).cuda()
    return a, b, cumsum


def _check_wgrad(c, a, b, counts):
    for g, (s, e) in enumerate(_ranges(counts)):
        if e == s:
            assert torch.all(c[g] == 0), f"group {g} not zero-filled"
            continue
        ref = a[s:e].float().t() @ b[s:e].float()
        torch.testing.assert_close(c[g].float(), ref, **TOL,
                                   msg=lambda m: f"group {g}: {m}")


# ------------------------------------------------------------------- wgrad
@pytest.mark.parametrize("counts,M,N", [
    # empty group, a group shorter than one k-tile, start rows that are no
    # multiple of 8 or 64
    ([1000, 0, 1500, 37, 1559], 1536, 2048),
    # the k-tile boundary from both sides, odd and even tile counts (double-
    # buffer parity), 8 x 48 = 384 output tiles > 256 persistent blocks
    ([1, 63, 64, 65, 128, 129, 0, 1700], 1536, 2048),
    # 16-multiples that are no 256-multiples: partial last m- and n-tiles
    ([700, 900, 0, 600], 528, 784),
])
def test_wgrad_direct(lib, counts, M, N):
    a, b, cumsum = _wgrad_inputs(counts, M, N, seed=21)
    c = lib.group_gemm_mn(a, b, cumsum, len(counts))
    _check_wgrad(c, a, b, counts)


def test_wgrad_direct_neighbour_poison(lib):
    """Rows outside a group contribute exactly nothing: with every other row
    NaN in both operands (and NaN rows behind the last group, the operands
    being views into a larger allocation) c[g] is bit-equal to the clean run."""
    counts = [1000, 0, 1500, 37, 1559]
    M, N = 1536, 2048
    G, rows = len(counts), sum(counts)
    a0, b0, cumsum = _wgrad_inputs(counts, M, N, seed=22)
    pad = 96
    a_big = torch.full((rows + pad, M), float("nan"), dtype=torch.bfloat16, device="cuda")
    b_big = torch.full((rows + pad, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    a_big[:rows] = a0
    b_big[:rows] = b0
    clean = lib.group_gemm_mn(a_big[:rows], b_big[:rows], cumsum, G)
    _check_wgrad(clean, a0, b0, counts)
    for g, (s, e) in enumerate(_ranges(counts)):
        if e == s:
            continue
        a_big.fill_(float("nan"))
        b_big.fill_(float("nan"))
        a_big[s:e] = a0[s:e]
        b_big[s:e] = b0[s:e]
        c = lib.group_gemm_mn(a_big[:rows], b_big[:rows], cumsum, G)
        assert torch.equal(c[g], clean[g]), f"group {g} picked up neighbour rows"
        assert torch.all(c[1] == 0), "empty group not zero-filled"


def test_wgrad_direct_deterministic(lib):
    counts = [1000, 0, 1500, 37, 1559]
    a, b, cumsum = _wgrad_inputs(counts, 1536, 2048, seed=23)
    c1 = lib.group_gemm_mn(a, b, cumsum, len(counts))
    c2 = lib.group_gemm_mn(a, b, cumsum, len(counts))
    assert torch.equal(c1, c2)


# ------------------------------------------------------------------- dgrad
def _dgrad_inputs(counts, K, N, seed):
    torch.manual_seed(seed)
    rows, G = sum(counts), len(counts)
    a = bf(torch.randn(rows, K) * 0.3).cuda()
    w = bf(torch.randn(G, K, N) * 0.3).cuda()
    cumsum = torch.tensor(counts).cumsum(0).cuda()
    return a, w, cumsum


@pytest.mark.parametrize("counts,K,N", [
    ([500, 0, 279, 333], 2048, 768),   # fc2 weights [G, H, I]
    ([500, 0, 279, 333], 1536, 2048),  # fc1 weights [G, 2I, H]
    ([5, 1000, 3], 1536, 784),         # partial n-tile, groups << one tile
])
def test_dgrad_direct(lib, counts, K, N):
    a, w, cumsum = _dgrad_inputs(counts, K, N, seed=24)
    c = lib.group_gemm_nk(a, w, cumsum, trans_b=False)
    for g, (s, e) in enumerate(_ranges(counts)):
        if e == s:
            continue
        ref = a[s:e].float() @ w[g].float()
        torch.testing.assert_close(c[s:e].float(), ref, **TOL,
                                   msg=lambda m: f"group {g}: {m}")


def test_dgrad_direct_equals_transposed_path(lib):
    """Bit-equal by construction: the transposed LDS reads give lane l the
    same k (32 ks + 8 (l >> 4) + 0..7) of the same column as the row reads of
    the transposed weights, the A side, tile walk and MFMA order are shared."""
    counts = [500, 0, 279, 333]
    a, w, cumsum = _dgrad_inputs(counts, 2048, 768, seed=24)
    c = lib.group_gemm_nk(a, w, cumsum, trans_b=False)
    ct = lib.group_gemm_nk(a, lib.weight_transpose(w), cumsum, trans_b=True)
    assert torch.equal(c, ct)


# ---------------------------------------------------------------- autograd
def test_fused_moe_fwd_bwd_vs_eager_direct_paths():
    """The toy fused MoE of test_fused_moe_fwd_bwd_vs_eager_gpu at sizes that
    reach the new dispatches (rows = 2200 >= 2048, H = 512, 2I = 1024, I = 512;
    rows >= 256 G), against the eager expert loop at that test's tolerances."""
    from veomni_amd.models.modeling import Experts, ModelConfig
    from veomni_amd.ops.kernels.moe import HipFusedMoeFunction

    torch.manual_seed(25)
    H, I, E, T = 512, 512, 4, 1100
    cfg = ModelConfig(hidden_size=H, num_experts=E, num_experts_per_tok=2,
                      moe_intermediate_size=I, vocab_size=64)
    experts = Experts(cfg).cuda().to(torch.bfloat16)
    with torch.no_grad():
        experts.gate_up_proj.normal_(0, 0.05)
        experts.down_proj.normal_(0, 0.05)
    hidden = bf(torch.randn(T, H) * 0.5).cuda()
    rw = torch.softmax(torch.randn(T, E), -1)
    top_w, top_i = torch.topk(rw, 2, -1)
    top_w = bf(top_w / top_w.sum(-1, keepdim=True)).cuda()
    top_i = top_i.cuda()

    h1 = hidden.clone().requires_grad_(True)
    gup1 = experts.gate_up_proj.detach().clone().requires_grad_(True)
    down1 = experts.down_proj.detach().clone().requires_grad_(True)
    tw1 = top_w.clone().requires_grad_(True)
    out_hip = HipFusedMoeFunction.apply(E, tw1, top_i, h1, gup1, down1)
    dy = bf(torch.randn_like(out_hip) * 0.1)
    out_hip.backward(dy)

    h2 = hidden.clone().requires_grad_(True)
    tw2 = top_w.clone().requires_grad_(True)
    out_eager = experts(h2, top_i, tw2)
    out_eager.backward(dy)

    tol = dict(rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(out_hip.float(), out_eager.float(), **tol)
    torch.testing.assert_close(h1.grad.float(), h2.grad.float(), **tol)
    torch.testing.assert_close(gup1.grad.float(), experts.gate_up_proj.grad.float(), **tol)
    torch.testing.assert_close(down1.grad.float(), experts.down_proj.grad.float(), **tol)
    torch.testing.assert_close(tw1.grad.float(), tw2.grad.float(), rtol=1e-1, atol=1e-1)
