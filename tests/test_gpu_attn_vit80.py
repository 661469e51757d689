"""The head_dim 80 HIP vision flash pair (pytest -m gpu): kernels through the
autograd function and through the vision tower.

Shapes: D = 80, bf16, H = 2, scale 80^-0.5, S <= 332. Reference: fp32 torch
autograd on the device from the same bf16 inputs with an explicit
block-diagonal mask (the _ref of tests/test_gpu_attn_d64.py without the causal
term), with that file's tolerances: output atol 3e-2, each gradient's max
error < 0.06 * max(|ref|max, 1). The LSE bound of that file's header (1e-4
against an fp64 logsumexp) holds here with at most 332 terms per row."""

import copy
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

H, D = 2, 80
SCALE = 80 ** -0.5
RAGGED = [0, 64, 128, 172, 176, 332]
LAYOUTS = {
    "aligned": [0, 64, 128, 192, 256],
    "ragged": RAGGED,
    "one_image": [0, 300],
}


@pytest.fixture(scope="module")
def data():
    """One [332, 3, H, 80] qkv tensor and one dO for the module (never
    modified); a layout of S rows takes the first S."""
    g = torch.Generator().manual_seed(80)
    qkv = (torch.randn(332, 3, H, D, generator=g) * 0.5).to(torch.bfloat16).cuda()
    do = (torch.randn(332, H, D, generator=g) * 0.5).to(torch.bfloat16).cuda()
    return qkv, do


def _ref(q, k, v, do, cu):
    S = q.shape[0]
    seg = torch.zeros(S, dtype=torch.long, device="cuda")
    for n, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
        seg[a:b] = n
    qf, kf, vf = (t.float().transpose(0, 1).requires_grad_(True) for t in (q, k, v))
    sc = torch.matmul(qf, kf.transpose(-1, -2)) * SCALE
    sc = sc.masked_fill(seg[:, None] != seg[None, :], float("-inf"))
    lse = torch.logsumexp(sc.detach().double(), dim=-1)
    out = torch.matmul(torch.softmax(sc, dim=-1), vf)
    grads = torch.autograd.grad(out, (qf, kf, vf), do.float().transpose(0, 1))
    return tuple(t.detach().transpose(0, 1) for t in (out, *grads)) + (lse,)


def _hip(q, k, v, do, cu):
    from veomni_amd.ops.kernels.attention import hip_vision_attention

    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    out = hip_vision_attention(q, k, v, cu, SCALE)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), do)
    return out.detach(), dq, dk, dv


def _inputs(data, S):
    qkv, do = data
    return [qkv[:S, i].contiguous() for i in range(3)] + [do[:S]]


@pytest.mark.parametrize("case", list(LAYOUTS) + ["strided_v"])
def test_vit80_pair_vs_autograd(data, case):
    from veomni_amd.ops import hip_lib
    from veomni_amd.ops.kernels.attention import segments_from_cu_seqlens

    cu = LAYOUTS.get(case, RAGGED)
    S = cu[-1]
    q, k, v, do = _inputs(data, S)
    got = _hip(q, k, v, do, cu)
    ref = _ref(q, k, v, do, cu)
    for t, r, nm in zip(got, ref, ("out", "dq", "dk", "dv")):
        assert t.shape == (S, H, D) and t.is_contiguous()
        assert torch.isfinite(t.float()).all(), f"{case} {nm}: non-finite"
        err = (t.float() - r).abs().max().item()
        m = r.abs().max().item()
        print(f"{case} {nm} max err {err:.3e} |ref|max {m:.3e}")
        if nm == "out":
            assert err <= 3e-2, err
        else:
            assert err < 0.06 * max(m, 1.0), f"{case} {nm}: {err} vs |ref|max {m}"
    seg = segments_from_cu_seqlens(cu, S, "cuda") if len(cu) > 2 else (None, None)
    o, lse = hip_lib.attn80_fwd(q, k, v, SCALE, *seg)
    assert torch.equal(o, got[0])
    e_lse = (lse.double() - ref[4]).abs().max().item()
    print(f"{case} LSE max err {e_lse:.3e}")
    assert torch.isfinite(lse).all() and e_lse <= 1e-4, e_lse

    if case == "one_image":
        # explicit [0, S) bounds against both bounds None (= one segment)
        lo = torch.zeros(S, dtype=torch.int32, device="cuda")
        hi = torch.full((S,), S, dtype=torch.int32, device="cuda")
        o2, lse2 = hip_lib.attn80_fwd(q, k, v, SCALE, lo, hi)
        g1 = hip_lib.attn80_bwd(q, k, v, o, lse, do, SCALE)
        g2 = hip_lib.attn80_bwd(q, k, v, o2, lse2, do, SCALE, lo, hi)
        for a, b in zip((o, lse, *g1), (o2, lse2, *g2)):
            assert torch.equal(a, b)
    if case == "strided_v":
        # q, k, v as views of one [S, 3, H, 80] tensor: v (and q, k) strided
        qkv = data[0][:S]
        views = [qkv[:, i] for i in range(3)]
        assert views[2].stride(0) == 3 * H * D
        for a, b, nm in zip(_hip(*views, do, cu), got, ("out", "dq", "dk", "dv")):
            assert torch.equal(a, b), f"strided views differ from copies: {nm}"


def test_vit80_reproducible(data):
    q, k, v, do = _inputs(data, 332)
    for a, b in zip(_hip(q, k, v, do, RAGGED), _hip(q, k, v, do, RAGGED)):
        assert torch.equal(a, b)


def test_vit80_tower_vs_eager():
    """A 2-block vision tower at head_dim 80 (block 1 full attention) on a grid
    that leaves partial windows: bf16 with the attention slots bound "hip"
    (every other op eager), bound "eager", and an fp32 eager copy. The hip
    error against fp32, for the output and the qkv.weight gradient of both
    blocks, is at most twice the eager-bf16 error; core = "sdpa" is the eager
    binding bit for bit."""
    from veomni_amd.models import VL_PRESETS, _init_vl_presets
    from veomni_amd.models.modeling import bind_ops
    from veomni_amd.models.vlm import VisionAttention, VisionTower, vision_window_index

    _init_vl_presets()
    cfg = dataclasses.replace(VL_PRESETS["tiny-vl"].vision, depth=2, hidden_size=160,
                              num_heads=2, fullatt_block_indexes=(1,))
    grids = [[1, 10, 20], [1, 8, 8]]
    lens = torch.tensor(vision_window_index(grids, cfg)[2]).diff()
    assert lens.unique().numel() > 1, "the grid must leave a partial window"
    torch.manual_seed(5)
    with torch.device("cuda"):
        tower = VisionTower(cfg).to(torch.bfloat16)
    n = sum(t * h * w for t, h, w in grids)
    px = torch.randn(n, tower.patch_embed.in_features, device="cuda")
    gout = torch.randn(n // cfg.merge_unit, cfg.out_hidden_size, device="cuda")

    def run(model, impl, dtype):
        bind_ops(impl)
        model.zero_grad(set_to_none=True)
        out = model(px.to(dtype), grids)
        out.backward(gout.to(dtype))
        return [out.detach().float()] + [b.attn.qkv.weight.grad.float().clone()
                                         for b in model.blocks]

    try:
        ref = run(copy.deepcopy(tower).float(), "eager", torch.float32)
        eager = run(tower, "eager", torch.bfloat16)
        hip = run(tower, {"attention": "hip"}, torch.bfloat16)
        VisionAttention.core = "sdpa"
        sdpa = run(tower, {"attention": "hip"}, torch.bfloat16)
    finally:
        VisionAttention.core = "slot"
        bind_ops("eager")
    for r, e, h_, s, nm in zip(ref, eager, hip, sdpa, ("out", "qkv0.grad", "qkv1.grad")):
        err_e, err_h = (e - r).abs().max().item(), (h_ - r).abs().max().item()
        print(f"{nm} |fp32|max {r.abs().max().item():.3e} eager {err_e:.3e} hip {err_h:.3e}")
        assert torch.isfinite(h_).all() and err_h <= 2 * err_e, (nm, err_h, err_e)
        assert torch.equal(s, e), f"core='sdpa' differs from the eager binding: {nm}"
    assert not torch.equal(hip[0], eager[0]), "the hip binding ran the twin"
