"""Clamped SwiGLU (`swiglu_limit`) on the MI355X (pytest -m gpu).

Kernel level: the clamped epilogue pair against the UNCLAMPED pair as the
yardstick (exact comparisons): clamping the input with torch and running the
unclamped kernel must give the same bits as the clamped kernel on the raw
input, with the gradient zeroed where the raw value is out of range.

Function level: every fused expert path with a limit against an fp64
restatement of the reference's merged-fc1 math (torch.clamp autograd), with
the eager bf16 experts on the same GPU setting the error scale.

Model level: tiny-moe with a limit, HIP op stack vs eager."""

import dataclasses

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from veomni_amd.ops import hip_lib

    return hip_lib


def bf(x):
    return x.to(torch.bfloat16)


# --------------------------------------------------------------- kernel level
# Forward grid: at most 2048 blocks x 256 lanes = 524288 vectors per pass.
# Backward: at most 2048 blocks x 4 waves = 8192 rows per pass.
# (8195, 520): 8195 * 65 = 532675 vectors (forward grid-strides) and 8195 rows
# (backward strides rows), with the strided tail landing mid-row. (3, 520):
# 65 vectors per half, not a multiple of the wave. (0, 64): no rows.
SHAPES = [(1, 8), (3, 520), (0, 64), (8195, 520)]
L = 0.5  # fc1 ~ N(0, 1): ~31 % of gate and ~62 % of up saturate


def _inputs(rows, I, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * rows + I)
    fc1 = bf(torch.randn(rows, 2 * I, generator=g)).cuda()
    dy = bf(torch.randn(rows, I, generator=g)).cuda()
    w = bf(torch.rand(rows, generator=g) + 0.25).cuda()
    return fc1, dy, w


def _clamp_torch(fc1, leff):
    I = fc1.shape[1] // 2
    return torch.cat([fc1[:, :I].clamp(max=leff),
                      fc1[:, I:].clamp(min=-leff, max=leff)], dim=1).contiguous()


def _in_range(fc1, leff):
    """True where the gradient passes: gate <= L, -L <= up <= L (inclusive)."""
    I = fc1.shape[1] // 2
    return torch.cat([fc1[:, :I] <= leff,
                      (fc1[:, I:] >= -leff) & (fc1[:, I:] <= leff)], dim=1)


def _assert_bites(fc1, leff):
    if fc1.numel() == 0:
        return
    I = fc1.shape[1] // 2
    g_share = (fc1[:, :I] > leff).float().mean().item()
    u_share = (fc1[:, I:].abs() > leff).float().mean().item()
    assert 0.10 <= g_share <= 0.90, g_share
    assert 0.10 <= u_share <= 0.90, u_share


@pytest.mark.parametrize("has_w", [True, False])
@pytest.mark.parametrize("rows,I", SHAPES)
def test_clamped_forward_equals_unclamped_on_clamped_input(lib, rows, I, has_w):
    fc1, _, w = _inputs(rows, I)
    w = w if has_w else None
    leff = lib.swiglu_limit_bf16(L)
    _assert_bites(fc1, leff)
    got = lib.silu_mul_weighted(fc1, w, limit=L)
    want = lib.silu_mul_weighted(_clamp_torch(fc1, leff), w)
    assert got.shape == (rows, I)
    assert torch.equal(got, want)


@pytest.mark.parametrize("has_w", [True, False])
@pytest.mark.parametrize("rows,I", SHAPES)
def test_clamped_backward_equals_masked_unclamped(lib, rows, I, has_w):
    fc1, dy, w = _inputs(rows, I)
    w = w if has_w else None
    leff = lib.swiglu_limit_bf16(L)
    _assert_bites(fc1, leff)
    dfc1, dw = lib.silu_mul_weighted_bwd(dy, fc1, w, limit=L)
    dfc1_u, dw_u = lib.silu_mul_weighted_bwd(dy, _clamp_torch(fc1, leff), w)
    want = torch.where(_in_range(fc1, leff), dfc1_u, torch.zeros_like(dfc1_u))
    assert torch.equal(dfc1, want)
    if has_w:
        # fp32 reassociation over at most I terms, nothing else
        torch.testing.assert_close(dw, dw_u, rtol=1e-4, atol=1e-6)
    else:
        assert dw is None


def test_boundary_values_inclusive(lib):
    """limit 7.12 rounds to bf16 7.125. Values exactly at +-L keep their
    gradient; the next bf16 outside gets exactly 0."""
    limit = 7.12
    leff = lib.swiglu_limit_bf16(limit)
    assert leff == 7.125

    def step(v, n):  # n bf16 ulps away from zero (n > 0) or towards it
        t = torch.tensor([v], dtype=torch.bfloat16)
        return (t.view(torch.int16) + n).view(torch.bfloat16).item()

    above, below = step(leff, 1), step(leff, -1)
    assert below < leff < above
    #        at +L  outside  inside  at -L   outside  inside  plain
    half = [leff, above, below, -leff, -above, -below, 0.5, -0.5]
    fc1 = bf(torch.tensor([half + half])).cuda()
    dy = torch.ones(1, 8, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(1, dtype=torch.bfloat16, device="cuda")
    dfc1, dw = lib.silu_mul_weighted_bwd(dy, fc1, w, limit=limit)
    dg, du = dfc1[0, :8].float().cpu(), dfc1[0, 8:].float().cpu()
    # gate: only the upper bound exists
    assert dg[1] == 0
    assert all(dg[j] != 0 for j in (0, 2, 3, 4, 5, 6, 7)), dg
    # up: both bounds
    assert du[1] == 0 and du[4] == 0
    assert all(du[j] != 0 for j in (0, 2, 3, 5, 6, 7)), du
    # forward clamps the outside values onto the bound
    out = lib.silu_mul_weighted(fc1, w, limit=limit)
    want = lib.silu_mul_weighted(_clamp_torch(fc1, leff), w)
    assert torch.equal(out, want)
    assert out[0, 0] == out[0, 1]
    assert torch.isfinite(dw).all()


@pytest.mark.parametrize("has_w", [True, False])
@pytest.mark.parametrize("rows,I", SHAPES)
def test_huge_limit_equals_unclamped(lib, rows, I, has_w):
    fc1, dy, w = _inputs(rows, I)
    w = w if has_w else None
    assert torch.equal(lib.silu_mul_weighted(fc1, w, limit=3e38),
                       lib.silu_mul_weighted(fc1, w))
    dfc1, dw = lib.silu_mul_weighted_bwd(dy, fc1, w, limit=3e38)
    dfc1_u, dw_u = lib.silu_mul_weighted_bwd(dy, fc1, w)
    assert torch.equal(dfc1, dfc1_u)
    if has_w:
        torch.testing.assert_close(dw, dw_u, rtol=1e-4, atol=1e-6)


def test_kernel_entry_rejects_bad_arguments(lib):
    fc1, _, w = _inputs(3, 520)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="limit"):
            lib.silu_mul_weighted(fc1, w, limit=bad)
    odd = bf(torch.randn(2, 2 * 12)).cuda()  # I = 12, not a multiple of 8
    with pytest.raises(RuntimeError, match="I % 8"):
        lib.silu_mul_weighted(odd, None, limit=L)


# ------------------------------------------------------------- function level
T, H, E, TOPK, I_MOE = 96, 128, 8, 2, 64
LIMIT = 0.25  # fc1 ~ N(0, 0.28) here: ~19 % of gate, ~37 % of up saturate
EMPTY_EXPERT = 5
NAMES = ("out", "d_hidden", "d_gate_up", "d_down", "d_top_w")


def _rel(x, ref):
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    return (torch.linalg.norm(x - ref) / torch.linalg.norm(ref)).item()


@pytest.fixture(scope="module")
def moe_case():
    """Inputs, the fp64 reference and the eager bf16 errors, computed once."""
    from veomni_amd.models.modeling import Experts, ModelConfig

    g = torch.Generator().manual_seed(8)
    gate_up = bf(torch.randn(E, 2 * I_MOE, H, generator=g) * 0.05)
    down = bf(torch.randn(E, H, I_MOE, generator=g) * 0.05)
    hidden = bf(torch.randn(T, H, generator=g) * 0.5)
    rw = torch.randn(T, E, generator=g)
    rw[:, EMPTY_EXPERT] = float("-inf")  # this expert gets no token
    top_w, top_i = torch.topk(torch.softmax(rw, -1), TOPK, -1)
    top_w = bf(top_w / top_w.sum(-1, keepdim=True))
    dy = bf(torch.randn(T, H, generator=g) * 0.1)
    assert (top_i == EMPTY_EXPERT).sum() == 0

    # fp64 restatement of the reference's merged-fc1 path with the clamp
    # (group_gemm.py: fc1 -> clamp gate / up -> silu(gate) * up -> * weight
    # -> fc2 -> sum over the routed slots), on the same bf16-valued inputs
    h64 = hidden.double().requires_grad_(True)
    gu64 = gate_up.double().requires_grad_(True)
    d64 = down.double().requires_grad_(True)
    w64 = top_w.double().requires_grad_(True)
    out64 = torch.zeros(T, H, dtype=torch.float64)
    sat_g, sat_u = [], []
    for k in range(TOPK):
        e = top_i[:, k]
        gate, up = torch.einsum("th,tfh->tf", h64, gu64[e]).chunk(2, dim=-1)
        sat_g.append(gate.detach() > LIMIT)
        sat_u.append(up.detach().abs() > LIMIT)
        act = F.silu(torch.clamp(gate, max=LIMIT)) * torch.clamp(up, min=-LIMIT, max=LIMIT)
        out64 = out64 + torch.einsum("ti,thi->th", act * w64[:, k, None], d64[e])
    out64.backward(dy.double())
    g_share = torch.cat(sat_g).float().mean().item()
    u_share = torch.cat(sat_u).float().mean().item()
    assert 0.10 <= g_share <= 0.90, g_share
    assert 0.10 <= u_share <= 0.90, u_share
    ref = dict(out=out64.detach(), d_hidden=h64.grad, d_gate_up=gu64.grad,
               d_down=d64.grad, d_top_w=w64.grad)

    # eager bf16 experts on the GPU: the error scale of a bf16 pipeline
    cfg = ModelConfig(hidden_size=H, num_experts=E, num_experts_per_tok=TOPK,
                      moe_intermediate_size=I_MOE, vocab_size=64, swiglu_limit=LIMIT)
    experts = Experts(cfg).cuda().to(torch.bfloat16)
    with torch.no_grad():
        experts.gate_up_proj.copy_(gate_up)
        experts.down_proj.copy_(down)
    h = hidden.cuda().requires_grad_(True)
    tw = top_w.cuda().requires_grad_(True)
    out = experts(h, top_i.cuda(), tw)
    out.backward(dy.cuda())
    eager = dict(out=out, d_hidden=h.grad, d_gate_up=experts.gate_up_proj.grad,
                 d_down=experts.down_proj.grad, d_top_w=tw.grad)
    err_eager = {n: _rel(eager[n], ref[n]) for n in NAMES}
    return dict(gate_up=gate_up.cuda(), down=down.cuda(), hidden=hidden.cuda(),
                top_w=top_w.cuda(), top_i=top_i.cuda(), dy=dy.cuda(), ref=ref,
                err_eager=err_eager)


def _leaves(c):
    return (c["hidden"].clone().requires_grad_(True),
            c["top_w"].clone().requires_grad_(True),
            c["gate_up"].clone().requires_grad_(True),
            c["down"].clone().requires_grad_(True))


def _check(name, c, got):
    """err_hip <= 2 * err_eager per tensor: both are bf16 pipelines with the
    same number of roundings, differing in operation order (routing weight
    before vs after fc2); 2 is the margin for that reordering."""
    for n in NAMES:
        e_hip, e_eager = _rel(got[n], c["ref"][n]), c["err_eager"][n]
        print(f"swiglu_limit parity {name:12s} {n:10s} err_hip {e_hip:.3e} "
              f"err_eager {e_eager:.3e} ratio {e_hip / e_eager:.2f}")
    for n in NAMES:
        e_hip, e_eager = _rel(got[n], c["ref"][n]), c["err_eager"][n]
        assert e_hip <= 2 * e_eager, (name, n, e_hip, e_eager)


def test_fused_function_merged_with_limit(moe_case):
    from veomni_amd.ops.kernels.moe import HipFusedMoeFunction

    c = moe_case
    h, tw, gu, dn = _leaves(c)
    out = HipFusedMoeFunction.apply(E, tw, c["top_i"], h, gu, dn, LIMIT)
    out.backward(c["dy"])
    _check("merged", c, dict(out=out, d_hidden=h.grad, d_gate_up=gu.grad,
                             d_down=dn.grad, d_top_w=tw.grad))


def test_fused_forward_split_weights_with_limit(moe_case):
    from veomni_amd.ops.kernels.moe import hip_fused_moe_forward

    c = moe_case
    h, tw, _, dn = _leaves(c)
    w1 = c["gate_up"][:, :I_MOE].clone().requires_grad_(True)
    w2 = c["gate_up"][:, I_MOE:].clone().requires_grad_(True)
    out = hip_fused_moe_forward(E, tw, c["top_i"], h, w1, w2, dn, None,
                                swiglu_limit=LIMIT)
    out.backward(c["dy"])
    _check("split", c, dict(out=out, d_hidden=h.grad,
                            d_gate_up=torch.cat([w1.grad, w2.grad], dim=1),
                            d_down=dn.grad, d_top_w=tw.grad))


def _ep_layout(c, h):
    """Single-rank EP bookkeeping around an expert class: expert-major
    permutation in, weighted fp32 unpermute out (the dispatch path with the
    all-to-all taken out)."""
    from veomni_amd.distributed.moe import permute

    routing_map = F.one_hot(c["top_i"], num_classes=E).permute(2, 1, 0).sum(dim=1)
    permuted, mapping = permute(h, routing_map)
    counts = routing_map.sum(dim=1)
    return routing_map, permuted, mapping, counts


def _ep_combine(c, y, tw, routing_map, mapping):
    from veomni_amd.distributed.moe import generate_weights_idx, unpermute

    return unpermute(y, generate_weights_idx(tw, c["top_i"], E),
                     c["hidden"].shape, mapping, routing_map)


def test_ep_class_with_limit(moe_case):
    from veomni_amd.ops.kernels.moe import EPMergedFc1HipGroupGemm

    c = moe_case
    h, tw, gu, dn = _leaves(c)
    routing_map, permuted, mapping, counts = _ep_layout(c, h)
    y = EPMergedFc1HipGroupGemm.apply(permuted, counts.cumsum(0), gu, dn, LIMIT)
    out = _ep_combine(c, y, tw, routing_map, mapping)
    out.backward(c["dy"])
    _check("ep", c, dict(out=out, d_hidden=h.grad, d_gate_up=gu.grad,
                         d_down=dn.grad, d_top_w=tw.grad))


def test_ep_a2a_class_with_limit_single_rank(moe_case):
    from veomni_amd.ops.kernels.moe import (EPMergedFc1HipGroupGemmA2A,
                                            ep_a2a_class_for_limit)

    cls = ep_a2a_class_for_limit(LIMIT)
    assert cls is ep_a2a_class_for_limit(LIMIT)
    assert cls is not EPMergedFc1HipGroupGemmA2A
    c = moe_case
    h, tw, gu, dn = _leaves(c)
    routing_map, permuted, mapping, counts = _ep_layout(c, h)
    y = cls.apply(permuted, counts.cumsum(0), None, (), (), counts.cpu(),
                  list(range(E)), gu, dn)
    out = _ep_combine(c, y, tw, routing_map, mapping)
    out.backward(c["dy"])
    _check("ep_a2a", c, dict(out=out, d_hidden=h.grad, d_gate_up=gu.grad,
                             d_down=dn.grad, d_top_w=tw.grad))


# ---------------------------------------------------------------- model level
# tiny-moe: normed hidden (rms 1) x N(0, 0.02) weights over H = 128 gives
# fc1 ~ N(0, 0.23); 0.125 is bf16-exact and saturates ~29 % of gate and
# ~58 % of up in layer 0 (checked below on the real activations)
MODEL_LIMIT = 0.125


@pytest.fixture
def _eager_after():
    yield
    from veomni_amd.models.modeling import bind_ops

    bind_ops("eager")


def _loss_and_gradnorm(model, batch):
    loss, _ = model(**batch)
    loss.backward()
    gn = torch.nn.utils.get_total_norm(
        [p.grad for p in model.parameters() if p.grad is not None])
    model.zero_grad(set_to_none=True)
    return float(loss), float(gn)


def _build(cfg):
    from veomni_amd.models.modeling import ForCausalLM

    with torch.device("cuda"):
        model = ForCausalLM(cfg)
    return model.to(torch.bfloat16)


def layer0_saturation(model, batch, limit):
    """Share of routed gate / up pre-activations beyond the limit in layer 0."""
    experts = model.model.layers[0].mlp.experts
    seen = {}

    def hook(mod, args):
        seen["hidden"], seen["top_i"] = args[0].detach(), args[1].detach()

    handle = experts.register_forward_pre_hook(hook)
    try:
        with torch.no_grad():
            model(**batch)
    finally:
        handle.remove()
    hidden, top_i = seen["hidden"].float(), seen["top_i"]
    gu = experts.gate_up_proj.detach().float()
    g_sat = u_sat = n = 0
    for k in range(top_i.shape[1]):
        gate, up = torch.einsum("th,tfh->tf", hidden, gu[top_i[:, k]]).chunk(2, dim=-1)
        g_sat += (gate > limit).sum().item()
        u_sat += (up.abs() > limit).sum().item()
        n += gate.numel()
    return g_sat / n, u_sat / n


def test_model_with_limit_hip_vs_eager(_eager_after):
    from veomni_amd.data import synthetic_batch
    from veomni_amd.models import PRESETS
    from veomni_amd.models.modeling import bind_ops
    from veomni_amd.ops import HIP_OPS_CONFIG

    cfg = dataclasses.replace(PRESETS["tiny-moe"], swiglu_limit=MODEL_LIMIT)
    batch = synthetic_batch(512, 256, seed=3, device="cuda")
    bind_ops("eager")
    model = _build(cfg)
    assert model.model.layers[0].mlp.experts.limit == MODEL_LIMIT
    g_share, u_share = layer0_saturation(model, batch, MODEL_LIMIT)
    assert 0.10 <= g_share <= 0.90, g_share
    assert 0.10 <= u_share <= 0.90, u_share
    l_eager, g_eager = _loss_and_gradnorm(model, batch)
    bind_ops(HIP_OPS_CONFIG)
    l_hip, g_hip = _loss_and_gradnorm(model, batch)
    # same assertions and tolerances as test_model_hip_vs_eager_gpu
    assert abs(l_hip - l_eager) / abs(l_eager) < 2e-2, (l_hip, l_eager)
    assert abs(g_hip - g_eager) / max(abs(g_eager), 1e-6) < 5e-2, (g_hip, g_eager)


def test_model_limit_none_equals_preset(_eager_after):
    from veomni_amd.data import synthetic_batch
    from veomni_amd.models import PRESETS, build_model
    from veomni_amd.models.modeling import bind_ops
    from veomni_amd.ops import HIP_OPS_CONFIG

    batch = synthetic_batch(512, 256, seed=3, device="cuda")
    bind_ops(HIP_OPS_CONFIG)

    def steady_loss(model):
        # The first HIP-bound forward of a freshly built model can differ
        # from every later one in the last bf16 bits (seen on the unmodified
        # preset too: 6.26659 once, then 6.269041538 on every repeat and in
        # every process). Compare the repeatable value: the second forward.
        with torch.no_grad():
            model(**batch)
            return float(model(**batch)[0])

    preset = build_model("tiny-moe", dtype=torch.bfloat16, device="cuda")
    same = _build(dataclasses.replace(PRESETS["tiny-moe"], swiglu_limit=None))
    limited = _build(dataclasses.replace(PRESETS["tiny-moe"], swiglu_limit=MODEL_LIMIT))
    l_preset = steady_loss(preset)
    assert steady_loss(same) == l_preset
    # and a limit does change the loss of this model
    assert steady_loss(limited) != l_preset
