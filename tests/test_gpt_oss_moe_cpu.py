"""gpt-oss experts (OpSlot moe_experts/gpt_oss) on CPU: registration, config
and preset plumbing, the eager GptOssExperts / GptOssTopKRouter against a
golden recorded from the reference (tests/golden/make_gpt_oss_moe_golden.py),
an fp64 gradcheck, the argument validation of the HIP entry point (it runs
before any device work) and eager EP on gloo."""

import dataclasses
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "gpt_oss_moe_golden.pt")
PARAMS = ("gate_up_proj", "gate_up_proj_bias", "down_proj", "down_proj_bias")

# the fp32 tolerances tests/test_attn_window_sinks_cpu.py takes from
# tests/test_logprobs_cpu.py
FWD_TOL = dict(rtol=2e-5, atol=1e-6)
GRAD_TOL = dict(rtol=2e-5, atol=3e-5)


def _cfg(E, H, I, topk, limit=7.0, **kw):
    from veomni_amd.models.modeling import ModelConfig

    return ModelConfig(hidden_size=H, num_experts=E, num_experts_per_tok=topk,
                       moe_intermediate_size=I, vocab_size=64,
                       expert_style="gpt_oss", swiglu_limit=limit, **kw)


def _experts(cfg, weights, dtype=torch.float32):
    from veomni_amd.models.modeling import GptOssExperts

    m = GptOssExperts(cfg)
    for p in PARAMS:  # replaced, not copied: an EP rank holds a slice of the bank
        setattr(m, p, torch.nn.Parameter(weights[p].clone().to(dtype)))
    return m


# ---------------------------------------------------------------- registration
def test_hip_gpt_oss_variant_registered():
    import veomni_amd.ops  # noqa: F401
    from veomni_amd.ops.kernel_registry import KERNEL_REGISTRY

    assert "hip" in KERNEL_REGISTRY.list_available("moe_experts", "gpt_oss")
    assert "hip" in KERNEL_REGISTRY.list_available("moe_experts", "standard")


def test_bind_ops_binds_both_expert_slots():
    from veomni_amd.models import modeling

    slot = modeling.veomni_gpt_oss_moe_experts_forward
    assert (slot.op_name, slot.variant) == ("moe_experts", "gpt_oss")
    modeling.bind_ops("eager")
    assert slot.use_eager_impl and not slot.use_non_eager_impl
    modeling.bind_ops({"moe_experts": "eager"})
    assert slot.use_eager_impl
    assert modeling.veomni_moe_experts_forward.use_eager_impl


# ---------------------------------------------------------------------- config
def test_config_validation():
    from veomni_amd.models.modeling import ModelConfig

    assert ModelConfig().expert_style == "standard"
    assert ModelConfig().swiglu_alpha == 1.702
    with pytest.raises(ValueError, match="expert_style"):
        ModelConfig(expert_style="quack")
    with pytest.raises(ValueError, match="swiglu_limit"):
        ModelConfig(expert_style="gpt_oss")
    cfg = ModelConfig(expert_style="gpt_oss", swiglu_limit=7.0)
    assert cfg.expert_style == "gpt_oss"


def test_preset_builds_with_gpt_oss_modules():
    from veomni_amd.models import PRESETS, build_model
    from veomni_amd.models.modeling import GptOssExperts, GptOssTopKRouter

    cfg = PRESETS["tiny-gpt-oss-moe"]
    tiny = PRESETS["tiny-moe"]
    assert cfg.expert_style == "gpt_oss" and cfg.swiglu_limit == 7.0
    assert cfg.swiglu_alpha == 1.702 and not cfg.qk_norm
    assert cfg.sliding_window is None and not cfg.attention_sinks
    for f in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers",
              "num_attention_heads", "num_key_value_heads", "head_dim",
              "num_experts", "num_experts_per_tok", "moe_intermediate_size"):
        assert getattr(cfg, f) == getattr(tiny, f), f
    model = build_model("tiny-gpt-oss-moe")
    E, H, I = cfg.num_experts, cfg.hidden_size, cfg.moe_intermediate_size
    sd = model.state_dict()
    for layer in range(cfg.num_hidden_layers):
        mlp = model.model.layers[layer].mlp
        assert isinstance(mlp.experts, GptOssExperts)
        assert isinstance(mlp.gate, GptOssTopKRouter)
        assert mlp.experts.alpha == 1.702 and mlp.experts.limit == 7.0
        pre = f"model.layers.{layer}.mlp."
        assert sd[pre + "experts.gate_up_proj"].shape == (E, H, 2 * I)
        assert sd[pre + "experts.gate_up_proj_bias"].shape == (E, 2 * I)
        assert sd[pre + "experts.down_proj"].shape == (E, I, H)
        assert sd[pre + "experts.down_proj_bias"].shape == (E, H)
        assert sd[pre + "gate.weight"].shape == (E, H)
        assert sd[pre + "gate.bias"].shape == (E,)
        # biases start at zero (HF _init_weights), weights do not
        for b in ("experts.gate_up_proj_bias", "experts.down_proj_bias", "gate.bias"):
            assert torch.count_nonzero(sd[pre + b]) == 0, b
        for w in ("experts.gate_up_proj", "experts.down_proj", "gate.weight"):
            assert torch.count_nonzero(sd[pre + w]) > 0, w
    plan = model.get_parallel_plan().extra_parallel_plan["ep"]
    for p in PARAMS:
        assert f"model.layers.*.mlp.experts.{p}" in plan, p
    # one tiny eager step runs end to end
    from veomni_amd.data import synthetic_batch
    from veomni_amd.models.modeling import bind_ops

    bind_ops("eager")
    loss, aux = model(**synthetic_batch(cfg.vocab_size, 32, seed=1))
    loss.backward()
    assert torch.isfinite(loss) and aux is not None
    assert model.model.layers[0].mlp.experts.gate_up_proj_bias.grad is not None


# state_dict keys of tiny-moe's first layer MoE block, as they have always been
TINY_MOE_MLP_KEYS = {"experts.gate_up_proj", "experts.down_proj", "gate.weight"}


def test_existing_presets_are_standard_and_unchanged():
    from veomni_amd.models import PRESETS, build_model
    from veomni_amd.models.modeling import Experts, TopKRouter

    for name, cfg in PRESETS.items():
        if name != "tiny-gpt-oss-moe":
            assert cfg.expert_style == "standard", name
    model = build_model("tiny-moe")
    pre = "model.layers.0.mlp."
    keys = {k[len(pre):] for k in model.state_dict() if k.startswith(pre)}
    assert keys == TINY_MOE_MLP_KEYS
    assert isinstance(model.model.layers[0].mlp.experts, Experts)
    assert isinstance(model.model.layers[0].mlp.gate, TopKRouter)
    assert not any(k.endswith("_bias") for k in model.state_dict())
    plan = model.get_parallel_plan().extra_parallel_plan["ep"]
    assert set(plan) == {"model.layers.*.mlp.experts.gate_up_proj",
                         "model.layers.*.mlp.experts.down_proj"}
    # the same parameters as an explicitly standard config, bit for bit
    same = dataclasses.replace(PRESETS["tiny-moe"], expert_style="standard")
    from veomni_amd.models.modeling import ForCausalLM

    other = ForCausalLM(same).state_dict()
    for k, v in model.state_dict().items():
        assert torch.equal(v, other[k]), k


# ---------------------------------------------------------------------- golden
@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


def _routed_saturation(gd, limit):
    hidden, idx = gd["in/hidden"], gd["router/indices"]
    sat_g = sat_u = n = 0
    for k in range(idx.shape[1]):
        e = idx[:, k]
        gu = torch.einsum("th,thf->tf", hidden, gd["in/gate_up_proj"][e]) \
            + gd["in/gate_up_proj_bias"][e]
        sat_g += (gu[:, ::2] > limit).sum().item()
        sat_u += (gu[:, 1::2].abs() > limit).sum().item()
        n += gu[:, ::2].numel()
    return sat_g / n, sat_u / n


@pytest.mark.parametrize("case", ["limit_1p5", "limit_default"])
def test_eager_experts_match_reference_golden(golden, case):
    gd = golden
    limit = float(gd[f"case/{case}/limit"])
    E, H, twoI = gd["in/gate_up_proj"].shape
    topk = gd["router/indices"].shape[1]
    cfg = _cfg(E, H, twoI // 2, topk, limit=limit,
               swiglu_alpha=float(gd[f"case/{case}/alpha"]))
    m = _experts(cfg, {p: gd[f"in/{p}"] for p in PARAMS})
    assert m.limit == limit
    g_share, u_share = _routed_saturation(gd, limit)
    if case == "limit_1p5":
        assert 0.10 <= g_share <= 0.90, g_share
        assert 0.10 <= u_share <= 0.90, u_share
    else:
        assert g_share < 0.01 and u_share < 0.01
    assert (gd["router/indices"] == 2).sum() == 0  # an expert without tokens
    hidden = gd["in/hidden"].clone().requires_grad_(True)
    rw = gd["router/scores"].clone().requires_grad_(True)
    out = m(hidden, gd["router/indices"], rw)
    out.backward(gd["in/dy"])
    torch.testing.assert_close(out, gd[f"case/{case}/out"], **FWD_TOL)
    torch.testing.assert_close(hidden.grad, gd[f"case/{case}/d_hidden"], **GRAD_TOL)
    torch.testing.assert_close(rw.grad, gd[f"case/{case}/d_routing_weights"], **GRAD_TOL)
    for p in PARAMS:
        torch.testing.assert_close(getattr(m, p).grad, gd[f"case/{case}/d_{p}"],
                                   **GRAD_TOL)


def test_cases_differ(golden):
    """The clamp is what separates the two golden cases."""
    assert not torch.allclose(golden["case/limit_1p5/out"],
                              golden["case/limit_default/out"], rtol=1e-2, atol=1e-3)


def test_eager_router_matches_reference_golden(golden):
    from veomni_amd.models.modeling import GptOssTopKRouter

    gd = golden
    E, H = gd["in/router_weight"].shape
    r = GptOssTopKRouter(_cfg(E, H, 8, gd["router/indices"].shape[1]))
    with torch.no_grad():
        r.weight.copy_(gd["in/router_weight"])
        r.bias.copy_(gd["in/router_bias"])
        logits, scores, idx = r(gd["in/hidden"])
    assert torch.equal(idx, gd["router/indices"])
    torch.testing.assert_close(logits, gd["router/logits"], **FWD_TOL)
    torch.testing.assert_close(scores, gd["router/scores"], **FWD_TOL)
    assert scores.dtype == logits.dtype
    torch.testing.assert_close(scores.sum(-1), torch.ones(scores.shape[0]))


# ------------------------------------------------------------------- gradcheck
def test_eager_experts_gradcheck_fp64():
    E, H, I, topk, T = 3, 8, 4, 2, 5
    g = torch.Generator().manual_seed(3)
    # |pre-activation| stays well inside the limit: gradcheck's finite
    # differences must not straddle a clamp bound
    w = {"gate_up_proj": torch.randn(E, H, 2 * I, generator=g, dtype=torch.float64) * 0.2,
         "gate_up_proj_bias": torch.randn(E, 2 * I, generator=g, dtype=torch.float64) * 0.2,
         "down_proj": torch.randn(E, I, H, generator=g, dtype=torch.float64) * 0.2,
         "down_proj_bias": torch.randn(E, H, generator=g, dtype=torch.float64) * 0.2}
    hidden = torch.randn(T, H, generator=g, dtype=torch.float64)
    idx = torch.stack([torch.arange(T) % E, (torch.arange(T) + 1) % E], dim=1)
    rw = torch.softmax(torch.randn(T, topk, generator=g, dtype=torch.float64), -1)
    m = _experts(_cfg(E, H, I, topk, limit=7.0), w, dtype=torch.float64)
    with torch.no_grad():
        gu = torch.einsum("th,ehf->tef", hidden, w["gate_up_proj"]) + w["gate_up_proj_bias"]
    assert gu.abs().max() < 6.0

    def fn(h, r, a, b, c, d):
        return torch.func.functional_call(
            m, dict(zip(PARAMS, (a, b, c, d))), (h, idx, r))

    leaves = [t.clone().requires_grad_(True)
              for t in (hidden, rw, *(w[p] for p in PARAMS))]
    assert torch.autograd.gradcheck(fn, leaves)


# ------------------------------------------------------------------ validation
def _call_entry(**override):
    from veomni_amd.ops.kernels.moe import hip_gpt_oss_fused_moe_forward

    E, H, I, topk, T = 4, 64, 32, 2, 8
    g = torch.Generator().manual_seed(2)
    dev = "cuda" if torch.cuda.is_available() else "cpu"

    def bf(*shape):
        return (torch.randn(*shape, generator=g) * 0.1).to(torch.bfloat16).to(dev)

    args = dict(
        num_experts=E,
        routing_weights=torch.full((T, topk), 0.5, dtype=torch.bfloat16, device=dev),
        selected_experts=torch.stack([torch.arange(T) % E, (torch.arange(T) + 1) % E], 1).to(dev),
        hidden_states=bf(T, H), gate_up_proj=bf(E, H, 2 * I),
        gate_up_proj_bias=bf(E, 2 * I), down_proj=bf(E, I, H),
        down_proj_bias=bf(E, H))
    for k, v in override.items():
        args[k] = v(args) if callable(v) else v
    return hip_gpt_oss_fused_moe_forward(**args)


@pytest.mark.parametrize("bad", [None, 0, -1.0, float("inf"), float("nan"), True])
def test_entry_rejects_bad_limit(bad):
    with pytest.raises(ValueError, match="swiglu_limit"):
        _call_entry(limit=bad)


@pytest.mark.parametrize("bad", [float("inf"), float("nan"), None, "x"])
def test_entry_rejects_bad_alpha(bad):
    with pytest.raises(ValueError, match="alpha"):
        _call_entry(alpha=bad)


@pytest.mark.parametrize("name,shape", [
    ("gate_up_proj", (4, 128, 64)),      # [E, 2I, H]: the standard bank's layout
    ("gate_up_proj", (4, 64, 63)),       # odd last dim
    ("gate_up_proj_bias", (4, 32)),
    ("down_proj", (4, 64, 32)),          # [E, H, I]
    ("down_proj_bias", (4, 32)),
    ("down_proj_bias", (3, 64)),
])
def test_entry_rejects_bad_shapes(name, shape):
    with pytest.raises(ValueError, match=name):
        _call_entry(**{name: lambda a: torch.zeros(shape, dtype=torch.bfloat16,
                                                   device=a["hidden_states"].device)})


def test_entry_accepts_valid_arguments():
    """Valid arguments pass validation and reach the device path. Without a
    GPU that path fails in the HIP library, which is all this can see here;
    it must not be a ValueError."""
    if torch.cuda.is_available():
        assert torch.isfinite(_call_entry().float()).all()
        return
    try:
        _call_entry()
    except ValueError as e:
        raise AssertionError(f"valid gpt-oss arguments rejected: {e!r}")
    except Exception:
        pass


def test_ep_a2a_class_cached_by_alpha_and_limit():
    from veomni_amd.ops.kernels import moe

    a = moe.gpt_oss_ep_a2a_class(1.702, 7.0)
    assert a is moe.gpt_oss_ep_a2a_class(1.702, 7.0)
    assert a is not moe.gpt_oss_ep_a2a_class(1.702, 1.5)
    assert a is not moe.gpt_oss_ep_a2a_class(1.0, 7.0)
    assert a is not moe.EPMergedFc1HipGroupGemmA2A


# ------------------------------------------------------- eager under EP (gloo)
WORLD = 2
EP_E, EP_TOPK, EP_T, EP_H, EP_I = 8, 2, 48, 32, 24
EP_LIMIT = 0.75
# the tolerance tests/test_dist_cpu.py uses for EP dispatch vs a local loop
EP_TOL = dict(rtol=1e-4, atol=1e-5)


def _ep_weights():
    g = torch.Generator().manual_seed(5)
    return {"gate_up_proj": torch.randn(EP_E, EP_H, 2 * EP_I, generator=g) * 0.1,
            "gate_up_proj_bias": torch.randn(EP_E, 2 * EP_I, generator=g) * 0.5,
            "down_proj": torch.randn(EP_E, EP_I, EP_H, generator=g) * 0.1,
            "down_proj_bias": torch.randn(EP_E, EP_H, generator=g) * 0.5}


def _ep_tokens(seed):
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(EP_T, EP_H, generator=g)
    sel = torch.randint(0, EP_E, (EP_T, EP_TOPK), generator=g)
    sel[:, 1] = (sel[:, 0] + 1) % EP_E  # distinct experts per token
    rw = torch.softmax(torch.randn(EP_T, EP_TOPK, generator=g), -1)
    dy = torch.randn(EP_T, EP_H, generator=g)
    return hidden, sel, rw, dy


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run(rank, world_size, fn, port):
    from veomni_amd.distributed.parallel_state import set_parallel_state

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        fn(rank, world_size)
    finally:
        set_parallel_state(None)
        dist.destroy_process_group()


def _ep_eager_gpt_oss(rank, ws):
    from veomni_amd.distributed.parallel_state import (init_parallel_state,
                                                       set_parallel_state)
    from veomni_amd.models.modeling import bind_ops

    bind_ops("eager")
    w = _ep_weights()
    local_e = EP_E // ws
    lo, hi = rank * local_e, (rank + 1) * local_e
    cfg = _cfg(EP_E, EP_H, EP_I, EP_TOPK, limit=EP_LIMIT)

    # non-EP expectation: the full bank on every rank's tokens; the local
    # experts' parameter grads collect contributions from all ranks' tokens
    set_parallel_state(None)
    ref = _experts(cfg, w)
    for rr in range(ws):
        hidden, sel, rw, dy = _ep_tokens(100 + rr)
        h_r = hidden.clone().requires_grad_(True)
        w_r = rw.clone().requires_grad_(True)
        out_r = ref(h_r, sel, w_r)
        (out_r * dy).sum().backward()
        if rr == rank:
            exp_out, exp_dh, exp_dw = out_r.detach(), h_r.grad, w_r.grad

    init_parallel_state(ep_size=ws)
    m = _experts(cfg, {p: v[lo:hi] for p, v in w.items()})
    m.num_experts = EP_E  # the module keeps the GLOBAL count; its bank is local
    hidden, sel, rw, dy = _ep_tokens(100 + rank)
    h = hidden.clone().requires_grad_(True)
    tw = rw.clone().requires_grad_(True)
    out = m(h, sel, tw)
    (out * dy).sum().backward()

    torch.testing.assert_close(out, exp_out, **EP_TOL)
    torch.testing.assert_close(h.grad, exp_dh, **EP_TOL)
    torch.testing.assert_close(tw.grad, exp_dw, **EP_TOL)
    for p in PARAMS:
        torch.testing.assert_close(getattr(m, p).grad, getattr(ref, p).grad[lo:hi],
                                   **EP_TOL)
    # the limit reached the EP expert compute: with another one the output differs
    other = _experts(dataclasses.replace(cfg, swiglu_limit=7.0),
                     {p: v[lo:hi] for p, v in w.items()})
    other.num_experts = EP_E
    with torch.no_grad():
        plain = other(hidden, sel, rw)
    assert not torch.allclose(plain, exp_out, rtol=1e-2, atol=1e-3)


def test_eager_gpt_oss_under_ep_matches_non_ep():
    mp.spawn(_run, args=(WORLD, _ep_eager_gpt_oss, _free_port()), nprocs=WORLD,
             join=True)
