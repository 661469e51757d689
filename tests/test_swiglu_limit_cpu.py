"""Clamped SwiGLU (`swiglu_limit`) on CPU: config plumbing, the eager
experts paths (plain and under gloo EP) against an fp32 restatement built
from torch.clamp + F.silu autograd, and the limit validation of the HIP
entry point (which needs no GPU: it runs before any device work)."""

import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from oracle import moe as oracle_moe

E, TOPK, T, H, I = 8, 2, 48, 32, 24
LIMIT = 0.25  # bf16-representable; fc1 ~ N(0, 0.57) below, so it bites

# fp32 tolerances of tests/test_model_parity_cpu.py (logits / grads)
FWD_TOL = dict(rtol=2e-5, atol=2e-5)
GRAD_TOL = dict(rtol=1e-4, atol=1e-6)


def _weights():
    g = torch.Generator().manual_seed(5)
    gate_up = torch.randn(E, 2 * I, H, generator=g) * 0.1
    down = torch.randn(E, H, I, generator=g) * 0.1
    return gate_up, down


def _tokens(seed):
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(T, H, generator=g)
    sel = torch.randint(0, E, (T, TOPK), generator=g)
    sel[:, 1] = (sel[:, 0] + 1) % E  # distinct experts per token
    rw = torch.softmax(torch.randn(T, TOPK, generator=g), -1)
    dy = torch.randn(T, H, generator=g)
    return hidden, sel, rw, dy


def _experts(limit, gate_up, down):
    from veomni_amd.models.modeling import Experts, ModelConfig

    cfg = ModelConfig(hidden_size=H, num_experts=E, num_experts_per_tok=TOPK,
                      moe_intermediate_size=I, vocab_size=64, swiglu_limit=limit)
    m = Experts(cfg)
    m.gate_up_proj = torch.nn.Parameter(gate_up.clone())
    m.down_proj = torch.nn.Parameter(down.clone())
    return m


def _ref_clamped_moe(hidden, sel, rw, gate_up, down, limit):
    """The reference's clamped-SwiGLU experts math, restated: per routed
    (token, slot) pair  y = (silu(clamp(g, max=L)) * clamp(u, -L, L)) @ down^T,
    weighted after the down projection. Returns (out, gate_raw, up_raw)."""
    out = torch.zeros_like(hidden)
    gates, ups = [], []
    for k in range(sel.shape[1]):
        e = sel[:, k]
        gu = torch.einsum("th,tfh->tf", hidden, gate_up[e])
        gate, up = gu.chunk(2, dim=-1)
        gates.append(gate.detach())
        ups.append(up.detach())
        h = F.silu(torch.clamp(gate, max=limit)) * torch.clamp(up, min=-limit, max=limit)
        y = torch.einsum("ti,thi->th", h, down[e])
        out = out + y * rw[:, k, None]
    return out, torch.cat(gates), torch.cat(ups)


def _assert_bites(gate_raw, up_raw, limit):
    g_share = (gate_raw > limit).float().mean().item()
    u_share = (up_raw.abs() > limit).float().mean().item()
    assert 0.10 <= g_share <= 0.90, g_share
    assert 0.10 <= u_share <= 0.90, u_share


def test_config_sets_experts_limit():
    from veomni_amd.models.modeling import Experts, ModelConfig

    base = dict(hidden_size=H, num_experts=E, num_experts_per_tok=TOPK,
                moe_intermediate_size=I, vocab_size=64)
    assert ModelConfig().swiglu_limit is None
    assert Experts(ModelConfig(**base)).limit is None
    assert Experts(ModelConfig(swiglu_limit=7.0, **base)).limit == 7.0


def test_eager_limit_matches_clamp_autograd():
    gate_up, down = _weights()
    hidden, sel, rw, dy = _tokens(100)

    m = _experts(LIMIT, gate_up, down)
    h1 = hidden.clone().requires_grad_(True)
    w1 = rw.clone().requires_grad_(True)
    out = m(h1, sel, w1)
    (out * dy).sum().backward()

    h2 = hidden.clone().requires_grad_(True)
    w2 = rw.clone().requires_grad_(True)
    gu2 = gate_up.clone().requires_grad_(True)
    d2 = down.clone().requires_grad_(True)
    ref, gate_raw, up_raw = _ref_clamped_moe(h2, sel, w2, gu2, d2, LIMIT)
    (ref * dy).sum().backward()

    _assert_bites(gate_raw, up_raw, LIMIT)
    torch.testing.assert_close(out, ref, **FWD_TOL)
    torch.testing.assert_close(h1.grad, h2.grad, **GRAD_TOL)
    torch.testing.assert_close(w1.grad, w2.grad, **GRAD_TOL)
    torch.testing.assert_close(m.gate_up_proj.grad, gu2.grad, **GRAD_TOL)
    torch.testing.assert_close(m.down_proj.grad, d2.grad, **GRAD_TOL)
    # and the clamp is what made the difference
    with torch.no_grad():
        plain = _experts(None, gate_up, down)(hidden, sel, rw)
    assert not torch.allclose(plain, ref.detach(), rtol=1e-2, atol=1e-3)


def test_no_limit_is_bit_equal_to_oracle():
    gate_up, down = _weights()
    hidden, sel, rw, _ = _tokens(100)
    m = _experts(None, gate_up, down)
    with torch.no_grad():
        out = m(hidden, sel, rw)
        ref = oracle_moe.eager_moe_forward(hidden, sel, rw, gate_up, down)
    assert torch.equal(out, ref)


# ------------------------------------------------------- eager under EP (gloo)
WORLD = 2
# the tolerance tests/test_dist_cpu.py uses for EP dispatch vs a local loop
EP_TOL = dict(rtol=1e-4, atol=1e-5)


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


def _ep_eager_limit(rank, ws):
    from veomni_amd.distributed.parallel_state import (init_parallel_state,
                                                       set_parallel_state)

    gate_up, down = _weights()
    local_e = E // ws
    lo, hi = rank * local_e, (rank + 1) * local_e

    # non-EP expectation: the full bank on every rank's tokens; the local
    # experts' weight grads collect contributions from all ranks' tokens
    set_parallel_state(None)
    ref = _experts(LIMIT, gate_up, down)
    for rr in range(ws):
        hidden, sel, rw, dy = _tokens(100 + rr)
        h_r = hidden.clone().requires_grad_(True)
        w_r = rw.clone().requires_grad_(True)
        out_r = ref(h_r, sel, w_r)
        (out_r * dy).sum().backward()
        if rr == rank:
            exp_out, exp_dh, exp_dw = out_r.detach(), h_r.grad, w_r.grad

    init_parallel_state(ep_size=ws)
    m = _experts(LIMIT, gate_up[lo:hi], down[lo:hi])
    hidden, sel, rw, dy = _tokens(100 + rank)
    h = hidden.clone().requires_grad_(True)
    w = rw.clone().requires_grad_(True)
    out = m(h, sel, w)
    (out * dy).sum().backward()

    torch.testing.assert_close(out, exp_out, **EP_TOL)
    torch.testing.assert_close(h.grad, exp_dh, **EP_TOL)
    torch.testing.assert_close(w.grad, exp_dw, **EP_TOL)
    torch.testing.assert_close(m.gate_up_proj.grad, ref.gate_up_proj.grad[lo:hi], **EP_TOL)
    torch.testing.assert_close(m.down_proj.grad, ref.down_proj.grad[lo:hi], **EP_TOL)
    # the limit reached the EP expert compute: without it the output differs
    with torch.no_grad():
        plain = _experts(None, gate_up[lo:hi], down[lo:hi])(hidden, sel, rw)
    assert not torch.allclose(plain, exp_out, rtol=1e-2, atol=1e-3)


def test_eager_limit_under_ep_matches_non_ep():
    mp.spawn(_run, args=(WORLD, _ep_eager_limit, _free_port()), nprocs=WORLD,
             join=True)


# ------------------------------------------------------ overlapped EP class cache
def test_ep_a2a_class_cached_by_limit():
    from veomni_amd.ops.kernels import moe

    assert moe.ep_a2a_class_for_limit(None) is moe.EPMergedFc1HipGroupGemmA2A
    a = moe.ep_a2a_class_for_limit(0.25)
    assert a is moe.ep_a2a_class_for_limit(0.25)
    assert a is not moe.EPMergedFc1HipGroupGemmA2A
    assert a is not moe.ep_a2a_class_for_limit(7.0)


# ------------------------------------------------------------ limit validation
def _call_hip_entry(limit):
    from veomni_amd.ops.kernels.moe import hip_fused_moe_forward

    gate_up, down = _weights()
    hidden, sel, rw, _ = _tokens(100)
    # device tensors where there is a device: the kernels must never be
    # handed host pointers
    dev = "cuda" if torch.cuda.is_available() else "cpu"

    def bf(x):
        return x.to(torch.bfloat16).to(dev)

    return hip_fused_moe_forward(E, bf(rw), sel.to(dev), bf(hidden), None, None,
                                 bf(down), bf(gate_up), swiglu_limit=limit)


@pytest.mark.parametrize("bad", [0, -1, float("inf"), float("nan")])
def test_hip_entry_rejects_bad_limit(bad):
    with pytest.raises(ValueError, match="swiglu_limit"):
        _call_hip_entry(bad)


def test_hip_entry_accepts_valid_limit():
    """A valid limit passes validation and reaches the device path. Without
    a GPU that path fails in the HIP library, which is all this can see
    here; it must not be the old NotImplementedError nor a ValueError."""
    if torch.cuda.is_available():
        assert torch.isfinite(_call_hip_entry(LIMIT).float()).all()
        return
    try:
        _call_hip_entry(LIMIT)
    except (NotImplementedError, ValueError) as e:
        raise AssertionError(f"valid swiglu_limit rejected: {e!r}")
    except Exception:
        pass
