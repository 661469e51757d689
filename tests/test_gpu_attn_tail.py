"""The causal flash pairs at sequence lengths that are no multiple of 256
(pytest -m gpu): head_dim 128 and 64 through hip_flash_attention, the
attention slot and a model.

Lengths: 8 (less than one wave and one kv tile: every block is a tail block),
257 (a second q block, a fifth dkv strip and a third dq block with one valid
row each), 333 (ragged for every tile size), 448 (ragged for 256 and 128, whole
64-row tiles). (B, Hq, Hkv) = (2, 4, 2), so a read past row S-1 lands in the
next head and an unmasked padded query row adds up to 255 terms to dK / dV.
Reference: fp32 torch autograd on the device from the same bf16 inputs (std
0.5), as _ref in tests/test_gpu_attn_d64.py; tolerances of
tests/test_gpu_attn_paths.py: output atol = 3e-2, each gradient (dsinks
included) max error < 0.06 * max(|ref|max, 1)."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B, HQ, HKV = 2, 4, 2
NAMES = ("out", "dq", "dk", "dv", "dsinks")


def _inputs(D, S, nb=B):
    g = torch.Generator().manual_seed(1000 * D + S)
    mk = lambda h: (torch.randn(nb, h, S, D, generator=g) * 0.5).to(torch.bfloat16).cuda()
    return mk(HQ), mk(HKV), mk(HKV), mk(HQ), torch.randn(HQ, generator=g).cuda()


def _ref(q, k, v, do, W=None, cu=None, sinks=None):
    """fp32 attention with autograd: key j is visible to query i iff j <= i,
    j > i - W and j is in i's document; optional sink column."""
    S, rep, scale = q.shape[2], q.shape[1] // k.shape[1], q.shape[-1] ** -0.5
    ar = torch.arange(S, device="cuda")
    lo = (ar - W + 1).clamp(min=0) if W is not None else torch.zeros_like(ar)
    for a, b in zip(cu[:-1], cu[1:]) if cu is not None else ():
        lo[a:b] = lo[a:b].clamp(min=a)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    sf = sinks.float().clone().requires_grad_(True) if sinks is not None else None
    sc = torch.matmul(qf, kf.repeat_interleave(rep, dim=1).transpose(-1, -2)) * scale
    allowed = (ar[None, :] <= ar[:, None]) & (ar[None, :] >= lo[:, None])
    sc = sc.masked_fill(~allowed, float("-inf"))
    if sf is not None:
        sc = torch.cat([sc, sf.reshape(1, -1, 1, 1).expand(q.shape[0], -1, S, 1)], dim=-1)
    p = torch.softmax(sc, dim=-1)
    if sf is not None:
        p = p[..., :-1]
    oref = torch.matmul(p, vf.repeat_interleave(rep, dim=1))
    oref.backward(do.float())
    return oref.detach(), qf.grad, kf.grad, vf.grad, sf.grad if sf is not None else None


def _hip(q, k, v, do, W=None, cu=None, sinks=None):
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens, hip_flash_attention

    S, ds, de = q.shape[2], None, None
    if cu is not None:
        ds, de = docs_from_cu_seqlens(torch.tensor(cu, dtype=torch.int32, device="cuda"), S)
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    if sinks is not None:
        sinks = sinks.detach().clone().requires_grad_(True)
    out = hip_flash_attention(q, k, v, q.shape[-1] ** -0.5, ds, de, sinks=sinks,
                              sliding_window=W)
    out.backward(do)
    return out.detach(), q.grad, k.grad, v.grad, (sinks.grad if sinks is not None else None)


def _check(got, ref, tag=""):
    for t, nm in zip(got, NAMES):
        assert t is None or torch.isfinite(t.float()).all(), f"{tag}{nm}: non-finite"
    print(f"{tag}out max err {(got[0].float() - ref[0]).abs().max().item():.3e}")
    torch.testing.assert_close(got[0].float(), ref[0].float(), rtol=0, atol=3e-2)
    for g, r, nm in zip(got[1:], ref[1:], NAMES[1:]):
        if r is None:
            assert g is None
            continue
        m = r.float().abs().max().item()
        err = (g.float() - r.float()).abs().max().item()
        print(f"{tag}{nm} max err {err:.3e} |ref|max {m:.3e}")
        assert err < 0.06 * max(m, 1.0), f"{tag}{nm}: max err {err} vs |ref|max {m}"


@pytest.mark.parametrize("case", ["plain", "docs", "window_sinks"])
@pytest.mark.parametrize("S", [8, 257, 333, 448])
@pytest.mark.parametrize("D", [128, 64])
def test_tail_pair_vs_autograd(D, S, case):
    q, k, v, do, sinks = _inputs(D, S, 1 if case == "docs" else B)
    kw = {"plain": {},
          "docs": dict(cu=[0, 100, S] if S > 100 else [0, 3, 8]),
          "window_sinks": dict(W=100 if S > 100 else 3, sinks=sinks)}[case]
    _check(_hip(q, k, v, do, **kw), _ref(q, k, v, do, **kw), tag=f"D{D} S{S} {case} ")


@pytest.mark.parametrize("D", [128, 64])
def test_tail_slot_dispatch(D):
    """hip_attention_forward at S = 333: the default core is hip_flash bit for
    bit, is not the sdpa core, and agrees with the reference."""
    from veomni_amd.ops.kernels.attention import hip_attention_forward

    q, k, v, do, _ = _inputs(D, 333)
    run = lambda **kw: hip_attention_forward(
        None, q, k, v, None, scaling=D ** -0.5, **kw)[0].transpose(1, 2)
    flash, sdpa, default = run(core="hip_flash"), run(core="sdpa"), run()
    assert torch.equal(default, flash), "default core is not hip_flash"
    assert not torch.equal(default, sdpa), "default core is the sdpa core"
    torch.testing.assert_close(default.float(), _ref(q, k, v, do)[0], rtol=0, atol=3e-2)


@pytest.mark.parametrize("D", [128, 64])
def test_tail_reproducible(D):
    q, k, v, do, sinks = _inputs(D, 333)
    a = _hip(q, k, v, do, W=100, sinks=sinks)
    b = _hip(q, k, v, do, W=100, sinks=sinks)
    for x, y, nm in zip(a, b, NAMES):
        assert torch.equal(x, y), f"{nm} differs between two runs"


def test_tail_model_vs_eager():
    """tiny-d128-swa on one packed batch of S = 333, all HIP ops against eager
    attention, with the comparison and bounds of
    test_model_window_sinks_vs_eager (tests/test_gpu_attn_window_sinks.py)."""
    from veomni_amd.models import build_model
    from veomni_amd.models.modeling import bind_ops
    from veomni_amd.ops import HIP_OPS_CONFIG

    S = 333
    torch.manual_seed(3)
    model = build_model("tiny-d128-swa", dtype=torch.bfloat16, device="cuda")
    cu = torch.tensor([0, 150, 280, S], dtype=torch.int32, device="cuda")
    ids = torch.randint(0, model.config.vocab_size, (1, S), device="cuda")
    pos = torch.cat([torch.arange(int(cu[i + 1]) - int(cu[i]), device="cuda")
                     for i in range(cu.numel() - 1)])[None]
    sink_params = [l.self_attn.sinks for l in model.model.layers]
    res = {}
    try:
        bind_ops("eager")
        m32 = copy.deepcopy(model).float()
        loss, _ = m32(ids, labels=ids, position_ids=pos, cu_seq_lens_q=cu)
        loss.backward()
        res["fp32", "sinks"] = [l.self_attn.sinks.grad.clone() for l in m32.model.layers]
        for name, impl in (("eager", "eager"),
                           ("rest", dict(HIP_OPS_CONFIG, attention="eager")),
                           ("hip", HIP_OPS_CONFIG)):
            bind_ops(impl)
            model.eval()
            with torch.no_grad():
                res[name, "logits"], _ = model(ids, position_ids=pos, cu_seq_lens_q=cu)
            model.train()
            model.zero_grad(set_to_none=True)
            loss, _ = model(ids, labels=ids, position_ids=pos, cu_seq_lens_q=cu)
            loss.backward()
            res[name, "sinks"] = [p.grad.float().clone() for p in sink_params]
    finally:
        bind_ops("eager")
    torch.testing.assert_close(res["hip", "logits"].float(), res["rest", "logits"].float(),
                               rtol=5e-2, atol=5e-1)
    for i, r in enumerate(res["fp32", "sinks"]):
        g = res["hip", "sinks"][i]
        err = {n: (res[n, "sinks"][i] - r).abs().max().item()
               for n in ("eager", "rest", "hip")}
        print(f"layer {i} sinks.grad |fp32|max {r.abs().max().item():.3e} err {err}")
        assert torch.isfinite(g).all() and g.abs().max().item() > 0
        assert err["hip"] <= 2 * max(err["rest"], err["eager"]), f"layer {i}: {err}"
