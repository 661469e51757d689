"""The head_dim 64 HIP flash pair (pytest -m gpu): kernels through the
autograd function, the attention slot and a model.

Shapes: D = 64, bf16, (B, Hq, Hkv) = (2, 4, 2), S = 512: the smallest length
with a second 256-row q block, hence with forward tile skipping, and with
more than one dq block and dkv strip. Reference: fp32 torch autograd on the
device from the same bf16 inputs, built as _ref in
tests/test_gpu_attn_window_sinks.py is, with that file's tolerances: output
atol = 3e-2; each gradient (dsinks included) max error < 0.06 * max(|ref|max,
1).

LSE bound (against an fp64 logsumexp of the same scores, sink included):
LSE = ln2 * (m + log2(l)). The scores are fp32 MFMA sums of exact bf16
products, scaled into the exp2 domain with one rounding: absolute error
<= 2 ulp(|s| log2e) <= 2 * 2^-18 for |s| log2e < 64 (the dominant sink, 30,
is 43.3). Each of the <= 513 terms of l then carries that as a relative
error of ln2 * 2^-17 plus one ulp of v_exp_f32; the fp32 sum of n terms adds
at most n * 2^-24 = 3.1e-5. m, log2(l) and the final product add three more
roundings of a value below 64 (3 * 2^-18 * ln2). Total < 6e-5; the test
allows 1e-4."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 64
SCALE = 1.0 / 8
B, HQ, HKV, S = 2, 4, 2, 512
PACKED = [0, 70, 256, 300, 512]


@pytest.fixture(scope="module")
def data():
    """One set of inputs for the whole module (never modified)."""
    g = torch.Generator().manual_seed(64)
    mk = lambda h: (torch.randn(B, h, S, D, generator=g) * 0.5).to(torch.bfloat16).cuda()
    q, k, v, do = mk(HQ), mk(HKV), mk(HKV), mk(HQ)
    sinks = torch.randn(HQ, generator=g).cuda()
    return q, k, v, do, sinks


def _ref(q, k, v, do, W=None, cu=None, sinks=None):
    """fp32 attention with autograd: key j is visible to query i iff j <= i,
    j > i - W and j is in i's document; optional sink column. Returns (out,
    dq, dk, dv, dsinks | None, lse fp64)."""
    rep = q.shape[1] // k.shape[1]
    ar = torch.arange(S, device="cuda")
    lo = (ar - W + 1).clamp(min=0) if W is not None else torch.zeros_like(ar)
    for a, b in zip(cu[:-1], cu[1:]) if cu is not None else ():
        lo[a:b] = lo[a:b].clamp(min=a)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    sf = sinks.float().clone().requires_grad_(True) if sinks is not None else None
    sc = torch.matmul(qf, kf.repeat_interleave(rep, dim=1).transpose(-1, -2)) * SCALE
    allowed = (ar[None, :] <= ar[:, None]) & (ar[None, :] >= lo[:, None])
    sc = sc.masked_fill(~allowed, float("-inf"))
    if sf is not None:
        sc = torch.cat([sc, sf.reshape(1, -1, 1, 1).expand(q.shape[0], -1, S, 1)], dim=-1)
    lse = torch.logsumexp(sc.detach().double(), dim=-1)
    p = torch.softmax(sc, dim=-1)
    if sf is not None:
        p = p[..., :-1]
    oref = torch.matmul(p, vf.repeat_interleave(rep, dim=1))
    oref.backward(do.float())
    return (oref.detach(), qf.grad, kf.grad, vf.grad,
            sf.grad if sf is not None else None, lse)


def _check(got, ref, tag=""):
    names = ("out", "dq", "dk", "dv", "dsinks")
    for t, nm in zip(got, names):
        if t is not None:
            assert torch.isfinite(t.float()).all(), f"{tag}{nm}: non-finite"
    err_o = (got[0].float() - ref[0]).abs().max().item()
    print(f"{tag}out max err {err_o:.3e}")
    torch.testing.assert_close(got[0].float(), ref[0].float(), rtol=0, atol=3e-2)
    for g, r, nm in zip(got[1:5], ref[1:5], names[1:]):
        if r is None:
            assert g is None
            continue
        m = r.float().abs().max().item()
        err = (g.float() - r.float()).abs().max().item()
        print(f"{tag}{nm} max err {err:.3e} |ref|max {m:.3e}")
        assert err < 0.06 * max(m, 1.0), f"{tag}{nm}: max err {err} vs |ref|max {m}"


def _hip(q, k, v, do, W=None, cu=None, sinks=None):
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens, hip_flash_attention

    ds = de = None
    if cu is not None:
        ds, de = docs_from_cu_seqlens(torch.tensor(cu, dtype=torch.int32, device="cuda"), S)
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    if sinks is not None:
        sinks = sinks.detach().clone().requires_grad_(True)
    out = hip_flash_attention(q, k, v, SCALE, ds, de, sinks=sinks, sliding_window=W)
    out.backward(do)
    return out.detach(), q.grad, k.grad, v.grad, (sinks.grad if sinks is not None else None)


CASES = {
    "plain": dict(),
    # diagonal only; straddles a 32-key subtile; q block 1 starts past key
    # tile 0; no multiple of any tile
    "W1": dict(W=1), "W33": dict(W=33), "W100": dict(W=100), "W300": dict(W=300),
    # document edges inside a subtile, on the q-block edge and just past it
    "packed": dict(cu=PACKED),
    "sinks": dict(sinks="normal"), "sinks_dominant": dict(sinks="dominant"),
    "combined": dict(W=100, cu=PACKED, sinks="normal"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_d64_pair_vs_autograd(data, case):
    from veomni_amd.ops import hip_lib
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens, window_bounds

    kw = dict(CASES[case])
    nb = 1 if "cu" in kw else B
    q, k, v, do = (t[:nb] for t in data[:4])
    if "sinks" in kw:
        kw["sinks"] = data[4] if kw["sinks"] == "normal" else \
            torch.full((HQ,), 30.0, device="cuda")
    got = _hip(q, k, v, do, **kw)
    ref = _ref(q, k, v, do, **kw)
    _check(got, ref, tag=f"{case} ")
    # LSE, from the forward call the autograd function makes
    ds = de = None
    if "cu" in kw:
        ds, de = docs_from_cu_seqlens(
            torch.tensor(kw["cu"], dtype=torch.int32, device="cuda"), S)
    lo, _ = window_bounds(S, kw.get("W"), ds, de, "cuda")
    o, lse = hip_lib.attn64_fwd(q, k, v, SCALE, lo, kw.get("sinks"))
    assert torch.equal(o, got[0])
    e_lse = (lse.double() - ref[5]).abs().max().item()
    print(f"{case} LSE max err {e_lse:.3e}")
    assert torch.isfinite(lse).all() and e_lse <= 1e-4, e_lse


def test_d64_dsinks_reproducible(data):
    q, k, v, do, sinks = data
    a = _hip(q, k, v, do, sinks=sinks)
    b = _hip(q, k, v, do, sinks=sinks)
    assert a[4].dtype == torch.float32 and a[4].shape == (HQ,)
    assert torch.equal(a[4], b[4]), "dsinks differs between two runs"


def test_d64_slot_dispatch(data):
    """hip_attention_forward on D = 64 with a window and sinks: the hip_flash
    and sdpa cores agree, the default is the hip_flash core bit for bit, and
    softcap still raises."""
    from veomni_amd.ops.kernels.attention import hip_attention_forward

    q, k, v, do, sinks = data
    do_t = do.transpose(1, 2).contiguous()   # the slot returns [B, S, h, D]

    def run(**kw):
        qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        sk = sinks.detach().clone().requires_grad_(True)
        out, _ = hip_attention_forward(None, qq, kk, vv, None, scaling=SCALE,
                                       sliding_window=100, s_aux=sk, **kw)
        out.backward(do_t)
        return out.detach().transpose(1, 2), qq.grad, kk.grad, vv.grad, sk.grad

    flash, sdpa, default = run(core="hip_flash"), run(core="sdpa"), run()
    ref = _ref(q, k, v, do, W=100, sinks=sinks)
    _check(flash, ref, tag="slot hip_flash ")
    _check(sdpa, ref, tag="slot sdpa ")
    _check(flash, sdpa, tag="slot hip_flash vs sdpa ")
    for x, y, nm in zip(default, flash, ("out", "dq", "dk", "dv", "dsinks")):
        assert torch.equal(x, y), f"default core is not hip_flash: {nm}"
    with pytest.raises(NotImplementedError):
        hip_attention_forward(None, q, k, v, None, scaling=SCALE, softcap=30.0)


def test_d64_model_vs_eager():
    """tiny-d128-swa at gpt-oss's head_dim 64 with attention bias (4 query / 2
    KV heads, W = 128 on every second layer, sinks; no preset of its own: an
    existing test pins which presets carry a window) on one packed batch of
    S = 512, bound "hip" against eager
    and an fp32 eager copy, in the shape and with the tolerances of
    test_model_window_sinks_vs_eager: logits and loss rtol 5e-2 / atol 5e-1
    against bf16 eager; the all-HIP sink-gradient error against fp32 at most
    twice the larger of the bf16 eager and the HIP-but-attention errors."""
    import dataclasses

    from veomni_amd.models import PRESETS
    from veomni_amd.models.modeling import ForCausalLM, bind_ops
    from veomni_amd.ops import HIP_OPS_CONFIG

    torch.manual_seed(3)
    cfg = dataclasses.replace(PRESETS["tiny-d128-swa"], head_dim=64, attention_bias=True)
    with torch.device("cuda"):
        model = ForCausalLM(cfg).to(torch.bfloat16)
    cu = torch.tensor([0, 150, 380, 512], dtype=torch.int32, device="cuda")
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
            res[name, "loss"] = loss.detach().float()
            res[name, "sinks"] = [p.grad.float().clone() for p in sink_params]
    finally:
        bind_ops("eager")
    for what in ("logits", "loss"):
        torch.testing.assert_close(res["hip", what].float(), res["eager", what].float(),
                                   rtol=5e-2, atol=5e-1)
    for i, r in enumerate(res["fp32", "sinks"]):
        g = res["hip", "sinks"][i]
        err = {n: (res[n, "sinks"][i] - r).abs().max().item()
               for n in ("eager", "rest", "hip")}
        print(f"layer {i} sinks.grad |fp32|max {r.abs().max().item():.3e} err {err}")
        assert torch.isfinite(g).all() and g.abs().max().item() > 0
        assert err["hip"] <= 2 * max(err["rest"], err["eager"]), f"layer {i}: {err}"
