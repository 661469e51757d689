"""The MLA HIP flash pair, q/k head_dim 192 and v head_dim 128 (pytest -m
gpu): kernels through the autograd function, the attention slot and a model.

Shapes: bf16, B = 2, S = 512 (the smallest length with a second 256-row q
block, more than one dq block and several dkv strips), heads (4, 4), the MLA
case, and (4, 2), which runs the group loop; tails S = 333 and S = 1.
Reference: fp32 torch autograd on the device from the same bf16 inputs, as
_ref in tests/test_gpu_attn_d64.py with V 128 wide, and that file's
tolerances (the same error sources: bf16 P, bf16 dS, bf16 stores): output
atol = 3e-2; each gradient max error < 0.06 * max(|ref|max, 1).

LSE bound (against an fp64 logsumexp of the same scores): LSE = ln2 * (m +
log2(l)). A score is an fp32 MFMA chain of 12 accumulation steps over exact
bf16 products, then scaled into the exp2 domain with one rounding: 13
roundings of values below 64, each <= one ulp = 2^-18, so <= 13 * 2^-18 =
5.0e-5 in the exp2 domain, 3.4e-5 after the factor ln2. Each of the <= 513
terms of l carries that as a relative error, plus one ulp of v_exp_f32
(1.2e-7); the fp32 sum of n terms adds at most n * 2^-24 = 3.1e-5. m, log2(l)
and the final product add three more roundings of a value below 64
(3 * 2^-18 * ln2 = 0.8e-5). Total < 7.4e-5; the test allows 1e-4."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DQK, DV = 192, 128
SCALE = DQK ** -0.5
B, S = 2, 512
PACKED = [0, 70, 256, 300, 512]


def _make(hq, hkv, s, b=B, seed=192):
    g = torch.Generator().manual_seed(seed)
    mk = lambda h, d: (torch.randn(b, h, s, d, generator=g) * 0.5).to(torch.bfloat16).cuda()
    return mk(hq, DQK), mk(hkv, DQK), mk(hkv, DV), mk(hq, DV)


@pytest.fixture(scope="module")
def data():
    """One set of inputs per head layout for the whole module (never modified)."""
    return {(4, 4): _make(4, 4, S), (4, 2): _make(4, 2, S)}


def _ref(q, k, v, do, W=None, cu=None):
    """fp32 attention with autograd: key j is visible to query i iff j <= i,
    j > i - W and j is in i's document. Returns (out, dq, dk, dv, lse fp64)."""
    s = q.shape[2]
    rep = q.shape[1] // k.shape[1]
    ar = torch.arange(s, device="cuda")
    lo = (ar - W + 1).clamp(min=0) if W is not None else torch.zeros_like(ar)
    for a, b in zip(cu[:-1], cu[1:]) if cu is not None else ():
        lo[a:b] = lo[a:b].clamp(min=a)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    sc = torch.matmul(qf, kf.repeat_interleave(rep, dim=1).transpose(-1, -2)) * SCALE
    allowed = (ar[None, :] <= ar[:, None]) & (ar[None, :] >= lo[:, None])
    sc = sc.masked_fill(~allowed, float("-inf"))
    lse = torch.logsumexp(sc.detach().double(), dim=-1)
    oref = torch.matmul(torch.softmax(sc, dim=-1), vf.repeat_interleave(rep, dim=1))
    oref.backward(do.float())
    return oref.detach(), qf.grad, kf.grad, vf.grad, lse


def _check(got, ref, tag=""):
    names = ("out", "dq", "dk", "dv")
    for t, nm in zip(got, names):
        assert torch.isfinite(t.float()).all(), f"{tag}{nm}: non-finite"
    print(f"{tag}out max err {(got[0].float() - ref[0].float()).abs().max().item():.3e}")
    torch.testing.assert_close(got[0].float(), ref[0].float(), rtol=0, atol=3e-2)
    for g, r, nm in zip(got[1:4], ref[1:4], names[1:]):
        m = r.float().abs().max().item()
        err = (g.float() - r.float()).abs().max().item()
        print(f"{tag}{nm} max err {err:.3e} |ref|max {m:.3e}")
        assert err < 0.06 * max(m, 1.0), f"{tag}{nm}: max err {err} vs |ref|max {m}"


def _docs(cu, s):
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens

    if cu is None:
        return None, None
    return docs_from_cu_seqlens(torch.tensor(cu, dtype=torch.int32, device="cuda"), s)


def _hip(q, k, v, do, W=None, cu=None):
    from veomni_amd.ops.kernels.attention import hip_flash_attention

    ds, de = _docs(cu, q.shape[2])
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = hip_flash_attention(q, k, v, SCALE, ds, de, sliding_window=W)
    out.backward(do)
    return out.detach(), q.grad, k.grad, v.grad


CASES = {
    "plain": dict(),
    # document edges inside a subtile, on the q-block edge and just past it
    "packed": dict(cu=PACKED),
    # straddles a 32-key subtile; longer than a q block
    "W33": dict(W=33), "W300": dict(W=300),
    "packed+W100": dict(W=100, cu=PACKED),
    # no multiple of any tile, documents to the ragged end; a single row
    "tail": dict(S=333, cu=[0, 70, 256, 333]),
    "S1": dict(S=1),
}


@pytest.mark.parametrize("heads", [(4, 4), (4, 2)], ids=["h4x4", "h4x2"])
@pytest.mark.parametrize("case", list(CASES))
def test_mla_pair_vs_autograd(data, heads, case):
    from veomni_amd.ops import hip_lib
    from veomni_amd.ops.kernels.attention import window_bounds

    kw = dict(CASES[case])
    s = kw.pop("S", S)
    nb = 1 if "cu" in kw else B
    src = data[heads] if s == S else _make(*heads, s, seed=s)
    q, k, v, do = (t[:nb] for t in src)
    got = _hip(q, k, v, do, **kw)
    ref = _ref(q, k, v, do, **kw)
    assert got[0].shape == (nb, heads[0], s, DV) and got[3].shape == v.shape
    _check(got, ref, tag=f"{case} {heads} ")
    # LSE, from the forward call the autograd function makes
    lo, _ = window_bounds(s, kw.get("W"), *_docs(kw.get("cu"), s), "cuda")
    o, lse = hip_lib.attn_mla_fwd(q, k, v, SCALE, lo)
    assert torch.equal(o, got[0])
    e_lse = (lse.double() - ref[4]).abs().max().item()
    print(f"{case} {heads} LSE max err {e_lse:.3e}")
    assert torch.isfinite(lse).all() and e_lse <= 1e-4, e_lse


def test_mla_grads_reproducible(data):
    q, k, v, do = (t[:1] for t in data[(4, 2)])
    a = _hip(q, k, v, do, cu=PACKED)
    b = _hip(q, k, v, do, cu=PACKED)
    for x, y, nm in zip(a[1:], b[1:], ("dq", "dk", "dv")):
        assert torch.equal(x, y), f"{nm} differs between two runs"


def test_mla_slot_dispatch(data):
    """hip_attention_forward on 192 / 128 with documents: the hip_flash and
    sdpa cores match the reference, the default is the hip_flash core bit for
    bit, s_aux takes the eager core, sinks and token_major raise."""
    from veomni_amd.ops.kernels.attention import hip_attention_forward, hip_flash_attention

    q, k, v, do = (t[:1] for t in data[(4, 2)])
    do_t = do.transpose(1, 2).contiguous()   # the slot returns [B, S, h, D]
    ds, de = _docs(PACKED, S)

    def run(**kw):
        qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        out, _ = hip_attention_forward(None, qq, kk, vv, None, scaling=SCALE,
                                       doc_start=ds, doc_end=de, **kw)
        out.backward(do_t)
        return out.detach().transpose(1, 2), qq.grad, kk.grad, vv.grad

    flash, sdpa, default = run(core="hip_flash"), run(core="sdpa"), run()
    ref = _ref(q, k, v, do, cu=PACKED)
    _check(flash, ref, tag="slot hip_flash ")
    _check(sdpa, ref, tag="slot sdpa ")
    for x, y, nm in zip(default, flash, ("out", "dq", "dk", "dv")):
        assert torch.equal(x, y), f"default core is not hip_flash: {nm}"
    # a sink of -30 adds exp(-30 - lse) to each row sum: below bf16 resolution
    sink = torch.full((4,), -30.0, device="cuda")
    _check(run(s_aux=sink), ref, tag="slot s_aux ")
    with pytest.raises(ValueError):
        hip_flash_attention(q, k, v, SCALE, sinks=sink)
    with pytest.raises(ValueError):
        hip_flash_attention(q, k, v, SCALE, token_major=True)


def test_mla_model_vs_eager():
    """tiny-mla on one packed batch of S = 512, bound HIP_OPS_CONFIG against
    eager: logits and loss at rtol 5e-2 / atol 5e-1 (test_d64_model_vs_eager's
    tolerances); every parameter gradient finite and non-zero."""
    from veomni_amd.models import build_model
    from veomni_amd.models.modeling import bind_ops
    from veomni_amd.ops import HIP_OPS_CONFIG

    torch.manual_seed(3)
    model = build_model("tiny-mla", dtype=torch.bfloat16, device="cuda")
    cu = torch.tensor([0, 150, 380, 512], dtype=torch.int32, device="cuda")
    ids = torch.randint(0, model.config.vocab_size, (1, S), device="cuda")
    pos = torch.cat([torch.arange(int(cu[i + 1]) - int(cu[i]), device="cuda")
                     for i in range(cu.numel() - 1)])[None]
    res = {}
    try:
        for name, impl in (("eager", "eager"), ("hip", HIP_OPS_CONFIG)):
            bind_ops(impl)
            model.eval()
            with torch.no_grad():
                res[name, "logits"], _ = model(ids, position_ids=pos, cu_seq_lens_q=cu)
            model.train()
            model.zero_grad(set_to_none=True)
            loss, _ = model(ids, labels=ids, position_ids=pos, cu_seq_lens_q=cu)
            loss.backward()
            res[name, "loss"] = loss.detach().float()
    finally:
        bind_ops("eager")
    for what in ("logits", "loss"):
        torch.testing.assert_close(res["hip", what].float(), res["eager", what].float(),
                                   rtol=5e-2, atol=5e-1)
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() \
            and p.grad.abs().max().item() > 0, n
