"""Sliding-window attention and attention sinks in the HIP flash pair
(pytest -m gpu): kernels, autograd function, attention slot and model.

Shapes: D = 128, bf16, (B, Hq, Hkv) = (2, 4, 2), S = 512: the smallest length
with a second 256-row q block, hence with forward tile skipping (t0 > 0), and
with more than one 128-row dq block and 64-row dkv strip.
Reference: fp32 torch autograd on the device from the same bf16 inputs, as in
tests/test_gpu_kernels.py::test_flash_attention_pair_vs_autograd, with the
tolerances of that test: output atol = 3e-2; each gradient (dsinks included)
max error < 0.06 * max(|ref|max, 1).

Window semantics (the reference's and HF's): key j is visible to query i iff
j <= i and j > i - W, inside i's document."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
SCALE = 1.0 / math.sqrt(D)
B, HQ, HKV, S = 2, 4, 2, 512


def bf(x):
    return x.to(torch.bfloat16)


@pytest.fixture(scope="module")
def lib():
    from veomni_amd.ops import hip_lib

    return hip_lib


@pytest.fixture(scope="module")
def data():
    """One set of inputs for the whole module (never modified)."""
    g = torch.Generator().manual_seed(77)
    q = bf(torch.randn(B, HQ, S, D, generator=g) * 0.5).cuda()
    k = bf(torch.randn(B, HKV, S, D, generator=g) * 0.5).cuda()
    v = bf(torch.randn(B, HKV, S, D, generator=g) * 0.5).cuda()
    do = bf(torch.randn(B, HQ, S, D, generator=g) * 0.5).cuda()
    sinks = torch.randn(HQ, generator=g).cuda()
    return q, k, v, do, sinks


def _lo_brute(W, cu=None):
    """First visible key of every row, straight from the rule in the module
    docstring (not from window_bounds)."""
    ar = torch.arange(S, device="cuda")
    lo = torch.zeros(S, dtype=torch.long, device="cuda")
    if W is not None:
        lo = (ar - W + 1).clamp(min=0)
    if cu is not None:
        ds = torch.zeros(S, dtype=torch.long, device="cuda")
        for a, b in zip(cu[:-1], cu[1:]):
            ds[a:b] = a
        lo = torch.maximum(lo, ds)
    return lo


def _ref(q, k, v, do, lo=None, sinks=None, scale=SCALE):
    """fp32 attention with autograd: causal mask, first visible key lo[i],
    optional sink column. Returns (out, dq, dk, dv, dsinks | None, lse)."""
    rep = q.shape[1] // k.shape[1]
    n = q.shape[2]
    qf = q.float().requires_grad_(True)
    kf = k.float().requires_grad_(True)
    vf = v.float().requires_grad_(True)
    sf = sinks.float().clone().requires_grad_(True) if sinks is not None else None
    kk = kf.repeat_interleave(rep, dim=1)
    vv = vf.repeat_interleave(rep, dim=1)
    sc = torch.matmul(qf, kk.transpose(-1, -2)) * scale
    ar = torch.arange(n, device=q.device)
    allowed = ar[None, :] <= ar[:, None]
    if lo is not None:
        allowed = allowed & (ar[None, :] >= lo[:, None])
    sc = sc.masked_fill(~allowed, float("-inf"))
    if sf is not None:
        col = sf.reshape(1, -1, 1, 1).expand(q.shape[0], -1, n, 1)
        sc = torch.cat([sc, col], dim=-1)
    lse = torch.logsumexp(sc.detach().double(), dim=-1)
    p = torch.softmax(sc, dim=-1)
    if sf is not None:
        p = p[..., :-1]
    oref = torch.matmul(p, vv)
    oref.backward(do.float())
    return (oref.detach(), qf.grad, kf.grad, vf.grad,
            sf.grad if sf is not None else None, lse)


def _hip(q, k, v, do, sinks=None, **kw):
    from veomni_amd.ops.kernels.attention import hip_flash_attention

    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    if sinks is not None:
        sinks = sinks.detach().clone().requires_grad_(True)
    token_major = kw.get("token_major", False)
    out = hip_flash_attention(q, k, v, SCALE, sinks=sinks, **kw)
    out.backward(do.transpose(1, 2).contiguous() if token_major else do)
    out = out.detach()
    if token_major:
        out = out.transpose(1, 2)
    return out, q.grad, k.grad, v.grad, (sinks.grad if sinks is not None else None)


def _check(got, ref, tag=""):
    names = ("out", "dq", "dk", "dv", "dsinks")
    for t, nm in zip(got, names):
        if t is not None:
            assert torch.isfinite(t.float()).all(), f"{tag}{nm}: non-finite"
    err_o = (got[0].float() - ref[0]).abs().max().item()
    print(f"{tag}out max err {err_o:.3e}")
    torch.testing.assert_close(got[0].float(), ref[0], rtol=0, atol=3e-2)
    for g, r, nm in zip(got[1:5], ref[1:5], names[1:]):
        if r is None:
            assert g is None
            continue
        m = r.abs().max().item()
        err = (g.float() - r).abs().max().item()
        print(f"{tag}{nm} max err {err:.3e} |ref|max {m:.3e}")
        assert err < 0.06 * max(m, 1.0), f"{tag}{nm}: max err {err} vs |ref|max {m}"


# ------------------------------------------------------------ 1. window only
# 1: the diagonal alone. 33 straddles a 32-key subtile. 64: one kv tile.
# 100: q block 1 starts at key tile 2 (t0 = (256-99)/64) and the dkv q loop of
# strip 0 stops at tile 3 of 8 (hi[63] = 163). 256: the q block size. 300: no
# multiple of any tile.
@pytest.mark.parametrize("nb", [2, 1])
@pytest.mark.parametrize("W", [1, 33, 64, 100, 256, 300])
def test_window_only(lib, data, W, nb):
    q, k, v, do, _ = (t[:nb] if t.dim() == 4 else t for t in data)
    got = _hip(q, k, v, do, sliding_window=W)
    ref = _ref(q, k, v, do, lo=_lo_brute(W))
    _check(got, ref, tag=f"W={W} B={nb} ")


# ------------------------------------------- 2. W = S through the bounds path
def test_full_window_bounds_path_equals_plain(lib, data):
    """W = S cuts nothing. window_bounds returns (None, None) for it (plain
    causal), so the bounds it would otherwise build, lo = 0 and hi = S, are
    passed directly with shared_bounds: the DOC kernels through the new entry
    points, B = 2. They always take the masked arithmetic, the plain ones the
    unmasked body on full tiles; the values are the same, bit for bit."""
    from veomni_amd.ops.kernels.attention import window_bounds

    q, k, v, do, _ = data
    assert window_bounds(S, S, None, None, "cuda") == (None, None)
    lo = torch.zeros(S, dtype=torch.int32, device="cuda")
    hi = torch.full((S,), S, dtype=torch.int32, device="cuda")
    plain = _hip(q, k, v, do)
    bounds = _hip(q, k, v, do, doc_start=lo, doc_end=hi, shared_bounds=True)
    for a, b, nm in zip(plain[:4], bounds[:4], ("out", "dq", "dk", "dv")):
        diff = (a.float() - b.float()).abs().max().item()
        print(f"{nm}: bounds path vs plain max abs diff {diff:.3e}")
        assert torch.equal(a, b), f"{nm}: bounds path != plain, max diff {diff}"


# ------------------------------------------------ 3. window + packed varlen
def test_window_packed_varlen(lib, data):
    """cu = [0, 200, 512], W = 100, B = 1 against per-document windowed fp32,
    and no leakage: document 2's outputs keep their bits when document 1's
    K / V are replaced."""
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens

    q, k, v, do, _ = (t[:1] if t.dim() == 4 else t for t in data)
    cu = [0, 200, 512]
    W = 100
    ds, de = docs_from_cu_seqlens(
        torch.tensor(cu, dtype=torch.int32, device="cuda"), S)
    got = _hip(q, k, v, do, doc_start=ds, doc_end=de, sliding_window=W)
    for i, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
        n = b - a
        lo = (torch.arange(n, device="cuda") - W + 1).clamp(min=0)
        sl = lambda t: t[:, :, a:b]
        ref = _ref(sl(q), sl(k), sl(v), sl(do), lo=lo)
        _check((sl(got[0]), sl(got[1]), sl(got[2]), sl(got[3]), None), ref,
               tag=f"doc {i} ")
    g = torch.Generator().manual_seed(78)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, :200] = bf(torch.randn(1, HKV, 200, D, generator=g)).cuda()
    v2[:, :, :200] = bf(torch.randn(1, HKV, 200, D, generator=g)).cuda()
    got2 = _hip(q, k2, v2, do, doc_start=ds, doc_end=de, sliding_window=W)
    assert torch.equal(got[0][:, :, 200:], got2[0][:, :, 200:]), \
        "document 2 outputs changed with document 1's K/V"
    assert not torch.equal(got[0][:, :, :200], got2[0][:, :, :200])


# ------------------------------------------------------------ 4. sinks only
@pytest.fixture(scope="module")
def plain_fwd(lib, data):
    """The existing plain kernel's O and LSE, its LSE error against an fp64
    logsumexp of the same inputs, and the fp64 scores' logsumexp itself."""
    q, k, v, do, _ = data
    o, lse = lib.attn_fwd(q, k, v, SCALE)
    rep = HQ // HKV
    sc = torch.matmul(q.double(), k.double().repeat_interleave(rep, dim=1)
                      .transpose(-1, -2)) * SCALE
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool, device="cuda"), 1)
    lse64 = torch.logsumexp(sc.masked_fill(mask, float("-inf")), dim=-1)
    err = (lse.double() - lse64).abs().max().item()
    return o, lse, lse64, err


@pytest.mark.parametrize("kind", ["normal", "dominant", "negligible"])
def test_sinks_only(lib, data, plain_fwd, kind):
    """Sinks drawn from N(0, 1), a dominant sink (+30: every score is far
    below it) and a negligible one (-30: every row's scores dominate).
    Everything finite; vs fp32; and the identities against the existing plain
    kernel, LSE_sink = logaddexp(LSE_plain, sink) and O_sink = O_plain *
    exp(LSE_plain - LSE_sink).

    LSE bound: the plain kernel's own max error against the fp64 logsumexp
    is measured (e_plain); the sink LSE may be off by 2 * e_plain against the
    fp64 sink-inclusive logsumexp (one more exp / log). Against logaddexp of
    the plain kernel's fp32 LSE that makes 3 * e_plain, since the plain LSE
    brings its own error along.
    O bound: the two runs round their probabilities to bf16 independently
    (relative 2^-9 each, so 2^-9 * max|V| on a row's P.V) and their outputs
    to bf16 (2^-9 * max|O|): 2 * 2^-9 * (max|V| + max|O|)."""
    q, k, v, do, sinks_n = data
    sinks = {"normal": sinks_n,
             "dominant": torch.full((HQ,), 30.0, device="cuda"),
             "negligible": torch.full((HQ,), -30.0, device="cuda")}[kind]
    o_plain, lse_plain, lse64, e_plain = plain_fwd

    o, lse = lib.attn_fwd_win_sink(q, k, v, SCALE, None, sinks)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    got = _hip(q, k, v, do, sinks=sinks)
    assert torch.equal(got[0], o)
    ref = _ref(q, k, v, do, sinks=sinks)
    _check(got, ref, tag=f"{kind} ")

    sk = sinks.double().reshape(1, HQ, 1).expand(B, HQ, S)
    lse64_sink = torch.logaddexp(lse64, sk)
    e_sink = (lse.double() - lse64_sink).abs().max().item()
    e_ident = (lse.double() - torch.logaddexp(lse_plain.double(), sk)).abs().max().item()
    print(f"{kind}: LSE err plain {e_plain:.3e} sink {e_sink:.3e} "
          f"identity {e_ident:.3e}")
    assert e_sink <= 2 * e_plain, (e_sink, e_plain)
    assert e_ident <= 3 * e_plain, (e_ident, e_plain)
    o_id = o_plain.float() * torch.exp(lse_plain - lse).unsqueeze(-1)
    tol = 2 * 2.0 ** -9 * (v.float().abs().max().item()
                           + o_plain.float().abs().max().item())
    e_o = (o.float() - o_id).abs().max().item()
    print(f"{kind}: O identity max err {e_o:.3e} (bound {tol:.3e})")
    assert e_o <= tol, (e_o, tol)


# ---------------------------------------------------------------- 5. dsinks
def test_dsinks_reproducible_and_layout_independent(lib, data):
    q, k, v, do, sinks = data
    ref = _ref(q, k, v, do, sinks=sinks)
    a = _hip(q, k, v, do, sinks=sinks)
    b = _hip(q, k, v, do, sinks=sinks)
    t = _hip(q, k, v, do, sinks=sinks, token_major=True)
    _check(a, ref, tag="head-major ")
    assert a[4].dtype == torch.float32 and a[4].shape == (HQ,)
    assert torch.equal(a[4], b[4]), "dsinks differs between two runs"
    for x, y, nm in zip(a, t, ("out", "dq", "dk", "dv", "dsinks")):
        assert torch.equal(x, y), f"{nm}: token-major != head-major"


# ----------------------------------------- 6. sinks + window + varlen at once
def test_sinks_window_varlen_function_level(lib, data):
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens

    q, k, v, do, sinks = (t[:1] if t.dim() == 4 else t for t in data)
    cu = [0, 200, 512]
    ds, de = docs_from_cu_seqlens(
        torch.tensor(cu, dtype=torch.int32, device="cuda"), S)
    got = _hip(q, k, v, do, sinks=sinks, doc_start=ds, doc_end=de,
               sliding_window=100)
    ref = _ref(q, k, v, do, lo=_lo_brute(100, cu), sinks=sinks)
    _check(got, ref, tag="sinks+W+varlen ")


# ------------------------------------------------------------- 7. slot level
def test_slot_honours_window_and_sinks(lib, data):
    """hip_attention_forward(..., sliding_window=100, s_aux=sinks) is not the
    call without them (it was, while both were ignored), on either layout,
    and the hip_flash core agrees with the sdpa core."""
    from veomni_amd.ops.kernels.attention import hip_attention_forward

    q, k, v, do, sinks = data
    do_t = do.transpose(1, 2).contiguous()   # the slot returns [B, S, h, D]

    def run(**kw):
        qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        sk = None
        if kw.get("s_aux") is not None:
            sk = kw["s_aux"].detach().clone().requires_grad_(True)
            kw["s_aux"] = sk
        out, _ = hip_attention_forward(None, qq, kk, vv, None, scaling=SCALE, **kw)
        out.backward(do_t)
        return (out.detach().transpose(1, 2), qq.grad, kk.grad, vv.grad,
                sk.grad if sk is not None else None)

    plain = run()
    flash = run(sliding_window=100, s_aux=sinks)
    flash_tm = run(sliding_window=100, s_aux=sinks, token_major_out=True)
    sdpa = run(sliding_window=100, s_aux=sinks, core="sdpa")
    diff = (flash[0].float() - plain[0].float()).abs().max().item()
    print(f"slot: windowed+sinks vs plain max abs diff {diff:.3e}")
    assert diff > 3e-2, "sliding_window / s_aux were ignored"
    for x, y in zip(flash, flash_tm):
        assert torch.equal(x, y)
    ref = _ref(q, k, v, do, lo=_lo_brute(100), sinks=sinks)
    _check(flash, ref, tag="slot hip_flash ")
    _check(sdpa, ref, tag="slot sdpa ")
    _check(flash, tuple(t.float() if t is not None else None for t in sdpa),
           tag="slot hip_flash vs sdpa ")
    with pytest.raises(NotImplementedError):
        hip_attention_forward(None, q, k, v, None, scaling=SCALE, softcap=30.0)


# ------------------------------------------------------------ 8. model level
def test_model_window_sinks_vs_eager(lib):
    """tiny-d128-swa (alternating sliding / full layers, W = 128, sinks) on a
    packed 3-document batch: HIP ops against eager, tolerance of
    test_attention_slot_varlen_vs_eager_model; then one backward step:
    sinks.grad is non-zero and close to eager. The sink gradients are ~1e-3,
    sums over 512 rows of signed terms, so the project's gradient bound with
    its floor of 1 would pass anything, and the cancellation amplifies every
    bf16 rounding upstream of the attention backward. The yardstick is
    therefore what the bf16 model around the attention costs: each bf16 run
    is compared with the eager run of an fp32 copy of the model, once all
    eager, once with every HIP op but attention ("rest": the noise the other
    ops' roundings put into the eager sink gradient) and once with all HIP
    ops. The all-HIP error may be at most twice the larger of the other two
    (two bf16 computations of one quantity with independent roundings; the
    bound of tests/test_gpu_swiglu_limit.py)."""
    import copy

    from veomni_amd.models import build_model
    from veomni_amd.models.modeling import bind_ops
    from veomni_amd.ops import HIP_OPS_CONFIG

    torch.manual_seed(3)
    model = build_model("tiny-d128-swa", dtype=torch.bfloat16, device="cuda")
    cu = torch.tensor([0, 150, 380, 512], dtype=torch.int32, device="cuda")
    ids = torch.randint(0, model.config.vocab_size, (1, S), device="cuda")
    pos = torch.cat([torch.arange(int(cu[i + 1]) - int(cu[i]), device="cuda")
                     for i in range(cu.numel() - 1)])[None]
    sink_params = [l.self_attn.sinks for l in model.model.layers]
    assert all(p is not None and p.shape == (4,) for p in sink_params)
    grads = {}
    try:
        bind_ops("eager")
        m32 = copy.deepcopy(model).float()
        loss, _ = m32(ids, labels=ids, position_ids=pos, cu_seq_lens_q=cu)
        loss.backward()
        grads["fp32", "sinks"] = [l.self_attn.sinks.grad.clone()
                                  for l in m32.model.layers]
        rest = dict(HIP_OPS_CONFIG, attention="eager")
        for name, impl in (("eager", "eager"), ("rest", rest),
                           ("hip", HIP_OPS_CONFIG)):
            bind_ops(impl)
            model.eval()
            with torch.no_grad():
                grads[name, "logits"], _ = model(ids, position_ids=pos,
                                                 cu_seq_lens_q=cu)
            model.train()
            model.zero_grad(set_to_none=True)
            loss, _ = model(ids, labels=ids, position_ids=pos, cu_seq_lens_q=cu)
            loss.backward()
            grads[name, "sinks"] = [p.grad.float().clone() for p in sink_params]
    finally:
        bind_ops("eager")
    torch.testing.assert_close(grads["hip", "logits"].float(),
                               grads["eager", "logits"].float(),
                               rtol=5e-2, atol=5e-1)
    for i, r in enumerate(grads["fp32", "sinks"]):
        g = grads["hip", "sinks"][i]
        m = r.abs().max().item()
        err = {n: (grads[n, "sinks"][i] - r).abs().max().item()
               for n in ("eager", "rest", "hip")}
        print(f"layer {i} sinks.grad |fp32 ref|max {m:.3e} err vs fp32: "
              f"eager bf16 {err['eager']:.3e} rest-hip {err['rest']:.3e} "
              f"all-hip {err['hip']:.3e}")
        assert torch.isfinite(g).all() and g.abs().max().item() > 0
        assert err["hip"] <= 2 * max(err["rest"], err["eager"]), \
            f"layer {i} sinks.grad: {err}"
