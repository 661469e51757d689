"""Attention prep with fewer copies (pytest -m gpu): the strided per-head
RMSNorm entry points, the flash pair with token-major O / dO, the
4-rows-per-wave backward preprocess, and Attention.forward with the q/k norm
node and token-major attention output against the per-op slot path.

The strided kernels change addressing only, so every comparison against the
contiguous / head-major entry points is torch.equal. The one exception is the
norm weight gradient: its per-wave partials (identical in both kernels) are
joined by a 16-way fp32 atomic combine in k_dw_reduce whose order is not
fixed. Reordering at most 16 fp32 addends moves the sum by about 16 * 2^-24
~= 1e-6 relative, so dw is held to rtol = 1e-5. With 6 rows only two
partials are non-zero, a + b == b + a, and dw has to be torch.equal too.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
EPS = 1e-6
DW_RTOL = 1e-5


@pytest.fixture(scope="module")
def lib():
    from veomni_amd.ops import hip_lib

    return hip_lib


def bf(x):
    return x.to(torch.bfloat16)


def _qkv(B, S, hq, hkv, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = bf(torch.randn(B, S, hq + 2 * hkv, D, generator=g)).cuda()
    w = bf(1.0 + 0.1 * torch.randn(D, generator=g)).cuda()
    return qkv, w


# ------------------------------------------------------------ strided norm
# B = 2, S = 5, hq = 3, hkv = 1: 5 heads in the qkv row, so slices are not
# 4-aligned; 30 q rows, not a multiple of 4 or 16, so a wave's 4 rows
# straddle tokens and batches.
def test_strided_norm_forward(lib):
    B, S, hq, hkv = 2, 5, 3, 1
    qkv, w = _qkv(B, S, hq, hkv, 0)
    for lo, h in ((0, hq), (hq, hkv)):
        x = qkv[:, :, lo:lo + h]
        y_ref, rstd_ref = lib.rmsnorm_fwd(x.contiguous(), w, EPS)
        y, rstd = lib.rmsnorm128_fwd_strided(x, w, EPS)
        # the default output is the transpose of a head-major buffer
        assert y.transpose(1, 2).is_contiguous()
        assert y.shape == (B, S, h, D)
        assert torch.equal(y, y_ref)
        assert torch.equal(rstd, rstd_ref)
        # token-major output (what the model's q/k norm node writes)
        y_tm = torch.full_like(y_ref, float("nan"))
        _, rstd_tm = lib.rmsnorm128_fwd_strided(x, w, EPS, y_tm)
        assert torch.equal(y_tm, y_ref)
        assert torch.equal(rstd_tm, rstd_ref)


def _norm_bwd_pair(lib, B, S, hq, hkv, seed, positive=False):
    qkv, w = _qkv(B, S, hq, hkv, seed)
    g = torch.Generator().manual_seed(seed + 100)
    dy_hm = bf(torch.randn(B, hq, S, D, generator=g)).cuda()
    if positive:
        qkv, dy_hm = qkv.abs(), dy_hm.abs()
    x = qkv[:, :, :hq]
    xc = x.contiguous()
    _, rstd = lib.rmsnorm_fwd(xc, w, EPS)
    # dy arrives head-major, as RoPE backward produces it
    dy = dy_hm.transpose(1, 2)
    dx_ref, dw_ref = lib.rmsnorm_bwd(dy.contiguous(), xc, w, rstd)
    dqkv = torch.full_like(qkv, float("nan"))
    dw = lib.rmsnorm128_bwd_strided(dy, x, w, rstd, dqkv[:, :, :hq])
    assert torch.equal(dqkv[:, :, :hq], dx_ref)
    assert torch.isnan(dqkv[:, :, hq:]).all(), "wrote outside the q slice"
    return dw, dw_ref


def test_strided_norm_backward(lib):
    # mixed signs: dx, and nothing written outside the slice
    _norm_bwd_pair(lib, 2, 5, 3, 1, 1)
    # dw against the rtol: same shape, x and dy >= 0. Every addend of a dw
    # element then has one sign, and only then is "reordering 16 addends
    # moves the sum by ~1e-6 relative" true; an element whose addends cancel
    # has no relative bound at all.
    dw, dw_ref = _norm_bwd_pair(lib, 2, 5, 3, 1, 1, positive=True)
    err = ((dw - dw_ref).abs() / dw_ref.abs().clamp_min(1e-30)).max().item()
    print(f"dw max rel err {err:.3e}")
    torch.testing.assert_close(dw, dw_ref, rtol=DW_RTOL, atol=0.0)


def test_strided_norm_backward_two_partials(lib):
    # 6 rows: waves 0 and 1 hold the only non-zero partials
    dw, dw_ref = _norm_bwd_pair(lib, 1, 2, 3, 1, 2)
    assert torch.equal(dw, dw_ref)


def test_strided_norm_backward_k_slice(lib):
    # a slice in the middle of the row: both neighbours stay untouched
    B, S, hq, hkv = 2, 5, 3, 1
    qkv, w = _qkv(B, S, hq, hkv, 3)
    x = qkv[:, :, hq:hq + hkv]
    _, rstd = lib.rmsnorm_fwd(x.contiguous(), w, EPS)
    dy = bf(torch.randn(B, hkv, S, D)).cuda().transpose(1, 2)
    dx_ref, _ = lib.rmsnorm_bwd(dy.contiguous(), x.contiguous(), w, rstd)
    dqkv = torch.full_like(qkv, float("nan"))
    lib.rmsnorm128_bwd_strided(dy, x, w, rstd, dqkv[:, :, hq:hq + hkv])
    assert torch.equal(dqkv[:, :, hq:hq + hkv], dx_ref)
    assert torch.isnan(dqkv[:, :, :hq]).all() and torch.isnan(dqkv[:, :, hq + hkv:]).all()


# --------------------------------------------------------- attention strides
def _attn_inputs(B, Hq, Hkv, S, seed):
    g = torch.Generator().manual_seed(seed)
    q = bf(torch.randn(B, Hq, S, D, generator=g) * 0.5).cuda()
    k = bf(torch.randn(B, Hkv, S, D, generator=g) * 0.5).cuda()
    v = bf(torch.randn(B, Hkv, S, D, generator=g) * 0.5).cuda()
    do = bf(torch.randn(B, Hq, S, D, generator=g) * 0.5).cuda()
    return q, k, v, do


def _two_docs(S, cut):
    ar = torch.arange(S)
    ds = torch.where(ar < cut, 0, cut).to(torch.int32).cuda()
    de = torch.where(ar < cut, cut, S).to(torch.int32).cuda()
    return ds, de


@pytest.mark.parametrize("varlen", [False, True], ids=["plain", "varlen2"])
def test_attention_token_major(lib, varlen):
    # varlen is the packed path (B == 1); the document cut is off every tile
    # boundary
    B, Hq, Hkv, S = (1, 4, 2, 512) if varlen else (2, 4, 2, 512)
    scale = 1.0 / math.sqrt(D)
    q, k, v, do = _attn_inputs(B, Hq, Hkv, S, 7 + int(varlen))
    ds, de = _two_docs(S, 200) if varlen else (None, None)

    o_hm, lse_hm = lib.attn_fwd(q, k, v, scale, ds)
    o_tm, lse_tm = lib.attn_fwd_token_major(q, k, v, scale, ds)
    assert o_tm.shape == (B, S, Hq, D) and o_tm.is_contiguous()
    assert torch.equal(o_tm.transpose(1, 2), o_hm)
    assert torch.equal(lse_tm, lse_hm)

    ref = lib.attn_bwd(q, k, v, o_hm, lse_hm, do, scale, ds, de)
    do_tm = do.transpose(1, 2).contiguous()
    got = lib.attn_bwd_token_major(q, k, v, o_tm, lse_tm, do_tm, scale, ds, de)
    for name, a, b in zip(("dq", "dk", "dv"), got, ref):
        assert torch.equal(a, b), name


def test_bwd_pre_four_rows(lib):
    B, Hq, S = 2, 4, 512
    g = torch.Generator().manual_seed(11)
    o = bf(torch.randn(B, Hq, S, D, generator=g)).cuda()
    do = bf(torch.randn(B, Hq, S, D, generator=g)).cuda()
    lse = torch.randn(B, Hq, S, generator=g).cuda()
    rows = B * Hq * S
    L = lib.get_lib()

    def run(fn, *args):
        delta = torch.empty(rows, dtype=torch.float32, device="cuda")
        lse2 = torch.empty(rows, dtype=torch.float32, device="cuda")
        lib.check(fn(lib.dptr(args[0]), lib.dptr(args[1]), lib.dptr(lse),
                     lib.dptr(delta), lib.dptr(lse2), *args[2:],
                     lib.cur_stream()), "bwd_pre")
        return delta, lse2

    d_ref, l_ref = run(L.vh_attn_bwd_pre_bf16, do, o, rows)
    # head-major strides through the 4-row kernel
    d_hm, l_hm = run(L.vh_attn_bwd_pre_ostrided_bf16, do, o, B, Hq, S,
                     Hq * S * D, S * D, D)
    # token-major
    o_tm, do_tm = (t.transpose(1, 2).contiguous() for t in (o, do))
    d_tm, l_tm = run(L.vh_attn_bwd_pre_ostrided_bf16, do_tm, o_tm, B, Hq, S,
                     S * Hq * D, D, Hq * D)
    for d, l in ((d_hm, l_hm), (d_tm, l_tm)):
        assert torch.equal(d, d_ref)
        assert torch.equal(l, l_ref)


# ------------------------------------------------------------------ module
def test_attention_module_fused_vs_slots():
    import veomni_amd.ops  # noqa: F401
    from veomni_amd.distributed.parallel_state import get_parallel_state
    from veomni_amd.models.modeling import (Attention, ModelConfig,
                                            RotaryEmbedding, bind_ops)
    from veomni_amd.ops import HIP_OPS_CONFIG

    cfg = ModelConfig(hidden_size=256, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=128, qk_norm=True,
                      num_hidden_layers=1)
    B, S = 2, 256
    torch.manual_seed(0)
    attn = Attention(cfg, 0).to(device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        attn.q_norm.weight.add_(0.1 * torch.randn_like(attn.q_norm.weight))
        attn.k_norm.weight.add_(0.1 * torch.randn_like(attn.k_norm.weight))
    rot = RotaryEmbedding(cfg).to("cuda")
    x0 = bf(torch.randn(B, S, cfg.hidden_size)).cuda()
    dy = bf(torch.randn(B, S, cfg.hidden_size)).cuda()
    pos = torch.arange(S, device="cuda")[None].expand(B, -1)
    cos, sin = rot(x0, pos)

    def run(layout):
        attn.qkv_layout = layout
        attn.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = attn(x, (cos, sin))
        y.backward(dy)
        grads = {n: p.grad.clone() for n, p in attn.named_parameters()}
        return y.detach(), x.grad, grads

    bind_ops(HIP_OPS_CONFIG)
    try:
        taken = attn._fused_layout_applies(
            torch.empty(B, S, 8, 128, device="cuda", dtype=torch.bfloat16),
            get_parallel_state(), {})
        assert taken, "the fused layout path is not taken on this config"
        y_f, dx_f, g_f = run("fused")
        y_s, dx_s, g_s = run("slots")
    finally:
        bind_ops("eager")
        attn.qkv_layout = "fused"

    # == on values: signed zeros count as equal (the slot path's
    # slice-backward adds +0 to every element)
    assert bool((y_f == y_s).all()) and not torch.isnan(y_f).any()
    assert bool((dx_f == dx_s).all()) and not torch.isnan(dx_f).any()
    for n in g_s:
        if "norm" in n:
            torch.testing.assert_close(g_f[n].float(), g_s[n].float(),
                                       rtol=DW_RTOL, atol=0.0)
        else:
            assert bool((g_f[n] == g_s[n]).all()), n
            assert not torch.isnan(g_f[n]).any(), n
