"""MI355X kernel parity tests (pytest -m gpu): every HIP kernel vs the CPU
oracle / fp32 torch references, at small sizes and with the edge cases the
reference tests (empty experts, ragged group sizes, duplicate routes)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import moe as omoe  # noqa: E402
from oracle import norms as onorms  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from veomni_amd.ops import hip_lib

    return hip_lib


def bf(x):
    return x.to(torch.bfloat16)


# ------------------------------------------------------------- token bookkeeping
def test_histogram_bitexact(lib, golden):
    for name in ("small", "tiny", "one_expert", "full"):
        idx = golden[f"scatter/{name}/expert_index"].cuda()
        E = int(golden[f"scatter/{name}/num_experts"])
        out = lib.expert_histogram(idx, E)
        assert torch.equal(out.cpu(), golden[f"scatter/{name}/histogram"]), name


def test_scatter_gather_vs_oracle(lib):
    torch.manual_seed(0)
    M, N, topk, E = 64, 128, 4, 8
    x = bf(torch.randn(M, N)).cuda()
    sel = torch.randint(0, E, (M, topk)).cuda()
    _, scatter_index = omoe.compute_expert_scatter_index(sel.cpu())
    scatter_index = scatter_index.cuda()
    out = lib.moe_scatter(x, scatter_index)
    ref = omoe.moe_scatter(x.cpu(), scatter_index.cpu())
    assert torch.equal(out.cpu(), ref)  # pure row copies: bit-exact
    g = lib.moe_gather(out, scatter_index)
    gref = omoe.moe_gather(ref, scatter_index.cpu())
    torch.testing.assert_close(g.cpu().float(), gref.float(), rtol=1e-2, atol=1e-2)


# ----------------------------------------------------------------- grouped GEMM
def _mk_groups(counts):
    cumsum = torch.tensor(counts).cumsum(0)
    return cumsum


@pytest.mark.parametrize("counts,N,K", [
    ([37, 0, 91, 128], 128, 64),       # ragged + empty group
    ([256, 256], 256, 128),            # aligned
    ([5, 1000, 3], 1536, 2048),        # skew at real widths
    ([64], 768, 2048),                 # single group, real fc1 shape
])
def test_group_gemm_nk_transb(lib, counts, N, K):
    torch.manual_seed(1)
    G = len(counts)
    rows = sum(counts)
    a = bf(torch.randn(rows, K) * 0.5).cuda()
    b = bf(torch.randn(G, N, K) * 0.5).cuda()
    cumsum = _mk_groups(counts).cuda()
    c = lib.group_gemm_nk(a, b, cumsum, trans_b=True)
    # fp32 reference per group
    start = 0
    for g in range(G):
        end = int(cumsum[g])
        if end == start:
            continue
        ref = (a[start:end].float() @ b[g].float().t())
        torch.testing.assert_close(c[start:end].float(), ref, rtol=2e-2, atol=2e-2)
        start = end


@pytest.mark.parametrize("counts,N,K", [
    ([37, 0, 91, 128], 64, 128),
    ([100, 400], 768, 1536),           # dgrad-like: B [K,N] with K=2I
])
def test_group_gemm_nk_notransb(lib, counts, N, K):
    torch.manual_seed(2)
    G = len(counts)
    rows = sum(counts)
    a = bf(torch.randn(rows, K) * 0.5).cuda()
    b = bf(torch.randn(G, K, N) * 0.5).cuda()
    cumsum = _mk_groups(counts).cuda()
    c = lib.group_gemm_nk(a, b, cumsum, trans_b=False)
    start = 0
    for g in range(G):
        end = int(cumsum[g])
        if end == start:
            continue
        ref = (a[start:end].float() @ b[g].float())
        torch.testing.assert_close(c[start:end].float(), ref, rtol=2e-2, atol=2e-2)
        start = end


@pytest.mark.parametrize("counts,M,N", [
    ([37, 0, 91, 60], 128, 64),
    ([300, 100], 1536, 2048),          # wgrad fc1 shape [G,2I,H]
])
def test_group_gemm_mn(lib, counts, M, N):
    torch.manual_seed(3)
    G = len(counts)
    rows = sum(counts)
    a = bf(torch.randn(rows, M) * 0.5).cuda()
    b = bf(torch.randn(rows, N) * 0.5).cuda()
    cumsum = _mk_groups(counts).cuda()
    c = lib.group_gemm_mn(a, b, cumsum, G)
    start = 0
    for g in range(G):
        end = int(cumsum[g])
        if end == start:
            assert torch.all(c[g] == 0), f"group {g} not zero-filled"
            continue
        ref = a[start:end].float().t() @ b[start:end].float()
        torch.testing.assert_close(c[g].float(), ref, rtol=2e-2, atol=2e-2)
        start = end


def test_group_gemm_asymmetric_layout(lib):
    """Transpose-detecting check (guide G9/G16): asymmetric B, M=N."""
    counts = [128]
    a = torch.zeros(128, 64)
    b = torch.zeros(1, 128, 64)
    for i in range(128):
        for j in range(64):
            b[0, i, j] = (i * 3 + j) % 7 - 3
    a[:, 0] = 1.0  # row r of C = b[:,0] broadcast? no: C[r,n] = sum_k a[r,k] b[n,k] = b[n,0]
    c = lib.group_gemm_nk(bf(a).cuda(), bf(b).cuda(), _mk_groups(counts).cuda(), trans_b=True)
    ref = a.float() @ b[0].float().t()
    torch.testing.assert_close(c.cpu().float(), ref, rtol=1e-3, atol=1e-3)


# ------------------------------------------------------------------ norms/rope
def test_rmsnorm_fwd_bwd(lib):
    torch.manual_seed(4)
    for T, H in [(64, 128), (67, 128), (33, 2048), (256, 4096)]:
        x = bf(torch.randn(T, H)).cuda()
        w = bf(torch.randn(H) * 0.1 + 1).cuda()
        y, rstd = lib.rmsnorm_fwd(x, w, 1e-6)
        ref = onorms.rms_norm(x.cpu(), w.cpu(), 1e-6)  # bf16 math, same order
        torch.testing.assert_close(y.cpu().float(), ref.float(), rtol=1e-2, atol=1e-2)
        dy = bf(torch.randn(T, H)).cuda()
        dx, dw = lib.rmsnorm_bwd(dy, x, w, rstd)
        rdx, rdw = onorms.rms_norm_bwd(dy.cpu().float(), x.cpu().float(), w.cpu().float(), 1e-6)
        torch.testing.assert_close(dx.cpu().float(), rdx, rtol=5e-2, atol=5e-2)
        # dw reference with the kernel's exact rounding: dw = sum dy * bf16(x*rs)
        # (forward downcasts x_hat to bf16 BEFORE the weight multiply, so the
        # exact autograd dw sees the rounded x_hat; the fp32 oracle does not)
        xh = (x.cpu().float() * rstd.cpu()[:, None]).to(torch.bfloat16).float()
        rdw_exact = (dy.cpu().float() * xh).sum(0)
        torch.testing.assert_close(dw.cpu(), rdw_exact, rtol=1e-2, atol=1e-2)
        torch.testing.assert_close(dw.cpu(), rdw, rtol=5e-2, atol=2e-1)


def test_rope_fwd_bwd(lib):
    torch.manual_seed(5)
    B, hq, hk, S, D = 2, 4, 2, 32, 64
    q = bf(torch.randn(B, hq, S, D)).cuda()
    k = bf(torch.randn(B, hk, S, D)).cuda()
    cos, sin = onorms.rope_cos_sin(D, S, 10000.0)
    cosb = bf(cos)[None].expand(B, S, D).contiguous().cuda()
    sinb = bf(sin)[None].expand(B, S, D).contiguous().cuda()
    qe, ke = lib.rope(q, k, cosb, sinb)
    rq2, rk2 = onorms.apply_rotary_pos_emb(q.cpu().float(), k.cpu().float(),
                                           cosb.cpu().float(), sinb.cpu().float(), unsqueeze_dim=1)
    torch.testing.assert_close(qe.cpu().float(), rq2, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(ke.cpu().float(), rk2, rtol=2e-2, atol=2e-2)
    # backward = negated sin: rope(rope(x)) with -sin returns x
    qb, kb = lib.rope(qe, ke, cosb, sinb, negate_sin=True)
    torch.testing.assert_close(qb.cpu().float(), q.cpu().float(), rtol=2e-2, atol=2e-2)


def test_silu_mul(lib):
    torch.manual_seed(6)
    g = bf(torch.randn(64, 256)).cuda()
    u = bf(torch.randn(64, 256)).cuda()
    out = lib.silu_mul(g, u)
    ref = onorms.silu_mul(g.cpu().float(), u.cpu().float())
    torch.testing.assert_close(out.cpu().float(), ref, rtol=2e-2, atol=2e-2)
    dy = bf(torch.randn(64, 256)).cuda()
    dg, du = lib.silu_mul_bwd(dy, g, u)
    gg = g.cpu().float().requires_grad_(True)
    uu = u.cpu().float().requires_grad_(True)
    onorms.silu_mul(gg, uu).backward(dy.cpu().float())
    torch.testing.assert_close(dg.cpu().float(), gg.grad, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(du.cpu().float(), uu.grad, rtol=3e-2, atol=3e-2)


# ------------------------------------------------------------------------- CE
def test_ce_fwd(lib):
    torch.manual_seed(7)
    rows, V = 33, 512
    logits = bf(torch.randn(rows, V) * 2).cuda()
    labels = torch.randint(0, V, (rows,)).cuda()
    labels[5] = -100
    num = int((labels != -100).sum())
    loss_rows, dlogits = lib.ce_fwd(logits, labels, 1.0 / num)
    lf = logits.cpu().float().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lf, labels.cpu(), ignore_index=-100,
                                            reduction="sum") / num
    ref.backward()
    torch.testing.assert_close(loss_rows.sum().cpu() / num, ref.detach(), rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(dlogits.cpu().float(), lf.grad, rtol=5e-2, atol=1e-3)


def test_ce_lowmem_matches_stash(lib, monkeypatch):
    """chunk_loss no-[T,V] streaming branch == dlogits-stash branch
    (seq-16384 configs exceed the 16 GiB stash limit)."""
    from veomni_amd.ops.kernels import cross_entropy as ce

    torch.manual_seed(3)
    B, T, H, V = 1, 640, 64, 512
    hid = bf(torch.randn(B, T, H)).cuda()
    w = bf(torch.randn(V, H) * 0.05).cuda()
    labels = torch.randint(0, V, (B, T)).cuda()
    labels[0, ::17] = -100

    def run():
        h = hid.clone().requires_grad_(True)
        ww = w.clone().requires_grad_(True)
        loss = ce.HipChunkCE.apply(h, ww, labels, 256)
        loss.backward()
        return loss.detach(), h.grad.clone(), ww.grad.clone()

    l_fast, gh_fast, gw_fast = run()
    monkeypatch.setattr(ce, "STASH_LIMIT_BYTES", 0)
    l_low, gh_low, gw_low = run()
    torch.testing.assert_close(l_low, l_fast, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(gh_low, gh_fast, rtol=2e-2, atol=1e-3)
    torch.testing.assert_close(gw_low.float(), gw_fast.float(), rtol=2e-2, atol=1e-3)


# ------------------------------------------------------------------ fused MoE
def test_fused_moe_vs_eager_bf16(lib, golden):
    """HIP fused path (weights before fc2) vs the reference's eager bf16
    output (golden) within the documented operator-ordering tolerance
    (ref tests/ops/test_fused_moe_split_vs_merged.py:30-38)."""
    from veomni_amd.ops.kernels.moe import HipFusedMoeFunction

    hidden = bf(golden["moe/hidden"]).cuda()
    gup = bf(golden["moe/gate_up_proj"]).cuda()
    down = bf(golden["moe/down_proj"]).cuda()
    top_i = golden["moe/top_i"].cuda()
    top_w = bf(golden["moe/top_w"]).cuda()
    # pad dims: toy golden has H=64, I=48 -> K=64 ok, N=2I=96 %16=0 ok
    out = HipFusedMoeFunction.apply(gup.shape[0], top_w, top_i, hidden, gup, down)
    ref = golden["moe/out_bf16"].float()
    torch.testing.assert_close(out.cpu().float(), ref, rtol=5e-2, atol=5e-2)


def test_fused_moe_fwd_bwd_vs_eager_gpu(lib):
    """HIP fused MoE (fwd+bwd) vs the eager per-expert loop run on GPU with
    identical bf16 weights — mirrors the reference's fused-vs-eager test."""
    from veomni_amd.models.modeling import Experts, ModelConfig
    from veomni_amd.ops.kernels.moe import HipFusedMoeFunction

    torch.manual_seed(8)
    cfg = ModelConfig(hidden_size=128, num_experts=8, num_experts_per_tok=2,
                      moe_intermediate_size=64, vocab_size=64)
    T = 96
    experts = Experts(cfg).cuda().to(torch.bfloat16)
    with torch.no_grad():
        experts.gate_up_proj.normal_(0, 0.05)
        experts.down_proj.normal_(0, 0.05)
    hidden = bf(torch.randn(T, 128) * 0.5).cuda()
    rw = torch.softmax(torch.randn(T, 8), -1)
    top_w, top_i = torch.topk(rw, 2, -1)
    top_w = bf(top_w / top_w.sum(-1, keepdim=True)).cuda()
    top_i = top_i.cuda()

    h1 = hidden.clone().requires_grad_(True)
    gup1 = experts.gate_up_proj.detach().clone().requires_grad_(True)
    down1 = experts.down_proj.detach().clone().requires_grad_(True)
    tw1 = top_w.clone().requires_grad_(True)
    out_hip = HipFusedMoeFunction.apply(8, tw1, top_i, h1, gup1, down1)
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


def test_group_gemm_nk8_ragged(lib):
    """Large-rows dispatch with an empty group and ragged tails, both B
    layouts. K = 96 is zero-padded to 128 by hip_lib, so the trans_b shapes
    (N 288 / K 128 and N 256 / K 2048) reach the persistent 256x256 nk256s
    kernel and the !trans_b shape (K < 1024) the 128x128 kernel. The 8-phase
    nk8 kernel is covered by test_group_gemm_nk8_notransb_wide."""
    torch.manual_seed(12)
    counts = [500, 0, 279, 333]
    G, rows = len(counts), sum(counts)
    cumsum = torch.tensor(counts).cumsum(0).cuda()
    for trans_b, N, K in [(True, 288, 96), (False, 288, 96), (True, 256, 2048)]:
        a = bf(torch.randn(rows, K) * 0.5).cuda()
        b = bf(torch.randn(G, N, K) * 0.5).cuda() if trans_b else bf(torch.randn(G, K, N) * 0.5).cuda()
        c = lib.group_gemm_nk(a, b, cumsum, trans_b=trans_b)
        start = 0
        for g in range(G):
            end = int(cumsum[g])
            if end == start:
                continue
            ref = a[start:end].float() @ (b[g].float().t() if trans_b else b[g].float())
            torch.testing.assert_close(c[start:end].float(), ref, rtol=3e-2, atol=3e-2,
                                       msg=lambda m: f"g={g} trans_b={trans_b} N={N} K={K}: {m}")
            start = end


def test_group_gemm_nk8_notransb_wide(lib):
    """!trans_b with K, N >= 1024 and rows >= 256*G is the one dispatch that
    reaches the 256x256 8-phase nk8 kernel: empty group, ragged tails, N a
    16-multiple but not a 256-multiple (partial last n-tile). Reference:
    per-group fp32 matmul on the device."""
    torch.manual_seed(14)
    counts = [500, 0, 279, 333]
    G, rows = len(counts), sum(counts)
    N, K = 1040, 1024
    cumsum = torch.tensor(counts).cumsum(0).cuda()
    a = bf(torch.randn(rows, K) * 0.5).cuda()
    b = bf(torch.randn(G, K, N) * 0.5).cuda()
    c = lib.group_gemm_nk(a, b, cumsum, trans_b=False)
    start = 0
    for g in range(G):
        end = int(cumsum[g])
        if end == start:
            continue
        ref = a[start:end].float() @ b[g].float()
        torch.testing.assert_close(c[start:end].float(), ref, rtol=3e-2, atol=3e-2,
                                   msg=lambda m: f"g={g}: {m}")
        start = end


def test_group_gemm_wgrad_transpose_path(lib):
    """Large-rows wgrad goes through transpose-pad + wg256; parity vs fp32
    per-group matmul with ragged + empty groups."""
    torch.manual_seed(13)
    counts = [1000, 0, 1500, 37, 1559]
    G, rows = len(counts), sum(counts)
    cumsum = torch.tensor(counts).cumsum(0).cuda()
    a = bf(torch.randn(rows, 1536) * 0.3).cuda()
    b = bf(torch.randn(rows, 2048) * 0.3).cuda()
    c = lib.group_gemm_mn(a, b, cumsum, G)
    start = 0
    for g in range(G):
        end = int(cumsum[g])
        if end == start:
            assert torch.all(c[g] == 0), f"group {g} not zero-filled"
            continue
        ref = a[start:end].float().t() @ b[start:end].float()
        torch.testing.assert_close(c[g].float(), ref, rtol=3e-2, atol=3e-2,
                                   msg=lambda m: f"group {g}: {m}")
        start = end


def test_flash_attention_pair_vs_autograd(lib):
    """In-repo flash fwd+bwd autograd pair (hip_flash slot) vs torch fp32
    autograd reference: causal, GQA, several shapes incl. non-diagonal S."""
    import math
    from veomni_amd.ops.kernels.attention import hip_flash_attention

    torch.manual_seed(5)
    for (B, Hq, Hkv, S) in [(1, 2, 1, 256), (2, 4, 2, 512)]:
        q = bf(torch.randn(B, Hq, S, 128) * 0.5).cuda().requires_grad_(True)
        k = bf(torch.randn(B, Hkv, S, 128) * 0.5).cuda().requires_grad_(True)
        v = bf(torch.randn(B, Hkv, S, 128) * 0.5).cuda().requires_grad_(True)
        do = bf(torch.randn(B, Hq, S, 128) * 0.5).cuda()
        scale = 1.0 / math.sqrt(128)
        out = hip_flash_attention(q, k, v, scale)
        out.backward(do)

        rep = Hq // Hkv
        qf = q.detach().float().requires_grad_(True)
        kf = k.detach().float().requires_grad_(True)
        vf = v.detach().float().requires_grad_(True)
        kk = kf.repeat_interleave(rep, dim=1)
        vv = vf.repeat_interleave(rep, dim=1)
        sc = torch.matmul(qf, kk.transpose(-1, -2)) * scale
        mask = torch.triu(torch.ones(S, S, dtype=torch.bool, device="cuda"), 1)
        p = torch.softmax(sc.masked_fill(mask, float("-inf")), dim=-1)
        oref = torch.matmul(p, vv)
        oref.backward(do.float())

        torch.testing.assert_close(out.float(), oref, rtol=0, atol=3e-2)
        for got, ref, nm in ((q.grad, qf.grad, "dq"), (k.grad, kf.grad, "dk"),
                             (v.grad, vf.grad, "dv")):
            m = ref.abs().max().item()
            err = (got.float() - ref).abs().max().item()
            assert err < 0.06 * max(m, 1.0), f"{nm}: max err {err} vs |ref|max {m}"


def test_flash_attention_varlen_packed(lib):
    """Packed 3-document batch through the HIP varlen path (doc_start/doc_end
    from cu_seqlens) vs per-document fp32 attention — fwd AND grads must
    bit-match document boundaries (no cross-document leakage).
    Ref: attention/flash.py:61-91, data_collator.py:50."""
    import math
    from veomni_amd.ops.kernels.attention import (docs_from_cu_seqlens,
                                                  hip_flash_attention)

    torch.manual_seed(11)
    S = 768
    # misaligned boundaries (not multiples of the 32/64/128 tile sizes)
    cu = torch.tensor([0, 200, 520, 768], dtype=torch.int32, device="cuda")
    ds, de = docs_from_cu_seqlens(cu, S)
    B, Hq, Hkv = 1, 4, 2
    q = bf(torch.randn(B, Hq, S, 128) * 0.5).cuda().requires_grad_(True)
    k = bf(torch.randn(B, Hkv, S, 128) * 0.5).cuda().requires_grad_(True)
    v = bf(torch.randn(B, Hkv, S, 128) * 0.5).cuda().requires_grad_(True)
    do = bf(torch.randn(B, Hq, S, 128) * 0.5).cuda()
    scale = 1.0 / math.sqrt(128)
    out = hip_flash_attention(q, k, v, scale, ds, de)
    out.backward(do)

    rep = Hq // Hkv
    for i in range(cu.numel() - 1):
        a, b = int(cu[i]), int(cu[i + 1])
        qf = q.detach()[:, :, a:b].float().requires_grad_(True)
        kf = k.detach()[:, :, a:b].float().requires_grad_(True)
        vf = v.detach()[:, :, a:b].float().requires_grad_(True)
        kk = kf.repeat_interleave(rep, dim=1)
        vv = vf.repeat_interleave(rep, dim=1)
        sc = torch.matmul(qf, kk.transpose(-1, -2)) * scale
        L = b - a
        mask = torch.triu(torch.ones(L, L, dtype=torch.bool, device="cuda"), 1)
        p = torch.softmax(sc.masked_fill(mask, float("-inf")), dim=-1)
        oref = torch.matmul(p, vv)
        oref.backward(do[:, :, a:b].float())
        torch.testing.assert_close(out[:, :, a:b].float(), oref,
                                   rtol=0, atol=3e-2)
        for got, ref, nm in ((q.grad[:, :, a:b], qf.grad, "dq"),
                             (k.grad[:, :, a:b], kf.grad, "dk"),
                             (v.grad[:, :, a:b], vf.grad, "dv")):
            m = ref.abs().max().item()
            err = (got.float() - ref).abs().max().item()
            assert err < 0.06 * max(m, 1.0), \
                f"doc {i} {nm}: max err {err} vs |ref|max {m}"


def test_attention_slot_varlen_vs_eager_model(lib):
    """Model-level packed batch: HIP ops (hip_flash core) vs eager on the
    same packed 3-doc batch — the collator's cu_seq_lens kwargs consumed
    end-to-end."""
    from veomni_amd.models import build_model
    from veomni_amd.models.modeling import bind_ops
    from veomni_amd.ops import HIP_OPS_CONFIG

    torch.manual_seed(3)
    model = build_model("tiny-d128", dtype=torch.bfloat16, device="cuda")
    model.eval()
    S = 512
    cu = torch.tensor([0, 150, 380, 512], dtype=torch.int32, device="cuda")
    ids = torch.randint(0, model.config.vocab_size, (1, S), device="cuda")
    pos = torch.cat([torch.arange(int(cu[i + 1]) - int(cu[i]), device="cuda")
                     for i in range(cu.numel() - 1)])[None]
    try:
        with torch.no_grad():
            bind_ops("eager")
            ref, _ = model(ids, position_ids=pos, cu_seq_lens_q=cu)
            bind_ops(HIP_OPS_CONFIG)
            got, _ = model(ids, position_ids=pos, cu_seq_lens_q=cu)
    finally:
        bind_ops("eager")
    torch.testing.assert_close(got.float(), ref.float(), rtol=5e-2, atol=5e-1)


def test_veadamw_vs_torch_fused(lib):
    """One-sweep HIP AdamW vs torch fused AdamW (both bf16 state), incl. the
    grad_scale (clip-fold) path."""
    from veomni_amd.optim import VeAdamW

    torch.manual_seed(7)
    shapes = [(128, 64), (264,), (16, 16, 8), (1024, 48)]
    base = [torch.randn(s) * 0.5 for s in shapes]
    pa = [bf(b.clone()).cuda().requires_grad_(True) for b in base]
    pb = [bf(b.clone()).cuda().requires_grad_(True) for b in base]
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    oa = VeAdamW(pa, **kw)
    ob = torch.optim.AdamW(pb, fused=True, **kw)
    for step in range(5):
        gs = [torch.randn_like(p) for p in pa]
        for a, b, g in zip(pa, pb, gs):
            a.grad = g.clone()
            b.grad = g.clone()
        if step >= 3:  # exercise the grad-scale fold on both
            sc = torch.full((), 2.0, device="cuda")
            oa.grad_scale = sc
            ob.grad_scale = sc
        oa.step()
        ob.step()
    for a, b, s in zip(pa, pb, shapes):
        torch.testing.assert_close(a.float(), b.float(), rtol=2e-2, atol=2e-2,
                                   msg=lambda m: f"shape {s}: {m}")


def test_veadamw_dtensor_params(lib):
    """VeAdamW must step DTensor-sharded (FSDP2-style) params through their
    local shards — the N>=2 bench path (1-rank mesh here)."""
    import torch.distributed as dist
    from veomni_amd.optim import VeAdamW

    if not dist.is_initialized():
        import os
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("gloo", rank=0, world_size=1)
    from torch.distributed.device_mesh import init_device_mesh
    from torch.distributed.tensor import Shard, distribute_tensor

    mesh = init_device_mesh("cuda", (1,))
    torch.manual_seed(9)
    full = bf(torch.randn(256, 64)).cuda()
    dt = torch.nn.Parameter(distribute_tensor(full.clone(), mesh, [Shard(0)]))
    plain = torch.nn.Parameter(full.clone())
    g = bf(torch.randn(256, 64)).cuda()
    dt.grad = distribute_tensor(g.clone(), mesh, [Shard(0)])
    plain.grad = g.clone()
    kw = dict(lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1)
    try:
        oa = VeAdamW([dt], **kw)
        ob = VeAdamW([plain], **kw)
        oa.step()
        ob.step()
        torch.testing.assert_close(dt.data.to_local(), plain.data, rtol=0, atol=0)
    finally:
        dist.destroy_process_group()
