"""Flash-attention kernels, the paths their loops can take (pytest -m gpu):
masked and unmasked loop bodies in the forward, dkv and dq kernels, the
packed-varlen instantiation against the plain one on a single document,
probabilities that underflow f32 (the raw v_exp_f32 flushes them), misaligned
varlen boundaries together with the split bodies, and the scale > 0 check.

Everything goes through hip_flash_attention, i.e. what the model runs.
Reference: fp32 torch autograd on the device. Tolerances are those of
tests/test_gpu_kernels.py::test_flash_attention_pair_vs_autograd: output
atol = 3e-2; each gradient max error < 0.06 * max(|ref|max, 1).

Measured on one MI355X (parent = the commit before the loop bodies were
split): the single-document varlen call is bit-equal to the plain call on
out, dq, dk and dv, on the parent and on this commit."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
SCALE = 1.0 / math.sqrt(D)


@pytest.fixture(scope="module")
def lib():
    from veomni_amd.ops import hip_lib

    return hip_lib


def bf(x):
    return x.to(torch.bfloat16)


def _inputs(B, Hq, Hkv, S, seed, qk_std=0.5):
    g = torch.Generator().manual_seed(seed)
    q = bf(torch.randn(B, Hq, S, D, generator=g) * qk_std).cuda()
    k = bf(torch.randn(B, Hkv, S, D, generator=g) * qk_std).cuda()
    v = bf(torch.randn(B, Hkv, S, D, generator=g) * 0.5).cuda()
    do = bf(torch.randn(B, Hq, S, D, generator=g) * 0.5).cuda()
    return q, k, v, do


def _hip(q, k, v, do, scale=SCALE, ds=None, de=None):
    from veomni_amd.ops.kernels.attention import hip_flash_attention

    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = hip_flash_attention(q, k, v, scale, ds, de)
    out.backward(do)
    return out.detach(), q.grad, k.grad, v.grad


def _ref(q, k, v, do, scale=SCALE):
    """fp32 causal attention with autograd on one [a, b) slice or the whole."""
    rep = q.shape[1] // k.shape[1]
    S = q.shape[2]
    qf = q.float().requires_grad_(True)
    kf = k.float().requires_grad_(True)
    vf = v.float().requires_grad_(True)
    kk = kf.repeat_interleave(rep, dim=1)
    vv = vf.repeat_interleave(rep, dim=1)
    sc = torch.matmul(qf, kk.transpose(-1, -2)) * scale
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool, device=q.device), 1)
    p = torch.softmax(sc.masked_fill(mask, float("-inf")), dim=-1)
    oref = torch.matmul(p, vv)
    oref.backward(do.float())
    return oref.detach(), qf.grad, kf.grad, vf.grad


def _check(got, ref, tag=""):
    out, dq, dk, dv = got
    oref, dqr, dkr, dvr = ref
    for t in got:
        assert torch.isfinite(t.float()).all(), f"{tag}non-finite result"
    err_o = (out.float() - oref).abs().max().item()
    print(f"{tag}out max err {err_o:.3e}")
    torch.testing.assert_close(out.float(), oref, rtol=0, atol=3e-2)
    for g, r, nm in ((dq, dqr, "dq"), (dk, dkr, "dk"), (dv, dvr, "dv")):
        m = r.abs().max().item()
        err = (g.float() - r).abs().max().item()
        print(f"{tag}{nm} max err {err:.3e} |ref|max {m:.3e}")
        assert err < 0.06 * max(m, 1.0), \
            f"{tag}{nm}: max err {err} vs |ref|max {m}"


# S = 512 is the smallest length at which the forward's second 256-row q block
# sees full kv tiles and diagonal ones; dq (128-row blocks) and dkv (64-row
# strips) see both as well. The second shape adds the GQA fold in dkv.
@pytest.mark.parametrize("B,Hq,Hkv,S", [(1, 2, 1, 512), (2, 4, 2, 512)])
def test_both_bodies_vs_autograd(lib, B, Hq, Hkv, S):
    q, k, v, do = _inputs(B, Hq, Hkv, S, seed=31)
    _check(_hip(q, k, v, do), _ref(q, k, v, do))


def test_single_document_varlen_equals_plain(lib):
    """One packed document covering the whole sequence: the varlen
    instantiation always takes the masked arithmetic, the plain one takes the
    unmasked body on full tiles; the arithmetic is otherwise the same, so the
    results are bit-equal. docs_from_cu_seqlens returns (None, None) for a
    single document (plain causal covers it), which would compare the plain
    kernels with themselves; the per-token bounds it would otherwise produce
    for cu_seqlens = [0, 512] are therefore built directly."""
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens

    S = 512
    cu = torch.tensor([0, S], dtype=torch.int32, device="cuda")
    assert docs_from_cu_seqlens(cu, S) == (None, None)
    ds = torch.zeros(S, dtype=torch.int32, device="cuda")
    de = torch.full((S,), S, dtype=torch.int32, device="cuda")
    q, k, v, do = _inputs(1, 2, 1, S, seed=32)
    plain = _hip(q, k, v, do)
    packed = _hip(q, k, v, do, ds=ds, de=de)
    for a, b, nm in zip(plain, packed, ("out", "dq", "dk", "dv")):
        diff = (a.float() - b.float()).abs().max().item()
        print(f"{nm}: varlen vs plain max abs diff {diff:.3e}")
        assert torch.equal(a, b), f"{nm}: varlen != plain, max diff {diff}"


def test_underflowing_probabilities(lib):
    """q, k ~ 6 randn: computed in fp64 on the CPU, 56 % of the unmasked
    probabilities of these inputs are below 2^-126, which the raw exp2 flushes
    to zero (they add up to at most 8e-38 per row). Scores jump by far more
    than the defer-max threshold, so the forward's rescale branch runs as
    well."""
    q, k, v, do = _inputs(1, 2, 1, 256, seed=7, qk_std=6.0)
    _check(_hip(q, k, v, do), _ref(q, k, v, do))


def test_varlen_misaligned_with_split_bodies(lib):
    """Two documents, boundary at 200 (no multiple of 32 / 64 / 128 / 256):
    the lower-bound mask together with the masked / unmasked bodies, against
    per-document references."""
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens

    S = 512
    cu = torch.tensor([0, 200, S], dtype=torch.int32, device="cuda")
    ds, de = docs_from_cu_seqlens(cu, S)
    q, k, v, do = _inputs(1, 4, 2, S, seed=33)
    got = _hip(q, k, v, do, ds=ds, de=de)
    for i in range(cu.numel() - 1):
        a, b = int(cu[i]), int(cu[i + 1])
        sl = [t[:, :, a:b] for t in (q, k, v, do)]
        _check([t[:, :, a:b] for t in got], _ref(*sl), tag=f"doc {i} ")


@pytest.mark.parametrize("scale", [0.0, -SCALE])
def test_nonpositive_scale_rejected(lib, scale):
    """A softmax scale is positive: the entry point refuses anything else
    before any launch, so the output buffer it was given stays untouched."""
    q, k, v, _ = _inputs(1, 2, 1, 256, seed=34)
    o = torch.full_like(q, 7.0)
    lse = torch.full((1, 2, 256), 7.0, dtype=torch.float32, device="cuda")
    rc = lib.get_lib().vh_attn_fwd_bf16(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
        1, 2, 1, 256, scale, None, None)
    torch.cuda.synchronize()
    assert rc != 0
    assert b"scale" in lib.get_lib().vh_last_error()
    assert bool((o == 7.0).all()) and bool((lse == 7.0).all())
    with pytest.raises(RuntimeError, match="scale"):
        lib.attn_fwd(q, k, v, scale)
