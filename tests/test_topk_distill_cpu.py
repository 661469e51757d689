"""CPU checks of the top-k forward-KL distillation path (teacher_topk_ids /
teacher_topk_log_probs with return_log_probs): the torch-only twin against
the reference's recorded outputs, the alignment modes, the metrics-only
contract of the two masses, each gradient term on its own, gradcheck, and
ForCausalLM.forward under the eager binding.

Golden: tests/golden/topk_distill_golden.pt, written by
make_topk_distill_golden.py from the reference's chunk_topk_distill_function
on CPU.

Tolerances. fp32 cases: rtol 1e-5 / atol 1e-6. test_logprobs_cpu.py uses
rtol 2e-5 / atol 1e-6 for the same op sequence; the tighter of the two is
asserted here. bf16 cases: as in test_logprobs_cpu.py the twin issues the
reference's op sequence one for one (same GEMM calls, bf16 temperature divide
before the upcast, teacher clamp and teacher_mass in the teacher's dtype,
cast before the backward divide, bf16 `+=` of dweight), so all five outputs
and both gradients are asserted bit-equal.
"""

import os
import types

import pytest
import torch

from veomni_amd.ops.kernels import cross_entropy as ce

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "topk_distill_golden.pt")
CASES = ["fp32_t1", "fp32_t07", "bf16_t1", "bf16_t07", "fp32_t07_clamp",
         "bf16_t07_clamp", "bf16_t07_shift", "bf16_t07_clamp_tlpbf16"]
OUT_KEYS = ["log_probs", "entropy", "distill", "student_mass", "teacher_mass"]
IGN = -100


@pytest.fixture(scope="module")
def tkg():
    return torch.load(GOLDEN, map_location="cpu")


def _case_inputs(tkg, name):
    dt = name.split("_")[0]
    use_shift = bool(tkg[f"case/{name}/use_shift"])
    sfx = "_shift" if use_shift else ""
    tlp = tkg[f"in/teacher_lp{sfx}"]
    if bool(tkg[f"case/{name}/tlp_bf16"]):
        tlp = tlp.to(torch.bfloat16)
    return dict(
        h=tkg[f"in/{dt}/hidden"].clone().requires_grad_(True),
        w=tkg[f"in/{dt}/weight"].clone().requires_grad_(True),
        ids=tkg[f"in/teacher_ids{sfx}"], tlp=tlp,
        shift=tkg["in/shift_labels"] if use_shift else None,
        clamp=float(tkg["meta/clamp"]) if bool(tkg[f"case/{name}/use_clamp"]) else None,
        temperature=float(tkg[f"case/{name}/temperature"]))


@pytest.mark.parametrize("name", CASES)
def test_eager_twin_matches_reference_golden(tkg, name):
    c = _case_inputs(tkg, name)
    outs = ce.eager_chunk_topk_distill_function(
        c["h"], c["w"], tkg["in/labels"], c["ids"], c["tlp"],
        chunk_size=int(tkg["meta/chunk_size"]),
        ignore_index=int(tkg["meta/ignore_index"]), shift_labels=c["shift"],
        temperature=c["temperature"], log_prob_min_clamp=c["clamp"])
    torch.autograd.backward(list(outs[:3]), [tkg["in/dlog_probs"],
                                             tkg["in/dentropy"], tkg["in/ddistill"]])
    got = [t.detach() for t in outs] + [c["h"].grad, c["w"].grad]
    for k, g in zip(OUT_KEYS + ["dhidden", "dweight"], got):
        want = tkg[f"case/{name}/{k}"]
        assert g.dtype == want.dtype and g.shape == want.shape, k
        if name.startswith("bf16"):
            assert torch.equal(g, want), (name, k, (g.float() - want.float()).abs().max())
        else:
            torch.testing.assert_close(g, want, rtol=1e-5, atol=1e-6,
                                       msg=lambda m: f"{name}/{k}: {m}")


def test_golden_covers_the_stated_cases(tkg):
    lab, ign = tkg["in/labels"], int(tkg["meta/ignore_index"])
    tgt = lab[:, 1:]
    inside = (tgt[0] == ign)
    assert inside.any() and not inside[-1], "ignored labels inside a row"
    assert (tgt[1, -3:] == ign).all(), "ignored labels at a row's end"
    assert {float(tkg[f"case/{c}/temperature"]) for c in CASES} == {1.0, 0.7}
    assert sum(bool(tkg[f"case/{c}/use_shift"]) for c in CASES) == 1
    assert sum(bool(tkg[f"case/{c}/tlp_bf16"]) for c in CASES) == 1
    assert sum(bool(tkg[f"case/{c}/use_clamp"]) for c in CASES) >= 2
    ids = tkg["in/teacher_ids"][:, 1:]
    valid = tgt != ign
    dup = torch.tensor([[len(set(r.tolist())) < r.numel() for r in b] for b in ids])
    assert (dup & valid).any(), "a valid slot with a duplicated teacher id"
    assert ((ids == tgt.unsqueeze(-1)).any(-1) & valid).any(), \
        "a valid slot with a teacher id equal to its label"
    assert os.path.getsize(GOLDEN) < 512 * 1024
    # student_mass is not vanishing: the teacher sits on the student's support
    assert float(tkg["case/fp32_t1/student_mass"][:, :-1][valid].mean()) > 0.3


@pytest.mark.parametrize("name", [c for c in CASES if "clamp" in c])
def test_golden_clamp_binds_on_part_of_the_entries(tkg, name):
    """The clamp binds on 1/4..3/4 of the valid student entries and on some
    but not all teacher entries (re-derived from the fixture's inputs)."""
    c = _case_inputs(tkg, name)
    tgt = tkg["in/labels"][:, 1:]
    logits = c["h"].detach()[:, :-1] @ c["w"].detach().t()
    logits = (logits / c["temperature"]).float()
    s_k = logits.log_softmax(-1).gather(-1, c["ids"][:, 1:])
    valid = (tgt != IGN).unsqueeze(-1).expand_as(s_k)
    fs = float((s_k < c["clamp"])[valid].float().mean())
    ft = float((c["tlp"][:, 1:].float() < c["clamp"])[valid].float().mean())
    print(name, "student", fs, "teacher", ft)
    assert 0.25 <= fs <= 0.75 and 0.0 < ft < 1.0


# ------------------------------------------------------------- fp64 statement
def _dense(h, w, tgt, ids, tlp, temperature=1.0, clamp=None, ign=IGN):
    """Plain-autograd fp64 statement on already aligned inputs."""
    logits = (h.double() @ w.double().t()) / temperature
    logp = logits.log_softmax(-1)
    valid = tgt != ign
    lp = logp.gather(-1, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    ent = -(logp.exp() * logp).sum(-1)
    s_k, t_k = logp.gather(-1, ids), tlp.double()
    sm, tm = s_k.exp().sum(-1), t_k.exp().sum(-1)
    if clamp is not None:
        s_k, t_k = s_k.clamp_min(clamp), t_k.clamp_min(clamp)
    dist = (t_k.exp() * (t_k - s_k)).sum(-1)
    z = torch.zeros_like(lp)
    return tuple(torch.where(valid, t, z) for t in (lp, ent, dist, sm, tm))


def _toy(seed=0, B=2, L=11, H=16, V=40, K=4):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, L, H, generator=g)
    w = torch.randn(V, H, generator=g) * 0.5
    lab = torch.randint(0, V, (B, L), generator=g)
    lab[0, 3] = IGN
    lab[1, 7:] = IGN
    noisy = (h @ w.t() + torch.randn(B, L, V, generator=g)).log_softmax(-1)
    tlp, ids = noisy.topk(K, dim=-1)
    ids = ids.clone()
    ids[0, 5, 3] = ids[0, 5, 0]              # a duplicate
    ids[1, 2, 1] = lab[1, 2]                 # an id equal to the label (all modes)
    return h, w, lab, ids, tlp.clone()


# ------------------------------------------------------------------ alignment
def test_alignment_default_equals_explicit_shift_plus_pad():
    h, w, lab, ids, tlp = _toy()
    kw = dict(chunk_size=4, temperature=0.7, log_prob_min_clamp=-2.0)
    outs = ce.eager_chunk_topk_distill_function(h, w, lab, ids, tlp, **kw)
    ref = ce.eager_chunk_topk_distill_function(
        h[:, :-1].contiguous(), w, None, ids[:, 1:].contiguous(),
        tlp[:, 1:].contiguous(), shift_labels=lab[:, 1:].contiguous(), **kw)
    for o, r in zip(outs, ref):
        assert o.shape == lab.shape and o.dtype == torch.float32
        assert torch.equal(o[:, :-1], r)
        assert (o[:, -1] == 0).all()                              # the pad slot
    want = _dense(h[:, :-1], w, lab[:, 1:], ids[:, 1:], tlp[:, 1:], 0.7, -2.0)
    for o, x in zip(outs, want):
        torch.testing.assert_close(o[:, :-1].double(), x, rtol=2e-5, atol=1e-6)


def test_alignment_explicit_shift_labels_used_as_is():
    h, w, lab, ids, tlp = _toy()
    shift = torch.roll(lab, 3, dims=1)
    outs = ce.eager_chunk_topk_distill_function(h, w, lab, ids, tlp, chunk_size=4,
                                                shift_labels=shift)
    want = _dense(h, w, shift, ids, tlp)
    for o, x in zip(outs, want):
        assert o.shape == shift.shape
        torch.testing.assert_close(o.double(), x, rtol=2e-5, atol=1e-6)
    assert (outs[2][:, -1] != 0).any(), "no pad slot with explicit shift_labels"


def test_alignment_sp_uses_everything_unshifted(monkeypatch):
    monkeypatch.setattr(ce, "get_parallel_state",
                        lambda: types.SimpleNamespace(sp_enabled=True))
    h, w, lab, ids, tlp = _toy()
    lab[1, -1] = 5
    outs = ce.eager_chunk_topk_distill_function(h, w, lab, ids, tlp, chunk_size=4)
    want = _dense(h, w, lab, ids, tlp)
    for o, x in zip(outs, want):
        assert o.shape == lab.shape
        torch.testing.assert_close(o.double(), x, rtol=2e-5, atol=1e-6)
    assert all(o[1, -1] != 0 for o in outs), "no pad slot under SP"


# ------------------------------------------------------------ masses, masking
@pytest.mark.parametrize("shift", [False, True])
def test_masses_are_metrics_only(shift):
    h, w, lab, ids, tlp = _toy()
    h.requires_grad_(True)
    w.requires_grad_(True)
    outs = ce.eager_chunk_topk_distill_function(
        h, w, lab, ids, tlp, chunk_size=4, shift_labels=lab if shift else None)
    lp, ent, dist, sm, tm = outs
    assert lp.requires_grad and ent.requires_grad and dist.requires_grad
    assert not sm.requires_grad and not tm.requires_grad
    assert sm.grad_fn is None and tm.grad_fn is None
    with pytest.raises(RuntimeError, match="does not require grad"):
        sm.sum().backward()
    # the others still differentiate after that
    dist.sum().backward()
    assert h.grad is not None and (w.grad != 0).any()


def test_ignored_positions_exact_zero_and_zero_grad():
    h, w, lab, ids, tlp = _toy()
    h.requires_grad_(True)
    outs = ce.eager_chunk_topk_distill_function(h, w, lab, ids, tlp, chunk_size=4,
                                                temperature=0.7)
    ign = torch.nn.functional.pad(lab[:, 1:] == IGN, (0, 1), value=True)
    assert ign.any() and (~ign).any()
    for o in outs:
        assert (o[ign] == 0).all()
    lp, ent, dist, sm, tm = outs
    assert (dist[~ign] >= 0).all() and (sm[~ign] > 0).all() and (tm[~ign] > 0).all()
    (lp.sum() + 0.3 * ent.sum() + 0.7 * dist.sum()).backward()
    assert (h.grad[ign] == 0).all() and (h.grad[~ign] != 0).any()


# --------------------------------------------------------- one term at a time
@pytest.mark.parametrize("clamp", [None, -2.0])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["log_probs", "entropy", "distill"])
def test_single_output_backward_matches_autograd(which, clamp):
    h, w, lab, ids, tlp = _toy(seed=3)
    h.requires_grad_(True)
    w.requires_grad_(True)
    outs = ce.eager_chunk_topk_distill_function(
        h, w, lab, ids, tlp, chunk_size=4, temperature=0.7, log_prob_min_clamp=clamp)
    g = torch.Generator().manual_seed(9)
    up = torch.randn(lab.shape, generator=g)
    outs[which].backward(up)

    h2 = h.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    dense = _dense(h2[:, :-1], w2, lab[:, 1:], ids[:, 1:], tlp[:, 1:], 0.7, clamp)
    dense[which].backward(up[:, :-1].double())
    # the bound of test_logprobs_cpu.py's single-output test: fp32 dlogits a
    # few ulp of O(3) each, V = 40 / B*L = 20 of them per gradient entry;
    # the distillation term's dlogits are bounded by teacher_mass <= 1
    torch.testing.assert_close(h.grad, h2.grad, rtol=2e-5, atol=3e-5)
    torch.testing.assert_close(w.grad, w2.grad, rtol=2e-5, atol=3e-5)
    if which == 2 and clamp is not None:
        s_k = dense_s_k(h2, w2, ids)
        bound = (s_k < clamp)[(lab[:, 1:] != IGN)]
        assert bound.any() and not bound.all(), "the clamp binds on part of the entries"


def dense_s_k(h, w, ids):
    logp = ((h.detach()[:, :-1].double() @ w.detach().double().t()) / 0.7).log_softmax(-1)
    return logp.gather(-1, ids[:, 1:])


def test_no_upstream_gradient_returns_none():
    h, w, lab, ids, tlp = _toy()
    h.requires_grad_(True)
    ids2, tlp2 = ids.reshape(-1, 4), tlp.reshape(-1, 4)
    outs = ce.EagerChunkTopkDistill.apply(h, w, lab, ids2, tlp2, 1.0, 4, IGN, None)
    fn = outs[0].grad_fn
    assert ce.EagerChunkTopkDistill.backward(fn, None, None, None) == (None,) * 9
    assert ce.HipChunkTopkDistill.backward(fn, None, None, None) == (None,) * 9


@pytest.mark.parametrize("clamp", [None, -2.5])
def test_gradcheck_fp64(clamp):
    T, H, V, K = 5, 4, 16, 3
    g = torch.Generator().manual_seed(11)
    h = torch.randn(T, H, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(V, H, generator=g, dtype=torch.float64, requires_grad=True)
    lab = torch.tensor([3, IGN, 15, 0, 7])
    logp = (h.detach() @ w.detach().t() / 0.7).log_softmax(-1)
    tlp, ids = (logp + 0.5 * torch.randn(T, V, generator=g, dtype=torch.float64)
                ).log_softmax(-1).topk(K, dim=-1)
    ids = ids.clone()
    ids[2, 2] = ids[2, 0]
    ids[3, 1] = 0
    if clamp is not None:
        s_k = logp.gather(-1, ids)[lab != IGN]
        # finite differences (eps 1e-6) must not straddle the clamp
        assert float((s_k - clamp).abs().min()) > 1e-2
        assert (s_k < clamp).any() and (s_k >= clamp).any()

    def fn(hh, ww):
        lp, ent, dist, _, _ = ce.eager_chunk_topk_distill_function(
            hh, ww, None, ids, tlp, chunk_size=2, shift_labels=lab,
            temperature=0.7, log_prob_min_clamp=clamp)
        return lp, ent, dist

    assert torch.autograd.gradcheck(fn, (h, w), eps=1e-6, atol=1e-6, rtol=1e-5)


# --------------------------------------------------------------- public surface
def test_hip_function_rejects_k_above_the_cap_and_other_dtypes():
    from veomni_amd.ops import hip_lib

    h, w, lab, _, _ = _toy()
    K = hip_lib.TOPK_MAX + 1
    ids = torch.zeros(2, 11, K, dtype=torch.int64)
    with pytest.raises(ValueError, match="eager"):
        ce.hip_chunk_topk_distill_function(h.bfloat16(), w.bfloat16(), lab, ids,
                                           torch.zeros(2, 11, K))
    with pytest.raises(TypeError, match="bf16"):
        ce.hip_chunk_topk_distill_function(h, w, lab, ids[..., :4],
                                           torch.zeros(2, 11, 4))


def test_model_forward_returns_distillation_payload_under_eager():
    import dataclasses

    from veomni_amd.data import synthetic_batch
    from veomni_amd.model_outputs import FusedLinearAuxOutput
    from veomni_amd.models import build_model
    from veomni_amd.models.modeling import bind_ops

    bind_ops("eager")
    torch.manual_seed(0)
    m = build_model("tiny-moe", dtype=torch.float32, device="cpu")
    V, K = m.config.vocab_size, 5
    b = synthetic_batch(V, 24, batch=2, seed=0, device="cpu")
    b["labels"][0, 5:8] = IGN
    g = torch.Generator().manual_seed(1)
    tlp, ids = torch.randn(2, 24, V, generator=g).log_softmax(-1).topk(K, dim=-1)

    out = m(**b, return_log_probs=True, temperature=0.7, chunk_size=16,
            teacher_topk_ids=ids, teacher_topk_log_probs=tlp,
            log_prob_min_clamp=-12.0)
    assert isinstance(out, FusedLinearAuxOutput)
    ign = torch.nn.functional.pad(b["labels"][:, 1:] == IGN, (0, 1), value=True)
    assert ign[0, 4:7].all() and ign[:, -1].all()
    for f in dataclasses.fields(out):
        t = getattr(out, f.name)
        assert t is not None and t.shape == b["labels"].shape, f.name
        assert t.dtype == torch.float32 and (t[ign] == 0).all(), f.name
    assert (out.distillation_losses[~ign] >= 0).all()
    assert (out.student_mass[~ign] > 0).all() and (out.teacher_mass[~ign] > 0).all()
    assert not out.student_mass.requires_grad and not out.teacher_mass.requires_grad
    out.distillation_losses.sum().backward()
    assert m.lm_head.weight.grad is not None and (m.lm_head.weight.grad != 0).any()

    # log_probs / entropy are what the call without a teacher returns
    plain = m(**b, return_log_probs=True, temperature=0.7, chunk_size=16)
    assert plain.distillation_losses is None and plain.student_mass is None \
        and plain.teacher_mass is None
    assert torch.equal(plain.log_probs, out.log_probs)
    assert torch.equal(plain.entropy, out.entropy)

    for kw in ({"teacher_topk_ids": ids}, {"teacher_topk_log_probs": tlp}):
        with pytest.raises(ValueError, match="must be provided together"):
            m(**b, return_log_probs=True, **kw)
    # as in the reference the teacher kwargs matter only with return_log_probs
    loss, aux = m(**b, teacher_topk_ids=ids)
    assert loss.dim() == 0
