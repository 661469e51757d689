"""CPU checks of the per-token log-probs / entropy path (return_log_probs):
the torch-only twin against the reference's recorded outputs, the three
label-alignment modes, the ignore_index contract, and the public surface
(hip_causal_lm_loss / ForCausalLM.forward).

Golden: tests/golden/logprobs_golden.pt, written by make_logprobs_golden.py
from the reference's chunk_logprobs_function on CPU.

Tolerances. fp32 cases: rtol 2e-5 (the bound test_oracle_golden.py uses for
fp32 logits), atol 1e-6 for entries that are sums cancelling towards 0.
bf16 cases: EagerChunkLogProbs issues the reference's op sequence one for
one (same GEMM calls, bf16 temperature divide before the upcast, cast before
the backward divide, bf16 `+=` of dweight), so every output and both
gradients are asserted bit-equal; the 1-ulp allowance is not used.
"""

import os
import types

import pytest
import torch

from veomni_amd.ops.kernels import cross_entropy as ce

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "logprobs_golden.pt")
CASES = ["fp32_t1", "fp32_t07", "bf16_t1", "bf16_t07", "bf16_t07_shift"]


@pytest.fixture(scope="module")
def lpg():
    return torch.load(GOLDEN, map_location="cpu")


def _run_case(lpg, name, fn, dlp=True, dent=True):
    dt = name.split("_")[0]
    h = lpg[f"in/{dt}/hidden"].clone().requires_grad_(True)
    w = lpg[f"in/{dt}/weight"].clone().requires_grad_(True)
    shift = lpg["in/shift_labels"] if bool(lpg[f"case/{name}/use_shift"]) else None
    lp, ent = fn(h, w, lpg["in/labels"], chunk_size=int(lpg["meta/chunk_size"]),
                 ignore_index=int(lpg["meta/ignore_index"]), shift_labels=shift,
                 temperature=float(lpg[f"case/{name}/temperature"]))
    outs, grads = [], []
    if dlp:
        outs.append(lp), grads.append(lpg["in/dlog_probs"])
    if dent:
        outs.append(ent), grads.append(lpg["in/dentropy"])
    torch.autograd.backward(outs, grads)
    return lp.detach(), ent.detach(), h.grad, w.grad


@pytest.mark.parametrize("name", CASES)
def test_eager_twin_matches_reference_golden(lpg, name):
    got = _run_case(lpg, name, ce.eager_chunk_logprobs_function)
    keys = ["log_probs", "entropy", "dhidden", "dweight"]
    for k, g in zip(keys, got):
        want = lpg[f"case/{name}/{k}"]
        assert g.dtype == want.dtype and g.shape == want.shape, k
        if name.startswith("bf16"):
            assert torch.equal(g, want), (name, k, (g.float() - want.float()).abs().max())
        else:
            torch.testing.assert_close(g, want, rtol=2e-5, atol=1e-6, msg=lambda m: f"{name}/{k}: {m}")


def test_golden_covers_the_stated_cases(lpg):
    lab, ign = lpg["in/labels"], int(lpg["meta/ignore_index"])
    tgt = lab[:, 1:]
    inside = (tgt[0] == ign)
    assert inside.any() and not inside[-1], "ignored labels inside a row"
    assert (tgt[1, -3:] == ign).all(), "ignored labels at a row's end"
    assert {float(lpg[f"case/{c}/temperature"]) for c in CASES} == {1.0, 0.7}
    assert sum(bool(lpg[f"case/{c}/use_shift"]) for c in CASES) == 1
    assert os.path.getsize(GOLDEN) < 300 * 1024


# ------------------------------------------------------------------ alignment
def _dense(h, w, tgt, temperature=1.0, ign=-100):
    """Plain-autograd fp64 statement on already aligned inputs."""
    logits = (h.double() @ w.double().t()) / temperature
    logp = logits.log_softmax(-1)
    valid = tgt != ign
    lp = logp.gather(-1, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    ent = -(logp.exp() * logp).sum(-1)
    z = torch.zeros_like(lp)
    return torch.where(valid, lp, z), torch.where(valid, ent, z)


def _toy(seed=0, B=2, L=11, H=16, V=40):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, L, H, generator=g)
    w = torch.randn(V, H, generator=g) * 0.5
    lab = torch.randint(0, V, (B, L), generator=g)
    lab[0, 3] = -100
    lab[1, 7:] = -100
    return h, w, lab


def test_alignment_default_shifts_and_pads():
    h, w, lab = _toy()
    lp, ent = ce.eager_chunk_logprobs_function(h, w, lab, chunk_size=4)
    assert lp.shape == lab.shape and ent.shape == lab.shape
    assert lp.dtype == torch.float32 and ent.dtype == torch.float32
    want_lp, want_ent = _dense(h[:, :-1], w, lab[:, 1:])
    torch.testing.assert_close(lp[:, :-1].double(), want_lp, rtol=2e-5, atol=1e-6)
    torch.testing.assert_close(ent[:, :-1].double(), want_ent, rtol=2e-5, atol=1e-6)
    assert (lp[:, -1] == 0).all() and (ent[:, -1] == 0).all()     # the pad slot


def test_alignment_explicit_shift_labels_used_as_is():
    h, w, lab = _toy()
    shift = torch.roll(lab, 3, dims=1)
    lp, ent = ce.eager_chunk_logprobs_function(h, w, lab, chunk_size=4,
                                               shift_labels=shift)
    assert lp.shape == shift.shape
    want_lp, want_ent = _dense(h, w, shift)
    torch.testing.assert_close(lp.double(), want_lp, rtol=2e-5, atol=1e-6)
    torch.testing.assert_close(ent.double(), want_ent, rtol=2e-5, atol=1e-6)
    assert (ent[:, -1] != 0).any(), "no pad slot with explicit shift_labels"


def test_alignment_sp_uses_labels_unshifted(monkeypatch):
    monkeypatch.setattr(ce, "get_parallel_state",
                        lambda: types.SimpleNamespace(sp_enabled=True))
    h, w, lab = _toy()
    lab[1, -1] = 5
    lp, ent = ce.eager_chunk_logprobs_function(h, w, lab, chunk_size=4)
    assert lp.shape == lab.shape
    want_lp, want_ent = _dense(h, w, lab)
    torch.testing.assert_close(lp.double(), want_lp, rtol=2e-5, atol=1e-6)
    torch.testing.assert_close(ent.double(), want_ent, rtol=2e-5, atol=1e-6)
    assert lp[1, -1] != 0 and ent[1, -1] != 0, "no pad slot under SP"


# ------------------------------------------------------- ignore_index contract
def test_ignored_positions_exact_zero_and_zero_grad():
    h, w, lab = _toy()
    h.requires_grad_(True)
    w.requires_grad_(True)
    lp, ent = ce.eager_chunk_logprobs_function(h, w, lab, chunk_size=4,
                                               temperature=0.7)
    ign = torch.nn.functional.pad(lab[:, 1:] == -100, (0, 1), value=True)
    assert ign.any() and (~ign).any()
    assert (lp[ign] == 0).all() and (ent[ign] == 0).all()
    assert (lp[~ign] < 0).all() and (ent[~ign] > 0).all()
    (lp.sum() + 0.3 * ent.sum()).backward()
    # hidden position t feeds only output slot t: ignored slots get no gradient
    assert (h.grad[ign] == 0).all()
    assert (h.grad[~ign] != 0).any() and (w.grad != 0).any()


@pytest.mark.parametrize("which", ["log_probs", "entropy"])
def test_single_output_backward_matches_autograd(which):
    h, w, lab = _toy(seed=3)
    h.requires_grad_(True)
    w.requires_grad_(True)
    lp, ent = ce.eager_chunk_logprobs_function(h, w, lab, chunk_size=4,
                                               temperature=0.7)
    g = torch.Generator().manual_seed(9)
    up = torch.randn(lab.shape, generator=g)
    (lp if which == "log_probs" else ent).backward(up)

    h2 = h.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    d_lp, d_ent = _dense(h2[:, :-1], w2, lab[:, 1:], temperature=0.7)
    (d_lp if which == "log_probs" else d_ent).backward(up[:, :-1].double())
    # The twin's dlogits are fp32: each carries a few ulp of
    # |up| * p * (|log p| + H) <= ~3 * 3, i.e. <= ~2e-6 absolute, and a
    # gradient entry sums V = 40 (dhidden) or B*L = 20 (dweight) of them
    # weighted by |w| or |h| ~ 0.4..1: worst case 40 * 0.4 * 2e-6 = 3e-5.
    # A dropped or mis-signed term is O(0.1).
    torch.testing.assert_close(h.grad, h2.grad, rtol=2e-5, atol=3e-5)
    torch.testing.assert_close(w.grad, w2.grad, rtol=2e-5, atol=3e-5)


def test_no_upstream_gradient_returns_none():
    h, w, lab = _toy()
    h.requires_grad_(True)
    lp, ent = ce.EagerChunkLogProbs.apply(h, w, lab, 1.0, 4, -100)
    assert ce.EagerChunkLogProbs.backward(lp.grad_fn, None, None) == (None,) * 6
    assert ce.HipChunkLogProbs.backward(lp.grad_fn, None, None) == (None,) * 6


# --------------------------------------------------------------- public surface
def test_aux_output_dataclass_fields():
    import dataclasses

    from veomni_amd.model_outputs import FusedLinearAuxOutput

    assert [f.name for f in dataclasses.fields(FusedLinearAuxOutput)] == [
        "log_probs", "entropy", "distillation_losses", "student_mass", "teacher_mass"]
    out = FusedLinearAuxOutput()
    assert all(getattr(out, f.name) is None for f in dataclasses.fields(out))


def test_hip_causal_lm_loss_raises_on_teacher_tensors():
    h, w, lab = _toy()
    ids = torch.zeros(2, 11, 4, dtype=torch.int64)
    for kw in ({"teacher_topk_ids": ids},
               {"teacher_topk_log_probs": torch.zeros(2, 11, 4)},
               {"teacher_topk_ids": ids, "teacher_topk_log_probs": torch.zeros(2, 11, 4),
                "return_log_probs": True}):
        with pytest.raises(NotImplementedError):
            ce.hip_causal_lm_loss(hidden_states=h, weights=w, labels=lab, **kw)


def test_hip_causal_lm_loss_routes_the_flag(monkeypatch):
    """return_log_probs reaches the log-probs function with every argument;
    the device function itself is covered by tests/test_gpu_logprobs.py."""
    from veomni_amd.model_outputs import FusedLinearAuxOutput

    seen = {}

    def fake(hidden_states, weights, labels, **kw):
        seen.update(kw)
        return "LP", "ENT"

    monkeypatch.setattr(ce, "hip_chunk_logprobs_function", fake)
    h, w, lab = _toy()
    loss, logits, aux = ce.hip_causal_lm_loss(
        hidden_states=h, weights=w, labels=lab, return_log_probs=True,
        temperature=0.7, shift_labels=lab, chunk_size=8)
    assert loss is None and logits is None
    assert isinstance(aux, FusedLinearAuxOutput)
    assert (aux.log_probs, aux.entropy) == ("LP", "ENT")
    assert seen == {"chunk_size": 8, "ignore_index": -100, "shift_labels": lab,
                    "temperature": 0.7}
    seen.clear()
    ce.hip_causal_lm_loss(hidden_states=h, weights=w, labels=lab,
                          return_log_probs=True)
    assert seen["chunk_size"] == 1024 and seen["temperature"] == 1.0


def test_vlm_forward_passes_the_flag_through():
    """VLForCausalLM.forward hands its kwargs to ForCausalLM.forward."""
    from veomni_amd.data import synthetic_vlm_batch
    from veomni_amd.model_outputs import FusedLinearAuxOutput
    from veomni_amd.models import build_vl_model
    from veomni_amd.models.modeling import bind_ops

    bind_ops("eager")
    torch.manual_seed(0)
    m = build_vl_model("tiny-vl", dtype=torch.float32, device="cpu")
    b = synthetic_vlm_batch(m.vl_config, 96, seed=1, device="cpu")
    out = m(**b, return_log_probs=True, temperature=0.7)
    assert isinstance(out, FusedLinearAuxOutput)
    assert out.log_probs.shape == b["labels"].shape
    ign = torch.nn.functional.pad(b["labels"][:, 1:] == -100, (0, 1), value=True)
    assert ign.any() and (out.log_probs[ign] == 0).all() and (out.entropy[ign] == 0).all()
    assert (out.log_probs[~ign] < 0).all()


def test_model_forward_returns_payload_under_eager():
    from veomni_amd.data import synthetic_batch
    from veomni_amd.model_outputs import FusedLinearAuxOutput
    from veomni_amd.models import build_model
    from veomni_amd.models.modeling import bind_ops

    bind_ops("eager")
    torch.manual_seed(0)
    m = build_model("tiny-moe", dtype=torch.float32, device="cpu")
    b = synthetic_batch(m.config.vocab_size, 24, batch=2, seed=0, device="cpu")
    b["labels"][0, 5:8] = -100

    loss, aux = m(**b)                              # the default call: unchanged
    assert loss.dim() == 0 and aux is not None

    out = m(**b, return_log_probs=True, temperature=0.7, chunk_size=16)
    assert isinstance(out, FusedLinearAuxOutput)
    assert out.log_probs.shape == b["labels"].shape == out.entropy.shape
    assert out.distillation_losses is None and out.student_mass is None
    assert (out.log_probs[0, 4:7] == 0).all() and (out.log_probs[:, -1] == 0).all()

    # at T = 1 the mean NLL over valid targets is the CE part of the loss
    out1 = m(**b, return_log_probs=True)
    n_valid = (b["labels"][:, 1:] != -100).sum()
    ce_loss = loss - m.config.router_aux_loss_coef * aux
    torch.testing.assert_close(-out1.log_probs.sum() / n_valid, ce_loss,
                               rtol=1e-5, atol=1e-6)
    out1.log_probs.sum().backward()
    assert m.lm_head.weight.grad is not None

    # explicit shift_labels: used as is, no pad slot
    out2 = m(**b, return_log_probs=True, shift_labels=b["labels"])
    assert (out2.log_probs[:, -1] != 0).all()
