"""GPU checks of the fused per-token log-probs / entropy path (pytest -m gpu):
vh_logprob_fwd / vh_logprob_bwd through hip_lib, HipChunkLogProbs and the
model's return_log_probs forward, against fp64 restatements on the same bf16
values and against the torch-only twin on the same device.

Kernel-level tolerances, counted from vh_logprob.hip's operation chain.
Units: e = 2^-24 (half an fp32 ulp, relative), F = max|f| + ln V per row
(|f|, |lse|, ln s, H <= F and |d| = |f - m| <= 2F).

  N(V) = ceil(V / 2048) + 3 + 45: the longest addition chain into s (or u):
      one add per 16-B vector a lane visits, 3 tree levels inside a vector,
      then 6 shuffle + 3 LDS merges of ~5 roundings each (two __expf, two
      products, one add). At V = 151936 N = 123. A relative error of s is
      an absolute error of ln s.

  log_probs = f_y - (m + ln s):
      d = f - m rounded once and __expf's d * log2(e) rounded once: each
      moves an exponent by <= e * 2F, hence lse by <= 2F e      -> 4 F e
      v_exp_f32 (1 ulp) and the chain into s                    -> (N + 1) e
      logf(s) (1 ulp of ln s <= F), m + ln s, f_y - lse (<= 2F) -> 4 F e
      tol_lp = (9 F + N) e            (9 rounds 8 + 1/F up)

  entropy = ln s - u / s, with D1 = sum p |d| (= |u| / s) and
  M2 = sum p |d| |log p + H|, both evaluated in fp64 from the inputs:
      ln s as above                                             -> (N + 1) e + F e
      u: the same chain plus one product per term; s again in the
      quotient; the division                                    -> (2N + 4) D1 e
      the two exponent roundings act through dH/df_j =
      -p_j (log p_j + H), each <= e * 2|d_j|                    -> 4 M2 e
      the final subtraction (H <= F)                            -> F e
      tol_ent = (3 F + N + (2N + 4) D1 + 4 M2) e
  D1 <= 2F and M2 <= 2F ln V, so this is c * e * F with a row-dependent c;
  D1 and M2 vanish on the all-equal, peaked and +-80 rows.

  dlogits = dlp (1[j==y] - p) - dent p ((f - lse) + H), p = exp(f - lse):
      p carries relative error rel_p = (13 F + N + 1) e: lse (9F + N), the
      subtraction (<= 2F), the log2(e) product (<= 2F), v_exp_f32 (1)
      dlp term: |dlp| (rel_p + 2e)       (p <= 1; subtract, multiply)
      dent term: p |log p + H| <= F, so |dent| (rel_p F + 5 F e + tol_ent)
      plus the one rounding to bf16, taken as 2^-8 relative.

Against torch on the same device (the twin's fp32 op sequence), in the same
tests: max error <= 2 * torch's max error + floor, floor = 2^-23 F (one fp32
ulp at the magnitude the outputs can reach) for the forward and one bf16 ulp
(2^-8) of the largest |dlogits| for the backward.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

E24 = 2.0 ** -24
IGN = -100


@pytest.fixture(autouse=True)
def _eager_after():
    yield
    from veomni_amd.models.modeling import bind_ops

    bind_ops("eager")


# ------------------------------------------------------------------ the rows
def _row(kind, V, g):
    """(bf16 row, label). Labels sit at column 0 or V-1 where noted."""
    if kind == "rand0":                       # sigma = 4, label at column 0
        return (torch.randn(V, generator=g) * 4), 0
    if kind == "randlast":                    # sigma = 4, label at column V-1
        return (torch.randn(V, generator=g) * 4), V - 1
    if kind == "rand":
        return (torch.randn(V, generator=g) * 4), int(torch.randint(0, V, (1,), generator=g))
    if kind == "ignored":
        return (torch.randn(V, generator=g) * 4), IGN
    if kind == "equal":                       # H = ln V, log p = -ln V
        return torch.full((V,), 1.5), V - 1
    if kind == "peaked":                      # one logit 30 above the rest
        r = torch.full((V,), -10.0)
        c = int(torch.randint(0, V, (1,), generator=g))
        r[c] = 20.0
        return r, c
    if kind == "pm80":                        # overflow safety
        r = torch.full((V,), 80.0)
        r[1::2] = -80.0
        return r, 1
    raise KeyError(kind)


ALL_KINDS = ["rand0", "equal", "ignored", "peaked", "pm80", "randlast", "rand"]
# (rows, V) -> the row kinds, cycled over the rows
SHAPES = {
    (5, 8): ["rand0", "equal", "ignored", "peaked", "pm80"],   # one vector, 255 idle lanes
    (3, 2048): ["pm80", "ignored", "randlast"],                # exactly one block pass
    (7, 2056): ALL_KINDS,                                      # one pass plus one vector
    (33, 4104): ALL_KINDS,
    (3, 151936): ["rand0", "peaked", "equal"],                 # the real vocabulary
}


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _ref64(x, lab, dlp, dent):
    """fp64 restatement on the bf16 values (device tensors)."""
    f = x.double()
    valid = (lab != IGN)
    safe = lab.clamp(min=0).unsqueeze(-1)
    logp = f.log_softmax(-1)
    p = logp.exp()
    H = -(p * logp).sum(-1)
    lp = logp.gather(-1, safe).squeeze(-1)
    onehot = torch.zeros_like(p).scatter_(-1, safe, 1.0)
    vm = valid.double().unsqueeze(-1)
    g = (dlp.double().unsqueeze(-1) * (onehot - p)
         - dent.double().unsqueeze(-1) * p * (logp + H.unsqueeze(-1))) * vm
    d = (f - f.max(-1, keepdim=True).values).abs()
    D1 = (p * d).sum(-1)
    M2 = (p * d * (logp + H.unsqueeze(-1)).abs()).sum(-1)
    z = torch.zeros_like(lp)
    return dict(lp=torch.where(valid, lp, z), ent=torch.where(valid, H, z), g=g,
                D1=D1, M2=M2, F=f.abs().max(-1).values + math.log(x.shape[1]),
                valid=valid)


def _torch32(x, lab, dlp, dent):
    """The twin's fp32 op sequence on the device (no GEMM): the yardstick."""
    f = x.float()
    valid = lab != IGN
    safe = lab.clamp(min=0).unsqueeze(-1)
    lp = f.log_softmax(-1).gather(-1, safe).squeeze(-1)
    probs = f.softmax(-1)
    H = torch.logsumexp(f, -1) - torch.sum(probs * f, -1)
    z = torch.zeros_like(lp)
    vm = valid.float()
    onehot = torch.zeros_like(probs).scatter_(-1, safe, 1.0)
    g = (dlp * vm).unsqueeze(-1) * (onehot - probs)
    g = g + probs * (f.log_softmax(-1) + H.unsqueeze(-1)) * (-(dent * vm).unsqueeze(-1))
    return torch.where(valid, lp, z), torch.where(valid, H, z), g.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def case(shape):
    """Device inputs plus both references, computed once per shape."""
    rows, V = shape
    g = torch.Generator().manual_seed(977 * rows + V)
    kinds = [SHAPES[shape][r % len(SHAPES[shape])] for r in range(rows)]
    built = [_row(k, V, g) for k in kinds]
    x = torch.stack([b[0] for b in built]).to(torch.bfloat16).cuda()
    lab = torch.tensor([b[1] for b in built], dtype=torch.int64).cuda()
    dlp = torch.randn(rows, generator=g).cuda()
    dent = torch.randn(rows, generator=g).cuda()
    return dict(x=x, lab=lab, dlp=dlp, dent=dent, kinds=kinds,
                ref=_ref64(x, lab, dlp, dent), t32=_torch32(x, lab, dlp, dent))


def _chain(V):
    return math.ceil(V / 2048) + 3 + 45


def _fwd_tols(ref, V):
    N, F = _chain(V), ref["F"]
    tol_lp = (9 * F + N) * E24
    tol_ent = (3 * F + N + (2 * N + 4) * ref["D1"] + 4 * ref["M2"]) * E24
    return tol_lp, tol_ent


def test_shapes_cover_every_row_kind():
    seen = {k for s in SHAPES for k in case(s)["kinds"]}
    assert seen == set(ALL_KINDS)
    labs = torch.cat([case(s)["lab"] for s in SHAPES]).tolist()
    assert 0 in labs and IGN in labs
    assert any(int(case(s)["lab"][i]) == s[1] - 1 for s in SHAPES for i in range(s[0]))


# ------------------------------------------------------------ kernel: forward
@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_kernel_forward_vs_fp64(shape):
    from veomni_amd.ops import hip_lib

    c = case(shape)
    ref, V = c["ref"], shape[1]
    lp, ent, lse, raw = hip_lib.logprob_fwd(c["x"], c["lab"])
    assert all(t.dtype == torch.float32 and t.shape == (shape[0],)
               for t in (lp, ent, lse, raw))
    assert all(torch.isfinite(t).all() for t in (lp, ent, lse, raw))
    tol_lp, tol_ent = _fwd_tols(ref, V)
    floor = 2 * E24 * ref["F"]
    t_lp, t_ent, _ = c["t32"]
    for name, got, want, tol, t32 in (("log_probs", lp, ref["lp"], tol_lp, t_lp),
                                      ("entropy", ent, ref["ent"], tol_ent, t_ent)):
        err = (got.double() - want).abs()
        err_t = (t32.double() - want).abs()
        for r, kind in enumerate(c["kinds"]):
            print(f"fwd {_ids(shape)} row {r} {kind:8s} {name:9s} ref {float(want[r]): .9e} "
                  f"err_hip {float(err[r]):.3e} err_torch32 {float(err_t[r]):.3e} "
                  f"tol {float(tol[r]):.3e}")
        assert (err <= tol).all(), (name, err.tolist(), tol.tolist())
        assert float(err.max()) <= 2 * float(err_t.max()) + float(floor.max()), \
            (name, float(err.max()), float(err_t.max()), float(floor.max()))
    # the unmasked statistics: lse = f_y - log p, ent_raw = entropy on valid rows
    v = ref["valid"]
    assert torch.equal(raw[v], ent[v])
    f_y = c["x"].float().gather(-1, c["lab"].clamp(min=0).unsqueeze(-1)).squeeze(-1)
    assert torch.equal((f_y - lse)[v], lp[v])
    # ignored rows: exactly zero everywhere
    for t in (lp, ent, lse, raw):
        assert (t[~v] == 0).all()


def test_kernel_forward_closed_forms():
    """all-equal row: H = ln V and log p = -ln V; peaked row: H ~ 4e-7."""
    for shape in SHAPES:
        c = case(shape)
        V = shape[1]
        for r, kind in enumerate(c["kinds"]):
            if kind == "equal":
                assert abs(float(c["ref"]["ent"][r]) - math.log(V)) < 1e-12
                assert abs(float(c["ref"]["lp"][r]) + math.log(V)) < 1e-12
            if kind == "peaked" and V == 151936:
                assert 3e-7 < float(c["ref"]["ent"][r]) < 5e-7


# ----------------------------------------------------------- kernel: backward
@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_kernel_backward_vs_fp64(shape):
    from veomni_amd.ops import hip_lib

    c = case(shape)
    ref, V = c["ref"], shape[1]
    _, _, lse, raw = hip_lib.logprob_fwd(c["x"], c["lab"])
    g = hip_lib.logprob_bwd(c["x"], c["lab"], lse, raw, c["dlp"], c["dent"])
    assert g.dtype == torch.bfloat16 and g.shape == c["x"].shape
    N, F = _chain(V), ref["F"]
    _, tol_ent = _fwd_tols(ref, V)
    rel_p = (13 * F + N + 1) * E24
    adlp, adent = c["dlp"].abs().double(), c["dent"].abs().double()
    tol_abs = adlp * (rel_p + 2 * E24) + adent * (rel_p * F + 5 * F * E24 + tol_ent)
    want = ref["g"]
    err = (g.double() - want).abs()
    tol = 2.0 ** -8 * want.abs() + tol_abs.unsqueeze(-1)
    err_t = (c["t32"][2].double() - want).abs()
    for r, kind in enumerate(c["kinds"]):
        print(f"bwd {_ids(shape)} row {r} {kind:8s} max|g| {float(want[r].abs().max()):.3e} "
              f"err_hip {float(err[r].max()):.3e} err_torch32 {float(err_t[r].max()):.3e} "
              f"abs_term {float(tol_abs[r]):.3e}")
    assert (err <= tol).all(), float((err - tol).max())
    floor = 2.0 ** -8 * float(want.abs().max())
    assert float(err.max()) <= 2 * float(err_t.max()) + floor
    assert (g[~ref["valid"]] == 0).all()


# ------------------------------------------------------------ bit-exact checks
def test_every_row_ignored():
    from veomni_amd.ops import hip_lib

    x = (torch.randn(4, 2056) * 4).to(torch.bfloat16).cuda()
    lab = torch.full((4,), IGN, dtype=torch.int64).cuda()
    outs = hip_lib.logprob_fwd(x, lab)
    for t in outs:
        assert (t == 0).all()
    buf = torch.ones_like(x)
    g = hip_lib.logprob_bwd(x, lab, outs[2], outs[3], torch.ones(4).cuda(),
                            torch.ones(4).cuda(), dlogits_out=buf)
    assert g.data_ptr() == buf.data_ptr() and (g == 0).all()


@pytest.mark.parametrize("shape", [(33, 4104), (3, 151936)], ids=_ids)
def test_two_runs_bit_identical(shape):
    from veomni_amd.ops import hip_lib

    c = case(shape)
    a = hip_lib.logprob_fwd(c["x"], c["lab"], temperature=0.7)
    b = hip_lib.logprob_fwd(c["x"], c["lab"], temperature=0.7)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    ga = hip_lib.logprob_bwd(c["x"], c["lab"], a[2], a[3], c["dlp"], c["dent"], 0.7)
    gb = hip_lib.logprob_bwd(c["x"], c["lab"], a[2], a[3], c["dlp"], c["dent"], 0.7)
    assert torch.equal(ga, gb)


@pytest.mark.parametrize("shape", [(7, 2056), (33, 4104), (3, 151936)], ids=_ids)
def test_temperature_matches_torch_division_on_device(shape):
    """logits / T and dlogits / T as torch evaluates them in bf16 on the
    device: the kernel's inv_temperature form must be bit-identical."""
    from veomni_amd.ops import hip_lib

    c = case(shape)
    T = 0.7
    scaled = c["x"] / T                       # torch, bf16, on the device
    assert scaled.dtype == torch.bfloat16
    a = hip_lib.logprob_fwd(c["x"], c["lab"], temperature=T)
    b = hip_lib.logprob_fwd(scaled, c["lab"], temperature=1.0)
    for name, u, v in zip(("log_probs", "entropy", "lse", "ent_raw"), a, b):
        assert torch.equal(u, v), (name, float((u - v).abs().max()))
    ga = hip_lib.logprob_bwd(c["x"], c["lab"], a[2], a[3], c["dlp"], c["dent"], T)
    gb = hip_lib.logprob_bwd(scaled, c["lab"], b[2], b[3], c["dlp"], c["dent"], 1.0) / T
    assert torch.equal(ga, gb), float((ga.float() - gb.float()).abs().max())
    # T == 1.0 leaves the logits alone
    one = hip_lib.logprob_fwd(c["x"], c["lab"], temperature=1.0)
    assert not torch.equal(one[0], a[0])


def test_null_upstream_equals_zero_upstream():
    from veomni_amd.ops import hip_lib

    c = case((33, 4104))
    x, lab = c["x"], c["lab"]
    _, _, lse, raw = hip_lib.logprob_fwd(x, lab)
    zero = torch.zeros_like(c["dlp"])
    assert torch.equal(hip_lib.logprob_bwd(x, lab, lse, raw, None, c["dent"]),
                       hip_lib.logprob_bwd(x, lab, lse, raw, zero, c["dent"]))
    assert torch.equal(hip_lib.logprob_bwd(x, lab, lse, raw, c["dlp"], None),
                       hip_lib.logprob_bwd(x, lab, lse, raw, c["dlp"], zero))
    assert (hip_lib.logprob_bwd(x, lab, lse, raw, None, None) == 0).all()


def test_no_stats_forward_and_argument_checks():
    from veomni_amd.ops import hip_lib

    c = case((7, 2056))
    full = hip_lib.logprob_fwd(c["x"], c["lab"])
    lp, ent, lse, raw = hip_lib.logprob_fwd(c["x"], c["lab"], want_stats=False)
    assert lse is None and raw is None
    assert torch.equal(lp, full[0]) and torch.equal(ent, full[1])
    with pytest.raises(RuntimeError, match="V % 8"):
        hip_lib.logprob_fwd(c["x"][:, :2052].contiguous(), c["lab"])


# -------------------------------------------------------------- function level
FT, FH, FV, FCHUNK = 37, 64, 2056, 16


@functools.lru_cache(maxsize=None)
def fcase():
    g = torch.Generator().manual_seed(4242)
    h = (torch.randn(FT, FH, generator=g)).to(torch.bfloat16).cuda()
    w = (torch.randn(FV, FH, generator=g) * 0.4).to(torch.bfloat16).cuda()
    lab = torch.randint(0, FV, (FT,), generator=g)
    lab[16:32] = IGN                          # the middle chunk fully ignored
    lab[3] = IGN
    lab[36] = FV - 1                          # the ragged last chunk (5 rows)
    up_lp = torch.randn(FT, generator=g).cuda()
    up_ent = torch.randn(FT, generator=g).cuda()
    return h, w, lab.cuda(), up_lp, up_ent


def _f64_function(h, w, lab, up_lp, up_ent, T):
    h64 = h.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    logp = ((h64 @ w64.t()) / T).log_softmax(-1)
    valid = lab != IGN
    lp = logp.gather(-1, lab.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    ent = -(logp.exp() * logp).sum(-1)
    z = torch.zeros_like(lp)
    lp, ent = torch.where(valid, lp, z), torch.where(valid, ent, z)
    torch.autograd.backward([lp, ent], [up_lp.double(), up_ent.double()])
    return lp.detach(), ent.detach(), h64.grad, w64.grad


@pytest.mark.parametrize("T", [1.0, 0.7])
def test_function_hip_vs_eager_vs_fp64(T):
    from veomni_amd.ops.kernels import cross_entropy as ce

    h, w, lab, up_lp, up_ent = fcase()
    want = _f64_function(h, w, lab, up_lp, up_ent, T)
    got = {}
    for name, fn in (("hip", ce.hip_chunk_logprobs_function),
                     ("eager", ce.eager_chunk_logprobs_function)):
        hh = h.clone().requires_grad_(True)
        ww = w.clone().requires_grad_(True)
        lp, ent = fn(hh, ww, lab, chunk_size=FCHUNK, shift_labels=lab, temperature=T)
        assert lp.shape == lab.shape and lp.dtype == torch.float32
        torch.autograd.backward([lp, ent], [up_lp, up_ent])
        assert hh.grad.dtype == torch.bfloat16 and ww.grad.dtype == torch.bfloat16
        got[name] = (lp.detach(), ent.detach(), hh.grad, ww.grad)
    lnV = math.log(FV)
    fmax = float(((h.double() @ w.double().t()) / T).abs().max())
    floors = {"log_probs": 2 * E24 * (fmax + lnV), "entropy": 2 * E24 * (fmax + lnV),
              "dhidden": 2.0 ** -8 * float(want[2].abs().max()),
              "dweight": 2.0 ** -8 * float(want[3].abs().max())}
    for i, name in enumerate(("log_probs", "entropy", "dhidden", "dweight")):
        e_hip = float((got["hip"][i].double() - want[i]).abs().max())
        e_eager = float((got["eager"][i].double() - want[i]).abs().max())
        print(f"function T={T} {name:9s} err_hip {e_hip:.3e} err_eager {e_eager:.3e} "
              f"floor {floors[name]:.3e}")
        assert e_hip <= 2 * e_eager + floors[name], (name, e_hip, e_eager)
    ign = lab == IGN
    for t in got["hip"][:2]:
        assert (t[ign] == 0).all()
    assert (got["hip"][2][ign] == 0).all()


def test_function_alignment_modes_and_no_grad(monkeypatch):
    import types

    from veomni_amd.ops.kernels import cross_entropy as ce

    h, w, lab, _, _ = fcase()
    h3 = h[:36].reshape(2, 18, FH)
    lab3 = lab[:36].reshape(2, 18).clone()
    lab3[:, -1] = 7
    kw = dict(chunk_size=FCHUNK, temperature=0.7)
    # explicit shift_labels: used as is, no pad slot
    lp_s, ent_s = ce.hip_chunk_logprobs_function(h3, w, None, shift_labels=lab3, **kw)
    assert lp_s.shape == lab3.shape and (ent_s[:, -1] != 0).all()
    # default: labels[..., 1:] against hidden[..., :-1, :], one trailing 0
    lp_d, ent_d = ce.hip_chunk_logprobs_function(h3, w, lab3, **kw)
    assert lp_d.shape == lab3.shape
    assert (lp_d[:, -1] == 0).all() and (ent_d[:, -1] == 0).all()
    lp_x, ent_x = ce.hip_chunk_logprobs_function(
        h3[:, :-1].contiguous(), w, None, shift_labels=lab3[:, 1:].contiguous(), **kw)
    # the default mode is exactly that call on the shifted inputs
    assert torch.equal(lp_d[:, :-1], lp_x) and torch.equal(ent_d[:, :-1], ent_x)
    lp_e, ent_e = ce.eager_chunk_logprobs_function(h3, w, lab3, **kw)
    assert (lp_d - lp_e).abs().max() < 1e-4 and (ent_d - ent_e).abs().max() < 1e-4
    # SP: labels arrive shifted, no shift and no pad
    monkeypatch.setattr(ce, "get_parallel_state",
                        lambda: types.SimpleNamespace(sp_enabled=True))
    lp_p, ent_p = ce.hip_chunk_logprobs_function(h3, w, lab3, **kw)
    assert torch.equal(lp_p, lp_s) and torch.equal(ent_p, ent_s)
    monkeypatch.undo()
    # no-grad call: same values, nothing recorded
    hh = h3.clone().requires_grad_(True)
    with torch.no_grad():
        lp_n, ent_n = ce.hip_chunk_logprobs_function(hh, w, lab3, **kw)
    assert lp_n.grad_fn is None and not lp_n.requires_grad
    lp_g, ent_g = ce.hip_chunk_logprobs_function(hh, w, lab3, **kw)
    assert lp_g.requires_grad and torch.equal(lp_g, lp_n) and torch.equal(ent_g, ent_n)
    # only one output used: the other upstream gradient is absent, not zero
    ent_g.sum().backward()
    assert hh.grad is not None and torch.isfinite(hh.grad).all()
    with pytest.raises(TypeError, match="bf16"):
        ce.hip_chunk_logprobs_function(h3.float(), w.float(), lab3)


# ----------------------------------------------------------------- model level
def test_model_return_log_probs_hip_vs_eager():
    """Only the cross-entropy slot differs between the two runs, so both see
    the same hidden states and the same bf16 chunk logits (|f| + ln V < 32):
    the two fp32 evaluations differ by their own rounding, < 50 operations of
    2^-24 * 32 each -> 1e-4 absolute."""
    from veomni_amd.data import synthetic_batch
    from veomni_amd.model_outputs import FusedLinearAuxOutput
    from veomni_amd.models import build_model
    from veomni_amd.models.modeling import bind_ops

    torch.manual_seed(0)
    batch = synthetic_batch(512, 256, seed=3, device="cuda")
    batch["labels"][0, 40:60] = IGN
    bind_ops("eager")
    model = build_model("tiny-dense", dtype=torch.bfloat16, device="cuda")
    with torch.no_grad():
        ref = model(**batch, return_log_probs=True, temperature=0.7)
    bind_ops({"cross_entropy_loss": "hip"})
    with torch.no_grad():
        out = model(**batch, return_log_probs=True, temperature=0.7)
    assert isinstance(out, FusedLinearAuxOutput) and isinstance(ref, FusedLinearAuxOutput)
    assert out.log_probs.shape == batch["labels"].shape
    assert out.distillation_losses is None
    d_lp = float((out.log_probs - ref.log_probs).abs().max())
    d_ent = float((out.entropy - ref.entropy).abs().max())
    print("model hip-vs-eager max diff", d_lp, d_ent)
    assert d_lp < 1e-4 and d_ent < 1e-4
    assert (out.log_probs[0, 39:59] == 0).all() and (out.entropy[:, -1] == 0).all()

    # -sum(log p) / n_valid is the HipChunkCE loss (suite's hip-vs-eager bound)
    loss, aux = model(**batch)
    assert aux is None
    out1 = model(**batch, return_log_probs=True)
    n_valid = (batch["labels"][:, 1:] != IGN).sum()
    nll = float(-out1.log_probs.sum() / n_valid)
    assert abs(nll - float(loss)) / abs(float(loss)) < 2e-2, (nll, float(loss))
    out1.log_probs.sum().backward()
    assert model.lm_head.weight.grad is not None
