"""GPU checks of the fused top-k forward-KL distillation path (pytest -m gpu):
vh_topk_kl_fwd / vh_topk_distill_bwd through hip_lib, HipChunkTopkDistill and
the model's teacher_topk_* forward, against fp64 restatements on the same
bf16 values and against the torch-only twin on the same device. Row kinds and
method are those of tests/test_gpu_logprobs.py, restated here.

Kernel-level tolerances, counted from vh_logprob.hip's operation chain.
Units: e = 2^-24 (half an fp32 ulp, relative), F = max|f| + ln V per row.

  s_k = f[i_k] - lse is a log-prob formed like log_probs, so it inherits
      tol_lp = (9 F + N) e,  N = ceil(V / 2048) + 3 + 45
  (the count in tests/test_gpu_logprobs.py: two exponent roundings 4 F e, the
  chain into s and v_exp_f32 (N + 1) e, logf / m + ln s / f - lse 4 F e).

  The K-term sums run per lane over k = lane, lane + 64, ... and then through
  6 shuffle levels: the longest addition chain is C = ceil(K / 64) + 6. expf
  here is the accurate one (1 ulp = 2 e). Nothing below the smallest normal
  fp32 number 2^-126 is representable: K 2^-126 is added to each bound.

  student_mass = sum exp(s_k): a term carries tol_lp (an absolute error of
      its exponent) + 2 e relative; the chain adds C e of the (all positive)
      partial sums                      -> sm (tol_lp + (2 + C) e)
  teacher_mass = sum exp(t_k), t exact  -> tm (2 + C) e
  distill = sum exp(t'_k) (t'_k - s'_k), d_k = t'_k - s'_k:
      exp 2 e, the subtraction e, the product e, relative to |term|; tol_lp
      of s'_k enters weighted by exp(t'_k); the chain adds C e of sum |term|
                                        -> sum_k exp(t'_k) (|d_k| (4 + C) e + tol_lp)
  max(x, c) is continuous: the clamp adds nothing to the forward bounds.

  dlogits = dlp (1[j==y] - p) - dent p ((f - lse) + H) + dd (M p - sparse_j):
      the first two terms as in tests/test_gpu_logprobs.py, with
      rel_p = (13 F + N + 1) e the relative error of p;
      M = sum w_k, w_k = exp(t'_k) [s_k >= c]: 2 e per term, a chain of
      C' = ceil(K / 256) + 6 + 3 adds (shuffles, then 3 LDS adds);
      M p: rel_p + e; sparse_j <= M: up to K terms of 2 e and K adds;
      the subtraction and the product by dd: 2 e. With p <= 1:
      |dd| M (rel_p + (C' + 2 K + 5) e)
  plus the one rounding to bf16, taken as 2^-8 relative. [s_k >= c] is not
  continuous: every case's clamp sits in a gap of the s_k values at least
  4 tol_lp wide, asserted, so kernel and reference agree on it.

Against torch on the same device (the twin's fp32 op sequence), in the same
tests: max error <= 2 * torch's max error + floor. The floor is one fp32 ulp
at the magnitude the output reaches: s_k is a difference of numbers up to F,
so 2^-23 F weighted as the output weights s_k (student_mass: by sm; distill:
by max(1, sum exp(t'_k))); teacher_mass, which sees no logit: 2^-23 tm; the
backward: one bf16 ulp (2^-8) of the largest |dlogits|.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

E24 = 2.0 ** -24
TINY = 2.0 ** -126
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
# (rows, V, K) -> the row kinds, cycled over the rows
SHAPES = {
    (5, 8, 3): ["rand0", "equal", "ignored", "peaked", "pm80"],   # one vector, idle lanes
    (7, 2056, 1): ALL_KINDS,                  # one block pass plus one vector; K = 1
    (7, 2056, 6): ALL_KINDS,                  # K below one wave
    (33, 4104, 256): ALL_KINDS,               # K above one wave, one block stride
    (3, 4104, 1024): ["rand0", "rand", "randlast"],               # K at the cap
    (3, 151936, 64): ["rand0", "peaked", "equal"],                # the real vocabulary
}
CLAMPS = [False, True]


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _teacher(x, lab, K, g):
    """Per row the top-K of log_softmax(row + noise) in fp32, then the forced
    entries: K >= 3: columns 0 and V-1 and one duplicate; K == 1: column 0,
    column V-1 or the top-1 by turns. rand0 rows (label 0) thereby carry an id
    equal to their label; with K >= 4 the last slot of every "rand" row is
    set to its label as well."""
    rows, V = x.shape
    noisy = (x.float().cpu() + torch.randn(rows, V, generator=g)).log_softmax(-1)
    tlp, ids = noisy.topk(K, dim=-1)
    ids, tlp = ids.clone(), tlp.clone()
    if K >= 3:
        ids[:, 0] = 0
        ids[:, 1] = V - 1
        ids[:, 2] = ids[:, 3] if K >= 4 else ids[:, 0]
    else:
        for r in range(rows):
            if r % 3 != 2:
                ids[r, 0] = 0 if r % 3 == 0 else V - 1
    if K >= 4:
        for r in range(rows):
            if int(lab[r]) not in (IGN, 0, V - 1):
                ids[r, K - 1] = int(lab[r])
    return ids, tlp


def _pick_clamp(s_valid):
    """The middle of the widest gap between neighbouring s_k values within
    the middle half of their sorted order, as an fp32 number; also the gap."""
    v = torch.sort(s_valid.flatten().double()).values
    n = v.numel()
    lo, hi = n // 4, max(n // 4 + 1, (3 * n) // 4)
    gaps = v[lo + 1:hi + 1] - v[lo:hi]
    i = int(torch.argmax(gaps))
    c = float(torch.tensor(float(v[lo + i] + v[lo + i + 1]) / 2, dtype=torch.float32))
    return c, float(gaps[i])


def _ref64(x, lab, ids, tlp, dlp, dent, dd, clamp):
    """fp64 restatement on the bf16 values (device tensors)."""
    f = x.double()
    valid = (lab != IGN)
    safe = lab.clamp(min=0).unsqueeze(-1)
    logp = f.log_softmax(-1)
    p = logp.exp()
    H = -(p * logp).sum(-1)
    s, t = logp.gather(-1, ids), tlp.double()
    sm, tm = s.exp().sum(-1), t.exp().sum(-1)
    sc, tc = (s, t) if clamp is None else (s.clamp_min(clamp), t.clamp_min(clamp))
    act = torch.ones_like(s) if clamp is None else (s >= clamp).double()
    term = tc.exp() * (tc - sc)
    dist = term.sum(-1)
    w = tc.exp() * act
    M = w.sum(-1)
    sparse = torch.zeros_like(p).scatter_add_(-1, ids, w)
    onehot = torch.zeros_like(p).scatter_(-1, safe, 1.0)
    vm = valid.double().unsqueeze(-1)
    g = (dlp.double().unsqueeze(-1) * (onehot - p)
         - dent.double().unsqueeze(-1) * p * (logp + H.unsqueeze(-1))
         + dd.double().unsqueeze(-1) * (M.unsqueeze(-1) * p - sparse)) * vm
    d = (f - f.max(-1, keepdim=True).values).abs()
    z = torch.zeros_like(H)
    return dict(dist=torch.where(valid, dist, z), sm=torch.where(valid, sm, z),
                tm=torch.where(valid, tm, z), g=g, s=s, valid=valid, M=M,
                abs_terms=term.abs().sum(-1), wsum=tc.exp().sum(-1),
                D1=(p * d).sum(-1),
                M2=(p * d * (logp + H.unsqueeze(-1)).abs()).sum(-1),
                F=f.abs().max(-1).values + math.log(x.shape[1]))


def _torch32(x, lab, ids, tlp, dlp, dent, dd, clamp):
    """The twin's fp32 op sequence on the device (no GEMM): the yardstick."""
    f = x.float()
    valid = lab != IGN
    safe = lab.clamp(min=0).unsqueeze(-1)
    logp = f.log_softmax(-1)
    probs = f.softmax(-1)
    H = torch.logsumexp(f, -1) - torch.sum(probs * f, -1)
    s = logp.gather(-1, ids)
    sm, tm = s.exp().sum(-1), tlp.exp().sum(-1)
    if clamp is None:
        sc, tc, w = s, tlp, tlp.exp()
    else:
        sc, tc = s.clamp_min(clamp), tlp.clamp_min(clamp)
        w = tc.exp() * (s >= clamp).float()
    dist = (tc.exp() * (tc - sc)).sum(-1)
    vm = valid.float()
    onehot = torch.zeros_like(probs).scatter_(-1, safe, 1.0)
    g = (dlp * vm).unsqueeze(-1) * (onehot - probs)
    g = g + probs * (logp + H.unsqueeze(-1)) * (-(dent * vm).unsqueeze(-1))
    sparse = torch.zeros_like(probs).scatter_add_(-1, ids, w)
    g = g + (dd * vm).unsqueeze(-1) * (-sparse + w.sum(-1, keepdim=True) * probs)
    z = torch.zeros_like(dist)
    return dict(dist=torch.where(valid, dist, z), sm=torch.where(valid, sm, z),
                tm=torch.where(valid, tm, z), g=g.to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def case(shape):
    """Device inputs plus the references without and with a clamp, once per
    shape. The clamp sits in a gap of the valid s_k values; two teacher
    log-probs are then moved so that it binds on some teacher entries too."""
    rows, V, K = shape
    g = torch.Generator().manual_seed(977 * rows + V + 31 * K)
    kinds = [SHAPES[shape][r % len(SHAPES[shape])] for r in range(rows)]
    built = [_row(k, V, g) for k in kinds]
    x = torch.stack([b[0] for b in built]).to(torch.bfloat16)
    lab = torch.tensor([b[1] for b in built], dtype=torch.int64)
    ids, tlp = _teacher(x, lab, K, g)
    assert int(ids.min()) >= 0 and int(ids.max()) < V      # nothing out of range
    x, lab, ids, tlp = x.cuda(), lab.cuda(), ids.cuda(), tlp.cuda()
    dlp = torch.randn(rows, generator=g).cuda()
    dent = torch.randn(rows, generator=g).cuda()
    dd = torch.randn(rows, generator=g).cuda()
    valid = lab != IGN
    s64 = x.double().log_softmax(-1).gather(-1, ids)
    clamp, gap = _pick_clamp(s64[valid])
    vr = [r for r in range(rows) if bool(valid[r])]
    tlp[vr[0], 0] = clamp - 1.0                           # binds on the teacher here
    tlp[vr[-1], K - 1] = min(clamp + 0.5, -0.01)           # and not here
    out = dict(x=x, lab=lab, ids=ids, tlp=tlp, dlp=dlp, dent=dent, dd=dd,
               kinds=kinds, clamp=clamp, gap=gap)
    for c in (None, clamp):
        out["ref", c is not None] = _ref64(x, lab, ids, tlp, dlp, dent, dd, c)
        out["t32", c is not None] = _torch32(x, lab, ids, tlp, dlp, dent, dd, c)
    return out


def _chain(V):
    return math.ceil(V / 2048) + 3 + 45


def _tol_lp(ref, V):
    return (9 * ref["F"] + _chain(V)) * E24


def _clamp_of(c, use_clamp):
    return c["clamp"] if use_clamp else None


def test_shapes_cover_the_stated_cases():
    for shape in SHAPES:
        rows, V, K = shape
        c = case(shape)
        ids, lab = c["ids"], c["lab"]
        valid = lab != IGN
        assert (ids == 0).any() and (ids == V - 1).any()
        assert ((ids == lab.unsqueeze(-1)).any(-1) & valid).any(), shape
        if K >= 3:
            dup = torch.tensor([len(set(r.tolist())) < K for r in ids.cpu()])
            assert dup.all(), shape
        # the clamp binds on some but not all entries, student and teacher
        # side, and no s_k is within reach of it
        s, t = c["ref", True]["s"][valid], c["tlp"][valid]
        assert (s < c["clamp"]).any() and (s >= c["clamp"]).any(), shape
        assert (t < c["clamp"]).any() and (t >= c["clamp"]).any(), shape
        tol = float(_tol_lp(c["ref", True], V)[valid].max())
        assert float((s - c["clamp"]).abs().min()) > 2 * tol, (shape, c["gap"], tol)
    seen = {k for s in SHAPES for k in case(s)["kinds"]}
    assert seen == set(ALL_KINDS)


# ------------------------------------------------------------ kernel: forward
@pytest.mark.parametrize("use_clamp", CLAMPS, ids=["noclamp", "clamp"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_kernel_forward_vs_fp64(shape, use_clamp):
    from veomni_amd.ops import hip_lib

    c = case(shape)
    rows, V, K = shape
    ref, t32 = c["ref", use_clamp], c["t32", use_clamp]
    clamp = _clamp_of(c, use_clamp)
    _, _, lse, _ = hip_lib.logprob_fwd(c["x"], c["lab"])
    dist, sm, tm = hip_lib.topk_kl_fwd(c["x"], c["lab"], lse, c["ids"], c["tlp"],
                                       log_prob_min_clamp=clamp)
    assert all(t.dtype == torch.float32 and t.shape == (rows,) for t in (dist, sm, tm))
    assert all(torch.isfinite(t).all() for t in (dist, sm, tm))
    C, F, tol_lp = math.ceil(K / 64) + 6, ref["F"], _tol_lp(ref, V)
    tols = {"sm": ref["sm"] * (tol_lp + (2 + C) * E24) + K * TINY,
            "tm": ref["tm"] * (2 + C) * E24 + K * TINY,
            "dist": ref["abs_terms"] * (4 + C) * E24 + ref["wsum"] * tol_lp + K * TINY}
    floors = {"sm": 2 * E24 * F * ref["sm"], "tm": 2 * E24 * ref["tm"],
              "dist": 2 * E24 * F * ref["wsum"].clamp(min=1.0)}
    v = ref["valid"]
    for name, got in (("sm", sm), ("tm", tm), ("dist", dist)):
        want, tol = ref[name], tols[name]
        err = (got.double() - want).abs()
        err_t = (t32[name].double() - want).abs()
        for r, kind in enumerate(c["kinds"]):
            print(f"fwd {_ids(shape)} clamp {clamp} row {r} {kind:8s} {name:4s} "
                  f"ref {float(want[r]): .9e} err_hip {float(err[r]):.3e} "
                  f"err_torch32 {float(err_t[r]):.3e} tol {float(tol[r]):.3e}")
        assert (err <= tol).all(), (name, err.tolist(), tol.tolist())
        assert float(err.max()) <= 2 * float(err_t.max()) + float(floors[name][v].max()), \
            (name, float(err.max()), float(err_t.max()), float(floors[name][v].max()))
        assert (got[~v] == 0).all()
    # the masses do not see the clamp
    d0, sm0, tm0 = hip_lib.topk_kl_fwd(c["x"], c["lab"], lse, c["ids"], c["tlp"])
    assert torch.equal(sm0, sm) and torch.equal(tm0, tm)
    assert use_clamp == (not torch.equal(d0, dist))


# ----------------------------------------------------------- kernel: backward
@pytest.mark.parametrize("use_clamp", CLAMPS, ids=["noclamp", "clamp"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_kernel_backward_vs_fp64(shape, use_clamp):
    from veomni_amd.ops import hip_lib

    c = case(shape)
    rows, V, K = shape
    ref, t32 = c["ref", use_clamp], c["t32", use_clamp]
    clamp = _clamp_of(c, use_clamp)
    _, _, lse, raw = hip_lib.logprob_fwd(c["x"], c["lab"])
    g = hip_lib.topk_distill_bwd(c["x"], c["lab"], lse, raw, c["ids"], c["tlp"],
                                 c["dlp"], c["dent"], c["dd"],
                                 log_prob_min_clamp=clamp)
    assert g.dtype == torch.bfloat16 and g.shape == c["x"].shape
    N, F = _chain(V), ref["F"]
    tol_ent = (3 * F + N + (2 * N + 4) * ref["D1"] + 4 * ref["M2"]) * E24
    rel_p = (13 * F + N + 1) * E24
    Cb = math.ceil(K / 256) + 6 + 3
    adlp, adent, add = (c[k].abs().double() for k in ("dlp", "dent", "dd"))
    tol_abs = (adlp * (rel_p + 2 * E24)
               + adent * (rel_p * F + 5 * F * E24 + tol_ent)
               + add * ref["M"] * (rel_p + (Cb + 2 * K + 5) * E24))
    want = ref["g"]
    err = (g.double() - want).abs()
    tol = 2.0 ** -8 * want.abs() + tol_abs.unsqueeze(-1)
    err_t = (t32["g"].double() - want).abs()
    for r, kind in enumerate(c["kinds"]):
        print(f"bwd {_ids(shape)} clamp {clamp} row {r} {kind:8s} "
              f"max|g| {float(want[r].abs().max()):.3e} err_hip {float(err[r].max()):.3e} "
              f"err_torch32 {float(err_t[r].max()):.3e} abs_term {float(tol_abs[r]):.3e}")
    assert (err <= tol).all(), float((err - tol).max())
    # the sparse columns one by one: every teacher column (duplicates among
    # them) and every label column, so a lost or doubled term cannot hide
    v = ref["valid"]
    safe = c["lab"].clamp(min=0).unsqueeze(-1)
    for name, cols in (("teacher", c["ids"]), ("label", safe)):
        e_c, t_c = err.gather(-1, cols)[v], tol.gather(-1, cols)[v]
        print(f"bwd {_ids(shape)} clamp {clamp} {name} columns: max err {float(e_c.max()):.3e} "
              f"max |want| {float(want.gather(-1, cols)[v].abs().max()):.3e}")
        assert (e_c <= t_c).all(), (name, float((e_c - t_c).max()))
    if K >= 3:
        dup_cols = c["ids"][:, 2:3]           # slot 2 repeats slot 3 (or slot 0)
        assert (err.gather(-1, dup_cols)[v] <= tol.gather(-1, dup_cols)[v]).all()
        # the duplicated column carries both weights: dropping one would show.
        # A result off by `lost` is at least lost - tol from the reference
        # when the rest is within tol, so lost > 2 tol is what detection needs
        if not use_clamp:
            w = c["tlp"].double().exp()
            other = 3 if K >= 4 else 0
            lost = (c["dd"].double() * w[:, other]).abs()[v]
            moved = lost > 2 * (tol.gather(-1, dup_cols).squeeze(-1)[v])
            assert moved.any(), "no row on which a lost duplicate term exceeds the tolerance"
    floor = 2.0 ** -8 * float(want.abs().max())
    assert float(err.max()) <= 2 * float(err_t.max()) + floor
    assert (g[~v] == 0).all()


# ------------------------------------------------------------ bit-exact checks
@pytest.mark.parametrize("T", [1.0, 0.7])
def test_null_ddistill_is_logprob_bwd_and_equals_zero_ddistill(T):
    from veomni_amd.ops import hip_lib

    c = case((33, 4104, 256))
    x, lab, ids, tlp = c["x"], c["lab"], c["ids"], c["tlp"]
    _, _, lse, raw = hip_lib.logprob_fwd(x, lab, temperature=T)
    base = hip_lib.logprob_bwd(x, lab, lse, raw, c["dlp"], c["dent"], T)
    for clamp in (None, c["clamp"]):
        none = hip_lib.topk_distill_bwd(x, lab, lse, raw, ids, tlp, c["dlp"],
                                        c["dent"], None, T, clamp)
        zero = hip_lib.topk_distill_bwd(x, lab, lse, raw, ids, tlp, c["dlp"],
                                        c["dent"], torch.zeros_like(c["dd"]), T, clamp)
        assert torch.equal(none, base)
        assert torch.equal(zero, base), float((zero.float() - base.float()).abs().max())
    only = hip_lib.topk_distill_bwd(x, lab, lse, raw, ids, tlp, None, None, c["dd"], T)
    zeros = torch.zeros_like(c["dd"])
    assert torch.equal(only, hip_lib.topk_distill_bwd(x, lab, lse, raw, ids, tlp,
                                                      zeros, zeros, c["dd"], T))
    assert (only[lab != IGN] != 0).any()


@pytest.mark.parametrize("shape", [(33, 4104, 256), (3, 151936, 64)], ids=_ids)
def test_two_runs_bit_identical(shape):
    from veomni_amd.ops import hip_lib

    c = case(shape)
    args = (c["x"], c["lab"])
    _, _, lse, raw = hip_lib.logprob_fwd(*args, temperature=0.7)
    a = hip_lib.topk_kl_fwd(*args, lse, c["ids"], c["tlp"], 0.7, c["clamp"])
    b = hip_lib.topk_kl_fwd(*args, lse, c["ids"], c["tlp"], 0.7, c["clamp"])
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    ga = hip_lib.topk_distill_bwd(*args, lse, raw, c["ids"], c["tlp"], c["dlp"],
                                  c["dent"], c["dd"], 0.7, c["clamp"])
    gb = hip_lib.topk_distill_bwd(*args, lse, raw, c["ids"], c["tlp"], c["dlp"],
                                  c["dent"], c["dd"], 0.7, c["clamp"])
    assert torch.equal(ga, gb)


@pytest.mark.parametrize("shape", [(7, 2056, 6), (33, 4104, 256), (3, 151936, 64)], ids=_ids)
def test_temperature_matches_torch_division_on_device(shape):
    """The T = 0.7 call equals the T = 1.0 call on x / 0.7 (torch, bf16, on
    the device), with a / 0.7 on the backward."""
    from veomni_amd.ops import hip_lib

    c = case(shape)
    T = 0.7
    scaled = c["x"] / T
    assert scaled.dtype == torch.bfloat16
    # a clamp for the scaled logits, clear of their s_k
    s = scaled.double().log_softmax(-1).gather(-1, c["ids"])[c["lab"] != IGN]
    clamp, _ = _pick_clamp(s)
    sa = hip_lib.logprob_fwd(c["x"], c["lab"], temperature=T)
    sb = hip_lib.logprob_fwd(scaled, c["lab"], temperature=1.0)
    for cl in (None, clamp):
        a = hip_lib.topk_kl_fwd(c["x"], c["lab"], sa[2], c["ids"], c["tlp"], T, cl)
        b = hip_lib.topk_kl_fwd(scaled, c["lab"], sb[2], c["ids"], c["tlp"], 1.0, cl)
        for name, u, v in zip(("distill", "student_mass", "teacher_mass"), a, b):
            assert torch.equal(u, v), (name, float((u - v).abs().max()))
        ga = hip_lib.topk_distill_bwd(c["x"], c["lab"], sa[2], sa[3], c["ids"], c["tlp"],
                                      c["dlp"], c["dent"], c["dd"], T, cl)
        gb = hip_lib.topk_distill_bwd(scaled, c["lab"], sb[2], sb[3], c["ids"], c["tlp"],
                                      c["dlp"], c["dent"], c["dd"], 1.0, cl) / T
        assert torch.equal(ga, gb), float((ga.float() - gb.float()).abs().max())
    one = hip_lib.topk_kl_fwd(c["x"], c["lab"], hip_lib.logprob_fwd(c["x"], c["lab"])[2],
                              c["ids"], c["tlp"])
    assert not torch.equal(one[0], a[0])


def test_every_row_ignored_and_dlogits_out():
    from veomni_amd.ops import hip_lib

    c = case((7, 2056, 6))
    x, ids, tlp = c["x"], c["ids"], c["tlp"]
    lab = torch.full((7,), IGN, dtype=torch.int64).cuda()
    _, _, lse, raw = hip_lib.logprob_fwd(x, lab)
    for t in hip_lib.topk_kl_fwd(x, lab, lse, ids, tlp, log_prob_min_clamp=-3.0):
        assert (t == 0).all()
    ones = torch.ones(7).cuda()
    buf = torch.ones_like(x)
    g = hip_lib.topk_distill_bwd(x, lab, lse, raw, ids, tlp, ones, ones, ones,
                                 dlogits_out=buf)
    assert g.data_ptr() == buf.data_ptr() and (g == 0).all()
    # valid rows: the result lands in the given buffer
    _, _, lse, raw = hip_lib.logprob_fwd(x, c["lab"])
    want = hip_lib.topk_distill_bwd(x, c["lab"], lse, raw, ids, tlp, c["dlp"],
                                    c["dent"], c["dd"])
    buf = torch.full_like(x, 7.0)
    g = hip_lib.topk_distill_bwd(x, c["lab"], lse, raw, ids, tlp, c["dlp"],
                                 c["dent"], c["dd"], dlogits_out=buf)
    assert g.data_ptr() == buf.data_ptr() and torch.equal(buf, want)
    with pytest.raises(AssertionError):
        hip_lib.topk_kl_fwd(x, c["lab"], lse, ids.to(torch.int32), tlp)


# -------------------------------------------------------------- function level
FT, FH, FV, FK, FCHUNK = 37, 64, 2056, 6, 16


@functools.lru_cache(maxsize=None)
def fcase():
    g = torch.Generator().manual_seed(4243)
    h = (torch.randn(FT, FH, generator=g)).to(torch.bfloat16)
    w = (torch.randn(FV, FH, generator=g) * 0.4).to(torch.bfloat16)
    lab = torch.randint(0, FV, (FT,), generator=g)
    lab[16:32] = IGN                          # the middle chunk fully ignored
    lab[3] = IGN
    lab[36] = FV - 1                          # the ragged last chunk (5 rows)
    noisy = (h.float() @ w.float().t() + torch.randn(FT, FV, generator=g)).log_softmax(-1)
    tlp, ids = noisy.topk(FK, dim=-1)
    ids, tlp = ids.clone(), tlp.clone()
    ids[:, 0], ids[:, 1] = 0, FV - 1
    ids[:, 2] = ids[:, 3]
    ids[5, 5] = lab[5]
    tlp[0, 4] = -30.0                         # below any clamp chosen below
    ups = [torch.randn(FT, generator=g).cuda() for _ in range(3)]
    return h.cuda(), w.cuda(), lab.cuda(), ids.cuda(), tlp.cuda(), ups


def _f64_function(h, w, lab, ids, tlp, ups, T, clamp):
    h64 = h.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    logp = ((h64 @ w64.t()) / T).log_softmax(-1)
    valid = lab != IGN
    lp = logp.gather(-1, lab.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    ent = -(logp.exp() * logp).sum(-1)
    s, t = logp.gather(-1, ids), tlp.double()
    sm, tm = s.exp().sum(-1), t.exp().sum(-1)
    if clamp is not None:
        s, t = s.clamp_min(clamp), t.clamp_min(clamp)
    dist = (t.exp() * (t - s)).sum(-1)
    z = torch.zeros_like(lp)
    outs = [torch.where(valid, o, z) for o in (lp, ent, dist, sm, tm)]
    torch.autograd.backward(outs[:3], [u.double() for u in ups])
    return [o.detach() for o in outs] + [h64.grad, w64.grad]


NAMES = ["log_probs", "entropy", "distill", "student_mass", "teacher_mass",
         "dhidden", "dweight"]


@pytest.mark.parametrize("use_clamp", CLAMPS, ids=["noclamp", "clamp"])
@pytest.mark.parametrize("T", [1.0, 0.7])
def test_function_hip_vs_eager_vs_fp64(T, use_clamp):
    from veomni_amd.ops.kernels import cross_entropy as ce

    h, w, lab, ids, tlp, ups = fcase()
    valid = lab != IGN
    clamp = None
    if use_clamp:
        # the fp64 logits differ from the GEMM's bf16 ones by up to 2^-9 |f|
        # each: keep every s_k further than that from the clamp
        s64 = ((h.double() @ w.double().t()) / T).log_softmax(-1).gather(-1, ids)[valid]
        clamp, gap = _pick_clamp(s64)
        fmax = float(((h.double() @ w.double().t()) / T).abs().max())
        assert gap / 2 > 2 * 2.0 ** -9 * fmax, (gap, fmax)
        assert (s64 < clamp).any() and (s64 >= clamp).any()
        assert (tlp[valid] < clamp).any() and (tlp[valid] >= clamp).any()
    want = _f64_function(h, w, lab, ids, tlp, ups, T, clamp)
    got = {}
    for name, fn in (("hip", ce.hip_chunk_topk_distill_function),
                     ("eager", ce.eager_chunk_topk_distill_function)):
        hh = h.clone().requires_grad_(True)
        ww = w.clone().requires_grad_(True)
        outs = fn(hh, ww, None, ids, tlp, chunk_size=FCHUNK, shift_labels=lab,
                  temperature=T, log_prob_min_clamp=clamp)
        assert all(o.shape == lab.shape and o.dtype == torch.float32 for o in outs)
        assert not outs[3].requires_grad and not outs[4].requires_grad
        torch.autograd.backward(list(outs[:3]), ups)
        assert hh.grad.dtype == torch.bfloat16 and ww.grad.dtype == torch.bfloat16
        got[name] = [o.detach() for o in outs] + [hh.grad, ww.grad]
    lnV = math.log(FV)
    fmax = float(((h.double() @ w.double().t()) / T).abs().max())
    F = fmax + lnV
    wsum = float(tlp.double().exp().sum(-1).max())
    floors = {"log_probs": 2 * E24 * F, "entropy": 2 * E24 * F,
              "distill": 2 * E24 * F * max(1.0, wsum),
              "student_mass": 2 * E24 * F * float(want[3].max()),
              "teacher_mass": 2 * E24 * float(want[4].max()),
              "dhidden": 2.0 ** -8 * float(want[5].abs().max()),
              "dweight": 2.0 ** -8 * float(want[6].abs().max())}
    for i, name in enumerate(NAMES):
        e_hip = float((got["hip"][i].double() - want[i]).abs().max())
        e_eager = float((got["eager"][i].double() - want[i]).abs().max())
        print(f"function T={T} clamp={clamp} {name:12s} err_hip {e_hip:.3e} "
              f"err_eager {e_eager:.3e} floor {floors[name]:.3e}")
        assert e_hip <= 2 * e_eager + floors[name], (name, e_hip, e_eager)
    ign = ~valid
    for t in got["hip"][:5]:
        assert (t[ign] == 0).all()
    assert (got["hip"][5][ign] == 0).all()


def test_function_alignment_modes_and_no_grad(monkeypatch):
    import types

    from veomni_amd.ops import hip_lib
    from veomni_amd.ops.kernels import cross_entropy as ce

    h, w, lab, ids, tlp, _ = fcase()
    h3 = h[:36].reshape(2, 18, FH)
    lab3 = lab[:36].reshape(2, 18).clone()
    lab3[:, -1] = 7
    ids3, tlp3 = ids[:36].reshape(2, 18, FK), tlp[:36].reshape(2, 18, FK)
    kw = dict(chunk_size=FCHUNK, temperature=0.7, log_prob_min_clamp=-4.0)
    fn = ce.hip_chunk_topk_distill_function
    # explicit shift_labels: used as is, no pad slot
    o_s = fn(h3, w, None, ids3, tlp3, shift_labels=lab3, **kw)
    assert all(o.shape == lab3.shape for o in o_s) and (o_s[2][:, -1] != 0).all()
    # default: labels[..., 1:] / teacher[..., 1:, :] against hidden[..., :-1, :]
    o_d = fn(h3, w, lab3, ids3, tlp3, **kw)
    o_x = fn(h3[:, :-1].contiguous(), w, None, ids3[:, 1:].contiguous(),
             tlp3[:, 1:].contiguous(), shift_labels=lab3[:, 1:].contiguous(), **kw)
    for d, x in zip(o_d, o_x):
        assert d.shape == lab3.shape and (d[:, -1] == 0).all()
        assert torch.equal(d[:, :-1], x)
    o_e = ce.eager_chunk_topk_distill_function(h3, w, lab3, ids3, tlp3, **kw)
    for d, e in zip(o_d, o_e):
        assert (d - e).abs().max() < 2e-4
    # log_probs / entropy are the log-probs path's, bit for bit
    lp, ent = ce.hip_chunk_logprobs_function(h3, w, lab3, chunk_size=FCHUNK,
                                             temperature=0.7)
    assert torch.equal(lp, o_d[0]) and torch.equal(ent, o_d[1])
    # SP: everything arrives shifted, no shift and no pad
    monkeypatch.setattr(ce, "get_parallel_state",
                        lambda: types.SimpleNamespace(sp_enabled=True))
    o_p = fn(h3, w, lab3, ids3, tlp3, **kw)
    for p, s in zip(o_p, o_s):
        assert torch.equal(p, s)
    monkeypatch.undo()
    # no-grad call: same values, nothing recorded
    hh = h3.clone().requires_grad_(True)
    with torch.no_grad():
        o_n = fn(hh, w, lab3, ids3, tlp3, **kw)
    assert all(o.grad_fn is None and not o.requires_grad for o in o_n)
    o_g = fn(hh, w, lab3, ids3, tlp3, **kw)
    assert o_g[2].requires_grad and not o_g[3].requires_grad and not o_g[4].requires_grad
    for a, b in zip(o_g, o_n):
        assert torch.equal(a, b)
    # only distill used: the other upstream gradients are absent, not zero
    o_g[2].sum().backward()
    assert hh.grad is not None and torch.isfinite(hh.grad).all() and (hh.grad != 0).any()
    # bf16 and int32 teacher tensors are upcast once
    o_b = fn(h3, w, lab3, ids3.to(torch.int32), tlp3.to(torch.bfloat16), **kw)
    o_f = fn(h3, w, lab3, ids3, tlp3.to(torch.bfloat16).float(), **kw)
    for a, b in zip(o_b, o_f):
        assert torch.equal(a, b)
    with pytest.raises(TypeError, match="bf16"):
        fn(h3.float(), w.float(), lab3, ids3, tlp3)
    K = hip_lib.TOPK_MAX + 1
    with pytest.raises(ValueError, match="eager"):
        fn(h3, w, lab3, torch.zeros(2, 18, K, dtype=torch.int64).cuda(),
           torch.zeros(2, 18, K).cuda())


# ----------------------------------------------------------------- model level
def test_model_topk_distill_hip_vs_eager():
    """Only the cross-entropy slot differs between the two runs, so both see
    the same hidden states and the same bf16 chunk logits (|f| + ln V < 32):
    each s_k differs by the two fp32 evaluations' own rounding, < 1e-4 (the
    argument of the log-probs model test). distill weights s_k by exp(t'_k)
    with teacher_mass <= 1, student_mass by exp(s_k) <= 1: both < 2e-4.
    teacher_mass sees no logit: K terms of one fp32 ulp of 1."""
    from veomni_amd.data import synthetic_batch
    from veomni_amd.model_outputs import FusedLinearAuxOutput
    from veomni_amd.models import build_model
    from veomni_amd.models.modeling import bind_ops

    K = 8
    torch.manual_seed(0)
    batch = synthetic_batch(512, 256, seed=3, device="cuda")
    batch["labels"][0, 40:60] = IGN
    g = torch.Generator().manual_seed(5)
    shape = tuple(batch["labels"].shape)
    tlp, ids = (torch.randn(*shape, 512, generator=g) * 3).log_softmax(-1).topk(K, dim=-1)
    kw = dict(return_log_probs=True, temperature=0.7, teacher_topk_ids=ids.cuda(),
              teacher_topk_log_probs=tlp.cuda(), log_prob_min_clamp=-8.0)
    bind_ops("eager")
    model = build_model("tiny-dense", dtype=torch.bfloat16, device="cuda")
    with torch.no_grad():
        ref = model(**batch, **kw)
    bind_ops({"cross_entropy_loss": "hip"})
    with torch.no_grad():
        out = model(**batch, **kw)
    assert isinstance(out, FusedLinearAuxOutput) and isinstance(ref, FusedLinearAuxOutput)
    for name in ("log_probs", "entropy", "distillation_losses", "student_mass",
                 "teacher_mass"):
        t = getattr(out, name)
        assert t.shape == batch["labels"].shape and t.dtype == torch.float32
        assert (t[0, 39:59] == 0).all() and (t[:, -1] == 0).all()
    assert float(ref.teacher_mass.max()) <= 1.0 + 1e-6
    d_dist = float((out.distillation_losses - ref.distillation_losses).abs().max())
    d_sm = float((out.student_mass - ref.student_mass).abs().max())
    d_tm = float((out.teacher_mass - ref.teacher_mass).abs().max())
    print("model hip-vs-eager max diff", d_dist, d_sm, d_tm)
    assert d_dist < 2e-4 and d_sm < 2e-4
    assert d_tm <= K * 2.0 ** -23
    assert (out.distillation_losses[0, :39] > 0).all()

    out1 = model(**batch, **kw)
    assert not out1.student_mass.requires_grad and not out1.teacher_mass.requires_grad
    out1.distillation_losses.sum().backward()
    gw = model.lm_head.weight.grad
    assert gw is not None and torch.isfinite(gw).all() and (gw != 0).any()
    with pytest.raises(ValueError, match="must be provided together"):
        model(**batch, return_log_probs=True, teacher_topk_ids=ids.cuda())
