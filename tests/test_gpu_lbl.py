"""GPU parity for the fused load-balancing-loss kernels (pytest -m gpu):
vh_lbl_fwd / vh_lbl_finish / vh_lbl_bwd through hip_lib and the "hip"
provider, against an fp64 CPU restatement of oracle/losses.py:65-93.

Tolerances. Counts are sums of integer weights and the selection acts on the
exact logits, so they are compared bit-for-bit. prob_sum / loss: rtol 2e-5
against fp64. The forward's fp32 accumulation chain at the shapes used here
is: <= 2 rows per lane (ceil(T / (P * rows_per_block)), reached at T=16449),
<= 6 in-wave combine adds, 15 cross-wave adds, then a double-precision finish;
each summand carries <= 16 ulp from __expf and the normalisation at |x| <= 8.
(2 + 6 + 15 + 16) * 2^-24 = 2.3e-6, inside the 2e-5 bound.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

UPSTREAM = 0.37


@pytest.fixture(autouse=True)
def _eager_after():
    yield
    from veomni_amd.models.modeling import bind_ops

    bind_ops("eager")


# ------------------------------------------------------------ fp64 reference
def ref_lbl(layers, top_k, mask=None):
    """fp64 CPU reference. Selection = stable descending sort of the upcast
    logits (largest first, ties to the lowest expert index). Returns
    (count, prob_sum, loss, coef, grads) with grads = d loss / d logits."""
    E = layers[0].shape[1]
    count = torch.zeros(E, dtype=torch.float64)
    prob_sum = torch.zeros(E, dtype=torch.float64)
    total = torch.zeros((), dtype=torch.float64)
    probs, weights = [], []
    for l in layers:
        x = l.detach().cpu().float()
        p = torch.softmax(x.double(), dim=-1)
        sel = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :top_k]
        if mask is not None:
            w = mask.detach().cpu().reshape(-1).double()
        else:
            w = torch.ones(x.shape[0], dtype=torch.float64)
        prob_sum += (p * w[:, None]).sum(dim=0)
        count.scatter_add_(0, sel.reshape(-1), w[:, None].expand(-1, top_k).reshape(-1))
        total = total + w.sum()
        probs.append(p)
        weights.append(w)
    if total == 0:
        coef = torch.zeros((), dtype=torch.float64)
    else:
        coef = E / (total * total)
    loss = torch.dot(count, prob_sum) * coef
    grads = [coef * w[:, None] * p * (count - (p * count).sum(dim=-1, keepdim=True))
             for p, w in zip(probs, weights)]
    return count, prob_sum, loss, coef, grads


def grid_logits(L, T, E, dtype, seed):
    """Tie-free rows: E distinct values from {-128..128}/16 (exact in bf16)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(L):
        idx = torch.rand(T, 257, generator=g).argsort(dim=1)[:, :E]
        out.append(((idx - 128).float() / 16).to(dtype))
    return out


# (L, T, E, k)
SHAPES = [
    (2, 1000, 128, 8),   # bench E and k; T no multiple of a block pass (64 rows)
    (1, 37, 60, 4),      # generic-E path, unaligned rows
    (2, 257, 256, 8),    # max E, one row past a 256 boundary
    (1, 5, 8, 8),        # k = E, fewer rows than lanes
    (4, 300, 64, 1),
    (1, 1, 128, 8),      # a single row
    (1, 8193, 128, 8),   # 129 blocks, the last one holding a single row
    # At E=128 one block pass covers 1024/16 = 64 rows and P is capped at
    # LBL_MAX_BLOCKS = 256, so one pass of the grid covers 16384 rows: at
    # T=16449 blocks 0 and 1 take two grid-stride iterations (block 1 with
    # one live row in its second), every other block one.
    (1, 16449, 128, 8),
]
DTYPES = [torch.bfloat16, torch.float32]


@functools.lru_cache(maxsize=None)
def grid_case(shape, dtype):
    """(cpu logits, fp64 reference), computed once per (shape, dtype)."""
    L, T, E, k = shape
    layers = grid_logits(L, T, E, dtype, seed=1000 + 7 * T + E)
    return layers, ref_lbl(layers, k)


def _ids(v):
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return str(v).replace("torch.", "")


def _close(actual, expected, rtol, atol=0.0):
    torch.testing.assert_close(actual.detach().cpu().double(), expected,
                               rtol=rtol, atol=atol)


def _grad_atol(coef, count):
    return 1e-5 * float(coef) * UPSTREAM * float(count.max())


# -------------------------------------------------------------- 1. golden
@pytest.mark.parametrize("masked", [False, True])
def test_lbl_reference_golden(golden, masked):
    from veomni_amd.ops.kernels.load_balancing_loss import hip_load_balancing_loss

    gl = tuple(golden[f"lbl/gate_logits_{i}"].cuda() for i in range(3))
    assert gl[0].dtype == torch.float32 and gl[0].shape == (48, 8)
    mask = golden["lbl/mask"].cuda() if masked else None
    loss = hip_load_balancing_loss(gl, 8, 2, mask)
    want = golden["lbl/loss_masked" if masked else "lbl/loss"]
    assert loss.dtype == torch.float32 and loss.dim() == 0
    print("golden", masked, float(loss), float(want))
    torch.testing.assert_close(loss.cpu(), want, rtol=2e-5, atol=0.0)


# --------------------------------------------------------- 2. grid parity
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_lbl_grid_forward(shape, dtype):
    from veomni_amd.ops import hip_lib

    layers, (count, prob_sum, loss, coef, _) = grid_case(shape, dtype)
    k = shape[3]
    dev = [l.cuda() for l in layers]
    g_loss, g_count, g_psum, g_coef = hip_lib.lbl_fwd(dev, k, None)
    print("grid fwd", shape, dtype, float(g_loss), float(loss),
          float((g_psum.cpu().double() / prob_sum - 1).abs().max()))
    assert torch.equal(g_count.cpu().double(), count)
    _close(g_psum, prob_sum, rtol=2e-5)
    _close(g_loss, loss, rtol=2e-5)
    _close(g_coef[0], coef, rtol=1e-6)


# ------------------------------------------------------------ 3. gradient
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_lbl_grid_gradient(shape, dtype):
    from veomni_amd.ops.kernels.load_balancing_loss import hip_load_balancing_loss

    layers, (count, _, loss, coef, grads) = grid_case(shape, dtype)
    E, k = shape[2], shape[3]
    dev = tuple(l.cuda().requires_grad_(True) for l in layers)
    out = hip_load_balancing_loss(dev, E, k)
    (UPSTREAM * out).backward()
    _close(out, loss, rtol=2e-5)
    rtol = 1e-5 if dtype == torch.float32 else 2.0 ** -7
    atol = _grad_atol(coef, count)
    for l, g in zip(dev, grads):
        assert l.grad is not None and l.grad.dtype == dtype
        err = (l.grad.cpu().double() - UPSTREAM * g).abs().max()
        print("grid bwd", shape, dtype, float(err), atol)
        _close(l.grad, UPSTREAM * g, rtol=rtol, atol=atol)


def test_lbl_frozen_layer_gets_no_grad():
    from veomni_amd.ops.kernels.load_balancing_loss import hip_load_balancing_loss

    shape = SHAPES[0]
    layers, (count, _, _, coef, grads) = grid_case(shape, torch.float32)
    a = layers[0].cuda().requires_grad_(True)
    b = layers[1].cuda()  # requires_grad=False
    out = hip_load_balancing_loss((a, b), shape[2], shape[3])
    (UPSTREAM * out).backward()
    assert b.grad is None
    _close(a.grad, UPSTREAM * grads[0], rtol=1e-5, atol=_grad_atol(coef, count))
    # the live layer's grad is the same as when both layers take grads
    a2 = layers[0].cuda().requires_grad_(True)
    b2 = layers[1].cuda().requires_grad_(True)
    (UPSTREAM * hip_load_balancing_loss((a2, b2), shape[2], shape[3])).backward()
    assert torch.equal(a.grad, a2.grad)


# ---------------------------------------------------------------- 4. mask
MASK_SHAPES = [(3, 4, 12, 8, 2), (2, 2, 640, 128, 8)]  # (L, B, S, E, k)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=_ids)
def test_lbl_masked(shape, dtype):
    from veomni_amd.ops import hip_lib
    from veomni_amd.ops.kernels.load_balancing_loss import hip_load_balancing_loss

    L, B, S, E, k = shape
    layers = grid_logits(L, B * S, E, dtype, seed=77 + S)
    mask = torch.ones(B, S, dtype=torch.int64)
    mask[:, S - S // 4:] = 0  # last quarter of each sequence masked
    count, prob_sum, loss, coef, grads = ref_lbl(layers, k, mask)

    dev = tuple(l.cuda().requires_grad_(True) for l in layers)
    mask_w = mask.cuda().reshape(-1).float()
    _, g_count, g_psum, _ = hip_lib.lbl_fwd([l.detach() for l in dev], k, mask_w)
    assert torch.equal(g_count.cpu().double(), count)
    _close(g_psum, prob_sum, rtol=2e-5)

    out = hip_load_balancing_loss(dev, E, k, mask.cuda())
    (UPSTREAM * out).backward()
    print("masked", shape, dtype, float(out.detach()), float(loss))
    _close(out, loss, rtol=2e-5)
    rtol = 1e-5 if dtype == torch.float32 else 2.0 ** -7
    dead = (mask.reshape(-1) == 0)
    for l, g in zip(dev, grads):
        _close(l.grad, UPSTREAM * g, rtol=rtol, atol=_grad_atol(coef, count))
        assert torch.count_nonzero(l.grad.cpu()[dead]) == 0


def test_lbl_all_zero_mask():
    from veomni_amd.ops.kernels.load_balancing_loss import hip_load_balancing_loss

    L, B, S, E, k = MASK_SHAPES[0]
    layers = grid_logits(L, B * S, E, torch.bfloat16, seed=5)
    dev = tuple(l.cuda().requires_grad_(True) for l in layers)
    out = hip_load_balancing_loss(dev, E, k, torch.zeros(B, S, dtype=torch.int64).cuda())
    out.backward()
    assert float(out.detach()) == 0.0
    for l in dev:
        assert torch.count_nonzero(l.grad) == 0


def test_lbl_mask_shape_mismatch():
    from veomni_amd.ops.kernels.load_balancing_loss import hip_load_balancing_loss

    layers = tuple(l.cuda() for l in grid_logits(2, 48, 8, torch.float32, seed=6))
    with pytest.raises(ValueError, match="Mismatch"):
        hip_load_balancing_loss(layers, 8, 2, torch.ones(4, 13).cuda())


# ------------------------------------------------------------ 5. tie rule
def test_lbl_ties_constant_rows():
    from veomni_amd.ops import hip_lib

    g = torch.Generator().manual_seed(11)
    x = (torch.randn(512, 1, generator=g) * 0.5).expand(512, 128).contiguous()
    _, count, psum, _ = hip_lib.lbl_fwd([x.bfloat16().cuda()], 8, None)
    want = torch.zeros(128)
    want[:8] = 512
    assert torch.equal(count.cpu(), want)
    _close(psum, torch.full((128,), 4.0, dtype=torch.float64), rtol=2e-5)


def test_lbl_ties_random_bf16():
    from veomni_amd.ops import hip_lib

    g = torch.Generator().manual_seed(12)
    x = (torch.randn(4096, 128, generator=g) * 0.5).bfloat16()
    k = 8
    srt = torch.sort(x.float(), dim=-1, descending=True).values
    assert int((srt[:, k - 1] == srt[:, k]).sum()) >= 1  # a tie at the k/k+1 cut
    count, prob_sum, loss, _, _ = ref_lbl([x], k)
    g_loss, g_count, g_psum, _ = hip_lib.lbl_fwd([x.cuda()], k, None)
    assert torch.equal(g_count.cpu().double(), count)
    _close(g_psum, prob_sum, rtol=2e-5)
    _close(g_loss, loss, rtol=2e-5)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_lbl_ties_signed_zero_and_neg_inf(dtype):
    """-0.0 ties with +0.0, and -inf logits are legal candidates (p = 0)
    that rank below every finite logit, lowest index first."""
    from veomni_amd.ops import hip_lib

    g = torch.Generator().manual_seed(13)
    vals = torch.tensor([float("-inf"), -0.0, 0.0, -1.0])
    k = 8
    for E in (128, 60):
        x = vals[torch.randint(0, 4, (300, E), generator=g)]
        x[:, 5] = 0.0          # no all--inf row
        x[:7, 6:] = float("-inf")  # rows with fewer than k finite logits
        x = x.to(dtype)
        count, prob_sum, loss, _, _ = ref_lbl([x], k)
        g_loss, g_count, g_psum, _ = hip_lib.lbl_fwd([x.cuda()], k, None)
        assert torch.equal(g_count.cpu().double(), count)
        _close(g_psum, prob_sum, rtol=2e-5)
        _close(g_loss, loss, rtol=2e-5)


# --------------------------------------------------------- 6. determinism
def test_lbl_forward_bit_reproducible():
    from veomni_amd.ops import hip_lib

    layers, _ = grid_case(SHAPES[-1], torch.bfloat16)
    dev = [l.cuda() for l in layers]
    a = hip_lib.lbl_fwd(dev, 8, None)
    b = hip_lib.lbl_fwd(dev, 8, None)
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u, v)


# -------------------------------------------------- 7. wiring through model
def test_lbl_bound_through_model():
    from veomni_amd.data import synthetic_batch
    from veomni_amd.models import build_model
    from veomni_amd.models import modeling
    from veomni_amd.models.modeling import bind_ops
    from veomni_amd.ops import HIP_OPS_CONFIG, hip_lib
    from veomni_amd.ops.kernels.load_balancing_loss import hip_load_balancing_loss

    torch.manual_seed(0)
    batch = synthetic_batch(512, 256, seed=3, device="cuda")
    model = build_model("tiny-moe", dtype=torch.bfloat16, device="cuda")
    E, k = model.config.num_experts, model.config.num_experts_per_tok

    bind_ops(HIP_OPS_CONFIG)
    with torch.no_grad():
        _, router_logits = model.model(batch["input_ids"],
                                       position_ids=batch["position_ids"])
    assert len(router_logits) == model.config.num_hidden_layers
    count, _, loss, _, _ = ref_lbl(list(router_logits), k)
    direct = hip_load_balancing_loss(router_logits, E, k, None)
    _, g_count, _, _ = hip_lib.lbl_fwd(list(router_logits), k, None)
    assert torch.equal(g_count.cpu().double(), count)
    _close(direct, loss, rtol=2e-5)

    bind_ops({**HIP_OPS_CONFIG, "load_balancing_loss": "hip"})
    assert modeling.veomni_load_balancing_loss.use_non_eager_impl
    captured = []
    hook = model.model.register_forward_hook(
        lambda mod, args, out: captured.append(tuple(r.detach() for r in out[1])))
    try:
        total, aux = model(**batch)
    finally:
        hook.remove()
    total.backward()
    want = hip_load_balancing_loss(captured[0], E, k, None)
    torch.testing.assert_close(aux.detach(), want, rtol=2e-5, atol=0.0)
    gates = [p for n, p in model.named_parameters() if n.endswith("gate.weight")]
    assert len(gates) == model.config.num_hidden_layers
    for p in gates:
        assert p.grad is not None
        assert bool(torch.isfinite(p.grad).all())
        assert int(torch.count_nonzero(p.grad)) > 0


# ----------------------------------------------------------- 8. error path
def test_lbl_rejects_out_of_contract_shapes():
    from veomni_amd.ops.kernels.load_balancing_loss import hip_load_balancing_loss

    wide = (torch.zeros(16, 512, dtype=torch.bfloat16, device="cuda"),)
    with pytest.raises(RuntimeError, match=r"vh_lbl_fwd failed.*E=512"):
        hip_load_balancing_loss(wide, 512, 2)
    small = (torch.zeros(16, 8, dtype=torch.float32, device="cuda"),)
    with pytest.raises(RuntimeError, match=r"vh_lbl_fwd failed.*top_k=9"):
        hip_load_balancing_loss(small, 8, 9)
