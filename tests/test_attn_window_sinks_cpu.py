"""Sliding-window attention and attention sinks, CPU side: the eager twin and
the attention slot's sdpa core against a golden recorded from the reference's
gpt-oss eager_attention_forward (tests/golden/make_attn_window_sinks_golden.py),
window_bounds against a brute-force mask, argument checks, the model
configuration, sync Ulysses on gloo, and the C ABI declarations.

Tolerances for the fp32 twins are those of tests/test_logprobs_cpu.py: rtol
2e-5, atol 1e-6 for forward values; gradients, which are sums that cancel
towards 0, rtol 2e-5 and atol 3e-5 (that file's bound for its gradients)."""

import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "attn_window_sinks_golden.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


def _cases(g):
    return sorted({k.split("/")[1] for k in g if k.startswith("case/")})


def _case(g, name):
    D = int(g[f"case/{name}/D"])
    W = int(g[f"case/{name}/W"])
    c = {k: g[f"in/d{D}/{k}"] for k in ("q", "k", "v", "do")}
    c["W"] = None if W < 0 else W
    c["sinks"] = g[f"in/d{D}/sinks"] if bool(g[f"case/{name}/use_sinks"]) else None
    c["scaling"] = float(g[f"case/{name}/scaling"])
    c["cu"] = g.get(f"case/{name}/cu_seqlens")
    for k in ("out", "dq", "dk", "dv", "dsinks"):
        c["want_" + k] = g.get(f"case/{name}/{k}")
    return c


def _compare(name, c, out, q, k, v, sinks):
    torch.testing.assert_close(out, c["want_out"], rtol=2e-5, atol=1e-6,
                               msg=lambda m: f"{name}/out: {m}")
    out.backward(c["do"])
    grads = [("dq", q.grad), ("dk", k.grad), ("dv", v.grad)]
    if sinks is not None:
        grads.append(("dsinks", sinks.grad))
    for nm, got in grads:
        torch.testing.assert_close(got, c["want_" + nm], rtol=2e-5, atol=3e-5,
                                   msg=lambda m: f"{name}/{nm}: {m}")


def _leaves(c):
    q, k, v = (c[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
    sinks = c["sinks"].clone().requires_grad_(True) if c["sinks"] is not None else None
    return q, k, v, sinks


def _docs(c):
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens

    if c["cu"] is None:
        return None, None
    return docs_from_cu_seqlens(c["cu"], c["q"].shape[2])


def test_golden_has_the_cases(golden):
    names = _cases(golden)
    assert {"window_d16", "sinks_d16", "both_d16", "both_docs_d16", "w1_d16",
            "both_d128", "both_docs_d128"} <= set(names), names
    assert os.path.getsize(GOLDEN) < (1 << 20)


def test_eager_twin_matches_reference_golden(golden):
    """modeling.sdpa_attention (the eager path of the model) with
    sliding_window / s_aux / doc bounds."""
    from veomni_amd.models.modeling import sdpa_attention

    for name in _cases(golden):
        c = _case(golden, name)
        q, k, v, sinks = _leaves(c)
        ds, de = _docs(c)
        out, _ = sdpa_attention(None, q, k, v, None, scaling=c["scaling"],
                                doc_start=ds, doc_end=de,
                                sliding_window=c["W"], s_aux=sinks)
        _compare(name, c, out, q, k, v, sinks)


def test_slot_sdpa_core_matches_reference_golden(golden):
    """hip_attention_forward: D = 16 and S % 256 != 0 take the sdpa core, and
    so does fp32; core="sdpa" says so explicitly."""
    from veomni_amd.ops.kernels.attention import hip_attention_forward

    for name in _cases(golden):
        c = _case(golden, name)
        q, k, v, sinks = _leaves(c)
        kw = {}
        if c["cu"] is not None:
            kw["cu_seq_lens_q"] = c["cu"]
        if sinks is not None:
            kw["s_aux"] = sinks
        out, _ = hip_attention_forward(None, q, k, v, None, scaling=c["scaling"],
                                       sliding_window=c["W"], core="sdpa", **kw)
        _compare(name, c, out, q, k, v, sinks)


def test_slot_differs_from_plain_causal(golden):
    from veomni_amd.ops.kernels.attention import hip_attention_forward

    c = _case(golden, "both_d16")
    plain, _ = hip_attention_forward(None, c["q"], c["k"], c["v"], None,
                                     scaling=c["scaling"])
    win, _ = hip_attention_forward(None, c["q"], c["k"], c["v"], None,
                                   scaling=c["scaling"], sliding_window=c["W"])
    snk, _ = hip_attention_forward(None, c["q"], c["k"], c["v"], None,
                                   scaling=c["scaling"], s_aux=c["sinks"])
    assert (plain - win).abs().max() > 1e-2
    assert (plain - snk).abs().max() > 1e-2


# ------------------------------------------------------------- window_bounds
def _brute_mask(S, W, cu):
    i = torch.arange(S)[:, None]
    j = torch.arange(S)[None, :]
    m = (j <= i) & (j > i - W)
    if cu is not None:
        doc = torch.zeros(S, dtype=torch.long)
        for n, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
            doc[a:b] = n
        m &= doc[:, None] == doc[None, :]
    return m


def test_window_bounds_equal_brute_force_mask():
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens, window_bounds

    gen = torch.Generator().manual_seed(5)
    for trial in range(40):
        S = int(torch.randint(2, 97, (1,), generator=gen))
        W = int(torch.randint(1, S + 8, (1,), generator=gen))
        ndoc = int(torch.randint(1, 5, (1,), generator=gen))
        cu = None
        if ndoc > 1 and S > ndoc:
            cuts = torch.randperm(S - 1, generator=gen)[:ndoc - 1].add(1).sort().values
            cu = [0] + cuts.tolist() + [S]
        ds = de = None
        if cu is not None:
            ds, de = docs_from_cu_seqlens(torch.tensor(cu, dtype=torch.int32), S)
        lo, hi = window_bounds(S, W, ds, de, "cpu")
        want = _brute_mask(S, W, cu)
        if lo is None:
            assert cu is None and W >= S
            assert torch.equal(want, _brute_mask(S, S, None))
            continue
        assert lo.dtype == torch.int32 and hi.dtype == torch.int32
        assert lo.shape == (S,) and hi.shape == (S,)
        assert (lo[1:] >= lo[:-1]).all() and (hi[1:] >= hi[:-1]).all(), (S, W, cu)
        ar = torch.arange(S)
        assert (lo <= ar).all() and (hi > ar).all() and (hi <= S).all()
        i, j = ar[:, None], ar[None, :]
        # row view (forward, dq): keys lo[i] .. i; column view (dkv): rows
        # j .. hi[j]-1, masked per row by lo again
        assert torch.equal((j <= i) & (j >= lo[:, None]), want), (S, W, cu)
        assert torch.equal((i >= j) & (i < hi[None, :]), want), (S, W, cu)


def test_window_bounds_plain_causal_and_cache():
    from veomni_amd.ops.kernels.attention import docs_from_cu_seqlens, window_bounds

    assert window_bounds(64, 64) == (None, None)
    assert window_bounds(64, 100) == (None, None)
    assert window_bounds(64, None) == (None, None)
    ds, de = docs_from_cu_seqlens(torch.tensor([0, 10, 64], dtype=torch.int32), 64)
    assert window_bounds(64, None, ds, de)[0] is ds
    a = window_bounds(64, 100, ds, de, "cpu")     # documents: still bounds
    assert a[0] is not None and torch.equal(a[0], ds) and torch.equal(a[1], de)
    b = window_bounds(64, 100, ds, de, "cpu")     # same forward, next layer
    assert a[0] is b[0] and a[1] is b[1]
    c = window_bounds(64, 7, ds, de, "cpu")
    assert c[0] is not a[0] and not torch.equal(c[0], a[0])


@pytest.mark.parametrize("bad", [0, -3, 2.5, "8", True, float("nan")])
def test_invalid_window_raises(bad):
    from veomni_amd.models.modeling import ModelConfig
    from veomni_amd.ops.kernels.attention import hip_attention_forward, window_bounds

    with pytest.raises(ValueError):
        window_bounds(32, bad)
    q = torch.zeros(1, 2, 8, 16)
    with pytest.raises(ValueError):
        hip_attention_forward(None, q, q, q, None, sliding_window=bad)
    with pytest.raises(ValueError):
        ModelConfig(sliding_window=bad)


def test_softcap_raises_in_both_cores():
    from veomni_amd.ops.kernels.attention import hip_attention_forward

    q = torch.zeros(1, 2, 8, 16)
    for core in ("hip_flash", "sdpa"):
        with pytest.raises(NotImplementedError):
            hip_attention_forward(None, q, q, q, None, softcap=30.0, core=core)
        for ok in (None, 0, 0.0):
            hip_attention_forward(None, q, q, q, None, softcap=ok, core=core)


def test_s_aux_shape_checked():
    from veomni_amd.ops.kernels.attention import hip_attention_forward

    q = torch.zeros(1, 2, 8, 16)
    with pytest.raises(ValueError):
        hip_attention_forward(None, q, q, q, None, s_aux=torch.zeros(3))
    with pytest.raises(ValueError):
        hip_attention_forward(None, q, q, q, None, s_aux=torch.zeros(1, 2))


# ------------------------------------------------------- config, preset, model
def test_config_preset_and_parameters():
    from veomni_amd.models import PRESETS, build_model
    from veomni_amd.models.modeling import ModelConfig

    d = ModelConfig()
    assert d.sliding_window is None and d.layer_types is None \
        and d.attention_sinks is False
    for name, cfg in PRESETS.items():
        if name != "tiny-d128-swa":
            assert cfg.sliding_window is None and not cfg.attention_sinks, name
    cfg = PRESETS["tiny-d128-swa"]
    assert cfg.head_dim == 128 and cfg.sliding_window == 128 and cfg.attention_sinks
    assert cfg.layer_types == ("sliding_attention", "full_attention")
    model = build_model("tiny-d128-swa")
    attn = [l.self_attn for l in model.model.layers]
    assert [a.sliding_window for a in attn] == [128, None]
    for a in attn:
        assert isinstance(a.sinks, torch.nn.Parameter)
        assert a.sinks.shape == (cfg.num_attention_heads,)
        assert 0 < a.sinks.std() < 5 * cfg.initializer_range
    assert "model.layers.0.self_attn.sinks" in model.state_dict()
    # no window / sinks: no parameter, no kwargs
    plain = build_model("tiny-d128")
    assert plain.model.layers[0].self_attn.sinks is None
    assert not any("sinks" in k for k in plain.state_dict())
    # a window without layer_types slides everywhere
    allw = ModelConfig(num_hidden_layers=3, sliding_window=16)
    assert [allw.layer_sliding_window(i) for i in range(3)] == [16, 16, 16]
    with pytest.raises(ValueError):
        ModelConfig(num_hidden_layers=2, sliding_window=16,
                    layer_types=("sliding_attention",))
    with pytest.raises(ValueError):
        ModelConfig(num_hidden_layers=1, layer_types=("chunked_attention",))


def test_model_window_changes_output_and_sinks_get_grad():
    from veomni_amd.models import build_model
    from veomni_amd.models.modeling import bind_ops

    bind_ops("eager")
    model = build_model("tiny-d128-swa")
    ids = torch.randint(0, 512, (1, 192), generator=torch.Generator().manual_seed(1))
    loss, _ = model(ids, labels=ids)
    loss.backward()
    for layer in model.model.layers:
        g = layer.self_attn.sinks.grad
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0
    with torch.no_grad():
        a, _ = model(ids)
        model.model.layers[0].self_attn.sliding_window = None
        b, _ = model(ids)
    assert (a - b).abs().max() > 1e-4
    # up to W tokens the window cuts nothing
    short = ids[:, :128]
    with torch.no_grad():
        b2, _ = model(short)
        model.model.layers[0].self_attn.sliding_window = 128
        a2, _ = model(short)
    torch.testing.assert_close(a2, b2, rtol=2e-5, atol=1e-6)


def test_async_ulysses_refuses_window_and_sinks():
    from veomni_amd.models import build_model

    class _PS:
        ulysses_enabled = True
        async_ulysses = True

    import veomni_amd.models.modeling as M

    model = build_model("tiny-d128-swa")
    orig = M.get_parallel_state
    M.get_parallel_state = lambda: _PS()
    try:
        with pytest.raises(NotImplementedError):
            model(torch.zeros(1, 8, dtype=torch.long))
    finally:
        M.get_parallel_state = orig


# ------------------------------------------------------------- sync Ulysses
def _run(rank, world_size, fn, port, args):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        fn(rank, world_size, *args)
    finally:
        from veomni_amd.distributed.parallel_state import set_parallel_state

        set_parallel_state(None)
        dist.destroy_process_group()


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _ulysses_swa(rank, ws):
    from veomni_amd.distributed.parallel_state import (init_parallel_state,
                                                       set_parallel_state)
    from veomni_amd.models import build_model
    from veomni_amd.models.modeling import bind_ops

    bind_ops("eager")
    S = 256                      # twice the preset's window
    ids = torch.randint(0, 512, (1, S), generator=torch.Generator().manual_seed(7))
    pos = torch.arange(S)[None]
    model = build_model("tiny-d128-swa")
    sinks = [l.self_attn.sinks for l in model.model.layers]

    # ws = 1 on the full sequence
    set_parallel_state(None)
    ref, _ = model.model(ids, position_ids=pos)
    ref.float().pow(2).sum().backward()
    ref_grads = [p.grad.clone() for p in sinks]
    model.zero_grad(set_to_none=True)

    # sync Ulysses: this rank's slice of the sequence, its heads' sinks
    init_parallel_state(ulysses_size=ws)
    n = S // ws
    sl = slice(rank * n, (rank + 1) * n)
    out, _ = model.model(ids[:, sl], position_ids=pos[:, sl])
    torch.testing.assert_close(out, ref[:, sl].detach(), rtol=1e-4, atol=1e-5)
    out.float().pow(2).sum().backward()
    heads = sinks[0].numel() // ws
    for p, want in zip(sinks, ref_grads):
        g = p.grad.clone()
        other = torch.ones(p.numel(), dtype=torch.bool)
        other[rank * heads:(rank + 1) * heads] = False
        assert (g[other] == 0).all() and g[~other].abs().max() > 0
        dist.all_reduce(g)
        torch.testing.assert_close(g, want, rtol=1e-4, atol=1e-5)


def test_sync_ulysses_matches_single_rank():
    mp.spawn(_run, args=(2, _ulysses_swa, _free_port(), ()), nprocs=2, join=True)


# ---------------------------------------------------------------------- ABI
def test_new_symbols_declared_and_bound():
    header = open(os.path.join(REPO, "include", "veomni_hip.h")).read()
    lib_py = open(os.path.join(REPO, "veomni_amd", "ops", "hip_lib.py")).read()
    declared = set(re.findall(r"^int\s+(vh_\w+)\s*\(", header, re.M))
    bound = set(re.findall(r'_sig\(lib, "(vh_\w+)"', lib_py))
    for sym in ("vh_attn_fwd_win_sink_bf16", "vh_attn_bwd_pre_sink_bf16",
                "vh_attn_bwd2_win_bf16"):
        assert sym in declared, sym
        assert sym in bound, sym
