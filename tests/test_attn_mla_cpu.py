"""MLA attention (q/k head_dim 192, v head_dim 128) without a GPU: config
validation, the tiny-mla preset and its state-dict names, the torch cores on
mixed head dims against an fp64 written-out softmax, and an MLAttention
forward/backward."""

import dataclasses

import pytest
import torch

from veomni_amd.models import PRESETS, build_model
from veomni_amd.models.modeling import MLAttention, ModelConfig, sdpa_attention
from veomni_amd.ops.kernels.attention import (docs_from_cu_seqlens,
                                              hip_attention_forward)


@pytest.mark.parametrize("bad", [dict(attention_style="mha"), dict(qk_norm=True),
                                 dict(attention_sinks=True), dict(attention_bias=True)])
def test_mla_config_validation(bad):
    with pytest.raises(ValueError):
        dataclasses.replace(PRESETS["tiny-mla"], **bad)


def test_mla_presets_and_state_dict_names():
    for name, cfg in PRESETS.items():
        assert cfg.attention_style == ("mla" if name == "tiny-mla" else "standard"), name
    cfg = PRESETS["tiny-mla"]
    assert cfg.head_dim == cfg.qk_rope_head_dim == 64
    keys = {k.split("self_attn.")[1] for k in build_model("tiny-mla").state_dict()
            if ".layers.0.self_attn." in k}
    assert keys == {f"{n}.weight" for n in (
        "q_a_proj", "q_a_layernorm", "q_b_proj", "kv_a_proj_with_mqa",
        "kv_a_layernorm", "kv_b_proj", "o_proj")}
    full_q = MLAttention(dataclasses.replace(cfg, q_lora_rank=None), 0)
    assert full_q.q_proj.weight.shape == (4 * 192, 256)
    assert full_q.o_proj.weight.shape == (256, 4 * 128)


@pytest.mark.parametrize("packed_window", [False, True])
def test_mla_torch_cores_mixed_head_dims(packed_window):
    S, scale = 48, 192 ** -0.5
    g = torch.Generator().manual_seed(5)
    q = torch.randn(1, 4, S, 192, generator=g)
    k = torch.randn(1, 2, S, 192, generator=g)
    v = torch.randn(1, 2, S, 128, generator=g)
    kw, lo = {}, torch.zeros(S, dtype=torch.long)
    if packed_window:
        ds, de = docs_from_cu_seqlens(torch.tensor([0, 10, 31, 48]), S)
        kw = dict(doc_start=ds, doc_end=de, sliding_window=7)
        lo = torch.maximum(ds.long(), torch.arange(S) - 6)
    ar = torch.arange(S)
    allowed = (ar[None, :] <= ar[:, None]) & (ar[None, :] >= lo[:, None])
    sc = torch.matmul(q.double(), k.double().repeat_interleave(2, 1).transpose(-1, -2)) * scale
    p = torch.exp(sc.masked_fill(~allowed, float("-inf")))
    ref = torch.matmul(p / p.sum(-1, keepdim=True), v.double().repeat_interleave(2, 1))
    ref = ref.transpose(1, 2)                     # both cores return [B, S, h, Dv]
    slot, _ = hip_attention_forward(None, q, k, v, None, scaling=scale, core="sdpa", **kw)
    eager, _ = sdpa_attention(None, q, k, v, None, scaling=scale, **kw)
    for out in (slot, eager):
        assert out.shape == (1, S, 4, 128)
        torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-6)


def test_mla_attention_module_cpu():
    cfg = PRESETS["tiny-mla"]
    torch.manual_seed(0)
    model = build_model("tiny-mla")
    ids = torch.randint(0, cfg.vocab_size, (1, 24))
    loss, _ = model(ids, labels=ids)
    loss.backward()
    assert torch.isfinite(loss)
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert isinstance(model.model.layers[0].self_attn, MLAttention)
