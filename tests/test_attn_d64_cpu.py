"""CPU: gpt-oss attention at head_dim 64 (tiny-d128-swa with head_dim 64 and
attention bias, the model tests/test_gpu_attn_d64.py runs on the HIP pair)
builds and runs one eager forward/backward."""

import dataclasses

import torch


def test_d64_swa_model_builds_and_runs_eager():
    from veomni_amd.models import PRESETS
    from veomni_amd.models.modeling import ForCausalLM, bind_ops

    torch.manual_seed(0)
    cfg = dataclasses.replace(PRESETS["tiny-d128-swa"], head_dim=64, attention_bias=True)
    assert (cfg.num_attention_heads, cfg.num_key_value_heads, cfg.hidden_size) == (4, 2, 256)
    assert cfg.sliding_window == 128 and cfg.attention_sinks
    model = ForCausalLM(cfg)
    for layer in model.model.layers:
        assert layer.self_attn.head_dim == 64
        assert layer.self_attn.sinks.shape == (4,)
        assert layer.self_attn.q_proj.bias is not None
    bind_ops("eager")
    ids = torch.randint(0, cfg.vocab_size, (1, 160))
    loss, _ = model(ids, labels=ids)
    loss.backward()
    assert torch.isfinite(loss)
    assert all(torch.isfinite(l.self_attn.sinks.grad).all() for l in model.model.layers)
