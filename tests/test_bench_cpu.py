"""CPU-checkable pieces of the bench contract: the analytic FLOP/param model
(the MFU denominator) against known model-card figures, and preset sanity."""

from veomni_amd.models import PRESETS

import bench


def test_active_params_known_values():
    # Qwen3-30B-A3B: ~3B activated parameters (the "A3B" in the name);
    # our count follows the reference count_flops.py convention (lm_head
    # included, input embedding lookup excluded).
    a = bench.active_params(PRESETS["qwen3-moe-30b"])
    assert 2.9e9 < a < 3.4e9, a
    # Llama-3-8B: 8.03B total, ~7.5B compute-active under the 6PT convention
    b = bench.active_params(PRESETS["llama3-8b"])
    assert 7.3e9 < b < 8.1e9, b


def test_step_flops_scales_linearly_in_tokens():
    cfg = PRESETS["qwen3-moe-30b"]
    f1 = bench.step_flops(cfg, 4096, 4096)
    f2 = bench.step_flops(cfg, 8192, 4096)
    assert abs(f2 / f1 - 2.0) < 1e-6


def test_dump_outputs_is_deterministic_float_npy(tmp_path):
    """--dump-outputs writer: float32 .npy files, the same sampled positions
    on every call, parameters and AdamW moments sampled alike."""
    import numpy as np
    import torch

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.Linear(96, 8))
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2)
    loss = model(torch.randn(4, 64)).square().mean()
    loss.backward()
    gnorm = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
    opt.step()

    bench.dump_outputs(str(tmp_path / "a"), loss, gnorm, model, opt)
    bench.dump_outputs(str(tmp_path / "b"), loss, gnorm, model, opt)
    names = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert names == ["adam_exp_avg_sample.npy", "grad_norm.npy", "loss.npy",
                     "params_sample.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n
        assert np.isfinite(a).all(), n
        total += a.nbytes
    assert total < 64 * 2**20
    ps = np.load(tmp_path / "a" / "params_sample.npy")
    # 4 tensors: 64*96 and 96*8 weights are capped, the biases are sampled
    # with replacement at their own size
    cap = bench.DUMP_PER_TENSOR
    assert ps.shape == (min(64 * 96, cap) + 96 + min(96 * 8, cap) + 8,)
    assert np.load(tmp_path / "a" / "adam_exp_avg_sample.npy").shape == ps.shape
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == float(loss.detach())


def test_moe_preset_matches_qwen3_30b_a3b_card():
    c = PRESETS["qwen3-moe-30b"]
    assert (c.num_hidden_layers, c.hidden_size, c.num_experts,
            c.num_experts_per_tok, c.moe_intermediate_size,
            c.num_attention_heads, c.num_key_value_heads,
            c.vocab_size) == (48, 2048, 128, 8, 768, 32, 4, 151936)
