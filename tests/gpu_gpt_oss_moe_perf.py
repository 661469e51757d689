#!/usr/bin/env python3
"""Microbench: the gpt-oss experts path (OpSlot moe_experts/gpt_oss).

Shape: one gpt-oss-20b MoE layer, H = I = 2880, E = 32, top-4, 8192 tokens
(32768 routed rows), bf16.

Part 1, per kernel: each kernel of vh_moe_gpt_oss.hip, time and GB/s against
its algorithmic bytes, next to the existing clamped SwiGLU pair
(vh_moe_silu_mul_clamp_weighted(_bwd)) at the same rows x I in the same run.
The clamped pair is timed twice per round (A and A'); the distance between
the two medians is the run-to-run spread the new kernels are judged against.

Part 2, whole function: HipGptOssFusedMoeFunction forward + backward against
the eager GptOssExperts loop (the only path there was before), plus the share
of the two column-sum launches in the fused backward.

Times are device events around `--inner` back-to-back calls (host launch
overhead amortised), variants alternating, median of `--repeats`."""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from veomni_amd.ops import hip_lib

HBM_PEAK_SPEC = 8.0e12      # B/s, HBM3E spec
HBM_PEAK_MEASURED = 6.29e12  # B/s, float4 copy
ALPHA = 1.702


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def event_time(fn, inner):
    """Seconds per call: device events around `inner` back-to-back calls."""
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / inner


def run_round(variants, warmup, repeats, inner):
    """variants: [(name, fn)]; returns {name: [seconds]} with the variants
    alternating inside every repeat."""
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(event_time(fn, inner))
    return times


def report(name, t, nbytes=None):
    m = median(t)
    line = f"{name:28s} {m * 1e6:9.1f} us  (min {min(t) * 1e6:.1f}, max {max(t) * 1e6:.1f})"
    if nbytes is not None:
        line += (f"  {nbytes / 1e6:7.0f} MB  {nbytes / m / 1e9:6.0f} GB/s  "
                 f"{nbytes / m / HBM_PEAK_SPEC:.1%} of spec, "
                 f"{nbytes / m / HBM_PEAK_MEASURED:.1%} of measured copy")
    print(line)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--hidden", type=int, default=2880)
    ap.add_argument("--inter", type=int, default=2880)
    ap.add_argument("--experts", type=int, default=32)
    ap.add_argument("--topk", type=int, default=4)
    ap.add_argument("--limit", type=float, default=7.0)
    ap.add_argument("--kernel-limit", type=float, default=0.5,
                    help="limit of the per-kernel part (N(0,1) input saturates)")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--fn-inner", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-function", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    T, H, I, E, K = a.tokens, a.hidden, a.inter, a.experts, a.topk
    rows = T * K
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)

    def randn(*shape, scale=1.0):
        return (torch.randn(*shape, device=dev, generator=g) * scale).to(torch.bfloat16)

    print(f"shape: T {T}, H {H}, I {I}, E {E}, top-{K} -> {rows} routed rows, bf16; "
          f"{a.repeats} repeats x {a.inner} calls, median; HBM peak "
          f"{HBM_PEAK_SPEC / 1e12:.1f} TB/s spec, {HBM_PEAK_MEASURED / 1e12:.2f} TB/s "
          "measured copy")

    # ------------------------------------------------------------ per kernel
    L = a.kernel_limit
    # balanced segments with two empty experts (first and one in the middle)
    counts = torch.full((E,), rows // (E - 2), dtype=torch.int64)
    counts[0] = 0
    counts[E // 2] = 0
    counts[-1] += rows - int(counts.sum())
    cumsum = counts.cumsum(0).to(dev)
    fc1 = randn(rows, 2 * I, scale=0.8)
    b1 = randn(E, 2 * I, scale=0.6)
    dy_i = randn(rows, I)
    fc2 = randn(rows, H)
    b2 = randn(E, H)
    dy_h = randn(rows, H)
    w_row = (torch.rand(rows, device=dev, generator=g) + 0.25).to(torch.bfloat16)

    glu_f = rows * 3 * I * 2 + E * 2 * I * 2
    glu_b = rows * 5 * I * 2 + E * 2 * I * 2
    clamp_f, clamp_b = rows * 3 * I * 2, rows * 5 * I * 2
    bs_f = rows * 2 * H * 2 + E * H * 2 + rows * 2
    bs_b = rows * 3 * H * 2 + E * H * 2 + rows * (2 + 4)
    cs_h = rows * H * 2 + E * H * 4
    cs_2i = rows * 2 * I * 2 + E * 2 * I * 4

    print(f"== per kernel (limit {L}) ==")
    fwd = [
        ("clamped fwd A (no w)", lambda: hip_lib.silu_mul_weighted(fc1, None, limit=L), clamp_f),
        ("gptoss_glu fwd", lambda: hip_lib.gptoss_glu(fc1, b1, cumsum, ALPHA, L), glu_f),
        ("clamped fwd A' (no w)", lambda: hip_lib.silu_mul_weighted(fc1, None, limit=L), clamp_f),
        ("clamped fwd (w)", lambda: hip_lib.silu_mul_weighted(fc1, w_row, limit=L),
         clamp_f + rows * 2),
        ("expert_bias_scale (w)", lambda: hip_lib.expert_bias_scale(fc2, b2, cumsum, w_row), bs_f),
        ("expert_bias_scale (no w)", lambda: hip_lib.expert_bias_scale(fc2, b2, cumsum, None),
         bs_f - rows * 2),
    ]
    bwd = [
        ("clamped bwd A (no w)",
         lambda: hip_lib.silu_mul_weighted_bwd(dy_i, fc1, None, limit=L), clamp_b),
        ("gptoss_glu bwd", lambda: hip_lib.gptoss_glu_bwd(dy_i, fc1, b1, cumsum, ALPHA, L), glu_b),
        ("clamped bwd A' (no w)",
         lambda: hip_lib.silu_mul_weighted_bwd(dy_i, fc1, None, limit=L), clamp_b),
        ("clamped bwd (w)",
         lambda: hip_lib.silu_mul_weighted_bwd(dy_i, fc1, w_row, limit=L),
         clamp_b + rows * 6),
        ("expert_bias_scale bwd (w)",
         lambda: hip_lib.expert_bias_scale_bwd(dy_h, fc2, b2, cumsum, w_row), bs_b),
        ("segment_colsum [rows, H]", lambda: hip_lib.segment_colsum(dy_h, cumsum), cs_h),
        ("segment_colsum [rows, 2I]", lambda: hip_lib.segment_colsum(fc1, cumsum), cs_2i),
    ]
    med = {}
    for title, group in (("forward", fwd), ("backward", bwd)):
        times = run_round([(n, f) for n, f, _ in group], a.warmup, a.repeats, a.inner)
        print(f"-- {title}")
        for n, _, nbytes in group:
            med[n] = report(n, times[n], nbytes)
        direction = "fwd" if title == "forward" else "bwd"
        ma, mb = med[f"clamped {direction} A (no w)"], med[f"clamped {direction} A' (no w)"]
        print(f"spread |A - A'| {abs(ma - mb) * 1e6:.1f} us "
              f"({abs(ma - mb) / ((ma + mb) / 2):.2%})")
    colsum_us = (med["segment_colsum [rows, H]"] + med["segment_colsum [rows, 2I]"]) * 1e6
    del fc1, dy_i, fc2, dy_h

    if a.skip_function:
        return

    # -------------------------------------------------------- whole function
    from veomni_amd.models.modeling import GptOssExperts, ModelConfig, bind_ops
    from veomni_amd.ops.kernels.moe import HipGptOssFusedMoeFunction

    print(f"== whole function (limit {a.limit}), forward + backward ==")
    bind_ops("eager")
    cfg = ModelConfig(hidden_size=H, num_experts=E, num_experts_per_tok=K,
                      moe_intermediate_size=I, vocab_size=64,
                      expert_style="gpt_oss", swiglu_limit=a.limit)
    with torch.device(dev):
        experts = GptOssExperts(cfg).to(torch.bfloat16)
    with torch.no_grad():
        experts.gate_up_proj.copy_(randn(E, H, 2 * I, scale=0.02))
        experts.gate_up_proj_bias.copy_(randn(E, 2 * I, scale=0.1))
        experts.down_proj.copy_(randn(E, I, H, scale=0.02))
        experts.down_proj_bias.copy_(randn(E, H, scale=0.1))
    hidden = randn(T, H).requires_grad_(True)
    logits = torch.randn(T, E, device=dev, generator=g)
    top_v, top_i = torch.topk(logits, K, dim=-1)
    top_w = torch.softmax(top_v, dim=-1).to(torch.bfloat16).requires_grad_(True)
    dy = randn(T, H, scale=0.1)
    params = [experts.gate_up_proj, experts.gate_up_proj_bias, experts.down_proj,
              experts.down_proj_bias]

    def clear():
        hidden.grad = top_w.grad = None
        for p in params:
            p.grad = None

    def fused_fwd():
        return HipGptOssFusedMoeFunction.apply(E, top_w, top_i, hidden, *params,
                                               ALPHA, a.limit)

    def fused():
        fused_fwd().backward(dy)
        clear()

    def eager():
        experts(hidden, top_i, top_w).backward(dy)
        clear()

    def fused_fwd_only():
        with torch.no_grad():
            fused_fwd()

    def eager_fwd_only():
        with torch.no_grad():
            experts(hidden, top_i, top_w)

    times = run_round([("fused fwd+bwd A", fused), ("eager fwd+bwd", eager),
                       ("fused fwd+bwd A'", fused), ("fused fwd", fused_fwd_only),
                       ("eager fwd", eager_fwd_only)],
                      2, a.repeats, a.fn_inner)
    m = {n: report(n, t) for n, t in times.items()}
    fa, fb = m["fused fwd+bwd A"], m["fused fwd+bwd A'"]
    fmean = (fa + fb) / 2
    print(f"spread |A - A'| {abs(fa - fb) * 1e6:.1f} us ({abs(fa - fb) / fmean:.2%})")
    print(f"eager / fused, forward + backward: {m['eager fwd+bwd'] / fmean:.2f}x; "
          f"forward only: {m['eager fwd'] / m['fused fwd']:.2f}x")
    bwd_us = (fmean - m["fused fwd"]) * 1e6
    print(f"fused backward = {bwd_us:.0f} us (fwd+bwd minus fwd); the two column sums "
          f"take {colsum_us:.0f} us of it ({colsum_us / bwd_us:.1%})")
    flops = 3 * 2.0 * rows * (H * 2 * I + I * H)
    print(f"grouped-GEMM algorithmic work: {flops / 1e12:.2f} TFLOP fwd+bwd, "
          f"{flops / fmean / 1e12:.0f} TFLOP/s over the fused call")


if __name__ == "__main__":
    main()
