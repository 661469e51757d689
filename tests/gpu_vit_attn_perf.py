#!/usr/bin/env python3
"""Microbench: the head_dim 80 HIP vision flash pair against the torch twin
(the segment-run SDPA loop) at the VL-7B bench shape: H = 16, four images of
13 104 patches (S = 52 416), with the window cu_seqlens and the image
cu_seqlens of vision_window_index. Hand-run on a GPU (not a test):

    python tests/gpu_vit_attn_perf.py [--reps 20]

q, k, v are views of one [S, 3, H, 80] tensor, as the model holds them.
Warm-up, then the two paths alternate; medians of device-event times."""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from veomni_amd.models.vlm import VisionConfig, vision_window_index  # noqa: E402
from veomni_amd.ops.kernels.attention import (  # noqa: E402
    eager_vision_attention, hip_vision_attention)


def timed(fn, qkv, do, cu, scale, backward):
    q, k, v = (qkv[:, i] for i in range(3))
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    out = fn(q, k, v, cu, scale)
    if backward:
        out.backward(do)
    end.record()
    torch.cuda.synchronize()
    qkv.grad = None
    return start.elapsed_time(end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    cfg = VisionConfig()
    grids = [[1, 182, 72]] * 4                      # 13 104 patches each
    _, cu_img, cu_win = vision_window_index(grids, cfg)
    S, H, D = cu_img[-1], cfg.num_heads, cfg.head_dim
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(S, 3, H, D, generator=g) * 0.5).to(torch.bfloat16).cuda()
    qkv.requires_grad_(True)
    do = (torch.randn(S, H, D, generator=g) * 0.5).to(torch.bfloat16).cuda()
    scale = D ** -0.5
    paths = (("hip", hip_vision_attention), ("twin", eager_vision_attention))
    for regime, cu in (("window", cu_win), ("full", cu_img)):
        lens = sorted({b - a for a, b in zip(cu, cu[1:])})
        print(f"{regime}: S={S} H={H} segments={len(cu) - 1} lengths={lens}")
        for backward in (False, True):
            times = {name: [] for name, _ in paths}
            for it in range(args.warmup + args.reps):
                for name, fn in paths:
                    t = timed(fn, qkv, do, cu, scale, backward)
                    if it >= args.warmup:
                        times[name].append(t)
            med = {n: statistics.median(t) for n, t in times.items()}
            print(f"  {'fwd+bwd' if backward else 'fwd    '}: "
                  + "  ".join(f"{n} {med[n]:8.3f} ms (min {min(times[n]):.3f}, "
                              f"max {max(times[n]):.3f})" for n in med)
                  + f"  twin/hip {med['twin'] / med['hip']:.2f}x")


if __name__ == "__main__":
    main()
