#!/usr/bin/env python3
"""Microbench: sliding-window attention and attention sinks in the HIP flash
pair against plain causal attention at the same length.

Shapes: B 1, Hq/Hkv 32/8, D 128, bf16, S in {4096, 8192}; W in {128, 1024,
4096}, each with and without sinks, next to plain causal and plain causal
with sinks. Times the forward alone (no_grad) and forward+backward through
hip_flash_attention, i.e. what the model runs (window_bounds included; it is
cached after the first call, as in a model's layers). All variants of a shape
run in one process, alternating: warm-up of every variant first, then
`--repeats` rounds in which each variant is timed once over `--inner`
back-to-back calls that end in a device synchronise; the figure is the median
round divided by `--inner`. The ratio to plain causal is printed next to the
fraction of the causal score area a window keeps, which is what tile skipping
could reach at best.

Run on an MI355X:  python tests/gpu_attn_window_perf.py"""

import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from veomni_amd.ops.kernels.attention import hip_flash_attention


def sync_time(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def kept_fraction(S, W):
    """Visible (q, k) pairs of a causal window over those of plain causal."""
    if W is None or W >= S:
        return 1.0
    full = S * (S + 1) / 2
    kept = W * (W + 1) / 2 + (S - W) * W
    return kept / full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--windows", type=int, nargs="+", default=[128, 1024, 4096])
    ap.add_argument("--hq", type=int, default=32)
    ap.add_argument("--hkv", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    D = 128
    scale = 1.0 / math.sqrt(D)

    for S in a.seqs:
        g = torch.Generator(device="cuda").manual_seed(S)
        mk = lambda h: (torch.randn(1, h, S, D, device="cuda", generator=g) * 0.5) \
            .to(torch.bfloat16).requires_grad_(True)
        q, k, v = mk(a.hq), mk(a.hkv), mk(a.hkv)
        do = (torch.randn(1, a.hq, S, D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        sinks = torch.randn(a.hq, device="cuda", generator=g).requires_grad_(True)

        variants = [("causal", None, False), ("causal+sinks", None, True)]
        for W in a.windows:
            variants += [(f"W={W}", W, False), (f"W={W}+sinks", W, True)]

        def make(W, use_sinks):
            kw = dict(sliding_window=W, sinks=sinks if use_sinks else None)

            def fwd():
                with torch.no_grad():
                    hip_flash_attention(q, k, v, scale, **kw)

            def fwd_bwd():
                hip_flash_attention(q, k, v, scale, **kw).backward(do)
                q.grad = k.grad = v.grad = sinks.grad = None

            return fwd, fwd_bwd

        fns = {name: make(W, s) for name, W, s in variants}
        for _ in range(a.warmup):
            for f, fb in fns.values():
                f()
                fb()
        tf = {n: [] for n in fns}
        tfb = {n: [] for n in fns}
        for _ in range(a.repeats):       # alternate the variants
            for n, (f, fb) in fns.items():
                tf[n].append(sync_time(f, a.inner))
                tfb[n].append(sync_time(fb, a.inner))

        base_f, base_fb = median(tf["causal"]), median(tfb["causal"])
        print(f"S={S} B=1 Hq/Hkv={a.hq}/{a.hkv} D={D} bf16; median of {a.repeats} "
              f"rounds x {a.inner} calls")
        print(f"{'variant':<16}{'kept':>7}{'fwd ms':>10}{'min':>8}{'max':>8}{'ratio':>7}"
              f"{'fwd+bwd ms':>12}{'min':>8}{'max':>8}{'ratio':>7}")
        for name, W, _ in variants:
            f, fb = median(tf[name]), median(tfb[name])
            print(f"{name:<16}{kept_fraction(S, W):>7.3f}"
                  f"{f * 1e3:>10.3f}{min(tf[name]) * 1e3:>8.3f}{max(tf[name]) * 1e3:>8.3f}"
                  f"{f / base_f:>7.3f}"
                  f"{fb * 1e3:>12.3f}{min(tfb[name]) * 1e3:>8.3f}{max(tfb[name]) * 1e3:>8.3f}"
                  f"{fb / base_fb:>7.3f}", flush=True)


if __name__ == "__main__":
    main()
