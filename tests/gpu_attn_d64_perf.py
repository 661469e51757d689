#!/usr/bin/env python3
"""Microbench: the head_dim 64 HIP flash pair against the torch core at
gpt-oss's attention shape.

Shapes: B 1, Hq/Hkv 64/8, D 64, bf16, S in {4096, 8192}. Variants: plain
causal; W = 128; W = 128 + sinks; sinks only; packed (4 documents). Each runs
forward alone (no_grad) and forward+backward through hip_attention_forward
with core="hip_flash" and core="sdpa". All variants and both cores of a shape
run in one process, alternating: warm-up of everything first, then
`--repeats` rounds in which each is timed once over `--inner` back-to-back
calls that end in a device synchronise. Printed: the median round, the
fastest and slowest round (the round-to-round spread), the sdpa / hip_flash
ratio, and the peak memory one forward+backward call allocates above what
was resident before it.

Run on an MI355X:  python tests/gpu_attn_d64_perf.py"""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from veomni_amd.ops.kernels.attention import hip_attention_forward


def sync_time(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def median(xs):
    return sorted(xs)[len(xs) // 2]


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--hq", type=int, default=64)
    ap.add_argument("--hkv", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    D, scale = 64, 0.125

    for S in a.seqs:
        g = torch.Generator(device="cuda").manual_seed(S)
        mk = lambda h: (torch.randn(1, h, S, D, device="cuda", generator=g) * 0.5) \
            .to(torch.bfloat16).requires_grad_(True)
        q, k, v = mk(a.hq), mk(a.hkv), mk(a.hkv)
        do = (torch.randn(1, S, a.hq, D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        sinks = torch.randn(a.hq, device="cuda", generator=g).requires_grad_(True)
        cu = torch.tensor([0, S // 8, S // 2, S - S // 4, S], dtype=torch.int32,
                          device="cuda")
        variants = {"causal": {}, "W=128": dict(sliding_window=128),
                    "W=128+sinks": dict(sliding_window=128, s_aux=sinks),
                    "sinks": dict(s_aux=sinks), "packed4": dict(cu_seq_lens_q=cu)}

        def make(kw, core):
            def fwd():
                with torch.no_grad():
                    hip_attention_forward(None, q, k, v, None, scaling=scale,
                                          core=core, **kw)

            def fwd_bwd():
                hip_attention_forward(None, q, k, v, None, scaling=scale,
                                      core=core, **kw)[0].backward(do)
                q.grad = k.grad = v.grad = sinks.grad = None

            return fwd, fwd_bwd

        fns = {(n, c): make(kw, c) for n, kw in variants.items()
               for c in ("hip_flash", "sdpa")}
        for _ in range(a.warmup):
            for f, fb in fns.values():
                f()
                fb()
        mem = {key: peak_mib(fb) for key, (_, fb) in fns.items()}
        tf = {key: [] for key in fns}
        tfb = {key: [] for key in fns}
        for _ in range(a.repeats):       # alternate variants and cores
            for key, (f, fb) in fns.items():
                tf[key].append(sync_time(f, a.inner))
                tfb[key].append(sync_time(fb, a.inner))

        print(f"S={S} B=1 Hq/Hkv={a.hq}/{a.hkv} D={D} bf16; median of {a.repeats} "
              f"rounds x {a.inner} calls (ms); peak = MiB allocated by one fwd+bwd")
        print(f"{'variant':<13}{'core':<11}{'fwd':>9}{'min':>9}{'max':>9}"
              f"{'fwd+bwd':>10}{'min':>9}{'max':>9}{'peak MiB':>10}{'sdpa/hip f+b':>14}")
        for n in variants:
            for c in ("hip_flash", "sdpa"):
                x, y = tf[n, c], tfb[n, c]
                ratio = median(tfb[n, "sdpa"]) / median(tfb[n, "hip_flash"])
                print(f"{n:<13}{c:<11}{median(x) * 1e3:>9.3f}{min(x) * 1e3:>9.3f}"
                      f"{max(x) * 1e3:>9.3f}{median(y) * 1e3:>10.3f}{min(y) * 1e3:>9.3f}"
                      f"{max(y) * 1e3:>9.3f}{mem[n, c]:>10.0f}{ratio:>14.2f}", flush=True)
        del fns, q, k, v, do
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
