#!/usr/bin/env python3
"""Microbench: the causal flash pairs at a length that is no multiple of 256.

Shapes: the 30B bench's attention shape (B 8, Hq/Hkv 32/4, D 128) and a
gpt-oss-like one (B 1, Hq/Hkv 64/8, D 64), bf16, forward + backward through
hip_attention_forward, plain causal and W = 128 + sinks.
  (a) S = 4000 on the tail kernels against core="sdpa" at S = 4000;
  (b) S = 4000 on the tail kernels against the aligned kernels at S = 4096
      (us per token: the price of the tail);
  (c) with --parent-lib: S = 4096 on this library against S = 4096 on another
      build of libveomni_hip.so (the parent commit's), in the order this,
      parent, parent, this, so that each library's own run-to-run spread
      (and any effect of the position in the round) stands next to the
      difference.
Everything of one shape runs in one process, alternating: warm-up of every
variant first, then `--repeats` rounds in which each variant is timed once
with device events around `--inner` back-to-back calls. Printed: median,
fastest and slowest round.

Run on an MI355X:  python tests/gpu_attn_tail_perf.py [--parent-lib PATH]"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from veomni_amd.ops import hip_lib
from veomni_amd.ops.kernels.attention import hip_attention_forward

SHAPES = {"30b": (8, 32, 4, 128), "gpt-oss": (1, 64, 8, 64)}


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--tail", type=int, default=4000)
    ap.add_argument("--aligned", type=int, default=4096)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"

    libs = {"this": hip_lib.get_lib()}
    if a.parent_lib:
        hip_lib._LIB, hip_lib.SO_PATH = None, os.path.abspath(a.parent_lib)
        libs["parent"] = hip_lib.get_lib()

    for shape in a.shapes:
        B, hq, hkv, D = SHAPES[shape]
        fns = {}
        for S in (a.tail, a.aligned):
            g = torch.Generator(device="cuda").manual_seed(S)
            mk = lambda h: (torch.randn(B, h, S, D, device="cuda", generator=g) * 0.5) \
                .to(torch.bfloat16).requires_grad_(True)
            q, k, v = mk(hq), mk(hkv), mk(hkv)
            do = (torch.randn(B, S, hq, D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
            sinks = torch.randn(hq, device="cuda", generator=g).requires_grad_(True)

            def make(kw, core, lib, q=q, k=k, v=v, do=do, sinks=sinks):
                def fwd_bwd():
                    hip_lib._LIB = libs[lib]
                    hip_attention_forward(None, q, k, v, None, scaling=D ** -0.5,
                                          core=core, **kw)[0].backward(do)
                    q.grad = k.grad = v.grad = sinks.grad = None
                return fwd_bwd

            for name, kw in (("causal", {}),
                             ("W=128+sinks", dict(sliding_window=128, s_aux=sinks))):
                fns[name, S, "hip_flash"] = make(kw, "hip_flash", "this")
                if S == a.tail:
                    fns[name, S, "sdpa"] = make(kw, "sdpa", "this")
                elif a.parent_lib:
                    fns[name, S, "parent"] = make(kw, "hip_flash", "parent")
                    fns[name, S, "parent again"] = make(kw, "hip_flash", "parent")
                    fns[name, S, "this again"] = make(kw, "hip_flash", "this")
        for _ in range(a.warmup):
            for f in fns.values():
                f()
        t = {key: [] for key in fns}
        for _ in range(a.repeats):       # alternate variants, cores and libraries
            for key, f in fns.items():
                t[key].append(event_ms(f, a.inner))
        hip_lib._LIB = libs["this"]

        print(f"{shape}: B={B} Hq/Hkv={hq}/{hkv} D={D} bf16, fwd+bwd; median of "
              f"{a.repeats} rounds x {a.inner} calls (ms)")
        print(f"{'variant':<13}{'S':>6} {'what':<14}{'median':>9}{'min':>9}{'max':>9}"
              f"{'us/token':>10}")
        for (name, S, what), x in t.items():
            med = sorted(x)[len(x) // 2]
            print(f"{name:<13}{S:>6} {what:<14}{med:>9.3f}{min(x):>9.3f}{max(x):>9.3f}"
                  f"{med * 1e3 / (B * S):>10.4f}", flush=True)
        del fns
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
