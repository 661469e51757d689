#!/usr/bin/env python3
"""Microbench: the MLA HIP flash pair (q/k head_dim 192, v head_dim 128)
against the torch core and against the zero-padded-V recipe.

Shapes: B 1, Hq = Hkv in {16, 32}, bf16, S in {4096, 8192}. Variants: plain
causal; packed (4 documents). Paths, through hip_attention_forward unless
noted:
  hip_flash  the vh_attn_mla_* pair;
  sdpa       the torch core as it runs without the pair (is_causal, or an
             explicit S x S document mask);
  padded     plain causal only: V zero-padded to 192 into torch SDPA with
             is_causal, output sliced back to 128 (what a flash-attn caller
             without a 192 / 128 kernel does).
Each runs forward alone (no_grad) and forward+backward. All variants and
paths of a shape run in one process, alternating: warm-up of everything
first, then `--repeats` rounds in which each is timed once, with device
events around `--inner` back-to-back calls followed by a synchronise.
Printed: the median round, the fastest and slowest round (the round-to-round
spread) and the achieved TFLOP/s of the median from the shape's operation
count: forward 2*S^2*H*(192+128)*0.5 (QK^T 192 deep, P.V 128 wide, causal
half); backward 2*S^2*H*(3*192 + 2*128)*0.5 (the recomputed QK^T, dQ and dK
192 deep or wide; dP and dV 128).

Run on an MI355X:  python tests/gpu_attn_mla_perf.py"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from veomni_amd.ops.kernels.attention import hip_attention_forward

DQK, DV = 192, 128


def event_time(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--heads", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    scale = DQK ** -0.5

    for S in a.seqs:
        for H in a.heads:
            g = torch.Generator(device="cuda").manual_seed(S + H)
            mk = lambda d: (torch.randn(1, H, S, d, device="cuda", generator=g) * 0.5) \
                .to(torch.bfloat16).requires_grad_(True)
            q, k, v = mk(DQK), mk(DQK), mk(DV)
            do = (torch.randn(1, S, H, DV, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
            cu = torch.tensor([0, S // 8, S // 2, S - S // 4, S], dtype=torch.int32,
                              device="cuda")

            def slot(core, **kw):
                return lambda: hip_attention_forward(None, q, k, v, None, scaling=scale,
                                                     core=core, **kw)[0]

            def padded():
                out = F.scaled_dot_product_attention(
                    q, k, F.pad(v, [0, DQK - DV]), scale=scale, is_causal=True)
                return out[..., :DV].transpose(1, 2)

            paths = {("causal", "hip_flash"): slot("hip_flash"),
                     ("causal", "sdpa"): slot("sdpa"),
                     ("causal", "padded"): padded,
                     ("packed4", "hip_flash"): slot("hip_flash", cu_seq_lens_q=cu),
                     ("packed4", "sdpa"): slot("sdpa", cu_seq_lens_q=cu)}

            def make(call):
                def fwd():
                    with torch.no_grad():
                        call()

                def fwd_bwd():
                    call().backward(do)
                    q.grad = k.grad = v.grad = None

                return fwd, fwd_bwd

            fns = {key: make(c) for key, c in paths.items()}
            for _ in range(a.warmup):
                for f, fb in fns.values():
                    f()
                    fb()
            tf = {key: [] for key in fns}
            tfb = {key: [] for key in fns}
            for _ in range(a.repeats):       # alternate variants and paths
                for key, (f, fb) in fns.items():
                    tf[key].append(event_time(f, a.inner))
                    tfb[key].append(event_time(fb, a.inner))

            fl_f = 2.0 * S * S * H * (DQK + DV) * 0.5
            fl_b = 2.0 * S * S * H * (3 * DQK + 2 * DV) * 0.5
            print(f"S={S} B=1 H={H} q/k {DQK} v {DV} bf16; median of {a.repeats} "
                  f"rounds x {a.inner} calls (ms); TFLOP/s of the median (causal count)")
            print(f"{'variant':<9}{'path':<11}{'fwd':>9}{'min':>9}{'max':>9}{'TF/s':>8}"
                  f"{'fwd+bwd':>10}{'min':>9}{'max':>9}{'TF/s':>8}")
            for (n, c), _ in paths.items():
                x, y = tf[n, c], tfb[n, c]
                print(f"{n:<9}{c:<11}{median(x) * 1e3:>9.3f}{min(x) * 1e3:>9.3f}"
                      f"{max(x) * 1e3:>9.3f}{fl_f / median(x) * 1e-12:>8.1f}"
                      f"{median(y) * 1e3:>10.3f}{min(y) * 1e3:>9.3f}{max(y) * 1e3:>9.3f}"
                      f"{(fl_f + fl_b) / median(y) * 1e-12:>8.1f}", flush=True)
            del fns, paths, q, k, v, do
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
