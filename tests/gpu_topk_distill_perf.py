#!/usr/bin/env python3
"""Microbench: top-k forward-KL distillation through the lm_head, the
torch-only twin (eager_chunk_topk_distill_function) vs the fused HIP provider
(hip_chunk_topk_distill_function), with hip_chunk_logprobs_function at the
same shape in the same run as the baseline the distillation adds to.

Shape (Qwen3 vocabulary): T 8192 tokens, H 2048, V 151936, K 64, chunk 1024,
bf16. Times, in one process and alternating (warm-up, then the median of
synchronised repeats): the no-grad forward and forward + backward of the
three implementations; the two new kernels alone on one [chunk, V] logits
block with device events around a batch of launches, as achieved GB/s
against their algorithmic bytes (fwd rows*(14 K + 24), bwd 4*rows*V +
18*rows*K), beside vh_logprob_bwd measured the same way; and the peak-memory
delta of each leg."""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from veomni_amd.ops import hip_lib
from veomni_amd.ops.kernels.cross_entropy import (
    eager_chunk_topk_distill_function,
    hip_chunk_logprobs_function,
    hip_chunk_topk_distill_function,
)


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def event_ms(fn, launches):
    """Per-launch device time of `launches` back-to-back calls."""
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(launches):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / launches


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--topk", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--clamp", type=float, default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    T, H, V, K, C = a.tokens, a.hidden, a.vocab, a.topk, a.chunk

    g = torch.Generator(device="cuda").manual_seed(0)
    hidden = torch.randn(1, T, H, device="cuda", generator=g).to(torch.bfloat16)
    weight = (torch.randn(V, H, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    labels = torch.randint(0, V, (1, T), device="cuda", generator=g)
    labels[0, 100:200] = -100
    # teacher: per chunk, the top-K of log_softmax(student logits + noise)
    ids = torch.empty(1, T, K, dtype=torch.int64, device="cuda")
    tlp = torch.empty(1, T, K, dtype=torch.float32, device="cuda")
    with torch.no_grad():
        for s in range(0, T, C):
            lg = torch.matmul(hidden[0, s:s + C], weight.t()).float()
            lg += torch.randn(lg.shape, device="cuda", generator=g)
            tlp[0, s:s + C], ids[0, s:s + C] = lg.log_softmax(-1).topk(K, dim=-1)
            del lg
    hidden.requires_grad_(True)
    weight.requires_grad_(True)
    ups = [torch.randn(1, T, device="cuda", generator=g) for _ in range(3)]
    kw = dict(chunk_size=C, temperature=a.temperature)
    tkw = dict(kw, log_prob_min_clamp=a.clamp)

    def clear():
        hidden.grad = None
        weight.grad = None

    def fwd(fn, teacher):
        def run():
            with torch.no_grad():
                if teacher:
                    fn(hidden, weight, labels, ids, tlp, **tkw)
                else:
                    fn(hidden, weight, labels, **kw)
        return run

    def fwd_bwd(fn, teacher):
        def run():
            if teacher:
                outs = fn(hidden, weight, labels, ids, tlp, **tkw)
                torch.autograd.backward(list(outs[:3]), ups)
            else:
                outs = fn(hidden, weight, labels, **kw)
                torch.autograd.backward(list(outs), ups[:2])
            clear()
        return run

    legs = {
        "eager   distill fwd (no grad)": fwd(eager_chunk_topk_distill_function, True),
        "hip     distill fwd (no grad)": fwd(hip_chunk_topk_distill_function, True),
        "hip    logprobs fwd (no grad)": fwd(hip_chunk_logprobs_function, False),
        "eager   distill fwd+bwd": fwd_bwd(eager_chunk_topk_distill_function, True),
        "hip     distill fwd+bwd": fwd_bwd(hip_chunk_topk_distill_function, True),
        "hip    logprobs fwd+bwd": fwd_bwd(hip_chunk_logprobs_function, False),
    }

    # results first: same inputs, both implementations
    with torch.no_grad():
        oe = eager_chunk_topk_distill_function(hidden, weight, labels, ids, tlp, **tkw)
        oh = hip_chunk_topk_distill_function(hidden, weight, labels, ids, tlp, **tkw)
    print("max |hip - eager|: " + "  ".join(
        f"{n} {float((h - e).abs().max()):.3e}" for n, h, e in zip(
            ("log_probs", "entropy", "distill", "student_mass", "teacher_mass"), oh, oe)))
    print(f"mean student_mass {float(oh[3].mean()):.3f}  teacher_mass {float(oh[4].mean()):.3f}  "
          f"distill {float(oh[2].mean()):.3f}")
    del oe, oh

    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(a.repeats):          # alternate the implementations
        for k, fn in legs.items():
            times[k].append(sync_time(fn))

    def peak(fn):
        clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    print(f"shape: T {T}, H {H}, V {V}, K {K}, chunk {C}, bf16, temperature "
          f"{a.temperature}, clamp {a.clamp}; {a.repeats} repeats, median")
    for k, ts in times.items():
        print(f"{k}: {median(ts) * 1e3:9.3f} ms  (min {min(ts) * 1e3:.3f}, "
              f"max {max(ts) * 1e3:.3f})")
    for leg in ("fwd (no grad)", "fwd+bwd"):
        e_ms = median(times[f"eager   distill {leg}"])
        h_ms = median(times[f"hip     distill {leg}"])
        l_ms = median(times[f"hip    logprobs {leg}"])
        print(f"{leg}: hip {e_ms / h_ms:.2f}x the twin; "
              f"{(h_ms - l_ms) * 1e3:+.3f} ms over the hip log-probs path")
    peaks = {k: peak(fn) for k, fn in legs.items()}
    print("peak memory delta (MiB): " + "  ".join(f"[{k}] {v:.0f}" for k, v in peaks.items()))
    print(f"for scale: one fp32 [chunk, V] tensor is {C * V * 4 / 2 ** 20:.0f} MiB, "
          f"one bf16 one {C * V * 2 / 2 ** 20:.0f} MiB, fp32 [V, H] {V * H * 4 / 2 ** 20:.0f} MiB")
    for leg in ("fwd (no grad)", "fwd+bwd"):
        d = peaks[f"hip     distill {leg}"] - peaks[f"hip    logprobs {leg}"]
        print(f"{leg}: hip distill peak - hip log-probs peak = {d:+.0f} MiB")

    # the kernels alone, on one chunk of logits
    clear()
    with torch.no_grad():
        logits = torch.matmul(hidden[0, :C], weight.t())
    lab = labels[0, :C].contiguous()
    cid, ctl = ids[0, :C].contiguous(), tlp[0, :C].contiguous()
    dlp, dent, dd = (u[0, :C].contiguous() for u in ups)
    _, _, lse, raw = hip_lib.logprob_fwd(logits, lab, a.temperature)
    dbuf = torch.empty_like(logits)
    kernels = {
        "topk_kl_fwd": (lambda: hip_lib.topk_kl_fwd(
            logits, lab, lse, cid, ctl, a.temperature, a.clamp), C * (14 * K + 24)),
        "topk_distill_bwd": (lambda: hip_lib.topk_distill_bwd(
            logits, lab, lse, raw, cid, ctl, dlp, dent, dd, a.temperature, a.clamp,
            dlogits_out=dbuf), 4 * C * V + 18 * C * K),
        "logprob_bwd": (lambda: hip_lib.logprob_bwd(
            logits, lab, lse, raw, dlp, dent, a.temperature, dlogits_out=dbuf), 4 * C * V),
    }
    for fn, _ in kernels.values():
        fn()
    ktimes = {k: [] for k in kernels}
    for _ in range(a.repeats):
        for k, (fn, _) in kernels.items():
            ktimes[k].append(event_ms(fn, a.launches))
    print(f"kernels alone on [{C}, {V}] bf16, K {K}, device events over {a.launches} "
          f"launches, median of {a.repeats}:")
    for k, (_, nbytes) in kernels.items():
        ms = median(ktimes[k])
        print(f"  {k:17s} {ms * 1e3:8.1f} us  {nbytes / (ms * 1e-3) / 1e9:6.0f} GB/s "
              f"({nbytes / 1e6:.2f} MB algorithmic)")


if __name__ == "__main__":
    main()
