#!/usr/bin/env python3
"""Microbench: per-token log-probs + entropy through the lm_head, the
torch-only twin (eager_chunk_logprobs_function) vs the fused HIP provider
(hip_chunk_logprobs_function).

Shape (Qwen3 vocabulary): T 8192 tokens, H 2048, V 151936, chunk 1024, bf16.
Times, in one process and alternating (warm-up, then the median of
synchronised repeats): the no-grad forward (the old-policy / reference-policy
call of a PPO step) and forward + backward (the actor call) of both
implementations; the two kernels alone on one [chunk, V] logits block with
device events around a batch of launches, as achieved GB/s against their
algorithmic bytes (fwd 2*rows*V, bwd 4*rows*V), beside vh_ce_fwd (6*rows*V)
measured the same way in the same run; and the peak-memory delta of each
implementation."""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from veomni_amd.ops import hip_lib
from veomni_amd.ops.kernels.cross_entropy import (
    eager_chunk_logprobs_function,
    hip_chunk_logprobs_function,
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
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    T, H, V, C = a.tokens, a.hidden, a.vocab, a.chunk

    g = torch.Generator(device="cuda").manual_seed(0)
    hidden = torch.randn(1, T, H, device="cuda", generator=g).to(torch.bfloat16)
    weight = (torch.randn(V, H, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    hidden.requires_grad_(True)
    weight.requires_grad_(True)
    labels = torch.randint(0, V, (1, T), device="cuda", generator=g)
    labels[0, 100:200] = -100
    up_lp = torch.randn(1, T, device="cuda", generator=g)
    up_ent = torch.randn(1, T, device="cuda", generator=g)
    kw = dict(chunk_size=C, temperature=a.temperature)

    def clear():
        hidden.grad = None
        weight.grad = None

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn(hidden, weight, labels, **kw)
        return run

    def fwd_bwd(fn):
        def run():
            lp, ent = fn(hidden, weight, labels, **kw)
            torch.autograd.backward([lp, ent], [up_lp, up_ent])
            clear()
        return run

    legs = {
        "eager fwd (no grad)": fwd(eager_chunk_logprobs_function),
        "hip   fwd (no grad)": fwd(hip_chunk_logprobs_function),
        "eager fwd+bwd": fwd_bwd(eager_chunk_logprobs_function),
        "hip   fwd+bwd": fwd_bwd(hip_chunk_logprobs_function),
    }

    # results first: same inputs, both implementations
    with torch.no_grad():
        le, ee = eager_chunk_logprobs_function(hidden, weight, labels, **kw)
        lh, eh = hip_chunk_logprobs_function(hidden, weight, labels, **kw)
    print(f"max |hip - eager|: log_probs {float((lh - le).abs().max()):.3e}  "
          f"entropy {float((eh - ee).abs().max()):.3e}")
    del le, ee, lh, eh

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

    print(f"shape: T {T}, H {H}, V {V}, chunk {C}, bf16, temperature "
          f"{a.temperature}; {a.repeats} repeats, median")
    for k, ts in times.items():
        print(f"{k}: {median(ts) * 1e3:9.3f} ms  (min {min(ts) * 1e3:.3f}, "
              f"max {max(ts) * 1e3:.3f})")
    for leg in ("fwd (no grad)", "fwd+bwd"):
        e_ms = median(times[f"eager {leg}"])
        h_ms = median(times[f"hip   {leg}"])
        print(f"speedup {leg}: {e_ms / h_ms:.2f}x")
    print("peak memory delta (MiB): " + "  ".join(
        f"{k} {peak(fn):.0f}" for k, fn in legs.items()))
    print(f"for scale: one fp32 [chunk, V] tensor is {C * V * 4 / 2 ** 20:.0f} MiB, "
          f"one bf16 one {C * V * 2 / 2 ** 20:.0f} MiB, fp32 [V, H] {V * H * 4 / 2 ** 20:.0f} MiB")

    # the kernels alone, on one chunk of logits
    clear()
    with torch.no_grad():
        logits = torch.matmul(hidden[0, :C], weight.t())
    lab = labels[0, :C].contiguous()
    dlp, dent = up_lp[0, :C].contiguous(), up_ent[0, :C].contiguous()
    _, _, lse, raw = hip_lib.logprob_fwd(logits, lab, a.temperature)
    dbuf = torch.empty_like(logits)
    kernels = {
        "logprob_fwd": (lambda: hip_lib.logprob_fwd(logits, lab, a.temperature), 2 * C * V),
        "logprob_bwd": (lambda: hip_lib.logprob_bwd(logits, lab, lse, raw, dlp, dent,
                                                    a.temperature, dlogits_out=dbuf), 4 * C * V),
        "ce_fwd": (lambda: hip_lib.ce_fwd(logits, lab, 1.0 / C, dlogits_out=dbuf), 6 * C * V),
    }
    for fn, _ in kernels.values():
        fn()
    ktimes = {k: [] for k in kernels}
    for _ in range(a.repeats):
        for k, (fn, _) in kernels.items():
            ktimes[k].append(event_ms(fn, a.launches))
    print(f"kernels alone on [{C}, {V}] bf16, device events over {a.launches} "
          f"launches, median of {a.repeats}:")
    for k, (_, nbytes) in kernels.items():
        ms = median(ktimes[k])
        print(f"  {k:12s} {ms * 1e3:8.1f} us  {nbytes / (ms * 1e-3) / 1e9:6.0f} GB/s "
              f"({nbytes / 1e6:.0f} MB algorithmic)")


if __name__ == "__main__":
    main()
