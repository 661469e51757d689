#!/usr/bin/env python3
"""Microbench: the MoE expert epilogue with and without swiglu_limit.

Shape (30B bench config): fc1 [32768 * 8, 2 * 768] bf16, with and without the
per-row routing weight. Three variants, forward and backward, alternated in
one process:
  unclamped  vh_moe_silu_mul_weighted(_bwd)        (the no-limit path)
  clamped    vh_moe_silu_mul_clamp_weighted(_bwd)  (swiglu_limit set)
  eager      the reference's torch chain with a limit: two masks, two clamped
             copies, silu, mul, mul; backward with silu_backward, masked_fill_
             and cat (ref group_gemm.py:24-42, :460-483)
The unclamped variant is timed twice per round (A and A'); the distance
between the two medians is the run-to-run spread the clamped pair is judged
against. Times are device events around `--inner` back-to-back calls, so
host launch overhead is amortised; GB/s are algorithmic bytes (forward
rows*3I*2, backward rows*5I*2, plus w_row / dw_row) over that time."""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from veomni_amd.ops import hip_lib

HBM_PEAK_SPEC = 8.0e12      # B/s, HBM3E spec
HBM_PEAK_MEASURED = 6.29e12  # B/s, float4 copy


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


def eager_fwd(fc1, w, limit):
    gate, up = fc1.chunk(2, dim=-1)
    mask_g = gate <= limit
    mask_u = (up >= -limit) & (up <= limit)
    gate = gate.clamp(max=limit)
    up = up.clamp(min=-limit, max=limit)
    act = torch.ops.aten.silu(gate) * up
    out = act * w[:, None] if w is not None else act
    return out, (gate, up, mask_g, mask_u, act)


def eager_bwd(dy, w, saved):
    gate, up, mask_g, mask_u, act = saved
    dact = dy * w[:, None] if w is not None else dy
    dw = torch.sum(act * dy, dim=-1) if w is not None else None
    d_up = torch.ops.aten.silu(gate) * dact
    d_gate = torch.ops.aten.silu_backward(dact * up, gate)
    d_gate.masked_fill_(~mask_g, 0)
    d_up.masked_fill_(~mask_u, 0)
    return torch.cat([d_gate, d_up], dim=-1), dw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32768 * 8)
    ap.add_argument("--inter", type=int, default=768)
    ap.add_argument("--limit", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows, I, L = a.rows, a.inter, a.limit

    g = torch.Generator(device="cuda").manual_seed(0)
    fc1 = torch.randn(rows, 2 * I, device="cuda", generator=g).to(torch.bfloat16)
    dy = torch.randn(rows, I, device="cuda", generator=g).to(torch.bfloat16)
    w_row = (torch.rand(rows, device="cuda", generator=g) + 0.25).to(torch.bfloat16)
    leff = hip_lib.swiglu_limit_bf16(L)
    g_share = (fc1[:, :I] > leff).float().mean().item()
    u_share = (fc1[:, I:].abs() > leff).float().mean().item()
    print(f"shape: fc1 [{rows}, {2 * I}] bf16, limit {L} (bf16 {leff}); saturated "
          f"gate {g_share:.1%} up {u_share:.1%}; {a.repeats} repeats x {a.inner} "
          f"calls, median; HBM peak {HBM_PEAK_SPEC / 1e12:.1f} TB/s spec, "
          f"{HBM_PEAK_MEASURED / 1e12:.2f} TB/s measured copy")

    for has_w in (True, False):
        w = w_row if has_w else None
        fwd_bytes = rows * 3 * I * 2 + (rows * 2 if has_w else 0)
        bwd_bytes = rows * 5 * I * 2 + (rows * (2 + 4) if has_w else 0)
        _, saved = eager_fwd(fc1, w, L)

        variants = {
            "fwd": [
                ("unclamped A", lambda: hip_lib.silu_mul_weighted(fc1, w)),
                ("clamped", lambda: hip_lib.silu_mul_weighted(fc1, w, limit=L)),
                ("unclamped A'", lambda: hip_lib.silu_mul_weighted(fc1, w)),
                ("eager", lambda: eager_fwd(fc1, w, L)),
            ],
            "bwd": [
                ("unclamped A", lambda: hip_lib.silu_mul_weighted_bwd(dy, fc1, w)),
                ("clamped", lambda: hip_lib.silu_mul_weighted_bwd(dy, fc1, w, limit=L)),
                ("unclamped A'", lambda: hip_lib.silu_mul_weighted_bwd(dy, fc1, w)),
                ("eager", lambda: eager_bwd(dy, w, saved)),
            ],
        }
        for direction, nbytes in (("fwd", fwd_bytes), ("bwd", bwd_bytes)):
            vs = variants[direction]
            for _ in range(a.warmup):
                for _, fn in vs:
                    fn()
            times = {name: [] for name, _ in vs}
            for _ in range(a.repeats):  # alternate the variants
                for name, fn in vs:
                    times[name].append(event_time(fn, a.inner))
            print(f"-- {direction}, has_w={int(has_w)}, {nbytes / 1e6:.0f} MB algorithmic")
            for name, _ in vs:
                t = times[name]
                m = median(t)
                print(f"{name:13s} {m * 1e6:8.1f} us  (min {min(t) * 1e6:.1f}, "
                      f"max {max(t) * 1e6:.1f})  {nbytes / m / 1e9:7.0f} GB/s  "
                      f"{nbytes / m / HBM_PEAK_SPEC:.1%} of spec, "
                      f"{nbytes / m / HBM_PEAK_MEASURED:.1%} of measured copy")
            ma, mb = median(times["unclamped A"]), median(times["unclamped A'"])
            mc = median(times["clamped"])
            print(f"spread |A - A'| {abs(ma - mb) * 1e6:.1f} us; clamped - "
                  f"mean(A, A') {(mc - (ma + mb) / 2) * 1e6:+.1f} us "
                  f"({(mc / ((ma + mb) / 2) - 1):+.2%})")
        del saved


if __name__ == "__main__":
    main()
