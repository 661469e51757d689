#!/usr/bin/env python3
"""Microbench: MoE load-balancing loss, eager torch vs the fused HIP provider.

Shape (30B bench config): 48 layers of [32768, 128] bf16 router logits with
requires_grad, top_k = 8. Times forward+backward of the model's eager
function (_eager_load_balancing_loss) and of hip_load_balancing_loss in the
same process, alternating (warm-up, then the median of synchronised repeats),
plus the hip forward and backward on their own with achieved GB/s against
the bytes the algorithm moves (fwd L*T*E*2, bwd twice that) and the
peak-memory delta of each implementation."""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from veomni_amd.models.modeling import _eager_load_balancing_loss
from veomni_amd.ops.kernels.load_balancing_loss import hip_load_balancing_loss


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--experts", type=int, default=128)
    ap.add_argument("--top-k", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    L, T, E, k = a.layers, a.tokens, a.experts, a.top_k

    g = torch.Generator(device="cuda").manual_seed(0)
    layers = tuple(
        (torch.randn(T, E, device="cuda", generator=g) * 0.5)
        .to(torch.bfloat16).requires_grad_(True) for _ in range(L))

    def clear():
        for l in layers:
            l.grad = None

    def eager_fb():
        _eager_load_balancing_loss(layers, E, k).backward()
        clear()

    def hip_fb():
        hip_load_balancing_loss(layers, E, k).backward()
        clear()

    state = {}

    def hip_f():
        state["loss"] = hip_load_balancing_loss(layers, E, k)

    def hip_b():
        state["loss"].backward()
        clear()

    # results first: same inputs, both implementations
    with torch.no_grad():
        le = float(_eager_load_balancing_loss(layers, E, k))
        lh = float(hip_load_balancing_loss(layers, E, k))
    print(f"loss eager {le:.8f}  hip {lh:.8f}  rel diff {abs(le - lh) / abs(le):.2e}")

    for _ in range(a.warmup):
        eager_fb()
        hip_fb()
    te, th, tf, tb = [], [], [], []
    for _ in range(a.repeats):  # alternate the two implementations
        te.append(sync_time(eager_fb))
        th.append(sync_time(hip_fb))
        tf.append(sync_time(hip_f))
        tb.append(sync_time(hip_b))

    # forward split: the per-layer stage-1 launches vs the finish pass
    from veomni_amd.ops import hip_lib

    lib = hip_lib.get_lib()
    det = [l.detach() for l in layers]
    blocks = [hip_lib.lbl_num_blocks(T, E) for _ in det]
    partial = torch.empty(sum(blocks), 2, E, dtype=torch.float32, device="cuda")
    cnt = torch.empty(E, dtype=torch.float32, device="cuda")
    psum = torch.empty_like(cnt)
    out2 = torch.empty(2, dtype=torch.float32, device="cuda")
    tw = torch.full((1,), float(L * T), dtype=torch.float32, device="cuda")

    def stage1():
        row0 = 0
        for l, P in zip(det, blocks):
            hip_lib.check(lib.vh_lbl_fwd(l.data_ptr(), 0, None, T, E, k,
                                         partial[row0].data_ptr(), P,
                                         hip_lib.cur_stream()), "vh_lbl_fwd")
            row0 += P

    def finish():
        hip_lib.check(lib.vh_lbl_finish(partial.data_ptr(), partial.shape[0], E,
                                        tw.data_ptr(), cnt.data_ptr(),
                                        psum.data_ptr(), out2.data_ptr(),
                                        hip_lib.cur_stream()), "vh_lbl_finish")

    for _ in range(a.warmup):
        stage1()
        finish()
    t1 = [sync_time(stage1) for _ in range(a.repeats)]
    t2 = [sync_time(finish) for _ in range(a.repeats)]
    print(f"hip fwd split: {L} stage-1 launches {median(t1) * 1e3:.3f} ms, "
          f"finish over {partial.shape[0]} partial rows {median(t2) * 1e3:.3f} ms")

    def peak(fn):
        clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    fwd_bytes = L * T * E * 2
    e_ms, h_ms = median(te) * 1e3, median(th) * 1e3
    f_ms, b_ms = median(tf) * 1e3, median(tb) * 1e3
    print(f"shape: {L} x [{T}, {E}] bf16, top_k {k}; {a.repeats} repeats, median")
    print(f"eager fwd+bwd: {e_ms:.3f} ms  (min {min(te) * 1e3:.3f}, max {max(te) * 1e3:.3f})")
    print(f"hip   fwd+bwd: {h_ms:.3f} ms  (min {min(th) * 1e3:.3f}, max {max(th) * 1e3:.3f})"
          f"  speedup {e_ms / h_ms:.1f}x")
    print(f"hip fwd: {f_ms:.3f} ms  {fwd_bytes / (f_ms * 1e-3) / 1e9:.0f} GB/s "
          f"({fwd_bytes / 1e6:.0f} MB)")
    print(f"hip bwd: {b_ms:.3f} ms  {2 * fwd_bytes / (b_ms * 1e-3) / 1e9:.0f} GB/s "
          f"({2 * fwd_bytes / 1e6:.0f} MB)")
    print(f"peak memory delta: eager {peak(eager_fb):.0f} MiB  hip {peak(hip_fb):.0f} MiB")


if __name__ == "__main__":
    main()
