"""CPU model of the [64 k][256 out] "reduction-slow" LDS image of
vh_group_gemm8.hip (TStage64 / tr_lane_off): the lane-linear glds fill with
the per-lane permuted source column, and the ds_read_b64_tr_b16 fragment
reads. Checks what the derivation next to tswz64 claims: the fill is a
bijection, every 16x16x32 fragment element is the (k, out) the MFMA operand
map wants, every lane address is 8-byte aligned, and no 32-lane half puts
two different addresses on one of the 64 banks."""

import numpy as np


def tswz64(k):
    return (k & 3) | (((k >> 3) & 1) << 2)


def fill_image():
    """LDS element i -> k * 1000 + out of the source element staged there."""
    lds = np.full(64 * 256, -1, dtype=np.int64)
    for i in range(4):                      # glds instruction
        for w in range(8):                  # wave
            for lane in range(64):
                krow = w * 2 + (lane >> 5)
                pb = (lane & 31) * 16
                seg = (pb >> 5) ^ tswz64(krow)
                col = seg * 16 + ((pb & 31) >> 1)
                k = i * 16 + krow
                dst = (i * 8192 + w * 1024 + lane * 16) // 2
                assert (lds[dst:dst + 8] == -1).all()
                lds[dst:dst + 8] = k * 1000 + col + np.arange(8)
    return lds


def lane_addr(out0, ks, half, lane):
    k = ((lane >> 4) << 3) + ((lane >> 2) & 3)
    return (k * 512 + (((out0 >> 4) ^ tswz64(k)) << 5) + (lane & 3) * 8
            + ks * 16384 + half * 2048)


def test_fill_is_a_bijection():
    lds = fill_image()
    assert (lds >= 0).all()
    assert len(set(lds.tolist())) == 64 * 256


def test_transposed_reads_deliver_the_mfma_operand():
    lds = fill_image()
    for ks in range(2):
        for out0 in range(0, 256, 16):
            for half in range(2):
                addr = [lane_addr(out0, ks, half, l) for l in range(64)]
                assert all(a % 8 == 0 and 0 <= a and a + 8 <= 32768 for a in addr)
                for lane in range(64):
                    g, i = lane >> 4, lane & 15
                    for q in range(4):
                        # lane i of group g: column i of the block, row q in
                        # element q; row q's columns 4p..4p+3 come from the
                        # address of lane 4q+p
                        src = addr[g * 16 + 4 * q + (i >> 2)] // 2 + (i & 3)
                        k = ks * 32 + 8 * g + 4 * half + q
                        assert lds[src] == k * 1000 + out0 + i


def test_transposed_reads_are_bank_conflict_free():
    for ks in range(2):
        for out0 in range(0, 256, 16):
            for half in range(2):
                addr = [lane_addr(out0, ks, half, l) for l in range(64)]
                for h32 in range(2):
                    on_bank = {}
                    for lane in range(h32 * 32, h32 * 32 + 32):
                        for d in range(2):  # 8 B = 2 banks
                            on_bank.setdefault((addr[lane] // 4 + d) % 64,
                                               set()).add(addr[lane] + 4 * d)
                    assert len(on_bank) == 64
                    assert max(len(v) for v in on_bank.values()) == 1
