#!/usr/bin/env python3
"""Build libveomni_hip.so in-tree (gfx950 only).

Run: python veomni_amd/csrc/build.py  (or via __graft_entry__.build()).
The .so lands at veomni_amd/libveomni_hip.so — git-ignored but shipped to the
GPU box by gpurun (built artefacts travel with the snapshot).
"""

import os
import subprocess
import sys
import tempfile

CSRC = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(CSRC)
OUT = os.path.join(PKG, "libveomni_hip.so")

# Sources compiled on their own with extra flags and linked in as objects
# (the other sources keep the one-command build and its code generation).
# vh_attention64.hip: no packed-fp32 VALU forms (v_pk_mul_f32 and friends) in
# the softmax stream. vh_group_gemm8.hip: the same flag for the indexed
# kernels (the file's ISA has no packed-fp32 instruction either way).
_NO_PK_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
EXTRA_FLAGS = {
    "vh_attention64.hip": _NO_PK_F32,
    "vh_attention80.hip": _NO_PK_F32,   # as vh_attention64.hip
    "vh_attention_mla.hip": _NO_PK_F32,  # as vh_attention64.hip
    "vh_group_gemm8.hip": _NO_PK_F32,
}

SOURCES = [
    "vh_abi.cpp",
    "vh_moe_ops.hip",
    "vh_moe_swiglu_limit.hip",
    "vh_moe_gpt_oss.hip",
    "vh_group_gemm.hip",
    "vh_group_gemm8.hip",
    "vh_norms.hip",
    "vh_attention.hip",
    "vh_attention64.hip",
    "vh_attention80.hip",
    "vh_attention_mla.hip",
    "vh_ce.hip",
    "vh_logprob.hip",
    "vh_adamw.hip",
    "vh_lbl.hip",
]


def build(verbose: bool = True) -> str:
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    headers = [os.path.join(CSRC, "vh_common.h"),
               os.path.join(os.path.dirname(PKG), "include", "veomni_hip.h")]
    newest_src = max(os.path.getmtime(s) for s in srcs + headers)
    if os.path.exists(OUT) and os.path.getmtime(OUT) > newest_src:
        if verbose:
            print(f"[vh build] up to date: {OUT}")
        return OUT
    base = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
    objs = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, flags in EXTRA_FLAGS.items():
            obj = os.path.join(tmp, name + ".o")
            cmd = [*base, *flags, "-c", "-x", "hip", os.path.join(CSRC, name),
                   "-o", obj]
            if verbose:
                print("[vh build]", " ".join(cmd))
            subprocess.run(cmd, check=True)
            objs.append(obj)
        cmd = [
            *base, "-shared", *objs, "-x", "hip",
            *[s for s in srcs if os.path.basename(s) not in EXTRA_FLAGS],
            "-o", OUT,
        ]
        if verbose:
            print("[vh build]", " ".join(cmd))
        subprocess.run(cmd, check=True)
    return OUT


if __name__ == "__main__":
    build()
    sys.exit(0)
