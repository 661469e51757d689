"""CPU checks for the fused load-balancing-loss provider: registration, the
opt-in env switch and the no-input contract (no compute without a GPU)."""

import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hip_provider_registered():
    from veomni_amd.ops import KERNEL_REGISTRY

    assert "hip" in KERNEL_REGISTRY.list_available("load_balancing_loss", "standard")


def test_default_binding_stays_eager():
    from veomni_amd.ops import HIP_OPS_CONFIG

    if "VEOMNI_LBL_IMPL" not in os.environ:
        assert HIP_OPS_CONFIG["load_balancing_loss"] == "eager"


def _child(value):
    env = {k: v for k, v in os.environ.items() if k != "VEOMNI_LBL_IMPL"}
    if value is not None:
        env["VEOMNI_LBL_IMPL"] = value
    code = ("from veomni_amd.ops import HIP_OPS_CONFIG as C; "
            "print(C['load_balancing_loss'])")
    return subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env,
                          capture_output=True, text=True)


def test_env_switch_selects_impl():
    r = _child(None)
    assert r.returncode == 0 and r.stdout.strip() == "eager", (r.stdout, r.stderr)
    r = _child("hip")
    assert r.returncode == 0 and r.stdout.strip() == "hip", (r.stdout, r.stderr)
    r = _child("eager")
    assert r.returncode == 0 and r.stdout.strip() == "eager", (r.stdout, r.stderr)


def test_env_switch_rejects_unknown_value():
    r = _child("triton")
    assert r.returncode != 0
    assert "ValueError" in r.stderr and "VEOMNI_LBL_IMPL" in r.stderr, r.stderr


def test_no_logits_returns_zero():
    from veomni_amd.ops.kernels.load_balancing_loss import hip_load_balancing_loss

    assert hip_load_balancing_loss(None, 8, 2) == 0
    assert hip_load_balancing_loss([], 8, 2) == 0  # not a tuple


def test_block_geometry_matches_kernel():
    # rows per block pass = 1024 / (pow2 >= ceil(E/8)); P is capped
    from veomni_amd.ops import hip_lib

    assert hip_lib.lbl_rows_per_block(128) == 64
    assert hip_lib.lbl_rows_per_block(60) == 128
    assert hip_lib.lbl_rows_per_block(8) == 1024
    assert hip_lib.lbl_rows_per_block(256) == 32
    assert hip_lib.lbl_num_blocks(1, 128) == 1
    assert hip_lib.lbl_num_blocks(65, 128) == 2
    assert hip_lib.lbl_num_blocks(8193, 128) == 129
    assert hip_lib.lbl_num_blocks(16449, 128) == hip_lib.LBL_MAX_BLOCKS == 256
