"""CPU: the host side of the head_dim 80 vision attention path: segment
bounds, the torch twin, argument errors and the OpSlot registration."""

import pytest
import torch

from veomni_amd.ops.kernel_registry import KERNEL_REGISTRY
from veomni_amd.ops.kernels import attention as A

RAGGED = [0, 64, 128, 172, 176, 332]


def test_segments_from_cu_seqlens():
    lo, hi = A.segments_from_cu_seqlens(RAGGED, 332)
    exp_lo = [0] * 64 + [64] * 64 + [128] * 44 + [172] * 4 + [176] * 156
    exp_hi = [64] * 64 + [128] * 64 + [172] * 44 + [176] * 4 + [332] * 156
    assert lo.dtype == hi.dtype == torch.int32
    assert lo.tolist() == exp_lo and hi.tolist() == exp_hi
    lo2, hi2 = A.segments_from_cu_seqlens(RAGGED, 332)
    assert lo2 is lo and hi2 is hi, "the same host list must hit the cache"
    with pytest.raises(ValueError):
        A.segments_from_cu_seqlens([0, 64, 300], 332)


def test_twin_vs_masked_reference():
    g = torch.Generator().manual_seed(80)
    q, k, v = (torch.randn(332, 2, 80, generator=g) for _ in range(3))
    seg = torch.repeat_interleave(torch.arange(5), torch.tensor(RAGGED).diff())
    sc = torch.einsum("shd,thd->hst", q, k) * 80 ** -0.5
    sc = sc.masked_fill(seg[:, None] != seg[None, :], float("-inf"))
    ref = torch.einsum("hst,thd->shd", torch.softmax(sc, dim=-1), v)
    out = A.eager_vision_attention(q, k, v, RAGGED, 80 ** -0.5)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape,dtype", [((8, 2, 64), torch.bfloat16),
                                         ((8, 2, 80), torch.float32)])
def test_hip_vision_attention_rejects(shape, dtype):
    x = torch.zeros(shape, dtype=dtype)
    with pytest.raises(ValueError):
        A.hip_vision_attention(x, x, x, [0, 8], 1.0)


def test_vision_varlen_registration():
    from veomni_amd.models.modeling import bind_ops, veomni_vision_attention

    assert set(KERNEL_REGISTRY.list_available("attention", "vision_varlen")) == {"eager", "hip"}
    specs = KERNEL_REGISTRY._specs["attention", "vision_varlen"]
    assert specs["eager"].factory() is A.eager_vision_attention
    assert specs["hip"].factory() is A.vision_attention_forward
    assert (veomni_vision_attention.op_name, veomni_vision_attention.variant) == \
        ("attention", "vision_varlen")
    bind_ops("eager")
    assert veomni_vision_attention.use_eager_impl
    # off head_dim 80 the "hip" implementation is the twin
    x = torch.randn(8, 2, 16)
    assert torch.equal(A.vision_attention_forward(x, x, x, [0, 4, 8], 0.25),
                       A.eager_vision_attention(x, x, x, [0, 4, 8], 0.25))
