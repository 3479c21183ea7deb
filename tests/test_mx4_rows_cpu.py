"""MXFP4 skinny GEMM ops off the GPU: the twins for 17..64 rows and None
outside, on a gate_up mismatch and on a K mismatch."""
import pytest
import torch

from trainingjob_operator_amd.ops import (linear_mx4_rows, mx4_rows_pays,
                                          swiglu_mx4_rows)
from trainingjob_operator_amd.ops.mx4_weight import quantize_mx4


def _weights():
    g = torch.Generator().manual_seed(11)
    w = torch.randn(64, 512, generator=g) * torch.logspace(-2, 1, 64)[:, None]
    return quantize_mx4(w), quantize_mx4(w, gate_up=True), g


@pytest.mark.parametrize("N", [17, 64])
def test_twins_for_17_to_64_rows(N):
    w4, gu4, g = _weights()
    x = torch.randn(N, 512, generator=g).bfloat16()
    assert mx4_rows_pays(x, w4) is True
    assert torch.equal(linear_mx4_rows(x, w4),
                       (x.float() @ w4.dequant().t()).bfloat16())
    gate, up = (x.float() @ gu4.dequant().t()).chunk(2, dim=-1)
    assert torch.equal(swiglu_mx4_rows(x, gu4),
                       (torch.nn.functional.silu(gate) * up).bfloat16())
    assert linear_mx4_rows(x, gu4) is None and swiglu_mx4_rows(x, w4) is None
    assert linear_mx4_rows(x[:, :256], w4) is None          # K mismatch


@pytest.mark.parametrize("N", [16, 65])
def test_none_outside_17_to_64_rows(N):
    w4, gu4, _ = _weights()
    x = torch.zeros(N, 512).bfloat16()
    assert linear_mx4_rows(x, w4) is None
    assert swiglu_mx4_rows(x, gu4) is None
