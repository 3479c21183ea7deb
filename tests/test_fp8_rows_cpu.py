"""fp8 skinny GEMM ops off the GPU: the twins for 17..64 rows, None outside,
and _proj's 40-row route."""
import pytest
import torch

from trainingjob_operator_amd.models.generate import _proj
from trainingjob_operator_amd.ops import (linear_fp8_rows, reference,
                                          swiglu_fp8_rows)
from trainingjob_operator_amd.ops.fp8_weight import quantize_rows


def _weights():
    g = torch.Generator().manual_seed(11)
    w = torch.randn(64, 512, generator=g) * torch.logspace(-2, 1, 64)[:, None]
    return quantize_rows(w), quantize_rows(w, gate_up=True), g


@pytest.mark.parametrize("N", [17, 40, 64])
def test_twins_for_17_to_64_rows(N):
    w8, gu8, g = _weights()
    x = torch.randn(N, 512, generator=g).bfloat16()
    assert torch.equal(linear_fp8_rows(x, w8),
                       reference.decode_linear_fp8(x, w8))
    assert torch.equal(swiglu_fp8_rows(x, gu8),
                       reference.decode_swiglu_fp8(x, gu8))
    assert linear_fp8_rows(x, gu8) is None and swiglu_fp8_rows(x, w8) is None
    assert linear_fp8_rows(x[:, :256], w8) is None          # K mismatch


@pytest.mark.parametrize("N", [16, 65])
def test_none_outside_17_to_64_rows(N):
    w8, gu8, _ = _weights()
    x = torch.zeros(N, 512).bfloat16()
    assert linear_fp8_rows(x, w8) is None
    assert swiglu_fp8_rows(x, gu8) is None


@torch.no_grad()
def test_proj_40_rows_is_the_twin():
    torch.manual_seed(3)
    lin = torch.nn.Linear(512, 1024, bias=False)
    w8 = quantize_rows(lin.weight)
    lin.weight.copy_(w8.dequant())
    lin.fp8_weight, lin.fp8_weight_version = w8, lin.weight._version
    x = torch.randn(40, 512).bfloat16()
    assert torch.equal(_proj(lin, x, fp8=True),
                       reference.decode_linear_fp8(x, w8))
