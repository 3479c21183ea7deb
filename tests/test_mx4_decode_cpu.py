"""Weight-only MXFP4 decode, off the GPU: the quantised format and the
weights="mxfp4" plumbing."""
import dataclasses

import pytest
import torch

from trainingjob_operator_amd.models.config import CONFIGS
from trainingjob_operator_amd.models.generate import (
    _mx4_weight, generate, quantize_decode_weights)
from trainingjob_operator_amd.models.llama import LlamaModel
from trainingjob_operator_amd.ops import decode_linear_mx4, decode_swiglu_mx4
from trainingjob_operator_amd.ops.mx4_weight import quantize_mx4

GRID = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6])


@pytest.mark.parametrize("M,K,gate_up", [(16, 512, False), (48, 1536, False),
                                         (32, 512, True)])
def test_format(M, K, gate_up):
    g = torch.Generator().manual_seed(M + K)
    w = torch.randn(M, K, generator=g) * torch.logspace(-3, 2, M)[:, None] \
        * torch.logspace(-2, 2, K // 32).repeat_interleave(32)
    w[3, 64:96] = 0                                 # an all-zero block
    w[5, 32:64] = 2.0 ** -130                       # under the exponent floor
    w = w.bfloat16().float()
    w4 = quantize_mx4(w.bfloat16(), gate_up=gate_up)
    assert w4.packed.dtype == torch.uint8 and w4.packed.numel() == M * K // 2
    assert w4.scale.dtype == torch.uint8 and w4.scale.numel() == M * K // 32
    assert w4.scale.min() >= 2 and w4.scale.max() < 255
    s = w4.scales()                                 # [M, K/32]
    amax = w.reshape(M, K // 32, 32).abs().amax(dim=2)
    assert torch.equal(s, torch.exp2(torch.log2(s).round())) and s[3, 2] == 1
    # the smallest power of two that keeps the block inside e2m1
    live = amax > 2.0 ** -120
    assert bool((amax <= 6 * s).all()) and bool(
        (amax[live] > 3 * s[live]).all()) and s[5, 1] == 2.0 ** -125
    deq = w4.dequant()
    se = s.repeat_interleave(32, dim=1)
    assert bool(torch.isin((deq / se).abs(), GRID).all())
    # nearest: within half the grid's gap at |w| / scale (0.5 below 2, 1 below
    # 4, 2 between 4 and 6), times the scale
    v = (w / se).abs()
    gap = torch.where(v < 2, 0.5, torch.where(v < 4, 1.0, 2.0))
    assert bool(((w - deq).abs() <= gap * se / 2).all())
    assert torch.equal(deq[3, 64:96], torch.zeros(32))
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)   # exact in bf16


def test_rounding_is_to_nearest_even():
    w = torch.zeros(16, 512)
    v = torch.tensor([6, 2.5, 3.5, 0.25, 0.75, 1.25, 1.75, 5, -2.5, -0.25])
    w[0, :10] = v                                   # amax 6: scale 1
    w[1, :10] = v * 2.0 ** -9
    want = torch.tensor([6, 2, 4, 0, 1, 1, 2, 4, -2, 0.0])
    deq = quantize_mx4(w).dequant()
    assert torch.equal(deq[0, :10], want)
    assert torch.equal(deq[1, :10], want * 2.0 ** -9)


def test_refused_shapes():
    assert quantize_mx4(torch.zeros(24, 512)) is None
    assert quantize_mx4(torch.zeros(16, 320)) is None
    assert quantize_mx4(torch.zeros(16, 512), gate_up=True) is None
    assert quantize_mx4(torch.zeros(16)) is None


@pytest.mark.parametrize("N", [1, 16])
def test_twins_against_the_dequantised_weight(N):
    g = torch.Generator().manual_seed(N)
    w = torch.randn(64, 512, generator=g) * torch.logspace(-2, 1, 64)[:, None]
    x = torch.randn(N, 512, generator=g).bfloat16()
    w4, gu4 = quantize_mx4(w), quantize_mx4(w, gate_up=True)
    want = x.float() @ w4.dequant().t()
    assert torch.equal(decode_linear_mx4(x, w4), want.bfloat16())
    gate, up = (x.float() @ gu4.dequant().t()).chunk(2, dim=-1)
    assert torch.equal(decode_swiglu_mx4(x, gu4),
                       (torch.nn.functional.silu(gate) * up).bfloat16())
    assert decode_linear_mx4(x, gu4) is None and decode_swiglu_mx4(x, w4) is None
    assert decode_linear_mx4(torch.zeros(17, 512).bfloat16(), w4) is None


def test_generate_mxfp4_runs_the_quantised_model():
    """fp32 on the CPU, every K a multiple of 512: weights="mxfp4" goes
    through the twins over the packed weights, weights="bf16" through
    F.linear over the written-back values. Both multiply the same fp32
    numbers and neither rounds its output, so the greedy tokens agree."""
    cfg = dataclasses.replace(CONFIGS["llama-tiny"], name="mx4-cpu",
                              hidden_size=512, intermediate_size=512,
                              num_heads=8, num_kv_heads=4, head_dim=64)
    torch.manual_seed(0)
    model = LlamaModel(cfg).eval()
    before = model.blocks[0].mlp.down_proj.weight.clone()
    prompt = torch.randint(0, cfg.vocab_size, (2, 7))
    got = generate(model, prompt, max_new_tokens=6, weights="mxfp4")
    assert quantize_decode_weights(model, "mxfp4") == 4 * cfg.num_layers + 1
    down = model.blocks[0].mlp.down_proj
    assert not torch.equal(down.weight, before)     # rounded in place
    assert torch.equal(down.weight, down.mx4_weight.dequant())
    assert torch.equal(got, generate(model, prompt, max_new_tokens=6))
    with pytest.raises(ValueError):                 # one format per model
        generate(model, prompt, max_new_tokens=1, weights="fp8")
    with torch.no_grad():                           # a written weight drops
        down.weight.mul_(2.0)                       # its MXFP4 copy
    assert _mx4_weight(down) is None
    assert quantize_decode_weights(model, "mxfp4") == 4 * cfg.num_layers + 1
    assert torch.equal(down.weight, down.mx4_weight.dequant())

    torch.manual_seed(0)
    fresh = LlamaModel(cfg).eval()
    generate(fresh, prompt, max_new_tokens=1, weights="fp8")
    with pytest.raises(ValueError):
        generate(fresh, prompt, max_new_tokens=1, weights="mxfp4")
