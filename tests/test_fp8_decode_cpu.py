"""Weight-only fp8 decode, off the GPU: the quantised format and the
weights="fp8" plumbing."""
import dataclasses

import pytest
import torch

from trainingjob_operator_amd.models.config import CONFIGS
from trainingjob_operator_amd.models.generate import (
    _fp8_weight, generate, quantize_decode_weights)
from trainingjob_operator_amd.models.llama import LlamaModel
from trainingjob_operator_amd.ops import decode_linear_fp8, decode_swiglu_fp8
from trainingjob_operator_amd.ops.fp8_weight import quantize_rows


@pytest.mark.parametrize("M,K,gate_up", [(16, 512, False), (48, 1536, False),
                                         (32, 512, True)])
def test_format(M, K, gate_up):
    g = torch.Generator().manual_seed(M + K)
    w = torch.randn(M, K, generator=g) * torch.logspace(-3, 2, M)[:, None]
    w[3] = 0                                        # an all-zero row
    w8 = quantize_rows(w.bfloat16(), gate_up=gate_up)
    assert w8.packed.dtype == torch.uint8 and w8.packed.numel() == M * K
    assert (w8.M, w8.K) == (M, K) and w8.scale.shape == (M,)
    s = w8.scale
    amax = w.bfloat16().float().abs().amax(dim=1)
    assert torch.equal(s, torch.exp2(torch.log2(s).round())) and s[3] == 1
    # the smallest power of two that keeps the row inside e4m3
    live = amax > 0
    assert bool((amax <= 448 * s).all()) and bool(
        (amax[live] > 224 * s[live]).all())
    q = (w.bfloat16().float() / s[:, None]).to(torch.float8_e4m3fn).float()
    assert q.abs().max() <= 448
    deq = w8.dequant()
    assert torch.equal(deq, q * s[:, None])         # layout round trip
    assert torch.equal(deq[3], torch.zeros(K))
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)   # exact in bf16


@pytest.mark.parametrize("N", [1, 16])
def test_twins_against_the_dequantised_weight(N):
    g = torch.Generator().manual_seed(N)
    w = torch.randn(64, 512, generator=g) * torch.logspace(-2, 1, 64)[:, None]
    x = torch.randn(N, 512, generator=g).bfloat16()
    w8, gu8 = quantize_rows(w), quantize_rows(w, gate_up=True)
    want = x.float() @ w8.dequant().t()
    assert torch.equal(decode_linear_fp8(x, w8), want.bfloat16())
    gate, up = (x.float() @ gu8.dequant().t()).chunk(2, dim=-1)
    assert torch.equal(decode_swiglu_fp8(x, gu8),
                       (torch.nn.functional.silu(gate) * up).bfloat16())
    assert decode_linear_fp8(x, gu8) is None and decode_swiglu_fp8(x, w8) is None
    assert decode_linear_fp8(torch.zeros(17, 512).bfloat16(), w8) is None


def test_generate_fp8_runs_the_quantised_model():
    """fp32 on the CPU, every K a multiple of 512: weights="fp8" goes through
    the twins over the packed weights, weights="bf16" through F.linear over
    the written-back values. Both multiply the same fp32 numbers and neither
    rounds its output, so the greedy tokens agree."""
    cfg = dataclasses.replace(CONFIGS["llama-tiny"], name="fp8-cpu",
                              hidden_size=512, intermediate_size=512,
                              num_heads=8, num_kv_heads=4, head_dim=64)
    torch.manual_seed(0)
    model = LlamaModel(cfg).eval()
    before = model.blocks[0].mlp.down_proj.weight.clone()
    prompt = torch.randint(0, cfg.vocab_size, (2, 7))
    got = generate(model, prompt, max_new_tokens=6, weights="fp8")
    assert quantize_decode_weights(model) == 4 * cfg.num_layers + 1
    down = model.blocks[0].mlp.down_proj
    assert not torch.equal(down.weight, before)     # rounded in place
    assert torch.equal(down.weight, down.fp8_weight.dequant())
    assert torch.equal(got, generate(model, prompt, max_new_tokens=6))
    with torch.no_grad():                           # a written weight drops
        down.weight.mul_(2.0)                       # its fp8 copy
    assert _fp8_weight(down) is None
    assert quantize_decode_weights(model) == 4 * cfg.num_layers + 1
    assert torch.equal(down.weight, down.fp8_weight.dequant())
    with pytest.raises(ValueError):
        generate(model, prompt, max_new_tokens=1, weights="int4")
