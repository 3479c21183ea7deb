"""packed_rope_attention off the GPU: the dispatch falls back to the
unpacked composition (RoPE on dense q/k + SDPA + transposes) and must give
exactly what the pieces give by hand, at any head_dim."""
import pytest
import torch
import torch.nn.functional as F

from trainingjob_operator_amd.models.config import LLAMA_SMOKE, LLAMA_TINY
from trainingjob_operator_amd.models.llama import _use_packed_attention
from trainingjob_operator_amd.ops import apply_rope, make_inv_freq
from trainingjob_operator_amd.ops.attention import (packed_rope_attention,
                                                    packed_supported)


def _by_hand(qkv, inv_freq, H, HKV, D):
    B, S, _ = qkv.shape
    q, k, v = qkv.split([H * D, HKV * D, HKV * D], dim=-1)
    q = apply_rope(q.reshape(B, S, H, D).contiguous(), inv_freq, S)
    k = apply_rope(k.reshape(B, S, HKV, D).contiguous(), inv_freq, S)
    v = v.reshape(B, S, HKV, D)
    o = F.scaled_dot_product_attention(
        q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
        is_causal=True, enable_gqa=H != HKV)
    return o.transpose(1, 2).reshape(B, S, H * D)


@pytest.mark.parametrize("H,HKV,D,S,dtype", [
    (4, 2, 16, 24, torch.float32),      # llama-tiny head size, GQA
    (2, 2, 128, 256, torch.bfloat16),   # the packed shape, but on the CPU
])
def test_cpu_fallback_is_the_unpacked_composition(H, HKV, D, S, dtype):
    torch.manual_seed(0)
    B = 2
    qkv0 = (torch.randn(B, S, (H + 2 * HKV) * D) * 0.5).to(dtype)
    go = (torch.randn(B, S, H * D) * 0.5).to(dtype)
    inv_freq = make_inv_freq(D, 10000.0)
    assert not packed_supported(qkv0, H, HKV)

    a = qkv0.clone().requires_grad_()
    ref = _by_hand(a, inv_freq, H, HKV, D)
    ref.backward(go)
    b = qkv0.clone().requires_grad_()
    out = packed_rope_attention(b, inv_freq, H, HKV)
    out.backward(go)
    assert out.shape == (B, S, H * D)
    assert torch.equal(out, ref)
    assert torch.equal(b.grad, a.grad)


def test_model_dispatch_stays_unpacked_off_gpu_and_at_small_heads():
    x128 = torch.zeros(1, 256, 4096, dtype=torch.bfloat16)
    assert not _use_packed_attention(x128, LLAMA_SMOKE)      # CPU tensor
    x16 = torch.zeros(1, 256, 128, dtype=torch.bfloat16)
    assert not _use_packed_attention(x16, LLAMA_TINY)        # head_dim 16
