"""MXFP4 MoE experts off the GPU: the torch twins of the routed MXFP4 GEMVs,
quantisation and tracking of the experts, and the one-format rule."""
import pytest
import torch

from trainingjob_operator_amd.models.generate import quantize_decode_weights
from trainingjob_operator_amd.models.moe_llama import (
    MoELlamaConfig, MoELlamaModel)
from trainingjob_operator_amd.ops import reference
from trainingjob_operator_amd.ops.mx4_weight import (
    mx4_expert_tables, quantize_mx4)
from trainingjob_operator_amd.parallel.ep import expert_mx4

CFG = MoELlamaConfig(
    name="moe-mx4-cpu", vocab_size=512, hidden_size=512,
    intermediate_size=1024, num_layers=1, num_heads=8, num_kv_heads=4,
    head_dim=64, rope_theta=10000.0, n_experts=4, top_k=2)


def test_twins_against_gather_and_matmul():
    g = torch.Generator().manual_seed(1)
    E, F, K, top_k = 3, 16, 512, 2
    w = [torch.randn(2 * F, K, generator=g) * 2.0 ** e for e in range(E)]
    plain = mx4_expert_tables([quantize_mx4(x) for x in w])
    gate_up = mx4_expert_tables([quantize_mx4(x, gate_up=True) for x in w])
    x = torch.randn(3, K, generator=g).bfloat16()
    idx = torch.tensor([2, 0, 1, 1, 0, 2])
    xp = x.float()[torch.arange(6) // top_k]
    deq = torch.stack([t.dequant() for t in plain.experts])[idx]
    want = torch.einsum("nk,nmk->nm", xp, deq)
    got = reference.decode_moe_mx4(x, idx, plain, 2 * F, K, top_k)
    assert torch.allclose(got.float(), want.bfloat16().float(), rtol=2 ** -7,
                          atol=1e-6)
    gate, up = want.chunk(2, dim=-1)
    got = reference.decode_moe_swiglu_mx4(x, idx, gate_up, F, K, top_k)
    assert torch.allclose(
        got.float(), (torch.nn.functional.silu(gate) * up).bfloat16().float(),
        rtol=2 ** -7, atol=1e-6)


def test_experts_quantised_exactly_counted_and_tracked():
    torch.manual_seed(0)
    model = MoELlamaModel(CFG).eval()
    moe = model.blocks[0].moe
    before = moe.experts[1].down_proj.weight.clone()
    n = CFG.num_layers * (2 + 2 * CFG.n_experts) + 1
    assert quantize_decode_weights(model, "mxfp4") == n
    gu4, d4 = expert_mx4(moe.experts[1])
    assert gu4.gate_up and (gu4.M, gu4.K, d4.M, d4.K) == (1024, 512, 512, 512)
    assert torch.equal(torch.cat([moe.experts[1].gate_proj.weight,
                                  moe.experts[1].up_proj.weight]),
                       gu4.dequant())
    assert torch.equal(moe.experts[1].down_proj.weight, d4.dequant())
    assert not torch.equal(moe.experts[1].down_proj.weight, before)

    cpu = torch.device("cpu")
    tables = moe._mx4_tables(cpu)
    assert moe._mx4_tables(cpu) is tables               # cached
    assert tables[1].s.tolist() == [expert_mx4(ex)[1].scale.data_ptr()
                                    for ex in moe.experts]
    with torch.no_grad():                               # a written weight
        moe.experts[2].up_proj.weight.mul_(2.0)         # drops the copy
    assert expert_mx4(moe.experts[2]) is None
    assert moe._mx4_tables(cpu) is None                 # the route is off
    assert quantize_decode_weights(model, "mxfp4") == n
    rebuilt = moe._mx4_tables(cpu)
    assert rebuilt[0].experts[2] is expert_mx4(moe.experts[2])[0]
    assert rebuilt[0].experts[0] is tables[0].experts[0]


def test_fp8_after_mxfp4_is_refused():
    """The dense projections alone would already refuse; here only the
    experts carry MXFP4."""
    torch.manual_seed(0)
    model = MoELlamaModel(CFG).eval()
    quantize_decode_weights(model, "mxfp4")
    for blk in model.blocks:
        del blk.attn.qkv_proj.mx4_weight, blk.attn.o_proj.mx4_weight
    del model.lm_head.mx4_weight
    with pytest.raises(ValueError, match="already quantised to mxfp4"):
        quantize_decode_weights(model, "fp8")
