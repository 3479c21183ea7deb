"""fp8 MoE experts off the GPU: quantisation of the experts, the pointer
tables' lifetime, the torch twins of the routed fp8 GEMVs and the
weights="fp8" plumbing of an MoE model."""
import torch

from trainingjob_operator_amd.models.generate import (
    generate, quantize_decode_weights)
from trainingjob_operator_amd.models.moe_llama import (
    MOE_TINY, MoELlamaConfig, MoELlamaModel)
from trainingjob_operator_amd.ops import reference
from trainingjob_operator_amd.ops.fp8_weight import (
    expert_tables, quantize_rows)
from trainingjob_operator_amd.parallel.ep import expert_fp8

CFG = MoELlamaConfig(
    name="moe-fp8-cpu", vocab_size=512, hidden_size=512,
    intermediate_size=1024, num_layers=1, num_heads=8, num_kv_heads=4,
    head_dim=64, rope_theta=10000.0, n_experts=4, top_k=2)


def test_experts_quantised_exactly_counted_and_tracked():
    torch.manual_seed(0)
    model = MoELlamaModel(CFG).eval()
    moe = model.blocks[0].moe
    before = moe.experts[1].down_proj.weight.clone()
    router = moe.router.weight.clone()
    n = CFG.num_layers * (2 + 2 * CFG.n_experts) + 1
    assert quantize_decode_weights(model) == n
    assert torch.equal(moe.router.weight, router)
    for ex in moe.experts:
        gu8, d8 = expert_fp8(ex)
        assert gu8.gate_up and (gu8.M, gu8.K, d8.M, d8.K) == (1024, 512,
                                                              512, 512)
        assert torch.equal(torch.cat([ex.gate_proj.weight,
                                      ex.up_proj.weight]), gu8.dequant())
        assert torch.equal(ex.down_proj.weight, d8.dequant())
    assert not torch.equal(moe.experts[1].down_proj.weight, before)

    cpu = torch.device("cpu")
    tables = moe._fp8_tables(cpu)
    assert moe._fp8_tables(cpu) is tables               # cached
    assert tables[0].w.tolist() == [expert_fp8(ex)[0].packed.data_ptr()
                                    for ex in moe.experts]
    assert tables[1].s.tolist() == [expert_fp8(ex)[1].scale.data_ptr()
                                    for ex in moe.experts]
    with torch.no_grad():                               # a written weight
        moe.experts[2].up_proj.weight.mul_(2.0)         # drops the fp8 copy
    assert expert_fp8(moe.experts[2]) is None
    assert moe._fp8_tables(cpu) is None
    assert quantize_decode_weights(model) == n
    rebuilt = moe._fp8_tables(cpu)
    assert rebuilt is not tables
    assert rebuilt[0].experts[2] is expert_fp8(moe.experts[2])[0]
    assert rebuilt[0].experts[0] is tables[0].experts[0]


def test_twins_against_gather_and_matmul():
    g = torch.Generator().manual_seed(1)
    E, F, K, top_k = 3, 16, 512, 2
    w = [torch.randn(2 * F, K, generator=g) * 2.0 ** e for e in range(E)]
    plain = expert_tables([quantize_rows(x) for x in w])
    gate_up = expert_tables([quantize_rows(x, gate_up=True) for x in w])
    x = torch.randn(3, K, generator=g).bfloat16()
    idx = torch.tensor([2, 0, 1, 1, 0, 2])
    xp = x.float()[torch.arange(6) // top_k]
    deq = torch.stack([t.dequant() for t in plain.experts])[idx]
    want = torch.einsum("nk,nmk->nm", xp, deq)
    got = reference.decode_moe_fp8(x, idx, plain, 2 * F, K, top_k)
    assert torch.allclose(got.float(), want.bfloat16().float(), rtol=2 ** -7,
                          atol=1e-6)
    gate, up = want.chunk(2, dim=-1)
    got = reference.decode_moe_swiglu_fp8(x, idx, gate_up, F, K, top_k)
    assert torch.allclose(
        got.float(), (torch.nn.functional.silu(gate) * up).bfloat16().float(),
        rtol=2 ** -7, atol=1e-6)


def test_unsupported_shapes_stay_untouched():
    """moe-tiny (hidden 64): no expert is quantised, and weights="fp8"
    decodes what "bf16" decodes."""
    torch.manual_seed(0)
    model = MoELlamaModel(MOE_TINY).eval()
    before = [p.clone() for p in model.parameters()]
    prompt = torch.randint(0, MOE_TINY.vocab_size, (2, 5))
    got = generate(model, prompt, max_new_tokens=4, weights="fp8")
    assert all(expert_fp8(ex) is None
               for blk in model.blocks for ex in blk.moe.experts)
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    assert torch.equal(got, generate(model, prompt, max_new_tokens=4))
