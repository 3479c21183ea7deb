"""Native MFMA flash-attention vs torch SDPA (GPU numerics).

Order matters: the mfma_probe test pins the fragment-layout assumptions the
attention kernel is built on (guide G9: asymmetric operands so a transposed
mapping cannot pass)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.ops import native  # noqa: E402

DEV = "cuda:0"
torch.manual_seed(0)


def test_mfma_probe_layout():
    lib = native.load(require=True)
    A = (torch.randn(16, 32) * 0.5).to(torch.bfloat16).to(DEV)
    B = (torch.randn(32, 16) * 0.5).to(torch.bfloat16).to(DEV)
    C = torch.empty(16, 16, dtype=torch.float32, device=DEV)
    lib.mfma_probe(native.stream_ptr(), A.data_ptr(), B.data_ptr(),
                   C.data_ptr())
    torch.cuda.synchronize()
    ref = A.float() @ B.float()
    assert torch.allclose(C.cpu(), ref.cpu(), atol=2e-2, rtol=1e-2), \
        f"max err {(C.cpu() - ref.cpu()).abs().max()}"


@pytest.mark.parametrize("B,H,S", [(1, 4, 512), (2, 8, 1024), (1, 32, 4096)])
def test_attn_fwd_matches_sdpa(B, H, S):
    from trainingjob_operator_amd.ops.attention import flash_attention_fwd_only
    D = 128
    q = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16)
    k = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16)
    v = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16)
    out, lse = flash_attention_fwd_only(q, k, v)
    ref = torch.nn.functional.scaled_dot_product_attention(
        q, k, v, is_causal=True)
    assert torch.allclose(out.float(), ref.float(), atol=3e-2, rtol=2e-2), \
        f"max err {(out.float() - ref.float()).abs().max()}"
    # lse vs fp32 reference on one head
    scores = (q[0, 0].float() @ k[0, 0].float().T) / math.sqrt(D)
    mask = torch.triu(torch.ones(S, S, device=DEV, dtype=torch.bool), 1)
    scores = scores.masked_fill(mask, float("-inf"))
    lse_ref = torch.logsumexp(scores, dim=-1)
    assert torch.allclose(lse[0, 0], lse_ref, atol=2e-2, rtol=1e-3), \
        f"lse max err {(lse[0, 0] - lse_ref).abs().max()}"


def test_attn_and_rmsnorm_grads_repeat_bit_exact():
    """The same inputs give the same bits every time: the attention kernels
    only read LDS tiles their own wave waited for or a barrier published,
    and the RMSNorm weight gradient is summed in a fixed order (no
    atomics). GQA shape with more than one 256-row q block and an RMSNorm
    row count that spans several reduce chunks."""
    from trainingjob_operator_amd.ops import fused_rmsnorm
    from trainingjob_operator_amd.ops.attention import flash_attention
    B, H, HKV, S, D = 2, 8, 2, 1024, 128
    g = torch.Generator(device=DEV).manual_seed(7)
    q0 = (torch.randn(B, H, S, D, device=DEV, generator=g) * 0.5).bfloat16()
    k0 = (torch.randn(B, HKV, S, D, device=DEV, generator=g) * 0.5).bfloat16()
    v0 = (torch.randn(B, HKV, S, D, device=DEV, generator=g) * 0.5).bfloat16()
    go = (torch.randn(B, H, S, D, device=DEV, generator=g) * 0.5).bfloat16()
    x0 = torch.randn(4100, 4096, device=DEV, generator=g).bfloat16()
    w0 = torch.randn(4096, device=DEV, generator=g).bfloat16()
    gy = torch.randn(4100, 4096, device=DEV, generator=g).bfloat16()

    def once():
        q, k, v = (t.clone().requires_grad_() for t in (q0, k0, v0))
        out = flash_attention(q, k, v)
        out.backward(go)
        x, w = x0.clone().requires_grad_(), w0.clone().requires_grad_()
        y, _ = fused_rmsnorm(x, w)
        y.backward(gy)
        return out.detach(), q.grad, k.grad, v.grad, x.grad, w.grad

    first = once()
    for _ in range(3):
        for name, a, b in zip(("out", "dq", "dk", "dv", "dx", "dw"),
                              first, once()):
            assert torch.equal(a, b), name


def test_attn_fwd_strided_inputs():
    """The model passes [B,S,H,D]-permuted views; strides must be honored."""
    from trainingjob_operator_amd.ops.attention import flash_attention_fwd_only
    B, H, S, D = 1, 8, 512, 128
    base = (torch.randn(B, S, H, D, device=DEV) * 0.5).to(torch.bfloat16)
    qp = base.permute(0, 2, 1, 3)  # [B,H,S,D], non-contiguous
    out, _ = flash_attention_fwd_only(qp, qp, qp)
    ref = torch.nn.functional.scaled_dot_product_attention(
        qp, qp, qp, is_causal=True)
    assert torch.allclose(out.float(), ref.float(), atol=3e-2, rtol=2e-2)


def test_attn_backward_via_aten():
    from trainingjob_operator_amd.ops.attention import flash_attention
    B, H, S, D = 1, 4, 1024, 128
    q = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16) \
        .requires_grad_()
    k = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16) \
        .requires_grad_()
    v = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16) \
        .requires_grad_()
    out = flash_attention(q, k, v)
    gout = torch.randn_like(out)
    (out.float() * gout.float()).sum().backward()

    q2 = q.detach().clone().requires_grad_()
    k2 = k.detach().clone().requires_grad_()
    v2 = v.detach().clone().requires_grad_()
    ref = torch.nn.functional.scaled_dot_product_attention(
        q2, k2, v2, is_causal=True)
    (ref.float() * gout.float()).sum().backward()

    for a, b, name in ((q, q2, "dq"), (k, k2, "dk"), (v, v2, "dv")):
        assert torch.allclose(a.grad.float(), b.grad.float(), atol=5e-2,
                              rtol=5e-2), \
            f"{name} max err {(a.grad.float() - b.grad.float()).abs().max()}"


def test_model_with_native_attention(monkeypatch):
    monkeypatch.setenv("AITJ_SDPA_BACKEND", "native")
    from trainingjob_operator_amd.training import TrainConfig, Trainer
    cfg = TrainConfig(model="llama-smoke", micro_batch=1, grad_accum=1,
                      seq_len=512, lr=1e-3)
    trainer = Trainer(cfg)
    l0 = trainer.train_step().item()
    assert l0 == l0
    torch.cuda.synchronize()


def test_mfma_probe32_layout():
    """v6 kernel's 32x32x16 fragment maps (asymmetric operands, G9)."""
    lib = native.load(require=True)
    A = (torch.randn(32, 16) * 0.5).to(torch.bfloat16).to(DEV)
    B = (torch.randn(16, 32) * 0.5).to(torch.bfloat16).to(DEV)
    C = torch.empty(32, 32, dtype=torch.float32, device=DEV)
    lib.mfma_probe32(native.stream_ptr(), A.data_ptr(), B.data_ptr(),
                     C.data_ptr())
    torch.cuda.synchronize()
    ref = A.float() @ B.float()
    assert torch.allclose(C.cpu(), ref.cpu(), atol=2e-2, rtol=1e-2), \
        f"max err {(C.cpu() - ref.cpu()).abs().max()}"


def test_attn_fwd_gqa():
    """v6 native GQA: kv heads fewer than q heads (llama-3 8:1 grouping)."""
    from trainingjob_operator_amd.ops.attention import flash_attention_fwd_only
    B, H, HKV, S, D = 2, 16, 4, 1024, 128
    q = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16)
    k = (torch.randn(B, HKV, S, D, device=DEV) * 0.5).to(torch.bfloat16)
    v = (torch.randn(B, HKV, S, D, device=DEV) * 0.5).to(torch.bfloat16)
    out, lse = flash_attention_fwd_only(q, k, v)
    ref = torch.nn.functional.scaled_dot_product_attention(
        q, k, v, is_causal=True, enable_gqa=True)
    assert torch.allclose(out.float(), ref.float(), atol=3e-2, rtol=2e-2), \
        f"max err {(out.float() - ref.float()).abs().max()}"


def test_attn_fwd_forced_rescale():
    """T13 defer-rescale branch test (guide rule 26): spike one K row so the
    running max jumps past THR at a late tile; compare against fp32 ref."""
    from trainingjob_operator_amd.ops.attention import flash_attention_fwd_only
    B, H, S, D = 1, 2, 1024, 128
    q = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16)
    k = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16)
    v = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16)
    # spike: K row 700 strongly aligned with EVERY q row -> max jump at the
    # tile containing kv=700 for all q >= 700
    k[:, :, 700, :] = (q.float().mean(dim=2) * 40.0).to(
        torch.bfloat16).unsqueeze(2)[:, :, 0, :]
    out, _ = flash_attention_fwd_only(q, k, v)
    sc = 1.0 / math.sqrt(D)
    for h in range(H):
        scores = (q[0, h].float() @ k[0, h].float().T) * sc
        mask = torch.triu(torch.ones(S, S, device=DEV, dtype=torch.bool), 1)
        scores = scores.masked_fill(mask, float("-inf"))
        ref = torch.softmax(scores, dim=-1) @ v[0, h].float()
        err = (out[0, h].float() - ref).abs().max()
        assert err < 5e-2, f"head {h} max err {err}"


def test_attn_gqa_backward_via_aten():
    """GQA fwd (v6) + aten backward must reduce dk/dv to the kv heads."""
    from trainingjob_operator_amd.ops.attention import flash_attention
    B, H, HKV, S, D = 1, 8, 2, 512, 128
    q = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16) \
        .requires_grad_()
    k = (torch.randn(B, HKV, S, D, device=DEV) * 0.5).to(torch.bfloat16) \
        .requires_grad_()
    v = (torch.randn(B, HKV, S, D, device=DEV) * 0.5).to(torch.bfloat16) \
        .requires_grad_()
    out = flash_attention(q, k, v)
    gout = torch.randn_like(out)
    (out.float() * gout.float()).sum().backward()

    q2 = q.detach().clone().requires_grad_()
    k2 = k.detach().clone().requires_grad_()
    v2 = v.detach().clone().requires_grad_()
    ref = torch.nn.functional.scaled_dot_product_attention(
        q2, k2, v2, is_causal=True, enable_gqa=True)
    (ref.float() * gout.float()).sum().backward()
    for a, b, name in ((q, q2, "dq"), (k, k2, "dk"), (v, v2, "dv")):
        assert a.grad.shape == b.grad.shape
        assert torch.allclose(a.grad.float(), b.grad.float(), atol=5e-2,
                              rtol=5e-2), \
            f"{name} max err {(a.grad.float() - b.grad.float()).abs().max()}"


def test_attn_native_backward_matches_ref():
    """Hand-written backward (delta/dq/dv/dk kernels) vs fp32 autograd."""
    from trainingjob_operator_amd.ops.attention import flash_attention
    for B, H, HKV, S in ((1, 4, 4, 512), (2, 8, 2, 1024), (1, 32, 8, 4096)):
        D = 128
        torch.manual_seed(B * 100 + S)
        q = (torch.randn(B, H, S, D, device=DEV) * 0.5).to(torch.bfloat16) \
            .requires_grad_()
        k = (torch.randn(B, HKV, S, D, device=DEV) * 0.5).to(torch.bfloat16) \
            .requires_grad_()
        v = (torch.randn(B, HKV, S, D, device=DEV) * 0.5).to(torch.bfloat16) \
            .requires_grad_()
        out = flash_attention(q, k, v)
        gout = torch.randn_like(out) * 0.5
        (out.float() * gout.float()).sum().backward()

        q2 = q.detach().clone().requires_grad_()
        k2 = k.detach().clone().requires_grad_()
        v2 = v.detach().clone().requires_grad_()
        ref = torch.nn.functional.scaled_dot_product_attention(
            q2, k2, v2, is_causal=True, enable_gqa=HKV != H)
        (ref.float() * gout.float()).sum().backward()
        for a, b2, name in ((q, q2, "dq"), (k, k2, "dk"), (v, v2, "dv")):
            err = (a.grad.float() - b2.grad.float()).abs().max()
            ok = torch.allclose(a.grad.float(), b2.grad.float(), atol=7e-2,
                                rtol=5e-2)
            assert ok, f"{name} max err {err} at B{B} H{H} HKV{HKV} S{S}"


def test_attn_fwd_fallback_shapes():
    """Dispatch coverage: S%128-only -> NW4 kernel; S%64-only (equal
    heads) -> v5 kernel. Both against library SDPA."""
    from trainingjob_operator_amd.ops.attention import flash_attention_fwd_only
    for B, H, HKV, S in ((1, 4, 2, 384),    # NW4 (S%256!=0, %128==0), GQA
                         (1, 4, 4, 192)):   # v5 (S%128!=0, %64==0)
        q = (torch.randn(B, H, S, 128, device=DEV) * 0.5).to(torch.bfloat16)
        k = (torch.randn(B, HKV, S, 128, device=DEV) * 0.5).to(torch.bfloat16)
        v = (torch.randn(B, HKV, S, 128, device=DEV) * 0.5).to(torch.bfloat16)
        if HKV != H and S % 128 != 0:
            k = k.repeat_interleave(H // HKV, dim=1)
            v = v.repeat_interleave(H // HKV, dim=1)
        out, _ = flash_attention_fwd_only(q, k, v)
        ref = torch.nn.functional.scaled_dot_product_attention(
            q, k, v, is_causal=True, enable_gqa=k.shape[1] != H)
        assert torch.allclose(out.float(), ref.float(), atol=3e-2,
                              rtol=2e-2), f"S={S}"


def test_fp8_projections_loss_parity(monkeypatch):
    """Opt-in fp8 forward projections: short-horizon loss parity vs bf16
    (the gate for publishing an fp8 config)."""
    import torch as t
    from trainingjob_operator_amd.training import TrainConfig, Trainer
    monkeypatch.delenv("AITJ_FP8_PROJ", raising=False)
    t.manual_seed(0)
    cfg = TrainConfig(model="llama-smoke", micro_batch=1, grad_accum=1,
                      seq_len=512, lr=1e-4)
    tr_bf = Trainer(cfg)
    l_bf = [float(tr_bf.train_step()) for _ in range(6)]
    del tr_bf
    t.cuda.empty_cache()
    t.manual_seed(0)
    cfg8 = TrainConfig(model="llama-smoke", micro_batch=1, grad_accum=1,
                      seq_len=512, lr=1e-4, fp8_projections=True)
    tr_f8 = Trainer(cfg8)
    l_f8 = [float(tr_f8.train_step()) for _ in range(6)]
    monkeypatch.delenv("AITJ_FP8_PROJ", raising=False)
    for a, b in zip(l_bf, l_f8):
        assert abs(a - b) < 0.15, (l_bf, l_f8)


def test_prompt_lookup_identical_on_gpu():
    """Speculative verify exercises the mid-cache offset-causal mask and
    the fused decode path on silicon; output must equal plain greedy."""
    import torch
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.generate import (
        generate, generate_lookup,
    )
    from trainingjob_operator_amd.training import build_model
    torch.manual_seed(3)
    m = build_model(CONFIGS["llama-smoke"], torch.device("cuda:0"))
    prompt = torch.tensor([[11, 12, 13, 11, 12, 13, 11, 12]],
                          device="cuda:0")
    ref = generate(m, prompt, max_new_tokens=24)
    got = generate_lookup(m, prompt, max_new_tokens=24, lookup_k=6)
    assert torch.equal(ref, got), (ref, got)
