"""The block-structured ring (AITJ_CP_ATTN=block) over gloo on CPU: the
lse-merge forward, the global-lse backward and the HKV-head travelling
gradients, on the fp32 reference twins of the native block ops."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _causal_gqa(q, k, v, dy):
    """Plain causal GQA attention; returns out and dq/dk/dv (HKV heads)."""
    B, H, S, D = q.shape
    G = H // k.shape[1]
    qr = q.clone().requires_grad_()
    kr = k.clone().requires_grad_()
    vr = v.clone().requires_grad_()
    ke = kr.repeat_interleave(G, dim=1)
    ve = vr.repeat_interleave(G, dim=1)
    s = (qr @ ke.transpose(-1, -2)) * D ** -0.5
    mask = torch.ones(S, S, dtype=torch.bool).triu(1)
    p = torch.softmax(s.masked_fill(mask, float("-inf")), dim=-1)
    o = p @ ve
    (o * dy).sum().backward()
    return o.detach(), qr.grad, kr.grad, vr.grad


def _ring_worker(rank, world, port, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["AITJ_CP_ATTN"] = "block"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from trainingjob_operator_amd.parallel.cp import ring_attention
        torch.manual_seed(5)
        B, H, HKV, S, D = 2, 4, 2, 16, 8
        Sb = S // world
        q = torch.randn(B, H, S, D)
        k = torch.randn(B, HKV, S, D)
        v = torch.randn(B, HKV, S, D)
        dy = torch.randn(B, H, S, D)

        sl = slice(rank * Sb, (rank + 1) * Sb)
        qs = q[:, :, sl].clone().requires_grad_()
        ks = k[:, :, sl].clone().requires_grad_()    # unexpanded: HKV heads
        vs = v[:, :, sl].clone().requires_grad_()
        o = ring_attention(qs, ks, vs, None)
        (o * dy[:, :, sl]).sum().backward()

        ro, rdq, rdk, rdv = _causal_gqa(q, k, v, dy)
        assert ks.grad.shape == (B, HKV, Sb, D)
        assert torch.allclose(o, ro[:, :, sl], atol=1e-5), "fwd"
        assert torch.allclose(qs.grad, rdq[:, :, sl], atol=1e-5), "dq"
        assert torch.allclose(ks.grad, rdk[:, :, sl], atol=1e-5), "dk"
        assert torch.allclose(vs.grad, rdv[:, :, sl], atol=1e-5), "dv"
        results[rank] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_block_ring_attention_matches_full(world):
    results = mp.Manager().dict()
    mp.spawn(_ring_worker, args=(world, _free_port(), results),
             nprocs=world, join=True)
    assert len(results) == world


def _cp_model_worker(rank, world, port, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["AITJ_CP_ATTN"] = "block"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from trainingjob_operator_amd.models.config import CONFIGS
        from trainingjob_operator_amd.models.llama import LlamaModel
        from trainingjob_operator_amd.ops import reference
        from trainingjob_operator_amd.parallel.cp import CPLlamaModel
        calls = [0]
        orig = reference.attention_block_fwd

        def counted(*a, **kw):
            calls[0] += 1
            return orig(*a, **kw)
        reference.attention_block_fwd = counted

        cfg = CONFIGS["llama-tiny"]
        torch.manual_seed(17)
        full = LlamaModel(cfg).float()
        cp = CPLlamaModel(cfg).float()
        cp.shard_from_full(full)

        g = torch.Generator().manual_seed(23)
        tokens = torch.randint(0, cfg.vocab_size, (2, 32), generator=g)
        targets = torch.randint(0, cfg.vocab_size, (2, 32), generator=g)

        loss = cp(tokens, targets)
        loss.backward()
        cp.allreduce_cp_grads()
        # rank r visits r + 1 blocks per layer
        assert calls[0] == cfg.num_layers * (rank + 1), calls[0]

        ref_loss = full(tokens, targets)
        ref_loss.backward()

        assert torch.allclose(loss, ref_loss, atol=1e-4), \
            (float(loss), float(ref_loss))
        ref = dict(full.named_parameters())
        for name, p in cp.named_parameters():
            assert p.grad is not None, name
            assert torch.allclose(p.grad, ref[name].grad, atol=1e-4,
                                  rtol=1e-3), name
        results[rank] = float(loss)
    finally:
        dist.destroy_process_group()


def test_cp_llama_block_matches_unsharded():
    world = 2
    results = mp.Manager().dict()
    mp.spawn(_cp_model_worker, args=(world, _free_port(), results),
             nprocs=world, join=True)
    assert len(results) == world
    assert abs(results[0] - results[1]) < 1e-6


def test_cp_attn_mode_rejects_unknown(monkeypatch):
    from trainingjob_operator_amd.parallel import cp
    monkeypatch.setenv("AITJ_CP_ATTN", "fast")
    with pytest.raises(ValueError):
        cp.uses_block_path(torch.zeros(1, 2, 4, 8), torch.zeros(1, 2, 4, 8))
    monkeypatch.setenv("AITJ_CP_ATTN", "legacy")
    assert not cp.uses_block_path(torch.zeros(1, 2, 4, 8),
                                  torch.zeros(1, 2, 4, 8))
    monkeypatch.delenv("AITJ_CP_ATTN")
    # auto on CPU: the native ops do not apply -> legacy path
    assert not cp.uses_block_path(torch.zeros(1, 2, 4, 8),
                                  torch.zeros(1, 2, 4, 8))


def test_reference_block_ops_match_full_softmax():
    """Two non-causal kv halves merged == softmax over all keys, forward
    and backward (global lse/delta), with GQA; causal block == masked
    softmax; the -inf accumulator start reproduces the block."""
    from trainingjob_operator_amd.ops import reference as R
    torch.manual_seed(3)
    B, H, HKV, Sq, Skv, D = 2, 4, 2, 8, 16, 8
    G = H // HKV
    q = torch.randn(B, H, Sq, D)
    k = torch.randn(B, HKV, Skv, D)
    v = torch.randn(B, HKV, Skv, D)
    dy = torch.randn(B, H, Sq, D)
    scale = D ** -0.5

    qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
    s = (qr @ kr.repeat_interleave(G, 1).transpose(-1, -2)) * scale
    ref = torch.softmax(s, dim=-1) @ vr.repeat_interleave(G, 1)
    (ref * dy).sum().backward()
    ref_lse = torch.logsumexp(s.detach(), dim=-1)

    o_acc = torch.zeros(B, H, Sq, D)
    lse_acc = torch.full((B, H, Sq), float("-inf"))
    halves = [slice(0, 8), slice(8, 16)]
    for i, sl in enumerate(halves):
        o_b, lse_b = R.attention_block_fwd(q, k[:, :, sl], v[:, :, sl], False)
        R.attn_merge_(o_acc, lse_acc, o_b, lse_b)
        if i == 0:
            assert torch.equal(o_acc, o_b) and torch.equal(lse_acc, lse_b)
    assert not torch.isnan(o_acc).any()
    assert torch.allclose(o_acc, ref.detach(), atol=1e-5)
    assert torch.allclose(lse_acc, ref_lse, atol=1e-5)

    delta = R.attention_delta(o_acc, dy)
    assert torch.allclose(delta, (ref.detach() * dy).sum(-1), atol=1e-5)
    dq = torch.zeros_like(q)
    for sl in halves:
        dq_b, dk_b, dv_b = R.attention_block_bwd(
            q, k[:, :, sl], v[:, :, sl], dy, lse_acc, delta, False)
        assert dk_b.shape == (B, HKV, 8, D)
        dq += dq_b
        assert torch.allclose(dk_b, kr.grad[:, :, sl], atol=1e-5)
        assert torch.allclose(dv_b, vr.grad[:, :, sl], atol=1e-5)
    assert torch.allclose(dq, qr.grad, atol=1e-5)

    # causal square block against masked softmax
    kc, vc = k[:, :, :Sq], v[:, :, :Sq]
    sc = (q @ kc.repeat_interleave(G, 1).transpose(-1, -2)) * scale
    mask = torch.ones(Sq, Sq, dtype=torch.bool).triu(1)
    pc = torch.softmax(sc.masked_fill(mask, float("-inf")), dim=-1)
    o_c, _ = R.attention_block_fwd(q, kc, vc, True)
    assert torch.allclose(o_c, pc @ vc.repeat_interleave(G, 1), atol=1e-5)

    # both sides at -inf: stays (0, -inf), no NaN
    o0 = torch.zeros(1, 1, 2, D)
    l0 = torch.full((1, 1, 2), float("-inf"))
    R.attn_merge_(o0, l0, torch.zeros(1, 1, 2, D),
                  torch.full((1, 1, 2), float("-inf")))
    assert not torch.isnan(o0).any() and not torch.isnan(l0).any()
