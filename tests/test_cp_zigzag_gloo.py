"""The zig-zag context-parallel layout over gloo on CPU (AITJ_CP_ATTN=block,
fp32 reference twins of the block ops): rectangular ring steps, per-half
lse merge, the low-half travelling dK/dV, and the sharded model against
the unsharded one."""
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
        from trainingjob_operator_amd.parallel.cp import (
            cp_shard_positions, ring_attention,
        )
        torch.manual_seed(5)
        B, H, HKV, S, D = 2, 4, 2, 16, 8
        Sb = S // world
        q = torch.randn(B, H, S, D)
        k = torch.randn(B, HKV, S, D)
        v = torch.randn(B, HKV, S, D)
        dy = torch.randn(B, H, S, D)

        rows = cp_shard_positions(S, world, rank, "zigzag")
        qs = q[:, :, rows].clone().requires_grad_()
        ks = k[:, :, rows].clone().requires_grad_()   # unexpanded: HKV heads
        vs = v[:, :, rows].clone().requires_grad_()
        o = ring_attention(qs, ks, vs, None, layout="zigzag")
        (o * dy[:, :, rows]).sum().backward()

        ro, rdq, rdk, rdv = _causal_gqa(q, k, v, dy)
        assert ks.grad.shape == (B, HKV, Sb, D)
        errs = {}
        for name, a, b in (("fwd", o, ro), ("dq", qs.grad, rdq),
                           ("dk", ks.grad, rdk), ("dv", vs.grad, rdv)):
            errs[name] = (a - b[:, :, rows]).abs().max().item()
            assert torch.allclose(a, b[:, :, rows], atol=1e-5), \
                (name, errs[name])
        print(f"rank {rank}/{world} max abs err {errs}")
        results[rank] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_zigzag_ring_attention_matches_full(world):
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
        cp = CPLlamaModel(cfg, layout="zigzag").float()
        cp.shard_from_full(full)

        g = torch.Generator().manual_seed(23)
        tokens = torch.randint(0, cfg.vocab_size, (2, 32), generator=g)
        targets = torch.randint(0, cfg.vocab_size, (2, 32), generator=g)

        loss = cp(tokens, targets)
        loss.backward()
        cp.allreduce_cp_grads()
        # every rank computes at every ring step
        assert calls[0] == cfg.num_layers * world, calls[0]

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


def test_cp_llama_zigzag_matches_unsharded():
    world = 2
    results = mp.Manager().dict()
    mp.spawn(_cp_model_worker, args=(world, _free_port(), results),
             nprocs=world, join=True)
    assert len(results) == world
    assert abs(results[0] - results[1]) < 1e-6
