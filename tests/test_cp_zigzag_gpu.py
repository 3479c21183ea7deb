"""The zig-zag context-parallel layout on the native kernels (GPU): the
ring schedule played on one device through the public block ops, the
packed CP attention op inside CPLlamaModel at world 1, and the packed op as
each rank of an emulated ring of two."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 128
FWD_TOL = dict(atol=3e-2, rtol=2e-2)
GRAD_TOL = dict(atol=7e-2, rtol=5e-2)


def _rand(gen, *shape):
    return (torch.randn(*shape, device=DEV, generator=gen) * 0.5).bfloat16()


def _close(a, b, tol, name):
    err = (a.float() - b.float()).abs().max().item()
    print(f"{name}: max abs err {err:.5f}")
    assert torch.allclose(a.float(), b.float(), **tol), f"{name} max err {err}"


def _emulated_zigzag_ring(q, k, v, gout, n):
    """Every virtual rank's cp_schedule on one device, through the public
    block ops only; shards are gathered by cp_shard_positions and results
    scattered back to global order."""
    from trainingjob_operator_amd.ops.attention import (
        attn_merge_, flash_attention_block_bwd, flash_attention_block_fwd,
        flash_attention_delta,
    )
    from trainingjob_operator_amd.parallel.cp import (
        _part, cp_schedule, cp_shard_positions,
    )
    B, H, S, _ = q.shape
    Sc = S // (2 * n)
    rows = [cp_shard_positions(S, n, r, "zigzag").to(DEV) for r in range(n)]
    out = torch.empty_like(q)
    dq = torch.empty_like(q)
    dk = torch.zeros(k.shape, dtype=torch.float32, device=DEV)
    dv = torch.zeros(v.shape, dtype=torch.float32, device=DEV)
    ks = [k[:, :, rw].contiguous() for rw in rows]
    vs = [v[:, :, rw].contiguous() for rw in rows]
    for r in range(n):
        qr, gr = q[:, :, rows[r]].contiguous(), gout[:, :, rows[r]].contiguous()
        sched = cp_schedule("zigzag", n, r)
        acc = [(torch.zeros(B, H, Sc, D, dtype=torch.float32, device=DEV),
                torch.full((B, H, Sc), float("-inf"), dtype=torch.float32,
                           device=DEV)) for _ in range(2)]
        for j, qp, kvp, causal in sched:
            o_j, lse_j = flash_attention_block_fwd(
                _part(qr, qp), _part(ks[j], kvp), _part(vs[j], kvp), causal)
            if qp == "full":
                for (o_acc, lse_acc), p in zip(acc, ("lo", "hi")):
                    attn_merge_(o_acc, lse_acc, _part(o_j, p),
                                _part(lse_j, p))
            else:
                assert qp == "hi"
                attn_merge_(acc[1][0], acc[1][1], o_j, lse_j)
        out_r = torch.cat([a[0] for a in acc], dim=2).bfloat16()
        lse_r = torch.cat([a[1] for a in acc], dim=2)
        out[:, :, rows[r]] = out_r
        delta = flash_attention_delta(out_r, gr)
        dq_r = torch.zeros(B, H, 2 * Sc, D, dtype=torch.float32, device=DEV)
        for j, qp, kvp, causal in sched:
            dq_b, dk_b, dv_b = flash_attention_block_bwd(
                _part(qr, qp), _part(ks[j], kvp), _part(vs[j], kvp),
                _part(gr, qp), _part(lse_r, qp), _part(delta, qp), causal)
            _part(dq_r, qp).add_(dq_b)
            kv_rows = _part(rows[j], kvp, dim=0)
            dk[:, :, kv_rows] += dk_b
            dv[:, :, kv_rows] += dv_b
        dq[:, :, rows[r]] = dq_r.bfloat16()
    return out, dq, dk.bfloat16(), dv.bfloat16()


@pytest.mark.parametrize("n", [2, 4])
def test_emulated_zigzag_ring_matches_dense_causal(n):
    B, H, HKV, Sc = 1, 4, 2, 256
    S = 2 * n * Sc
    g = torch.Generator(device=DEV).manual_seed(60 + n)
    q, gout = _rand(g, B, H, S, D), _rand(g, B, H, S, D)
    k, v = _rand(g, B, HKV, S, D), _rand(g, B, HKV, S, D)
    out, dq, dk, dv = _emulated_zigzag_ring(q, k, v, gout, n)
    q32, k32, v32 = (t.float().requires_grad_() for t in (q, k, v))
    ro = torch.nn.functional.scaled_dot_product_attention(
        q32, k32, v32, is_causal=True, enable_gqa=True)
    (ro * gout.float()).sum().backward()
    _close(out, ro.detach(), FWD_TOL, "out")
    _close(dq, q32.grad, GRAD_TOL, "dq")
    _close(dk, k32.grad, GRAD_TOL, "dk")
    _close(dv, v32.grad, GRAD_TOL, "dv")


# Spread between the legacy fp32-matmul ring and the dense LlamaModel, both
# bf16 models of the same math (tests/test_block_attention_gpu.py,
# profiles/r04_ring_attention.md). A CP path on the native kernels may
# differ from the dense model by twice that, the margin the block-path test
# there uses.
LEGACY_VS_DENSE = dict(loss=3.73e-4, qkv=8.43e-3, o=8.33e-3)


def _world1(monkeypatch, layout):
    """loss + layer-0 qkv_proj/o_proj grads at world 1 with the setup of
    _cp_world1 in tests/test_block_attention_gpu.py (llama-smoke, seq 512,
    seeds 17/23, bf16 projections). layout None: the dense LlamaModel."""
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.ops import make_inv_freq
    from trainingjob_operator_amd.parallel import cp
    from trainingjob_operator_amd.training import build_model
    cfg = CONFIGS["llama-smoke"]
    monkeypatch.delenv("AITJ_FP8_PROJ", raising=False)
    monkeypatch.delenv("AITJ_CP_ATTN", raising=False)
    torch.manual_seed(17)
    full = build_model(cfg, torch.device(DEV))
    g = torch.Generator().manual_seed(23)
    tokens = torch.randint(0, cfg.vocab_size, (1, 512), generator=g).to(DEV)
    targets = torch.randint(0, cfg.vocab_size, (1, 512), generator=g).to(DEV)
    packed = [0]
    if layout is None:
        model = full
    else:
        with torch.device(DEV):
            model = cp.CPLlamaModel(cfg, layout=layout)
        model = model.to(torch.bfloat16)
        model.inv_freq = make_inv_freq(cfg.head_dim, cfg.rope_theta,
                                       device=DEV)
        model.shard_from_full(full)

        def no_torch_rope(*a, **kw):
            raise AssertionError("the torch _rope_offset ran")
        monkeypatch.setattr(cp, "_rope_offset", no_torch_rope)
        orig = cp._PackedCPAttention.apply

        def counted(*a, **kw):
            packed[0] += 1
            return orig(*a, **kw)
        monkeypatch.setattr(cp._PackedCPAttention, "apply", counted)
    loss = model(tokens, targets)
    loss.backward()
    attn = model.blocks[0].attn
    return (loss.item(), attn.qkv_proj.weight.grad.float(),
            attn.o_proj.weight.grad.float(), packed[0])


def _spread(a, b):
    return dict(loss=abs(a[0] - b[0]),
                qkv=((a[1] - b[1]).abs().max() / b[1].abs().max()).item(),
                o=((a[2] - b[2]).abs().max() / b[2].abs().max()).item())


@pytest.fixture(scope="module")
def dense():
    mp = pytest.MonkeyPatch()
    try:
        yield _world1(mp, None)
    finally:
        mp.undo()


@pytest.mark.parametrize("layout,packed_env", [("zigzag", None),
                                               ("contiguous", "1")])
def test_cp_model_world1_packed_op_matches_dense(monkeypatch, dense, layout,
                                                 packed_env):
    """Zig-zag takes the packed op by itself, a contiguous shard under
    AITJ_CP_PACKED=1; neither runs the torch RoPE."""
    from trainingjob_operator_amd.models.config import CONFIGS
    if packed_env is None:
        monkeypatch.delenv("AITJ_CP_PACKED", raising=False)
    else:
        monkeypatch.setenv("AITJ_CP_PACKED", packed_env)
    got = _world1(monkeypatch, layout)
    assert got[3] == CONFIGS["llama-smoke"].num_layers, \
        "the packed CP attention op did not run in every layer"
    spread = _spread(got, dense)
    print(f"{layout} packed vs dense:", spread,
          "(exactly zero)" if not any(spread.values()) else "",
          "legacy vs dense:", LEGACY_VS_DENSE)
    for key, bound in LEGACY_VS_DENSE.items():
        assert spread[key] <= 2 * bound, (key, spread[key], bound)


@pytest.mark.parametrize("layout", ["zigzag", "contiguous"])
def test_packed_cp_op_on_an_emulated_two_rank_ring(monkeypatch, layout):
    """_PackedCPAttention as rank 0 and rank 1 of a ring of two on one
    device: the rank and the ring shift are patched so that the other
    rank's rotated K and V arrive as the ring would deliver them. Checks
    what is local to a rank, its output rows and its un-rotated dq, against
    fp32 RoPE + causal SDPA over the whole sequence; the rectangular steps
    run on the strided views of the packed buffers here. dK/dV travel
    between ranks and are covered by the emulated ring above and the gloo
    tests."""
    from trainingjob_operator_amd.ops import make_inv_freq, reference as R
    from trainingjob_operator_amd.ops.attention import rope_packed_at
    from trainingjob_operator_amd.parallel import cp
    n, B, H, HKV, Sb = 2, 1, 4, 2, 512
    S, W = n * Sb, (H + 2 * HKV) * D
    g = torch.Generator(device=DEV).manual_seed(81)
    qkv = _rand(g, B, S, W)
    gout = _rand(g, B, S, H * D)
    inv_freq = make_inv_freq(D, 500000.0, device=DEV)
    rows = [cp.cp_shard_positions(S, n, r, layout).to(DEV) for r in range(n)]
    shards = [qkv[:, rw].contiguous() for rw in rows]
    K, V = [], []
    for r in range(n):
        rot = torch.empty(B, Sb, (H + HKV) * D, dtype=torch.bfloat16,
                          device=DEV)
        rope_packed_at(shards[r], rot, inv_freq, H + HKV, Sb,
                       *cp._shard_segments(layout, n, r, Sb))
        _, k, v = cp._PackedCPAttention._views(rot, shards[r], B, Sb, H, HKV,
                                               D)
        K.append(k.contiguous())
        V.append(v.contiguous())

    x = qkv.float().view(B, S, H + 2 * HKV, D)
    qf = x[:, :, :H].clone().requires_grad_()
    pos = torch.arange(S, device=DEV)
    ro = torch.nn.functional.scaled_dot_product_attention(
        R.rope_at(qf, inv_freq, pos).transpose(1, 2),
        R.rope_at(x[:, :, H:H + HKV], inv_freq, pos).transpose(1, 2),
        x[:, :, H + HKV:].transpose(1, 2), is_causal=True, enable_gqa=True)
    ro = ro.transpose(1, 2).reshape(B, S, H * D)
    (ro * gout.float()).sum().backward()
    rdq = qf.grad.reshape(B, S, H * D)

    for r in range(n):
        step = [0]

        def shift(tensors, group, r=r):
            step[0] += 1
            j = (r - step[0]) % n
            out = [K[j], V[j]]
            if len(tensors) == 4:   # travelling dK/dV: a fresh pair arrives
                out += [torch.zeros_like(tensors[2]),
                        torch.zeros_like(tensors[3])]
            return out
        monkeypatch.setattr(cp, "_ring_rank", lambda group, r=r: (n, r))
        monkeypatch.setattr(cp, "_ring_shift", shift)
        x_r = shards[r].clone().requires_grad_()
        o = cp._PackedCPAttention.apply(x_r, inv_freq, H, HKV, D ** -0.5,
                                        None, layout)
        step[0] = 0                 # the backward is a second ring pass
        o.backward(gout[:, rows[r]].contiguous())
        _close(o, ro.detach()[:, rows[r]], FWD_TOL, f"rank {r} out")
        _close(x_r.grad[..., :H * D], rdq[:, rows[r]], GRAD_TOL,
               f"rank {r} dq")
