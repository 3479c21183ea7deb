"""Zig-zag context parallelism, the parts that need neither a GPU nor a
process group: the schedule as a pure function, the shard index helpers,
the fp32 RoPE-at-positions twin, and ring_attention at world 1."""
import pytest
import torch

from trainingjob_operator_amd.parallel import cp

RANKS = (1, 2, 3, 4, 8)


def _chunks(layout, n, r, part):
    """Global chunk ids of a schedule part of rank r's shard."""
    ids = cp.cp_shard_chunks(layout, n, r)
    if part == "full":
        return ids
    assert len(ids) == 2, (layout, part)
    return ids[:1] if part == "lo" else ids[1:]


def _covered(layout, n):
    """[(q chunk, kv chunk, causal step, rank, step)] over the whole ring."""
    out = []
    for r in range(n):
        steps = cp.cp_schedule(layout, n, r)
        assert len(steps) == n
        for t, (j, qp, kvp, causal) in enumerate(steps):
            assert j == (r - t) % n
            if qp is None:
                continue
            for qc in _chunks(layout, n, r, qp):
                for kc in _chunks(layout, n, j, kvp):
                    if causal and kc > qc:
                        continue        # masked out inside the causal block
                    out.append((qc, kc, causal, r, t))
    return out


@pytest.mark.parametrize("layout", cp.LAYOUTS)
@pytest.mark.parametrize("n", RANKS)
def test_schedule_covers_the_causal_triangle_once(layout, n):
    cov = _covered(layout, n)
    nc = n if layout == "contiguous" else 2 * n
    pairs = [(qc, kc) for qc, kc, *_ in cov]
    want = [(qc, kc) for qc in range(nc) for kc in range(qc + 1)]
    assert sorted(pairs) == want          # exactly kv <= q, each once
    for qc, kc, causal, _, _ in cov:
        if qc == kc:
            assert causal, f"diagonal chunk {qc} in a non-causal step"


@pytest.mark.parametrize("n", RANKS)
def test_zigzag_gives_every_rank_equal_area_at_every_step(n):
    """key x query area in chunk^2 units, a diagonal chunk pair counting 1/2."""
    areas = {}
    for qc, kc, _, r, t in _covered("zigzag", n):
        areas[(r, t)] = areas.get((r, t), 0.0) + (0.5 if qc == kc else 1.0)
    assert len(areas) == n * n            # no idle step anywhere
    assert set(areas.values()) == {2.0}, areas


@pytest.mark.parametrize("n", RANKS)
def test_contiguous_schedule_is_the_j_le_r_rule(n):
    for r in range(n):
        j = r
        for t, step in enumerate(cp.cp_schedule("contiguous", n, r)):
            if j <= r:
                assert step == (j, "full", "full", j == r)
            else:
                assert step == (j, None, None, False)
            j = (j - 1) % n


@pytest.mark.parametrize("n", RANKS)
def test_shard_positions_permute_and_unshard_round_trips(n):
    S = 2 * n * 3
    Sc = S // (2 * n)
    pos = [cp.cp_shard_positions(S, n, r, "zigzag") for r in range(n)]
    assert sorted(torch.cat(pos).tolist()) == list(range(S))
    for r in range(n):
        lo, hi = r, 2 * n - 1 - r
        assert pos[r].tolist() == (list(range(lo * Sc, (lo + 1) * Sc))
                                   + list(range(hi * Sc, (hi + 1) * Sc)))
        assert cp.cp_shard_positions(S, n, r, "contiguous").tolist() == \
            list(range(r * S // n, (r + 1) * S // n))
    x = torch.arange(2 * S * 3).reshape(2, S, 3)
    for layout in cp.LAYOUTS:
        shards = [x.index_select(1, cp.cp_shard_positions(S, n, r, layout))
                  for r in range(n)]
        assert torch.equal(cp.cp_unshard(shards, layout), x)
    with pytest.raises(AssertionError):
        cp.cp_shard_positions(2 * n + 1, n, 0, "zigzag")


def test_rope_at_twin_equals_rows_of_the_full_rotation():
    from trainingjob_operator_amd.ops import make_inv_freq, reference as R
    torch.manual_seed(2)
    S, nh, D, n = 24, 3, 16, 3
    inv_freq = make_inv_freq(D, 10000.0)
    x = torch.randn(S, nh, D)
    full = R.rope_rotate(x, inv_freq, S)
    for r in range(n):
        pos = cp.cp_shard_positions(S, n, r, "zigzag")
        got = R.rope_at(x[pos], inv_freq, pos)
        assert torch.equal(got, full[pos])
        back = R.rope_at(got, inv_freq, pos, sign=-1.0)
        assert torch.allclose(back, x[pos], atol=1e-6)
    # batched, bf16 in and out
    xb = torch.randn(2, S, nh, D).bfloat16()
    pos = cp.cp_shard_positions(S, n, 1, "zigzag")
    got = R.rope_at(xb[:, pos], inv_freq, pos)
    want = R.rope_rotate(xb.reshape(2 * S, nh, D), inv_freq, S)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, want.reshape(2, S, nh, D)[:, pos])


def _causal_gqa(q, k, v, dy):
    B, H, S, D = q.shape
    G = H // k.shape[1]
    qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
    s = (qr @ kr.repeat_interleave(G, 1).transpose(-1, -2)) * D ** -0.5
    mask = torch.ones(S, S, dtype=torch.bool).triu(1)
    o = torch.softmax(s.masked_fill(mask, float("-inf")), -1) \
        @ vr.repeat_interleave(G, 1)
    (o * dy).sum().backward()
    return o.detach(), qr.grad, kr.grad, vr.grad


def test_ring_attention_zigzag_world1_is_causal_attention(monkeypatch):
    monkeypatch.setenv("AITJ_CP_ATTN", "block")
    torch.manual_seed(4)
    B, H, HKV, S, D = 2, 4, 2, 16, 8
    q, dy = torch.randn(B, H, S, D), torch.randn(B, H, S, D)
    k, v = torch.randn(B, HKV, S, D), torch.randn(B, HKV, S, D)
    qs, ks, vs = (t.clone().requires_grad_() for t in (q, k, v))
    o = cp.ring_attention(qs, ks, vs, None, layout="zigzag")
    (o * dy).sum().backward()
    ro, rdq, rdk, rdv = _causal_gqa(q, k, v, dy)
    assert ks.grad.shape == (B, HKV, S, D)
    for name, a, b in (("out", o, ro), ("dq", qs.grad, rdq),
                       ("dk", ks.grad, rdk), ("dv", vs.grad, rdv)):
        err = (a - b).abs().max().item()
        print(f"{name}: max abs err {err:.2e}")
        assert torch.allclose(a, b, atol=1e-5), (name, err)


def test_legacy_ring_refuses_zigzag(monkeypatch):
    monkeypatch.setenv("AITJ_CP_ATTN", "legacy")
    x = torch.zeros(1, 2, 4, 8)
    with pytest.raises(ValueError) as e:
        cp.ring_attention(x, x, x, None, layout="zigzag")
    assert "AITJ_CP_ATTN" in str(e.value) and "zigzag" in str(e.value)


def test_unknown_layout_raises(monkeypatch):
    x = torch.zeros(1, 2, 4, 8)
    with pytest.raises(ValueError):
        cp.ring_attention(x, x, x, None, layout="striped")
    with pytest.raises(ValueError):
        cp.cp_schedule("striped", 2, 0)
    with pytest.raises(ValueError):
        cp.CPLlamaModel(None, layout="striped")
    monkeypatch.setenv("AITJ_CP_LAYOUT", "striped")
    with pytest.raises(ValueError):
        cp.cp_layout_from_env()


def test_launcher_takes_cp_layout(monkeypatch):
    """--cp-layout reaches the parser with AITJ_CP_LAYOUT as its default."""
    import argparse
    from trainingjob_operator_amd.launcher import main as launcher
    seen = {}

    def parse(self, argv=None):
        for a in self._actions:
            if a.dest == "cp_layout":
                seen["default"], seen["choices"] = a.default, a.choices
        raise SystemExit(0)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    for env, want in ((None, "contiguous"), ("zigzag", "zigzag")):
        if env is None:
            monkeypatch.delenv("AITJ_CP_LAYOUT", raising=False)
        else:
            monkeypatch.setenv("AITJ_CP_LAYOUT", env)
        with pytest.raises(SystemExit):
            launcher.main([])
        assert seen["default"] == want
        assert tuple(seen["choices"]) == ("contiguous", "zigzag")
