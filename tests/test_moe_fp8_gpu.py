"""Routed fp8 decode GEMVs (hip/ops.hip gemv_moe_fp8 / gemv_moe_fp8_swiglu):
every pair against the one-row dense fp8 GEMV over its expert (bit for bit),
against fp64 over the dequantised experts, with the unhit experts poisoned,
and through cached decode steps of a small MoE model."""
import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.models.generate import (  # noqa: E402
    KVCache, _forward_cached, build_inference_model, quantize_decode_weights,
)
from trainingjob_operator_amd.models.moe_llama import (  # noqa: E402
    MoELlamaConfig,
)
from trainingjob_operator_amd.ops import (  # noqa: E402
    decode_linear_fp8, decode_moe_fp8, decode_moe_swiglu_fp8,
    decode_swiglu_fp8, reference,
)
from trainingjob_operator_amd.ops.fp8_weight import (  # noqa: E402
    expert_tables, quantize_rows,
)
from trainingjob_operator_amd.parallel import ep  # noqa: E402

DEV = torch.device("cuda:0")
E, M = 4, 32                        # experts; output rows (F for swiglu)
A = 4 * 3.58e-7                     # tests/test_fp8_decode_gpu.py: fp32 order
ROUTES = {"one": [2], "round_robin": [0, 1, 2, 3], "skip_1": [0, 2, 3]}


def cases(fn):
    """K = 512 is one chunk, 1024 two waves per tile (SPLIT = 2)."""
    for mark in (
            pytest.mark.parametrize("route", list(ROUTES)),
            pytest.mark.parametrize("N,xdiv",
                                    [(1, 1), (2, 2), (16, 2), (16, 1)]),
            pytest.mark.parametrize("K", [512, 1024]),
            pytest.mark.parametrize("swiglu", [False, True],
                                    ids=["plain", "swiglu"])):
        fn = mark(fn)
    return fn


@functools.lru_cache(maxsize=None)
def _experts(swiglu, K):
    """E experts' Fp8Weights on the GPU, w ~ N(0, 1/K), and their tables."""
    g = torch.Generator().manual_seed(100 * K + swiglu)
    rows = 2 * M if swiglu else M
    w8 = [quantize_rows((torch.randn(rows, K, generator=g) * K ** -0.5)
                        .bfloat16(), gate_up=swiglu).to(DEV) for _ in range(E)]
    return w8, expert_tables(w8)


@functools.lru_cache(maxsize=None)
def _case(swiglu, K, N, xdiv, route):
    """(x, idx list, idx on the GPU, tables, the kernel's y)."""
    w8, tables = _experts(swiglu, K)
    g = torch.Generator().manual_seed(7 * N + K + xdiv)
    x = torch.randn(-(-N // xdiv), K, generator=g).bfloat16().to(DEV)
    idx = [ROUTES[route][n % len(ROUTES[route])] for n in range(N)]
    idx_d = torch.tensor(idx, dtype=torch.int64, device=DEV)
    op = decode_moe_swiglu_fp8 if swiglu else decode_moe_fp8
    y = op(x, idx_d, tables, M, K, xdiv)
    assert y.shape == (N, M) and y.dtype == torch.bfloat16
    return x, idx, idx_d, tables, y


@cases
def test_grouping_changes_no_bit(swiglu, K, N, xdiv, route):
    x, idx, _, tables, y = _case(swiglu, K, N, xdiv, route)
    one = decode_swiglu_fp8 if swiglu else decode_linear_fp8
    for n, e in enumerate(idx):
        want = one(x[n // xdiv][None], tables.experts[e])
        assert torch.equal(y[n], want[0]), (n, e)


@cases
def test_accuracy_against_fp64(swiglu, K, N, xdiv, route):
    """|y - ref| <= 2**-7 |ref| + A elementwise, and for silu(g) * u the
    summation term A (1.1 |u| + |silu(g)|): test_fp8_decode_gpu.py's bounds."""
    x, idx, _, tables, y = _case(swiglu, K, N, xdiv, route)
    xr = x.double().cpu()[[n // xdiv for n in range(N)]]
    w = torch.stack([tables.experts[e].dequant().double().cpu() for e in idx])
    ref = torch.einsum("nk,nmk->nm", xr, w)
    slack = torch.full_like(ref[:, :M], A)
    if swiglu:
        g, u = ref.chunk(2, dim=-1)
        silu = g / (1 + torch.exp(-g))
        ref, slack = silu * u, A * (1.1 * u.abs() + silu.abs())
    err = (y.double().cpu() - ref).abs() - 2.0 ** -7 * ref.abs()
    print(f"gemv_moe_fp8 swiglu={swiglu} K={K} N={N} xdiv={xdiv} {route}: "
          f"max(|err| - 2^-7|ref|) = {err.max().item():.3e}, A = {A:.3e}")
    assert (err <= slack).all()


@cases
def test_unhit_experts_are_not_read(swiglu, K, N, xdiv, route):
    """NaN bytes and NaN scales in every expert no pair is routed to."""
    x, idx, idx_d, tables, y = _case(swiglu, K, N, xdiv, route)
    poisoned = [w if e in idx else dataclasses.replace(
        w, packed=torch.full_like(w.packed, 0x7f),
        scale=torch.full_like(w.scale, float("nan")))
        for e, w in enumerate(tables.experts)]
    op = decode_moe_swiglu_fp8 if swiglu else decode_moe_fp8
    got = op(x, idx_d, expert_tables(poisoned), M, K, xdiv)
    assert torch.isfinite(got.float()).all() and torch.equal(got, y)


@torch.no_grad()
@pytest.mark.parametrize("B", [1, 8])
def test_model_steps_match_twins(B, monkeypatch):
    """8 teacher-forced decode steps of a 2-layer MoE model under
    weights="fp8": the routed kernels against the same quantised model on
    their torch twins, within 2e-2 max|ref| + 2e-2 (the model-level bound of
    test_fp8_decode_gpu.py)."""
    cfg = MoELlamaConfig(
        name="moe-fp8-test", vocab_size=512, hidden_size=512,
        intermediate_size=1024, num_layers=2, num_heads=4, num_kv_heads=2,
        head_dim=128, rope_theta=10000.0, n_experts=4, top_k=2)
    torch.manual_seed(5)
    model = build_inference_model(cfg, DEV)
    assert quantize_decode_weights(model) == \
        cfg.num_layers * (2 + 2 * cfg.n_experts) + 1
    assert all(ep.expert_fp8(ex) is not None
               for blk in model.blocks for ex in blk.moe.experts)
    names = ("decode_moe_swiglu_fp8", "decode_moe_fp8")
    calls = []

    def spy(fn, route):
        def run(*a):
            y = fn(*a)
            assert y is not None
            calls.append((route, fn.__name__))
            return y
        return run

    routes = {"gpu": [spy(getattr(ep, n), "gpu") for n in names],
              "twin": [spy(getattr(reference, n), "twin") for n in names]}
    S0, steps = 5, 8
    prompt = torch.randint(0, cfg.vocab_size, (B, S0),
                           generator=torch.Generator().manual_seed(B)).to(DEV)
    caches = {r: KVCache(cfg, B, S0 + steps, DEV, torch.bfloat16)
              for r in routes}
    out = {r: [] for r in routes}
    cur = prompt
    for _ in range(steps + 1):
        for r, fns in routes.items():
            for n, fn in zip(names, fns):
                monkeypatch.setattr(ep, n, fn)
            out[r].append(_forward_cached(model, cur, caches[r], True)[:, -1])
        cur = out["gpu"][-1].argmax(dim=-1)[:, None]
    n_steps = steps + (1 if B * S0 * cfg.top_k <= 16 else 0)
    for r in routes:
        assert calls.count((r, "decode_moe_fp8")) == n_steps * cfg.num_layers
    gpu, twin = (torch.stack(out[r]).float() for r in routes)
    err = (gpu - twin).abs().max().item()
    bound = 2e-2 * twin.abs().max().item() + 2e-2
    print(f"B={B}: max |kernels - twins| logits {err:.3e}, bound {bound:.3e}")
    assert err <= bound
