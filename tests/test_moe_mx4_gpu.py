"""Routed MXFP4 decode GEMVs (hip/ops.hip gemv_moe_mx4 / gemv_moe_mx4_swiglu):
every pair against the one-row dense MXFP4 GEMV over its expert (bit for
bit), against fp64 over the dequantised experts, with the unhit experts
poisoned, and through cached decode steps of a small MoE model."""
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
    decode_linear_mx4, decode_moe_mx4, decode_moe_swiglu_mx4,
    decode_swiglu_mx4, native, reference,
)
from trainingjob_operator_amd.ops.mx4_weight import (  # noqa: E402
    mx4_expert_tables, quantize_mx4,
)
from trainingjob_operator_amd.parallel import ep  # noqa: E402

DEV = torch.device("cuda:0")
E, M = 4, 32                        # experts; output rows (F for swiglu)
# fp32 summation order. max |fp32 CPU matmul - fp64| over exactly the
# operands of the cases below (seeds included) is 1.81e-7 for the plain GEMV
# and 2.38e-7 for the gate and up sums of the SwiGLU; A is 4x the larger,
# because the kernel's MFMA chain and split order differ from the CPU's
# blocked sums.
A = 4 * 2.38e-7
ROUTES = {"one": [2], "round_robin": [0, 1, 2, 3], "skip_1": [0, 2, 3]}


def cases(fn):
    """K = 512 is one chunk, 1024 two waves per tile (SPLIT = 2, see
    test_split_rule), 1536 an odd chunk count: wave 0 owns two chunks."""
    for mark in (
            pytest.mark.parametrize("route", list(ROUTES)),
            pytest.mark.parametrize("N,xdiv",
                                    [(1, 1), (2, 2), (16, 2), (16, 1)]),
            pytest.mark.parametrize("K", [512, 1024, 1536]),
            pytest.mark.parametrize("swiglu", [False, True],
                                    ids=["plain", "swiglu"])):
        fn = mark(fn)
    return fn


@functools.lru_cache(maxsize=None)
def _experts(swiglu, K):
    """E experts' Mx4Weights on the GPU, w ~ N(0, 1/K), and their tables."""
    g = torch.Generator().manual_seed(100 * K + swiglu)
    rows = 2 * M if swiglu else M
    w4 = [quantize_mx4((torch.randn(rows, K, generator=g) * K ** -0.5)
                       .bfloat16(), gate_up=swiglu).to(DEV) for _ in range(E)]
    return w4, mx4_expert_tables(w4)


@functools.lru_cache(maxsize=None)
def _case(swiglu, K, N, xdiv, route):
    """(x, idx list, idx on the GPU, tables, the kernel's y)."""
    w4, tables = _experts(swiglu, K)
    g = torch.Generator().manual_seed(7 * N + K + xdiv)
    x = torch.randn(-(-N // xdiv), K, generator=g).bfloat16().to(DEV)
    idx = [ROUTES[route][n % len(ROUTES[route])] for n in range(N)]
    idx_d = torch.tensor(idx, dtype=torch.int64, device=DEV)
    op = decode_moe_swiglu_mx4 if swiglu else decode_moe_mx4
    y = op(x, idx_d, tables, M, K, xdiv)
    assert y.shape == (N, M) and y.dtype == torch.bfloat16
    return x, idx, idx_d, tables, y


def test_split_rule():
    split = [native.load().gemv_mx4_split(M // 16, K) for K in (512, 1024)]
    assert split[0] == 1 and split[1] > 1


@cases
def test_grouping_changes_no_bit(swiglu, K, N, xdiv, route):
    x, idx, _, tables, y = _case(swiglu, K, N, xdiv, route)
    one = decode_swiglu_mx4 if swiglu else decode_linear_mx4
    for n, e in enumerate(idx):
        want = one(x[n // xdiv][None], tables.experts[e])
        assert torch.equal(y[n], want[0]), (n, e)


@cases
def test_accuracy_against_fp64(swiglu, K, N, xdiv, route):
    """|y - ref| <= 2**-7 |ref| + A elementwise, and for silu(g) * u the
    summation term A (1.1 |u| + |silu(g)|): test_mx4_decode_gpu.py's bounds."""
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
    print(f"gemv_moe_mx4 swiglu={swiglu} K={K} N={N} xdiv={xdiv} {route}: "
          f"max(|err| - 2^-7|ref| - slack) = {(err - slack).max().item():.3e}"
          f", A = {A:.3e}")
    assert (err <= slack).all()


@cases
def test_unhit_experts_are_not_read(swiglu, K, N, xdiv, route):
    """Every expert no pair is routed to holds value bytes 0x77 (6.0, 6.0)
    and scale bytes 0xFF, which the kernel's shift turns into inf."""
    x, idx, idx_d, tables, y = _case(swiglu, K, N, xdiv, route)
    poisoned = [w if e in idx else dataclasses.replace(
        w, packed=torch.full_like(w.packed, 0x77),
        scale=torch.full_like(w.scale, 0xFF))
        for e, w in enumerate(tables.experts)]
    op = decode_moe_swiglu_mx4 if swiglu else decode_moe_mx4
    got = op(x, idx_d, mx4_expert_tables(poisoned), M, K, xdiv)
    assert torch.isfinite(got.float()).all() and torch.equal(got, y)


@torch.no_grad()
@pytest.mark.parametrize("B", [1, 8])
def test_model_steps_match_twins(B, monkeypatch):
    """8 teacher-forced decode steps of a 2-layer MoE model under
    weights="mxfp4": the routed kernels against the same quantised model on
    their torch twins, within 2e-2 max|ref| + 2e-2 (the model-level bound of
    test_moe_fp8_gpu.py)."""
    cfg = MoELlamaConfig(
        name="moe-mx4-test", vocab_size=512, hidden_size=512,
        intermediate_size=1024, num_layers=2, num_heads=4, num_kv_heads=2,
        head_dim=128, rope_theta=10000.0, n_experts=4, top_k=2)
    torch.manual_seed(5)
    model = build_inference_model(cfg, DEV)
    assert quantize_decode_weights(model, "mxfp4") == \
        cfg.num_layers * (2 + 2 * cfg.n_experts) + 1
    assert all(ep.expert_mx4(ex) is not None
               for blk in model.blocks for ex in blk.moe.experts)
    names = ("decode_moe_swiglu_mx4", "decode_moe_mx4")
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
        for n in names:
            assert calls.count((r, n)) == n_steps * cfg.num_layers
    gpu, twin = (torch.stack(out[r]).float() for r in routes)
    err = (gpu - twin).abs().max().item()
    bound = 2e-2 * twin.abs().max().item() + 2e-2
    print(f"B={B}: max |kernels - twins| logits {err:.3e}, bound {bound:.3e}")
    assert err <= bound
