"""MXFP4 skinny GEMM for 17..64 rows (hip/ops.hip gemm_mx4_rows /
gemm_mx4_rows_swiglu) against the dequantised weight: exact on one-hot rows
at every staged position and stage edge, bounded against fp64 on random ones,
nothing written outside [N, M], a fixed order, and the routes that take it."""
import ctypes
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.models.config import CONFIGS  # noqa: E402
from trainingjob_operator_amd.models.generate import (  # noqa: E402
    KVCache, _forward_cached, _mlp_cached, _proj, build_inference_model,
    quantize_decode_weights,
)
from trainingjob_operator_amd.models.paged import (  # noqa: E402
    PagedKVCache, _verify_paged,
)
from trainingjob_operator_amd.ops import (  # noqa: E402
    linear_mx4_rows, mx4_rows_pays, native, swiglu_mx4_rows,
)
from trainingjob_operator_amd.ops.mx4_weight import quantize_mx4  # noqa: E402

DEV = torch.device("cuda:0")
ROWS = [17, 32, 33, 64]
# 4 tiles and 3 (no T > 1 divides them); one step, an odd number of chunks
# (stage parity), many steps. The shape rule gives these few tiles S = 4 at
# every K, its largest; the other S run through the forced entry.
SHAPES = [(64, 512), (48, 1536), (64, 4096)]
# the public op, then every (T, S) the forced entry takes; T = 1 shares nothing
ROUTES = [None, (1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4), (4, 1), (4, 2)]
# fp32 summation order. max |fp32 CPU matmul - fp64| over the accuracy cases
# below (these operands, seeds included), measured on the CPU, is 4.06e-7
# plain and 5.03e-7 for the gate and up sums; 4 x the larger exceeds the
# 1.28e-6 of tests/test_mx4_decode_gpu.py (more rows, more draws), so A is
# the measured value: the kernel's MFMA chain and slice order differ from
# the CPU's blocked sums.
A = 4 * 5.03e-7


@functools.lru_cache(maxsize=None)
def _case(M, K, gate_up, spread):
    """(Mx4Weight of [M or 2M, K] on the GPU, its dequantised fp32 values on
    the CPU), w ~ N(0, 1/K); spread: magnitudes over 5 decades along the rows
    and 4 along the k blocks, so that many distinct scale bytes occur."""
    g = torch.Generator().manual_seed(1000 * M + K + gate_up)
    rows = 2 * M if gate_up else M
    w = torch.randn(rows, K, generator=g) * K ** -0.5
    if spread:
        w = w * torch.logspace(-3, 2, rows)[:, None] * torch.logspace(
            -2, 2, K // 32)[torch.randperm(K // 32, generator=g)
                            ].repeat_interleave(32)
    w4 = quantize_mx4(w.bfloat16(), gate_up=gate_up)
    return w4.to(DEV), w4.dequant()


def _x(N, K):
    g = torch.Generator().manual_seed(7 * N + K)
    return torch.randn(N, K, generator=g).bfloat16()


def _run(x, w4, route):
    """The public op, or (T, S) forced into the middle of a sentinel-filled
    [N + 2, M] buffer whose guard rows must come back untouched."""
    if route is None:
        return (swiglu_mx4_rows if w4.gate_up else linear_mx4_rows)(x, w4)
    N, cols = x.shape[0], w4.M // 2 if w4.gate_up else w4.M
    buf = torch.full((N + 2, cols), -7.0, dtype=torch.bfloat16, device=DEV)
    rc = native.load().gemm_mx4_rows_ab(
        native.stream_ptr(), int(w4.gate_up), *route,
        *(ctypes.c_void_p(t.data_ptr()) for t in (w4.packed, w4.scale, x,
                                                  buf[1:])), cols, w4.K, N)
    assert rc == 0
    assert bool((buf[0] == -7).all()) and bool((buf[N + 1] == -7).all())
    return buf[1:N + 1]


def _silu_mul(g, u):
    return g / (1 + torch.exp(-g)) * u


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("M,K", SHAPES)
def test_one_hot_rows_read_the_weight_exactly(M, K, N, route):
    """Every k of the widest first step (512), every 128-wide k-block edge -
    and so every stage edge of every S - with its neighbours, and K - 1."""
    cols = set(range(min(K, 512))) | {K - 1}
    for edge in range(128, K, 128):
        cols |= {edge - 1, edge, edge + 1}
    cols = sorted(cols)
    w4, deq = _case(M, K, False, True)
    gu4, gdeq = _case(M, K, True, True)
    assert w4.scale.unique().numel() >= 16
    for i in range(0, len(cols), N):
        c = (cols[i:i + N] * N)[:N]                 # always N rows
        x = torch.zeros(N, K)
        x[torch.arange(N), torch.tensor(c)] = 1.0
        x = x.bfloat16().to(DEV)
        y = _run(x, w4, route)
        assert y.shape == (N, M) and y.dtype == torch.bfloat16
        assert torch.equal(y.float().cpu(), deq[:, c].t()), c
        want = _silu_mul(gdeq[:M, c].t(), gdeq[M:, c].t()).bfloat16()
        assert torch.equal(_run(x, gu4, route).cpu(), want), c


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("M,K", SHAPES)
def test_accuracy_against_fp64(M, K, N):
    """|y - ref| <= 2**-7 |ref| + A elementwise; for silu(g) * u the
    summation term is A (1.1 |u| + |silu(g)|), as in test_mx4_decode_gpu."""
    w4, deq = _case(M, K, False, False)
    gu4, gdeq = _case(M, K, True, False)
    x = _x(N, K)
    ref = x.double() @ deq.double().t()
    y = linear_mx4_rows(x.to(DEV), w4).double().cpu()
    excess = ((y - ref).abs() - 2.0 ** -7 * ref.abs()).max().item()
    print(f"gemm_mx4_rows {M}x{K} N={N}: max(|err| - 2^-7|ref|) = "
          f"{excess:.3e}, A = {A:.3e}")
    assert excess <= A
    g, u = (x.double() @ gdeq.double().t()).chunk(2, dim=-1)
    ref = _silu_mul(g, u)
    y = swiglu_mx4_rows(x.to(DEV), gu4).double().cpu()
    slack = A * (1.1 * u.abs() + _silu_mul(g, torch.ones_like(g)).abs())
    excess = ((y - ref).abs() - 2.0 ** -7 * ref.abs() - slack).max().item()
    print(f"gemm_mx4_rows_swiglu {M}x{K} N={N}: excess = {excess:.3e}")
    assert excess <= 0


@pytest.mark.parametrize("gate_up", [False, True])
def test_order_is_fixed_and_rows_do_not_depend_on_n(gate_up):
    w4, _ = _case(48, 1536, gate_up, False)
    x = _x(64, 1536).to(DEV)
    y = _run(x, w4, None)
    assert torch.equal(y, _run(x, w4, None))
    for j in (0, 16, 37, 63):
        x17 = torch.cat([x[j:j + 1], x[:16]])
        assert torch.equal(_run(x17, w4, None)[0], y[j]), j


def test_refusals():
    w4, _ = _case(64, 512, False, False)
    gu4, _ = _case(64, 512, True, False)
    for n in (16, 65):
        xn = torch.zeros(n, 512, dtype=torch.bfloat16, device=DEV)
        assert linear_mx4_rows(xn, w4) is None
        assert swiglu_mx4_rows(xn, gu4) is None
    x = _x(17, 512).to(DEV)
    assert linear_mx4_rows(x, gu4) is None and swiglu_mx4_rows(x, w4) is None
    p = [ctypes.c_void_p(t.data_ptr()) for t in (w4.packed, w4.scale, x, x)]
    ab = native.load().gemm_mx4_rows_ab
    assert ab(native.stream_ptr(), 0, 4, 4, *p, 64, 512, 17) != 0
    assert ab(native.stream_ptr(), 0, 3, 1, *p, 64, 512, 17) != 0
    assert ab(native.stream_ptr(), 0, 1, 1, *p, 64, 512, 16) != 0
    assert ab(native.stream_ptr(), 0, 1, 1, *p, 72, 512, 17) != 0
    assert ab(native.stream_ptr(), 0, 1, 1, *p, 64, 768, 17) != 0


@torch.no_grad()
def test_proj_and_mlp_take_the_rows_route():
    torch.manual_seed(2)

    def lin(k, m):
        return torch.nn.Linear(k, m, bias=False, device=DEV,
                               dtype=torch.bfloat16)
    head, mlp = lin(512, 1024), types.SimpleNamespace(
        gate_up_proj=lin(512, 1024), down_proj=lin(512, 512))
    model = types.SimpleNamespace(
        blocks=[types.SimpleNamespace(
            attn=types.SimpleNamespace(qkv_proj=head, o_proj=head), mlp=mlp)],
        lm_head=head, embed=types.SimpleNamespace(weight=None))
    assert quantize_decode_weights(model, "mxfp4") == 5
    x = torch.randn(40, 512, device=DEV).bfloat16()
    assert mx4_rows_pays(x, head.mx4_weight)
    assert mx4_rows_pays(x, mlp.gate_up_proj.mx4_weight)
    assert torch.equal(_proj(head, x, fp8=True),
                       linear_mx4_rows(x, head.mx4_weight))
    h = swiglu_mx4_rows(x, mlp.gate_up_proj.mx4_weight)
    assert torch.equal(_mlp_cached(mlp, x, fp8=True),
                       _proj(mlp.down_proj, h, fp8=True))


@torch.no_grad()
def test_verify_step_40_rows_matches_bf16_route():
    """llama-smoke, 8 slots x (lookup_k 4 + 1) tokens: one verify forward
    over the MXFP4 weights against the same step over the written-back bf16
    weights, the bound of tests/test_mx4_decode_gpu.py on the logits."""
    torch.manual_seed(5)
    cfg = CONFIGS["llama-smoke"]
    model = build_inference_model(cfg, DEV)
    assert quantize_decode_weights(model, "mxfp4") == 4 * cfg.num_layers + 1
    B, S0, T = 8, 20, 5
    gen = torch.Generator().manual_seed(4)
    prompt = torch.randint(0, cfg.vocab_size, (B, S0), generator=gen).to(DEV)
    cont = KVCache(cfg, B, S0, DEV, torch.bfloat16)
    _forward_cached(model, prompt, cont)
    paged = PagedKVCache(cfg, n_pages=B, max_slots=B, max_pages_per_seq=1,
                         device=DEV, dtype=torch.bfloat16)
    for b in range(B):
        assert paged.admit(b, S0 + T)
        paged.load_prefix(b, [k[b] for k in cont.k], [v[b] for v in cont.v],
                          S0)
        paged.ensure_row(b, S0 + T - 1)
    toks = torch.randint(0, cfg.vocab_size, (B, T), generator=gen).to(DEV)
    n_q = torch.full((B,), T, dtype=torch.int32, device=DEV)
    got = _verify_paged(model, toks, paged, n_q, True).float()
    ref = _verify_paged(model, toks, paged, n_q, False).float()
    err = (got - ref).abs().max().item()
    bound = 2e-2 * ref.abs().max().item() + 2e-2
    print(f"verify step, 40 rows: max |mxfp4 - bf16| logits {err:.3e}, "
          f"bound {bound:.3e}")
    assert err <= bound
