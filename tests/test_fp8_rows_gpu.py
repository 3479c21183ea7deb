"""fp8 skinny GEMM for 17..64 rows (hip/ops.hip gemm_fp8_rows /
gemm_fp8_rows_swiglu): every output row is the bits of the one-row fp8 GEMV,
nothing outside [N, M] is written, and _proj takes the route."""
import ctypes
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.models.generate import (  # noqa: E402
    _proj, quantize_decode_weights,
)
from trainingjob_operator_amd.ops import (  # noqa: E402
    decode_linear_fp8, decode_swiglu_fp8, linear_fp8_rows, native,
    swiglu_fp8_rows,
)
from trainingjob_operator_amd.ops.fp8_weight import quantize_rows  # noqa: E402

DEV = torch.device("cuda:0")
ROWS = [17, 32, 33, 64]
M = 64                  # 4 row tiles: 1, 2 and 4 of them per wave all divide
A = 4 * 3.58e-7         # tests/test_fp8_decode_gpu.py: fp32 summation order
SPLITS = [1, 2, 4, 8]   # every value the split rule returns


def _k_for(split):
    """The smallest K at which M's tiles get this split."""
    lib = native.load()
    return next(K for K in range(512, 4096 + 1, 512)
                if lib.gemv_fp8_split(M // 16, K) == split)


@functools.lru_cache(maxsize=None)
def _case(K, N, gate_up, spread=True):
    """(x [N, K] bf16, Fp8Weight of [M or 2M, K]) on the GPU and the stacked
    one-row results of the decode op; spread: a power of two in 2^-12..2^7 per
    weight row, so that every row has a scale of its own."""
    g = torch.Generator().manual_seed(100 * K + N + gate_up)
    rows = 2 * M if gate_up else M
    w = torch.randn(rows, K, generator=g) * K ** -0.5
    if spread:
        w = w * torch.exp2(torch.randint(-12, 8, (rows, 1), generator=g))
    w8 = quantize_rows(w.bfloat16(), gate_up=gate_up).to(DEV)
    x = torch.randn(N, K, generator=g).bfloat16().to(DEV)
    one = decode_swiglu_fp8 if gate_up else decode_linear_fp8
    return x, w8, torch.cat([one(x[n:n + 1], w8) for n in range(N)])


def _rows(x, w8, r):
    """The public op (r = 0, which allocates exactly [N, M]), or r row tiles
    per wave forced through the benchmark entry, into the middle of a
    sentinel-filled buffer whose other rows must come back untouched."""
    N = x.shape[0]
    if r == 0:
        op = swiglu_fp8_rows if w8.gate_up else linear_fp8_rows
        return op(x, w8)
    cols = w8.M // 2 if w8.gate_up else w8.M
    buf = torch.full((N + 2, cols), -7.0, dtype=torch.bfloat16, device=DEV)
    rc = native.load().gemm_fp8_rows_ab(
        native.stream_ptr(), int(w8.gate_up), r,
        *(ctypes.c_void_p(t.data_ptr()) for t in (w8.packed, w8.scale, x,
                                                  buf[1:])), cols, w8.K, N)
    assert rc == 0
    assert bool((buf[0] == -7).all()) and bool((buf[N + 1] == -7).all())
    return buf[1:N + 1]


@pytest.mark.parametrize("r", [0, 1, 2, 4])
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("split", SPLITS)
def test_rows_bit_equal_one_row_gemv(split, N, r):
    K = _k_for(split)
    x, w8, want = _case(K, N, False)
    y = _rows(x, w8, r)
    assert y.shape == (N, M) and y.dtype == torch.bfloat16
    for n in range(N):
        assert torch.equal(y[n], want[n]), n


@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("split", SPLITS)
def test_swiglu_rows_bit_equal_one_row_gemv(split, N, r):
    K = _k_for(split)
    x, gu8, want = _case(K, N, True)
    y = _rows(x, gu8, r)
    assert y.shape == (N, M) and y.dtype == torch.bfloat16
    for n in range(N):
        assert torch.equal(y[n], want[n]), n


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("split", SPLITS)
def test_rows_match_fp64(split, N):
    """|y - ref| <= 2**-7 |ref| + A elementwise, the bound and the operands
    (w ~ N(0, 1/K), unit-normal x) of test_fp8_decode_gpu's
    test_accuracy_against_fp64."""
    K = _k_for(split)
    x, w8, _ = _case(K, N, False, spread=False)
    ref = x.double().cpu() @ w8.dequant().double().cpu().t()
    y = linear_fp8_rows(x, w8).double().cpu()
    excess = ((y - ref).abs() - 2.0 ** -7 * ref.abs()).max().item()
    print(f"gemm_fp8_rows {M}x{K} N={N}: max(|err| - 2^-7|ref|) = "
          f"{excess:.3e}, A = {A:.3e}")
    assert excess <= A


def test_refusals():
    x, w8, _ = _case(512, 17, False)
    x, gu8, _ = _case(512, 17, True)
    for n in (16, 65):
        xn = torch.zeros(n, 512, dtype=torch.bfloat16, device=DEV)
        assert linear_fp8_rows(xn, w8) is None
        assert swiglu_fp8_rows(xn, gu8) is None
    assert linear_fp8_rows(x, gu8) is None and swiglu_fp8_rows(x, w8) is None


@torch.no_grad()
def test_proj_takes_rows_route():
    torch.manual_seed(2)
    lin = torch.nn.Linear(512, 1024, bias=False, device=DEV,
                          dtype=torch.bfloat16)
    model = types.SimpleNamespace(
        blocks=[], lm_head=lin, embed=types.SimpleNamespace(weight=None))
    assert quantize_decode_weights(model) == 1
    x = torch.randn(40, 512, device=DEV).bfloat16()
    y = _proj(lin, x, fp8=True)
    assert torch.equal(y, linear_fp8_rows(x, lin.fp8_weight))
    for i in range(40):
        assert torch.equal(y[i], _proj(lin, x[i:i + 1], fp8=True)[0]), i
