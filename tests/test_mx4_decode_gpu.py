"""Weight-only MXFP4 decode GEMVs (hip/ops.hip gemv_mx4 / gemv_mx4_swiglu)
against the dequantised weight: exact on one-hot rows, bounded on random
ones, and through the captured and the paged decode step of llama-smoke."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.models.config import CONFIGS  # noqa: E402
from trainingjob_operator_amd.models.decode_graph import (  # noqa: E402
    DecodeSession,
)
from trainingjob_operator_amd.models.generate import (  # noqa: E402
    KVCache, _forward_cached, build_inference_model, quantize_decode_weights,
)
from trainingjob_operator_amd.models.paged import (  # noqa: E402
    PagedKVCache, _step_paged,
)
from trainingjob_operator_amd.ops import (  # noqa: E402
    decode_linear_mx4, decode_swiglu_mx4,
)
from trainingjob_operator_amd.ops.mx4_weight import quantize_mx4  # noqa: E402

DEV = torch.device("cuda:0")
# one and several tiles, one and several chunks, an odd chunk count, every
# split the rule picks (1, 2, 4 and, for one tile of 8 chunks, 8)
SHAPES = [(16, 512), (48, 1536), (32, 2048), (16, 4096)]
SWIGLU = [(16, 512), (48, 1536), (16, 4096)]       # (F, K)
ROWS = [1, 8, 9, 16]
# fp32 summation order. max |fp32 CPU matmul - fp64| over the accuracy cases
# below (these operands, seeds included) is 3.19e-7 for the GEMV and 2.38e-7
# for the gate and up sums of the SwiGLU; A is 4x the larger, because the
# kernel's MFMA chain and split order differ from the CPU's blocked sums.
A = 4 * 3.19e-7


@functools.lru_cache(maxsize=None)
def _weight(M, K, gate_up=False, spread=False):
    """(Mx4Weight on the GPU, its dequantised [M, K] fp32 values on the CPU),
    w ~ N(0, 1/K); spread: magnitudes over 5 decades along the rows and 4
    along the k blocks, so that neighbouring blocks have different scales."""
    g = torch.Generator().manual_seed(1000 * M + K)
    w = torch.randn(M, K, generator=g) * K ** -0.5
    if spread:
        w = w * torch.logspace(-3, 2, M)[:, None] * torch.logspace(
            -2, 2, K // 32)[torch.randperm(K // 32, generator=g)
                            ].repeat_interleave(32)
    w4 = quantize_mx4(w.bfloat16(), gate_up=gate_up)
    return w4.to(DEV), w4.dequant()


def _x(N, K):
    g = torch.Generator().manual_seed(7 * N + K)
    return torch.randn(N, K, generator=g).bfloat16()


def _one_hot_batches(K, N):
    """All 128 positions of the first k-block (nibble, byte, word and lane
    order), and every MX block edge - and so every chunk edge - with its
    neighbours, up to K - 1."""
    cols = set(range(128)) | {K - 1}
    for edge in range(32, K, 32):
        cols |= {edge - 1, edge, edge + 1}
    cols = sorted(cols)
    for i in range(0, len(cols), N):
        c = (cols[i:i + N] * N)[:N]                 # always N rows
        x = torch.zeros(N, K)
        x[torch.arange(N), torch.tensor(c)] = 1.0
        yield c, x.bfloat16().to(DEV)


def _silu_mul(g, u):
    return g / (1 + torch.exp(-g)) * u


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("M,K", SHAPES)
def test_one_hot_rows_read_the_weight_exactly(M, K, N):
    w4, deq = _weight(M, K, spread=True)
    assert w4.scale.unique().numel() >= 16          # 9 decades: ~30 binades
    for c, x in _one_hot_batches(K, N):
        y = decode_linear_mx4(x, w4)
        assert y.shape == (N, M) and y.dtype == torch.bfloat16
        assert torch.equal(y.float().cpu(), deq[:, c].t()), c


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("F,K", SWIGLU)
def test_swiglu_one_hot_rows_exact(F, K, N):
    gu4, deq = _weight(2 * F, K, True, spread=True)
    for c, x in _one_hot_batches(K, N):
        y = decode_swiglu_mx4(x, gu4)
        want = _silu_mul(deq[:F, c].t(), deq[F:, c].t()).bfloat16()
        assert torch.equal(y.cpu(), want), c


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("M,K", SHAPES + [(16, 14336)])
def test_accuracy_against_fp64(M, K, N):
    """|y - ref| <= 2**-7 |ref| + A elementwise: twice bf16's worst rounding
    of the output, plus the summation order."""
    w4, deq = _weight(M, K)
    x = _x(N, K)
    ref = x.double() @ deq.double().t()
    y = decode_linear_mx4(x.to(DEV), w4).double().cpu()
    excess = ((y - ref).abs() - 2.0 ** -7 * ref.abs()).max().item()
    print(f"gemv_mx4 {M}x{K} N={N}: max(|err| - 2^-7|ref|) = {excess:.3e}, "
          f"A = {A:.3e}")
    assert excess <= A


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("F,K", SWIGLU)
def test_swiglu_accuracy_against_fp64(F, K, N):
    """The same bound on silu(g) * u. An error A in g moves the product by
    at most 1.1 |u| A (silu' <= 1.1) and one in u by |silu(g)| A, so the
    summation term is A (1.1 |u| + |silu(g)|)."""
    gu4, deq = _weight(2 * F, K, True)
    x = _x(N, K)
    g, u = (x.double() @ deq.double().t()).chunk(2, dim=-1)
    ref = _silu_mul(g, u)
    y = decode_swiglu_mx4(x.to(DEV), gu4).double().cpu()
    slack = A * (1.1 * u.abs() + _silu_mul(g, torch.ones_like(g)).abs())
    excess = ((y - ref).abs() - 2.0 ** -7 * ref.abs() - slack).max().item()
    print(f"gemv_mx4_swiglu {F}x{K} N={N}: excess = {excess:.3e}")
    assert excess <= 0


def test_same_bits_every_call_and_17_rows_refused():
    w4, _ = _weight(48, 1536)
    x = _x(16, 1536).to(DEV)
    assert torch.equal(decode_linear_mx4(x, w4), decode_linear_mx4(x, w4))
    assert decode_linear_mx4(torch.zeros(17, 1536, dtype=torch.bfloat16,
                                         device=DEV), w4) is None


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(5)
    m = build_inference_model(CONFIGS["llama-smoke"], DEV)
    assert quantize_decode_weights(m, "mxfp4") == 4 * m.cfg.num_layers + 1
    return m


def _close(got, ref, what):
    """The bound tests/test_paged_engine_gpu.py puts on two routes of one
    model."""
    err = (got.float() - ref.float()).abs().max().item()
    bound = 2e-2 * ref.float().abs().max().item() + 2e-2
    print(f"{what}: max |mxfp4 - bf16| logits {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@torch.no_grad()
def test_captured_session_step_matches_bf16_route(model):
    prompt = torch.randint(0, model.cfg.vocab_size, (1, 24),
                           generator=torch.Generator().manual_seed(3)).to(DEV)
    logits = {}
    for weights in ("mxfp4", "bf16"):
        ses = DecodeSession(model, 1, 32, weights=weights)
        ses.generate(prompt, 1)                     # prefill + one replay
        logits[weights] = ses.dec.logits.clone()
    _close(logits["mxfp4"], logits["bf16"], "captured step")


@torch.no_grad()
def test_paged_step_8_slots_matches_bf16_route(model):
    cfg = model.cfg
    B, S0 = 8, 20
    prompt = torch.randint(0, cfg.vocab_size, (B, S0),
                           generator=torch.Generator().manual_seed(4)).to(DEV)
    cont = KVCache(cfg, B, S0 + 2, DEV, torch.bfloat16)
    cur = _forward_cached(model, prompt, cont)[:, -1].argmax(dim=-1)
    paged = PagedKVCache(cfg, n_pages=B, max_slots=B, max_pages_per_seq=1,
                         device=DEV, dtype=torch.bfloat16)
    for b in range(B):
        assert paged.admit(b, S0 + 1)
        paged.load_prefix(b, [k[b] for k in cont.k], [v[b] for v in cont.v],
                          S0)
    logits = {}
    for weights in ("mxfp4", "bf16"):
        paged.sync_pos([S0] * B)                    # the same row both times
        logits[weights] = _step_paged(model, cur[:, None], paged,
                                      weights == "mxfp4")
    _close(logits["mxfp4"], logits["bf16"], "paged step, 8 slots")
