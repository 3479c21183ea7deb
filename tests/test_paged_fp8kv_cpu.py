"""The fp8 KV cache format (ops/reference.py twin) on the CPU: rounding
bound, the V image's row permutation, the cache's page-in path and the
engine's refusals."""
import math

import pytest
import torch

from trainingjob_operator_amd.models.config import LlamaConfig
from trainingjob_operator_amd.models.paged import PagedEngine, PagedKVCache
from trainingjob_operator_amd.ops import reference
from trainingjob_operator_amd.training import build_model

CPU = torch.device("cpu")
CFG = LlamaConfig(name="tiny-d128", vocab_size=256, hidden_size=256,
                  intermediate_size=512, num_layers=2, num_heads=4,
                  num_kv_heads=2, head_dim=128, max_seq_len=256)
F8 = torch.float8_e4m3fn


def _rows(n, seed, dtype=torch.float32):
    """[n, 128] rows spanning decades; row 1 is zero, row 2 one nonzero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 128, generator=g) * torch.exp2(
        torch.randint(-20, 1, (n, 128), generator=g).float())
    x = x * torch.exp2(torch.randint(-8, 9, (n, 1), generator=g).float())
    x[1:3] = 0
    x[2, 77] = -3.3e-4
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_round_trip_bound(dtype):
    k, v = _rows(40, 1, dtype), _rows(40, 2, dtype)
    k8, v8, sc = reference.kv_fp8_quant_rows(k, v)
    assert torch.equal(sc[1], torch.ones(2))                  # amax == 0
    assert torch.equal(torch.exp2(torch.log2(sc).round()), sc)  # powers of 2
    for x, x8, s in ((k, k8, sc[:, 0]), (v, v8, sc[:, 1])):
        xf = x.float()
        amax = xf.abs().amax(dim=1)
        nz = amax > 0                 # the smallest power of two that fits
        assert (amax <= 448 * s).all() and (amax[nz] > 224 * s[nz]).all()
        deq = x8.view(F8).float() * s[:, None]
        err = (deq - xf).abs()
        assert (err <= 2.0 ** -4 * xf.abs() + 2.0 ** -10 * s[:, None]).all()


def test_v_image_rows_equal_page_at_once():
    """64 rows written one at a time (kv_fp8_v_offsets) leave the bytes the
    whole-page permutation leaves, and kv_fp8_dequant undoes both."""
    n_kv = 2
    k = _rows(3 * n_kv * 64, 3).reshape(3, n_kv, 64, 128)
    v = _rows(3 * n_kv * 64, 4).reshape(3, n_kv, 64, 128)
    k8p, v8p, scp = reference.kv_fp8_quant_pages(k, v)
    pools = (torch.zeros(3, n_kv, 64, 128, dtype=torch.uint8),
             torch.zeros(3, n_kv, 64, 128, dtype=torch.uint8),
             torch.zeros(3, n_kv, 2, 64))
    for page in (2, 0, 1):
        for row in torch.randperm(64, generator=torch.Generator()
                                  .manual_seed(page)).tolist():
            k8, v8, sc = reference.kv_fp8_quant_rows(k[page, :, row],
                                                     v[page, :, row])
            reference.kv_fp8_write_rows(
                *pools, torch.tensor([page]), torch.tensor([row]),
                k8[None], v8[None], sc[None])
    assert all(torch.equal(a, b) for a, b in zip(pools, (k8p, v8p, scp)))
    kd, vd = reference.kv_fp8_dequant(*pools, torch.float32)
    k8, v8, sc = reference.kv_fp8_quant_rows(k, v)
    assert torch.equal(kd, k8.view(F8).float() * sc[..., 0:1])
    assert torch.equal(vd, v8.view(F8).float() * sc[..., 1:2])


def test_cache_load_prefix_and_decode_twin():
    """An fp8 cache paged in from a contiguous prefix attends exactly like a
    plain cache paged in from the row-wise dequantised prefix (fp32)."""
    length, n_kv = 150, CFG.num_kv_heads
    ks, vs = ([_rows(n_kv * 160, s + li).reshape(n_kv, 160, 128)
               for li in range(CFG.num_layers)] for s in (10, 20))
    caches = []
    for kv_dtype in ("fp8", "bf16"):
        c = PagedKVCache(CFG, 8, 2, 3, CPU, torch.float32, kv_dtype=kv_dtype)
        c.free_pages = [3, 6, 0, 5, 1, 7, 2, 4]
        assert c.admit(1, length + 1)
        caches.append(c)
    f8, plain = caches
    f8.load_prefix(1, ks, vs, length)
    deq = []
    for k, v in zip(ks, vs):
        k8, v8, sc = reference.kv_fp8_quant_rows(k, v)
        deq.append((k8.view(F8).float() * sc[..., 0:1],
                    v8.view(F8).float() * sc[..., 1:2]))
    plain.load_prefix(1, [d[0] for d in deq], [d[1] for d in deq], length)
    f8.check_block_table()
    assert f8.kv_scale[0].shape == (8, n_kv, 2, 64)
    q = torch.randn(2, CFG.num_heads, 1, 128,
                    generator=torch.Generator().manual_seed(9))
    pos = torch.tensor([-1, length - 1])
    for li in range(CFG.num_layers):
        got = reference.decode_attention_paged_fp8(
            q, f8.k[li], f8.v[li], f8.kv_scale[li], f8.block_table, pos,
            1 / math.sqrt(128))
        ref = reference.decode_attention_paged(
            q, plain.k[li], plain.v[li], plain.block_table, pos,
            1 / math.sqrt(128))
        assert torch.equal(got, ref) and ref[1].abs().max() > 0


@pytest.mark.parametrize("kw", [{"prefill": "paged"}, {"lookup_k": 2}])
def test_engine_refuses_unported_routes(kw):
    torch.manual_seed(0)
    model = build_model(CFG, CPU).float().eval()
    with pytest.raises(ValueError, match="follow-up"):
        PagedEngine(model, max_slots=2, kv="fp8", **kw)
    eng = PagedEngine(model, max_slots=2, n_pages=4, kv="fp8")
    assert eng.cache.kv_dtype == "fp8"
    eng.submit(list(range(1, 62)), 6)            # crosses the page boundary
    (out,) = eng.run().values()
    assert out.numel() == 61 + 6
    eng.cache.check_block_table()
