"""fp8 KV cache kernels (rope_cache_paged_fp8, attn_decode_paged_fp8, head_dim
128): the write byte for byte against the twin, exact row selection, fp64
softmax attention over the dequantised rows, the garbage contract, and the
decode step on llama-smoke against the twins and against the bf16 cache."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.models import paged  # noqa: E402
from trainingjob_operator_amd.models.config import CONFIGS  # noqa: E402
from trainingjob_operator_amd.models.generate import (  # noqa: E402
    KVCache, _forward_cached, build_inference_model,
)
from trainingjob_operator_amd.ops import (  # noqa: E402
    decode_attention_paged_fp8, native, reference, rope_cache_paged,
    rope_cache_paged_fp8,
)

DEV = torch.device("cuda:0")
D, R = 128, 64
SCALE = 1.0 / math.sqrt(D)
# |fp8-KV logits - exact-KV logits| and max |logits| of the same 10 steps on
# the fp32 CPU twin of llama-smoke: the format's own error (profiles/r18)
TWIN_FORMAT_ERR, TWIN_MAX_LOGIT = 0.277, 4.57


@pytest.mark.parametrize("nh,nkv", [(8, 2), (8, 8), (8, 1)])
def test_write_matches_twin_bytes(nh, nkv):
    """q is rope_cache_paged's q; K bytes, V image bytes and scales are the
    twin's quantisation of the rows the bf16 kernel writes (same rope, so the
    quantisation alone is compared); every other pool byte keeps its value."""
    native.load(require=True)
    g = torch.Generator().manual_seed(nkv)
    pos_l = [0, 63, -1, 64, 200]
    B, max_pages, n_pages = len(pos_l), 4, 24
    qkv = torch.randn(B, nh + 2 * nkv, D, generator=g) * torch.exp2(
        torch.randint(-12, 8, (B, nh + 2 * nkv, 1), generator=g).float())
    qkv[3, nh + nkv] = 0                         # one all-zero v row
    qkv = qkv.to(torch.bfloat16).to(DEV).reshape(B, -1)
    inv_freq = (1.0 / (5e5 ** (torch.arange(64).float() / 64))).to(DEV)
    table = torch.randperm(n_pages, generator=g)[:B * max_pages].reshape(
        B, max_pages).int().to(DEV)
    pos = torch.tensor(pos_l, device=DEV)
    kb = torch.zeros(n_pages, nkv, R, D, dtype=torch.bfloat16, device=DEV)
    vb = torch.zeros_like(kb)
    q_ref = rope_cache_paged(qkv, kb, vb, inv_freq, table, pos, nh, nkv)
    start = tuple(torch.randint(0, 0x7f, (n_pages, nkv, R, D), generator=g)
                  .to(torch.uint8).to(DEV) for _ in range(2)) + (
        torch.rand(n_pages, nkv, 2, R, generator=g).to(DEV),)
    got = tuple(t.clone() for t in start)
    q = rope_cache_paged_fp8(qkv, *got, inv_freq, table, pos, nh, nkv)
    assert torch.equal(q, q_ref) and not q[2].any()
    want = tuple(t.clone() for t in start)
    act = [b for b in range(B) if pos_l[b] >= 0]
    page = torch.stack([table[b, pos_l[b] // R] for b in act]).long()
    row = torch.tensor([pos_l[b] % R for b in act], device=DEV)
    reference.kv_fp8_write_rows(
        *want, page, row,
        *reference.kv_fp8_quant_rows(kb[page, :, row], vb[page, :, row]))
    for name, a, b in zip(("k8", "v8 image", "scales"), got, want):
        assert torch.equal(a, b), name


def test_selects_one_row_exactly():
    """Slot b's K makes row j_b outscore every other row by > 200: the output
    must be the dequantised V row j_b, bit for bit, for all q heads; j = every
    row of the second page and row 0 of the first."""
    native.load(require=True)
    H, n_kv = 8, 2
    targets = [0] + list(range(64, 128))
    B = len(targets)
    g = torch.Generator().manual_seed(7)
    mag = torch.exp2(-(torch.arange(128) % 12).float())[:, None]  # <= 1
    k = (torch.rand(B, n_kv, 128, D, generator=g) - 0.5) * mag
    v = torch.randn(B, n_kv, 128, D, generator=g) * torch.exp2(
        (torch.arange(128) % 10).float() - 6)[:, None]
    for b, j in enumerate(targets):
        k[b, :, j] = 32.0 * 2 ** (j % 3)
    # q head h = f_h * ones: score_j >= 11.3 * 32 f_h, any other <= 5.7 f_h
    q = (torch.ones(B, H, 1, D) * (1 + torch.arange(H) % 3 * 0.5)
         [None, :, None, None]).to(torch.bfloat16).to(DEV)
    k8, v8, sc = reference.kv_fp8_quant_pages(
        *(t.reshape(B, n_kv, 2, R, D).transpose(1, 2).reshape(
            B * 2, n_kv, R, D).to(DEV) for t in (k, v)))
    table = torch.randperm(2 * B + 6, generator=g)[:2 * B].reshape(B, 2)
    pools = tuple(t.new_zeros(2 * B + 6, *t.shape[1:]) for t in (k8, v8, sc))
    for pool, src in zip(pools, (k8, v8, sc)):
        pool[table.reshape(-1).to(DEV)] = src
    pos = torch.full((B,), 127, device=DEV)
    out = decode_attention_paged_fp8(q, *pools, table.int().to(DEV), pos,
                                     SCALE)
    _, vd = reference.kv_fp8_dequant(k8, v8, sc)        # [2B, n_kv, 64, D]
    for b, j in enumerate(targets):
        want = vd[2 * b + j // R, :, j % R]             # [n_kv, D]
        want = want[:, None].expand(n_kv, H // n_kv, D).reshape(H, D)
        assert torch.equal(out[b, :, 0], want), f"row {j}"


POS = [0, 15, 16, 63, -1, 64, 200]     # MFMA row-tile and page boundaries
MAX_PAGES, N_PAGES = 4, 32


@functools.lru_cache(maxsize=None)
def _case(H, n_kv):
    """Unit-normal inputs in permuted pages, kernel output, fp64 reference."""
    native.load(require=True)
    B = len(POS)
    g = torch.Generator().manual_seed(10 * H + n_kv)
    q = torch.randn(B, H, 1, D, generator=g).to(torch.bfloat16).to(DEV)
    pools = reference.kv_fp8_quant_pages(
        torch.randn(N_PAGES, n_kv, R, D, generator=g).to(DEV),
        torch.randn(N_PAGES, n_kv, R, D, generator=g).to(DEV))
    table = torch.randperm(N_PAGES, generator=g)[:B * MAX_PAGES].reshape(
        B, MAX_PAGES).int().to(DEV)
    pos = torch.tensor(POS, device=DEV)
    out = decode_attention_paged_fp8(q, *pools, table, pos, SCALE)
    kd, vd = reference.kv_fp8_dequant(*pools, torch.float64)
    ref = torch.zeros(B, H, D, dtype=torch.float64, device=DEV)
    for b in range(B):
        if POS[b] < 0:
            continue
        L = POS[b] + 1
        kk, vv = (t[table[b].long()].permute(1, 0, 2, 3).reshape(
            n_kv, -1, D)[:, :L] for t in (kd, vd))
        p = torch.softmax(torch.einsum(
            "kgd,ksd->kgs", q[b, :, 0].double().reshape(n_kv, -1, D), kk)
            * SCALE, dim=-1)
        ref[b] = torch.einsum("kgs,ksd->kgd", p, vv).reshape(H, D)
    return q, pools, table, pos, out, ref


SHAPES = [(8, 2), (8, 8), (8, 1), (16, 1)]


@pytest.mark.parametrize("H,n_kv", SHAPES)
def test_decode_matches_fp64(H, n_kv):
    """2e-2 max abs (bf16 P and out: test_paged_verify_gpu's bound); idle: 0."""
    q, pools, table, pos, out, ref = _case(H, n_kv)
    err = (out[:, :, 0].double() - ref).abs().amax(dim=(1, 2))
    print(f"H {H} n_kv {n_kv}: per slot {[f'{e:.2e}' for e in err.tolist()]}")
    assert not out[POS.index(-1)].any()
    assert err.max().item() < 2e-2


@pytest.mark.parametrize("H,n_kv", SHAPES)
def test_decode_ignores_garbage(H, n_kv):
    """NaN bytes (0x7f) and NaN scales in every row beyond pos and in every
    page that holds no valid row change no bit of the output."""
    q, pools, table, pos, out, _ = _case(H, n_kv)
    keep = torch.zeros(N_PAGES, R, dtype=torch.bool, device=DEV)
    for b, p in enumerate(POS):
        n = p // R + 1 if p >= 0 else 0
        rows = torch.arange(n * R, device=DEV) <= p
        keep[table[b, :n].long()] = rows.reshape(n, R)
    k8, v8, sc = pools
    kd = torch.where(keep[:, None, :, None], k8, 0x7f)
    # the image keeps rows apart only after the inverse permutation
    vd = reference.kv_fp8_v_image(torch.where(
        keep[:, None, :, None], reference.kv_fp8_v_image(v8, inverse=True),
        0x7f))
    sd = torch.where(keep[:, None, None, :], sc, float("nan"))
    got = decode_attention_paged_fp8(q, kd, vd.contiguous(), sd, table, pos,
                                     SCALE)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, out)


@torch.no_grad()
def test_model_steps_match_twins_and_bf16_cache():
    """llama-smoke, 8 slots at 58..61 rows, 10 teacher-forced steps across the
    page boundary on three caches: fp8 on the kernels, the same pools on the
    twins, and bf16. Kernels against twins: 2e-2 max|ref| + 2e-2 (the bound
    between attention implementations of test_paged_engine_gpu's family); fp8
    against bf16 pages: that plus twice the format's error, TWIN_FORMAT_ERR."""
    native.load(require=True)
    cfg = CONFIGS["llama-smoke"]
    torch.manual_seed(5)
    model = build_inference_model(cfg, DEV)
    B, steps = 8, 10
    lens = [58 + b % 4 for b in range(B)]
    g = torch.Generator().manual_seed(3)
    caches = {n: paged.PagedKVCache(
        cfg, 3 * B, B, 2, DEV, torch.bfloat16,
        kv_dtype="bf16" if n == "bf16" else "fp8")
        for n in ("gpu", "twin", "bf16")}
    cur = []
    for b, n in enumerate(lens):
        prompt = torch.randint(0, cfg.vocab_size, (1, n), generator=g)
        tmp = KVCache(cfg, 1, n, DEV, torch.bfloat16)
        cur.append(_forward_cached(model, prompt.to(DEV), tmp)[0, -1].argmax())
        for c in caches.values():
            assert c.admit(b, n + steps)
            c.load_prefix(b, [k[0] for k in tmp.k], [v[0] for v in tmp.v], n)
    cur = torch.stack(cur)
    names = ("rope_cache_paged_fp8", "decode_attention_paged_fp8")
    kernels = [getattr(paged, n) for n in names]
    out = {n: [] for n in caches}
    for i in range(steps):
        for name, c in caches.items():
            for b in range(B):
                c.ensure_row(b, lens[b] + i)
            try:
                for n in names if name == "twin" else ():
                    setattr(paged, n, getattr(reference, n))
                out[name].append(paged._step_paged(model, cur[:, None], c))
            finally:
                for n, fn in zip(names, kernels):
                    setattr(paged, n, fn)
            c.advance()
            c.check_block_table()
        cur = out["gpu"][-1].argmax(dim=-1)
    assert max(lens) + steps > R and all(len(o) == 2
                                         for o in caches["gpu"].owned)
    gpu, twin, bf16 = (torch.stack(out[n]).float() for n in caches)
    top = twin.abs().max().item()
    err_tw, err_bf = ((gpu - x).abs().max().item() for x in (twin, bf16))
    print(f"max |logit| {top:.3e}: kernels vs twins {err_tw:.3e}, fp8 KV vs "
          f"bf16 KV {err_bf:.3e} (CPU twin {TWIN_FORMAT_ERR:.3e} at "
          f"{TWIN_MAX_LOGIT:.3e})")
    assert err_tw <= 2e-2 * top + 2e-2
    assert err_bf <= 2 * TWIN_FORMAT_ERR + 2e-2 * bf16.abs().max().item() + 2e-2
