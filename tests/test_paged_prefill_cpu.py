"""Chunked, batched prefill straight into the paged KV cache, on a CPU
llama-tiny in fp32: the torch twins of the two prefill kernels, the engine
with prefill="paged", and the server option."""
import ctypes

import pytest
import torch

from trainingjob_operator_amd.models import paged as paged_mod
from trainingjob_operator_amd.models.config import CONFIGS
from trainingjob_operator_amd.models.generate import (
    KVCache, _forward_cached, generate,
)
from trainingjob_operator_amd.models.paged import (
    PagedEngine, generate_ragged, pages_for,
)
from trainingjob_operator_amd.ops import native, prefill_work, reference
from trainingjob_operator_amd.training import build_model

CPU = torch.device("cpu")
SEED = 19                 # test_paged_cpu.py's model init
LENGTHS = (3, 64, 70, 150)
NEW = 8


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(SEED)
    return build_model(CONFIGS["llama-tiny"], CPU).float().eval()


def _prompts(lengths=LENGTHS, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 512, (n,), generator=g) for n in lengths]


# ---------------------------------------------------------------------------
# twins
# ---------------------------------------------------------------------------

H, N_KV, D = 4, 2, 16
N_PAGES, MAX_PAGES = 12, 4
# (slot, pos0, n_rows): every pos0 of {0, 37, 64, 100} and every n_rows of
# {1, 5, 64, 130} occurs, over two slots
CHUNKS = [(0, 0, 130), (1, 37, 5), (0, 130, 1), (1, 64, 64), (1, 128, 1),
          (0, 131, 5)]
CHUNKS2 = [(0, 100, 130), (1, 0, 1), (1, 1, 64), (0, 64, 5), (1, 100, 64)]


def _pools(seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(N_PAGES, N_KV, 64, D, generator=g)
    v = torch.randn(N_PAGES, N_KV, 64, D, generator=g)
    perm = torch.randperm(N_PAGES, generator=g)[:2 * MAX_PAGES]
    table = perm.reshape(2, MAX_PAGES).to(torch.int32)     # shuffled pages
    return k, v, table


def _dense(q, k_pool, v_pool, table, chunks, scale):
    """Dense masked softmax attention on the gathered cache, row by row of
    the chunk list (packed in order)."""
    o = torch.zeros_like(q)
    G = H // N_KV
    row = 0
    for slot, pos0, n in chunks:
        k = k_pool[table[slot].long()].permute(1, 0, 2, 3).reshape(
            N_KV, -1, D).repeat_interleave(G, dim=0)       # [H, L, D]
        v = v_pool[table[slot].long()].permute(1, 0, 2, 3).reshape(
            N_KV, -1, D).repeat_interleave(G, dim=0)
        for r in range(n):
            p = pos0 + r
            s = torch.einsum("hd,hsd->hs", q[row + r], k[:, :p + 1]) * scale
            o[row + r] = torch.einsum("hs,hsd->hd", torch.softmax(s, -1),
                                      v[:, :p + 1])
        row += n
    return o


@pytest.mark.parametrize("chunks", [CHUNKS, CHUNKS2])
def test_prefill_attention_twin_matches_dense(chunks):
    k_pool, v_pool, table = _pools(3)
    T = sum(n for _, _, n in chunks)
    q = torch.randn(T, H, D, generator=torch.Generator().manual_seed(4))
    scale = D ** -0.5
    work, tok_slot, tok_pos = prefill_work(chunks)
    assert work.dtype == torch.int32 and work.shape[1] == 4
    assert tok_slot.dtype == torch.int32 and tok_pos.dtype == torch.int64
    assert tok_slot.numel() == tok_pos.numel() == T
    tiles = [(p0 + n - 1) // 64 for _, _, n, p0 in work.tolist()]
    assert tiles == sorted(tiles, reverse=True)            # heaviest first
    assert all(1 <= n <= 256 for _, _, n, _ in work.tolist())
    got = reference.prefill_attention_paged(q, k_pool, v_pool, table, work,
                                            scale)
    want = _dense(q, k_pool, v_pool, table, chunks, scale)
    assert (got - want).abs().max().item() < 1e-5

    # rows no position reaches may hold anything finite
    seen = torch.zeros(2, MAX_PAGES * 64, dtype=torch.bool)
    for slot, pos0, n in chunks:
        seen[slot, :pos0 + n] = True
    k2, v2 = torch.full_like(k_pool, 1e4), torch.full_like(v_pool, 1e4)
    for slot in range(2):
        for j in range(MAX_PAGES):
            keep = seen[slot, j * 64:(j + 1) * 64]
            pg = int(table[slot, j])
            k2[pg][:, keep] = k_pool[pg][:, keep]
            v2[pg][:, keep] = v_pool[pg][:, keep]
    got2 = reference.prefill_attention_paged(q, k2, v2, table, work, scale)
    assert torch.equal(got, got2)


def test_rope_rows_twin_equals_per_token_twin():
    nh, nkv = H, N_KV
    g = torch.Generator().manual_seed(7)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    _, _, table = _pools(5)
    tok_slot = torch.tensor([0] * 35 + [1] * 35, dtype=torch.int32)
    tok_pos = torch.cat([torch.arange(60, 95), torch.arange(0, 35)])
    tok_pos[17] = -1                                       # a padding token
    T = tok_pos.numel()
    qkv = torch.randn(T, (nh + 2 * nkv) * D, generator=g)
    k0 = torch.randn(N_PAGES, nkv, 64, D, generator=g)
    v0 = torch.randn(N_PAGES, nkv, 64, D, generator=g)

    ka, va = k0.clone(), v0.clone()
    qa = reference.rope_cache_paged_rows(qkv, ka, va, inv_freq, table,
                                         tok_slot, tok_pos, nh, nkv)
    kb, vb = k0.clone(), v0.clone()
    qb = torch.empty_like(qa)
    for t in range(T):
        s = int(tok_slot[t])
        qb[t] = reference.rope_cache_paged(
            qkv[t:t + 1], kb, vb, inv_freq, table[s:s + 1],
            tok_pos[t:t + 1], nh, nkv)[0]
    assert torch.equal(qa, qb)
    assert torch.equal(ka, kb) and torch.equal(va, vb)
    assert not qa[17].any()                                # zero q
    # exactly the addressed rows changed: T - 1 rows per pool
    changed = (ka != k0).any(dim=-1).any(dim=1)            # [n_pages, 64]
    assert int(changed.sum()) == T - 1
    assert int((va != v0).any(dim=-1).any(dim=1).sum()) == T - 1


@pytest.mark.skipif(not native.available(), reason="libhipops.so not built")
def test_work_clamp_matches_the_kernels():
    """The kernel's clamp of a work row (exported for the host) against the
    twin's, and its guarantees, on in- and out-of-range rows."""
    lib = native.load(require=True)
    vals = [-2 ** 31, -7, -1, 0, 1, 5, 63, 64, 255, 256, 257, 1000,
            2 ** 31 - 1]
    g = torch.Generator().manual_seed(0)
    for T, B, max_pages in ((1, 1, 1), (70, 2, 3), (300, 3, 4), (900, 8, 2)):
        for _ in range(200):
            row = [vals[int(i)] for i in
                   torch.randint(0, len(vals), (4,), generator=g)]
            io = (ctypes.c_int * 4)(*row)
            assert lib.attn_prefill_work_decode(io, T, B, max_pages) == 0
            slot, q_row0, n_rows, pos0 = list(io)
            assert (slot, q_row0, n_rows, pos0) == \
                reference.prefill_work_clamp(row, T, B, max_pages)
            assert 0 <= slot < B and 1 <= n_rows <= 256
            assert 0 <= q_row0 and q_row0 + n_rows <= T
            assert 0 <= pos0 and pos0 + n_rows <= max_pages * 64


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def refs(model):
    """Default-engine outputs per prompt, with the reference's top-2 margin
    asserted (as test_paged_cpu.py does) so that fp32 reordering between
    the two prefill paths cannot flip a token."""
    prompts = _prompts()
    with torch.no_grad():
        outs = generate_ragged(model, prompts, NEW, max_slots=2)
        for p, r in zip(prompts, outs):
            assert torch.equal(r, generate(model, p[None], NEW)[0])
            cont = KVCache(model.cfg, 1, r.numel(), CPU, torch.float32)
            logs = [_forward_cached(model, p[None], cont)[0, -1]]
            for t in r[p.numel():-1]:
                logs.append(
                    _forward_cached(model, t.reshape(1, 1), cont)[0, -1])
            for lg, t in zip(logs, r[p.numel():]):
                top2 = lg.topk(2).values
                assert int(lg.argmax()) == int(t)
                assert float(top2[0] - top2[1]) > 1e-3, "pick another SEED"
    return prompts, outs


def test_engine_paged_prefill_same_tokens(model, refs):
    prompts, outs = refs
    got = generate_ragged(model, prompts, NEW, max_slots=2, prefill_chunk=32)
    for r, o in zip(outs, got):
        assert torch.equal(r, o)
    # seeded sampling draws from the same logits in the same order
    a = generate_ragged(model, prompts[:3], NEW, temperature=0.8, top_k=20,
                        seed=5, max_slots=2)
    b = generate_ragged(model, prompts[:3], NEW, temperature=0.8, top_k=20,
                        seed=5, max_slots=2, prefill_chunk=32)
    for r, o in zip(a, b):
        assert torch.equal(r, o)


def test_engine_paged_prefill_bookkeeping(model, refs):
    """70 and 150 tokens first: the 70 finishes its prefill and decodes
    while the 150 is still being prefilled 32 tokens a step."""
    prompts, outs = refs
    order = [2, 3, 0, 1]
    eng = PagedEngine(model, max_slots=2, n_pages=8, max_pages_per_seq=3,
                      prefill="paged", prefill_chunk=32)
    reqs = [eng.submit_request(prompts[i], NEW) for i in order]
    long_req = reqs[1]
    prefill_steps_long = overlapped = 0
    while not eng.idle:
        before = long_req.n_prefilled
        new_before = {r.id: r.n_new for r in reqs}
        eng.step()
        eng.cache.check_block_table()
        for r in reqs:
            if r.prefilling:
                assert eng.cache.host_pos[r.slot] == -1
                assert len(eng.cache.owned[r.slot]) == \
                    pages_for(r.n_prefilled)
        if long_req.n_prefilled > before:
            prefill_steps_long += 1
            assert long_req.n_prefilled - before <= 32
            if any(r is not long_req and r.n_new > new_before[r.id]
                   and new_before[r.id] > 0 for r in reqs):
                overlapped += 1
    assert prefill_steps_long >= 5                    # ceil(150 / 32)
    assert overlapped >= 3, overlapped                # decode went on
    assert eng.prefill_steps >= 5
    assert eng.cache.pages_free == eng.cache.n_pages == 8
    assert eng.cache.pages_unreserved == 8
    for i, r in zip(order, reqs):
        assert r.done.is_set() and r.error is None
        assert r.tokens == outs[i].tolist()


def test_engine_rejects_bad_prefill_option(model):
    with pytest.raises(ValueError):
        PagedEngine(model, max_slots=1, n_pages=1, prefill="chunked")
    with pytest.raises(ValueError):
        PagedEngine(model, max_slots=1, n_pages=1, prefill="paged",
                    prefill_chunk=0)


@pytest.mark.parametrize("chunk", [None, 0])
def test_default_path_never_enters_paged_prefill(model, refs, monkeypatch,
                                                 chunk):
    def boom(*a, **k):
        raise AssertionError("_prefill_paged entered on the default path")
    monkeypatch.setattr(paged_mod, "_prefill_paged", boom)
    prompts, outs = refs
    got = generate_ragged(model, prompts[:2], NEW, max_slots=2,
                          prefill_chunk=chunk)
    for r, o in zip(outs, got):
        assert torch.equal(r, o)
    eng = PagedEngine(model, max_slots=1, n_pages=1)
    assert eng.prefill == "contiguous"


def test_prefill_failure_fails_all_and_returns_pages(model, monkeypatch):
    prompts = _prompts()
    eng = PagedEngine(model, max_slots=2, n_pages=8, max_pages_per_seq=3,
                      prefill="paged", prefill_chunk=32)
    reqs = [eng.submit_request(p, NEW) for p in prompts[1:]]
    eng.step()                                   # two admitted, one queued
    eng.cache.check_block_table()
    assert eng.cache.pages_free < 8

    def boom(*a, **k):
        raise RuntimeError("prefill broke")
    monkeypatch.setattr(paged_mod, "_prefill_paged", boom)
    with pytest.raises(RuntimeError):
        eng.step()
    for r in reqs:
        assert r.done.is_set() and isinstance(r.error, RuntimeError)
        assert r.slot is None and not r.prefilling
    assert eng.idle
    assert eng.cache.pages_free == eng.cache.pages_unreserved == 8
    eng.cache.check_block_table()


# ---------------------------------------------------------------------------
# server
# ---------------------------------------------------------------------------

def test_server_prefill_chunk(model, refs):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from trainingjob_operator_amd.launcher.serve import create_app
    prompts = [p.tolist() for p in refs[0]]
    body = {"prompt_tokens": prompts, "max_new_tokens": NEW}
    with TestClient(create_app(model, "llama-tiny", paged=True,
                               max_slots=2)) as c:
        assert c.get("/info").json()["prefill_chunk"] == 0
        base = c.post("/generate", json=body)
        assert base.status_code == 200, base.text
    with TestClient(create_app(model, "llama-tiny", paged=True, max_slots=2,
                               prefill_chunk=32)) as c:
        info = c.get("/info").json()
        assert info["paged"] is True and info["prefill_chunk"] == 32
        r = c.post("/generate", json=body)
        assert r.status_code == 200, r.text
        assert r.json()["tokens"] == base.json()["tokens"]
        assert r.json()["tokens"] == [o.tolist() for o in refs[1]]
        info = c.get("/info").json()
        assert info["pages_free"] == info["pages_total"]
