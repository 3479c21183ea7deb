"""Paged KV cache, continuous-batching engine and the paged server on a
CPU llama-tiny in fp32 (the torch twins of the paged kernels)."""
import threading

import pytest
import torch

from trainingjob_operator_amd.models.config import CONFIGS
from trainingjob_operator_amd.models.generate import (
    KVCache, _forward_cached, generate,
)
from trainingjob_operator_amd.models.paged import (
    PagedEngine, PagedKVCache, _step_paged, generate_ragged,
)
from trainingjob_operator_amd.training import build_model

CPU = torch.device("cpu")
SEED = 19                 # model init: reference top-2 margin 6e-3 (asserted)
LENGTHS = (3, 64, 70)
NEW = 8


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(SEED)
    return build_model(CONFIGS["llama-tiny"], CPU).float().eval()


def _prompts(lengths=LENGTHS, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 512, (n,), generator=g) for n in lengths]


def _cache(n_pages=6, max_slots=3, max_pages=4):
    return PagedKVCache(CONFIGS["llama-tiny"], n_pages, max_slots,
                        max_pages, CPU, torch.float32)


def test_allocator_reserve_grow_release():
    c = _cache()
    assert c.admit(0, 130)                       # 3 pages reserved
    assert c.pages_free == 6 and c.pages_unreserved == 3
    assert c.admit(1, 128)                       # 2 pages
    assert c.pages_unreserved == 1
    assert not c.admit(2, 65)                    # 2 pages: not now
    assert c.reserved[2] == 0
    with pytest.raises(ValueError):
        c.admit(2, 4 * 64 + 1)                   # > max_pages_per_seq: never
    with pytest.raises(ValueError):
        _cache(n_pages=2).admit(0, 3 * 64)       # > the pool: never
    # physical pages are taken as the position crosses page boundaries
    c.set_pos(0, 0)
    for row in range(130):
        c.ensure_row(0, row)
        assert len(c.owned[0]) == row // 64 + 1
    c.set_pos(0, 129)
    c.ensure_row(1, 0)
    c.set_pos(1, 0)
    c.check_block_table()
    assert c.pages_free == 2
    owned = c.owned[0] + c.owned[1]
    assert len(set(owned)) == len(owned) == 4    # never owned twice
    with pytest.raises(AssertionError):
        c.grow(0)                                # past the reservation
    c.release(0)
    c.check_block_table()
    assert c.pages_free == 5 and c.host_pos[0] == -1
    assert int(c.pos[0]) == -1
    assert c.admit(2, 65)                        # fits after the release
    c.release(1)
    c.release(2)
    c.check_block_table()
    assert c.pages_free == c.n_pages == c.pages_unreserved


def test_check_block_table_rejects_corruption():
    def fresh():
        c = _cache()
        for s, rows in ((0, 100), (1, 64)):
            assert c.admit(s, rows)
            c.ensure_row(s, rows - 1)
            c.set_pos(s, rows - 1)
        c.check_block_table()
        return c

    c = fresh()
    c.block_table[1, 0] = c.owned[0][0]          # device table: page twice
    with pytest.raises(AssertionError):
        c.check_block_table()
    c = fresh()
    c.owned[1][0] = c.owned[0][1]                # host + device: owned twice
    c.block_table[1, 0] = c.owned[0][1]
    with pytest.raises(AssertionError):
        c.check_block_table()
    c = fresh()
    c.free_pages.append(c.owned[0][0])           # owned page on the free list
    with pytest.raises(AssertionError):
        c.check_block_table()
    c = fresh()
    c.block_table[0, 1] = c.n_pages              # out of range
    with pytest.raises(AssertionError):
        c.check_block_table()
    c = fresh()
    c.pos[0] = 5                                 # device pos off the mirror
    with pytest.raises(AssertionError):
        c.check_block_table()
    c = fresh()
    c.free_pages.pop()                           # a page leaked
    with pytest.raises(AssertionError):
        c.check_block_table()


def test_engine_queue_waits_and_refuses(model):
    eng = PagedEngine(model, max_slots=2, n_pages=2, max_pages_per_seq=2)
    with pytest.raises(ValueError):
        eng.submit(torch.arange(120), 9)         # 3 pages: can never fit
    a = eng.submit(torch.arange(60), 6)          # 2 pages: the whole pool
    b = eng.submit(torch.arange(5), 3)           # fits only after a is done
    done = []
    eng.step()
    assert eng.slots[0] is not None and eng.slots[0].id == a
    assert eng.slots[1] is None and len(eng.queue) == 1     # b waits
    while not eng.idle:
        done += [r.id for r in eng.step()]
        eng.cache.check_block_table()
    assert done == [a, b]
    assert eng.cache.pages_free == 2


@torch.no_grad()
def test_generate_ragged_matches_generate(model):
    """Ragged prompts (3, 64, 70 tokens; 8 new) against generate() per
    prompt: teacher-forced paged logits within 1e-4 of the contiguous
    path's, and the same tokens. The reference's top-2 margin is checked
    so that a near-tie cannot decide the token comparison."""
    prompts = _prompts()
    refs = [generate(model, p[None], NEW)[0] for p in prompts]

    # reference logits, step by step, on the contiguous cache
    ref_logits = []
    for p, r in zip(prompts, refs):
        cont = KVCache(model.cfg, 1, r.numel(), CPU, torch.float32)
        logs = [_forward_cached(model, p[None], cont)[0, -1]]
        for t in r[p.numel():-1]:
            logs.append(_forward_cached(model, t.reshape(1, 1), cont)[0, -1])
        for lg, t in zip(logs, r[p.numel():]):
            top2 = lg.topk(2).values
            assert int(lg.argmax()) == int(t)
            assert float(top2[0] - top2[1]) > 1e-3, "pick another SEED"
        ref_logits.append(logs)

    # teacher-forced paged steps: 4 slots, the last one idle
    eng = PagedEngine(model, max_slots=4, n_pages=8, max_pages_per_seq=2)
    for p in prompts:
        eng.submit(p, NEW)
    eng._admit([])
    cache = eng.cache
    for i in range(1, NEW):
        cur = torch.tensor([int(r[p.numel() + i - 1])
                            for p, r in zip(prompts, refs)] + [0])
        for s in range(3):
            cache.ensure_row(s, cache.host_pos[s])
        got = _step_paged(model, cur[:, None], cache)
        cache.advance()
        cache.check_block_table()
        assert torch.isfinite(got).all()
        for s in range(3):
            err = (got[s] - ref_logits[s][i]).abs().max().item()
            assert err < 1e-4, (LENGTHS[s], i, err)

    outs = generate_ragged(model, prompts, NEW)
    for r, o in zip(refs, outs):
        assert torch.equal(r, o)
    # seeded sampling: each request draws like generate() at batch 1
    outs = generate_ragged(model, prompts, NEW, temperature=0.8, top_k=20,
                           seed=5, max_slots=2)
    for p, o in zip(prompts, outs):
        r = generate(model, p[None], NEW, temperature=0.8, top_k=20,
                     seed=5)[0]
        assert torch.equal(r, o)


def test_generate_ragged_eos_returns_pages_early(model):
    p = _prompts()[0]
    full = generate_ragged(model, [p], NEW)[0]
    eos = int(full[p.numel() + 2])               # third generated token
    eng = PagedEngine(model, max_slots=1, n_pages=1)
    eng.submit(p, NEW, eos_token=eos)
    out = eng.run()[0]
    cut = full[:p.numel() + NEW].tolist().index(eos, p.numel()) + 1
    assert out.tolist() == full[:cut].tolist()
    assert eng.cache.pages_free == 1


# ---------------------------------------------------------------------------
# server
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def paged_client(model):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from trainingjob_operator_amd.launcher.serve import create_app
    with TestClient(create_app(model, "llama-tiny", paged=True)) as c:
        yield c


def test_paged_server_ragged_request(paged_client):
    prompts = [p.tolist() for p in _prompts()]
    r = paged_client.post("/generate", json={"prompt_tokens": prompts,
                                             "max_new_tokens": NEW})
    assert r.status_code == 200, r.text
    body = r.json()
    assert [len(t) for t in body["tokens"]] == [n + NEW for n in LENGTHS]
    assert body["decode_tok_s"] > 0
    for p, t in zip(prompts, body["tokens"]):
        one = paged_client.post("/generate", json={
            "prompt_tokens": [p], "max_new_tokens": NEW})
        assert one.status_code == 200, one.text
        assert one.json()["tokens"] == [t]
    info = paged_client.get("/info").json()
    assert info["paged"] is True and info["max_slots"] == 8
    assert info["pages_free"] == info["pages_total"] > 0
    # validation still holds, and an impossible request is a 400
    assert paged_client.post("/generate", json={
        "prompt_tokens": []}).status_code == 400
    assert paged_client.post("/generate", json={
        "prompt_tokens": [[1] * 30000], "max_new_tokens": 8
    }).status_code == 400
    # prompt_lookup keeps the batch-1 path
    base = paged_client.post("/generate", json={
        "prompt_tokens": [[5, 6, 7, 5, 6, 7, 5, 6]],
        "max_new_tokens": 12}).json()["tokens"]
    spec = paged_client.post("/generate", json={
        "prompt_tokens": [[5, 6, 7, 5, 6, 7, 5, 6]],
        "max_new_tokens": 12, "prompt_lookup": 4}).json()["tokens"]
    assert base == spec


def test_paged_server_concurrent_requests(paged_client):
    prompts = [p.tolist() for p in _prompts((9, 40), seed=2)]
    results = [None, None]

    def call(i):
        results[i] = paged_client.post("/generate", json={
            "prompt_tokens": [prompts[i]], "max_new_tokens": 6 + 10 * i})

    threads = [threading.Thread(target=call, args=(i,)) for i in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert all(not t.is_alive() for t in threads)
    for i, r in enumerate(results):
        assert r is not None and r.status_code == 200, r and r.text
        toks = r.json()["tokens"][0]
        assert toks[:len(prompts[i])] == prompts[i]
        assert len(toks) == len(prompts[i]) + 6 + 10 * i
    info = paged_client.get("/info").json()
    assert info["paged"] is True
    assert info["pages_free"] == info["pages_total"]
    m = paged_client.get("/metrics")
    if m.status_code == 200:                     # prometheus_client present
        assert "aitj_serve_pages_free" in m.text
        assert "aitj_serve_active_slots" in m.text


def test_default_server_still_rejects_ragged(model):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from trainingjob_operator_amd.launcher.serve import create_app
    c = TestClient(create_app(model, "llama-tiny"))
    assert c.post("/generate", json={
        "prompt_tokens": [[1, 2], [1]]}).status_code == 400
    assert "paged" not in c.get("/info").json()
