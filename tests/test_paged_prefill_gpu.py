"""Paged prefill on the GPU: rope_cache_paged_rows against the per-sequence
kernel, attn_prefill_paged against the v7 forward (bit equality) and the
fp32 twin (ragged chunks), its clamps, _prefill_paged against the contiguous
prefill on llama-smoke, and the engine with prefill="paged"."""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.models.config import CONFIGS  # noqa: E402
from trainingjob_operator_amd.models.decode_graph import (  # noqa: E402
    _step_static,
)
from trainingjob_operator_amd.models.generate import (  # noqa: E402
    KVCache, _forward_cached, build_inference_model,
)
from trainingjob_operator_amd.models.paged import (  # noqa: E402
    PagedEngine, _prefill_paged, _step_paged,
)
from trainingjob_operator_amd.ops import (  # noqa: E402
    native, prefill_attention_paged, prefill_work, reference,
    rope_cache_paged, rope_cache_paged_rows,
)
from trainingjob_operator_amd.ops.attention import (  # noqa: E402
    flash_attention_fwd_v7,
)

DEV = torch.device("cuda:0")
D = 128
FWD_TOL = dict(atol=3e-2, rtol=2e-2)     # tests/test_doc_attention_gpu.py
SCALE = 1.0 / math.sqrt(D)


def _randn(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


def _paged(k, v, n_pages, seed):
    """Contiguous [n_kv, S, D] k/v -> shuffled pools + a one-slot table."""
    n_kv, S, _ = k.shape
    n = (S + 63) // 64
    order = list(range(n_pages))
    random.Random(seed).shuffle(order)
    pages = order[:n]
    k_pool = _randn(n_pages, n_kv, 64, D, seed=seed + 100)
    v_pool = _randn(n_pages, n_kv, 64, D, seed=seed + 101)
    for j, pg in enumerate(pages):
        rows = slice(j * 64, min(S, j * 64 + 64))
        k_pool[pg, :, :rows.stop - rows.start] = k[:, rows]
        v_pool[pg, :, :rows.stop - rows.start] = v[:, rows]
    table = torch.tensor([pages], dtype=torch.int32, device=DEV)
    return k_pool, v_pool, table


# ---------------------------------------------------------------------------
# rope_cache_paged_rows
# ---------------------------------------------------------------------------

def test_rope_rows_same_bits_as_per_sequence_kernel():
    native.load(require=True)
    nh, nkv, n_pages, max_pages = 4, 2, 6, 2
    inv_freq = (1.0 / (500000.0 ** (torch.arange(0, D, 2).float() / D))
                ).to(DEV)
    table = torch.tensor([[4, 1], [2, 5]], dtype=torch.int32, device=DEV)
    tok_slot = torch.tensor([0] * 35 + [1] * 35, dtype=torch.int32,
                            device=DEV)
    tok_pos = torch.cat([torch.arange(60, 95), torch.arange(0, 35)]).to(DEV)
    tok_pos[50] = -1
    T = 70
    qkv = _randn(T, (nh + 2 * nkv) * D, seed=1)
    k0 = _randn(n_pages, nkv, 64, D, seed=2)
    v0 = _randn(n_pages, nkv, 64, D, seed=3)

    ka, va = k0.clone(), v0.clone()
    qa = rope_cache_paged_rows(qkv, ka, va, inv_freq, table, tok_slot,
                               tok_pos, nh, nkv)
    kb, vb = k0.clone(), v0.clone()
    qb = torch.empty_like(qa)
    for t in range(T):
        s = int(tok_slot[t])
        qb[t] = rope_cache_paged(qkv[t:t + 1], kb, vb, inv_freq,
                                 table[s:s + 1].contiguous(),
                                 tok_pos[t:t + 1].contiguous(), nh, nkv)[0]
    assert torch.equal(qa, qb)
    assert torch.equal(ka, kb) and torch.equal(va, vb)
    assert not qa[50].any()
    # only the addressed rows may differ from the initial pools
    addressed = torch.zeros(n_pages, 64, dtype=torch.bool, device=DEV)
    for t in range(T):
        p = int(tok_pos[t])
        if p >= 0:
            addressed[int(table[int(tok_slot[t]), p // 64]), p % 64] = True
    assert int(addressed.sum()) == T - 1
    for new, old in ((ka, k0), (va, v0)):
        keep = ~addressed[:, None, :, None].expand_as(new)
        assert torch.equal(new[keep], old[keep])


# ---------------------------------------------------------------------------
# attn_prefill_paged
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("H,n_kv", [(4, 2), (4, 4), (4, 1)])
def test_same_bits_as_v7_on_the_gathered_cache(H, n_kv):
    native.load(require=True)
    outs = {}
    for S in (256, 512):
        q = _randn(S, H, D, seed=10 + S)
        k = _randn(n_kv, S, D, seed=11 + S)
        v = _randn(n_kv, S, D, seed=12 + S)
        ref, _ = flash_attention_fwd_v7(q.transpose(0, 1)[None], k[None],
                                        v[None], SCALE)
        ref = ref[0].transpose(0, 1)                       # [S, H, D]
        k_pool, v_pool, table = _paged(k, v, 11, seed=S)
        work, _, _ = prefill_work([(0, 0, S)], DEV)
        o = prefill_attention_paged(q, k_pool, v_pool, table, work, SCALE)
        assert o is not None
        assert torch.equal(o, ref), f"S={S}"
        outs[S] = (q, k_pool, v_pool, table, ref)
    # the second half alone, as a chunk at pos0 = 256 over the 512-row cache
    q, k_pool, v_pool, table, ref = outs[512]
    work, _, _ = prefill_work([(0, 256, 256)], DEV)
    o = prefill_attention_paged(q[256:].contiguous(), k_pool, v_pool, table,
                                work, SCALE)
    assert torch.equal(o, ref[256:])


RAGGED = [(0, 0, 1), (1, 0, 37), (0, 5, 64), (2, 63, 2), (1, 64, 130),
          (0, 100, 300)]                  # (slot, pos0, n_rows)
GAP = 3                                   # unused q/o rows before each chunk


def _ragged_case(H=4, n_kv=2, max_pages=7, n_pages=24):
    order = list(range(n_pages))
    random.Random(5).shuffle(order)
    table = torch.tensor(order[:3 * max_pages], dtype=torch.int32,
                         device=DEV).reshape(3, max_pages)
    k_pool = _randn(n_pages, n_kv, 64, D, seed=20)
    v_pool = _randn(n_pages, n_kv, 64, D, seed=21)
    rows, used, cur = [], [], 0
    for slot, pos0, n in RAGGED:
        cur += GAP
        for off in range(0, n, 256):
            rows.append((slot, cur + off, min(256, n - off), pos0 + off))
        used.append((cur, cur + n))
        cur += n
    T = cur + GAP
    rows.sort(key=lambda r: -((r[3] + r[2] - 1) // 64))
    work = torch.tensor(rows, dtype=torch.int32, device=DEV)
    q = _randn(T, H, D, seed=22)
    valid = torch.zeros(T, dtype=torch.bool, device=DEV)
    for a, b in used:
        valid[a:b] = True
    return q, k_pool, v_pool, table, work, valid


def test_ragged_chunks_match_the_twin_and_ignore_garbage():
    native.load(require=True)
    q, k_pool, v_pool, table, work, valid = _ragged_case()
    o = prefill_attention_paged(q, k_pool, v_pool, table, work, SCALE)
    ref = reference.prefill_attention_paged(q, k_pool, v_pool, table, work,
                                            SCALE)
    err = (o[valid].float() - ref[valid].float()).abs().max().item()
    print(f"ragged chunks vs fp32 twin: max abs err {err:.3e}")
    torch.testing.assert_close(o[valid].float(), ref[valid].float(),
                               **FWD_TOL)
    # deterministic
    o_again = prefill_attention_paged(q, k_pool, v_pool, table, work, SCALE)
    assert torch.equal(o[valid], o_again[valid])

    # +-1e4 in every cache row no position reaches, in every page outside
    # the table, and in the q/o rows outside the work list
    n_pages, n_kv = k_pool.shape[:2]
    sign = torch.where(torch.arange(D, device=DEV) % 2 == 0, 1e4, -1e4).to(
        torch.bfloat16)
    k2 = sign.expand_as(k_pool).clone()
    v2 = (-sign).expand_as(v_pool).clone()
    last = {}
    for slot, pos0, n in RAGGED:
        last[slot] = max(last.get(slot, 0), pos0 + n)
    for slot, rows in last.items():
        for j in range((rows + 63) // 64):
            pg = int(table[slot, j])
            r = min(64, rows - j * 64)
            k2[pg, :, :r] = k_pool[pg, :, :r]
            v2[pg, :, :r] = v_pool[pg, :, :r]
    q2 = torch.where(valid[:, None, None], q, sign.expand_as(q))
    o2 = (-sign).expand_as(q).clone()
    ret = prefill_attention_paged(q2, k2, v2, table, work, SCALE, out=o2)
    assert ret is o2
    assert torch.equal(o2[valid], o[valid])
    assert torch.equal(o2[~valid], (-sign).expand_as(q)[~valid])  # unwritten


def test_clamps_keep_every_access_inside_the_operands():
    """Out-of-range work and table fields complete and leave the canaries
    around q, o and the pools intact. Every field is clamped before it forms
    an address, so nothing here relies on an access going out of range."""
    native.load(require=True)
    H, n_kv, T, B, max_pages, n_pages = 4, 2, 70, 2, 2, 5
    pad = 4096

    def framed(*shape, seed):
        n = math.prod(shape)
        buf = torch.full((n + 2 * pad,), 7.0, dtype=torch.bfloat16,
                         device=DEV)
        buf[pad:pad + n] = _randn(n, seed=seed)
        return buf, buf[pad:pad + n].view(*shape)

    qb, q = framed(T, H, D, seed=30)
    ob, o = framed(T, H, D, seed=31)
    kb, k_pool = framed(n_pages, n_kv, 64, D, seed=32)
    vb, v_pool = framed(n_pages, n_kv, 64, D, seed=33)
    big = 2 ** 31 - 1
    table = torch.tensor([[-5, 99], [big, -big]], dtype=torch.int32,
                         device=DEV)
    work = torch.tensor([
        [0, 0, 70, 0],                    # valid
        [7, 60, 40, 100],                 # slot, rows and positions beyond
        [-3, -9, -1, -4],
        [big, big, big, big],
        [-big, 69, 300, 127],
        [1, T, 0, max_pages * 64],
    ], dtype=torch.int32, device=DEV)
    for row in work.tolist():             # what the kernel makes of them
        s, r0, n, p0 = reference.prefill_work_clamp(row, T, B, max_pages)
        assert 0 <= s < B and 0 <= r0 and r0 + n <= T
        assert 1 <= n <= 256 and 0 <= p0 and p0 + n <= max_pages * 64
    ret = prefill_attention_paged(q, k_pool, v_pool, table, work, SCALE,
                                  out=o)
    assert ret is o
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all()
    for buf in (qb, ob, kb, vb):
        assert (buf[:pad] == 7.0).all() and (buf[-pad:] == 7.0).all()


# ---------------------------------------------------------------------------
# _prefill_paged and the engine on llama-smoke
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    native.load(require=True)
    torch.manual_seed(5)
    return build_inference_model(CONFIGS["llama-smoke"], DEV)


def _prompts(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    vocab = CONFIGS["llama-smoke"].vocab_size
    return [torch.randint(0, vocab, (n,), generator=g).to(DEV)
            for n in lengths]


def _close(got, ref, what):
    err = (got.float() - ref.float()).abs().max().item()
    bound = 2e-2 * ref.float().abs().max().item() + 2e-2
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (what, err, bound)


@torch.no_grad()
def test_prefill_paged_matches_contiguous_prefill(model):
    """5, 64 and 130 tokens in one packed batch, the 130 again in chunks of
    50 in a fourth slot: last-row logits against _forward_cached's, then 4
    teacher-forced paged decode steps against the contiguous step."""
    cfg = model.cfg
    lengths, steps = [5, 64, 130], 4
    prompts = _prompts(lengths, 13)
    ref_last, ref_tok, ref_logits = [], [], []
    for p in prompts:
        S0 = p.numel()
        cont = KVCache(cfg, 1, S0 + steps + 4, DEV, torch.bfloat16)
        last = _forward_cached(model, p[None], cont)[0, -1]
        pos_t = torch.full((1,), S0, dtype=torch.int64, device=DEV)
        arange = torch.arange(cont.max_len, device=DEV)
        toks, logs = [int(last.argmax())], []
        for _ in range(steps):
            cur = torch.tensor([[toks[-1]]], device=DEV)
            lg = _step_static(model, cur, cont, pos_t, arange)
            logs.append(lg[0].float())
            toks.append(int(lg.argmax()))
        ref_last.append(last)
        ref_tok.append(toks)
        ref_logits.append(logs)

    eng = PagedEngine(model, max_slots=4, n_pages=12, max_pages_per_seq=3)
    cache = eng.cache
    random.Random(7).shuffle(cache.free_pages)
    slot_len = lengths + [130]
    for s, n in enumerate(slot_len):
        assert cache.admit(s, n + steps + 1)
    chunks = [(s, 0, n) for s, n in enumerate(lengths)]
    last_rows, row = [], 0
    for s, _, n in chunks:
        cache.ensure_row(s, n - 1)
        row += n
        last_rows.append(row - 1)
    got = _prefill_paged(model, torch.cat(prompts)[None], cache, chunks,
                         last_rows)
    assert got.shape == (3, cfg.vocab_size)
    for s in range(3):
        _close(got[s], ref_last[s], f"packed prefill, len {lengths[s]}")
    # the 130-token prompt in chunks of 50
    for p0 in (0, 50, 100):
        n = min(50, 130 - p0)
        cache.ensure_row(3, p0 + n - 1)
        got = _prefill_paged(model, prompts[2][p0:p0 + n][None], cache,
                             [(3, p0, n)], [n - 1] if p0 + n == 130 else [])
        assert got.shape[0] == (1 if p0 + n == 130 else 0)
    _close(got[0], ref_last[2], "chunked prefill, len 130")

    for s, n in enumerate(slot_len):
        cache.set_pos(s, n)
    cache.check_block_table()
    ref_of = [0, 1, 2, 2]
    for i in range(steps):
        cur = torch.tensor([ref_tok[r][i] for r in ref_of], device=DEV)
        for s in range(4):
            cache.ensure_row(s, cache.host_pos[s])
        got = _step_paged(model, cur[:, None], cache).float()
        cache.advance()
        cache.check_block_table()
        for s, r in enumerate(ref_of):
            _close(got[s], ref_logits[r][i], f"slot {s} decode step {i}")


@torch.no_grad()
def test_engine_paged_prefill_slot_reuse(model):
    """test_slot_reuse_continuous_batching with prefill="paged"."""
    lengths = [7, 70, 33, 64, 3]
    news = [4, 9, 2, 6, 12]
    prompts = _prompts(lengths, 17)
    eng = PagedEngine(model, max_slots=2, n_pages=6, max_pages_per_seq=3,
                      prefill="paged", prefill_chunk=64)
    ids = [eng.submit(p, n) for p, n in zip(prompts, news)]
    done, steps = {}, 0
    while not eng.idle:
        for r in eng.step():
            done[r.id] = r.tokens
        eng.cache.check_block_table()
        steps += 1
        assert steps < 64
    assert sorted(done) == sorted(ids)
    for rid, p, n in zip(ids, prompts, news):
        assert done[rid][:p.numel()] == p.tolist()
        assert len(done[rid]) == p.numel() + n
    assert eng.cache.pages_free == eng.cache.n_pages
    assert eng.prefill_steps >= 2
