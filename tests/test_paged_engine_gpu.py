"""Paged cache + continuous-batching engine on llama-smoke (2 layers,
head_dim 128): the paged step against the contiguous step, a ragged batch
against per-prompt batch-1 decode, and slot reuse."""
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
    PagedEngine, PagedKVCache, _step_paged,
)
from trainingjob_operator_amd.ops import native  # noqa: E402

DEV = torch.device("cuda:0")


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


@torch.no_grad()
def test_step_paged_same_bits_as_step_static(model):
    """3 equal-length prompts: the same prefilled rows in shuffled pages,
    10 greedy steps across the 64-row page boundary; logits bit-equal."""
    cfg = model.cfg
    B, S0, steps = 3, 60, 10
    prompt = torch.stack(_prompts([S0] * B, 11))
    cont = KVCache(cfg, B, S0 + steps + 4, DEV, torch.bfloat16)
    last = _forward_cached(model, prompt, cont)[:, -1]

    paged = PagedKVCache(cfg, n_pages=16, max_slots=B, max_pages_per_seq=2,
                         device=DEV, dtype=torch.bfloat16)
    random.Random(3).shuffle(paged.free_pages)
    for b in range(B):
        assert paged.admit(b, S0 + steps)
        paged.load_prefix(b, [k[b] for k in cont.k], [v[b] for v in cont.v],
                          S0)
    paged.check_block_table()

    pos_t = torch.full((1,), S0, dtype=torch.int64, device=DEV)
    arange = torch.arange(cont.max_len, device=DEV)
    cur = last.argmax(dim=-1)
    for i in range(steps):
        for b in range(B):
            paged.ensure_row(b, S0 + i)
        ref = _step_static(model, cur[:, None], cont, pos_t, arange)
        got = _step_paged(model, cur[:, None], paged)
        paged.advance()
        assert torch.equal(got, ref), f"step {i} (pos {S0 + i})"
        cur = ref.argmax(dim=-1)
    assert S0 + steps > 64                        # the boundary was crossed
    assert all(len(o) == 2 for o in paged.owned)
    paged.check_block_table()


@torch.no_grad()
def test_ragged_batch_matches_batch1_teacher_forced(model):
    """Prompts of 5, 64 and 130 tokens in one paged batch (4 slots, one
    idle), fed the batch-1 reference's tokens: every active slot's logits
    within the bf16 bound of the reference's at each of 8 steps."""
    cfg = model.cfg
    lengths, steps = [5, 64, 130], 8
    prompts = _prompts(lengths, 13)
    ref_tok, ref_logits = [], []
    for p in prompts:
        S0 = p.numel()
        cont = KVCache(cfg, 1, S0 + steps + 4, DEV, torch.bfloat16)
        last = _forward_cached(model, p[None], cont)[:, -1]
        pos_t = torch.full((1,), S0, dtype=torch.int64, device=DEV)
        arange = torch.arange(cont.max_len, device=DEV)
        toks, logs = [int(last.argmax())], []
        for _ in range(steps):
            cur = torch.tensor([[toks[-1]]], device=DEV)
            lg = _step_static(model, cur, cont, pos_t, arange)
            logs.append(lg[0].float())
            toks.append(int(lg.argmax()))
        ref_tok.append(toks)
        ref_logits.append(logs)

    eng = PagedEngine(model, max_slots=4, n_pages=8, max_pages_per_seq=3)
    random.Random(7).shuffle(eng.cache.free_pages)
    # the engine's own prefill path, slot by slot; slot 3 stays idle
    for p in prompts:
        eng.submit(p, steps + 1)
    eng._admit([])
    assert [r is not None for r in eng.slots] == [True, True, True, False]
    for s in range(3):                  # same prefill -> same first token
        assert eng.slots[s].tokens[-1] == ref_tok[s][0]
    cache = eng.cache
    bit_equal = True
    for i in range(steps):
        cur = torch.tensor([ref_tok[s][i] for s in range(3)] + [0],
                           device=DEV)
        for s in range(3):
            cache.ensure_row(s, cache.host_pos[s])
        got = _step_paged(model, cur[:, None], cache).float()
        cache.advance()
        cache.check_block_table()
        assert torch.isfinite(got).all()
        for s in range(3):
            ref = ref_logits[s][i]
            err = (got[s] - ref).abs().max().item()
            bound = 2e-2 * ref.abs().max().item() + 2e-2
            bit_equal = bit_equal and torch.equal(got[s], ref)
            print(f"len {lengths[s]} step {i}: max err {err:.3e} "
                  f"(bound {bound:.3e})")
            assert err <= bound, (lengths[s], i, err, bound)
    print(f"ragged vs batch-1 logits bit-equal: {bit_equal}")


@torch.no_grad()
def test_slot_reuse_continuous_batching(model):
    """5 requests through 2 slots: all finish with their prompt as prefix
    and the requested length, the table is valid after every step and all
    pages come back."""
    lengths = [7, 70, 33, 64, 3]
    news = [4, 9, 2, 6, 12]
    prompts = _prompts(lengths, 17)
    eng = PagedEngine(model, max_slots=2, n_pages=6, max_pages_per_seq=3)
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
    # two slots shared the work: fewer steps than one request at a time
    assert steps < sum(news)
