"""Paged speculative verify on a CPU llama-tiny in fp32: the torch twin of
attn_verify_paged, and the engine's prompt-lookup steps against plain
decode."""
import pytest
import torch

from trainingjob_operator_amd.models.config import CONFIGS
from trainingjob_operator_amd.models.paged import PagedEngine, generate_ragged
from trainingjob_operator_amd.ops import reference
from trainingjob_operator_amd.training import build_model

CPU = torch.device("cpu")
NEW = 12


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(19)
    return build_model(CONFIGS["llama-tiny"], CPU).float().eval()


def _prompts(model):
    """Two random prompts (5 and 66 tokens), then two repetitive ones of 62
    and 54: a random prompt, its own greedy continuation, and the start of
    both again, which the model then replays."""
    g = torch.Generator().manual_seed(0)
    rnd = [torch.randint(0, 512, (n,), generator=g) for n in (5, 66, 24, 20)]
    outs = generate_ragged(model, rnd[2:], NEW)
    return rnd[:2] + [torch.cat([o, o[:p.numel() + 2]])
                      for p, o in zip(rnd[2:], outs)]


@pytest.mark.parametrize("D", [16, 128])
def test_twin_matches_dense_masked_softmax(D):
    B, T, H, n_kv, R, max_pages = 4, 5, 4, 2, 64, 3
    g = torch.Generator().manual_seed(D)
    q = torch.randn(B, T, H, D, generator=g)
    kp = torch.randn(16, n_kv, R, D, generator=g)
    vp = torch.randn(16, n_kv, R, D, generator=g)
    table = torch.randperm(16, generator=g)[:B * max_pages].reshape(
        B, max_pages).to(torch.int32)
    pos = torch.tensor([0, 62, -1, 130])
    nq = [5, 3, 2, 1]
    scale = D ** -0.5
    # garbage beyond each slot's last valid row must not matter
    kd, vd = kp.clone(), vp.clone()
    for b in range(B):
        rows = torch.arange(max_pages * R) > max(int(pos[b]), 0) + nq[b] - 1
        for j, page in enumerate(table[b].tolist()):
            kd[page][:, rows[j * R:(j + 1) * R]] = float("nan")
            vd[page][:, rows[j * R:(j + 1) * R]] = float("nan")
    got = reference.verify_attention_paged(
        q, kd, vd, table, pos, torch.tensor(nq, dtype=torch.int32), scale)
    for b in range(B):
        k = kp[table[b].long()].permute(1, 0, 2, 3).reshape(n_kv, -1, D)
        v = vp[table[b].long()].permute(1, 0, 2, 3).reshape(n_kv, -1, D)
        for t in range(T):
            if pos[b] < 0 or t >= nq[b]:
                assert not got[b, t].any()
                continue
            L = int(pos[b]) + t + 1
            s = torch.einsum("kgd,ksd->kgs", q[b, t].reshape(n_kv, 2, D),
                             k[:, :L]) * scale
            ref = torch.einsum("kgs,ksd->kgd", torch.softmax(s, -1), v[:, :L])
            assert (got[b, t] - ref.reshape(H, D)).abs().max() < 1e-5


def _run(model, prompts, lookup_k, eos=None):
    """Drain an engine step by step; returns (outputs, engine, the token
    runs each step gave request 2)."""
    eng = PagedEngine(model, max_slots=3, n_pages=8, max_pages_per_seq=2,
                      lookup_k=lookup_k)
    reqs = [eng.submit_request(p, NEW, eos_token=eos) for p in prompts]
    runs = []
    while not eng.idle:
        before = len(reqs[2].tokens)
        eng.step()
        eng.cache.check_block_table()
        runs.append(reqs[2].tokens[before:])
    assert eng.cache.pages_free == 8
    return [r.tokens for r in reqs], eng, runs


def test_lookup_engine_matches_plain_decode(model):
    """lookup_k=4 gives the tokens of lookup_k=0 for ragged prompts (two of
    them repetitive, four requests over three slots, one crossing row 64
    while it drafts), accepts drafts, stops on an EOS inside an accepted
    run, and hands every page back."""
    prompts = _prompts(model)
    plain, eng0, _ = _run(model, prompts, 0)
    spec, eng, runs = _run(model, prompts, 4)
    assert spec == plain
    assert eng.accepted >= 1 and eng.steps < eng0.steps
    assert generate_ragged(model, prompts[:2], 4, lookup_k=4)[1].tolist() \
        == plain[1][:66 + 4]
    assert len(plain[2]) > 64 > prompts[2].numel()
    # an EOS that request 2 first emits in the middle of an accepted run
    gen = plain[2][prompts[2].numel():]
    # (runs[0] also holds the prefill's token, so it does not count)
    eos, off = None, 0
    for i, run in enumerate(runs):
        for j, t in enumerate(run[:-1]):
            if i > 0 and eos is None and gen.index(t) == off + j:
                eos = t
        off += len(run)
    assert eos is not None, "no fresh token inside an accepted run"
    cut = prompts[2].numel() + gen.index(eos) + 1
    for k in (0, 4):
        assert _run(model, prompts, k, eos=eos)[0][2] == plain[2][:cut]


def test_lookup_with_graph_is_refused(model):
    with pytest.raises(ValueError):
        PagedEngine(model, max_slots=2, lookup_k=4, graph=True)
