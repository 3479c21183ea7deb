"""Paged speculative verify (attn_verify_paged, head_dim 128) against fp32
softmax attention over the gathered rows, its row independence and garbage
contract bit for bit, and _verify_paged against T teacher-forced decode
steps."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.models.config import CONFIGS  # noqa: E402
from trainingjob_operator_amd.models.generate import (  # noqa: E402
    KVCache, _forward_cached, build_inference_model,
)
from trainingjob_operator_amd.models.paged import (  # noqa: E402
    PagedKVCache, _step_paged, _verify_paged,
)
from trainingjob_operator_amd.ops import (  # noqa: E402
    native, reference, verify_attention_paged,
)

DEV = "cuda:0"
D, R, MAX_PAGES, N_PAGES, B = 128, 64, 5, 32, 4
POS = [0, 60, 64, 200]       # first row, a draft straddling a page boundary
#                              at T=8, a page start, mid table
SCALE = 1.0 / math.sqrt(D)
SHAPES = [(8, 2), (8, 8), (8, 1)]
TS = [1, 5, 8]


@functools.lru_cache(maxsize=None)
def _case(H, n_kv, T):
    """Inputs, the all-valid kernel output and the fp32 reference, made once
    per shape and never written to."""
    native.load(require=True)
    gen = torch.Generator().manual_seed(100 * n_kv + T)

    def mk(*shape):
        return torch.randn(*shape, generator=gen).to(torch.bfloat16).to(DEV)

    q, kp, vp = mk(B, T, H, D), mk(N_PAGES, n_kv, R, D), mk(N_PAGES, n_kv, R, D)
    table = torch.randperm(N_PAGES, generator=gen)[:B * MAX_PAGES].reshape(
        B, MAX_PAGES).to(torch.int32).to(DEV)
    pos = torch.tensor(POS, dtype=torch.int64, device=DEV)
    n_q = torch.full((B,), T, dtype=torch.int32, device=DEV)
    out = verify_attention_paged(q, kp, vp, table, pos, n_q, SCALE)
    assert out is not None and out.shape == (B, T, H, D)
    ref = torch.empty(B, T, H, D, device=DEV)
    for b in range(B):
        k = kp[table[b].long()].permute(1, 0, 2, 3).reshape(n_kv, -1, D).float()
        v = vp[table[b].long()].permute(1, 0, 2, 3).reshape(n_kv, -1, D).float()
        for t in range(T):
            L = POS[b] + t + 1
            qg = q[b, t].float().reshape(n_kv, H // n_kv, D)
            p = torch.softmax(
                torch.einsum("kgd,ksd->kgs", qg, k[:, :L]) * SCALE, dim=-1)
            ref[b, t] = torch.einsum("kgs,ksd->kgd", p, v[:, :L]).reshape(H, D)
    return q, kp, vp, table, pos, n_q, out, ref


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("H,n_kv", SHAPES)
def test_verify_matches_fp32(H, n_kv, T):
    """Kernel and twin within the decode bound (2e-2, unit-normal inputs) of
    fp32 softmax attention over rows 0..pos+t."""
    q, kp, vp, table, pos, n_q, out, ref = _case(H, n_kv, T)
    err = (out.float() - ref).abs().max().item()
    tw = reference.verify_attention_paged(q, kp, vp, table, pos, n_q, SCALE)
    err_tw = (tw.float() - ref).abs().max().item()
    print(f"H {H} n_kv {n_kv} T {T}: kernel {err:.3e} twin {err_tw:.3e}")
    assert err < 2e-2 and err_tw < 2e-2


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("H,n_kv", SHAPES)
def test_verify_rows_independent(H, n_kv, T):
    """Ragged n_q and an idle slot: valid rows keep the bits of the
    all-valid call, every other row is exactly zero."""
    q, kp, vp, table, pos, _, out, _ = _case(H, n_kv, T)
    nq = [min(n, T) for n in (1, 3, T, 2)]
    n_q = torch.tensor(nq, dtype=torch.int32, device=DEV)
    got = verify_attention_paged(q, kp, vp, table, pos, n_q, SCALE)
    for b in range(B):
        assert torch.equal(got[b, :nq[b]], out[b, :nq[b]]), f"slot {b}"
        assert not got[b, nq[b]:].any(), f"slot {b} rows beyond n_q"
    idle = pos.clone()
    idle[1] = -1
    got = verify_attention_paged(q, kp, vp, table, idle, n_q, SCALE)
    assert not got[1].any()
    for b in (0, 2, 3):
        assert torch.equal(got[b, :nq[b]], out[b, :nq[b]]), f"slot {b}"


@pytest.mark.parametrize("H,n_kv,T", [(8, 2, 5), (8, 1, 8), (8, 8, 1)])
def test_verify_reads_only_valid_rows(H, n_kv, T):
    """The kernel is NaN-safe: NaN in every page outside the table and in
    every row beyond pos[b]+n_q[b]-1 of the owned pages changes no bit."""
    q, kp, vp, table, pos, _, out, _ = _case(H, n_kv, T)
    nq = [min(n, T) for n in (1, 3, T, 2)]
    n_q = torch.tensor(nq, dtype=torch.int32, device=DEV)
    clean = verify_attention_paged(q, kp, vp, table, pos, n_q, SCALE)
    keep = torch.zeros(N_PAGES, R, dtype=torch.bool, device=DEV)
    for b in range(B):
        rows = torch.arange(MAX_PAGES * R, device=DEV) <= POS[b] + nq[b] - 1
        keep[table[b].long()] = rows.reshape(MAX_PAGES, R)
    nan = torch.full_like(kp, float("nan"))
    kd = torch.where(keep[:, None, :, None], kp, nan)
    vd = torch.where(keep[:, None, :, None], vp, nan)
    got = verify_attention_paged(q, kd, vd, table, pos, n_q, SCALE)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, clean)
    for b in range(B):
        assert torch.equal(clean[b, :nq[b]], out[b, :nq[b]])


@torch.no_grad()
def test_verify_paged_matches_teacher_forced_steps():
    """llama-smoke (head_dim 128), slots at 61 and 130 rows plus an idle one:
    one 5-token verify forward against 5 decode steps fed the same tokens,
    across the row-64 page boundary."""
    native.load(require=True)
    torch.manual_seed(5)
    cfg = CONFIGS["llama-smoke"]
    model = build_inference_model(cfg, torch.device(DEV))
    lengths, T = [61, 130], 5
    gen = torch.Generator().manual_seed(17)
    caches = [PagedKVCache(cfg, 8, 3, 4, torch.device(DEV), torch.bfloat16)
              for _ in range(2)]
    for s, n in enumerate(lengths):
        prompt = torch.randint(0, cfg.vocab_size, (1, n), generator=gen).to(DEV)
        tmp = KVCache(cfg, 1, n, torch.device(DEV), torch.bfloat16)
        _forward_cached(model, prompt, tmp)
        for c in caches:
            assert c.admit(s, n + T)
            c.load_prefix(s, [k[0] for k in tmp.k], [v[0] for v in tmp.v], n)
    toks = torch.randint(0, cfg.vocab_size, (3, T), generator=gen).to(DEV)
    steps, spec = caches
    ref = []
    for i in range(T):
        for s in range(2):
            steps.ensure_row(s, steps.host_pos[s])
        ref.append(_step_paged(model, toks[:, i:i + 1], steps).float())
        steps.advance()
    for s, n in enumerate(lengths):
        spec.ensure_row(s, n + T - 1)
    n_q = torch.full((3,), T, dtype=torch.int32, device=DEV)
    got = _verify_paged(model, toks, spec, n_q).float()
    assert spec.pos.tolist() == lengths + [-1]
    spec.check_block_table()
    assert torch.isfinite(got).all()
    for i in range(T):
        for s in range(2):
            err = (got[s, i] - ref[i][s]).abs().max().item()
            bound = 2e-2 * ref[i][s].abs().max().item() + 2e-2
            print(f"len {lengths[s]} token {i}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (s, i, err, bound)
