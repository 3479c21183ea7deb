"""Paged decode kernels (attn_decode_paged, rope_cache_paged; head_dim
128 for attention) against the contiguous kernels bit for bit and against
the fp32 torch references."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.ops import (  # noqa: E402
    decode_attention, decode_attention_paged, make_inv_freq, native,
    reference, rope_cache_paged,
)

DEV = "cuda:0"
D = 128
R = 64                       # rows per page
MAX_PAGES = 5
N_PAGES = 32
POS = [0, 63, 64, 200]       # first row, last row of a page, first row of
#                              the second page, mid fourth page
SCALE = 1.0 / math.sqrt(D)


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    native.load(require=True)


def _mk(shape, gen, scale=1.0):
    x = torch.randn(*shape, dtype=torch.float32, generator=gen) * scale
    return x.to(torch.bfloat16).to(DEV)


def _case(H, n_kv, seed=31, B=4):
    """Random pools, q and a table of distinct, permuted pages."""
    gen = torch.Generator().manual_seed(seed)
    q = _mk((B, H, 1, D), gen)
    kp = _mk((N_PAGES, n_kv, R, D), gen)
    vp = _mk((N_PAGES, n_kv, R, D), gen)
    perm = torch.randperm(N_PAGES, generator=gen)[:B * MAX_PAGES]
    table = perm.reshape(B, MAX_PAGES).to(torch.int32).to(DEV)
    pos = torch.tensor(POS[:B], dtype=torch.int64, device=DEV)
    return q, kp, vp, table, pos


def _contig(pool, table_row):
    """One slot's pages as a contiguous [1, n_kv, MAX_PAGES*64, D] cache."""
    g = pool[table_row.long()]                    # [MAX_PAGES, n_kv, R, D]
    return g.permute(1, 0, 2, 3).reshape(
        1, pool.shape[1], MAX_PAGES * R, D).contiguous()


def _fp32_masked_softmax(q, kc, vc, pos):
    """q [1,H,1,D], caches [1,n_kv,L,D]: attention over rows 0..pos."""
    H, n_kv = q.shape[1], kc.shape[1]
    qg = q.float().reshape(1, n_kv, H // n_kv, D)
    s = torch.einsum("bkgd,bksd->bkgs", qg, kc.float()) / math.sqrt(D)
    s[..., pos + 1:] = float("-inf")
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bkgs,bksd->bkgd", p, vc.float()).reshape(1, H, 1, D)


@pytest.mark.parametrize("H,n_kv", [(8, 2), (8, 8), (8, 1)])
def test_paged_attention_bit_identical_to_contiguous(H, n_kv):
    """A page-permuted cache gives the bits of attn_decode on the gathered
    contiguous cache, slot by slot, and both sit within the fp32 bound of
    test_decode_attention_matches_fp32."""
    q, kp, vp, table, pos = _case(H, n_kv)
    o = decode_attention_paged(q, kp, vp, table, pos, SCALE)
    assert o is not None and o.shape == (4, H, 1, D)
    for b, p in enumerate(POS):
        kc, vc = _contig(kp, table[b]), _contig(vp, table[b])
        pos_t = torch.full((1,), p, dtype=torch.int64, device=DEV)
        ref = decode_attention(q[b:b + 1], kc, vc, pos_t, SCALE)
        assert ref is not None
        assert torch.equal(o[b:b + 1], ref), f"slot {b} pos {p}"
        f32 = _fp32_masked_softmax(q[b:b + 1], kc, vc, p)
        err = (o[b:b + 1].float() - f32).abs().max().item()
        assert err < 2e-2, f"slot {b} pos {p}: {err}"
    tw = reference.decode_attention_paged(q, kp, vp, table, pos, SCALE)
    assert (o.float() - tw.float()).abs().max().item() < 2e-2


def test_paged_attention_reads_only_valid_rows():
    """NaN in every page outside the table and in every row beyond pos[b]
    of the owned pages: output finite and equal to the clean run."""
    q, kp, vp, table, pos = _case(8, 2, seed=37)
    clean = decode_attention_paged(q, kp, vp, table, pos, SCALE)
    kn, vn = kp.clone(), vp.clone()
    owned = torch.zeros(N_PAGES, dtype=torch.bool, device=DEV)
    owned[table.long().reshape(-1)] = True
    kn[~owned] = float("nan")
    vn[~owned] = float("nan")
    for b, p in enumerate(POS):
        for j in range(MAX_PAGES):
            first = max(0, p + 1 - j * R)         # first invalid row in page
            if first < R:
                page = int(table[b, j])
                kn[page, :, first:] = float("nan")
                vn[page, :, first:] = float("nan")
    got = decode_attention_paged(q, kn, vn, table, pos, SCALE)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, clean)
    tw = reference.decode_attention_paged(q, kn, vn, table, pos, SCALE)
    assert torch.isfinite(tw.float()).all()


def test_idle_slot_is_zero_and_writes_nothing():
    """pos[1] = -1: attention row exactly zero, rope_cache_paged leaves
    both pools as they were and zeros q; other slots unaffected."""
    q, kp, vp, table, pos = _case(8, 2, seed=41)
    full = decode_attention_paged(q, kp, vp, table, pos, SCALE)
    idle = pos.clone()
    idle[1] = -1
    o = decode_attention_paged(q, kp, vp, table, idle, SCALE)
    assert (o[1] == 0).all()
    for b in (0, 2, 3):
        assert torch.equal(o[b], full[b])

    gen = torch.Generator().manual_seed(43)
    nh, nkv = 8, 2
    inv_freq = make_inv_freq(D, 500000.0, device=DEV)
    qkv = _mk((4, (nh + 2 * nkv) * D), gen)
    all_idle = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    k0, v0 = kp.clone(), vp.clone()
    qo = rope_cache_paged(qkv, kp, vp, inv_freq, table, all_idle, nh, nkv)
    assert torch.equal(kp, k0) and torch.equal(vp, v0)
    assert (qo == 0).all()
    # one idle slot among active ones: its pages untouched, others written
    ka, va = kp.clone(), vp.clone()
    qa = rope_cache_paged(qkv, ka, va, inv_freq, table, pos, nh, nkv)
    kb, vb = kp.clone(), vp.clone()
    qb = rope_cache_paged(qkv, kb, vb, inv_freq, table, idle, nh, nkv)
    assert (qb[1] == 0).all()
    for b in (0, 2, 3):
        assert torch.equal(qb[b], qa[b])
    page1 = int(table[1, POS[1] // R])
    assert torch.equal(kb[page1], kp[page1])
    assert torch.equal(vb[page1], vp[page1])
    rest = torch.ones(N_PAGES, dtype=torch.bool, device=DEV)
    rest[page1] = False
    assert torch.equal(kb[rest], ka[rest]) and torch.equal(vb[rest], va[rest])


@pytest.mark.parametrize("Dh", [128, 64])
def test_rope_cache_paged_matches_reference(Dh):
    """q and the written k row within 2e-2 of the torch Neox rotation, v
    row exact, every other row of both pools untouched, and for equal
    positions the bits of rope_cache on a contiguous cache."""
    gen = torch.Generator().manual_seed(47 + Dh)
    B, nh, nkv = 3, 8, 2
    positions = [37, 63, 64]
    inv_freq = make_inv_freq(Dh, 10000.0, device=DEV)
    qkv = _mk((B, (nh + 2 * nkv) * Dh), gen)
    kp = _mk((N_PAGES, nkv, R, Dh), gen)
    vp = _mk((N_PAGES, nkv, R, Dh), gen)
    k0, v0 = kp.clone(), vp.clone()
    perm = torch.randperm(N_PAGES, generator=gen)[:B * MAX_PAGES]
    table = perm.reshape(B, MAX_PAGES).to(torch.int32).to(DEV)
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    q = rope_cache_paged(qkv, kp, vp, inv_freq, table, pos, nh, nkv)
    torch.cuda.synchronize()

    f = qkv.float().reshape(B, nh + 2 * nkv, Dh)
    half = Dh // 2
    written = torch.zeros(N_PAGES, R, dtype=torch.bool, device=DEV)
    for b, p in enumerate(positions):
        ang = p * inv_freq.float()
        c, s = ang.cos(), ang.sin()

        def rope_ref(x):
            x1, x2 = x[..., :half], x[..., half:]
            return torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1)

        page, row = int(table[b, p // R]), p % R
        written[page, row] = True
        assert (q[b].float() - rope_ref(f[b, :nh])).abs().max() < 2e-2
        assert (kp[page, :, row].float()
                - rope_ref(f[b, nh:nh + nkv])).abs().max() < 2e-2
        assert torch.equal(vp[page, :, row].float(), f[b, nh + nkv:])
    keep = ~written[:, None, :, None].expand_as(kp)
    assert torch.equal(kp[keep], k0[keep])
    assert torch.equal(vp[keep], v0[keep])

    # the torch twin does the same work
    kt, vt = k0.clone(), v0.clone()
    qt = reference.rope_cache_paged(qkv, kt, vt, inv_freq, table, pos, nh,
                                    nkv)
    assert (qt.float() - q.float()).abs().max() < 2e-2
    assert (kt.float() - kp.float()).abs().max() < 2e-2
    assert torch.equal(vt, vp)

    # equal positions: the contiguous kernel's bits
    lib = native.load(require=True)
    for p in positions:
        same = torch.full((B,), p, dtype=torch.int64, device=DEV)
        kq, vq = k0.clone(), v0.clone()
        qp = rope_cache_paged(qkv, kq, vq, inv_freq, table, same, nh, nkv)
        Lmax = MAX_PAGES * R
        kc = torch.zeros(B, nkv, Lmax, Dh, dtype=torch.bfloat16, device=DEV)
        vc = torch.zeros_like(kc)
        qc = torch.empty(B, nh, Dh, dtype=torch.bfloat16, device=DEV)
        pos_t = torch.full((1,), p, dtype=torch.int64, device=DEV)
        rc = lib.rope_cache(native.stream_ptr(), qkv.data_ptr(),
                            qc.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                            inv_freq.data_ptr(), pos_t.data_ptr(), B, nh,
                            nkv, Lmax, Dh)
        native.check_rc(rc, "rope_cache", "test")
        assert torch.equal(qp, qc)
        for b in range(B):
            page = int(table[b, p // R])
            assert torch.equal(kq[page, :, p % R], kc[b, :, p])
            assert torch.equal(vq[page, :, p % R], vc[b, :, p])


def test_paged_launchers_refuse_unsupported_arguments():
    """The wrappers keep decode_attention's contract: None off the
    supported shapes, never a launch."""
    q, kp, vp, table, pos = _case(8, 2)
    assert decode_attention_paged(q, kp, vp, table.long(), pos, SCALE) is None
    assert decode_attention_paged(q[:, :7], kp, vp, table, pos, SCALE) is None
    assert decode_attention_paged(q[..., :64].contiguous(),
                                  kp[..., :64].contiguous(),
                                  vp[..., :64].contiguous(), table, pos,
                                  SCALE) is None
    lib = native.load(require=True)
    assert lib.attn_decode_paged(None, None, None, None, None, None, None,
                                 None, 4, 8, 3, N_PAGES, MAX_PAGES,
                                 SCALE) == -1
    assert lib.rope_cache_paged(None, None, None, None, None, None, None,
                                None, 4, 8, 2, N_PAGES, MAX_PAGES, 24) == -1
