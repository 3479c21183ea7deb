"""Pair ownership of the causal unsplit dv/dk workgroups, on the host.

With AITJ_ATTN_BWD_FOLD=2 workgroup rank runs two phases, half-block rank
(128 kv rows, heavy) and then half-block 2n-1-rank (light), and in each the
waves w and w+4 share the 32-row strip w of the half-block: wave role
wid >> 2 computes that 32-row sub of every q tile, accumulates two of the
four d subtiles, and reads the other sub's fragments from its partner.
attn_bwd_pair says who does what and is exported as attn_bwd_pair_decode.
dk and dv are allocated with torch.empty, so a strip (or a d subtile of one)
nobody owns could read back stale but correct on the GPU: that every one has
exactly one owner is checked here."""
import ctypes

import pytest

from trainingjob_operator_amd.ops import native

pytestmark = pytest.mark.skipif(
    not native.available(), reason="libhipops.so not built")

ROW_BLOCKS = [1, 2, 3, 8, 16, 17]
WAVES = 8
FIELDS = ("kv0w", "qt0", "sub", "ds0", "ds1", "peer")


def _decode(rank, phase, wid, n):
    lib = native.load(require=True)
    out = [ctypes.c_int() for _ in FIELDS]
    rc = lib.attn_bwd_pair_decode(rank, phase, wid, n,
                                  *[ctypes.byref(o) for o in out])
    assert rc == 0, (rank, phase, wid, n)
    return dict(zip(FIELDS, (o.value for o in out)))


def _pairs(n):
    """{(rank, phase): [decode of each wave]}"""
    return {(rank, phase): [_decode(rank, phase, wid, n)
                            for wid in range(WAVES)]
            for rank in range(n) for phase in (0, 1)}


def _first_tile(kv0w):
    """First 64-row q tile the kernels' `qt * 64 + 63 >= kv0w` lets in."""
    return kv0w // 64


@pytest.mark.parametrize("n", ROW_BLOCKS)
def test_every_strip_has_one_rank_phase_and_wave_pair(n):
    owners = {}
    for (rank, phase), waves in _pairs(n).items():
        for wid, w in enumerate(waves):
            owners.setdefault(w["kv0w"], []).append((rank, phase, wid))
    assert sorted(owners) == [32 * s for s in range(8 * n)]
    for kv0w, who in owners.items():
        assert len(who) == 2, (n, kv0w, who)
        (r0, p0, w0), (r1, p1, w1) = sorted(who)
        assert (r0, p0) == (r1, p1) and w1 == w0 + 4, (n, kv0w, who)


@pytest.mark.parametrize("n", ROW_BLOCKS)
def test_partners_split_the_subs_and_the_d_subtiles(n):
    for (rank, phase), waves in _pairs(n).items():
        for w in range(4):
            a, b = waves[w], waves[w + 4]
            assert a["kv0w"] == b["kv0w"] and a["qt0"] == b["qt0"]
            assert {a["sub"], b["sub"]} == {0, 1}
            da = set(range(a["ds0"], a["ds1"]))
            db = set(range(b["ds0"], b["ds1"]))
            assert not (da & db) and da | db == {0, 1, 2, 3}
            assert a["peer"] == w + 4 and b["peer"] == w
            # the wave that computes sub r owns chunks 2r, 2r+1 and
            # accumulates d subtiles 2r, 2r+1
            for x in (a, b):
                assert (x["ds0"], x["ds1"]) == (2 * x["sub"],
                                                2 * x["sub"] + 2)


@pytest.mark.parametrize("n", ROW_BLOCKS)
def test_first_q_tile_is_the_half_blocks_own(n):
    for (rank, phase), waves in _pairs(n).items():
        hb = rank if phase == 0 else 2 * n - 1 - rank
        assert [w["kv0w"] for w in waves[:4]] == \
            [hb * 128 + s * 32 for s in range(4)]
        qt0s = {w["qt0"] for w in waves}
        assert qt0s == {2 * hb}, (n, rank, phase)
        assert 2 * hb == min(_first_tile(w["kv0w"]) for w in waves)
        assert 0 <= 2 * hb < 4 * n


@pytest.mark.parametrize("n", ROW_BLOCKS)
def test_every_workgroup_walks_the_same_tile_steps(n):
    pairs = _pairs(n)
    for rank in range(n):
        steps = sum(4 * n - pairs[(rank, phase)][0]["qt0"]
                    for phase in (0, 1))
        assert steps == 4 * n + 2, (n, rank, steps)


@pytest.mark.parametrize("n", ROW_BLOCKS)
def test_the_two_half_blocks_of_a_rank_are_distinct(n):
    pairs = _pairs(n)
    for rank in range(n):
        heavy = pairs[(rank, 0)][0]["kv0w"]
        light = pairs[(rank, 1)][0]["kv0w"]
        assert heavy < light, (n, rank)              # heavy phase first
        assert heavy // 128 + light // 128 == 2 * n - 1


def test_out_of_range_arguments_are_refused():
    lib = native.load(require=True)
    x = ctypes.c_int()
    p = [ctypes.byref(x)] * 6
    assert lib.attn_bwd_pair_decode(0, 0, 0, 16, *p) == 0
    assert lib.attn_bwd_pair_decode(15, 1, 7, 16, *p) == 0
    assert lib.attn_bwd_pair_decode(16, 0, 0, 16, *p) != 0
    assert lib.attn_bwd_pair_decode(-1, 0, 0, 16, *p) != 0
    assert lib.attn_bwd_pair_decode(0, 2, 0, 16, *p) != 0
    assert lib.attn_bwd_pair_decode(0, -1, 0, 16, *p) != 0
    assert lib.attn_bwd_pair_decode(0, 0, 8, 16, *p) != 0
    assert lib.attn_bwd_pair_decode(0, 0, -1, 16, *p) != 0
    assert lib.attn_bwd_pair_decode(0, 0, 0, 0, *p) != 0


def test_the_knob_pairs_only_causal_unsplit_launches(monkeypatch):
    """AITJ_ATTN_BWD_FOLD=2 selects the pair kernels for a causal unsplit
    launch of any size; split and non-causal launches never pair, and 0 and
    1 keep their meaning."""
    lib = native.load(require=True)
    IDENTITY, FOLD, PAIR = 0, 1, 2
    shapes = [(1, 2, 2, 256), (2, 32, 8, 4096), (8, 32, 8, 4096)]
    for kernel in (0, 1):
        for B, H, HKV, S in shapes:
            monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", "2")
            assert lib.attn_bwd_fold_mode(B, H, HKV, S, 1, 0, kernel) == PAIR
            assert lib.attn_bwd_fold_mode(B, H, HKV, S, 1, 1, kernel) != PAIR
            assert lib.attn_bwd_fold_mode(B, H, HKV, S, 0, 0, kernel) == \
                IDENTITY
            monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", "0")
            assert lib.attn_bwd_fold_mode(B, H, HKV, S, 1, 0, kernel) == \
                IDENTITY
            monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", "1")
            assert lib.attn_bwd_fold_mode(B, H, HKV, S, 1, 0, kernel) == FOLD
            assert lib.attn_bwd_fold_mode(B, H, HKV, S, 1, 1, kernel) == FOLD
            monkeypatch.delenv("AITJ_ATTN_BWD_FOLD")
            # unset: split launches never pair either
            assert lib.attn_bwd_fold_mode(B, H, HKV, S, 1, 1, kernel) != PAIR
            assert lib.attn_bwd_fold_mode(B, H, HKV, S, 0, 0, kernel) == \
                IDENTITY
