"""Block-id decode of the scheduled attention kernels, on the host.

The v7 forward and the dq/dv/dk kernels launch a 1-D grid and decode the
block id to (row block rank, head, batch) with attn_sched_block; the same
function is exported as attn_sched_decode. The ops allocate their outputs
with torch.empty, so a tile no workgroup owns can read back a stale but
correct value on the GPU: that every tile has exactly one owner is checked
here, where it cannot hide.

rank 0 is the heaviest row block under the causal mask: a block of rank r
walks n_row_blocks - r units. Observed placement deals blocks round-robin
over 8 XCDs, so id % 8 labels the blocks that share one."""
import ctypes
from collections import Counter, defaultdict

import pytest

from trainingjob_operator_amd.ops import native

pytestmark = pytest.mark.skipif(
    not native.available(), reason="libhipops.so not built")

LEGACY, BALANCED = 0, 1
ROW_BLOCKS = [1, 2, 3, 8, 16, 17]
HEADS = [(1, 1), (2, 2), (4, 1), (6, 2), (32, 8)]
BATCHES = [1, 2, 3, 5]


def _decode_all(sched, n, H, B):
    lib = native.load(require=True)
    r, h, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    out = []
    for i in range(n * H * B):
        rc = lib.attn_sched_decode(sched, i, n, H, B, ctypes.byref(r),
                                   ctypes.byref(h), ctypes.byref(b))
        assert rc == 0, (sched, i, n, H, B)
        out.append((r.value, h.value, b.value))
    return out


@pytest.mark.parametrize("sched", [LEGACY, BALANCED])
@pytest.mark.parametrize("H,HKV", HEADS)
def test_decode_is_a_bijection(sched, H, HKV):
    """Every (row block, head, batch) is hit exactly once, for q-head grids
    (fwd, dq, split dv/dk) and kv-head grids (unsplit dv/dk) alike."""
    for heads in {H, HKV}:
        for n in ROW_BLOCKS:
            for B in BATCHES:
                got = _decode_all(sched, n, heads, B)
                want = {(r, h, b) for r in range(n) for h in range(heads)
                        for b in range(B)}
                assert len(got) == len(want) and set(got) == want, \
                    (sched, n, heads, B)


def test_legacy_is_the_former_3d_grid():
    """legacy = grid(n, heads, batch) read x-fastest, rank = blockIdx.x."""
    n, H, B = 3, 6, 2
    got = _decode_all(LEGACY, n, H, B)
    assert got == [(x, y, z) for z in range(B) for y in range(H)
                   for x in range(n)]


@pytest.mark.parametrize("H,HKV", HEADS)
def test_balanced_is_heavy_first_in_every_class(H, HKV):
    """Work (n - rank) never increases along one id % 8 class."""
    for heads in {H, HKV}:
        for n in ROW_BLOCKS:
            for B in BATCHES:
                got = _decode_all(BALANCED, n, heads, B)
                for c in range(8):
                    work = [n - r for (r, _, _) in got[c::8]]
                    assert work == sorted(work, reverse=True), \
                        (n, heads, B, c)


def test_out_of_range_ids_are_refused():
    lib = native.load(require=True)
    x = ctypes.c_int()
    p = ctypes.byref(x)
    assert lib.attn_sched_decode(BALANCED, 16 * 32 * 2, 16, 32, 2, p, p, p) != 0
    assert lib.attn_sched_decode(BALANCED, -1, 16, 32, 2, p, p, p) != 0
    assert lib.attn_sched_decode(2, 0, 16, 32, 2, p, p, p) != 0
    assert lib.attn_sched_decode(LEGACY, 0, 0, 32, 2, p, p, p) != 0


def test_flagship_classes_are_equal_and_keep_kv_heads_together():
    """B=2, H=32, HKV=8, S=4096 (16 row blocks): the eight classes carry
    the same work, and all blocks that read one kv head's K/V sit in one
    class. The legacy order has neither property."""
    n, H, HKV, B = 16, 32, 8, 2
    group = H // HKV
    got = _decode_all(BALANCED, n, H, B)
    totals = Counter()
    ranks = defaultdict(Counter)
    classes_of = defaultdict(set)
    for i, (r, h, b) in enumerate(got):
        totals[i % 8] += n - r
        ranks[i % 8][r] += 1
        classes_of[(b, h // group)].add(i % 8)
    assert len(set(totals.values())) == 1 and len(totals) == 8, totals
    assert all(ranks[c] == ranks[0] for c in range(8))     # same multiset
    assert len(classes_of) == HKV * B
    assert all(len(c) == 1 for c in classes_of.values()), classes_of

    # unsplit dv/dk grid: kv heads are the heads
    got = _decode_all(BALANCED, n, HKV, B)
    totals = Counter()
    for i, (r, _, _) in enumerate(got):
        totals[i % 8] += n - r
    assert len(set(totals.values())) == 1 and len(totals) == 8, totals

    legacy = Counter()
    for i, (r, _, _) in enumerate(_decode_all(LEGACY, n, H, B)):
        legacy[i % 8] += n - r
    assert max(legacy.values()) > min(legacy.values())


def test_ws_bytes_follows_the_split_knob(monkeypatch):
    """Host-only sizing: 0 on the unsplit path, two [B,H,S,128] fp32
    arrays on the split one; unset is unsplit; auto splits the flagship
    shape, not MHA and not a grid with 2 workgroups per CU."""
    lib = native.load(require=True)
    full = 2 * 2 * 32 * 4096 * 128 * 4
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "0")
    assert lib.attn_bwd_ws_bytes(2, 32, 8, 4096, 1) == 0
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "1")
    assert lib.attn_bwd_ws_bytes(2, 32, 8, 4096, 1) == full
    assert lib.attn_bwd_ws_bytes(2, 32, 8, 4000, 1) == 0     # refused shape
    monkeypatch.delenv("AITJ_ATTN_BWD_SPLIT")
    assert lib.attn_bwd_ws_bytes(2, 32, 8, 4096, 1) == 0
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "auto")
    assert lib.attn_bwd_ws_bytes(2, 32, 8, 4096, 1) == full
    assert lib.attn_bwd_ws_bytes(2, 32, 8, 4096, 0) == 0     # 1 per CU
    assert lib.attn_bwd_ws_bytes(1, 32, 8, 4096, 0) == full // 2
    assert lib.attn_bwd_ws_bytes(4, 32, 8, 4096, 1) == 0     # 2 per CU
    assert lib.attn_bwd_ws_bytes(2, 32, 32, 4096, 1) == 0
