"""Document-masked attention off the GPU: the layout helpers of
ops/docmask.py, the fp32 reference twins, the SDPA fallback of
packed_rope_attention, the model plumbing, and the host twin of the kernels'
clamped tile ranges."""
import ctypes
import math

import pytest
import torch

from trainingjob_operator_amd.ops import native
from trainingjob_operator_amd.ops.docmask import (
    check_doc_bounds, doc_bounds_from_eos, doc_bounds_from_lengths,
    doc_mask_dense,
)

EOS = 7


def _loop_bounds(tokens, eos):
    """The definition, one token at a time."""
    B, S = tokens.shape
    out = torch.zeros(2, B, S, dtype=torch.int32)
    for b in range(B):
        row = tokens[b].tolist()
        at = 0
        for s in range(S):
            out[0, b, s] = at
            if row[s] == eos:
                at = s + 1
        nxt = S - 1
        for s in range(S - 1, -1, -1):
            if row[s] == eos:
                nxt = s
            out[1, b, s] = nxt
    return out


def _tokens(S, eos_at):
    t = torch.full((S,), 3, dtype=torch.int64)
    for i in eos_at:
        t[i] = EOS
    return t


@pytest.mark.parametrize("eos_at", [
    [0], [15], [5, 6], [], [0, 15], [3, 4, 5, 9]],
    ids=["first", "last", "two-in-a-row", "none", "both-ends", "run"])
def test_bounds_from_eos_matches_loop(eos_at):
    tokens = _tokens(16, eos_at)[None]
    got = doc_bounds_from_eos(tokens, EOS)
    assert got.dtype == torch.int32 and got.shape == (2, 1, 16)
    assert got.is_contiguous()
    assert torch.equal(got, _loop_bounds(tokens, EOS))
    check_doc_bounds(got)


def test_bounds_from_eos_two_in_a_row_is_a_one_token_document():
    got = doc_bounds_from_eos(_tokens(16, [5, 6])[None], EOS)
    assert got[0, 0, 6] == 6 and got[1, 0, 6] == 6
    assert got[0, 0, 7] == 7 and got[1, 0, 7] == 15


def test_bounds_from_eos_differing_batch_rows():
    g = torch.Generator().manual_seed(0)
    tokens = torch.randint(0, 12, (4, 64), generator=g)
    tokens[2] = 3                                     # a row with no eos
    got = doc_bounds_from_eos(tokens, EOS)
    assert torch.equal(got, _loop_bounds(tokens, EOS))
    assert not torch.equal(got[:, 0], got[:, 1])
    check_doc_bounds(got)


def test_bounds_from_lengths_round_trip():
    lengths = [[1, 63, 64, 65, 300, 19], [37, 475]]
    b = doc_bounds_from_lengths(lengths)
    assert b.dtype == torch.int32 and b.shape == (2, 2, 512)
    check_doc_bounds(b)
    for row, lens in enumerate(lengths):
        starts = torch.unique_consecutive(b[0, row]).tolist()
        ends = torch.unique_consecutive(b[1, row]).tolist()
        assert [e - s + 1 for s, e in zip(starts, ends)] == lens
    # and through tokens: an eos at every document end gives the same
    tokens = torch.full((2, 512), 3)
    tokens.scatter_(1, b[1].long(), EOS)
    assert torch.equal(doc_bounds_from_eos(tokens, EOS), b)
    with pytest.raises(AssertionError):
        doc_bounds_from_lengths([[256, 256], [256, 255]])


def test_check_doc_bounds_rejects_a_non_partition():
    good = doc_bounds_from_lengths([[8, 24]])
    check_doc_bounds(good)
    for s, which, val in [(3, 0, 2),      # start inside another document
                          (3, 1, 20),     # end past its document
                          (10, 0, 9),     # a start that is not a boundary
                          (31, 1, 32),    # end outside the window
                          (0, 0, -1)]:
        bad = good.clone()
        bad[which, 0, s] = val
        with pytest.raises(AssertionError):
            check_doc_bounds(bad)
    with pytest.raises(AssertionError):
        check_doc_bounds(good.long())


def test_mask_dense_is_the_definition():
    S = 64
    b = doc_bounds_from_lengths([[1, 20, 43], [64]])
    m = doc_mask_dense(b)
    assert m.dtype == torch.bool and m.shape == (2, 1, S, S)
    for bi in range(2):
        for q in range(S):
            for kv in range(S):
                want = int(b[0, bi, q]) <= kv <= q
                assert bool(m[bi, 0, q, kv]) == want
                # the kv-side form of the same predicate
                assert want == (kv <= q <= int(b[1, bi, kv]))


def _rand_qkv(B, H, HKV, S, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, S, D, generator=g),
            torch.randn(B, HKV, S, D, generator=g),
            torch.randn(B, HKV, S, D, generator=g),
            torch.randn(B, H, S, D, generator=g))


def test_reference_twin_matches_sdpa_with_dense_mask():
    from trainingjob_operator_amd.ops.reference import (
        attention_delta, attention_doc_bwd, attention_doc_fwd,
    )
    B, H, HKV, S, D = 2, 4, 2, 48, 16
    q, k, v, gout = _rand_qkv(B, H, HKV, S, D)
    b = doc_bounds_from_lengths([[5, 1, 42], [30, 18]])
    o, lse = attention_doc_fwd(q, k, v, b)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(
        qa, ka, va, attn_mask=doc_mask_dense(b), enable_gqa=True)
    torch.testing.assert_close(o, ref, atol=1e-5, rtol=1e-5)
    # lse against logsumexp over the allowed keys
    s = (q[1, 3] @ k[1, 1].T) / math.sqrt(D)
    s = s.masked_fill(~doc_mask_dense(b)[1, 0], float("-inf"))
    torch.testing.assert_close(lse[1, 3], torch.logsumexp(s, -1),
                               atol=1e-5, rtol=1e-5)
    (ref * gout).sum().backward()
    dq, dk, dv = attention_doc_bwd(q, k, v, gout, lse,
                                   attention_delta(o, gout), b)
    torch.testing.assert_close(dq, qa.grad, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(dk, ka.grad, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(dv, va.grad, atol=1e-4, rtol=1e-4)


def _packed(B, S, H, HKV, D, seed=1):
    from trainingjob_operator_amd.ops import make_inv_freq
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, (H + 2 * HKV) * D, generator=g)
    return qkv, make_inv_freq(D, 10000.0)


def test_fallback_is_per_document_causal_attention():
    """Each document's rows equal a causal call on that document alone,
    although RoPE ran at window positions: RoPE is relative."""
    from trainingjob_operator_amd.ops.attention import packed_rope_attention
    B, S, H, HKV, D = 2, 48, 4, 2, 16
    lengths = [[5, 1, 42], [30, 18]]
    qkv, inv_freq = _packed(B, S, H, HKV, D)
    b = doc_bounds_from_lengths(lengths)
    o = packed_rope_attention(qkv, inv_freq, H, HKV, doc_bounds=b)
    assert o.shape == (B, S, H * D)
    for bi, lens in enumerate(lengths):
        at = 0
        for n in lens:
            alone = packed_rope_attention(qkv[bi:bi + 1, at:at + n].clone(),
                                          inv_freq, H, HKV)
            torch.testing.assert_close(o[bi:bi + 1, at:at + n], alone,
                                       atol=2e-5, rtol=1e-5)
            at += n


def test_fallback_single_document_is_the_call_without_bounds():
    from trainingjob_operator_amd.ops.attention import packed_rope_attention
    B, S, H, HKV, D = 2, 48, 4, 2, 16
    qkv, inv_freq = _packed(B, S, H, HKV, D)
    b = doc_bounds_from_lengths([[S]] * B)
    torch.testing.assert_close(
        packed_rope_attention(qkv, inv_freq, H, HKV, doc_bounds=b),
        packed_rope_attention(qkv, inv_freq, H, HKV), atol=1e-6, rtol=1e-6)


def test_llama_model_takes_document_bounds():
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.llama import LlamaModel
    torch.manual_seed(0)
    model = LlamaModel(CONFIGS["llama-tiny"]).eval()
    B, S = 2, 32
    g = torch.Generator().manual_seed(2)
    tokens = torch.randint(0, 512, (B, S), generator=g)
    targets = torch.randint(0, 512, (B, S), generator=g)
    b = doc_bounds_from_lengths([[16, 16]] * B)
    with torch.no_grad():
        assert float(model(tokens, targets, b)) != float(model(tokens,
                                                                targets))
        logits = model(tokens, doc_bounds=b)
        other = tokens.clone()
        other[:, 16:] = torch.randint(0, 512, (B, 16), generator=g)
        torch.testing.assert_close(model(other, doc_bounds=b)[:, :16],
                                   logits[:, :16], atol=0, rtol=0)
        # the direction plain causal attention does not give: document 1
        # does not see document 0
        other = tokens.clone()
        other[:, :16] = torch.randint(0, 512, (B, 16), generator=g)
        torch.testing.assert_close(model(other, doc_bounds=b)[:, 16:],
                                   logits[:, 16:], atol=1e-6, rtol=1e-6)
        assert not torch.allclose(model(other)[:, 16:],
                                  model(tokens)[:, 16:], atol=1e-3)
    # through activation checkpointing too
    ck = LlamaModel(CONFIGS["llama-tiny"], checkpoint_activations=True)
    ck.load_state_dict(model.state_dict())
    ck.train()
    loss = ck(tokens, targets, b)
    loss.backward()
    with torch.no_grad():
        torch.testing.assert_close(loss, model(tokens, targets, b),
                                   atol=1e-6, rtol=1e-6)


def test_moe_model_refuses_document_bounds():
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.moe_llama import MoELlamaModel
    model = MoELlamaModel(CONFIGS["moe-tiny"])
    tokens = torch.zeros(1, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="doc"):
        model(tokens, doc_bounds=doc_bounds_from_lengths([[8, 8]]))


# --- host twin of the kernels' clamped tile ranges --------------------------

needs_lib = pytest.mark.skipif(not native.available(),
                               reason="libhipops.so not built")
FWD, BWD = 0, 1
INT_MAX = 2 ** 31 - 1


def _tiles(kind, value, block, S):
    lib = native.load(require=True)
    first, last = ctypes.c_int(), ctypes.c_int()
    rc = lib.attn_doc_tiles_decode(kind, value, block, S,
                                   ctypes.byref(first), ctypes.byref(last))
    assert rc == 0, (kind, value, block, S)
    return first.value, last.value


@needs_lib
@pytest.mark.parametrize("S", [256, 768, 4096])
def test_tile_ranges_for_valid_bounds(S):
    """fwd/dq: from the tile of the block's first start to the block's last
    (diagonal) tile; dv/dk: from the block's first tile to the tile of its
    last end."""
    for blk in range(S // 256):
        diag_q, diag_kv = blk * 4 + 3, blk * 4
        for start in {0, 1, 63, 64, 65, blk * 256 - 1, blk * 256}:
            if 0 <= start <= blk * 256:
                assert _tiles(FWD, start, blk, S) == (start // 64, diag_q)
        for end in {blk * 256 + 255, blk * 256 + 256, blk * 256 + 319,
                    S - 65, S - 64, S - 1}:
            if blk * 256 + 255 <= end < S:
                assert _tiles(BWD, end, blk, S) == (diag_kv, end // 64)


@needs_lib
@pytest.mark.parametrize("S", [256, 768, 4096])
def test_tile_ranges_stay_in_range_for_any_int(S):
    values = [-INT_MAX - 1, -INT_MAX, -65, -64, -1, 0, 1, 255, 256, S - 1, S,
              S + 63, S + 64, 10 * S, INT_MAX - 64, INT_MAX - 1, INT_MAX]
    for blk in range(S // 256):
        for val in values:
            first, last = _tiles(FWD, val, blk, S)
            assert 0 <= first <= last == blk * 4 + 3
            assert first <= blk * 4          # never past the block's own rows
            first, last = _tiles(BWD, val, blk, S)
            assert blk * 4 == first <= last <= S // 64 - 1


@needs_lib
def test_tile_decode_refuses_arguments_outside_a_launch():
    lib = native.load(require=True)
    a, b = ctypes.c_int(), ctypes.c_int()
    for kind, blk, S in [(2, 0, 256), (0, -1, 256), (0, 1, 256), (0, 0, 384),
                         (1, 0, 0)]:
        assert lib.attn_doc_tiles_decode(kind, 0, blk, S, ctypes.byref(a),
                                         ctypes.byref(b)) != 0
