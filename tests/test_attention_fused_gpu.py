"""The fused dK/dV pair walk (AITJ_ATTN_BWD_FOLD=3) on the GPU.

attn_bwd_dkdv_pair_kernel walks each causal unsplit kv strip once for both
gradients: the pair ownership of attn_bwd_dk_pair_kernel, with P kept next
to dS, both swapped between the partner waves, and dvacc accumulated before
dkacc over the same chunks in the same order as the two single kernels. So
dk and dv are compared with torch.equal against the identity ownership
(AITJ_ATTN_BWD_FOLD=0), over repeats (a missed barrier would show as a
run-to-run difference), and dq, which the knob does not touch, with them.
The gradients land in a sentinel buffer with a spare head after each range,
so a strip or d subtile nobody wrote, or one written outside its range,
shows. Split and non-causal launches ignore the knob."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.ops import native  # noqa: E402

DEV = "cuda:0"
D = 128
# (B, H, HKV, S): one workgroup row, both phases, no GQA loop; two ranks, so
# half-block i pairs with 2n-1-i, a group of 2 q heads, two batches; odd n
# with a group of 4
SHAPES = [(1, 2, 2, 256), (2, 4, 2, 512), (1, 8, 2, 768)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
FUSED = 3


def _randn(g, *shape):
    return (torch.randn(*shape, device=DEV, generator=g) * 0.5).bfloat16()


def _sentinel(*shape):
    """Raw bf16 bits 0x7A00 | i % 251: large finite values no kernel output
    lands on (the pattern of tests/test_packed_attention_gpu.py)."""
    n = 1
    for s in shape:
        n *= s
    bits = (torch.arange(n, device=DEV, dtype=torch.int32) % 251 + 0x7A00)
    return bits.to(torch.int16).view(torch.bfloat16).reshape(shape).clone()


def _bhsd(row, S):
    return (S * row, D, row)


_CASES = {}


def _case(shape, packed=False):
    """Inputs and the forward's (out, lse) of one shape, made once and shared
    (never modified). packed: q, k and v are views of one [B, S,
    (H + 2 HKV) * 128] buffer, as the model's QKV projection leaves them."""
    key = (shape, packed)
    if key in _CASES:
        return _CASES[key]
    from trainingjob_operator_amd.ops.attention import flash_attention_fwd_only
    B, H, HKV, S = shape
    g = torch.Generator(device=DEV).manual_seed(53 + S + H)
    if packed:
        qkv = _randn(g, B, S, H + 2 * HKV, D)
        q, k, v = (t.transpose(1, 2) for t in
                   qkv.split((H, HKV, HKV), dim=2))
    else:
        q, k, v = _randn(g, B, H, S, D), _randn(g, B, HKV, S, D), \
            _randn(g, B, HKV, S, D)
    go = _randn(g, B, S, H * D)                    # as o_proj hands it back
    out, lse = flash_attention_fwd_only(q.contiguous(), k.contiguous(),
                                        v.contiguous())
    _CASES[key] = (q, k, v, go, out, lse)
    return _CASES[key]


def _run_bwd(shape, q, k, v, go, out, lse):
    """Backward through the strided entry into a sentinel buffer
    [q heads | spare | k heads | spare | v heads | spare]. Returns dense
    (dq, dk, dv) after checking the sentinels, and whether the launch was
    split."""
    B, H, HKV, S = shape
    scale = 1.0 / math.sqrt(D)
    lib = native.load(require=True)
    W = (H + 2 * HKV + 3) * D
    kh0, vh0 = H + 1, H + 1 + HKV + 1
    buf = _sentinel(B, S, W)
    keep = buf.clone()
    delta = torch.empty(B, H, S, dtype=torch.float32, device=DEV)
    esz = buf.element_size()
    nbytes = lib.attn_bwd_ws_bytes(B, H, HKV, S, 1)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    st = native.stride_array(q.stride()[:3], k.stride()[:3], v.stride()[:3],
                             out.stride()[:3], _bhsd(H * D, S),
                             _bhsd(W, S), _bhsd(W, S), _bhsd(W, S))
    rc = lib.attn_bwd_strided_ws(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        out.data_ptr(), go.data_ptr(), lse.data_ptr(), delta.data_ptr(),
        buf.data_ptr(), buf.data_ptr() + kh0 * D * esz,
        buf.data_ptr() + vh0 * D * esz, st, B, H, HKV, S, scale,
        ws.data_ptr() if nbytes else None, nbytes)
    assert rc == 0
    torch.cuda.synchronize()

    heads = buf.view(B, S, W // D, D)
    kheads = keep.view_as(heads)
    kept = heads.new_zeros(W // D, dtype=torch.bool)
    kept[[H, kh0 + HKV, vh0 + HKV]] = True
    assert torch.equal(heads[:, :, kept], kheads[:, :, kept]), \
        "backward wrote outside the dq/dk/dv head ranges"
    same = heads[:, :, ~kept].view(torch.int16) == \
        kheads[:, :, ~kept].view(torch.int16)
    assert not same.any(), f"{int(same.sum())} sentinel values survive"

    dq = heads[:, :, :H].transpose(1, 2).contiguous()
    dk = heads[:, :, kh0:kh0 + HKV].transpose(1, 2).contiguous()
    dv = heads[:, :, vh0:vh0 + HKV].transpose(1, 2).contiguous()
    return dq, dk, dv, (nbytes > 0)


def _fused_against_identity(shape, case, monkeypatch):
    B, H, HKV, S = shape
    lib = native.load(require=True)
    monkeypatch.delenv("AITJ_ATTN_SCHED", raising=False)
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "0")
    monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", "0")
    *off, used_ws = _run_bwd(shape, *case)
    assert not used_ws
    monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", "3")
    for kernel in (0, 1):                     # the fused kernel really runs
        assert lib.attn_bwd_fold_mode(B, H, HKV, S, 1, 0, kernel) == FUSED
    for rep in range(3):
        *on, used_ws = _run_bwd(shape, *case)
        assert not used_ws
        for name, a, b in zip(("dq", "dk", "dv"), on, off):
            assert torch.equal(a, b), \
                f"{name} differs between fused and identity, repeat {rep}"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_keeps_every_bit(shape, monkeypatch):
    _fused_against_identity(shape, _case(shape), monkeypatch)


def test_fused_keeps_every_bit_through_packed_strides(monkeypatch):
    shape = SHAPES[1]
    _fused_against_identity(shape, _case(shape, packed=True), monkeypatch)


def test_unset_fuses_up_to_four_workgroups_per_cu(monkeypatch):
    """Unset, a causal unsplit launch of up to four workgroups per CU (the
    largest grid measured) fuses; a larger one keeps the identity for both
    kernels."""
    lib = native.load(require=True)
    monkeypatch.delenv("AITJ_ATTN_BWD_FOLD", raising=False)
    for kernel in (0, 1):
        assert lib.attn_bwd_fold_mode(2, 32, 8, 4096, 1, 0, kernel) == FUSED
        assert lib.attn_bwd_fold_mode(8, 32, 8, 4096, 1, 0, kernel) == FUSED
        assert lib.attn_bwd_fold_mode(16, 32, 8, 4096, 1, 0, kernel) == 0
        # split launches keep the fold (here 8 workgroups)
        assert lib.attn_bwd_fold_mode(1, 4, 2, 512, 1, 1, kernel) == 1


def test_split_launches_ignore_the_fused_knob(monkeypatch):
    shape = SHAPES[1]
    case = _case(shape)
    monkeypatch.delenv("AITJ_ATTN_SCHED", raising=False)
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "1")
    res = {}
    for fold in ("0", "3"):
        monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", fold)
        *res[fold], used_ws = _run_bwd(shape, *case)
        assert used_ws
    for name, off, on in zip(("dq", "dk", "dv"), res["0"], res["3"]):
        assert torch.equal(on, off), \
            f"split {name} depends on AITJ_ATTN_BWD_FOLD=3"


def test_noncausal_block_bwd_ignores_the_fused_knob(monkeypatch):
    from trainingjob_operator_amd.ops.attention import (
        flash_attention_block_bwd, flash_attention_block_fwd,
        flash_attention_delta)
    B, H, HKV, S = 1, 4, 2, 512
    monkeypatch.delenv("AITJ_ATTN_BWD_SPLIT", raising=False)
    g = torch.Generator(device=DEV).manual_seed(59)
    q, k, v = _randn(g, B, H, S, D), _randn(g, B, HKV, S, D), \
        _randn(g, B, HKV, S, D)
    do = _randn(g, B, H, S, D)
    o, lse = flash_attention_block_fwd(q, k, v, False)
    delta = flash_attention_delta(o, do)
    res = {}
    for fold in ("0", "3"):
        monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", fold)
        res[fold] = flash_attention_block_bwd(q, k, v, do, lse, delta, False)
        torch.cuda.synchronize()
    for name, off, on in zip(("dq", "dk", "dv"), res["0"], res["3"]):
        assert torch.equal(on, off), f"non-causal {name} depends on the knob"
