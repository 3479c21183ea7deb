"""Pair ownership of the causal unsplit dK/dV workgroups
(AITJ_ATTN_BWD_FOLD=2) on the GPU.

The pair kernels let the two waves of a SIMD share one 32-row kv strip:
each computes one 32-row sub of every q tile, they swap the packed P / dS
fragments through LDS, and each accumulates two of the strip's four d
subtiles over all four q chunks in the order the single owner uses. Every
accumulator meets the same fragments in the same order, so dq, dk and dv
are compared with torch.equal against the identity ownership, under both
block schedules and over repeats (a missed barrier in the exchange would
show as a run-to-run difference). The gradients land in sentinel buffers
with a spare head after each range, so a strip or d subtile nobody wrote,
or one written outside its range, shows. The paired result is also held
against fp32 SDPA autograd at the suite's gradient tolerance."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.ops import native  # noqa: E402

DEV = "cuda:0"
D = 128
# n = S/256 row blocks: 1 (both phases inside one block, strips that sit
# out the first tile), 2, 3 (odd, a group of 4 q heads so the chain crosses
# q heads), 4 with two batches
SHAPES = [(1, 2, 2, 256), (1, 4, 2, 512), (1, 8, 2, 768), (2, 8, 2, 1024)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
# the suite's gradient tolerance (tests/test_attention_gpu.py)
ATOL, RTOL = 7e-2, 5e-2
PAIR = 2


def _randn(g, *shape):
    return (torch.randn(*shape, device=DEV, generator=g) * 0.5).bfloat16()


def _sentinel(*shape):
    """The pattern of tests/test_packed_attention_gpu.py: raw bf16 bits
    0x7A00 | i % 251, large finite values no kernel output lands on."""
    n = 1
    for s in shape:
        n *= s
    bits = (torch.arange(n, device=DEV, dtype=torch.int32) % 251 + 0x7A00)
    return bits.to(torch.int16).view(torch.bfloat16).reshape(shape).clone()


def _bhsd(row, S):
    return (S * row, D, row)


_CASES = {}


def _case(shape):
    """Inputs, the forward's (out, lse) and the fp32 SDPA autograd reference
    of one shape, made once and shared (never modified) by every test."""
    if shape in _CASES:
        return _CASES[shape]
    from trainingjob_operator_amd.ops.attention import flash_attention_fwd_only
    B, H, HKV, S = shape
    g = torch.Generator(device=DEV).manual_seed(37 + S + H)
    q, k, v = _randn(g, B, H, S, D), _randn(g, B, HKV, S, D), \
        _randn(g, B, HKV, S, D)
    go = _randn(g, B, S, H * D)                    # as o_proj hands it back
    out, lse = flash_attention_fwd_only(q, k, v)
    q32, k32, v32 = (t.float().requires_grad_() for t in (q, k, v))
    o32 = torch.nn.functional.scaled_dot_product_attention(
        q32, k32, v32, is_causal=True, enable_gqa=H != HKV)
    o32.backward(go.view(B, S, H, D).transpose(1, 2).float())
    ref = tuple(t.grad.detach() for t in (q32, k32, v32))
    _CASES[shape] = (q, k, v, go, out, lse, ref)
    return _CASES[shape]


def _run_bwd(shape, q, k, v, go, out, lse):
    """Backward through the strided entry into a sentinel buffer
    [q heads | spare | k heads | spare | v heads | spare]. Returns dense
    (dq, dk, dv) after checking the sentinels."""
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
    # a strip or d subtile no wave wrote still holds its sentinel bits
    same = heads[:, :, ~kept].view(torch.int16) == \
        kheads[:, :, ~kept].view(torch.int16)
    assert not same.any(), f"{int(same.sum())} sentinel values survive"

    dq = heads[:, :, :H].transpose(1, 2).contiguous()
    dk = heads[:, :, kh0:kh0 + HKV].transpose(1, 2).contiguous()
    dv = heads[:, :, vh0:vh0 + HKV].transpose(1, 2).contiguous()
    return dq, dk, dv, (nbytes > 0)


def _err(a, b):
    d = (a.float() - b.float()).abs()
    return d.max().item(), d.pow(2).mean().sqrt().item()


def _set_sched(monkeypatch, sched):
    if sched == "default":
        monkeypatch.delenv("AITJ_ATTN_SCHED", raising=False)
    else:
        monkeypatch.setenv("AITJ_ATTN_SCHED", sched)


@pytest.mark.parametrize("sched", ["default", "legacy"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pair_keeps_every_bit(shape, sched, monkeypatch):
    q, k, v, go, out, lse, ref = _case(shape)
    B, H, HKV, S = shape
    lib = native.load(require=True)
    _set_sched(monkeypatch, sched)
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "0")
    monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", "0")
    *off, used_ws = _run_bwd(shape, q, k, v, go, out, lse)
    assert not used_ws
    monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", "2")
    for kernel in (0, 1):                     # the pair kernels really run
        assert lib.attn_bwd_fold_mode(B, H, HKV, S, 1, 0, kernel) == PAIR
    runs = []
    for _ in range(3):
        *on, used_ws = _run_bwd(shape, q, k, v, go, out, lse)
        assert not used_ws
        runs.append(on)
    for rep, on in enumerate(runs):
        for name, a, b in zip(("dq", "dk", "dv"), on, off):
            assert torch.equal(a, b), \
                f"{name} differs between pair and identity, repeat {rep}, " \
                f"sched={sched}"
    for name, got, want in zip(("dq", "dk", "dv"), runs[0], ref):
        mx, rms = _err(got, want)
        print(f"{shape} sched={sched} pair {name} vs fp32: "
              f"max {mx:.3e} rms {rms:.3e}")
        assert torch.allclose(got.float(), want, atol=ATOL, rtol=RTOL), \
            f"{name} with pair, sched={sched}: max err {mx}"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_split_launches_ignore_the_pair_knob(shape, monkeypatch):
    q, k, v, go, out, lse, _ = _case(shape)
    monkeypatch.delenv("AITJ_ATTN_SCHED", raising=False)
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "1")
    res = {}
    for fold in ("0", "2"):
        monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", fold)
        *res[fold], used_ws = _run_bwd(shape, q, k, v, go, out, lse)
        assert used_ws
    for name, off, on in zip(("dq", "dk", "dv"), res["0"], res["2"]):
        assert torch.equal(on, off), \
            f"split {name} depends on AITJ_ATTN_BWD_FOLD=2"


def test_noncausal_block_bwd_ignores_the_pair_knob(monkeypatch):
    """The non-causal instantiations keep the identity ownership whatever
    the flag says."""
    from trainingjob_operator_amd.ops.attention import (
        flash_attention_block_bwd, flash_attention_block_fwd,
        flash_attention_delta)
    B, H, HKV, S = 1, 4, 2, 512
    monkeypatch.delenv("AITJ_ATTN_BWD_SPLIT", raising=False)
    g = torch.Generator(device=DEV).manual_seed(41)
    q, k, v = _randn(g, B, H, S, D), _randn(g, B, HKV, S, D), \
        _randn(g, B, HKV, S, D)
    do = _randn(g, B, H, S, D)
    o, lse = flash_attention_block_fwd(q, k, v, False)
    delta = flash_attention_delta(o, do)
    res = {}
    for fold in ("0", "2"):
        monkeypatch.setenv("AITJ_ATTN_BWD_FOLD", fold)
        res[fold] = flash_attention_block_bwd(q, k, v, do, lse, delta, False)
        torch.cuda.synchronize()
    for name, off, on in zip(("dq", "dk", "dv"), res["0"], res["2"]):
        assert torch.equal(on, off), f"non-causal {name} depends on the knob"
