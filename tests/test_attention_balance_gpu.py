"""Attention schedules (AITJ_ATTN_SCHED) and the per-q-head split of dK/dV
(AITJ_ATTN_BWD_SPLIT) on the GPU.

The block-id decode only changes which workgroup computes which tile, so
everything it touches is compared with torch.equal. The split changes the
fp32 association of the sum over a kv head's q heads and nothing else
(still one bf16 rounding per output), so split against unsplit is held
below the error both already have against fp32: a re-association term of
order 2^-24 under a shared bf16 rounding of order 2^-9."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.ops import native  # noqa: E402

DEV = "cuda:0"
D = 128
SHAPES = [(1, 6, 2, 768), (3, 4, 1, 512), (1, 2, 2, 256), (2, 8, 2, 1024)]
COMBOS = [(sched, split) for sched in ("legacy", "balanced")
          for split in ("0", "1")]
# the suite's gradient tolerance (tests/test_attention_gpu.py)
ATOL, RTOL = 7e-2, 5e-2


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
    """Inputs and the fp32 SDPA autograd reference of one shape, made once
    and shared (never modified) by every test that needs them."""
    if shape in _CASES:
        return _CASES[shape]
    B, H, HKV, S = shape
    g = torch.Generator(device=DEV).manual_seed(17 + S + H)
    q, k, v = _randn(g, B, H, S, D), _randn(g, B, HKV, S, D), \
        _randn(g, B, HKV, S, D)
    go = _randn(g, B, S, H * D)                    # as o_proj hands it back
    q32, k32, v32 = (t.float().requires_grad_() for t in (q, k, v))
    o32 = torch.nn.functional.scaled_dot_product_attention(
        q32, k32, v32, is_causal=True, enable_gqa=H != HKV)
    o32.backward(go.view(B, S, H, D).transpose(1, 2).float())
    ref = tuple(t.grad.detach() for t in (q32, k32, v32))
    _CASES[shape] = (q, k, v, go, ref)
    return _CASES[shape]


def _run(shape, q, k, v, go):
    """Forward and backward through the strided entries into sentinel
    buffers with one spare head after each written range. Returns
    (out, lse, dq, dk, dv) as dense tensors after checking the sentinels."""
    B, H, HKV, S = shape
    scale = 1.0 / math.sqrt(D)
    lib = native.load(require=True)

    # forward: [o heads | spare]
    WO = (H + 1) * D
    obuf = _sentinel(B, S, WO)
    okeep = obuf.clone()
    lse = torch.empty(B, H, S, dtype=torch.float32, device=DEV)
    st = native.stride_array(q.stride()[:3], k.stride()[:3], v.stride()[:3],
                             _bhsd(WO, S))
    rc = lib.attn_fwd_strided(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        obuf.data_ptr(), lse.data_ptr(), st, B, H, HKV, S, scale)
    assert rc == 0
    oheads = obuf.view(B, S, H + 1, D)
    out = oheads[:, :, :H].transpose(1, 2).contiguous()

    # backward: [q heads | spare | k heads | spare | v heads | spare]
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

    okept = oheads.new_zeros(H + 1, dtype=torch.bool)
    okept[H] = True
    assert torch.equal(oheads[:, :, okept], okeep.view_as(oheads)[:, :, okept])
    heads = buf.view(B, S, W // D, D)
    kheads = keep.view_as(heads)
    kept = heads.new_zeros(W // D, dtype=torch.bool)
    kept[[H, kh0 + HKV, vh0 + HKV]] = True
    assert torch.equal(heads[:, :, kept], kheads[:, :, kept]), \
        "backward wrote outside the dq/dk/dv head ranges"
    # a tile no workgroup wrote still holds its sentinel bits
    same = heads[:, :, ~kept].view(torch.int16) == \
        kheads[:, :, ~kept].view(torch.int16)
    assert not same.any(), f"{int(same.sum())} sentinel values survive"
    osame = oheads[:, :, ~okept].view(torch.int16) == \
        okeep.view_as(oheads)[:, :, ~okept].view(torch.int16)
    assert not osame.any(), f"{int(osame.sum())} sentinel values survive in o"

    dq = heads[:, :, :H].transpose(1, 2).contiguous()
    dk = heads[:, :, kh0:kh0 + HKV].transpose(1, 2).contiguous()
    dv = heads[:, :, vh0:vh0 + HKV].transpose(1, 2).contiguous()
    return out, lse.clone(), dq, dk, dv, (nbytes > 0)


def _err(a, b):
    d = (a.float() - b.float()).abs()
    return d.max().item(), d.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_schedules_and_split_agree(shape, monkeypatch):
    B, H, HKV, S = shape
    q, k, v, go, (rq, rk, rv) = _case(shape)
    res = {}
    for sched, split in COMBOS:
        monkeypatch.setenv("AITJ_ATTN_SCHED", sched)
        monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", split)
        *res[(sched, split)], used_ws = _run(shape, q, k, v, go)
        assert used_ws == (split == "1")

    base = res[("legacy", "0")]
    for combo in COMBOS:
        out, lse, dq, dk, dv = res[combo]
        assert torch.equal(out, base[0]), f"out differs under {combo}"
        assert torch.equal(lse, base[1]), f"lse differs under {combo}"
        assert torch.equal(dq, base[2]), f"dq differs under {combo}"
        for name, got, ref in (("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
            mx, rms = _err(got, ref)
            print(f"{shape} {combo} {name} vs fp32: max {mx:.3e} rms {rms:.3e}")
            assert torch.allclose(got.float(), ref, atol=ATOL, rtol=RTOL), \
                f"{name} under {combo}: max err {mx}"
    for split in ("0", "1"):
        a, b = res[("legacy", split)], res[("balanced", split)]
        assert torch.equal(a[3], b[3]), f"dk differs by schedule, split={split}"
        assert torch.equal(a[4], b[4]), f"dv differs by schedule, split={split}"

    # re-association noise stays under the rounding both paths share
    for i, name, ref in ((3, "dk", rk), (4, "dv", rv)):
        uns, spl = res[("balanced", "0")][i], res[("balanced", "1")][i]
        d_max, d_rms = _err(spl, uns)
        e_max, e_rms = _err(uns, ref)
        print(f"{shape} {name}: |split-unsplit| max {d_max:.3e} rms "
              f"{d_rms:.3e}; |unsplit-fp32| max {e_max:.3e} rms {e_rms:.3e}")
        assert d_max <= e_max and d_rms <= e_rms, (name, d_max, d_rms,
                                                   e_max, e_rms)


def test_split_repeats_bit_exact(monkeypatch):
    shape = SHAPES[0]
    q, k, v, go, _ = _case(shape)
    monkeypatch.setenv("AITJ_ATTN_SCHED", "balanced")
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "1")
    first = _run(shape, q, k, v, go)
    for _ in range(2):
        again = _run(shape, q, k, v, go)
        for a, b in zip(first[:5], again[:5]):
            assert torch.equal(a, b)


def test_entry_without_workspace_matches(monkeypatch):
    """attn_bwd_strided (no workspace argument) takes the split path with a
    transient workspace of its own and lands on the same bits."""
    from trainingjob_operator_amd.ops.attention import flash_attention_fwd_only
    shape = SHAPES[0]
    B, H, HKV, S = shape
    q, k, v, go, _ = _case(shape)
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "1")
    monkeypatch.delenv("AITJ_ATTN_SCHED", raising=False)
    _, _, rdq, rdk, rdv, _ = _run(shape, q, k, v, go)
    out, lse = flash_attention_fwd_only(q, k, v)
    lib = native.load(require=True)
    delta = torch.empty(B, H, S, dtype=torch.float32, device=DEV)
    dq = torch.empty_like(q)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    st = native.stride_array(q.stride()[:3], k.stride()[:3], v.stride()[:3],
                             out.stride()[:3], _bhsd(H * D, S),
                             dq.stride()[:3], dk.stride()[:3],
                             dv.stride()[:3])
    rc = lib.attn_bwd_strided(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        out.data_ptr(), go.data_ptr(), lse.data_ptr(), delta.data_ptr(),
        dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), st, B, H, HKV, S,
        1.0 / math.sqrt(D))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(dq, rdq) and torch.equal(dk, rdk) \
        and torch.equal(dv, rdv)


def test_missing_workspace_is_refused(monkeypatch):
    """Split forced, workspace null or short: every _ws entry returns
    nonzero (only the return code is looked at)."""
    B, H, HKV, S = 1, 4, 2, 256
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "1")
    lib = native.load(require=True)
    need = lib.attn_bwd_ws_bytes(B, H, HKV, S, 1)
    assert need == 2 * B * H * S * D * 4
    g = torch.Generator(device=DEV).manual_seed(2)
    q, k, v = _randn(g, B, H, S, D), _randn(g, B, HKV, S, D), \
        _randn(g, B, HKV, S, D)
    out, go = _randn(g, B, H, S, D), _randn(g, B, H, S, D)
    lse = torch.zeros(B, H, S, dtype=torch.float32, device=DEV)
    delta = torch.zeros_like(lse)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    small = torch.empty(need - 16, dtype=torch.uint8, device=DEV)
    sp = native.stream_ptr()
    t = lambda x: x.stride()[:3]
    for ws, nbytes in ((None, 0), (None, need), (small.data_ptr(), need - 16)):
        rc = lib.attn_bwd_ws(
            sp, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
            go.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
            dk.data_ptr(), dv.data_ptr(), *t(q), *t(k), *t(v), B, H, HKV, S,
            0.1, ws, nbytes)
        assert rc != 0
        st8 = native.stride_array(t(q), t(k), t(v), t(out), t(go), t(dq),
                                  t(dk), t(dv))
        rc = lib.attn_bwd_strided_ws(
            sp, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
            go.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
            dk.data_ptr(), dv.data_ptr(), st8, B, H, HKV, S, 0.1, ws, nbytes)
        assert rc != 0
        st7 = native.stride_array(t(q), t(k), t(v), t(go), t(dq), t(dk),
                                  t(dv))
        for causal in (0, 1):
            rc = lib.attn_block_bwd_ws(
                sp, q.data_ptr(), k.data_ptr(), v.data_ptr(), go.data_ptr(),
                lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                dk.data_ptr(), dv.data_ptr(), st7, B, H, HKV, S, 0.1, causal,
                ws, nbytes)
            assert rc != 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("split", ["0", "1"])
def test_noncausal_block_bwd_against_fp32_twin(split, monkeypatch):
    from trainingjob_operator_amd.ops import reference
    from trainingjob_operator_amd.ops.attention import (
        flash_attention_block_bwd, flash_attention_block_fwd,
        flash_attention_delta)
    B, H, HKV, S = 1, 4, 2, 512
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", split)
    g = torch.Generator(device=DEV).manual_seed(23)
    q, k, v = _randn(g, B, H, S, D), _randn(g, B, HKV, S, D), \
        _randn(g, B, HKV, S, D)
    do = _randn(g, B, H, S, D)
    o, lse = flash_attention_block_fwd(q, k, v, False)
    delta = flash_attention_delta(o, do)
    dq, dk, dv = flash_attention_block_bwd(q, k, v, do, lse, delta, False)
    rdq, rdk, rdv = reference.attention_block_bwd(
        q.float(), k.float(), v.float(), do.float(), lse, delta, False)
    torch.cuda.synchronize()
    for name, got, ref in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        mx, rms = _err(got, ref)
        print(f"non-causal split={split} {name}: max {mx:.3e} rms {rms:.3e}")
        assert torch.allclose(got.float(), ref.float(), atol=ATOL,
                              rtol=RTOL), f"{name}: max err {mx}"
