"""Rectangular non-causal attention blocks (S_q != S_kv) of the native flash
kernels, as the zig-zag context-parallel ring calls them (GPU numerics).

Every rect call here runs twice: through the public wrapper, and through
the C entry on operands that are interior slices of larger NaN-filled
tensors. An out-of-range read then shows as NaN in a result and a stray
write as a changed surround; the two results must be bit-identical.

Tolerances are those of tests/test_block_attention_gpu.py: the same kernels
against the same kind of fp32 reference."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 128
PAD = 64            # guard rows around [.., S, 128] operands
PADF = 256          # guard elements around flat fp32 buffers
FWD_TOL = dict(atol=3e-2, rtol=2e-2)
LSE_TOL = dict(atol=2e-2, rtol=1e-3)
GRAD_TOL = dict(atol=7e-2, rtol=5e-2)
NAN = float("nan")


def _rand(gen, *shape):
    return (torch.randn(*shape, device=DEV, generator=gen) * 0.5).bfloat16()


@functools.lru_cache(maxsize=None)
def _qkv(seed, B, H, HKV, Sq, Skv):
    """q, k, v, gout: shared between tests, read-only."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (_rand(g, B, H, Sq, D), _rand(g, B, HKV, Skv, D),
            _rand(g, B, HKV, Skv, D), _rand(g, B, H, Sq, D))


def _ref_attention(q, k, v, causal, gout=None):
    """fp32 SDPA (GQA-aware); with gout also dq/dk/dv by autograd."""
    q32, k32, v32 = (t.float().detach().clone().requires_grad_(gout is not None)
                     for t in (q, k, v))
    o = torch.nn.functional.scaled_dot_product_attention(
        q32, k32, v32, is_causal=causal, enable_gqa=k.shape[1] != q.shape[1])
    if gout is None:
        return o
    (o * gout.float()).sum().backward()
    return o.detach(), q32.grad, k32.grad, v32.grad


@functools.lru_cache(maxsize=None)
def _ref(seed, B, H, HKV, Sq, Skv):
    q, k, v, gout = _qkv(seed, B, H, HKV, Sq, Skv)
    return _ref_attention(q, k, v, False, gout)


def _ref_lse(q, k, h):
    hkv = h // (q.shape[1] // k.shape[1])
    s = (q[0, h].float() @ k[0, hkv].float().T) / math.sqrt(D)
    return torch.logsumexp(s, dim=-1)


def _close(a, b, tol, name):
    err = (a.float() - b.float()).abs().max().item()
    print(f"{name}: max abs err {err:.5f}")
    assert torch.allclose(a.float(), b.float(), **tol), f"{name} max err {err}"


class Guards:
    """Operands inside NaN-filled surroundings, and the check that the
    surroundings are still NaN everywhere."""

    def __init__(self):
        self.surrounds = []

    def rows(self, src=None, shape=None, permuted=False):
        """A [B,h,S,128] bf16 operand: a copy of src, or all NaN (an output
        the kernel must fill). permuted: [B,S,h,128] storage."""
        B, h, S, _ = shape or src.shape
        if permuted:
            base = torch.full((B, S + 2 * PAD, h, D), NAN,
                              dtype=torch.bfloat16, device=DEV)
            view = base[:, PAD:PAD + S].permute(0, 2, 1, 3)
            self.surrounds += [base[:, :PAD], base[:, PAD + S:]]
        else:
            base = torch.full((B, h, S + 2 * PAD, D), NAN,
                              dtype=torch.bfloat16, device=DEV)
            view = base[:, :, PAD:PAD + S]
            self.surrounds += [base[:, :, :PAD], base[:, :, PAD + S:]]
        if src is not None:
            view.copy_(src)
        return view

    def flat(self, src=None, shape=None):
        """A dense fp32 tensor in the middle of a flat NaN buffer."""
        shape = tuple(shape or src.shape)
        n = math.prod(shape)
        base = torch.full((n + 2 * PADF,), NAN, dtype=torch.float32,
                          device=DEV)
        view = base[PADF:PADF + n].view(shape)
        self.surrounds += [base[:PADF], base[PADF + n:]]
        if src is not None:
            view.copy_(src)
        return view

    def check(self):
        for s in self.surrounds:
            assert bool(torch.isnan(s).all()), "a surround was written"


def _tri(t):
    assert t.stride(-1) == 1
    return (t.stride(0), t.stride(1), t.stride(2))


def _lib():
    from trainingjob_operator_amd.ops import native
    return native, native.load(require=True)


def _raw_fwd(q, k, v, causal=False, permuted=False):
    """attn_block_fwd_rect on guarded operands -> (rc, out, lse, guards)."""
    native, lib = _lib()
    B, H, Sq, _ = q.shape
    HKV, Skv = k.shape[1], k.shape[2]
    g = Guards()
    gq, gk, gv = (g.rows(t, permuted=permuted) for t in (q, k, v))
    out = g.rows(shape=(B, H, Sq, D), permuted=permuted)
    lse = g.flat(shape=(B, H, Sq))
    st = native.stride_array(_tri(gq), _tri(gk), _tri(gv), _tri(out))
    rc = lib.attn_block_fwd_rect(
        native.stream_ptr(), gq.data_ptr(), gk.data_ptr(), gv.data_ptr(),
        out.data_ptr(), lse.data_ptr(), st, B, H, HKV, Sq, Skv,
        1.0 / math.sqrt(D), 1 if causal else 0)
    torch.cuda.synchronize()
    g.check()
    return rc, out, lse


def _raw_bwd(q, k, v, gout, lse, delta, causal=False, ws_short=0):
    """attn_block_bwd_rect_ws on guarded operands, workspace by the rect
    rule (ws_short bytes less than it asks for) -> (rc, dq, dk, dv)."""
    native, lib = _lib()
    B, H, Sq, _ = q.shape
    HKV, Skv = k.shape[1], k.shape[2]
    g = Guards()
    gq, gk, gv, gg = (g.rows(t) for t in (q, k, v, gout))
    glse, gdelta = g.flat(lse), g.flat(delta)
    dq = g.rows(shape=(B, H, Sq, D))
    dk = g.rows(shape=(B, HKV, Skv, D))
    dv = g.rows(shape=(B, HKV, Skv, D))
    need = lib.attn_bwd_ws_bytes_rect(B, H, HKV, Sq, Skv, 1 if causal else 0)
    ws, ws_ptr = None, None
    if need > 0:
        ws = g.flat(shape=((need - ws_short) // 4,))
        ws_ptr = ws.data_ptr()
    st = native.stride_array(_tri(gq), _tri(gk), _tri(gv), _tri(gg),
                             _tri(dq), _tri(dk), _tri(dv))
    rc = lib.attn_block_bwd_rect_ws(
        native.stream_ptr(), gq.data_ptr(), gk.data_ptr(), gv.data_ptr(),
        gg.data_ptr(), glse.data_ptr(), gdelta.data_ptr(), dq.data_ptr(),
        dk.data_ptr(), dv.data_ptr(), st, B, H, HKV, Sq, Skv,
        1.0 / math.sqrt(D), 1 if causal else 0, ws_ptr,
        max(need - ws_short, 0))
    torch.cuda.synchronize()
    g.check()
    return rc, dq, dk, dv, need


def _no_nan(*ts):
    for t in ts:
        assert not bool(torch.isnan(t).any()), "NaN: an out-of-range read " \
            "or an unwritten output"


def _fwd(q, k, v, permuted=False):
    """Public wrapper and guarded C entry, bit-identical -> (out, lse)."""
    from trainingjob_operator_amd.ops.attention import (
        flash_attention_block_fwd,
    )
    if permuted:
        q, k, v = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
                   for t in (q, k, v))
        assert not q.is_contiguous()
    out, lse = flash_attention_block_fwd(q, k, v, False)
    rc, gout_, glse = _raw_fwd(q, k, v, permuted=permuted)
    assert rc == 0
    _no_nan(gout_, glse)
    assert torch.equal(out, gout_) and torch.equal(lse, glse)
    return out, lse


def _bwd(q, k, v, gout, lse, delta):
    from trainingjob_operator_amd.ops.attention import (
        flash_attention_block_bwd,
    )
    dq, dk, dv = flash_attention_block_bwd(q, k, v, gout, lse, delta, False)
    rc, gdq, gdk, gdv, _ = _raw_bwd(q, k, v, gout, lse, delta)
    assert rc == 0
    _no_nan(gdq, gdk, gdv)
    assert torch.equal(dq, gdq) and torch.equal(dk, gdk) \
        and torch.equal(dv, gdv)
    return dq, dk, dv


@pytest.mark.parametrize("Sq,Skv,permuted", [
    (512, 256, False), (256, 512, False), (768, 256, False),
    (256, 768, False), (256, 512, True)])
def test_rect_fwd_matches_fp32(Sq, Skv, permuted):
    """q blocks 1-2 and kv tiles 4-11 exist on one side only: a kernel that
    still took one length for both would read or skip them."""
    B, H, HKV = 2, 4, 2
    q, k, v, _ = _qkv(Sq + 3 * Skv, B, H, HKV, Sq, Skv)
    out, lse = _fwd(q, k, v, permuted)
    assert out.shape == (B, H, Sq, D) and lse.shape == (B, H, Sq)
    _close(out, _ref(Sq + 3 * Skv, B, H, HKV, Sq, Skv)[0], FWD_TOL, "out")
    _close(lse[0, 3], _ref_lse(q, k, 3), LSE_TOL, "lse")


def test_rect_fwd_forced_rescale():
    """Defer-rescale branch in the last kv tile, which only the S_kv bound
    reaches: K row 450 is a 40x copy of the mean q direction."""
    B, H, Sq, Skv = 1, 2, 256, 512
    q, k, v, _ = (t.clone() for t in _qkv(9, B, H, H, Sq, Skv))
    k[:, :, 450, :] = (q.float().mean(dim=2) * 40.0).bfloat16()
    out, _ = _fwd(q, k, v)
    _close(out, _ref_attention(q, k, v, False), FWD_TOL, "out")


@pytest.mark.parametrize("B,H,HKV,Sq,Skv,split", [
    (2, 8, 2, 512, 256, False), (2, 8, 2, 256, 512, False),
    (1, 4, 4, 256, 768, False), (2, 8, 2, 512, 256, True)])
def test_rect_bwd_matches_fp32_autograd(monkeypatch, B, H, HKV, Sq, Skv,
                                        split):
    from trainingjob_operator_amd.ops.attention import flash_attention_delta
    _, lib = _lib()
    if split:
        monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "1")
        assert lib.attn_bwd_ws_bytes_rect(B, H, HKV, Sq, Skv, 0) == \
            2 * B * H * Skv * D * 4
    else:
        monkeypatch.delenv("AITJ_ATTN_BWD_SPLIT", raising=False)
        assert lib.attn_bwd_ws_bytes_rect(B, H, HKV, Sq, Skv, 0) == 0
    seed = B * 100 + Sq + 3 * Skv
    q, k, v, gout = _qkv(seed, B, H, HKV, Sq, Skv)
    out, lse = _fwd(q, k, v)
    delta = flash_attention_delta(out, gout)
    dq, dk, dv = _bwd(q, k, v, gout, lse, delta)
    assert dq.shape == (B, H, Sq, D)
    assert dk.shape == (B, HKV, Skv, D) and dv.shape == (B, HKV, Skv, D)
    _, rdq, rdk, rdv = _ref(seed, B, H, HKV, Sq, Skv)
    _close(dq, rdq, GRAD_TOL, "dq")
    _close(dk, rdk, GRAD_TOL, "dk")
    _close(dv, rdv, GRAD_TOL, "dv")


def test_rect_blocks_with_global_statistics():
    """256 q rows x 768 keys as one rect (256 x 512) and one square
    (256 x 256) block merged; the backward per block on the MERGED lse and
    delta gives the gradients of the 768-key problem."""
    from trainingjob_operator_amd.ops.attention import (
        attn_merge_, flash_attention_block_bwd, flash_attention_block_fwd,
        flash_attention_delta,
    )
    B, H, HKV, Sq, Skv = 2, 4, 2, 256, 768
    q, k, v, gout = _qkv(77, B, H, HKV, Sq, Skv)
    ro, rdq, rdk, rdv = _ref(77, B, H, HKV, Sq, Skv)
    cuts = [slice(0, 512), slice(512, 768)]
    o_acc = torch.zeros(B, H, Sq, D, dtype=torch.float32, device=DEV)
    lse_acc = torch.full((B, H, Sq), float("-inf"), dtype=torch.float32,
                         device=DEV)
    o_j, lse_j = _fwd(q, k[:, :, cuts[0]], v[:, :, cuts[0]])
    attn_merge_(o_acc, lse_acc, o_j, lse_j)
    o_j, lse_j = flash_attention_block_fwd(q, k[:, :, cuts[1]],
                                           v[:, :, cuts[1]], False)
    attn_merge_(o_acc, lse_acc, o_j, lse_j)
    _close(o_acc, ro, FWD_TOL, "merged out")
    _close(lse_acc[0, 3], _ref_lse(q, k, 3), LSE_TOL, "merged lse")
    delta = flash_attention_delta(o_acc.bfloat16(), gout)
    dq = torch.zeros_like(o_acc)
    for i, sl in enumerate(cuts):
        fn = _bwd if i == 0 else (
            lambda *a: flash_attention_block_bwd(*a, False))
        dq_b, dk_b, dv_b = fn(q, k[:, :, sl], v[:, :, sl], gout, lse_acc,
                              delta)
        dq += dq_b
        _close(dk_b, rdk[:, :, sl], GRAD_TOL, f"dk block {i}")
        _close(dv_b, rdv[:, :, sl], GRAD_TOL, f"dv block {i}")
    _close(dq, rdq, GRAD_TOL, "dq")


def test_rect_fwd_bwd_repeats_bit_exact():
    from trainingjob_operator_amd.ops.attention import (
        flash_attention_block_bwd, flash_attention_block_fwd,
        flash_attention_delta,
    )
    q, k, v, gout = _qkv(7, 2, 8, 2, 512, 256)

    def once():
        out, lse = flash_attention_block_fwd(q, k, v, False)
        delta = flash_attention_delta(out, gout)
        return (out, lse,
                *flash_attention_block_bwd(q, k, v, gout, lse, delta, False))

    first = once()
    for _ in range(3):
        for name, a, b in zip(("out", "lse", "dq", "dk", "dv"), first,
                              once()):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("causal", [False, True])
def test_square_through_rect_entry_is_the_square_entry(causal):
    from trainingjob_operator_amd.ops.attention import (
        flash_attention_block_bwd, flash_attention_block_fwd,
        flash_attention_delta,
    )
    q, k, v, gout = _qkv(5, 2, 4, 2, 512, 512)
    out, lse = flash_attention_block_fwd(q, k, v, causal)
    rc, rout, rlse = _raw_fwd(q, k, v, causal=causal)
    assert rc == 0
    assert torch.equal(out, rout) and torch.equal(lse, rlse)
    delta = flash_attention_delta(out, gout)
    dq, dk, dv = flash_attention_block_bwd(q, k, v, gout, lse, delta, causal)
    rc, rdq, rdk, rdv, _ = _raw_bwd(q, k, v, gout, lse, delta, causal=causal)
    assert rc == 0
    assert torch.equal(dq, rdq) and torch.equal(dk, rdk) \
        and torch.equal(dv, rdv)


def _all_nan(*ts):
    for t in ts:
        assert bool(torch.isnan(t).all()), "a refused call wrote an output"


def test_rect_entries_refuse_and_launch_nothing(monkeypatch):
    """A refused shape returns nonzero (the wrappers raise) and no kernel
    runs: the NaN-filled outputs stay NaN."""
    from trainingjob_operator_amd.ops.attention import (
        flash_attention_block_bwd, flash_attention_block_fwd,
    )
    monkeypatch.delenv("AITJ_ATTN_BWD_SPLIT", raising=False)
    q, k, v, gout = _qkv(31, 1, 4, 2, 512, 256)
    lse = torch.zeros(1, 4, 512, device=DEV)
    # causal and rectangular
    with pytest.raises(AssertionError):
        flash_attention_block_fwd(q, k, v, True)
    with pytest.raises(AssertionError):
        flash_attention_block_bwd(q, k, v, gout, lse, lse, True)
    rc, out, glse = _raw_fwd(q, k, v, causal=True)
    assert rc != 0
    _all_nan(out, glse)
    rc, dq, dk, dv, _ = _raw_bwd(q, k, v, gout, lse, lse, causal=True)
    assert rc != 0
    _all_nan(dq, dk, dv)
    # S_kv = 128: not a multiple of 256
    k1, v1 = k[:, :, :128], v[:, :, :128]
    with pytest.raises(AssertionError):
        flash_attention_block_fwd(q, k1, v1, False)
    rc, out, glse = _raw_fwd(q, k1, v1)
    assert rc != 0
    _all_nan(out, glse)
    rc, dq, dk, dv, _ = _raw_bwd(q, k1, v1, gout, lse, lse)
    assert rc != 0
    _all_nan(dq, dk, dv)
    # split dv/dk with a workspace one float short
    monkeypatch.setenv("AITJ_ATTN_BWD_SPLIT", "1")
    rc, dq, dk, dv, need = _raw_bwd(q, k, v, gout, lse, lse, ws_short=4)
    assert need == 2 * 1 * 4 * 256 * D * 4
    assert rc == -2
    _all_nan(dq, dk, dv)
    native, _ = _lib()
    with pytest.raises(RuntimeError):
        native.check_rc(rc, "attn_block_bwd_rect_ws")
