"""Packed-QKV RoPE + attention against the unpacked composition (GPU).

The packed path runs the same kernels with the same rounding points and
the same summation order as apply_rope on dense q/k + flash_attention +
the transposes; only addresses differ. Every comparison is therefore
torch.equal, not a tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from trainingjob_operator_amd.ops import native  # noqa: E402

DEV = "cuda:0"
D = 128


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape):
    return (torch.randn(*shape, device=DEV, generator=g) * 0.5).bfloat16()


def _inv_freq():
    from trainingjob_operator_amd.ops import make_inv_freq
    return make_inv_freq(D, 500000.0, device=DEV)


def _composition(qkv, inv_freq, H, HKV):
    """The oracle: dense q/k, one RoPE each, [B,h,S,D] flash attention,
    transpose back."""
    from trainingjob_operator_amd.ops import apply_rope
    from trainingjob_operator_amd.ops.attention import flash_attention
    B, S, _ = qkv.shape
    q, k, v = qkv.split([H * D, HKV * D, HKV * D], dim=-1)
    q = q.reshape(B, S, H, D).contiguous()
    k = k.reshape(B, S, HKV, D).contiguous()
    v = v.reshape(B, S, HKV, D)
    q = apply_rope(q, inv_freq, S).transpose(1, 2)
    k = apply_rope(k, inv_freq, S).transpose(1, 2)
    o = flash_attention(q, k, v.transpose(1, 2))
    return o.transpose(1, 2).reshape(B, S, H * D)


@pytest.mark.parametrize("B,H,HKV,S", [(2, 4, 2, 512), (1, 2, 2, 256)])
def test_packed_matches_composition_bitwise(B, H, HKV, S):
    from trainingjob_operator_amd.ops.attention import packed_rope_attention
    g = _gen(11)
    qkv0 = _randn(g, B, S, (H + 2 * HKV) * D)
    go = _randn(g, B, S, H * D)
    inv_freq = _inv_freq()

    ref_in = qkv0.clone().requires_grad_()
    ref = _composition(ref_in, inv_freq, H, HKV)
    ref.backward(go)

    new_in = qkv0.clone().requires_grad_()
    out = packed_rope_attention(new_in, inv_freq, H, HKV)
    out.backward(go)
    torch.cuda.synchronize()

    assert out.shape == (B, S, H * D) and out.is_contiguous()
    assert torch.equal(out, ref), \
        f"o differs: max {(out.float() - ref.float()).abs().max()}"
    assert torch.equal(new_in.grad, ref_in.grad), (
        "dqkv differs: max "
        f"{(new_in.grad.float() - ref_in.grad.float()).abs().max()}")


def _sentinel(*shape):
    """A recognisable non-constant bf16 pattern (raw bits 0x7A00 | i % 251:
    large finite values no kernel output lands on by accident)."""
    n = 1
    for s in shape:
        n *= s
    bits = (torch.arange(n, device=DEV, dtype=torch.int32) % 251 + 0x7A00)
    return bits.to(torch.int16).view(torch.bfloat16).reshape(shape).clone()


def _bhsd(row, S):
    return (S * row, D, row)


def test_strided_forward_keeps_sentinels():
    """attn_fwd_strided writes o into heads [HKV, HKV+H) of a packed
    [B,S,(H+2HKV)*D] buffer (packed row stride, head offset): the head
    ranges before and after it — the v range included — keep the sentinel,
    the view equals the contiguous entry point bit for bit."""
    from trainingjob_operator_amd.ops.attention import flash_attention_fwd_only
    B, H, HKV, S = 2, 4, 2, 512
    W = (H + 2 * HKV) * D
    g = _gen(5)
    q, k, v = _randn(g, B, H, S, D), _randn(g, B, HKV, S, D), \
        _randn(g, B, HKV, S, D)
    ref_o, ref_lse = flash_attention_fwd_only(q, k, v)

    buf = _sentinel(B, S, W)
    keep = buf.clone()
    lse = torch.empty(B, H, S, dtype=torch.float32, device=DEV)
    lib = native.load(require=True)
    st = native.stride_array(q.stride()[:3], k.stride()[:3], v.stride()[:3],
                             _bhsd(W, S))
    rc = lib.attn_fwd_strided(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        buf.data_ptr() + HKV * D * buf.element_size(), lse.data_ptr(),
        st, B, H, HKV, S, 1.0 / D ** 0.5)
    assert rc == 0
    torch.cuda.synchronize()
    heads = buf.view(B, S, H + 2 * HKV, D)
    assert torch.equal(heads[:, :, HKV:HKV + H].transpose(1, 2), ref_o)
    assert torch.equal(lse, ref_lse)
    kheads = keep.view_as(heads)
    assert torch.equal(heads[:, :, :HKV], kheads[:, :, :HKV]) and \
        torch.equal(heads[:, :, HKV + H:], kheads[:, :, HKV + H:]), \
        "forward wrote outside its head range"


def test_strided_backward_keeps_sentinels():
    """attn_bwd_strided with dout as [B,S,H*D] and dq/dk/dv as head ranges
    of packed buffers one head wider than needed: the spare head keeps the
    sentinel, the views equal the contiguous entry point bit for bit."""
    from trainingjob_operator_amd.ops.attention import (
        _native_backward, flash_attention_fwd_only)
    B, H, HKV, S = 2, 4, 2, 512
    g = _gen(6)
    q, k, v = _randn(g, B, H, S, D), _randn(g, B, HKV, S, D), \
        _randn(g, B, HKV, S, D)
    go = _randn(g, B, S, H * D)                      # as o_proj returns it
    scale = 1.0 / D ** 0.5
    out, lse = flash_attention_fwd_only(q, k, v)
    go_bhsd = go.view(B, S, H, D).transpose(1, 2)
    ref_dq, ref_dk, ref_dv = _native_backward(q, k, v, out, lse, go_bhsd,
                                              scale)

    # layout: [q heads | spare | k heads | spare | v heads | spare]
    W = (H + 2 * HKV + 3) * D
    kh0, vh0 = H + 1, H + 1 + HKV + 1
    buf = _sentinel(B, S, W)
    keep = buf.clone()
    delta = torch.empty(B, H, S, dtype=torch.float32, device=DEV)
    esz = buf.element_size()
    lib = native.load(require=True)
    st = native.stride_array(q.stride()[:3], k.stride()[:3], v.stride()[:3],
                             out.stride()[:3], _bhsd(H * D, S),
                             _bhsd(W, S), _bhsd(W, S), _bhsd(W, S))
    rc = lib.attn_bwd_strided(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        out.data_ptr(), go.data_ptr(), lse.data_ptr(), delta.data_ptr(),
        buf.data_ptr(), buf.data_ptr() + kh0 * D * esz,
        buf.data_ptr() + vh0 * D * esz, st, B, H, HKV, S, scale)
    assert rc == 0
    torch.cuda.synchronize()
    heads = buf.view(B, S, W // D, D)
    assert torch.equal(heads[:, :, :H].transpose(1, 2), ref_dq)
    assert torch.equal(heads[:, :, kh0:kh0 + HKV].transpose(1, 2), ref_dk)
    assert torch.equal(heads[:, :, vh0:vh0 + HKV].transpose(1, 2), ref_dv)
    kept = heads.new_zeros(W // D, dtype=torch.bool)
    kept[[H, kh0 + HKV, vh0 + HKV]] = True
    assert torch.equal(heads[:, :, kept], keep.view_as(heads)[:, :, kept]), \
        "backward wrote outside the dq/dk/dv head ranges"


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_packed_rope_matches_apply_rope(sign):
    """One launch over 4 q + 2 k heads of packed [T, 8*D] rows, in place
    and out of place, against the dense-rows kernel; the 2 v heads are
    not touched."""
    from trainingjob_operator_amd.ops.functional import _rope_run
    Bq, S, H, HKV = 2, 256, 4, 2
    T, W, R = Bq * S, (H + 2 * HKV) * D, (H + HKV) * D
    g = _gen(3)
    x = _randn(g, T, W)
    inv_freq = _inv_freq()
    lib = native.load(require=True)
    heads = x.view(T, H + 2 * HKV, D)
    ref_q = _rope_run(heads[:, :H].contiguous(), inv_freq, S, sign)
    ref_k = _rope_run(heads[:, H:H + HKV].contiguous(), inv_freq, S, sign)
    ref = torch.cat([ref_q, ref_k], dim=1).reshape(T, R)

    # out of place, into a narrower packed buffer
    out = _sentinel(T, R)
    rc = lib.rope_packed(native.stream_ptr(), x.data_ptr(), out.data_ptr(),
                         inv_freq.data_ptr(), T, H + HKV, W, R, S, D, sign)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ref)

    # in place: q and k ranges rotated, v range bit-unchanged
    y = x.clone()
    rc = lib.rope_packed(native.stream_ptr(), y.data_ptr(), y.data_ptr(),
                         inv_freq.data_ptr(), T, H + HKV, W, W, S, D, sign)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(y[:, :R], ref)
    assert torch.equal(y[:, R:], x[:, R:])


def _one_step(packed: bool, monkeypatch):
    """One step of llama-smoke (2 layers) at micro_batch 2 x grad_accum 2;
    returns loss, parameters and how often the packed function ran."""
    from trainingjob_operator_amd.ops import attention
    from trainingjob_operator_amd.training import TrainConfig, Trainer
    with monkeypatch.context() as m:
        m.setenv("AITJ_ATTN_PACKED", "1" if packed else "0")
        # knobs that would silently route the step down the unpacked path
        for var in ("AITJ_SDPA_BACKEND", "AITJ_DISABLE_GQA", "AITJ_ATTN_BWD",
                    "AITJ_FP8_PROJ"):
            m.delenv(var, raising=False)
        calls = []
        real = attention._PackedRopeAttention.apply

        def counting_apply(*args):
            calls.append(tuple(args[0].shape))
            return real(*args)

        m.setattr(attention._PackedRopeAttention, "apply",
                  staticmethod(counting_apply))
        cfg = TrainConfig(model="llama-smoke", micro_batch=2, grad_accum=2,
                          seq_len=512)
        trainer = Trainer(cfg)
        loss = trainer.train_step().detach().clone()
        torch.cuda.synchronize()
        return loss, trainer.store.flat_param.detach().clone(), calls


def test_train_step_packed_equals_unpacked_bitwise(monkeypatch):
    """One llama-smoke step (head_dim 128, B=2, S=512, two micro-batches)
    from the same seed with and without the packed path: same loss bits,
    same parameter bits. The packed run must really take the packed
    kernels (once per layer per micro-batch), the other run never."""
    from trainingjob_operator_amd.models.config import LLAMA_SMOKE as cfg
    loss_p, params_p, calls_p = _one_step(True, monkeypatch)
    loss_u, params_u, calls_u = _one_step(False, monkeypatch)
    W = (cfg.num_heads + 2 * cfg.num_kv_heads) * cfg.head_dim
    assert calls_p == [(2, 512, W)] * (cfg.num_layers * 2), calls_p
    assert calls_u == []
    assert torch.equal(loss_p, loss_u), f"{loss_p.item()} vs {loss_u.item()}"
    assert torch.equal(params_p, params_u), (
        "params differ: max "
        f"{(params_p.float() - params_u.float()).abs().max()}")
