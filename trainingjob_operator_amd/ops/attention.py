"""Native MFMA flash attention (hip/attention.hip): hand-written CDNA4
forward AND backward, the default SDPA path for training.

Forwards:
  * v7 (S % 256 == 0, the production path): 8-wave swapped-operand
    32x32x16 MFMA, in-register softmax, 3-slot all-glds K/V ring with
    ONE raw barrier per tile, native GQA — 299 us vs the aotriton
    library's 425 at the flagship shape.
  * v5 (S % 64 == 0 fallback): 4-wave 16x16x32 kernel with the LDS P
    round-trip; requires equal head counts (GQA expanded by the caller).

Backward (S % 256 == 0): delta + dq + dv + dk kernels (fwd+bwd 2858 us
vs aotriton's 4140 — profiles/attention_kernel_notes.md). The forward
emits O + logsumexp at natural-log scale — exactly what
aten::_scaled_dot_product_flash_attention_backward consumes — so the
aten backward remains a drop-in fallback (AITJ_ATTN_BWD=aten, and the
automatic path for S % 256 != 0).

Block ops for context-parallel ring attention (parallel/cp.py; lengths
% 256 == 0, native GQA): flash_attention_block_fwd/_bwd run the
v7 forward and the dq/dv/dk kernels with a compile-time causal switch —
causal=True is the code above, bit for bit (S_q == S_kv); causal=False
visits every kv tile with no mask, for blocks wholly below the diagonal,
and may be rectangular: k.shape[2] != q.shape[2] routes to the rect
entries (attn_block_fwd_rect, attn_block_bwd_rect_ws; lse/delta
[B,H,S_q], dk/dv [B,HKV,S_kv,128], workspace by attn_bwd_ws_bytes_rect),
which the zig-zag ring needs for its half-shard steps. rope_packed_at
is rope_packed at shard positions (one or two position segments). The
backward takes lse and delta as inputs, so the ring passes the merged
(global) ones; flash_attention_delta exposes the delta kernel;
attn_merge_ folds one block's (o, lse) into an fp32 running pair.
ops/reference.py holds fp32 torch twins of all four.

Scheduling (hip/attention.hip, `attn_sched_block`): the v7 forward and the
dq/dv/dk kernels launch on a 1-D grid and decode the block id to (row
block, head, batch). AITJ_ATTN_SCHED=legacy is the former order (row
blocks fastest, heavy-first only inside one head); balanced (the default)
is rank-major - every head's heaviest row block first - with each XCD
class (id % 8) holding equal work and whole kv heads. Results are
bit-identical between the two; `lib.attn_sched_decode` is the host copy
of the decode.

Split dK/dV: with AITJ_ATTN_BWD_SPLIT=1, or by the library's measured
rule with AITJ_ATTN_BWD_SPLIT=auto (GQA and too few kv workgroups to
balance the causal walk - see `attn_bwd_use_split`), dv and dk run one
workgroup per (kv block, q head, batch) into an fp32 workspace
[2,B,H,S,128] and `attn_bwd_reduce_kernel` sums each kv head's group in
fixed order and rounds once to bf16: deterministic, one rounding per
output as before, only the fp32 association differs from the unsplit
walk. That is enough to move a few thousand dk/dv values per layer pass
by one bf16 step, so a training step no longer reproduces the unsplit
run bit for bit; unset (or 0) therefore stays on the unsplit walk. The
wrappers here size the workspace with `lib.attn_bwd_ws_bytes(B, H, HKV,
S, causal)`, allocate it with torch.empty and call the `_ws` entries
(`attn_bwd_ws`, `attn_bwd_strided_ws`, `attn_block_bwd_ws`), which launch
nothing and return nonzero on a missing or short workspace. The entries
without `_ws` keep their signatures, decide the same way and take a
stream-ordered transient workspace themselves; they refuse a capturing
stream. Both variables are read on every call.

Folded dK/dV strips (`attn_bwd_strips`, `attn_bwd_use_fold`): a causal
dv/dk workgroup may pair the four 32-row kv strips of half-block i (of
128 rows) with those of half-block S/128-1-i instead of owning 256
neighbouring rows, so that every workgroup does the same causal work and
each SIMD runs one active wave until the walk reaches its light strip.
Every strip keeps its accumulation order: dk and dv are bit-identical
either way. AITJ_ATTN_BWD_FOLD=0 never folds, 1 always folds causal
launches, unset follows the measured rule (fold when the dv/dk grid has at
most one workgroup per CU - the flagship step does); read on every call.
`lib.attn_bwd_strips_decode` is the host copy of the ownership function.

Paired dK/dV strips (`attn_bwd_pair`, AITJ_ATTN_BWD_FOLD=2): the causal
unsplit `attn_bwd_dv_pair_kernel` / `attn_bwd_dk_pair_kernel` run the two
half-blocks of the fold one after the other, and the two waves of a SIMD
(w and w+4) share one strip: each computes one 32-row half of every q
tile, they swap the packed P / dS fragments through 16 KB of LDS, and each
accumulates two of the strip's four 32-column d subtiles over all four q
chunks. Every accumulator keeps its order, so dk and dv are bit-identical
again, and every workgroup walks S/64 + 2 tile steps per q head with both
waves of each SIMD busy. Split and non-causal launches never pair (2 then
means unset). Unset follows the measured rule per kernel: where the grid
has at most one workgroup per CU dk pairs and dv folds (the flagship step
does), above that both keep the identity. `lib.attn_bwd_pair_decode` is
the host copy of the ownership function and `lib.attn_bwd_fold_mode` says
which ownership a launch of a given shape gets.

Document-masked attention (`flash_attention_docs`, `packed_rope_attention(
..., doc_bounds=)`; layouts in ops/docmask.py): a window that holds several
documents attends causally inside each one. The layout is one int32 tensor
bounds [2,B,S] (first and last window index of every token's document); q
sees kv iff bounds[0,b,q] <= kv <= q, shared by all heads, RoPE positions
window-absolute (RoPE is relative, so scores inside a document do not
depend on its offset). The document mode of `attn_fwd_v7_kernel` and
`attn_bwd_dq_kernel` is the v7 forward and dq with one int32 load per lane
and `kvr < start` next to the causal test; the kv walk starts at the tile of the q block's
first document start, a wave sits out tiles before the smallest start of
its rows, and every tile that a start cuts is masked.
That of `attn_bwd_dv_kernel` / `attn_bwd_dk_kernel` loads end per kv row,
masks q > end and stops the q walk at the tile of the kv block's last document
end. They use identity strip ownership, unsplit, with no workspace:
AITJ_ATTN_BWD_FOLD and AITJ_ATTN_BWD_SPLIT do not apply to document
launches (AITJ_ATTN_SCHED does). One document of S tokens computes the
causal result bit for bit; block-aligned documents compute what separate
causal calls compute, bit for bit. All ranges derived from bounds are
clamped in the kernels (`lib.attn_doc_tiles_decode` is the host copy), so
any int32 content is memory-safe and only valid layouts are exact;
`check_doc_bounds` validates one, with a sync, for tests. The causal
entries, the block ops and the ring are untouched. ops/reference.py holds
the fp32 twins (`attention_doc_fwd`, `attention_doc_bwd`). Shapes the
kernels do not cover (CPU, other head sizes, S % 256 != 0) fall back, in
packed_rope_attention, to SDPA under `doc_mask_dense(bounds)`.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from . import native
from .docmask import doc_mask_dense


def _supported(q: torch.Tensor, k: torch.Tensor) -> bool:
    B, H, S, D = q.shape
    HKV = k.shape[1]
    return (q.dtype == torch.bfloat16 and D == 128
            and (S % 256 == 0 or (S % 64 == 0 and HKV == H))
            and q.stride(-1) == 1 and k.stride(-1) == 1
            and H % HKV == 0)


def _bwd_workspace(lib, B, H, HKV, S, causal, device):
    """The fp32 workspace the native backward wants for this call: (tensor
    or None, data pointer, bytes). Sized by the library's own rule
    (attn_bwd_ws_bytes, 0 when dv/dk run unsplit) and taken from torch's
    allocator, which orders it on the current stream and keeps it in the
    capture pool while a graph records."""
    nbytes = lib.attn_bwd_ws_bytes(B, H, HKV, S, 1 if causal else 0)
    if nbytes <= 0:
        return None, None, 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws, ws.data_ptr(), nbytes


def _bwd_workspace_rect(lib, B, H, HKV, S_q, S_kv, device):
    """_bwd_workspace for a non-causal S_q x S_kv block
    (attn_bwd_ws_bytes_rect: the partials are kv rows)."""
    nbytes = lib.attn_bwd_ws_bytes_rect(B, H, HKV, S_q, S_kv, 0)
    if nbytes <= 0:
        return None, None, 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws, ws.data_ptr(), nbytes


def _run_fwd(q, k, v, scale):
    B, H, S, D = q.shape
    HKV = k.shape[1]
    lib = native.load(require=True)
    out = torch.empty(B, H, S, D, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
    rc = lib.attn_fwd(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        out.data_ptr(), lse.data_ptr(),
        q.stride(0), q.stride(1), q.stride(2),
        k.stride(0), k.stride(1), k.stride(2),
        v.stride(0), v.stride(1), v.stride(2),
        B, H, HKV, S, scale)
    native.check_rc(rc, "attn_fwd", f"B={B} H={H} HKV={HKV} S={S}")
    return out, lse


class _NativeFlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        out, lse = _run_fwd(q, k, v, scale)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, out, lse = ctx.saved_tensors
        B, H, S, D = q.shape
        if S % 256 == 0 and os.environ.get("AITJ_ATTN_BWD") != "aten":
            return (*_native_backward(q, k, v, out, lse, gout, ctx.scale),
                    None)
        # None -> undefined Tensor: selects the dense (non-varlen) path in
        # the aten flash backward (empty tensors select varlen and fail).
        philox = torch.empty(0, dtype=torch.int64, device=q.device)
        dq, dk, dv = torch.ops.aten._scaled_dot_product_flash_attention_backward(
            gout.contiguous(), q, k, v, out, lse,
            None, None, S, S, 0.0, True,
            philox, philox, scale=ctx.scale)
        return dq, dk, dv, None


def _native_backward(q, k, v, out, lse, gout, scale):
    """Hand-written CDNA4 flash backward (delta + dq + dv + dk kernels)."""
    B, H, S, D = q.shape
    HKV = k.shape[1]
    lib = native.load(require=True)
    dout = gout.contiguous()
    delta = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
    dq = torch.empty(B, H, S, D, dtype=torch.bfloat16, device=q.device)
    dk = torch.empty(B, HKV, S, D, dtype=torch.bfloat16, device=q.device)
    dv = torch.empty(B, HKV, S, D, dtype=torch.bfloat16, device=q.device)
    ws, ws_ptr, ws_bytes = _bwd_workspace(lib, B, H, HKV, S, True, q.device)
    rc = lib.attn_bwd_ws(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
        dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
        q.stride(0), q.stride(1), q.stride(2),
        k.stride(0), k.stride(1), k.stride(2),
        v.stride(0), v.stride(1), v.stride(2),
        B, H, HKV, S, scale, ws_ptr, ws_bytes)
    native.check_rc(rc, "attn_bwd_ws", f"B={B} H={H} HKV={HKV} S={S}")
    return dq, dk, dv


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    scale: Optional[float] = None) -> torch.Tensor:
    """Causal flash attention over [B, H, S, D=128] bf16; k/v may carry
    fewer (GQA) heads when S % 256 == 0 (the v6 kernel maps them)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    assert _supported(q, k), (
        f"native flash attention needs bf16, D=128, S%256==0 (or S%64==0 "
        f"with equal head counts), d-contiguous strides; got {q.shape} "
        f"{q.dtype} kv={k.shape}")
    return _NativeFlashAttention.apply(q, k, v, scale)


# ---------------------------------------------------------------------------
# Document-masked causal attention (bounds: ops/docmask.py)
# ---------------------------------------------------------------------------

def _check_bounds(bounds, B: int, S: int, device) -> None:
    """Shape, dtype and placement only: the kernels clamp every range they
    derive from the content, so no value needs a (syncing) look."""
    assert isinstance(bounds, torch.Tensor), \
        f"bounds must be an int32 [2,B,S] tensor, got {type(bounds).__name__}"
    assert bounds.dtype == torch.int32 and tuple(bounds.shape) == (2, B, S) \
        and bounds.is_contiguous() and bounds.device == device, (
            f"bounds must be contiguous int32 [2,{B},{S}] on {device}, got "
            f"{bounds.dtype} {tuple(bounds.shape)} on {bounds.device}")


def docs_supported(q: torch.Tensor, k: torch.Tensor) -> bool:
    """Shapes the document kernels cover: GPU bf16 [B,H,S,128] /
    [B,HKV,S,128], S % 256 == 0, H % HKV == 0, unit last stride."""
    return block_supported(q, k) and k.shape[2] == q.shape[2]


def _run_doc_fwd(q, k, v, bounds, scale):
    B, H, S, D = q.shape
    HKV = k.shape[1]
    _check_bounds(bounds, B, S, q.device)
    lib = native.load(require=True)
    out = torch.empty(B, H, S, D, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
    st = native.stride_array(_tri(q), _tri(k), _tri(v), _tri(out))
    rc = lib.attn_doc_fwd_strided(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        out.data_ptr(), lse.data_ptr(), bounds.data_ptr(), st,
        B, H, HKV, S, scale)
    native.check_rc(rc, "attn_doc_fwd_strided",
                    f"B={B} H={H} HKV={HKV} S={S}")
    return out, lse


def _native_doc_backward(q, k, v, out, lse, gout, bounds, scale):
    """delta + dq + dv + dk under the document mask (identity strip
    ownership, unsplit, no workspace)."""
    B, H, S, D = q.shape
    HKV = k.shape[1]
    _check_bounds(bounds, B, S, q.device)
    lib = native.load(require=True)
    dout = gout.contiguous()
    delta = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
    dq = torch.empty(B, H, S, D, dtype=torch.bfloat16, device=q.device)
    dk = torch.empty(B, HKV, S, D, dtype=torch.bfloat16, device=q.device)
    dv = torch.empty(B, HKV, S, D, dtype=torch.bfloat16, device=q.device)
    st = native.stride_array(_tri(q), _tri(k), _tri(v), _tri(out),
                             _tri(dout), _tri(dq), _tri(dk), _tri(dv))
    rc = lib.attn_doc_bwd_strided(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
        dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), bounds.data_ptr(), st,
        B, H, HKV, S, scale)
    native.check_rc(rc, "attn_doc_bwd_strided",
                    f"B={B} H={H} HKV={HKV} S={S}")
    return dq, dk, dv


class _NativeDocAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, bounds, scale):
        out, lse = _run_doc_fwd(q, k, v, bounds, scale)
        ctx.save_for_backward(q, k, v, out, lse, bounds)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, out, lse, bounds = ctx.saved_tensors
        return (*_native_doc_backward(q, k, v, out, lse, gout, bounds,
                                      ctx.scale), None, None)


def flash_attention_docs(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                         bounds: torch.Tensor,
                         scale: Optional[float] = None) -> torch.Tensor:
    """Document-masked causal flash attention over [B,H,S,128] bf16 with
    k, v [B,HKV,S,128] (native GQA), S % 256 == 0: q row s sees kv rows
    bounds[0,b,s] .. s. bounds is a contiguous int32 [2,B,S] on q's device
    (ops/docmask.py); only its shape is checked here, the kernels are safe
    for any content and exact for a valid layout. Positions fed to RoPE
    before this call stay window-absolute: RoPE is relative, so scores
    inside a document do not depend on its offset."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    assert docs_supported(q, k) and v.shape == k.shape and v.is_cuda \
        and v.dtype == q.dtype and v.stride(-1) == 1, (
            f"flash_attention_docs needs GPU bf16 [B,H,S,128] / [B,HKV,S,128] "
            f"with S%256==0, H%HKV==0, d-contiguous strides; got "
            f"{tuple(q.shape)} {q.dtype} kv={tuple(k.shape)}")
    _check_bounds(bounds, q.shape[0], q.shape[2], q.device)
    return _NativeDocAttention.apply(q, k, v, bounds, scale)


def flash_attention_docs_fwd_only(q, k, v, bounds, scale=None):
    """Forward-only entry returning (out, lse) for tests/benchmarks."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    return _run_doc_fwd(q, k, v, bounds, scale)


# ---------------------------------------------------------------------------
# RoPE + attention straight on the packed QKV projection output
# ---------------------------------------------------------------------------

def _bhsd_strides(row: int, D: int, S: int):
    """(batch, head, row) strides of a head range inside packed rows of
    `row` elements — a [B,S,heads,D] buffer read as [B,heads,S,D]."""
    return (S * row, D, row)


def _rope_packed(lib, x, out, inv_freq, n_tokens, n_rot, x_row, out_row,
                 S, D, sign):
    assert inv_freq.device == x.device and inv_freq.dtype == torch.float32, (
        f"inv_freq must be fp32 on {x.device}, got "
        f"{inv_freq.dtype}@{inv_freq.device}")
    rc = lib.rope_packed(native.stream_ptr(), x.data_ptr(), out.data_ptr(),
                         inv_freq.data_ptr(), n_tokens, n_rot, x_row,
                         out_row, S, D, sign)
    native.check_rc(rc, "rope_packed", f"D={D} n_rot={n_rot} row={x_row}")


def rope_packed_at(x, out, inv_freq, n_rot, S, seg_len, pos_a, pos_b=0,
                   sign=1.0, D=128):
    """RoPE over heads [0, n_rot) of the packed rows of x [B,S,row] into
    out [B,S,row'] (bf16, contiguous, may be the same tensor) at shard
    positions: local row s sits at pos_a + s while s < seg_len, then at
    pos_b + (s - seg_len). S == seg_len is a contiguous shard at offset
    pos_a, S == 2*seg_len the zig-zag shard; the launcher refuses anything
    else. Rounds exactly as the dense RoPE kernels do."""
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() \
        and out.dtype == torch.bfloat16 and out.is_contiguous() \
        and x.dim() == 3 and out.shape[:2] == x.shape[:2] \
        and x.shape[1] == S, (x.shape, x.dtype, out.shape, out.dtype, S)
    assert inv_freq.device == x.device and inv_freq.dtype == torch.float32, (
        f"inv_freq must be fp32 on {x.device}, got "
        f"{inv_freq.dtype}@{inv_freq.device}")
    lib = native.load(require=True)
    rc = lib.rope_packed_at(native.stream_ptr(), x.data_ptr(), out.data_ptr(),
                            inv_freq.data_ptr(), x.shape[0] * S, n_rot,
                            x.shape[2], out.shape[2], S, D, sign, seg_len,
                            pos_a, pos_b)
    native.check_rc(rc, "rope_packed_at",
                    f"D={D} n_rot={n_rot} S={S} seg_len={seg_len} "
                    f"pos=({pos_a},{pos_b})")


class _PackedRopeAttention(torch.autograd.Function):
    """qkv [B,S,(H+2HKV)*128] -> o [B,S,H*128] with no layout copies: one
    RoPE launch over the q|k head range, the v7 forward reading q/k/v and
    writing o through strides; the backward kernels write their head
    ranges of one dqkv buffer, un-rotated in place by one RoPE launch.
    With bounds (a document layout, ops/docmask.py) the same buffers and
    strides go through the document entries instead."""

    @staticmethod
    def forward(ctx, qkv, inv_freq, n_heads, n_kv_heads, scale, bounds=None):
        B, S, W = qkv.shape
        D = 128
        H, HKV = n_heads, n_kv_heads
        assert W == (H + 2 * HKV) * D
        qkv = qkv.contiguous()
        lib = native.load(require=True)
        R = (H + HKV) * D
        rot = torch.empty(B, S, R, dtype=torch.bfloat16, device=qkv.device)
        _rope_packed(lib, qkv, rot, inv_freq, B * S, H + HKV, W, R, S, D, 1.0)
        o = torch.empty(B, S, H * D, dtype=torch.bfloat16, device=qkv.device)
        lse = torch.empty(B, H, S, dtype=torch.float32, device=qkv.device)
        esz = qkv.element_size()
        st = native.stride_array(
            _bhsd_strides(R, D, S), _bhsd_strides(R, D, S),
            _bhsd_strides(W, D, S), _bhsd_strides(H * D, D, S))
        if bounds is None:
            rc = lib.attn_fwd_strided(
                native.stream_ptr(), rot.data_ptr(),
                rot.data_ptr() + H * D * esz,
                qkv.data_ptr() + (H + HKV) * D * esz,
                o.data_ptr(), lse.data_ptr(), st, B, H, HKV, S, scale)
            native.check_rc(rc, "attn_fwd_strided",
                            f"B={B} H={H} HKV={HKV} S={S}")
        else:
            _check_bounds(bounds, B, S, qkv.device)
            rc = lib.attn_doc_fwd_strided(
                native.stream_ptr(), rot.data_ptr(),
                rot.data_ptr() + H * D * esz,
                qkv.data_ptr() + (H + HKV) * D * esz,
                o.data_ptr(), lse.data_ptr(), bounds.data_ptr(), st,
                B, H, HKV, S, scale)
            native.check_rc(rc, "attn_doc_fwd_strided",
                            f"B={B} H={H} HKV={HKV} S={S}")
        ctx.save_for_backward(rot, qkv, o, lse, inv_freq, bounds)
        ctx.dims = (B, S, H, HKV, D)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, gout):
        rot, qkv, o, lse, inv_freq, bounds = ctx.saved_tensors
        B, S, H, HKV, D = ctx.dims
        W, R = (H + 2 * HKV) * D, (H + HKV) * D
        lib = native.load(require=True)
        # the o_proj GEMM hands back a dense [B,S,H*D] gradient
        dout = gout if gout.is_contiguous() else gout.contiguous()
        delta = torch.empty(B, H, S, dtype=torch.float32, device=qkv.device)
        dqkv = torch.empty(B, S, W, dtype=torch.bfloat16, device=qkv.device)
        esz = qkv.element_size()
        rs, ws, os_ = (_bhsd_strides(R, D, S), _bhsd_strides(W, D, S),
                       _bhsd_strides(H * D, D, S))
        st = native.stride_array(rs, rs, ws, os_, os_, ws, ws, ws)
        if bounds is None:
            ws, ws_ptr, ws_bytes = _bwd_workspace(lib, B, H, HKV, S, True,
                                                  qkv.device)
            rc = lib.attn_bwd_strided_ws(
                native.stream_ptr(), rot.data_ptr(),
                rot.data_ptr() + H * D * esz,
                qkv.data_ptr() + (H + HKV) * D * esz,
                o.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                delta.data_ptr(),
                dqkv.data_ptr(), dqkv.data_ptr() + H * D * esz,
                dqkv.data_ptr() + (H + HKV) * D * esz,
                st, B, H, HKV, S, ctx.scale, ws_ptr, ws_bytes)
            native.check_rc(rc, "attn_bwd_strided_ws",
                            f"B={B} H={H} HKV={HKV} S={S}")
        else:
            rc = lib.attn_doc_bwd_strided(
                native.stream_ptr(), rot.data_ptr(),
                rot.data_ptr() + H * D * esz,
                qkv.data_ptr() + (H + HKV) * D * esz,
                o.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                delta.data_ptr(),
                dqkv.data_ptr(), dqkv.data_ptr() + H * D * esz,
                dqkv.data_ptr() + (H + HKV) * D * esz,
                bounds.data_ptr(), st, B, H, HKV, S, ctx.scale)
            native.check_rc(rc, "attn_doc_bwd_strided",
                            f"B={B} H={H} HKV={HKV} S={S}")
        _rope_packed(lib, dqkv, dqkv, inv_freq, B * S, H + HKV, W, W, S, D,
                     -1.0)
        return dqkv, None, None, None, None, None


def packed_supported(qkv: torch.Tensor, n_heads: int, n_kv_heads: int) -> bool:
    """Shapes the packed path covers: GPU bf16 [B,S,(H+2HKV)*128] with
    S % 256 == 0 (the v7 forward + native backward kernels)."""
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3
            and qkv.shape[1] % 256 == 0 and n_heads % n_kv_heads == 0
            and qkv.shape[2] == (n_heads + 2 * n_kv_heads) * 128)


def unpacked_rope_attention(qkv, inv_freq, n_heads, n_kv_heads, scale=None,
                            doc_bounds=None):
    """The copying composition packed_rope_attention replaces (and its
    fallback): split, dense q/k, RoPE each, [B,h,S,D] attention, transpose
    back. Any head_dim; native flash attention where it applies, torch
    SDPA elsewhere. With doc_bounds the attention is flash_attention_docs
    where that applies and SDPA under doc_mask_dense(doc_bounds) elsewhere;
    RoPE positions stay window-absolute either way."""
    from .functional import apply_rope
    B, S, W = qkv.shape
    D = W // (n_heads + 2 * n_kv_heads)
    q, k, v = qkv.split([n_heads * D, n_kv_heads * D, n_kv_heads * D], dim=-1)
    q = q.reshape(B, S, n_heads, D).contiguous()
    k = k.reshape(B, S, n_kv_heads, D).contiguous()
    v = v.reshape(B, S, n_kv_heads, D)
    q = apply_rope(q, inv_freq, S).transpose(1, 2)
    k = apply_rope(k, inv_freq, S).transpose(1, 2)
    v = v.transpose(1, 2)
    if doc_bounds is not None:
        if docs_supported(q, k):
            o = flash_attention_docs(q, k, v, doc_bounds, scale)
        else:
            o = torch.nn.functional.scaled_dot_product_attention(
                q, k, v, attn_mask=doc_mask_dense(doc_bounds), scale=scale,
                enable_gqa=n_heads != n_kv_heads)
    elif qkv.is_cuda and _supported(q, k):
        o = flash_attention(q, k, v, scale)
    else:
        o = torch.nn.functional.scaled_dot_product_attention(
            q, k, v, is_causal=True, scale=scale,
            enable_gqa=n_heads != n_kv_heads)
    return o.transpose(1, 2).reshape(B, S, n_heads * D)


def packed_rope_attention(qkv: torch.Tensor, inv_freq: torch.Tensor,
                          n_heads: int, n_kv_heads: int,
                          scale: Optional[float] = None,
                          doc_bounds: Optional[torch.Tensor] = None
                          ) -> torch.Tensor:
    """Causal RoPE attention on the fused projection output:
    qkv [B,S,(H+2HKV)*D] -> o [B,S,H*D]. D = 128 bf16 on the GPU with
    S % 256 == 0 runs the copy-free packed kernels; everything else (CPU,
    other head sizes, other S) runs the unpacked composition. doc_bounds
    (int32 [2,B,S], ops/docmask.py) masks attention at document boundaries:
    the packed layout then goes through the document entries, still with no
    copies, and the fallback is SDPA under the dense mask. None is the
    causal path, unchanged."""
    if packed_supported(qkv, n_heads, n_kv_heads):
        if scale is None:
            scale = 1.0 / math.sqrt(128)
        if doc_bounds is None:
            return _PackedRopeAttention.apply(qkv, inv_freq, n_heads,
                                              n_kv_heads, scale)
        return _PackedRopeAttention.apply(qkv, inv_freq, n_heads, n_kv_heads,
                                          scale, doc_bounds)
    return unpacked_rope_attention(qkv, inv_freq, n_heads, n_kv_heads, scale,
                                   doc_bounds)


def flash_attention_fwd_only(q, k, v, scale=None):
    """Forward-only entry returning (out, lse) for tests/benchmarks."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    return _run_fwd(q, k, v, scale)


def _fwd_entry(entry: str, q, k, v, scale=None, kv_heads_arg: bool = True):
    """Call one forward A/B entry of the library by name -> (out, lse). Every
    entry takes (batch, heads, kv heads, S); v5 has no GQA and no kv heads."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    B, H, S, D = q.shape
    dims = (B, H, k.shape[1], S) if kv_heads_arg else (B, H, S)
    lib = native.load(require=True)
    out = torch.empty(B, H, S, D, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
    rc = getattr(lib, entry)(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        out.data_ptr(), lse.data_ptr(),
        q.stride(0), q.stride(1), q.stride(2),
        k.stride(0), k.stride(1), k.stride(2),
        v.stride(0), v.stride(1), v.stride(2),
        *dims, scale)
    native.check_rc(rc, entry, f"B={B} H={H} S={S}")
    return out, lse


def flash_attention_fwd_nw8(q, k, v, scale=None):
    """The 8-wave (BM=256) instantiation, kept callable for A/B."""
    return _fwd_entry("attn_fwd_nw8", q, k, v, scale)


def flash_attention_fwd_v7(q, k, v, scale=None):
    """The 3-deep all-glds pipeline forward (A/B candidate)."""
    return _fwd_entry("attn_fwd_v7", q, k, v, scale)


def flash_attention_fwd_v5(q, k, v, scale=None):
    """The 4-wave v5 forward, kept callable for A/B benchmarking."""
    return _fwd_entry("attn_fwd_v5", q, k, v, scale, kv_heads_arg=False)


# ---------------------------------------------------------------------------
# Block ops for context-parallel ring attention (parallel/cp.py)
# ---------------------------------------------------------------------------

def block_supported(q: torch.Tensor, k: torch.Tensor) -> bool:
    """Shapes the native block ops cover: GPU bf16 [B,H,S_q,128] /
    [B,HKV,S_kv,128] with S_q % 256 == 0 and S_kv % 256 == 0, H % HKV == 0,
    unit last stride. S_q != S_kv is a rectangular block, non-causal only
    (the ops themselves refuse causal=True there)."""
    if q.dim() != 4 or k.dim() != 4:
        return False
    B, H, S, D = q.shape
    HKV, Skv = k.shape[1], k.shape[2]
    return (q.is_cuda and k.is_cuda and q.dtype == torch.bfloat16
            and k.dtype == torch.bfloat16 and D == 128 and k.shape[-1] == 128
            and S > 0 and S % 256 == 0 and Skv > 0 and Skv % 256 == 0
            and H % HKV == 0 and q.stride(-1) == 1 and k.stride(-1) == 1)


def _tri(t: torch.Tensor):
    assert t.stride(-1) == 1, f"last stride must be 1, got {t.stride()}"
    return (t.stride(0), t.stride(1), t.stride(2))


def _block_dims(q, k, v, causal, op):
    """(B, H, HKV, S_q, S_kv) of one block call."""
    assert block_supported(q, k) and v.shape == k.shape \
        and v.dtype == q.dtype and v.is_cuda and v.stride(-1) == 1, (
            f"{op} needs GPU bf16 [B,H,S_q,128] / [B,HKV,S_kv,128] with "
            f"S_q%256==0 and S_kv%256==0; got q {tuple(q.shape)} {q.dtype} "
            f"kv {tuple(k.shape)} {tuple(v.shape)}")
    B, H, S, _ = q.shape
    assert not (causal and k.shape[2] != S), (
        f"{op}: a causal block is square, got S_q={S} S_kv={k.shape[2]}")
    return B, H, k.shape[1], S, k.shape[2]


def flash_attention_block_fwd(q, k, v, causal: bool,
                              scale: Optional[float] = None):
    """One attention block: causal=True is the S x S diagonal block of a
    longer causal problem (bit-identical to the dense forward), causal=False
    a block wholly below the diagonal, S_q x S_kv with k.shape[2] != q.shape[2]
    allowed (the rect entries; a square call takes the square entry as
    before). Returns (o bf16 [B,H,S_q,128], lse fp32 [B,H,S_q], natural
    log)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    B, H, HKV, S, Skv = _block_dims(q, k, v, causal,
                                    "flash_attention_block_fwd")
    lib = native.load(require=True)
    out = torch.empty(B, H, S, 128, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
    st = native.stride_array(_tri(q), _tri(k), _tri(v), _tri(out))
    if Skv != S:
        rc = lib.attn_block_fwd_rect(
            native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
            out.data_ptr(), lse.data_ptr(), st, B, H, HKV, S, Skv, scale, 0)
        native.check_rc(rc, "attn_block_fwd_rect",
                        f"B={B} H={H} HKV={HKV} S_q={S} S_kv={Skv}")
        return out, lse
    rc = lib.attn_block_fwd(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        out.data_ptr(), lse.data_ptr(), st, B, H, HKV, S, scale,
        1 if causal else 0)
    native.check_rc(rc, "attn_block_fwd", f"B={B} H={H} HKV={HKV} S={S}")
    return out, lse


def flash_attention_delta(out: torch.Tensor,
                          dout: torch.Tensor) -> torch.Tensor:
    """delta[b,h,s] = sum_d out*dout (fp32 [B,H,S]) from bf16
    [B,H,S,128] operands — computed once per ring backward from the
    merged output."""
    assert (out.is_cuda and out.dtype == torch.bfloat16
            and dout.dtype == torch.bfloat16 and out.shape == dout.shape
            and out.dim() == 4 and out.shape[-1] == 128
            and out.shape[2] % 16 == 0), (out.shape, out.dtype, dout.dtype)
    B, H, S, _ = out.shape
    lib = native.load(require=True)
    delta = torch.empty(B, H, S, dtype=torch.float32, device=out.device)
    st = native.stride_array(_tri(out), _tri(dout))
    rc = lib.attn_delta(native.stream_ptr(), out.data_ptr(), dout.data_ptr(),
                        delta.data_ptr(), st, B, H, S)
    native.check_rc(rc, "attn_delta", f"B={B} H={H} S={S}")
    return delta


def flash_attention_block_bwd(q, k, v, dout, lse, delta, causal: bool,
                              scale: Optional[float] = None):
    """dq [B,H,S_q,128], dk, dv [B,HKV,S_kv,128] (bf16) of one block. lse
    and delta (fp32 [B,H,S_q]) are inputs: the block's own, or the merged
    global ones when the block is one of several a q row attends to.
    S_kv != S_q (causal=False only) takes the rect entry and sizes the
    workspace by its rule."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    B, H, HKV, S, Skv = _block_dims(q, k, v, causal,
                                    "flash_attention_block_bwd")
    assert dout.shape == q.shape and dout.dtype == torch.bfloat16
    assert lse.shape == (B, H, S) and delta.shape == (B, H, S)
    assert lse.dtype == torch.float32 and delta.dtype == torch.float32
    lib = native.load(require=True)
    if dout.stride(-1) != 1:
        dout = dout.contiguous()
    lse, delta = lse.contiguous(), delta.contiguous()
    dq = torch.empty(B, H, S, 128, dtype=torch.bfloat16, device=q.device)
    dk = torch.empty(B, HKV, Skv, 128, dtype=torch.bfloat16, device=q.device)
    dv = torch.empty(B, HKV, Skv, 128, dtype=torch.bfloat16, device=q.device)
    st = native.stride_array(_tri(q), _tri(k), _tri(v), _tri(dout),
                             _tri(dq), _tri(dk), _tri(dv))
    if Skv != S:
        ws, ws_ptr, ws_bytes = _bwd_workspace_rect(lib, B, H, HKV, S, Skv,
                                                   q.device)
        rc = lib.attn_block_bwd_rect_ws(
            native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
            dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
            dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), st,
            B, H, HKV, S, Skv, scale, 0, ws_ptr, ws_bytes)
        native.check_rc(rc, "attn_block_bwd_rect_ws",
                        f"B={B} H={H} HKV={HKV} S_q={S} S_kv={Skv}")
        return dq, dk, dv
    ws, ws_ptr, ws_bytes = _bwd_workspace(lib, B, H, HKV, S, causal,
                                          q.device)
    rc = lib.attn_block_bwd_ws(
        native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
        dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), st,
        B, H, HKV, S, scale, 1 if causal else 0, ws_ptr, ws_bytes)
    native.check_rc(rc, "attn_block_bwd_ws", f"B={B} H={H} HKV={HKV} S={S}")
    return dq, dk, dv


def attn_merge_(o_acc, lse_acc, o_blk, lse_blk) -> None:
    """In place: fold (o_blk bf16, lse_blk) into the running fp32 pair
    (o_acc [B,H,S,128], lse_acc [B,H,S]). Start from o=0, lse=-inf."""
    B, H, S, D = o_acc.shape
    assert (o_acc.is_cuda and D == 128 and o_acc.dtype == torch.float32
            and lse_acc.dtype == torch.float32
            and lse_blk.dtype == torch.float32
            and o_blk.dtype == torch.bfloat16
            and o_acc.is_contiguous() and lse_acc.is_contiguous()
            and o_blk.shape == o_acc.shape
            and lse_acc.shape == (B, H, S) and lse_blk.shape == (B, H, S)), (
        o_acc.shape, o_acc.dtype, o_blk.shape, o_blk.dtype, lse_acc.shape,
        lse_blk.shape)
    lib = native.load(require=True)
    lse_blk = lse_blk.contiguous()
    st = native.stride_array(_tri(o_blk))
    rc = lib.attn_merge(native.stream_ptr(), o_acc.data_ptr(),
                        lse_acc.data_ptr(), o_blk.data_ptr(),
                        lse_blk.data_ptr(), st, B, H, S)
    native.check_rc(rc, "attn_merge", f"B={B} H={H} S={S}")
