"""Context parallelism: ring attention over sequence-sharded activations.

The last parallel axis in the family (DP/TP/SP/PP/EP/PS are siblings in
this package): every rank holds a FULL replica of the weights but only a
contiguous S/cp block of the sequence. Everything except attention is
token-local (embedding, norms, MLP, loss), so the one distributed op is
attention itself: K/V blocks circulate around the ring while each rank's
Q stays put, partial softmax state merging exactly like flash attention
merges tiles (running max + sum-of-exp + rescaled accumulator). Causality
means rank r only attends blocks j <= r — later blocks still transit the
ring (uniform communication) but skip compute.

The backward is a second ring pass: dK/dV accumulators travel WITH their
K/V blocks (each visiting rank adds its contribution; after cp hops the
block and its gradient are home), while dQ accumulates locally. P is
recomputed per block from the saved logsumexp, flash-style, so activation
memory stays O(Sb) per rank.

xGMI mapping: ring neighbor exchange is exactly one point-to-point link
per hop (7 links x ~153 GB/s per MI355X), the communication pattern ring
attention was designed for; compute of block t overlaps the transit of
block t+1 when the blocks are large enough to cover link latency.

Distinct from sequence parallelism (sp.py): SP sharding spans the TP
group and gathers the FULL sequence back for attention (it saves memory
on norms/residuals only); CP never materializes the full sequence
anywhere — it is how a context longer than one GPU's activation budget
trains at all.

Two implementations of the per-block math sit under the same ring
schedule, chosen by AITJ_CP_ATTN:

  * block (what `auto`, the default, takes when ops.attention.
    block_supported holds for the local shard: GPU, bf16, D=128,
    Sb % 256 == 0): every visited block is one call of the native flash
    kernels — flash_attention_block_fwd (causal on the diagonal block,
    non-causal below it) giving (o_j, lse_j), folded into an fp32
    (o, lse) accumulator by attn_merge_; the backward computes delta once
    from the merged output and calls flash_attention_block_bwd per block
    with the GLOBAL lse and delta. No [Sb,Sb] tensor exists anywhere, and
    K/V and the travelling fp32 dK/dV keep their HKV heads (GQA is native
    in the kernels), so a Llama-3 32:8 hop moves a quarter of the bytes.
    AITJ_CP_ATTN=block forces this structure everywhere, on the fp32 torch
    twins in ops/reference.py where the native ops do not apply — that is
    how the gloo tests reach it on CPU.
  * legacy (AITJ_CP_ATTN=legacy, and what `auto` falls back to): fp32
    torch.matmul block math with an explicit [B,H,Sb,Sb] score tensor and
    GQA expanded before the ring.

Sharding layout (the `layout` argument of ring_attention, CPAttention,
CPBlock, CPLlamaModel and CPTrainer; --cp-layout / AITJ_CP_LAYOUT in the
launcher): "contiguous", the default, is the rule above — rank r visits
r+1 blocks, so a compute-then-shift ring waits cp - 0.5 block units for
cp/2 of mean work. "zigzag" cuts the sequence into 2*cp chunks and gives
rank r chunks r and 2cp-1-r; every rank then does the same work at every
step. `cp_schedule(layout, n, r)` is the single statement of both: one
(j, q_part, kv_part, causal) per ring step. A zig-zag step is the causal
Sb x Sb block when the shard meets itself, all q rows x the low half of
the visiting K/V for j < r, the high half of the q rows x the whole
visiting K/V for j > r — rectangular non-causal blocks, which the native
block ops take when Sb/2 % 256 == 0. The forward keeps one fp32 (o, lse)
pair per half; in the backward the travelling dK/dV receive only their
low half at j < r steps. Zig-zag exists on the block structure only
(native ops or their twins); AITJ_CP_ATTN=legacy with it raises.
`cp_shard_positions` / `cp_unshard` map local rows to global tokens and
back; CPLlamaModel.forward(tokens) without targets returns logits in
shard order.

Packed op: where the native block ops apply, a zig-zag shard on the GPU
(and a contiguous one under AITJ_CP_PACKED=1, read on every call) runs
_PackedCPAttention on the projection output [B,Sb,(H+2HKV)*128]: one
rope_packed_at launch at the shard's positions, block ops on strided views
(no split/reshape/transpose copies), gradients into the head ranges of one
dqkv buffer, un-rotated in place. A contiguous shard otherwise keeps the
torch _rope_offset path: the native rotation rounds differently, so
switching it would move today's bits.

Gloo-verified against the unsharded model (loss + every weight gradient)
in tests/test_cp_gloo.py, tests/test_cp_block_gloo.py and
tests/test_cp_zigzag_gloo.py; the native block ops are verified on the GPU
in tests/test_block_attention_gpu.py, tests/test_rect_block_attention_gpu.py
and tests/test_cp_zigzag_gpu.py. The multi-rank ring over RCCL has not been
timed (profiles/r04_ring_attention.md measures one rank's work on one GPU,
profiles/r07_zigzag_cp.md every virtual rank's schedule step by step).

No reference counterpart: the reference operator has no parallelism at
all (SURVEY.md §2.3 — replica counts are its only notion of scale).
"""
from __future__ import annotations

import math
import os
from typing import List, Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from ..models.config import LlamaConfig
from ..ops import fused_cross_entropy, fused_rmsnorm, make_inv_freq
from .tp import _group_size


def _ring_shift(tensors: List[torch.Tensor], group) -> List[torch.Tensor]:
    """Send every tensor to rank+1, receive from rank-1 (one xGMI hop).
    Even ranks send first, odd ranks receive first — no deadlock at any
    ring size (including 2, where isend/irecv pair up)."""
    n = _group_size(group)
    r = dist.get_rank(group)
    dst = dist.get_global_rank(group, (r + 1) % n) if group else (r + 1) % n
    src = dist.get_global_rank(group, (r - 1) % n) if group else (r - 1) % n
    sends = [t.contiguous() for t in tensors]
    outs = [torch.empty_like(t) for t in sends]
    reqs = []
    if r % 2 == 0:
        for t in sends:
            reqs.append(dist.isend(t, dst, group=group))
        for o in outs:
            reqs.append(dist.irecv(o, src, group=group))
    else:
        for o in outs:
            reqs.append(dist.irecv(o, src, group=group))
        for t in sends:
            reqs.append(dist.isend(t, dst, group=group))
    for q in reqs:
        q.wait()
    return outs


def _block_scores(q32: torch.Tensor, kj: torch.Tensor, scale: float,
                  diagonal: bool) -> torch.Tensor:
    """scale * q @ k^T with the in-block causal mask when this is the
    diagonal block (global causality between blocks is handled by the
    j <= r schedule)."""
    s = torch.matmul(q32, kj.float().transpose(-1, -2)) * scale
    if diagonal:
        Sb = s.shape[-1]
        mask = torch.ones(Sb, Sb, dtype=torch.bool,
                          device=s.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    return s


def _cp_attn_mode() -> str:
    mode = os.environ.get("AITJ_CP_ATTN", "auto")
    if mode not in ("auto", "legacy", "block"):
        raise ValueError(
            f"AITJ_CP_ATTN={mode!r}: expected auto, legacy or block")
    return mode


LAYOUTS = ("contiguous", "zigzag")


def _check_layout(layout: str) -> str:
    if layout not in LAYOUTS:
        raise ValueError(
            f"cp layout {layout!r}: expected contiguous or zigzag")
    return layout


def cp_layout_from_env() -> str:
    """AITJ_CP_LAYOUT (contiguous when unset), validated."""
    return _check_layout(os.environ.get("AITJ_CP_LAYOUT", "contiguous"))


def cp_shard_chunks(layout: str, n: int, r: int) -> List[int]:
    """Global chunk ids rank r holds, in local row order. Contiguous cuts
    the sequence into n chunks and rank r holds chunk r; zig-zag cuts it
    into 2n and rank r holds chunk r (the low half of its shard) and chunk
    2n-1-r (the high half)."""
    _check_layout(layout)
    assert 0 <= r < n, (r, n)
    return [r] if layout == "contiguous" else [r, 2 * n - 1 - r]


def cp_schedule(layout: str, n: int, r: int):
    """The ring schedule of rank r in a ring of n: one (j, q_part, kv_part,
    causal) per ring step t = 0..n-1, where j = (r - t) % n is the rank the
    visiting K/V shard comes from and the parts, each "full", "lo" or "hi"
    (whole shard, its first or its second half of rows), say which local q
    rows meet which rows of that shard. q_part None: the step computes
    nothing (the shard only transits). This is the single statement of the
    schedule: the ring forward and backward, the one-GPU emulation test and
    scripts/ringbench.py all walk it.

      contiguous  j <= r computes, full x full, causal on j == r;
      zigzag      j == r  full x full, causal (in local order, low chunk
                          then high chunk, the shard on itself is exactly a
                          causal Sb x Sb block)
                  j <  r  full x lo: every local row sees the visiting low
                          chunk, none sees its high chunk
                  j >  r  hi x full: only the local high chunk lies after
                          the visiting shard, and after all of it
    so every zig-zag step of every rank is 2 chunk x chunk units of work
    (the diagonal step counting its two causal chunks as halves)."""
    _check_layout(layout)
    assert 0 <= r < n, (r, n)
    steps = []
    for t in range(n):
        j = (r - t) % n
        if j == r:
            steps.append((j, "full", "full", True))
        elif layout == "contiguous":
            steps.append((j, "full", "full", False) if j < r
                         else (j, None, None, False))
        elif j < r:
            steps.append((j, "full", "lo", False))
        else:
            steps.append((j, "hi", "full", False))
    return steps


def cp_shard_positions(S: int, n: int, r: int,
                       layout: str = "contiguous") -> torch.Tensor:
    """Global token index of every local row of rank r (int64 [S/n])."""
    chunks = cp_shard_chunks(layout, n, r)
    per = n * len(chunks)
    assert S % per == 0, f"seq_len {S} not divisible by {per} ({layout})"
    Sc = S // per
    return torch.cat([torch.arange(c * Sc, (c + 1) * Sc) for c in chunks])


def cp_unshard(shards, layout: str = "contiguous", dim: int = 1):
    """Inverse of the sharding: per-rank tensors (rank order, sequence on
    `dim`) back to one tensor in global token order."""
    n = len(shards)
    S = sum(t.shape[dim] for t in shards)
    pos = torch.cat([cp_shard_positions(S, n, r, layout) for r in range(n)])
    inv = torch.empty_like(pos)
    inv[pos] = torch.arange(S)
    return torch.cat(list(shards), dim=dim).index_select(
        dim, inv.to(shards[0].device))


def _part(t: torch.Tensor, part: str, dim: int = 2) -> torch.Tensor:
    """Rows of a shard named by a schedule part (a view)."""
    if part == "full":
        return t
    h = t.shape[dim] // 2
    return t.narrow(dim, 0 if part == "lo" else h, h)


def _block_ops(q, k, layout: str = "contiguous"):
    """(block_fwd, delta, block_bwd, merge_) — the native flash kernels
    where they apply (to every block of the layout: the zig-zag blocks are
    Sb x Sb, Sb x Sb/2 and Sb/2 x Sb), their fp32 torch twins elsewhere."""
    from ..ops import attention as A
    from ..ops import reference as R
    if layout == "zigzag":
        q, k = _part(q, "hi"), _part(k, "lo")
    if A.block_supported(q, k):
        return (A.flash_attention_block_fwd, A.flash_attention_delta,
                A.flash_attention_block_bwd, A.attn_merge_)
    return (R.attention_block_fwd, R.attention_delta,
            R.attention_block_bwd, R.attn_merge_)


def uses_block_path(q, k, layout: str = "contiguous") -> bool:
    """Whether ring_attention(q, k, ...) takes the block-structured ring
    (k/v at HKV heads) or the legacy one (k/v expanded to H heads). The
    zig-zag layout exists on the block structure only."""
    mode = _cp_attn_mode()
    if _check_layout(layout) == "zigzag":
        if mode == "legacy":
            raise ValueError(
                "AITJ_CP_ATTN=legacy cannot run the zigzag cp layout "
                "(AITJ_CP_LAYOUT / --cp-layout zigzag): the legacy matmul "
                "ring is contiguous only")
        return True
    if mode == "legacy":
        return False
    if mode == "block":
        return True
    from ..ops.attention import block_supported
    return block_supported(q, k)


def _ring_rank(group):
    n = _group_size(group)
    return n, (dist.get_rank(group) if n > 1 else 0)


def _block_ring_forward(q, k, v, group, scale, layout):
    """The block-structured ring forward over [B,H,Sb,D] / [B,HKV,Sb,D]
    operands (any strides with a unit last one). Returns the fp32
    accumulator pairs in local row order: [(o, lse)] for contiguous,
    [(o_lo, lse_lo), (o_hi, lse_hi)] for zig-zag — per half and contiguous,
    so that a full-q block result merges as two half views and a high-half
    result as one."""
    n, r = _ring_rank(group)
    block_fwd, _, _, merge_ = _block_ops(q, k, layout)
    B, H, Sb, D = q.shape
    parts = ("full",) if layout == "contiguous" else ("lo", "hi")
    rows = Sb // len(parts)
    acc = [(torch.zeros(B, H, rows, D, dtype=torch.float32, device=q.device),
            torch.full((B, H, rows), float("-inf"), dtype=torch.float32,
                       device=q.device)) for _ in parts]
    kj, vj = k, v
    for t, (j, qp, kvp, causal) in enumerate(cp_schedule(layout, n, r)):
        if qp is not None:
            o_j, lse_j = block_fwd(_part(q, qp), _part(kj, kvp),
                                   _part(vj, kvp), causal, scale)
            if qp == "full":
                for (o_acc, lse_acc), p in zip(acc, parts):
                    merge_(o_acc, lse_acc, _part(o_j, p), _part(lse_j, p))
            else:                        # "hi": the second accumulator
                merge_(acc[1][0], acc[1][1], o_j, lse_j)
        if t + 1 < n:
            kj, vj = _ring_shift([kj, vj], group)
    return acc


def _block_ring_backward(q, k, v, dout, lse, delta, group, scale, layout):
    """The second ring pass on the merged lse/delta (fp32 [B,H,Sb]): fp32
    dq [B,H,Sb,D] and the fp32 dk/dv [B,HKV,Sb,D] that travelled with
    their K/V shard and are home again. A rectangular step adds into the
    rows it covers only: dq's high half at j > r, the travelling dK/dV's
    low half at j < r."""
    n, r = _ring_rank(group)
    _, _, block_bwd, _ = _block_ops(q, k, layout)
    dq = torch.zeros(q.shape, dtype=torch.float32, device=q.device)
    kj, vj = k, v
    dkj = torch.zeros(k.shape, dtype=torch.float32, device=k.device)
    dvj = torch.zeros(v.shape, dtype=torch.float32, device=v.device)
    for j, qp, kvp, causal in cp_schedule(layout, n, r):
        if qp is not None:
            dq_b, dk_b, dv_b = block_bwd(
                _part(q, qp), _part(kj, kvp), _part(vj, kvp),
                _part(dout, qp), _part(lse, qp), _part(delta, qp), causal,
                scale)
            _part(dq, qp).add_(dq_b)
            _part(dkj, kvp).add_(dk_b)
            _part(dvj, kvp).add_(dv_b)
        # n shifts total: the (k, dk, dv) triplet arrives back home
        if n > 1:
            kj, vj, dkj, dvj = _ring_shift([kj, vj, dkj, dvj], group)
    return dq, dkj, dvj


class _RingAttention(torch.autograd.Function):
    """Causal ring attention over [B, H, Sb, D] blocks. block=True: the
    block-structured ring (k/v [B, HKV, Sb, D]); block=False: the legacy
    fp32 matmul ring (equal kv heads — the module expands GQA first)."""

    @staticmethod
    def _block_forward(ctx, q, k, v, group, scale, layout):
        acc = _block_ring_forward(q, k, v, group, scale, layout)
        if len(acc) == 1:
            o_acc, lse_acc = acc[0]
        else:
            o_acc = torch.cat([a[0] for a in acc], dim=2)
            lse_acc = torch.cat([a[1] for a in acc], dim=2)
        out = o_acc.to(q.dtype)
        ctx.save_for_backward(q, k, v, out, lse_acc)
        ctx.group, ctx.scale = group, scale
        return out

    @staticmethod
    def _block_backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        _, delta_fn, _, _ = _block_ops(q, k, ctx.layout)
        dout = dout.to(q.dtype)
        delta = delta_fn(out, dout)           # once, from the merged out
        dq, dk, dv = _block_ring_backward(q, k, v, dout, lse, delta,
                                          ctx.group, ctx.scale, ctx.layout)
        return (dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype),
                None, None, None, None)

    @staticmethod
    def forward(ctx, q, k, v, group, scale, block=False,
                layout="contiguous"):
        ctx.block, ctx.layout = block, layout
        if block:
            return _RingAttention._block_forward(ctx, q, k, v, group, scale,
                                                 layout)
        n = _group_size(group)
        r = dist.get_rank(group) if n > 1 else 0
        q32 = q.float()
        B, H, Sb, D = q.shape
        o = torch.zeros(B, H, Sb, D, dtype=torch.float32, device=q.device)
        m = torch.full((B, H, Sb, 1), float("-inf"), device=q.device)
        l = torch.zeros(B, H, Sb, 1, device=q.device)
        kj, vj = k, v
        j = r
        for t in range(n):
            if j <= r:
                s = _block_scores(q32, kj, scale, diagonal=(j == r))
                m_new = torch.maximum(m, s.amax(dim=-1, keepdim=True))
                p = torch.exp(s - m_new)
                alpha = torch.exp(m - m_new)
                l = l * alpha + p.sum(dim=-1, keepdim=True)
                o = o * alpha + torch.matmul(p, vj.float())
                m = m_new
            if t + 1 < n:
                kj, vj = _ring_shift([kj, vj], group)
                j = (j - 1) % n
        out32 = o / l
        lse = m + torch.log(l)
        ctx.save_for_backward(q, k, v, out32, lse)
        ctx.group, ctx.scale = group, scale
        return out32.to(q.dtype)

    @staticmethod
    def backward(ctx, dout):
        if ctx.block:
            return _RingAttention._block_backward(ctx, dout)
        q, k, v, out32, lse = ctx.saved_tensors
        group, scale = ctx.group, ctx.scale
        n = _group_size(group)
        r = dist.get_rank(group) if n > 1 else 0
        q32, do32 = q.float(), dout.float()
        delta = (do32 * out32).sum(dim=-1, keepdim=True)
        dq = torch.zeros_like(q32)
        kj, vj = k, v
        dkj = torch.zeros_like(k, dtype=torch.float32)
        dvj = torch.zeros_like(v, dtype=torch.float32)
        j = r
        for t in range(n):
            if j <= r:
                s = _block_scores(q32, kj, scale, diagonal=(j == r))
                p = torch.exp(s - lse)            # recomputed, flash-style
                dvj += torch.matmul(p.transpose(-1, -2), do32)
                dp = torch.matmul(do32, vj.float().transpose(-1, -2))
                ds = p * (dp - delta)
                dq += scale * torch.matmul(ds, kj.float())
                dkj += scale * torch.matmul(ds.transpose(-1, -2), q32)
            # n shifts total: the (k, dk, dv) triplet arrives back home
            if n > 1:
                kj, vj, dkj, dvj = _ring_shift([kj, vj, dkj, dvj], group)
                j = (j - 1) % n
        return (dq.to(q.dtype), dkj.to(k.dtype), dvj.to(v.dtype),
                None, None, None, None)


def ring_attention(q, k, v, group, scale: Optional[float] = None,
                   layout: str = "contiguous"):
    """Causal ring attention; q [B, H, Sb, D] and k/v [B, HKV, Sb, D]
    are this rank's sequence shard: tokens [r*Sb, (r+1)*Sb) for
    layout="contiguous", chunks r and 2n-1-r of 2n (cp_shard_positions) for
    layout="zigzag", which gives every rank the same work at every ring
    step. Zig-zag needs an even Sb and exists on the block structure only:
    auto takes the native ops where they cover the half-shard blocks
    (Sb/2 % 256 == 0 on the GPU) and the fp32 twins elsewhere;
    AITJ_CP_ATTN=legacy with it raises ValueError.

    Head-count contract: when uses_block_path(q, k) holds (AITJ_CP_ATTN=
    block, or auto with a shard the native block kernels cover) k/v may
    carry HKV <= H heads with H % HKV == 0; they circulate unexpanded and
    dk/dv come back at HKV heads. On the legacy path (AITJ_CP_ATTN=legacy,
    or auto elsewhere) k/v must already be expanded to H heads."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    block = uses_block_path(q, k, layout)
    if layout == "zigzag":
        assert q.shape[2] % 2 == 0 and k.shape[2] == q.shape[2], (
            f"zigzag shards are two chunks: q {tuple(q.shape)} "
            f"k {tuple(k.shape)}")
    if block:
        assert q.shape[1] % k.shape[1] == 0 and k.shape == v.shape, (
            q.shape, k.shape, v.shape)
    else:
        assert k.shape[1] == q.shape[1], (
            f"legacy ring attention needs kv heads expanded to "
            f"{q.shape[1]}, got {k.shape[1]}")
    return _RingAttention.apply(q, k, v, group, scale, block, layout)


def _rope_offset(x: torch.Tensor, inv_freq: torch.Tensor,
                 pos0: int) -> torch.Tensor:
    """Differentiable Neox rotation at positions pos0..pos0+Sb-1
    (x [B, Sb, nh, D]); the shard's global offset makes every rank agree
    on absolute positions."""
    B, Sb, nh, D = x.shape
    half = D // 2
    pos = (torch.arange(Sb, device=x.device) + pos0).float()
    ang = pos[:, None] * inv_freq[None, :].float()
    cos = ang.cos()[None, :, None, :]
    sin = ang.sin()[None, :, None, :]
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    return torch.cat([x1 * cos - x2 * sin,
                      x1 * sin + x2 * cos], dim=-1).to(x.dtype)


def _shard_segments(layout: str, n: int, r: int, Sb: int):
    """(seg_len, pos_a, pos_b) of rank r's shard for rope_packed_at."""
    if layout == "contiguous":
        return Sb, r * Sb, 0
    Sc = Sb // 2
    return Sc, r * Sc, (2 * n - 1 - r) * Sc


class _PackedCPAttention(torch.autograd.Function):
    """qkv [B,Sb,(H+2HKV)*128] -> o [B,Sb,H*128] of one sequence shard on
    the GPU, modelled on ops.attention._PackedRopeAttention: one
    rope_packed_at launch over the q|k head range, the ring's block ops on
    strided [B,heads,Sb,128] views of rot/qkv, lse merge into fp32
    accumulators; backward: delta once, the ring on the merged lse/delta,
    bf16 dq/dk/dv into the head ranges of one dqkv buffer, un-rotated in
    place by one rope_packed_at(sign=-1). The contiguous copies left are
    the K/V send buffers of _ring_shift and the fp32 lse/delta halves."""

    @staticmethod
    def _views(rot, qkv, B, Sb, H, HKV, D):
        r4 = rot.view(B, Sb, H + HKV, D)
        q = r4[:, :, :H].permute(0, 2, 1, 3)
        k = r4[:, :, H:].permute(0, 2, 1, 3)
        v = qkv.view(B, Sb, H + 2 * HKV, D)[:, :, H + HKV:].permute(0, 2, 1, 3)
        return q, k, v

    @staticmethod
    def forward(ctx, qkv, inv_freq, n_heads, n_kv_heads, scale, group,
                layout):
        from ..ops.attention import rope_packed_at
        B, Sb, W = qkv.shape
        D = 128
        H, HKV = n_heads, n_kv_heads
        assert W == (H + 2 * HKV) * D
        qkv = qkv.contiguous()
        n, r = _ring_rank(group)
        seg = _shard_segments(layout, n, r, Sb)
        rot = torch.empty(B, Sb, (H + HKV) * D, dtype=torch.bfloat16,
                          device=qkv.device)
        rope_packed_at(qkv, rot, inv_freq, H + HKV, Sb, *seg, sign=1.0)
        q, k, v = _PackedCPAttention._views(rot, qkv, B, Sb, H, HKV, D)
        acc = _block_ring_forward(q, k, v, group, scale, layout)
        o = torch.empty(B, Sb, H * D, dtype=torch.bfloat16, device=qkv.device)
        o4 = o.view(B, Sb, H, D).permute(0, 2, 1, 3)
        rows = Sb // len(acc)
        for i, (o_acc, _) in enumerate(acc):   # one rounding, as the ring's
            o4.narrow(2, i * rows, rows).copy_(o_acc)
        lse = acc[0][1] if len(acc) == 1 else torch.cat(
            [a[1] for a in acc], dim=2)
        ctx.save_for_backward(rot, qkv, o, lse, inv_freq)
        ctx.dims = (B, Sb, H, HKV, D)
        ctx.scale, ctx.group, ctx.layout, ctx.seg = scale, group, layout, seg
        return o

    @staticmethod
    def backward(ctx, gout):
        from ..ops.attention import flash_attention_delta, rope_packed_at
        rot, qkv, o, lse, inv_freq = ctx.saved_tensors
        B, Sb, H, HKV, D = ctx.dims
        W = (H + 2 * HKV) * D
        q, k, v = _PackedCPAttention._views(rot, qkv, B, Sb, H, HKV, D)
        dout = gout if gout.is_contiguous() else gout.contiguous()
        dout4 = dout.view(B, Sb, H, D).permute(0, 2, 1, 3)
        o4 = o.view(B, Sb, H, D).permute(0, 2, 1, 3)
        delta = flash_attention_delta(o4, dout4)
        dq, dk, dv = _block_ring_backward(q, k, v, dout4, lse, delta,
                                          ctx.group, ctx.scale, ctx.layout)
        dqkv = torch.empty(B, Sb, W, dtype=torch.bfloat16, device=qkv.device)
        d4 = dqkv.view(B, Sb, H + 2 * HKV, D)
        d4[:, :, :H].permute(0, 2, 1, 3).copy_(dq)
        d4[:, :, H:H + HKV].permute(0, 2, 1, 3).copy_(dk)
        d4[:, :, H + HKV:].permute(0, 2, 1, 3).copy_(dv)
        rope_packed_at(dqkv, dqkv, inv_freq, H + HKV, Sb, *ctx.seg, sign=-1.0)
        return dqkv, None, None, None, None, None, None


def cp_packed_enabled() -> bool:
    """AITJ_CP_PACKED=1: a contiguous shard takes the packed op too (its
    RoPE then comes from the native kernel, not from fp32 torch cos/sin, so
    the bits move — hence opt-in). Read on every call."""
    return os.environ.get("AITJ_CP_PACKED", "0") == "1"


def packed_cp_supported(qkv: torch.Tensor, n_heads: int, n_kv_heads: int,
                        layout: str) -> bool:
    """Shards the packed op covers: GPU bf16 [B,Sb,(H+2HKV)*128] whose ring
    blocks the native block ops cover (Sb % 256 == 0 contiguous, Sb % 512
    == 0 zig-zag), and not the legacy ring."""
    per = 256 if layout == "contiguous" else 512
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3
            and qkv.shape[1] > 0 and qkv.shape[1] % per == 0
            and n_heads % n_kv_heads == 0
            and qkv.shape[2] == (n_heads + 2 * n_kv_heads) * 128
            and _cp_attn_mode() != "legacy")


class CPAttention(nn.Module):
    """Attention over a sequence shard: replicated weights (same layout
    as models.llama.Attention), rope at global positions. K/V enter the
    block-structured ring at their HKV heads; the legacy ring gets them
    expanded (it needs full kv heads for its block matmuls). A zig-zag
    shard on the GPU, and a contiguous one under AITJ_CP_PACKED=1, runs
    _PackedCPAttention on the projection output where the native block ops
    apply."""

    def __init__(self, cfg: LlamaConfig, group=None,
                 layout: str = "contiguous"):
        super().__init__()
        self.cfg = cfg
        self.group = group
        self.layout = _check_layout(layout)
        H = cfg.hidden_size
        self.q_size = cfg.num_heads * cfg.head_dim
        self.kv_size = cfg.num_kv_heads * cfg.head_dim
        self.qkv_proj = nn.Linear(H, self.q_size + 2 * self.kv_size,
                                  bias=False)
        self.o_proj = nn.Linear(self.q_size, H, bias=False)

    def forward(self, x_s: torch.Tensor, inv_freq: torch.Tensor,
                pos0: int) -> torch.Tensor:
        B, Sb, _ = x_s.shape
        cfg = self.cfg
        layout = self.layout
        qkv = self.qkv_proj(x_s)
        if ((layout == "zigzag" or cp_packed_enabled())
                and cfg.head_dim == 128
                and packed_cp_supported(qkv, cfg.num_heads, cfg.num_kv_heads,
                                        layout)):
            o = _PackedCPAttention.apply(
                qkv, inv_freq, cfg.num_heads, cfg.num_kv_heads,
                1.0 / math.sqrt(cfg.head_dim), self.group, layout)
            return self.o_proj(o)
        q, k, v = qkv.split([self.q_size, self.kv_size, self.kv_size],
                            dim=-1)
        q = q.reshape(B, Sb, cfg.num_heads, cfg.head_dim)
        k = k.reshape(B, Sb, cfg.num_kv_heads, cfg.head_dim)
        v = v.reshape(B, Sb, cfg.num_kv_heads, cfg.head_dim)
        if layout == "contiguous":
            q = _rope_offset(q, inv_freq, pos0).transpose(1, 2)
            k = _rope_offset(k, inv_freq, pos0).transpose(1, 2)
        else:
            from ..ops.reference import rope_at
            n, r = _ring_rank(self.group)
            pos = cp_shard_positions(Sb * n, n, r, layout).to(x_s.device)
            q = rope_at(q, inv_freq, pos).transpose(1, 2)
            k = rope_at(k, inv_freq, pos).transpose(1, 2)
        v = v.transpose(1, 2)
        G = cfg.num_heads // cfg.num_kv_heads
        if G > 1 and not uses_block_path(q, k, layout):
            k = k.repeat_interleave(G, dim=1)
            v = v.repeat_interleave(G, dim=1)
        o = ring_attention(q, k, v, self.group, layout=layout)
        o = o.transpose(1, 2).reshape(B, Sb, self.q_size)
        return self.o_proj(o)


class CPBlock(nn.Module):
    def __init__(self, cfg: LlamaConfig, group=None,
                 layout: str = "contiguous"):
        super().__init__()
        self.cfg = cfg
        self.attn = CPAttention(cfg, group, layout)
        from ..models.llama import MLP
        self.mlp = MLP(cfg)
        self.input_norm_weight = nn.Parameter(torch.ones(cfg.hidden_size))
        self.post_attn_norm_weight = nn.Parameter(
            torch.ones(cfg.hidden_size))

    def forward(self, x_s, residual_s, inv_freq, pos0):
        normed, residual_s = fused_rmsnorm(x_s, self.input_norm_weight,
                                           residual_s, self.cfg.norm_eps)
        attn_out = self.attn(normed, inv_freq, pos0)
        normed, residual_s = fused_rmsnorm(attn_out,
                                           self.post_attn_norm_weight,
                                           residual_s, self.cfg.norm_eps)
        return self.mlp(normed), residual_s


class _AllReduceSumLoss(torch.autograd.Function):
    """fwd: sum the per-rank partial losses so every rank reports the
    GLOBAL loss; bwd: identity (d global / d local = 1) — each rank then
    backprops exactly its own partial term, and allreduce_cp_grads sums
    the resulting replica gradients into the global gradient."""

    @staticmethod
    def forward(ctx, x, group):
        y = x.clone()
        dist.all_reduce(y, group=group)
        return y

    @staticmethod
    def backward(ctx, g):
        return g, None


class CPLlamaModel(nn.Module):
    """Llama with every weight replicated and the sequence sharded cp
    ways: layout="contiguous" gives rank r the tokens [r*Sb, (r+1)*Sb),
    layout="zigzag" the chunks r and 2cp-1-r of 2cp (cp_shard_positions),
    which evens out the causal work over the ring. forward takes the FULL
    batch (every rank slices its own shard — the callers already feed
    identical data to the group) and returns the global loss on every
    rank. Without targets it returns this rank's logits in SHARD order:
    row i is token cp_shard_positions(S, cp, r, layout)[i]; cp_unshard puts
    the ranks' pieces back into global order."""

    def __init__(self, cfg: LlamaConfig, group=None,
                 layout: str = "contiguous"):
        super().__init__()
        self.cfg = cfg
        self.group = group
        self.layout = _check_layout(layout)
        self.embed = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.blocks = nn.ModuleList(CPBlock(cfg, group, layout)
                                    for _ in range(cfg.num_layers))
        self.final_norm_weight = nn.Parameter(torch.ones(cfg.hidden_size))
        self.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size,
                                 bias=False)
        self.register_buffer("inv_freq",
                             make_inv_freq(cfg.head_dim, cfg.rope_theta),
                             persistent=False)

    def forward(self, tokens: torch.Tensor,
                targets: Optional[torch.Tensor] = None):
        n = _group_size(self.group)
        r = dist.get_rank(self.group) if n > 1 else 0
        S = tokens.shape[1]
        assert S % max(n, 1) == 0, (S, n)
        Sb = S // max(n, 1)
        if self.layout == "contiguous":
            pos0 = r * Sb
            tok_s = tokens[:, pos0:pos0 + Sb]
        else:
            pos = cp_shard_positions(S, n, r, self.layout)
            pos0 = int(pos[0])              # on the host: no device sync
            pos = pos.to(tokens.device)
            tok_s = tokens.index_select(1, pos)
        x_s = self.embed(tok_s)
        residual_s = None
        for blk in self.blocks:
            x_s, residual_s = blk(x_s, residual_s, self.inv_freq, pos0)
        normed_s, _ = fused_rmsnorm(x_s, self.final_norm_weight,
                                    residual_s, self.cfg.norm_eps)
        logits_s = self.lm_head(normed_s)
        if targets is None:
            return logits_s                 # this rank's block of logits
        if self.layout == "contiguous":
            tgt_s = targets[:, pos0:pos0 + Sb].reshape(-1)
        else:
            tgt_s = targets.index_select(1, pos).reshape(-1)
        T = logits_s.shape[0] * logits_s.shape[1]
        per_tok = fused_cross_entropy(
            logits_s.reshape(T, -1).contiguous(), tgt_s)
        n_valid = (targets.reshape(-1) != -100).sum().clamp(min=1)
        local = per_tok.sum() / n_valid     # global denominator
        if n == 1:
            return local
        return _AllReduceSumLoss.apply(local, self.group)

    @torch.no_grad()
    def shard_from_full(self, full) -> None:
        """Weights replicate 1:1 from an unsharded LlamaModel (same
        module names/shapes — only the activations are sharded)."""
        mine = dict(self.named_parameters())
        for name, p in full.named_parameters():
            mine[name].copy_(p)

    @torch.no_grad()
    def allreduce_cp_grads(self) -> None:
        """Sum replica gradients over the CP group (each rank backpropped
        only its own partial loss term). Call after backward, before the
        optimizer — like DP's all-reduce but with SUM semantics because
        the partials already carry the global 1/n_valid."""
        if _group_size(self.group) == 1:
            return
        for p in self.parameters():
            if p.grad is not None:
                dist.all_reduce(p.grad, group=self.group)


# ---------------------------------------------------------------------------
# DP x CP trainer
# ---------------------------------------------------------------------------

class CPTopology:
    """world = dp x cp; cp peers are ADJACENT ranks (ring hops are one
    xGMI link) and share the data batch; dp replicas stream their own."""

    def __init__(self, cp_size: int = 0):
        if not dist.is_initialized():
            self.world, self.rank = 1, 0
            self.cp_size, self.cp_rank, self.cp_group = 1, 0, None
            self.dp_size, self.dp_rank = 1, 0
            return
        world = dist.get_world_size()
        rank = dist.get_rank()
        cp = cp_size or world
        if world % cp != 0:
            raise ValueError(f"world {world} not divisible by cp={cp}")
        self.world, self.rank = world, rank
        self.cp_size, self.dp_size = cp, world // cp
        self.cp_rank, self.dp_rank = rank % cp, rank // cp
        self.cp_group = None
        for d in range(self.dp_size):          # new_group is collective
            g = dist.new_group(list(range(d * cp, (d + 1) * cp)))
            if d == self.dp_rank:
                self.cp_group = g
        if self.cp_size == 1:
            self.cp_group = None


class CPTrainer:
    """Context-parallel trainer: weights replicated, sequence sharded
    cp-ways (ring attention), dp on top for throughput.

    Gradient seam: each rank backprops its own partial of the GLOBAL
    loss (see _AllReduceSumLoss), so the flat grad needs one SUM
    all-reduce over the whole world, pre-scaled by 1/dp for the
    data-parallel mean. After it every rank holds identical global
    gradients, so the optimizer's local grad-norm clip is globally
    correct and checkpoints are a single rank-0 stream (any-world-size
    resume like DP)."""

    def __init__(self, cfg, cp_size: int = 0, device=None,
                 layout: Optional[str] = None):
        from ..launcher.data import make_batches
        from ..models.config import CONFIGS
        from ..optim import FlatAdamW
        from .flat import FlatParamStore

        if getattr(cfg, "doc_mask", False):
            raise ValueError(
                "CPTrainer does not support doc_mask: ring attention has no "
                "document mask and would attend across documents")
        self.cfg = cfg
        mcfg = CONFIGS[cfg.model]
        self.device = torch.device(device or "cpu")
        self.topo = CPTopology(cp_size)
        # layout None: AITJ_CP_LAYOUT, contiguous when unset
        self.layout = _check_layout(layout) if layout else cp_layout_from_env()
        assert cfg.seq_len % self.topo.cp_size == 0, \
            (cfg.seq_len, self.topo.cp_size)
        if self.layout == "zigzag":
            assert cfg.seq_len % (2 * self.topo.cp_size) == 0, (
                f"zigzag cp layout needs seq_len % (2*cp) == 0, got "
                f"{cfg.seq_len} with cp={self.topo.cp_size}")
        torch.manual_seed(cfg.seed)            # identical init everywhere
        with torch.device(self.device):
            model = CPLlamaModel(mcfg, group=self.topo.cp_group,
                                 layout=self.layout)
        self.model = model.to(torch.bfloat16)
        self.model.inv_freq = make_inv_freq(mcfg.head_dim, mcfg.rope_theta,
                                            device=self.device)
        self.store = FlatParamStore(self.model, device=self.device)
        self.opt = FlatAdamW(self.store, lr=cfg.lr, betas=cfg.betas,
                             weight_decay=cfg.weight_decay,
                             clip_grad_norm=cfg.clip_grad_norm)
        # cp peers consume the SAME stream (each slices its own block)
        self.data = make_batches(cfg, self.device, rank=self.topo.dp_rank)
        self.step_count = 0

    def _sync_grads(self) -> None:
        if self.topo.world == 1:
            return
        fg = self.store.flat_grad
        if self.topo.dp_size > 1:
            fg.mul_(1.0 / self.topo.dp_size)
        dist.all_reduce(fg)                     # SUM over dp x cp

    def train_step(self):
        cfg = self.cfg
        if cfg.warmup_steps or cfg.lr_decay_steps:
            from ..optim import lr_at
            self.opt.lr = lr_at(self.opt.step_count, cfg.lr,
                                cfg.warmup_steps, cfg.lr_decay_steps,
                                cfg.min_lr)
        loss = None
        for _ in range(cfg.grad_accum):
            tokens, targets = next(self.data)
            loss = self.model(tokens, targets)
            (loss / cfg.grad_accum).backward()
        self._sync_grads()
        self.opt.step(grad_pre_scale=1.0)
        self.opt.zero_grad()
        self.step_count += 1
        return loss.detach()
