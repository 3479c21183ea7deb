"""Pure-PyTorch reference implementations of every HIP op.

Used (a) as the CPU execution path (gloo multi-process tests run these),
(b) as the fp32 numerics baseline GPU tests compare the HIP kernels against
(the repo-wide rule: numerics tests for a HIP kernel compare it against a
plain PyTorch fp32 reference of the same op).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch


def rmsnorm_fwd(x: torch.Tensor, res_in: Optional[torch.Tensor],
                w: torch.Tensor, eps: float) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """Returns (y, res_out, rrms). Math in fp32, outputs cast back."""
    if res_in is not None:
        res_out = (x.float() + res_in.float()).to(x.dtype)
        xr = res_out.float()
    else:
        res_out = None
        xr = x.float()
    rrms = torch.rsqrt(xr.pow(2).mean(dim=-1, keepdim=True) + eps)
    y = (xr * rrms * w.float()).to(x.dtype)
    return y, res_out, rrms.squeeze(-1)


def rmsnorm_bwd(dy: torch.Tensor, res_out: torch.Tensor, w: torch.Tensor,
                rrms: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (dx, dw) in fp32 math."""
    H = res_out.shape[-1]
    xr = res_out.float()
    r = rrms.unsqueeze(-1).float()
    dxh = dy.float() * w.float()
    dot = (dxh * xr).sum(dim=-1, keepdim=True)
    dx = r * dxh - xr * (r ** 3) * dot / H
    dw = (dy.float() * xr * r).reshape(-1, H).sum(dim=0)
    return dx.to(dy.dtype), dw


def rope_rotate(x: torch.Tensor, inv_freq: torch.Tensor, seq_len: int,
                sign: float = 1.0) -> torch.Tensor:
    """x: [T, n_heads, D]; neox half-rotation; pos = token_index % seq_len."""
    T, n_heads, D = x.shape
    half = D // 2
    pos = (torch.arange(T, device=x.device) % seq_len).float()
    ang = pos[:, None] * inv_freq[None, :].float()  # [T, half]
    cos = torch.cos(ang)[:, None, :]                # [T, 1, half]
    sin = torch.sin(ang)[:, None, :] * sign
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    o1 = x1 * cos - x2 * sin
    o2 = x1 * sin + x2 * cos
    return torch.cat([o1, o2], dim=-1).to(x.dtype)


def rope_at(x: torch.Tensor, inv_freq: torch.Tensor, positions: torch.Tensor,
            sign: float = 1.0) -> torch.Tensor:
    """Twin of rope_packed_at: x [..., S, n_heads, D], positions [S] (the
    global token index of every local row, e.g. cp_shard_positions); neox
    half-rotation in fp32, result in x.dtype. Differentiable."""
    half = x.shape[-1] // 2
    assert positions.shape == (x.shape[-3],), (positions.shape, x.shape)
    ang = positions.to(x.device).float()[:, None] * inv_freq[None, :].float()
    cos = torch.cos(ang)[:, None, :]                # [S, 1, half]
    sin = torch.sin(ang)[:, None, :] * sign
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    return torch.cat([x1 * cos - x2 * sin,
                      x1 * sin + x2 * cos], dim=-1).to(x.dtype)


PAGE_ROWS = 64      # rows per KV-cache page (== the decode kernel's chunk)


def _paged_gather(pool: torch.Tensor, block_table: torch.Tensor
                  ) -> torch.Tensor:
    """pool [n_pages, n_kv, 64, D] through block_table [B, max_pages] ->
    the logical caches [B, n_kv, max_pages*64, D]. Table entries are
    clamped into the pool like the kernels clamp them."""
    B, max_pages = block_table.shape
    n_pages, n_kv, R, D = pool.shape
    tbl = block_table.long().clamp(0, n_pages - 1)
    return pool[tbl].permute(0, 2, 1, 3, 4).reshape(
        B, n_kv, max_pages * R, D)


def decode_attention_paged(q: torch.Tensor, k_pool: torch.Tensor,
                           v_pool: torch.Tensor, block_table: torch.Tensor,
                           pos: torch.Tensor, scale: float) -> torch.Tensor:
    """Twin of attn_decode_paged: q [B,H,1,D] attends rows 0..pos[b] of
    slot b's pages; fp32 math, any head_dim, result in q.dtype. A slot
    with pos[b] < 0 is idle and comes out as zeros. Rows beyond pos[b]
    are never used, whatever they hold."""
    B, H, _, D = q.shape
    n_kv = k_pool.shape[1]
    G = H // n_kv
    k = _paged_gather(k_pool, block_table).float()
    v = _paged_gather(v_pool, block_table).float()
    L = k.shape[2]
    valid = (torch.arange(L, device=q.device)[None, :]
             <= pos.to(q.device)[:, None])                  # [B, L]
    vm = valid[:, None, :, None]
    k = torch.where(vm, k, torch.zeros_like(k))
    v = torch.where(vm, v, torch.zeros_like(v))
    s = torch.einsum("bkgd,bksd->bkgs", q.reshape(B, n_kv, G, D).float(),
                     k) * scale
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    active = (pos.to(q.device) >= 0)[:, None, None, None]
    s = torch.where(active, s, torch.zeros_like(s))         # idle: no nan
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("bkgs,bksd->bkgd", p, v)
    o = torch.where(active, o, torch.zeros_like(o))
    return o.reshape(B, H, 1, D).to(q.dtype)


def rope_cache_paged(qkv: torch.Tensor, k_pool: torch.Tensor,
                     v_pool: torch.Tensor, inv_freq: torch.Tensor,
                     block_table: torch.Tensor, pos: torch.Tensor,
                     num_heads: int, num_kv_heads: int) -> torch.Tensor:
    """Twin of rope_cache_paged: qkv [B, (nh+2*nkv)*D] packed q | k | v.
    Ropes q and k (neox, fp32) at pos[b], writes k and v into row pos%64
    of page block_table[b][pos//64] IN PLACE and returns q [B, nh, D].
    An idle slot (pos[b] < 0) writes nothing and gets a zero q."""
    n_pages, _, R, D = k_pool.shape
    B = qkv.shape[0]
    half = D // 2
    x = qkv.reshape(B, num_heads + 2 * num_kv_heads, D)
    q, k, v = x.split([num_heads, num_kv_heads, num_kv_heads], dim=1)
    pos = pos.to(qkv.device)
    active = pos >= 0
    p = pos.clamp(0, block_table.shape[1] * R - 1)
    ang = p.float()[:, None] * inv_freq[None, :].float()   # [B, half]
    cos, sin = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]

    def rot(t):
        tf = t.float()
        t1, t2 = tf[..., :half], tf[..., half:]
        return torch.cat([t1 * cos - t2 * sin,
                          t1 * sin + t2 * cos], dim=-1).to(t.dtype)

    qr, kr = rot(q), rot(k)
    qr = torch.where(active[:, None, None], qr, torch.zeros_like(qr))
    page = block_table.long().gather(1, (p // R)[:, None]).squeeze(1)
    page = page.clamp(0, n_pages - 1)
    row = p % R
    k_pool[page[active], :, row[active]] = kr[active].to(k_pool.dtype)
    v_pool[page[active], :, row[active]] = v[active].to(v_pool.dtype)
    return qr.contiguous()


def rope_cache_paged_rows(qkv: torch.Tensor, k_pool: torch.Tensor,
                          v_pool: torch.Tensor, inv_freq: torch.Tensor,
                          block_table: torch.Tensor, tok_slot: torch.Tensor,
                          tok_pos: torch.Tensor, num_heads: int,
                          num_kv_heads: int) -> torch.Tensor:
    """Twin of rope_cache_paged_rows: rope_cache_paged for T packed tokens
    of several sequences. Token t belongs to block-table row tok_slot[t]
    (clamped into the table) and sits at cache position tok_pos[t]; a
    token with tok_pos < 0 writes nothing and gets a zero q. Every token is
    its own 'slot' of the per-sequence twin, with its sequence's table
    row, so the result equals that twin called token by token."""
    B = block_table.shape[0]
    slot = tok_slot.to(block_table.device).long().clamp(0, B - 1)
    return rope_cache_paged(qkv, k_pool, v_pool, inv_freq,
                            block_table[slot], tok_pos, num_heads,
                            num_kv_heads)


PREFILL_BLOCK_ROWS = 256    # q rows of one work-list block (the v7 tile)


def prefill_work_clamp(row, T: int, B: int, max_pages: int):
    """(slot, q_row0, n_rows, pos0) as the prefill kernel uses them: every
    field clamped so that all rows and positions stay inside q and the
    table, whatever the row holds."""
    slot, q_row0, n_rows, pos0 = (int(x) for x in row)
    cap = min(PREFILL_BLOCK_ROWS, T, max_pages * PAGE_ROWS)
    slot = min(max(slot, 0), B - 1)
    n_rows = min(max(n_rows, 1), cap)
    q_row0 = min(max(q_row0, 0), T - n_rows)
    pos0 = min(max(pos0, 0), max_pages * PAGE_ROWS - n_rows)
    return slot, q_row0, n_rows, pos0


def prefill_attention_paged(q: torch.Tensor, k_pool: torch.Tensor,
                            v_pool: torch.Tensor, block_table: torch.Tensor,
                            work: torch.Tensor, scale: float,
                            out: Optional[torch.Tensor] = None
                            ) -> torch.Tensor:
    """Twin of attn_prefill_paged: q [T, H, D] packed rows of several
    sequences. work [n, 4] int32 rows (slot, q_row0, n_rows, pos0): rows
    q_row0 .. q_row0+n_rows-1 sit at cache positions pos0 .. of block-table
    row `slot`, and the row at position p attends cache rows 0..p. fp32
    math, any head_dim, result in q.dtype. Rows of `out` (zeros if not
    given) that no work row names are left as they are; cache rows beyond
    a row's position are never used, whatever they hold."""
    T, H, D = q.shape
    n_pages, n_kv, R, _ = k_pool.shape
    G = H // n_kv
    B, max_pages = block_table.shape
    o = torch.zeros_like(q) if out is None else out
    tbl = block_table.long().clamp(0, n_pages - 1).cpu()
    for row in work.cpu().tolist():
        slot, q_row0, n_rows, pos0 = prefill_work_clamp(row, T, B, max_pages)
        L = pos0 + n_rows
        pages = tbl[slot, :(L + R - 1) // R].to(k_pool.device)
        k = k_pool[pages].permute(1, 0, 2, 3).reshape(n_kv, -1, D)[:, :L]
        v = v_pool[pages].permute(1, 0, 2, 3).reshape(n_kv, -1, D)[:, :L]
        qb = q[q_row0:q_row0 + n_rows].float().reshape(n_rows, n_kv, G, D)
        s = torch.einsum("rkgd,ksd->kgrs", qb, k.float()) * scale
        p_row = pos0 + torch.arange(n_rows, device=q.device)
        seen = torch.arange(L, device=q.device)[None, :] <= p_row[:, None]
        s = s.masked_fill(~seen[None, None], float("-inf"))
        p = torch.softmax(s, dim=-1)
        ob = torch.einsum("kgrs,ksd->rkgd", p, v.float())
        o[q_row0:q_row0 + n_rows] = ob.reshape(n_rows, H, D).to(o.dtype)
    return o


def swiglu_fwd(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    gf = g.float()
    return (gf * torch.sigmoid(gf) * u.float()).to(g.dtype)


def swiglu_bwd(dout: torch.Tensor, g: torch.Tensor,
               u: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    gf, uf, dof = g.float(), u.float(), dout.float()
    sg = torch.sigmoid(gf)
    silu = gf * sg
    du = dof * silu
    dg = dof * uf * sg * (1 + gf * (1 - sg))
    return dg.to(g.dtype), du.to(u.dtype)


def ce_fwd(logits: torch.Tensor, targets: torch.Tensor,
           ignore_index: int = -100) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (loss_per_row fp32 [T], lse fp32 [T]); ignored rows get 0."""
    lf = logits.float()
    lse = torch.logsumexp(lf, dim=-1)
    valid = targets != ignore_index
    safe_t = targets.clamp_min(0)
    picked = lf.gather(-1, safe_t.unsqueeze(-1).long()).squeeze(-1)
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse))
    return loss, lse


def ce_bwd(logits: torch.Tensor, targets: torch.Tensor, lse: torch.Tensor,
           gscale: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    lf = logits.float()
    p = torch.exp(lf - lse.unsqueeze(-1))
    valid = (targets != ignore_index)
    safe_t = targets.clamp_min(0).long()
    p.scatter_add_(-1, safe_t.unsqueeze(-1),
                   -torch.ones_like(lse).unsqueeze(-1))
    p = p * (gscale * valid.float()).unsqueeze(-1)
    return p.to(logits.dtype)


def adamw_step(p32: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
               grad: torch.Tensor, p_bf16: torch.Tensor, lr: float,
               beta1: float, beta2: float, eps: float, weight_decay: float,
               step: int, clip: float = 0.0,
               normsq: Optional[torch.Tensor] = None,
               pre_scale: float = 1.0) -> None:
    """In-place flat AdamW matching the HIP kernel (decoupled weight decay).
    pre_scale folds the DDP 1/world_size average into the update."""
    g = grad.float() * pre_scale
    if clip > 0.0 and normsq is not None:
        norm = normsq.sqrt() * pre_scale
        g = g * (clip / torch.clamp(norm, min=clip))
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    mhat = m / bc1
    vhat = v / bc2
    p32.add_(-lr * (mhat / (vhat.sqrt() + eps) + weight_decay * p32))
    p_bf16.copy_(p32.to(p_bf16.dtype))


# ---------------------------------------------------------------------------
# Block attention for the context-parallel ring (twins of the native block
# ops in ops/attention.py): fp32 math, any dtype / head_dim / length.
# q [B,H,Sq,D]; k, v [B,HKV,Skv,D] with H % HKV == 0.
# ---------------------------------------------------------------------------

def _expand_kv(x: torch.Tensor, n_heads: int) -> torch.Tensor:
    g = n_heads // x.shape[1]
    return x if g == 1 else x.repeat_interleave(g, dim=1)


def _block_scores(q, k, causal: bool, scale: float) -> torch.Tensor:
    s = torch.matmul(q.float(),
                     _expand_kv(k, q.shape[1]).float().transpose(-1, -2))
    s = s * scale
    if causal:
        mask = torch.ones(s.shape[-2], s.shape[-1], dtype=torch.bool,
                          device=s.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    return s


def attention_block_fwd(q, k, v, causal: bool, scale: Optional[float] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One attention block: (o in q.dtype, lse fp32 [B,H,Sq], natural log)."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    s = _block_scores(q, k, causal, scale)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = torch.matmul(p, _expand_kv(v, q.shape[1]).float())
    return o.to(q.dtype), lse


def attention_delta(out: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
    """delta[b,h,s] = sum_d out * dout (fp32)."""
    return (out.float() * dout.float()).sum(dim=-1)


def attention_block_bwd(q, k, v, dout, lse, delta, causal: bool,
                        scale: Optional[float] = None):
    """dq, dk, dv of one block given lse and delta — the block's own or
    the merged (global) ones of a longer key range. dk/dv come back at
    k's head count (summed over each GQA group), all in the input dtypes."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    B, H, Sq, D = q.shape
    HKV, Skv = k.shape[1], k.shape[2]
    s = _block_scores(q, k, causal, scale)
    p = torch.exp(s - lse.float().unsqueeze(-1))
    do32 = dout.float()
    dv = torch.matmul(p.transpose(-1, -2), do32)
    dp = torch.matmul(do32, _expand_kv(v, H).float().transpose(-1, -2))
    ds = p * (dp - delta.float().unsqueeze(-1)) * scale
    dq = torch.matmul(ds, _expand_kv(k, H).float())
    dk = torch.matmul(ds.transpose(-1, -2), q.float())
    if HKV != H:
        dk = dk.reshape(B, HKV, H // HKV, Skv, D).sum(dim=2)
        dv = dv.reshape(B, HKV, H // HKV, Skv, D).sum(dim=2)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


def _doc_scores(q, k, bounds, scale: float) -> torch.Tensor:
    from .docmask import doc_mask_dense
    s = _block_scores(q, k, False, scale)
    return s.masked_fill(~doc_mask_dense(bounds), float("-inf"))


def attention_doc_fwd(q, k, v, bounds, scale: Optional[float] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Twin of the document-masked forward (ops/docmask.py: q sees kv iff
    bounds[0,b,q] <= kv <= q): (o in q.dtype, lse fp32 [B,H,S])."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    s = _doc_scores(q, k, bounds, scale)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = torch.matmul(p, _expand_kv(v, q.shape[1]).float())
    return o.to(q.dtype), lse


def attention_doc_bwd(q, k, v, dout, lse, delta, bounds,
                      scale: Optional[float] = None):
    """Twin of the document-masked backward: dq, dk, dv from lse and delta,
    dk/dv at k's head count, all in the input dtypes."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    B, H, S, D = q.shape
    HKV = k.shape[1]
    s = _doc_scores(q, k, bounds, scale)
    p = torch.exp(s - lse.float().unsqueeze(-1))
    do32 = dout.float()
    dv = torch.matmul(p.transpose(-1, -2), do32)
    dp = torch.matmul(do32, _expand_kv(v, H).float().transpose(-1, -2))
    ds = p * (dp - delta.float().unsqueeze(-1)) * scale
    dq = torch.matmul(ds, _expand_kv(k, H).float())
    dk = torch.matmul(ds.transpose(-1, -2), q.float())
    if HKV != H:
        dk = dk.reshape(B, HKV, H // HKV, S, D).sum(dim=2)
        dv = dv.reshape(B, HKV, H // HKV, S, D).sum(dim=2)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


def attn_merge_(o_acc: torch.Tensor, lse_acc: torch.Tensor,
                o_blk: torch.Tensor, lse_blk: torch.Tensor) -> None:
    """Fold one block (o_blk, lse_blk) into the fp32 running pair in place.
    An accumulator at (0, -inf) comes out equal to the block."""
    lse_new = torch.logaddexp(lse_acc, lse_blk.float())
    # rows where both are -inf: keep weights 0 instead of exp(nan)
    dead = torch.isinf(lse_new) & (lse_new < 0)
    wa = torch.exp(lse_acc - lse_new).masked_fill(dead, 0.0).unsqueeze(-1)
    wb = torch.exp(lse_blk.float() - lse_new).masked_fill(dead, 0.0)
    o_acc.mul_(wa).add_(o_blk.float() * wb.unsqueeze(-1))
    lse_acc.copy_(lse_new)
