"""Document layouts for document-masked causal attention.

A layout is one int32 tensor `bounds` of shape [2, B, S], contiguous, on the
device of q: bounds[0, b, s] is the window index of the first token of the
document that holds token s, bounds[1, b, s] that of its last token inside
the window. q may see kv iff bounds[0,b,q] <= kv <= q; for valid bounds
that equals kv <= q <= bounds[1,b,kv]. Valid bounds partition [0, S) into
contiguous intervals, with start and end constant on each (hence
non-decreasing in s). The mask is shared by all heads.

RoPE positions stay window-absolute under the mask. RoPE is relative, so
the scores inside a document do not depend on the document's offset in the
window.
"""
from __future__ import annotations

from typing import List, Sequence

import torch


def doc_bounds_from_eos(tokens: torch.Tensor, eos_token: int) -> torch.Tensor:
    """bounds [2,B,S] of tokens [B,S]: a token equal to eos_token is the
    last token of its document, the next token starts a new one. Tensor ops
    on the tokens' device only: no host sync, no loop over S."""
    assert tokens.dim() == 2, tokens.shape
    B, S = tokens.shape
    idx = torch.arange(S, device=tokens.device).expand(B, S)
    is_end = tokens == eos_token
    is_start = torch.ones_like(is_end)
    is_start[:, 1:] = is_end[:, :-1]
    # start: the latest document start at or before s; end: the earliest
    # document end at or after s (the window's last token ends its document)
    start = torch.cummax(torch.where(is_start, idx, 0), dim=1).values
    rev_end = torch.where(is_end, idx, S - 1).flip(1)
    end = torch.cummin(rev_end, dim=1).values.flip(1)
    return torch.stack([start, end]).to(torch.int32).contiguous()


def doc_bounds_from_lengths(lengths: Sequence[Sequence[int]],
                            device=None) -> torch.Tensor:
    """bounds [2,B,S] from B lists of document lengths that each sum to S."""
    rows: List[List[List[int]]] = [[], []]
    S = sum(lengths[0])
    for lens in lengths:
        assert all(n > 0 for n in lens) and sum(lens) == S, (
            f"document lengths {list(lens)} must be positive and sum to {S}")
        start, end, at = [], [], 0
        for n in lens:
            start += [at] * n
            end += [at + n - 1] * n
            at += n
        rows[0].append(start)
        rows[1].append(end)
    return torch.tensor(rows, dtype=torch.int32, device=device)


def doc_mask_dense(bounds: torch.Tensor) -> torch.Tensor:
    """The mask as a dense bool [B,1,S,S] (True = q row may see kv column):
    for the fp32 reference and the SDPA fallback."""
    S = bounds.shape[-1]
    idx = torch.arange(S, device=bounds.device)
    start = bounds[0].to(torch.int64)
    allowed = (idx[None, None, :] >= start[:, :, None]) \
        & (idx[None, None, :] <= idx[None, :, None])
    return allowed.unsqueeze(1)


def check_doc_bounds(bounds: torch.Tensor) -> None:
    """Assert that bounds is a valid layout. Syncs with the device: for
    tests and debugging, never on the hot path."""
    assert bounds.dtype == torch.int32 and bounds.dim() == 3 \
        and bounds.shape[0] == 2 and bounds.is_contiguous(), (
            f"bounds must be contiguous int32 [2,B,S], got "
            f"{bounds.dtype} {tuple(bounds.shape)}")
    start, end = bounds[0].cpu().long(), bounds[1].cpu().long()
    S = start.shape[1]
    idx = torch.arange(S)
    assert bool(((0 <= start) & (start <= idx) & (idx <= end)
                 & (end < S)).all()), "need 0 <= start <= s <= end < S"
    # every token of [start, end] names the same interval
    assert bool((start.gather(1, end) == start).all()) and \
        bool((end.gather(1, start) == end).all()), \
        "start and end must be constant on each document"
    assert bool((start[:, 0] == 0).all()) and bool((end[:, -1] == S - 1).all())
    if S > 1:
        same = start[:, 1:] == start[:, :-1]
        new = (start[:, 1:] == idx[1:]) & (end[:, :-1] == idx[:-1])
        assert bool((same & (end[:, 1:] == end[:, :-1]) | new).all()), \
            "documents must be contiguous intervals that partition [0, S)"
