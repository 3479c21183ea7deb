"""Paged KV cache and ragged continuous-batch decode.

The contiguous decode stack (generate.KVCache, decode_graph._step_static)
keeps one [B, n_kv, max_len, D] slab per layer and ONE position for the
whole batch, so every row of a batch must sit at the same length and a
request holds its whole slab until the batch ends. Here the cache is a
pool of 64-row pages, every sequence ("slot") has its own position and
its own row of a block table, and the two decode kernels read both on the
device (ops.rope_cache_paged, ops.decode_attention_paged):

  * PagedKVCache — the per-layer pools, the free list, the block table
    (host mirror + device tensor updated in place) and the positions;
  * _step_paged  — _step_static with the two paged calls; shape-stable,
    so it can be captured in a hipGraph like the contiguous step;
  * PagedEngine  — slots over one cache: submit() queues a request,
    step() admits queued requests into free slots (prefill through the
    ordinary _forward_cached, then load_prefix), decodes one token for
    every active slot and frees the slots of finished requests, which
    the next step refills. That refill is the continuous batching;
  * _prefill_paged — the opt-in prefill (PagedEngine(prefill="paged")):
    one packed forward over prompt chunks of several slots that writes
    the pages directly (ops.rope_cache_paged_rows) and attends them
    through the block table (ops.prefill_attention_paged), bounded per
    step by prefill_chunk;
  * generate_ragged — prompts of different lengths in, one tensor each out.

Admission reserves ceil((prompt + max_new_tokens) / 64) pages up front
and takes the physical pages as the position crosses page boundaries, so
an admitted request can always finish; one that does not fit waits in the
queue, one that can never fit is refused at submit(). On-demand
allocation with preemption is a follow-up (docs/SERVING.md).
"""
from __future__ import annotations

import math
import threading
from collections import deque
from typing import Dict, List, Optional

import torch

from ..ops import (decode_attention_paged, decode_linear, fused_rmsnorm,
                   prefill_attention_paged, prefill_work, reference,
                   rope_cache_paged, rope_cache_paged_rows)
from .generate import KVCache, _forward_cached, _layers_cached, _sample

PAGE_ROWS = reference.PAGE_ROWS


def pages_for(n_rows: int) -> int:
    return (n_rows + PAGE_ROWS - 1) // PAGE_ROWS


class PagedKVCache:
    """Per-layer [n_pages, n_kv, 64, D] key/value pools shared by
    `max_slots` sequences.

    Device state read by the kernels: `block_table` [max_slots,
    max_pages_per_seq] int32 (physical page of each logical page) and
    `pos` [max_slots] int64 (the row the next decoded token occupies; -1
    = idle slot). Both are updated in place, so a captured step keeps
    reading the same buffers. The host keeps the free list, the pages
    each slot owns and reserved, and a mirror of `pos`.
    """

    def __init__(self, cfg, n_pages: int, max_slots: int,
                 max_pages_per_seq: int, device, dtype):
        assert n_pages > 0 and max_slots > 0 and max_pages_per_seq > 0
        shape = (n_pages, cfg.num_kv_heads, PAGE_ROWS, cfg.head_dim)
        self.k: List[torch.Tensor] = [
            torch.zeros(shape, device=device, dtype=dtype)
            for _ in range(cfg.num_layers)]
        self.v: List[torch.Tensor] = [
            torch.zeros(shape, device=device, dtype=dtype)
            for _ in range(cfg.num_layers)]
        self.n_pages = n_pages
        self.max_slots = max_slots
        self.max_pages_per_seq = max_pages_per_seq
        self.block_table = torch.zeros(max_slots, max_pages_per_seq,
                                       dtype=torch.int32, device=device)
        self.pos = torch.full((max_slots,), -1, dtype=torch.int64,
                              device=device)
        # host side; pages are handed out from the END of free_pages
        self.free_pages: List[int] = list(range(n_pages - 1, -1, -1))
        self.owned: List[List[int]] = [[] for _ in range(max_slots)]
        self.reserved: List[int] = [0] * max_slots
        self.host_pos: List[int] = [-1] * max_slots
        # prompt rows a slot under paged prefill holds so far; -1 = the
        # slot is not prefilling (idle or decoding)
        self.prefilled: List[int] = [-1] * max_slots

    # -- accounting ------------------------------------------------------
    @property
    def pages_free(self) -> int:
        return len(self.free_pages)

    @property
    def pages_unreserved(self) -> int:
        """Free pages not promised to an admitted slot."""
        promised = sum(r - len(o) for r, o in zip(self.reserved, self.owned))
        return len(self.free_pages) - promised

    def can_ever_fit(self, n_rows: int) -> bool:
        return pages_for(n_rows) <= min(self.n_pages,
                                        self.max_pages_per_seq)

    # -- slot lifecycle --------------------------------------------------
    def admit(self, slot: int, n_rows_reserved: int) -> bool:
        """Reserve the pages `n_rows_reserved` cache rows need for an idle
        slot. False = does not fit now (wait for a release); ValueError =
        can never fit this cache."""
        assert self.reserved[slot] == 0 and not self.owned[slot], \
            f"slot {slot} is in use"
        need = pages_for(max(1, n_rows_reserved))
        if not self.can_ever_fit(n_rows_reserved):
            raise ValueError(
                f"{n_rows_reserved} rows need {need} pages; the cache has "
                f"{self.n_pages} and allows {self.max_pages_per_seq} per "
                "sequence")
        if need > self.pages_unreserved:
            return False
        self.reserved[slot] = need
        return True

    def grow(self, slot: int) -> int:
        """Take the slot's next physical page out of its reservation."""
        j = len(self.owned[slot])
        assert j < self.reserved[slot], \
            f"slot {slot} grows past its {self.reserved[slot]} reserved pages"
        page = self.free_pages.pop()
        self.owned[slot].append(page)
        self.block_table[slot, j] = page
        return page

    def ensure_row(self, slot: int, row: int) -> None:
        """Own every page up to the one holding `row`."""
        while len(self.owned[slot]) <= row // PAGE_ROWS:
            self.grow(slot)

    def set_pos(self, slot: int, pos: int) -> None:
        self.host_pos[slot] = pos
        self.pos[slot] = pos

    def advance(self) -> None:
        """Host mirror of the step's in-kernel `pos += (pos >= 0)`."""
        self.host_pos = [p + 1 if p >= 0 else p for p in self.host_pos]

    def release(self, slot: int) -> None:
        """Return the slot's pages and reservation; the slot goes idle."""
        self.free_pages.extend(reversed(self.owned[slot]))
        self.owned[slot] = []
        self.reserved[slot] = 0
        self.prefilled[slot] = -1
        self.block_table[slot].zero_()
        self.set_pos(slot, -1)

    def load_prefix(self, slot: int, k_layers, v_layers,
                    length: int) -> None:
        """Scatter rows 0..length-1 of a contiguous cache (per layer
        [n_kv, >=length, D]) into the slot's pages and put the slot at
        position `length`, the row its next token will occupy. Torch ops,
        off the hot path."""
        assert 0 < length
        self.ensure_row(slot, length)
        n_full = pages_for(length)
        pages = torch.tensor(self.owned[slot][:n_full], dtype=torch.long,
                             device=self.pos.device)
        pad = n_full * PAGE_ROWS - length
        for pool, layers in ((self.k, k_layers), (self.v, v_layers)):
            for li, src in enumerate(layers):
                src = src[:, :length].to(pool[li].dtype)
                if pad:
                    src = torch.nn.functional.pad(src, (0, 0, 0, pad))
                n_kv, _, D = src.shape
                pool[li][pages] = src.reshape(
                    n_kv, n_full, PAGE_ROWS, D).transpose(0, 1)
        self.set_pos(slot, length)

    # -- validation ------------------------------------------------------
    def check_block_table(self) -> None:
        """Raise AssertionError unless the table is consistent: device
        table and positions equal the host mirror, entries in range, no
        page owned twice, no owned page on the free list, every page
        accounted for, positions inside the owned pages. A slot without a
        position owns pages only while it is being prefilled, and then
        exactly the pages of the rows prefilled so far."""
        table = self.block_table.cpu().tolist()
        pos = self.pos.cpu().tolist()
        seen = set()
        free = set(self.free_pages)
        assert len(free) == len(self.free_pages), "duplicate free page"
        for s in range(self.max_slots):
            own = self.owned[s]
            assert len(own) <= self.reserved[s] <= self.max_pages_per_seq, \
                f"slot {s} owns {len(own)} of {self.reserved[s]} reserved"
            assert pos[s] == self.host_pos[s], \
                f"slot {s} device pos {pos[s]} != host {self.host_pos[s]}"
            # the next row may open a page that the next step takes
            assert pos[s] <= len(own) * PAGE_ROWS \
                and pos[s] < max(1, self.reserved[s]) * PAGE_ROWS, \
                f"slot {s} pos {pos[s]} beyond its {len(own)} pages"
            if pos[s] < 0 and self.prefilled[s] >= 0:
                assert len(own) == pages_for(self.prefilled[s]), \
                    f"prefilling slot {s} owns {len(own)} pages for " \
                    f"{self.prefilled[s]} rows"
            elif pos[s] < 0:
                assert not own, f"idle slot {s} owns pages"
            else:
                assert self.prefilled[s] < 0, \
                    f"slot {s} decodes while marked prefilling"
            for j, page in enumerate(table[s][:len(own)]):
                assert page == own[j], \
                    f"slot {s} page {j}: device {page} != host {own[j]}"
                assert 0 <= page < self.n_pages, f"page {page} out of range"
                assert page not in seen, f"page {page} owned twice"
                assert page not in free, f"owned page {page} is free"
                seen.add(page)
        assert len(seen) + len(free) == self.n_pages, "page leaked"
        assert self.pages_unreserved >= 0, "more reserved than free"


@torch.no_grad()
def _step_paged(model, cur: torch.Tensor,
                cache: PagedKVCache) -> torch.Tensor:
    """One decode step for every slot of a paged cache: cur [B, 1] token
    ids (B = cache.max_slots; idle slots carry any valid id) -> logits
    [B, V]. decode_graph._step_static with the two paged calls; positions
    and pages are read on the device and the step ends by advancing every
    active position, so all shapes are fixed and the call is
    stream-capturable. Rows of idle slots come out finite and unused."""
    cfg = model.cfg
    B = cur.shape[0]
    scale = 1.0 / math.sqrt(cfg.head_dim)

    def attend(li, blk, qkv):
        q = rope_cache_paged(qkv.reshape(B, -1), cache.k[li], cache.v[li],
                             model.inv_freq, cache.block_table, cache.pos,
                             cfg.num_heads, cfg.num_kv_heads)
        q = q[:, :, None, :]                               # [B, nh, 1, D]
        o = decode_attention_paged(q, cache.k[li], cache.v[li],
                                   cache.block_table, cache.pos, scale)
        if o is None:                 # off-GPU or head_dim != 128: twin
            o = reference.decode_attention_paged(
                q, cache.k[li], cache.v[li], cache.block_table, cache.pos,
                scale)
        return o

    x, residual = _layers_cached(model, model.embed(cur), attend)  # [B, 1, H]
    normed, _ = fused_rmsnorm(x, model.final_norm_weight, residual,
                              cfg.norm_eps)
    logits = decode_linear(normed, model.lm_head.weight)
    cache.pos.add_((cache.pos >= 0).to(cache.pos.dtype))   # in-graph advance
    return logits.reshape(B, -1)


@torch.no_grad()
def _prefill_paged(model, tokens: torch.Tensor, cache: PagedKVCache,
                   chunks, last_rows) -> torch.Tensor:
    """One packed prefill forward straight into the pages: tokens [1, T]
    are the concatenated chunks = [(slot, pos0, n_tokens), ...] of several
    sequences, whose pages up to each chunk's last row the caller owns
    (ensure_row). Every layer ropes q/k at the tokens' own positions and
    writes k/v into the pages (ops.rope_cache_paged_rows), then attends
    the cache rows 0..position through the block table
    (ops.prefill_attention_paged). last_rows names the packed rows that
    end a prompt; only those go through the final norm and lm_head:
    returns logits [len(last_rows), V]. cache.pos is neither read nor
    written: a slot stays idle for the decode step until the engine sets
    its position."""
    cfg = model.cfg
    T = tokens.shape[1]
    dev = tokens.device
    scale = 1.0 / math.sqrt(cfg.head_dim)
    work, tok_slot, tok_pos = prefill_work(chunks, dev)
    assert tok_slot.numel() == T, (tok_slot.numel(), T)

    def attend(li, blk, qkv):
        q = rope_cache_paged_rows(qkv.reshape(T, -1), cache.k[li],
                                  cache.v[li], model.inv_freq,
                                  cache.block_table, tok_slot, tok_pos,
                                  cfg.num_heads, cfg.num_kv_heads)
        o = prefill_attention_paged(q, cache.k[li], cache.v[li],
                                    cache.block_table, work, scale)
        if o is None:                 # off-GPU or head_dim != 128: twin
            o = reference.prefill_attention_paged(
                q, cache.k[li], cache.v[li], cache.block_table, work, scale)
        return o

    x, residual = _layers_cached(model, model.embed(tokens),   # [1, T, H]
                                 attend)
    if not last_rows:                 # no prompt ends in this batch
        return x.new_zeros(0, model.lm_head.weight.shape[0])
    rows = torch.tensor(list(last_rows), dtype=torch.long, device=dev)
    x = x[:, rows]
    if residual is not None:
        residual = residual[:, rows]
    normed, _ = fused_rmsnorm(x.contiguous(), model.final_norm_weight,
                              None if residual is None
                              else residual.contiguous(), cfg.norm_eps)
    logits = decode_linear(normed, model.lm_head.weight)
    return logits.reshape(len(rows), -1)


class PagedRequest:
    """One sequence in the engine. `tokens` grows from the prompt;
    `done` is set when it finished (or failed: `error`). With paged
    prefill, `n_prefilled` counts the prompt tokens already in the pages
    and `prefilling` holds until the whole prompt is."""

    def __init__(self, rid: int, prompt: List[int], max_new_tokens: int,
                 temperature: float, top_k: int, eos_token: Optional[int],
                 seed: Optional[int]):
        self.id = rid
        self.prompt_len = len(prompt)
        self.tokens: List[int] = list(prompt)
        self.max_new_tokens = max_new_tokens
        self.temperature = temperature
        self.top_k = top_k
        self.eos_token = eos_token
        self.generator = None
        if seed is not None:
            self.generator = torch.Generator(device="cpu").manual_seed(seed)
        self.slot: Optional[int] = None
        self.prefilling = False
        self.n_prefilled = 0
        self.admit_seq = -1           # admission order among prefilling slots
        self.error: Optional[BaseException] = None
        self.done = threading.Event()

    @property
    def n_new(self) -> int:
        return len(self.tokens) - self.prompt_len

    @property
    def finished(self) -> bool:
        return (self.n_new >= self.max_new_tokens
                or (self.eos_token is not None and self.n_new > 0
                    and self.tokens[-1] == self.eos_token))


class PagedEngine:
    """Continuous-batching decode over one PagedKVCache.

    submit() may be called from any thread; step()/run() from one. Each
    step() first refills free slots from the queue (in arrival order; a
    request whose reservation does not fit now waits, and holds back the
    ones behind it), then decodes one token for every active slot.

    graph=True captures _step_paged once at max_slots and replays it; the
    host writes tokens, table rows and positions between replays. Like
    the contiguous decode graph it is opt-in and validated outside the
    test suite (scripts/graphcheck.py --paged).

    prefill="contiguous" (default) prefills each admitted request at once
    on a temporary batch-1 contiguous cache and pages the result in.
    prefill="paged" admits a request as *prefilling* (slot taken, pages
    reserved, device position still -1 so the decode step skips it) and
    every step() packs up to `prefill_chunk` prompt tokens of the
    prefilling slots, in admission order, into one _prefill_paged forward
    that writes the pages directly: short prompts share a batch, a long
    prompt spans several steps while the other slots keep decoding. A
    prompt that completes gets its first token and joins the same step's
    decode. Prefill always runs eagerly, between graph replays.
    """

    def __init__(self, model, max_slots: int = 8,
                 n_pages: Optional[int] = None,
                 max_pages_per_seq: Optional[int] = None,
                 graph: bool = False, prefill: str = "contiguous",
                 prefill_chunk: int = 512):
        if prefill not in ("contiguous", "paged"):
            raise ValueError(f"prefill must be 'contiguous' or 'paged', "
                             f"not {prefill!r}")
        if prefill == "paged" and prefill_chunk < 1:
            raise ValueError("prefill_chunk must be >= 1")
        self.prefill = prefill
        self.prefill_chunk = int(prefill_chunk)
        self.prefill_steps = 0
        self._admit_seq = 0
        self.model = model
        self.device = model.embed.weight.device
        if n_pages is None:
            n_pages = 32 * max_slots           # 2048 rows per slot
        if max_pages_per_seq is None:
            max_pages_per_seq = min(n_pages, 128)
        self.max_slots = max_slots
        self.cache = PagedKVCache(model.cfg, n_pages, max_slots,
                                  max_pages_per_seq, self.device,
                                  model.embed.weight.dtype)
        self.cur = torch.zeros(max_slots, dtype=torch.long,
                               device=self.device)
        self._host_cur = [0] * max_slots
        self.slots: List[Optional[PagedRequest]] = [None] * max_slots
        self.queue: deque = deque()
        self._lock = threading.Lock()
        self._work = threading.Condition(self._lock)
        self._next_id = 0
        self.graph_mode = bool(graph) and self.device.type == "cuda"
        self._graph = None
        self._graph_logits = None
        self.steps = 0

    # -- queue -----------------------------------------------------------
    def submit_request(self, prompt, max_new_tokens: int,
                       temperature: float = 0.0, top_k: int = 0,
                       eos_token: Optional[int] = None,
                       seed: Optional[int] = None) -> PagedRequest:
        """Queue one sequence and hand back the request object (its
        `done` event is what a server handler waits on). ValueError if it
        can never fit the cache."""
        if isinstance(prompt, torch.Tensor):
            prompt = prompt.reshape(-1).tolist()
        prompt = [int(t) for t in prompt]
        if not prompt:
            raise ValueError("empty prompt")
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        rows = len(prompt) + max_new_tokens
        if not self.cache.can_ever_fit(rows):
            raise ValueError(
                f"prompt {len(prompt)} + {max_new_tokens} new tokens needs "
                f"{pages_for(rows)} pages; the cache has "
                f"{self.cache.n_pages} and allows "
                f"{self.cache.max_pages_per_seq} per sequence")
        with self._work:
            req = PagedRequest(self._next_id, prompt, max_new_tokens,
                               temperature, top_k, eos_token, seed)
            self._next_id += 1
            self.queue.append(req)
            self._work.notify_all()
        return req

    def submit(self, prompt, max_new_tokens: int, temperature: float = 0.0,
               top_k: int = 0, eos_token: Optional[int] = None,
               seed: Optional[int] = None) -> int:
        """Queue one sequence; returns its id."""
        return self.submit_request(prompt, max_new_tokens, temperature,
                                   top_k, eos_token, seed).id

    @property
    def n_active(self) -> int:
        return sum(r is not None for r in self.slots)

    @property
    def idle(self) -> bool:
        with self._lock:
            return not self.queue and self.n_active == 0

    def wait_for_work(self, stop: threading.Event) -> None:
        """Block until a request is queued or active, or `stop` is set
        (whoever sets it calls wake())."""
        with self._work:
            while not stop.is_set() and not self.queue \
                    and self.n_active == 0:
                self._work.wait()

    def wake(self) -> None:
        with self._work:
            self._work.notify_all()

    # -- stepping --------------------------------------------------------
    def _pick(self, req: PagedRequest, logits_row: torch.Tensor,
              greedy_tok: Optional[int]) -> int:
        if req.temperature <= 0.0:
            return greedy_tok if greedy_tok is not None \
                else int(logits_row.argmax())
        return int(_sample(logits_row[None].cpu(), req.temperature,
                           req.top_k, req.generator)[0])

    def _retire(self, req: PagedRequest, finished: list) -> None:
        if req.slot is not None:
            self.cache.release(req.slot)
            self.slots[req.slot] = None
            self._host_cur[req.slot] = 0
            req.slot = None
        finished.append(req)
        req.done.set()

    def _admit(self, finished: list) -> None:
        for slot in range(self.max_slots):
            if self.slots[slot] is not None:
                continue
            with self._lock:
                if not self.queue:
                    return
                req = self.queue[0]
                rows = req.prompt_len + req.max_new_tokens
                if not self.cache.admit(slot, rows):
                    return                     # wait for a release
                self.queue.popleft()
            req.slot = slot
            self.slots[slot] = req
            # prefill once on a batch-1 contiguous cache of the prompt's
            # length (the ordinary prefill path), then page it in
            prompt = torch.tensor([req.tokens], dtype=torch.long,
                                  device=self.device)
            tmp = KVCache(self.model.cfg, 1, req.prompt_len, self.device,
                          self.model.embed.weight.dtype)
            last = _forward_cached(self.model, prompt, tmp)[0, -1]
            self.cache.load_prefix(slot, [k[0] for k in tmp.k],
                                   [v[0] for v in tmp.v], req.prompt_len)
            tok = self._pick(req, last, None)
            req.tokens.append(tok)
            if req.finished:
                self._retire(req, finished)
            else:
                self._host_cur[slot] = tok

    def _admit_paged(self) -> None:
        """_admit's slot and reservation rule (arrival order, the same
        cache.admit), without the prefill: the request is marked
        prefilling and its slot's device position stays -1."""
        for slot in range(self.max_slots):
            if self.slots[slot] is not None:
                continue
            with self._lock:
                if not self.queue:
                    return
                req = self.queue[0]
                rows = req.prompt_len + req.max_new_tokens
                if not self.cache.admit(slot, rows):
                    return                     # wait for a release
                self.queue.popleft()
            req.slot = slot
            req.prefilling = True
            req.n_prefilled = 0
            req.admit_seq = self._admit_seq
            self._admit_seq += 1
            self.slots[slot] = req
            self.cache.prefilled[slot] = 0

    def _prefill_step(self, finished: list) -> None:
        """Up to prefill_chunk prompt tokens of the prefilling slots, in
        admission order, through one packed _prefill_paged; prompts that
        complete get their first token and their position."""
        pending = sorted((r for r in self.slots
                          if r is not None and r.prefilling),
                         key=lambda r: r.admit_seq)
        budget = self.prefill_chunk
        chunks, toks, last_rows, completing = [], [], [], []
        for req in pending:
            if budget <= 0:
                break
            n = min(budget, req.prompt_len - req.n_prefilled)
            p0 = req.n_prefilled
            self.cache.ensure_row(req.slot, p0 + n - 1)
            chunks.append((req.slot, p0, n))
            toks.extend(req.tokens[p0:p0 + n])
            budget -= n
            if p0 + n == req.prompt_len:
                last_rows.append(len(toks) - 1)
                completing.append(req)
        if not chunks:
            return
        tokens = torch.tensor([toks], dtype=torch.long, device=self.device)
        logits = _prefill_paged(self.model, tokens, self.cache, chunks,
                                last_rows)
        self.prefill_steps += 1
        for slot, p0, n in chunks:
            self.slots[slot].n_prefilled = p0 + n
            self.cache.prefilled[slot] = p0 + n
        greedy = None
        if any(r.temperature <= 0.0 for r in completing):
            greedy = logits.argmax(dim=-1).tolist()        # one sync
        for i, req in enumerate(completing):
            tok = self._pick(req, logits[i], greedy[i] if greedy else None)
            req.tokens.append(tok)
            req.prefilling = False
            self.cache.prefilled[req.slot] = -1
            if req.finished:
                self._retire(req, finished)
            else:
                self.cache.set_pos(req.slot, req.prompt_len)
                self._host_cur[req.slot] = tok

    def _decode(self) -> torch.Tensor:
        self.cur.copy_(torch.tensor(self._host_cur, dtype=torch.long))
        if not self.graph_mode:
            return _step_paged(self.model, self.cur[:, None], self.cache)
        if self._graph is None:
            self._capture()
        self._graph.replay()
        return self._graph_logits

    def _capture(self) -> None:
        """Warm up and capture _step_paged with EVERY slot idle: an idle
        slot writes no k/v and keeps its position, so neither the warmup
        nor anything the capture might execute disturbs the cache."""
        saved = self.cache.pos.clone()
        self.cache.pos.fill_(-1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                _step_paged(self.model, self.cur[:, None], self.cache)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._graph_logits = _step_paged(self.model, self.cur[:, None],
                                             self.cache)
        self._graph = g
        self.cache.pos.copy_(saved)

    @torch.no_grad()
    def step(self) -> List[PagedRequest]:
        """Refill free slots, decode one token per active slot; returns
        the requests that finished during this step."""
        finished: List[PagedRequest] = []
        try:
            if self.prefill == "paged":
                self._admit_paged()
                self._prefill_step(finished)
            else:
                self._admit(finished)
            active = [r for r in self.slots
                      if r is not None and not r.prefilling]
            if not active:
                return finished
            for req in active:      # page for the row this step writes
                self.cache.ensure_row(req.slot,
                                      self.cache.host_pos[req.slot])
            logits = self._decode()
            self.cache.advance()
            self.steps += 1
            greedy = None
            if any(r.temperature <= 0.0 for r in active):
                greedy = logits.argmax(dim=-1).tolist()    # one sync
            for req in active:
                tok = self._pick(req, logits[req.slot],
                                 greedy[req.slot] if greedy else None)
                req.tokens.append(tok)
                if req.finished:
                    self._retire(req, finished)
                else:
                    self._host_cur[req.slot] = tok
            return finished
        except BaseException as e:
            self._fail_all(e)
            raise

    def _fail_all(self, err: BaseException) -> None:
        """A step raised: nobody may wait forever. Fail every active and
        queued request and hand the pages back."""
        with self._lock:
            pending = list(self.queue)
            self.queue.clear()
        for req in [r for r in self.slots if r is not None] + pending:
            req.error = err
            if req.slot is not None:
                try:
                    self.cache.release(req.slot)
                except Exception:
                    pass
                self.slots[req.slot] = None
                req.slot = None
            req.prefilling = False
            req.done.set()

    def run(self) -> Dict[int, torch.Tensor]:
        """Drain the queue: step until nothing is queued or active.
        Returns {id: tokens (prompt + generated)}."""
        out: Dict[int, torch.Tensor] = {}
        while not self.idle:
            for req in self.step():
                out[req.id] = torch.tensor(req.tokens, dtype=torch.long,
                                           device=self.device)
        return out


@torch.no_grad()
def generate_ragged(model, prompts: List[torch.Tensor], max_new_tokens: int,
                    temperature: float = 0.0, top_k: int = 0,
                    eos_token: Optional[int] = None,
                    seed: Optional[int] = None, max_slots: int = 8,
                    n_pages: Optional[int] = None,
                    graph: bool = False,
                    prefill_chunk: Optional[int] = None
                    ) -> List[torch.Tensor]:
    """generate() for prompts of DIFFERENT lengths: every prompt is its
    own engine request (own position, own pages, own generator seeded
    with `seed`), decoded together `max_slots` at a time. Returns one
    1-D tensor (prompt + generated) per prompt, in order. prefill_chunk:
    None or 0 = prefill each prompt at once on a contiguous cache; N > 0 =
    paged prefill, at most N prompt tokens per engine step."""
    was_training = model.training
    model.eval()
    try:
        need = max(pages_for(int(p.numel()) + max_new_tokens)
                   for p in prompts)
        max_slots = max(1, min(max_slots, len(prompts)))
        if n_pages is None:
            n_pages = need * max_slots
        paged = {"prefill": "paged", "prefill_chunk": int(prefill_chunk)} \
            if prefill_chunk else {}
        eng = PagedEngine(model, max_slots=max_slots, n_pages=n_pages,
                          max_pages_per_seq=need, graph=graph, **paged)
        ids = [eng.submit(p, max_new_tokens, temperature, top_k, eos_token,
                          seed) for p in prompts]
        done = eng.run()
        return [done[i] for i in ids]
    finally:
        if was_training:
            model.train()
