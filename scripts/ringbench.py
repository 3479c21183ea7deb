#!/usr/bin/env python3
"""Ring-attention microbench on ONE GPU, no process group: the work of the
last context-parallel rank (the one that visits all cp blocks: the causal
diagonal block plus cp-1 full blocks), forward and forward+backward,
through the native block ops and through the legacy fp32-matmul block math
of parallel/cp.py. Reports time and peak allocated memory for each, the
non-causal block forward against aten SDPA, and the time per kv tile of
the non-causal forward against the causal one.

usage: ringbench.py [--iters N] [--legacy-iters N] [--legacy-max-gb G]
                    [--totals 8192,32768] [--cps 2,4,8]
                    [--layout contiguous|zigzag|both] [--rounds N]

With --layout the report is the ring's critical path instead: every virtual
rank's cp_schedule (parallel/cp.py) is timed step by step, forward (block
forward + lse merge) and backward (block backward + the fp32 dq/dK/dV
adds), and each layout gets the sum over ring steps of the SLOWEST rank's
step: what a compute-then-shift ring waits for. "both" alternates the two
layouts --rounds times in one process and adds the contiguous/zigzag ratio
next to the tile-count ratio (cp - 0.5) / (cp / 2); it also times the
rectangular non-causal forwards against the square one per (row block, kv
tile) visit.

Communication is not part of it: K/V blocks are local slices.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from trainingjob_operator_amd.ops.attention import (
    attn_merge_, flash_attention_block_bwd, flash_attention_block_fwd,
    flash_attention_delta)
from trainingjob_operator_amd.parallel.cp import (
    _block_scores, _part, cp_schedule)

B, H, HKV, D = 1, 32, 8, 128
DEV = "cuda"


def timed(fn, warmup, iters):
    """(us per call, peak bytes allocated above the resident inputs)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / iters * 1e6
    return us, torch.cuda.max_memory_allocated() - base


def block_fwd(q, ks, vs, scale):
    """_RingAttention._block_forward of the last rank, blocks r..0."""
    Sb = q.shape[2]
    o_acc = torch.zeros(B, H, Sb, D, dtype=torch.float32, device=DEV)
    lse_acc = torch.full((B, H, Sb), float("-inf"), dtype=torch.float32,
                         device=DEV)
    for i, (kj, vj) in enumerate(zip(ks, vs)):
        o_j, lse_j = flash_attention_block_fwd(q, kj, vj, i == 0, scale)
        attn_merge_(o_acc, lse_acc, o_j, lse_j)
    return o_acc.to(q.dtype), lse_acc


def block_fwd_bwd(q, ks, vs, dout, scale):
    out, lse = block_fwd(q, ks, vs, scale)
    delta = flash_attention_delta(out, dout)
    dq = torch.zeros(q.shape, dtype=torch.float32, device=DEV)
    for i, (kj, vj) in enumerate(zip(ks, vs)):
        dq_b, dk_b, dv_b = flash_attention_block_bwd(
            q, kj, vj, dout, lse, delta, i == 0, scale)
        dq += dq_b
        # the travelling fp32 dK/dV accumulators of the ring
        dk_b.float()
        dv_b.float()
    return dq.to(q.dtype)


def legacy_fwd(q, ks, vs, scale):
    """The legacy loop body of _RingAttention.forward (kv heads expanded)."""
    Sb = q.shape[2]
    q32 = q.float()
    o = torch.zeros(B, H, Sb, D, dtype=torch.float32, device=DEV)
    m = torch.full((B, H, Sb, 1), float("-inf"), device=DEV)
    l = torch.zeros(B, H, Sb, 1, device=DEV)
    for i, (kj, vj) in enumerate(zip(ks, vs)):
        s = _block_scores(q32, kj, scale, diagonal=(i == 0))
        m_new = torch.maximum(m, s.amax(dim=-1, keepdim=True))
        p = torch.exp(s - m_new)
        alpha = torch.exp(m - m_new)
        l = l * alpha + p.sum(dim=-1, keepdim=True)
        o = o * alpha + torch.matmul(p, vj.float())
        m = m_new
    return o / l, m + torch.log(l)


def legacy_fwd_bwd(q, ks, vs, dout, scale):
    out32, lse = legacy_fwd(q, ks, vs, scale)
    q32, do32 = q.float(), dout.float()
    delta = (do32 * out32).sum(dim=-1, keepdim=True)
    dq = torch.zeros_like(q32)
    for i, (kj, vj) in enumerate(zip(ks, vs)):
        s = _block_scores(q32, kj, scale, diagonal=(i == 0))
        p = torch.exp(s - lse)
        dvj = torch.matmul(p.transpose(-1, -2), do32)
        dp = torch.matmul(do32, vj.float().transpose(-1, -2))
        ds = p * (dp - delta)
        dq += scale * torch.matmul(ds, kj.float())
        dkj = scale * torch.matmul(ds.transpose(-1, -2), q32)
        del dvj, dkj
    return dq.to(q.dtype)


def ring_critical_path(S, cp, layout, scale, iters):
    """Per-step times of every virtual rank under cp_schedule(layout) and
    the ring's critical path (sum over steps of the slowest rank)."""
    Sb = S // cp
    g = torch.Generator(device=DEV).manual_seed(S + cp)

    def rnd(*shape):
        return (torch.randn(*shape, device=DEV, generator=g) * .5).bfloat16()
    ks = [rnd(B, HKV, Sb, D) for _ in range(cp)]
    vs = [rnd(B, HKV, Sb, D) for _ in range(cp)]
    parts = ("full",) if layout == "contiguous" else ("lo", "hi")
    rows = Sb // len(parts)
    fwd = [[0.0] * cp for _ in range(cp)]       # [rank][step] us
    bwd = [[0.0] * cp for _ in range(cp)]
    for r in range(cp):
        q, dout = rnd(B, H, Sb, D), rnd(B, H, Sb, D)
        sched = cp_schedule(layout, cp, r)
        acc = [(torch.zeros(B, H, rows, D, dtype=torch.float32, device=DEV),
                torch.full((B, H, rows), float("-inf"), dtype=torch.float32,
                           device=DEV)) for _ in parts]

        def fwd_step(j, qp, kvp, causal):
            o_j, lse_j = flash_attention_block_fwd(
                _part(q, qp), _part(ks[j], kvp), _part(vs[j], kvp), causal,
                scale)
            if qp == "full":
                for (o_acc, lse_acc), p in zip(acc, parts):
                    attn_merge_(o_acc, lse_acc, _part(o_j, p),
                                _part(lse_j, p))
            else:
                attn_merge_(acc[1][0], acc[1][1], o_j, lse_j)

        for t, (j, qp, kvp, causal) in enumerate(sched):
            if qp is not None:
                fwd[r][t], _ = timed(lambda: fwd_step(j, qp, kvp, causal), 1,
                                     iters)
        # the repeated merges only raised lse: P = exp(s - lse) stays <= 1
        out = torch.cat([a[0] for a in acc], dim=2).to(q.dtype)
        lse = torch.cat([a[1] for a in acc], dim=2)
        delta = flash_attention_delta(out, dout)
        dq = torch.zeros(q.shape, dtype=torch.float32, device=DEV)
        dkj = torch.zeros(ks[0].shape, dtype=torch.float32, device=DEV)
        dvj = torch.zeros(vs[0].shape, dtype=torch.float32, device=DEV)

        def bwd_step(j, qp, kvp, causal):
            dq_b, dk_b, dv_b = flash_attention_block_bwd(
                _part(q, qp), _part(ks[j], kvp), _part(vs[j], kvp),
                _part(dout, qp), _part(lse, qp), _part(delta, qp), causal,
                scale)
            _part(dq, qp).add_(dq_b)
            _part(dkj, kvp).add_(dk_b)
            _part(dvj, kvp).add_(dv_b)

        for t, (j, qp, kvp, causal) in enumerate(sched):
            if qp is not None:
                bwd[r][t], _ = timed(lambda: bwd_step(j, qp, kvp, causal), 1,
                                     iters)
        del q, dout, acc, out, lse, delta, dq, dkj, dvj
    crit_f = sum(max(fwd[r][t] for r in range(cp)) for t in range(cp))
    crit_b = sum(max(bwd[r][t] for r in range(cp)) for t in range(cp))
    return dict(
        S=S, cp=cp, Sb=Sb, layout=layout, ring_fwd_us=crit_f,
        ring_bwd_us=crit_b, ring_fwdbwd_us=crit_f + crit_b,
        rank_fwd_us=[sum(x) for x in fwd], rank_bwd_us=[sum(x) for x in bwd],
        slowest_fwd_step_us=[max(fwd[r][t] for r in range(cp))
                             for t in range(cp)],
        slowest_bwd_step_us=[max(bwd[r][t] for r in range(cp))
                             for t in range(cp)])


def rect_vs_square(Sb, scale, iters):
    """Non-causal forward: ns per (row block, kv tile) visit of the square
    Sb x Sb block and of the two rectangular blocks of a zig-zag step."""
    g = torch.Generator(device=DEV).manual_seed(Sb)

    def rnd(*shape):
        return (torch.randn(*shape, device=DEV, generator=g) * .5).bfloat16()
    q, k, v = rnd(B, H, Sb, D), rnd(B, HKV, Sb, D), rnd(B, HKV, Sb, D)
    row = dict(Sb=Sb)
    for name, qp, kvp in (("square", "full", "full"),
                          ("full_x_lo", "full", "lo"),
                          ("hi_x_full", "hi", "full")):
        qq, kk, vv = _part(q, qp), _part(k, kvp), _part(v, kvp)
        us, _ = timed(lambda: flash_attention_block_fwd(qq, kk, vv, False,
                                                        scale), 3, iters)
        visits = B * H * (qq.shape[2] // 256) * (kk.shape[2] // 64)
        row[f"{name}_fwd_us"] = us
        row[f"{name}_ns_per_visit"] = us * 1e3 / visits
    return row


def layout_report(args, scale):
    layouts = (["contiguous", "zigzag"] if args.layout == "both"
               else [args.layout])
    seen_sb = set()
    for S in (int(x) for x in args.totals.split(",")):
        for cp in (int(x) for x in args.cps.split(",")):
            got = {}
            for rnd_i in range(args.rounds):
                for layout in layouts:          # alternated, one process
                    row = ring_critical_path(S, cp, layout, scale,
                                             args.iters)
                    row["round"] = rnd_i
                    got.setdefault(layout, []).append(row)
                    print(json.dumps(row), flush=True)
                    torch.cuda.empty_cache()
            if len(layouts) == 2:
                best = {lay: {k: min(r[k] for r in rows) for k in
                              ("ring_fwd_us", "ring_bwd_us",
                               "ring_fwdbwd_us")}
                        for lay, rows in got.items()}
                print(json.dumps(dict(
                    S=S, cp=cp, tile_count_ratio=(cp - 0.5) / (cp / 2),
                    **{f"{k}_contiguous_over_zigzag":
                       best["contiguous"][k] / best["zigzag"][k]
                       for k in best["zigzag"]})), flush=True)
            Sb = S // cp
            if "zigzag" in layouts and Sb % 512 == 0 and Sb not in seen_sb:
                seen_sb.add(Sb)
                print(json.dumps(rect_vs_square(Sb, scale, args.iters)),
                      flush=True)
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--legacy-iters", type=int, default=2)
    ap.add_argument("--legacy-max-gb", type=float, default=150.0,
                    help="skip legacy runs whose score tensors alone "
                         "(~4 live [B,H,Sb,Sb] fp32) exceed this")
    ap.add_argument("--totals", default="8192,32768")
    ap.add_argument("--cps", default="2,4,8")
    ap.add_argument("--layout", choices=("contiguous", "zigzag", "both"),
                    default=None,
                    help="report the ring's critical path per cp layout "
                         "(see the module docstring) instead of the last "
                         "rank's block-vs-legacy comparison")
    ap.add_argument("--rounds", type=int, default=2,
                    help="with --layout: how often the layouts alternate")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ringbench needs a GPU"
    scale = D ** -0.5
    if args.layout:
        return layout_report(args, scale)
    rows = []
    seen_sb = set()
    for S in (int(x) for x in args.totals.split(",")):
        for cp in (int(x) for x in args.cps.split(",")):
            Sb = S // cp
            g = torch.Generator(device=DEV).manual_seed(S + cp)

            def rnd(*shape):
                return (torch.randn(*shape, device=DEV, generator=g)
                        * .5).bfloat16()
            q, dout = rnd(B, H, Sb, D), rnd(B, H, Sb, D)
            # the last rank's visit order: its own block, then r-1 .. 0
            ks = [rnd(B, HKV, Sb, D) for _ in range(cp)]
            vs = [rnd(B, HKV, Sb, D) for _ in range(cp)]
            row = dict(S=S, cp=cp, Sb=Sb)
            us, mem = timed(lambda: block_fwd(q, ks, vs, scale), 2,
                            args.iters)
            row["block_fwd_us"], row["block_fwd_peak_mb"] = us, mem / 2**20
            us, mem = timed(lambda: block_fwd_bwd(q, ks, vs, dout, scale), 2,
                            args.iters)
            row["block_fwdbwd_us"], row["block_fwdbwd_peak_mb"] = \
                us, mem / 2**20
            est_gb = 4 * B * H * Sb * Sb * 4 / 2**30
            if est_gb <= args.legacy_max_gb:
                try:
                    G = H // HKV
                    kse = [k.repeat_interleave(G, dim=1) for k in ks]
                    vse = [v.repeat_interleave(G, dim=1) for v in vs]
                    us, mem = timed(lambda: legacy_fwd(q, kse, vse, scale), 1,
                                    args.legacy_iters)
                    row["legacy_fwd_us"], row["legacy_fwd_peak_mb"] = \
                        us, mem / 2**20
                    us, mem = timed(
                        lambda: legacy_fwd_bwd(q, kse, vse, dout, scale), 1,
                        args.legacy_iters)
                    row["legacy_fwdbwd_us"], row["legacy_fwdbwd_peak_mb"] = \
                        us, mem / 2**20
                except torch.OutOfMemoryError:
                    row["legacy_oom"] = True
                kse = vse = None
            else:
                row["legacy_skipped_est_gb"] = est_gb
            if Sb not in seen_sb:
                seen_sb.add(Sb)
                k0, v0 = ks[0], vs[0]
                nc, _ = timed(lambda: flash_attention_block_fwd(
                    q, k0, v0, False, scale), 3, args.iters)
                ca, _ = timed(lambda: flash_attention_block_fwd(
                    q, k0, v0, True, scale), 3, args.iters)
                at, _ = timed(lambda: F.scaled_dot_product_attention(
                    q, k0, v0, is_causal=False, enable_gqa=True), 3,
                    args.iters)
                nqb = Sb // 256
                row["noncausal_fwd_us"] = nc
                row["causal_fwd_us"] = ca
                row["aten_noncausal_fwd_us"] = at
                # (workgroup, kv tile) visits: every tile vs up to the diagonal
                row["noncausal_ns_per_tile"] = \
                    nc * 1e3 / (B * H * nqb * (Sb // 64))
                row["causal_ns_per_tile"] = \
                    ca * 1e3 / (B * H * 2 * nqb * (nqb + 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del q, dout, ks, vs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
