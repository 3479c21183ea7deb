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
from trainingjob_operator_amd.parallel.cp import _block_scores

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--legacy-iters", type=int, default=2)
    ap.add_argument("--legacy-max-gb", type=float, default=150.0,
                    help="skip legacy runs whose score tensors alone "
                         "(~4 live [B,H,Sb,Sb] fp32) exceed this")
    ap.add_argument("--totals", default="8192,32768")
    ap.add_argument("--cps", default="2,4,8")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ringbench needs a GPU"
    scale = D ** -0.5
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
