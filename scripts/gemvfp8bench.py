#!/usr/bin/env python3
"""fp8 decode GEMVs against the route the same rows take without them, on
the llama3-8b decode shapes: gemv_bf16 / gemv_swiglu up to 8 rows, F.linear
(+ swiglu_packed) at 16.

Each route is timed as a captured graph of 64 launches, replayed until the
window is about 0.1 s, so that the launch interval of the host does not
stand in for a kernel of a few microseconds. The launches of a graph walk
round enough copies of the weight (512 MB of fp8, 1 GB of bf16) that no
launch finds its weight in a cache the one before it filled. The two routes
alternate inside every round; reported are the median time per launch over
the rounds, the spread (max - min) and the weight bytes per second, with the
share of the weight-stream floor at peak HBM bandwidth."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from trainingjob_operator_amd.ops import (decode_linear, decode_linear_fp8,
                                          decode_swiglu, decode_swiglu_fp8,
                                          native, swiglu_packed)
from trainingjob_operator_amd.ops.fp8_weight import quantize_rows

PEAK_HBM = 8.0e12                     # B/s, MI355X HBM3E
SHAPES = [("qkv", 6144, 4096, False), ("o", 4096, 4096, False),
          ("gate_up", 28672, 4096, True), ("down", 4096, 14336, False),
          ("lm_head", 128256, 4096, False)]


LAUNCHES = 64


def _graph(fn, copies):
    """A captured graph of LAUNCHES calls of fn over the copies in turn."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for c in copies:
            fn(c)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(LAUNCHES):
            fn(copies[i % len(copies)])
    return g


def _time(g, replays):
    """us per launch."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (replays * LAUNCHES) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1,
                    help="seconds of replays per sample")
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 4, 8, 16])
    args = ap.parse_args()
    lib = native.load(require=True)
    torch.manual_seed(0)
    print("| shape | N | split | fp8 us (spread) | fp8 TB/s | of floor | "
          "parent us (spread) | parent TB/s | of floor | parent/fp8 |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name, M, K, gate_up in SHAPES:
        n_copies = -(-(512 << 20) // (M * K))
        ws, w8s = [], []
        for _ in range(n_copies):
            w = (torch.randn(M, K, device="cuda") * K ** -0.5).bfloat16()
            w8 = quantize_rows(w, gate_up=gate_up)
            w.copy_(w8.dequant())
            ws.append(w)
            w8s.append(w8)
        split = lib.gemv_fp8_split((M // 2 if gate_up else M) // 16, K)
        for N in args.rows:
            x = torch.randn(N, K, device="cuda").bfloat16()
            if gate_up:
                def fp8(w8):
                    return decode_swiglu_fp8(x, w8)

                def parent(w):
                    h = decode_swiglu(x, w)
                    return h if h is not None else swiglu_packed(
                        decode_linear(x, w))
            else:
                def fp8(w8):
                    return decode_linear_fp8(x, w8)

                def parent(w):
                    return decode_linear(x, w)
            a, b = fp8(w8s[0]).float(), parent(ws[0]).float()
            err = (a - b).abs().max().item()
            assert err <= 2e-2 * b.abs().max().item() + 2e-2, (name, N, err)
            g8, gp = _graph(fp8, w8s), _graph(parent, ws)
            r8 = max(2, int(args.window / (_time(g8, 2) * LAUNCHES * 1e-6)))
            rp = max(2, int(args.window / (_time(gp, 2) * LAUNCHES * 1e-6)))
            t8, tp = [], []
            for _ in range(args.rounds):
                t8.append(_time(g8, r8))
                tp.append(_time(gp, rp))
            m8, mp = statistics.median(t8), statistics.median(tp)
            b8, bp = M * K, 2 * M * K               # weight bytes
            print(f"| {name} {M}x{K} | {N} | {split} | {m8:.1f} "
                  f"({max(t8) - min(t8):.1f}) | {b8 / m8 / 1e6:.2f} | "
                  f"{b8 / PEAK_HBM / (m8 * 1e-6):.0%} | {mp:.1f} "
                  f"({max(tp) - min(tp):.1f}) | {bp / mp / 1e6:.2f} | "
                  f"{bp / PEAK_HBM / (mp * 1e-6):.0%} | {mp / m8:.2f}x |",
                  flush=True)
            del g8, gp
        del ws, w8s


if __name__ == "__main__":
    main()
