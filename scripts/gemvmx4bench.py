#!/usr/bin/env python3
"""MXFP4 decode GEMVs against the fp8 GEMVs and against the bf16 route
(gemv_bf16 / gemv_swiglu up to 8 rows, F.linear + swiglu_packed at 16), on
the llama3-8b decode shapes.

The method is gemvfp8bench.py's: each side is timed as a captured graph of 64
launches, replayed until the window is about 0.1 s; the launches walk round
enough copies of the weight (512 MB of MXFP4, 1 GB of fp8, 2 GB of bf16)
that no launch finds its weight in a cache; the sides alternate inside every
round; reported are the median time per launch, the spread (max - min) and
the share of the side's own byte floor (weight and scale bytes at peak HBM
bandwidth). Every side has its own weights (its own quantisation of the same
random values), the MXFP4 ones written back for the bf16 route.

--ab times the kernel's variants instead (gemv_mx4_ab): the loads of one or
of two chunks in flight per wave, at the rule's split, half and twice it."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from trainingjob_operator_amd.ops import (decode_linear, decode_linear_fp8,
                                          decode_linear_mx4, decode_swiglu,
                                          decode_swiglu_fp8,
                                          decode_swiglu_mx4, native,
                                          swiglu_packed)
from trainingjob_operator_amd.ops.fp8_weight import quantize_rows
from trainingjob_operator_amd.ops.mx4_weight import quantize_mx4

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
    return (time.perf_counter() - t0) / (replays * LAUNCHES * 1e-6)


def _rounds(graphs, args):
    """{side: [us per launch, one per round]}, sides alternating."""
    reps = {k: max(2, int(args.window / (_time(g, 2) * LAUNCHES * 1e-6)))
            for k, g in graphs.items()}
    t = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k, g in graphs.items():
            t[k].append(_time(g, reps[k]))
    return t


def _cell(t, floor_bytes):
    m = statistics.median(t)
    return (f"{m:.1f} ({max(t) - min(t):.1f}) | "
            f"{floor_bytes / PEAK_HBM / (m * 1e-6):.0%}")


def _sides(M, K, gate_up):
    n_copies = -(-(1 << 30) // (M * K))
    ws, w8s, w4s = [], [], []
    for _ in range(n_copies):
        w = (torch.randn(M, K, device="cuda") * K ** -0.5).bfloat16()
        w8s.append(quantize_rows(w, gate_up=gate_up))
        w4s.append(quantize_mx4(w, gate_up=gate_up))
        w.copy_(w4s[-1].dequant())
        ws.append(w)
    return ws, w8s, w4s


def compare(args, lib):
    print("| shape | N | mx4 us (spread) | of floor | fp8 us (spread) | "
          "of floor | bf16 us (spread) | of floor | fp8/mx4 | bf16/mx4 |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name, M, K, gate_up in SHAPES:
        ws, w8s, w4s = _sides(M, K, gate_up)
        for N in args.rows:
            x = torch.randn(N, K, device="cuda").bfloat16()

            def bf16(w):
                if not gate_up:
                    return decode_linear(x, w)
                h = decode_swiglu(x, w)
                return h if h is not None else swiglu_packed(
                    decode_linear(x, w))
            lin8 = decode_swiglu_fp8 if gate_up else decode_linear_fp8
            lin4 = decode_swiglu_mx4 if gate_up else decode_linear_mx4
            a, b = lin4(x, w4s[0]).float(), bf16(ws[0]).float()
            err = (a - b).abs().max().item()
            assert err <= 2e-2 * b.abs().max().item() + 2e-2, (name, N, err)
            t = _rounds({"mx4": _graph(lambda w: lin4(x, w), w4s),
                         "fp8": _graph(lambda w: lin8(x, w), w8s),
                         "bf16": _graph(bf16, ws)}, args)
            m = {k: statistics.median(v) for k, v in t.items()}
            e = M * K
            print(f"| {name} {M}x{K} | {N} | "
                  f"{_cell(t['mx4'], e // 2 + e // 32)} | "
                  f"{_cell(t['fp8'], e + 4 * M)} | {_cell(t['bf16'], 2 * e)} "
                  f"| {m['fp8'] / m['mx4']:.2f}x | "
                  f"{m['bf16'] / m['mx4']:.2f}x |", flush=True)
        del ws, w8s, w4s


def ab(args, lib):
    print("| shape | N | rule split | variant: us (spread), of floor |")
    print("|---|---|---|---|")
    for name, M, K, gate_up in SHAPES:
        rows = M // 2 if gate_up else M
        _, _, w4s = _sides(M, K, gate_up)
        rule = lib.gemv_mx4_split(rows // 16, K)
        splits = [s for s in (rule // 2, rule, rule * 2)
                  if 1 <= s <= min(8, K // 512)]
        for N in args.rows:
            x = torch.randn(N, K, device="cuda").bfloat16()
            y = torch.empty(N, rows, device="cuda", dtype=torch.bfloat16)

            def variant(two, split):
                def fn(w4):
                    rc = lib.gemv_mx4_ab(native.stream_ptr(), int(gate_up),
                                         two, split, w4.packed.data_ptr(),
                                         w4.scale.data_ptr(), x.data_ptr(),
                                         y.data_ptr(), rows, K, N)
                    native.check_rc(rc, "gemv_mx4_ab", f"{name} {split}")
                return fn
            t = _rounds({f"{'two' if two else 'one'}/s{s}":
                         _graph(variant(two, s), w4s)
                         for s in splits for two in (0, 1)}, args)
            e = M * K
            cells = "; ".join(f"{k}: {_cell(v, e // 2 + e // 32)}"
                              .replace(" | ", ", ") for k, v in t.items())
            print(f"| {name} {M}x{K} | {N} | {rule} | {cells} |", flush=True)
        del w4s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1,
                    help="seconds of replays per sample")
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--ab", action="store_true")
    args = ap.parse_args()
    lib = native.load(require=True)
    torch.manual_seed(0)
    (ab if args.ab else compare)(args, lib)


if __name__ == "__main__":
    main()
