#!/usr/bin/env python3
"""Routed fp8 MoE decode GEMVs (ops.decode_moe_swiglu_fp8 / decode_moe_fp8)
against the bf16 routed pair they replace (gemv_moe_swiglu / gemv_moe), on
the moe-8x7b expert shapes, for N routed pairs and three routing patterns:
every pair its own expert, two pairs per expert, all pairs one expert.

Each side is timed as a captured graph of LAUNCHES calls that walk round
COPIES full expert sets, so that no call finds its experts in a cache the
call before it filled (one expert's fp8 gate|up is 117 MB). The sides
alternate inside every round; reported are the median us per call, the
spread (max - min), and each side's own weight-byte floor at peak HBM
bandwidth: hit experts x fp8 bytes for the grouped kernel, pairs x bf16
bytes for the routed bf16 kernel.

    moefp8bench.py [--rounds R] [--pairs N ...]
    moefp8bench.py --engine moe-8x7b [batch ...]  # decode tok/s, fp8 / bf16

--engine hands over to genfp8bench.py (two DecodeSessions of one quantised
model alternating under the captured graph), with moe-8x7b as the default."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

PEAK_HBM = 8.0e12                     # B/s, MI355X HBM3E
H, FF, E, TOP_K = 4096, 14336, 8, 2   # moe-8x7b
LAUNCHES, COPIES = 16, 4
PATTERNS = {"distinct": lambda n: n, "two_per_expert": lambda n: n // 2,
            "one_expert": lambda n: 0}


def _graph(fn, sets):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s in sets:
            fn(s)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(LAUNCHES):
            fn(sets[i % len(sets)])
    return g


def _time(g, replays):
    """us per call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (replays * LAUNCHES) * 1e6


def _expert_set():
    """One layer's experts: bf16 gate, up, down pointer tables (the values
    the fp8 copies dequantise to) and the two Fp8ExpertTables."""
    from trainingjob_operator_amd.ops.fp8_weight import (expert_tables,
                                                         quantize_rows)
    keep, gu8s, d8s = [], [], []
    for _ in range(E):
        gu = (torch.randn(2 * FF, H, device="cuda") * H ** -0.5).bfloat16()
        dn = (torch.randn(H, FF, device="cuda") * FF ** -0.5).bfloat16()
        gu8, d8 = quantize_rows(gu, gate_up=True), quantize_rows(dn)
        gu.copy_(gu8.dequant())
        dn.copy_(d8.dequant())
        keep.append((gu, dn))
        gu8s.append(gu8)
        d8s.append(d8)

    def table(ptrs):
        return torch.tensor(ptrs, dtype=torch.int64, device="cuda")
    return {"keep": keep,
            "tg": table([gu.data_ptr() for gu, _ in keep]),
            "tu": table([gu[FF:].data_ptr() for gu, _ in keep]),
            "td": table([dn.data_ptr() for _, dn in keep]),
            "gu8": expert_tables(gu8s), "d8": expert_tables(d8s)}


def kernels(args):
    from trainingjob_operator_amd.ops import (decode_moe_fp8,
                                              decode_moe_swiglu_fp8, native)
    lib = native.load(require=True)
    torch.manual_seed(0)
    sets = [_expert_set() for _ in range(COPIES)]
    print("| op | N | routing | experts hit | fp8 us (spread) | fp8 floor us "
          "| of floor | bf16 us (spread) | bf16 floor us | of floor | "
          "bf16/fp8 |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for op in ("gate_up", "down"):
        for N in args.pairs:
            for pat, rule in PATTERNS.items():
                route = [rule(n) for n in range(N)]
                if max(route) >= E:
                    continue                    # more pairs than experts
                idx = torch.tensor(route, dtype=torch.int64, device="cuda")
                if op == "gate_up":
                    x = torch.randn(-(-N // TOP_K), H, device="cuda").bfloat16()
                    yb = torch.empty(N, FF, dtype=torch.bfloat16, device="cuda")

                    def fp8(s):
                        return decode_moe_swiglu_fp8(x, idx, s["gu8"], FF, H,
                                                     TOP_K)

                    def bf16(s):
                        rc = lib.gemv_moe_swiglu(
                            native.stream_ptr(), s["tg"].data_ptr(),
                            s["tu"].data_ptr(), idx.data_ptr(), x.data_ptr(),
                            yb.data_ptr(), FF, H, N, TOP_K)
                        native.check_rc(rc, "gemv_moe_swiglu")
                        return yb
                    w_elems = 2 * FF * H
                else:
                    x = torch.randn(N, FF, device="cuda").bfloat16()
                    yb = torch.empty(N, H, dtype=torch.bfloat16, device="cuda")

                    def fp8(s):
                        return decode_moe_fp8(x, idx, s["d8"], H, FF, 1)

                    def bf16(s):
                        rc = lib.gemv_moe(
                            native.stream_ptr(), s["td"].data_ptr(),
                            idx.data_ptr(), x.data_ptr(), yb.data_ptr(), H,
                            FF, N, 1)
                        native.check_rc(rc, "gemv_moe")
                        return yb
                    w_elems = H * FF
                a, b = fp8(sets[0]).float(), bf16(sets[0]).float()
                err = (a - b).abs().max().item()
                assert err <= 2e-2 * b.abs().max().item() + 2e-2, (op, N, err)
                g8, gb = _graph(fp8, sets), _graph(bf16, sets)
                r8 = max(2, int(args.window / (_time(g8, 2) * LAUNCHES * 1e-6)))
                rb = max(2, int(args.window / (_time(gb, 2) * LAUNCHES * 1e-6)))
                t8, tb = [], []
                for _ in range(args.rounds):
                    t8.append(_time(g8, r8))
                    tb.append(_time(gb, rb))
                m8, mb = statistics.median(t8), statistics.median(tb)
                hit = len(set(route))
                f8 = hit * w_elems / PEAK_HBM * 1e6
                fb = N * 2 * w_elems / PEAK_HBM * 1e6
                print(f"| {op} | {N} | {pat} | {hit} | {m8:.1f} "
                      f"({max(t8) - min(t8):.1f}) | {f8:.1f} | {f8 / m8:.0%} | "
                      f"{mb:.1f} ({max(tb) - min(tb):.1f}) | {fb:.1f} | "
                      f"{fb / mb:.0%} | {mb / m8:.2f}x |", flush=True)
                del g8, gb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", nargs="?", const="moe-8x7b", metavar="MODEL",
                    help="decode tok/s of MODEL instead: the arguments left "
                         "over (batch ..., --new, --rounds) go to genfp8bench")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1,
                    help="seconds of replays per sample")
    ap.add_argument("--pairs", type=int, nargs="+", default=[2, 8, 16])
    args, rest = ap.parse_known_args()
    if not torch.cuda.is_available():
        sys.exit("moefp8bench needs a GPU")
    if args.engine:
        import genfp8bench
        sys.argv = [sys.argv[0], args.engine] + rest + ["--rounds",
                                                        str(args.rounds)]
        return genfp8bench.main()
    if rest:
        ap.error(f"unrecognised arguments: {rest}")
    kernels(args)


if __name__ == "__main__":
    main()
