#!/usr/bin/env python3
"""Routed MXFP4 MoE decode GEMVs (ops.decode_moe_swiglu_mx4 / decode_moe_mx4)
on the moe-8x7b expert shapes, for N routed pairs and three routing patterns
(every pair its own expert, two pairs per expert, all pairs one expert: 1, 2,
4 and 8 hit experts), against

    mx4x2  the same kernel with the loads of two chunks in flight
           (gemv_moe_mx4_ab; bit-equal, asserted),
    fp8    gemv_moe_fp8 on an fp8 copy of the same experts,
    bf16   the bf16 routed pair (gemv_moe_swiglu / gemv_moe) these calls ran
           on before, over the values the MXFP4 copies dequantise to.

Each side is timed as a captured graph of LAUNCHES calls that walk round
COPIES full expert sets, so that no call finds its experts in a cache the
call before it filled. The sides alternate inside every round; reported are
the median us per call, the spread (max - min), and the share of each side's
own weight-byte floor at peak HBM bandwidth: hit experts x 4.25-bit bytes for
MXFP4, hit experts x fp8 bytes, pairs x bf16 bytes.

    moemx4bench.py [--rounds R] [--pairs N ...]
    moemx4bench.py --engine [MODEL] [batch ...] [--new N]

--engine: decode tok/s of MODEL (moe-8x7b) under the captured graph with
weights="mxfp4" (MXFP4 experts), with the same model's experts on the bf16
routed pair (what weights="mxfp4" ran before the experts were quantised: the
session is captured with the experts' MXFP4 copies hidden), and with
weights="fp8" on a second model from the same seed."""
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
BYTES = {"mx4": 4.25 / 8, "mx4x2": 4.25 / 8, "fp8": 1.0, "bf16": 2.0}


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
    the MXFP4 copies dequantise to), the two Mx4ExpertTables and the two
    Fp8ExpertTables of an fp8 copy."""
    from trainingjob_operator_amd.ops.fp8_weight import (expert_tables,
                                                         quantize_rows)
    from trainingjob_operator_amd.ops.mx4_weight import (mx4_expert_tables,
                                                         quantize_mx4)
    keep, gu4s, d4s, gu8s, d8s = [], [], [], [], []
    for _ in range(E):
        gu = (torch.randn(2 * FF, H, device="cuda") * H ** -0.5).bfloat16()
        dn = (torch.randn(H, FF, device="cuda") * FF ** -0.5).bfloat16()
        gu4, d4 = quantize_mx4(gu, gate_up=True), quantize_mx4(dn)
        gu.copy_(gu4.dequant())
        dn.copy_(d4.dequant())
        keep.append((gu, dn))
        gu4s.append(gu4)
        d4s.append(d4)
        gu8s.append(quantize_rows(gu, gate_up=True))
        d8s.append(quantize_rows(dn))

    def table(ptrs):
        return torch.tensor(ptrs, dtype=torch.int64, device="cuda")
    return {"keep": keep,
            "tg": table([gu.data_ptr() for gu, _ in keep]),
            "tu": table([gu[FF:].data_ptr() for gu, _ in keep]),
            "td": table([dn.data_ptr() for _, dn in keep]),
            "gu4": mx4_expert_tables(gu4s), "d4": mx4_expert_tables(d4s),
            "gu8": expert_tables(gu8s), "d8": expert_tables(d8s)}


def kernels(args):
    from trainingjob_operator_amd.ops import (
        decode_moe_fp8, decode_moe_mx4, decode_moe_swiglu_fp8,
        decode_moe_swiglu_mx4, native)
    lib = native.load(require=True)
    torch.manual_seed(0)
    sets = [_expert_set() for _ in range(COPIES)]
    names = list(BYTES)
    print("| op | N | routing | experts hit | "
          + " | ".join(f"{s} us (spread) | of floor" for s in names)
          + " | mx4x2/mx4 | bf16/mx4 | fp8/mx4 |")
    print("|---" * (7 + 2 * len(names)) + "|")
    for op in ("gate_up", "down"):
        swiglu = op == "gate_up"
        M, K, xdiv = (FF, H, TOP_K) if swiglu else (H, FF, 1)
        for N in args.pairs:
            for pat, rule in PATTERNS.items():
                route = [rule(n) for n in range(N)]
                if max(route) >= E:
                    continue                    # more pairs than experts
                idx = torch.tensor(route, dtype=torch.int64, device="cuda")
                x = torch.randn(-(-N // xdiv), K, device="cuda").bfloat16()
                yb = torch.empty(N, M, dtype=torch.bfloat16, device="cuda")
                y2 = torch.empty_like(yb)
                t4, t8 = ("gu4", "gu8") if swiglu else ("d4", "d8")

                def mx4(s):
                    f = decode_moe_swiglu_mx4 if swiglu else decode_moe_mx4
                    return f(x, idx, s[t4], M, K, xdiv)

                def mx4x2(s):
                    rc = lib.gemv_moe_mx4_ab(
                        native.stream_ptr(), int(swiglu), 1,
                        s[t4].w.data_ptr(), s[t4].s.data_ptr(),
                        idx.data_ptr(), x.data_ptr(), y2.data_ptr(), M, K, N,
                        E, xdiv)
                    native.check_rc(rc, "gemv_moe_mx4_ab")
                    return y2

                def fp8(s):
                    f = decode_moe_swiglu_fp8 if swiglu else decode_moe_fp8
                    return f(x, idx, s[t8], M, K, xdiv)

                def bf16(s):
                    if swiglu:
                        rc = lib.gemv_moe_swiglu(
                            native.stream_ptr(), s["tg"].data_ptr(),
                            s["tu"].data_ptr(), idx.data_ptr(), x.data_ptr(),
                            yb.data_ptr(), M, K, N, xdiv)
                    else:
                        rc = lib.gemv_moe(
                            native.stream_ptr(), s["td"].data_ptr(),
                            idx.data_ptr(), x.data_ptr(), yb.data_ptr(), M, K,
                            N, xdiv)
                    native.check_rc(rc, "gemv_moe")
                    return yb

                fns = {"mx4": mx4, "mx4x2": mx4x2, "fp8": fp8, "bf16": bf16}
                a, b = mx4(sets[0]), bf16(sets[0]).float()
                assert torch.equal(a, mx4x2(sets[0])), (op, N, pat)
                err = (a.float() - b).abs().max().item()
                assert err <= 2e-2 * b.abs().max().item() + 2e-2, (op, N, err)
                graphs = {s: _graph(f, sets) for s, f in fns.items()}
                reps = {s: max(2, int(args.window /
                                      (_time(g, 2) * LAUNCHES * 1e-6)))
                        for s, g in graphs.items()}
                t = {s: [] for s in names}
                for _ in range(args.rounds):
                    for s in names:
                        t[s].append(_time(graphs[s], reps[s]))
                med = {s: statistics.median(v) for s, v in t.items()}
                hit = len(set(route))
                row = f"| {op} | {N} | {pat} | {hit} |"
                for s in names:
                    floor = ((N if s == "bf16" else hit) * (2 if swiglu else 1)
                             * M * K * BYTES[s] / PEAK_HBM * 1e6)
                    row += (f" {med[s]:.1f} ({max(t[s]) - min(t[s]):.1f}) |"
                            f" {floor / med[s]:.0%} |")
                print(row + f" {med['mx4x2'] / med['mx4']:.2f}x |"
                      f" {med['bf16'] / med['mx4']:.2f}x |"
                      f" {med['fp8'] / med['mx4']:.2f}x |", flush=True)
                del graphs


def engine(args, name, batches):
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.decode_graph import DecodeSession
    from trainingjob_operator_amd.models.generate import (
        build_inference_model, quantize_decode_weights)
    from trainingjob_operator_amd.parallel import ep
    cfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    models = {}
    for fmt in ("mxfp4", "fp8"):
        torch.manual_seed(0)
        models[fmt] = build_inference_model(cfg, dev)
        n = quantize_decode_weights(models[fmt], fmt)
        print(f"{name}: {n} weights quantised to {fmt}", flush=True)
    for batch in batches:
        g = torch.Generator().manual_seed(batch)
        prompt = torch.randint(0, cfg.vocab_size, (batch, args.prompt),
                               generator=g).to(dev)
        max_len = args.prompt + args.new + 8
        ses, outs = {}, {}
        # the hidden capture first: it drops the layer's cached tables, which
        # a graph captured before it would still point into
        for side, fmt in (("mxfp4, bf16 experts", "mxfp4"),
                          ("mxfp4", "mxfp4"), ("fp8", "fp8")):
            hide = side != fmt
            has = ep.expert_mx4
            if hide:                    # capture on the bf16 routed pair
                ep.expert_mx4 = lambda ex: None
            try:
                ses[side] = DecodeSession(models[fmt], batch, max_len,
                                          weights=fmt)
                outs[side] = ses[side].generate(prompt, 8)
            finally:
                ep.expert_mx4 = has
        agree = (outs["mxfp4"] == outs["mxfp4, bf16 experts"]).float().mean()
        print(f"b{batch}: tokens of the two expert routes {agree:.0%} equal",
              flush=True)
        tps = {w: [] for w in ses}
        for _ in range(args.rounds):
            for w, s in ses.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.generate(prompt, args.new)
                torch.cuda.synchronize()
                tps[w].append(batch * args.new / (time.perf_counter() - t0))
        med = {w: statistics.median(v) for w, v in tps.items()}
        for w, v in tps.items():
            print(f"b{batch} {w}: {med[w]:.1f} tok/s incl. prefill (spread "
                  f"{max(v) - min(v):.1f}, {batch * 1e3 / med[w]:.2f} "
                  f"ms/token)")
        print(f"b{batch} mxfp4 / bf16 experts: "
              f"{med['mxfp4'] / med['mxfp4, bf16 experts']:.2f}x, mxfp4 / "
              f"fp8: {med['mxfp4'] / med['fp8']:.2f}x", flush=True)
        del ses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", nargs="*", metavar="MODEL [batch ...]",
                    help="decode tok/s of MODEL (moe-8x7b) at the batches "
                         "(1 8) instead of the kernel table")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1,
                    help="seconds of replays per sample")
    ap.add_argument("--pairs", type=int, nargs="+", default=[2, 8, 16])
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moemx4bench needs a GPU")
    if args.engine is not None:
        name = args.engine[0] if args.engine else "moe-8x7b"
        return engine(args, name, [int(b) for b in args.engine[1:]] or [1, 8])
    kernels(args)


if __name__ == "__main__":
    main()
