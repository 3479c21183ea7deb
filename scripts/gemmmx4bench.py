#!/usr/bin/env python3
"""MXFP4 skinny GEMM (17..64 rows, x staged in LDS and shared between T row
tiles) on the llama3-8b projection shapes against every route the same rows
have without it, and a paged verify step.

  python scripts/gemmmx4bench.py kernels [--rows 17 32 40 64] [--rounds 5]
  python scripts/gemmmx4bench.py verify [model]

kernels: per shape and N, alternating in one process,
  rows     linear_mx4_rows / swiglu_mx4_rows ((T, S) by the rule)
  tTsS     the same kernel with T row tiles per workgroup and S k slices
           forced; t1 stages x for one tile: nothing is shared
  bf16     what _proj took: decode_linear over the written-back bf16 weight,
           which is F.linear above 8 rows (+ swiglu_packed for gate|up)
  gemv     decode_linear_mx4 / decode_swiglu_mx4 ceil(N / 16) times
  fp8      linear_fp8_rows / swiglu_fp8_rows on an fp8 copy of the weight
timed as in scripts/gemmfp8bench.py: a captured graph of 64 launches walking
round 512 MB of weight copies, replayed for about 0.1 s per sample; median us
per call (spread = max - min) over the rounds, and each side's share of its
own weight-byte floor at peak HBM bandwidth (4.25, 8 or 16 bits per weight).
"takes" is the dispatch rule's answer (gemm_mx4_rows_pays) for the call; the
1024x512 row is the small-weight end of that rule.

verify: _verify_paged, 8 slots x (lookup_k 4 + 1) = 40 rows at 512 cached
rows per slot, weights mxfp4 against bf16 on one quantised model,
alternating; host clock around 10 synchronised steps, median of the rounds."""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from gemvfp8bench import LAUNCHES, PEAK_HBM, SHAPES, _graph, _time
from trainingjob_operator_amd.ops import (decode_linear, decode_linear_mx4,
                                          decode_swiglu_mx4, linear_fp8_rows,
                                          linear_mx4_rows, native,
                                          swiglu_fp8_rows, swiglu_mx4_rows,
                                          swiglu_packed)
from trainingjob_operator_amd.ops.fp8_weight import quantize_rows
from trainingjob_operator_amd.ops.mx4_weight import quantize_mx4

TS = [(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4), (4, 1), (4, 2)]
BITS = {"bf16": 16.0, "fp8": 8.0}          # every other side: 4.25


def _forced(lib, x, w4, t, s):
    N, cols = x.shape[0], w4.M // 2 if w4.gate_up else w4.M
    y = torch.empty(N, cols, dtype=torch.bfloat16, device=x.device)

    def run(w):
        rc = lib.gemm_mx4_rows_ab(
            native.stream_ptr(), int(w.gate_up), t, s,
            *(ctypes.c_void_p(p.data_ptr()) for p in (w.packed, w.scale, x,
                                                      y)), cols, w.K, N)
        assert rc == 0
        return y
    return run


def kernels(args):
    lib = native.load(require=True)
    torch.manual_seed(0)
    names = ["rows"] + [f"t{t}s{s}" for t, s in TS] + ["bf16", "gemv", "fp8"]
    print("| shape | N | rule T,S | takes | " + " | ".join(
        f"{n} us (spread)" for n in names) + " | of floor: rows / bf16 / "
        "gemv / fp8 | bf16/rows |")
    print("|---|---|---|---|" + "---|" * (len(names) + 2))
    for name, M, K, gate_up in SHAPES + [("small", 1024, 512, False)]:
        if args.shapes and name not in args.shapes:
            continue
        n_copies = min(LAUNCHES, -(-(512 << 20) // (M * K)))
        ws, w4s, w8s = [], [], []
        for _ in range(n_copies):
            w = (torch.randn(M, K, device="cuda") * K ** -0.5).bfloat16()
            w4 = quantize_mx4(w, gate_up=gate_up)
            w.copy_(w4.dequant())
            ws.append(w)
            w4s.append(w4)
            w8s.append(quantize_rows(w, gate_up=gate_up))
        tiles = (M // 2 if gate_up else M) // 16
        rule = lib.gemm_mx4_rows_shape(tiles, K, int(gate_up))
        for N in args.rows:
            x = torch.randn(N, K, device="cuda").bfloat16()
            one = decode_swiglu_mx4 if gate_up else decode_linear_mx4
            rows = swiglu_mx4_rows if gate_up else linear_mx4_rows
            rows8 = swiglu_fp8_rows if gate_up else linear_fp8_rows

            def bf16(w):
                y = decode_linear(x, w)
                return swiglu_packed(y) if gate_up else y

            def gemv(w4):
                return [one(x[i:i + 16], w4) for i in range(0, N, 16)]
            sides = {"rows": (lambda w4: rows(x, w4), w4s),
                     "bf16": (bf16, ws), "gemv": (gemv, w4s),
                     "fp8": (lambda w8: rows8(x, w8), w8s)}
            for t, s in TS:
                sides[f"t{t}s{s}"] = (_forced(lib, x, w4s[0], t, s), w4s)
            want = torch.cat(gemv(w4s[0])).float()
            bound = 2e-2 * want.abs().max().item() + 2e-2
            for k, (f, c) in sides.items():       # one model on every side
                if k not in ("gemv", "fp8"):
                    err = (f(c[0]).float() - want).abs().max().item()
                    assert err <= bound, (name, N, k, err)
            graphs = {k: _graph(f, c) for k, (f, c) in sides.items()}
            reps = {k: max(2, int(args.window / (_time(g, 2) * LAUNCHES
                                                 * 1e-6)))
                    for k, g in graphs.items()}
            ts = {k: [] for k in graphs}
            for _ in range(args.rounds):
                for k, g in graphs.items():
                    ts[k].append(_time(g, reps[k]))
            med = {k: statistics.median(v) for k, v in ts.items()}
            cells = [f"{med[k]:.1f} ({max(ts[k]) - min(ts[k]):.1f})"
                     for k in names]
            floor = " / ".join(
                f"{M * K * BITS.get(k, 4.25) / 8 / PEAK_HBM / (med[k] * 1e-6):.0%}"
                for k in ("rows", "bf16", "gemv", "fp8"))
            takes = "yes" if lib.gemm_mx4_rows_pays(
                tiles, K, N, int(gate_up)) else "no"
            print(f"| {name} {M}x{K} | {N} | {rule >> 8},{rule & 255} | "
                  f"{takes} | " + " | ".join(cells) + f" | {floor} | "
                  f"{med['bf16'] / med['rows']:.2f}x |", flush=True)
            del graphs
        del ws, w4s, w8s


@torch.no_grad()
def verify(args):
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.generate import (
        build_inference_model, quantize_decode_weights)
    from trainingjob_operator_amd.models.paged import (PagedKVCache,
                                                       _verify_paged)
    native.load(require=True)
    cfg = CONFIGS[args.model]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_inference_model(cfg, dev)
    quantize_decode_weights(model, "mxfp4")
    B, T, fill = 8, 5, 512
    cache = PagedKVCache(cfg, n_pages=B * 9, max_slots=B,
                         max_pages_per_seq=9, device=dev,
                         dtype=torch.bfloat16)
    for b in range(B):
        assert cache.admit(b, fill + T)
        cache.ensure_row(b, fill + T - 1)
    cache.sync_pos([fill] * B)
    tokens = torch.randint(0, cfg.vocab_size, (B, T), device=dev)
    n_q = torch.full((B,), T, dtype=torch.int32, device=dev)

    def step(mx4):
        return _verify_paged(model, tokens, cache, n_q, mx4)

    a, b = step(True).float(), step(False).float()
    err = (a - b).abs().max().item()
    ts = {True: [], False: []}
    for _ in range(args.rounds):
        for mx4 in (True, False):
            step(mx4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                step(mx4)
            torch.cuda.synchronize()
            ts[mx4].append((time.perf_counter() - t0) / 10 * 1e3)
    m4, mb = statistics.median(ts[True]), statistics.median(ts[False])
    print(f"{args.model} verify step, {B} slots x {T} tokens = {B * T} rows, "
          f"{fill} cached rows per slot; max |mxfp4 - bf16| logits {err:.3e} "
          f"(max |bf16| {b.abs().max().item():.3e})")
    print(f"  weights mxfp4 {m4:.3f} ms (spread "
          f"{max(ts[True]) - min(ts[True]):.3f})")
    print(f"  weights bf16  {mb:.3f} ms (spread "
          f"{max(ts[False]) - min(ts[False]):.3f})   bf16/mxfp4 "
          f"{mb / m4:.2f}x")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "gemmmx4bench needs a GPU"
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "verify"])
    ap.add_argument("model", nargs="?", default="llama3-8b")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1,
                    help="seconds of replays per sample")
    ap.add_argument("--rows", type=int, nargs="+", default=[17, 32, 40, 64])
    ap.add_argument("--shapes", nargs="*", default=[],
                    help="shape names to run (default: all)")
    args = ap.parse_args()
    kernels(args) if args.mode == "kernels" else verify(args)
