#!/usr/bin/env python3
"""fp8 skinny GEMM (17..64 rows) on the llama3-8b projection shapes against
the two routes the same rows had without it, and a paged verify step.

  python scripts/gemmfp8bench.py kernels [--rows 17 32 40 64] [--rounds 5]
  python scripts/gemmfp8bench.py verify [model]

kernels: per shape and N, alternating in one process,
  rows     linear_fp8_rows / swiglu_fp8_rows (row tiles per wave by the rule)
  r1/2/4   the same kernel with 1, 2, 4 row tiles per wave forced (r1 is the
           one-tile grid: every tile's workgroup re-reads x from L2)
  bf16     what _proj took: decode_linear over the bf16 weight, which is
           F.linear above 8 rows (+ swiglu_packed for gate|up)
  gemv     decode_linear_fp8 / decode_swiglu_fp8 ceil(N / 16) times
timed as in scripts/gemvfp8bench.py: a captured graph of 64 launches walking
round 512 MB (fp8) / 1 GB (bf16) of weight copies, replayed for about 0.1 s
per sample; median us per call (spread = max - min) over the rounds, and the
share of the fp8 weight-byte floor at peak HBM bandwidth. "takes" is the
dispatch rule's answer (gemm_fp8_rows_pays) for the call; the 1024x512 row
is the small-weight end of that rule.

verify: _verify_paged, 8 slots x (lookup_k 4 + 1) = 40 rows at 512 cached
rows per slot, weights fp8 against bf16 on one quantised model, alternating;
host clock around 10 synchronised steps, median of the rounds."""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from gemvfp8bench import LAUNCHES, PEAK_HBM, SHAPES, _graph, _time
from trainingjob_operator_amd.ops import (decode_linear, decode_linear_fp8,
                                          decode_swiglu_fp8, linear_fp8_rows,
                                          native, swiglu_fp8_rows,
                                          swiglu_packed)
from trainingjob_operator_amd.ops.fp8_weight import quantize_rows


def _forced(lib, x, w8, r):
    """The kernel with r row tiles per wave, or None where r does not go."""
    N, cols = x.shape[0], w8.M // 2 if w8.gate_up else w8.M
    if (cols // 16) % r or (w8.gate_up and r == 4):
        return None
    y = torch.empty(N, cols, dtype=torch.bfloat16, device=x.device)

    def run(w):
        rc = lib.gemm_fp8_rows_ab(
            native.stream_ptr(), int(w.gate_up), r,
            *(ctypes.c_void_p(t.data_ptr()) for t in (w.packed, w.scale, x,
                                                      y)), cols, w.K, N)
        assert rc == 0
        return y
    return run


def kernels(args):
    lib = native.load(require=True)
    torch.manual_seed(0)
    names = ["rows", "r1", "r2", "r4", "bf16", "gemv"]
    print("| shape | N | split | rule r | takes | " + " | ".join(
        f"{n} us (spread)" for n in names) + " | rows of floor | bf16/rows | "
        "gemv/rows |")
    print("|---|---|---|---|---|" + "---|" * (len(names) + 3))
    for name, M, K, gate_up in SHAPES + [("small", 1024, 512, False)]:
        n_copies = min(LAUNCHES, -(-(512 << 20) // (M * K)))
        ws, w8s = [], []
        for _ in range(n_copies):
            w = (torch.randn(M, K, device="cuda") * K ** -0.5).bfloat16()
            w8 = quantize_rows(w, gate_up=gate_up)
            w.copy_(w8.dequant())
            ws.append(w)
            w8s.append(w8)
        tiles = (M // 2 if gate_up else M) // 16
        split = lib.gemv_fp8_split(tiles, K)
        rule = lib.gemm_fp8_rows_r(tiles, K, int(gate_up))
        for N in args.rows:
            x = torch.randn(N, K, device="cuda").bfloat16()
            one = decode_swiglu_fp8 if gate_up else decode_linear_fp8
            rows = swiglu_fp8_rows if gate_up else linear_fp8_rows

            def bf16(w):
                y = decode_linear(x, w)
                return swiglu_packed(y) if gate_up else y

            def gemv(w8):
                return [one(x[i:i + 16], w8) for i in range(0, N, 16)]
            sides = {"rows": (lambda w8: rows(x, w8), w8s),
                     "bf16": (bf16, ws), "gemv": (gemv, w8s)}
            for r in (1, 2, 4):
                f = _forced(lib, x, w8s[0], r)
                if f is not None:
                    sides[f"r{r}"] = (f, w8s)
            want = torch.cat(gemv(w8s[0]))
            for k, (f, c) in sides.items():       # same bits, or bf16-close
                got = f(c[0])
                if k == "bf16":
                    err = (got.float() - want.float()).abs().max().item()
                    assert err <= 2e-2 * want.float().abs().max().item() \
                        + 2e-2, (name, N, err)
                elif k != "gemv":
                    assert torch.equal(got, want), (name, N, k)
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
                     if k in med else "-" for k in names]
            floor = M * K / PEAK_HBM / (med["rows"] * 1e-6)
            takes = "yes" if lib.gemm_fp8_rows_pays(
                tiles, K, N, int(gate_up)) else "no"
            print(f"| {name} {M}x{K} | {N} | {split} | {rule} | {takes} | "
                  + " | ".join(cells) + f" | {floor:.0%} | "
                  f"{med['bf16'] / med['rows']:.2f}x | "
                  f"{med['gemv'] / med['rows']:.2f}x |", flush=True)
            del graphs
        del ws, w8s


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
    quantize_decode_weights(model)
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

    def step(fp8):
        return _verify_paged(model, tokens, cache, n_q, fp8)

    a, b = step(True).float(), step(False).float()
    err = (a - b).abs().max().item()
    ts = {True: [], False: []}
    for _ in range(args.rounds):
        for fp8 in (True, False):
            step(fp8)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                step(fp8)
            torch.cuda.synchronize()
            ts[fp8].append((time.perf_counter() - t0) / 10 * 1e3)
    m8, mb = statistics.median(ts[True]), statistics.median(ts[False])
    print(f"{args.model} verify step, {B} slots x {T} tokens = {B * T} rows, "
          f"{fill} cached rows per slot; max |fp8 - bf16| logits {err:.3e} "
          f"(max |bf16| {b.abs().max().item():.3e})")
    print(f"  weights fp8  {m8:.3f} ms (spread "
          f"{max(ts[True]) - min(ts[True]):.3f})")
    print(f"  weights bf16 {mb:.3f} ms (spread "
          f"{max(ts[False]) - min(ts[False]):.3f})   bf16/fp8 {mb / m8:.2f}x")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "gemmfp8bench needs a GPU"
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "verify"])
    ap.add_argument("model", nargs="?", default="llama3-8b")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1,
                    help="seconds of replays per sample")
    ap.add_argument("--rows", type=int, nargs="+", default=[17, 32, 40, 64])
    args = ap.parse_args()
    kernels(args) if args.mode == "kernels" else verify(args)
