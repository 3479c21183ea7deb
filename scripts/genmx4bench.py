#!/usr/bin/env python3
"""Decode tokens/s under the captured graph with MXFP4, fp8 and bf16 decode
weights. A model carries one quantised format, so two models are built from
one seed: one quantised to MXFP4 (it also serves the bf16 side, from the
written-back values) and one to fp8. The three DecodeSessions alternate
inside every round. Also checks once that the MXFP4 graph emits the eager
MXFP4 tokens.

    genmx4bench.py [model] [batch ...] [--new N] [--rounds R]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", nargs="?", default="llama3-8b")
    ap.add_argument("batch", nargs="*", type=int, default=[1, 8])
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.decode_graph import DecodeSession
    from trainingjob_operator_amd.models.generate import (
        build_inference_model, generate, quantize_decode_weights)
    cfg = CONFIGS[args.model]
    dev = torch.device("cuda:0")
    models = {}
    for fmt in ("mxfp4", "fp8"):
        torch.manual_seed(0)
        models[fmt] = build_inference_model(cfg, dev)
        n = quantize_decode_weights(models[fmt], fmt)
        print(f"{args.model}: {n} weights quantised to {fmt}", flush=True)
    models["bf16"] = models["mxfp4"]
    for batch in args.batch:
        g = torch.Generator().manual_seed(batch)
        prompt = torch.randint(0, cfg.vocab_size, (batch, args.prompt),
                               generator=g).to(dev)
        max_len = args.prompt + args.new + 8
        ses = {w: DecodeSession(m, batch, max_len, weights=w)
               for w, m in models.items()}
        outs = {w: s.generate(prompt, 8) for w, s in ses.items()}  # capture
        eager = generate(models["mxfp4"], prompt, max_new_tokens=8,
                         weights="mxfp4")
        agree = (outs["mxfp4"] == eager).float().mean().item()
        print(f"b{batch}: mxfp4 graph against mxfp4 eager tokens: "
              f"{agree:.0%} equal", flush=True)
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
        print(f"b{batch} mxfp4 / fp8: {med['mxfp4'] / med['fp8']:.2f}x, "
              f"mxfp4 / bf16: {med['mxfp4'] / med['bf16']:.2f}x", flush=True)
        del ses


if __name__ == "__main__":
    main()
