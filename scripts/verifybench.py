#!/usr/bin/env python3
"""Paged speculative verify microbench: attn_verify_paged against the two
older routes to the same result, and the engine with and without prompt
lookup.

  python scripts/verifybench.py kernels
  python scripts/verifybench.py engine [model]

kernels: B slots whose T query tokens end at row fill - 1. The new kernel
against prefill_attention_paged with one work row per slot (every T) and
against decode_attention_paged (T = 1). engine: the 8 ragged requests of
scripts/pagedbench.py with lookup_k 0 and 4 on random-init weights; the
prompts are made repetitive (a random head and the model's own continuation
of it, repeated to the prompt's length) so that drafts can hit, and the
acceptance rate is printed next to tok/s, which means nothing without it.

Both sides of every comparison run in this process, alternating round by
round; a round is N back-to-back calls between two device events. Printed
per side: median over the rounds and the min..max spread. The times are
CALL times (launches and the workspace allocation included).
"""
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from pagedbench import DEV, ab_rounds, paged_case, report


def kernels():
    from trainingjob_operator_amd.ops import (
        decode_attention_paged, native, prefill_attention_paged,
        prefill_work, verify_attention_paged,
    )
    native.load(require=True)
    H, n_kv, D = 32, 8, 128
    scale = 1.0 / math.sqrt(D)
    for B, rows, fill, T in ((8, 2048, 2048, 1), (8, 2048, 2048, 4),
                             (8, 2048, 2048, 8), (8, 8192, 512, 8),
                             (1, 2048, 2048, 8)):
        kp, vp, table, pos, kc, vc = paged_case(B, n_kv, D, rows // 64,
                                                fill, seed=rows + T)
        del kc, vc
        torch.manual_seed(T)
        q = (torch.randn(B, T, H, D, device=DEV) * .5).bfloat16()
        pos0 = pos - (T - 1)                      # the first token's row
        n_q = torch.full((B,), T, dtype=torch.int32, device=DEV)
        work, _, _ = prefill_work([(b, fill - T, T) for b in range(B)], DEV)
        qp = q.reshape(B * T, H, D)
        sides = {
            "attn_verify_paged": lambda: verify_attention_paged(
                q, kp, vp, table, pos0, n_q, scale),
            "attn_prefill_paged": lambda: prefill_attention_paged(
                qp, kp, vp, table, work, scale),
        }
        a = sides["attn_verify_paged"]().float()
        err = (a - sides["attn_prefill_paged"]().float().reshape(a.shape)
               ).abs().max().item()
        note = f"max |verify - prefill| {err:.2e}"
        if T == 1:
            qd = q.reshape(B, H, 1, D)
            sides["attn_decode_paged"] = lambda: decode_attention_paged(
                qd, kp, vp, table, pos, scale)
            err = (a.reshape(B, H, 1, D)
                   - sides["attn_decode_paged"]().float()).abs().max().item()
            note += f", max |verify - decode| {err:.2e}"
        report(f"B={B} H={H} n_kv={n_kv} T={T} fill {fill} in a {rows}-row "
               f"table ({note})", ab_rounds(sides))
        del kp, vp


def engine(model_name):
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.generate import build_inference_model
    from trainingjob_operator_amd.models.paged import (
        PagedEngine, generate_ragged,
    )
    cfg = CONFIGS[model_name]
    m = build_inference_model(cfg, torch.device(DEV))
    lengths = [37, 128, 300, 512, 64, 700, 200, 450]
    new = 64
    g = torch.Generator().manual_seed(1)
    heads = [torch.randint(0, cfg.vocab_size, (n // 3,),
                           generator=g).to(DEV) for n in lengths]
    conts = generate_ragged(m, heads, new, max_slots=8)
    prompts = [c[:n // 3 + min(new, n // 3)].repeat(3)[:n]
               for c, n in zip(conts, lengths)]
    assert [p.numel() for p in prompts] == lengths

    def run(k):
        eng = PagedEngine(m, max_slots=8, n_pages=8 * 12, lookup_k=k)
        ids = [eng.submit(p, new) for p in prompts]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = eng.run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return [done[i] for i in ids], len(prompts) * new / dt, eng

    a, _, _ = run(0)                               # warmup + agreement
    b, _, _ = run(4)
    agree = sum(int((x == y).sum()) for x, y in zip(a, b)) \
        / sum(x.numel() for x in a)
    print(f"{model_name}: 8 ragged repetitive requests (prompts {lengths}, "
          f"{new} new each), token agreement lookup_k 4 vs 0 {agree:.3f}")
    res = {0: [], 4: []}
    for _ in range(3):
        for k in (0, 4):
            _, tps, eng = run(k)
            res[k].append(tps)
            stats = (eng.steps, eng.drafted, eng.accepted)
        print(f"  lookup_k 4: {stats[0]} verify steps, {stats[2]} of "
              f"{stats[1]} draft tokens accepted")
    for k, xs in res.items():
        print(f"  lookup_k {k}   median {statistics.median(xs):8.1f} tok/s   "
              f"spread {min(xs):.1f}..{max(xs):.1f}  ({len(xs)} rounds, "
              "prefill included)")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "verifybench needs a GPU"
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "kernels":
        kernels()
    elif mode == "engine":
        engine(sys.argv[2] if len(sys.argv) > 2 else "llama3-8b")
    else:
        sys.exit(f"unknown mode {mode!r}")
