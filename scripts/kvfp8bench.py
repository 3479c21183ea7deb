#!/usr/bin/env python3
"""fp8 KV cache microbench: the fp8 decode route against the two bf16 routes
to the same attention, the fp8 cache write against the bf16 one, and the
engine with kv="fp8" against kv="bf16".

  python scripts/kvfp8bench.py kernels
  python scripts/kvfp8bench.py engine [model] [--prompt N] [--new N]

kernels: B slots at row fill - 1 of a rows-long table, H=32, n_kv=8.
attn_decode_paged_fp8 reads the quantised copy of the very pools that
attn_decode_paged and attn_verify_paged (T = 1) read in bf16. engine: 8
requests with prompts of about `--prompt` tokens on random-init weights,
graph=True and weights="fp8" on both sides; token agreement between the two
caches is printed, not judged (random-init logits sit within rounding of each
other).

Both sides of every comparison run in this process, alternating round by
round; a round is N back-to-back calls between two device events. Printed
per side: median over the rounds and the min..max spread. Kernel times are
CALL times (launches and the workspace allocation included).
"""
import argparse
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
        decode_attention_paged, decode_attention_paged_fp8, make_inv_freq,
        native, reference, rope_cache_paged, rope_cache_paged_fp8,
        verify_attention_paged,
    )
    native.load(require=True)
    H, n_kv, D = 32, 8, 128
    scale = 1.0 / math.sqrt(D)
    for B, rows, fill in ((8, 2048, 2048), (1, 2048, 2048), (8, 8192, 512),
                          (1, 8192, 512)):
        kp, vp, table, pos, kc, vc = paged_case(B, n_kv, D, rows // 64, fill,
                                                seed=rows + B)
        del kc, vc
        pools = tuple(t.contiguous()
                      for t in reference.kv_fp8_quant_pages(kp, vp))
        torch.manual_seed(B)
        q = (torch.randn(B, H, 1, D, device=DEV) * .5).bfloat16()
        qv = q.reshape(B, 1, H, D)
        n_q = torch.ones(B, dtype=torch.int32, device=DEV)
        sides = {
            "attn_decode_paged_fp8": lambda: decode_attention_paged_fp8(
                q, *pools, table, pos, scale),
            "attn_decode_paged": lambda: decode_attention_paged(
                q, kp, vp, table, pos, scale),
            "attn_verify_paged": lambda: verify_attention_paged(
                qv, kp, vp, table, pos, n_q, scale),
        }
        a = sides["attn_decode_paged_fp8"]().float()
        tw = reference.decode_attention_paged_fp8(q, *pools, table, pos,
                                                  scale).float()
        b = sides["attn_decode_paged"]().float()
        live = fill * n_kv * B * 2 * D
        report(f"B={B} H={H} n_kv={n_kv} fill {fill} in a {rows}-row table "
               f"(max |fp8 - twin| {(a - tw).abs().max().item():.2e}, "
               f"|fp8 - bf16 route| {(a - b).abs().max().item():.2e}; live "
               f"KV bytes fp8 {live * 132 // 128 / 1e6:.1f} MB, bf16 "
               f"{live * 2 / 1e6:.1f} MB)", ab_rounds(sides))
        del kp, vp, pools

    B, nh = 8, H
    kp, vp, table, pos, kc, vc = paged_case(B, n_kv, D, 32, 1000, seed=5)
    del kc, vc
    pools = tuple(t.contiguous() for t in reference.kv_fp8_quant_pages(kp, vp))
    inv_freq = make_inv_freq(D, 500000.0, device=DEV)
    qkv = (torch.randn(B, (nh + 2 * n_kv) * D, device=DEV) * .5).bfloat16()
    a = rope_cache_paged(qkv, kp, vp, inv_freq, table, pos, nh, n_kv)
    b = rope_cache_paged_fp8(qkv, *pools, inv_freq, table, pos, nh, n_kv)
    assert torch.equal(a, b), "fp8 write: q differs from rope_cache_paged"
    report(f"rope + cache write B={B} nh={nh} nkv={n_kv} D={D}", ab_rounds({
        "rope_cache_paged_fp8": lambda: rope_cache_paged_fp8(
            qkv, *pools, inv_freq, table, pos, nh, n_kv),
        "rope_cache_paged": lambda: rope_cache_paged(
            qkv, kp, vp, inv_freq, table, pos, nh, n_kv),
    }))


def engine(model_name, prompt_len, new, rounds):
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.generate import build_inference_model
    from trainingjob_operator_amd.models.paged import PagedEngine, pages_for
    cfg = CONFIGS[model_name]
    m = build_inference_model(cfg, torch.device(DEV))
    g = torch.Generator().manual_seed(1)
    lengths = [prompt_len - 37 * i for i in range(8)]
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).to(DEV)
               for n in lengths]
    per_seq = pages_for(prompt_len + new)
    engines = {kv: PagedEngine(m, max_slots=8, n_pages=8 * per_seq,
                               max_pages_per_seq=per_seq, graph=True,
                               weights="fp8", kv=kv)
               for kv in ("fp8", "bf16")}
    for kv, eng in engines.items():
        c = eng.cache
        byts = sum(t.numel() * t.element_size() for t in (c.k[0], c.v[0]))
        if kv == "fp8":
            byts += c.kv_scale[0].numel() * 4
        print(f"kv {kv}: {c.n_pages} pages, {byts / 2**20:.1f} MiB of pools "
              f"per layer ({byts // c.n_pages} bytes per page)")

    def run(kv):
        """Prefill outside the clock (it is the same contiguous prefill on
        both sides): the first step admits all 8 requests."""
        eng = engines[kv]
        reqs = [eng.submit_request(p, new) for p in prompts]
        eng.step()
        torch.cuda.synchronize()
        s0, t0 = eng.steps, time.perf_counter()
        while not eng.idle:
            eng.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return [r.tokens for r in reqs], 8 * (eng.steps - s0) / dt

    outs = {kv: run(kv)[0] for kv in engines}          # warmup + capture
    same = sum(x == y for a, b in zip(outs["fp8"], outs["bf16"])
               for x, y in zip(a[-new:], b[-new:])) / (8 * new)
    print(f"{model_name}: 8 slots, prompts {lengths}, {new} new each, graph, "
          f"fp8 weights; token agreement kv fp8 vs bf16 {same:.3f} "
          "(recorded, not judged)")
    res = {kv: [] for kv in engines}
    for _ in range(rounds):
        for kv in engines:
            res[kv].append(run(kv)[1])
    for kv, xs in res.items():
        med = statistics.median(xs)
        print(f"  kv {kv:<5} median {med:8.1f} tok/s   spread {min(xs):.1f}.."
              f"{max(xs):.1f}  ({8e3 / med:.3f} ms/step, {len(xs)} rounds, "
              "decode steps only)")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "kvfp8bench needs a GPU"
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="kernels",
                    choices=("kernels", "engine"))
    ap.add_argument("model", nargs="?", default="llama3-8b")
    ap.add_argument("--prompt", type=int, default=1984)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.mode == "kernels":
        kernels()
    else:
        engine(args.model, args.prompt, args.new, args.rounds)
