#!/usr/bin/env python3
"""Paged prefill microbench: attn_prefill_paged against the v7 forward on
the same rows gathered contiguous, and the engine with prefill="paged"
against prefill="contiguous".

  python scripts/prefillbench.py kernels
  python scripts/prefillbench.py engine [model] [prefill_chunk]

Both sides of every comparison run in this process, alternating round by
round, after their outputs were checked against each other. Printed per
side: median over the rounds and the min..max spread. Kernel times are
CALL times (launches included) between two device events; engine numbers
are wall time, tok/s over the whole run (prefill included) and the time
from submission to each request's first token.
"""
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

DEV = "cuda:0"
ROUNDS, CALLS = 9, 50


def ab_rounds(sides, rounds=ROUNDS, calls=CALLS):
    for fn in sides.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    return out


def report(title, res):
    print(title)
    for name, xs in res.items():
        print(f"  {name:<20} median {statistics.median(xs):8.2f} us/call   "
              f"spread {min(xs):.2f}..{max(xs):.2f}  ({len(xs)} rounds)")


def kernels():
    from trainingjob_operator_amd.ops import (
        native, prefill_attention_paged, prefill_work, reference,
    )
    from trainingjob_operator_amd.ops.attention import flash_attention_fwd_v7
    native.load(require=True)
    H, n_kv, D = 32, 8, 128
    scale = 1.0 / math.sqrt(D)
    for T in (2048, 4096):
        g = torch.Generator().manual_seed(T)
        q = (torch.randn(T, H, D, generator=g) * .5).bfloat16().to(DEV)
        k = (torch.randn(n_kv, T, D, generator=g) * .5).bfloat16().to(DEV)
        v = (torch.randn(n_kv, T, D, generator=g) * .5).bfloat16().to(DEV)
        n = T // 64
        perm = torch.randperm(n + 8, generator=g)[:n].to(DEV)
        kp = torch.zeros(n + 8, n_kv, 64, D, dtype=torch.bfloat16, device=DEV)
        vp = torch.zeros_like(kp)
        kp[perm] = k.reshape(n_kv, n, 64, D).transpose(0, 1)
        vp[perm] = v.reshape(n_kv, n, 64, D).transpose(0, 1)
        table = perm.to(torch.int32)[None].contiguous()
        work, _, _ = prefill_work([(0, 0, T)], DEV)
        q4, k4, v4 = q.transpose(0, 1)[None], k[None], v[None]
        o = torch.empty_like(q)
        a = flash_attention_fwd_v7(q4, k4, v4, scale)[0][0].transpose(0, 1)
        b = prefill_attention_paged(q, kp, vp, table, work, scale, out=o)
        assert torch.equal(a, b), "paged prefill != v7"
        res = ab_rounds({
            "attn_fwd_v7": lambda: flash_attention_fwd_v7(q4, k4, v4, scale),
            "attn_prefill_paged": lambda: prefill_attention_paged(
                q, kp, vp, table, work, scale, out=o),
        })
        report(f"one sequence T={T} H={H} n_kv={n_kv} from position 0, "
               f"pages shuffled (bit-equal outputs)", res)
        del kp, vp

    # ragged: 8 chunks of 37..700 tokens, one slot each, from position 0
    lengths = [37, 128, 300, 512, 64, 700, 200, 450]
    max_pages = 11
    g = torch.Generator().manual_seed(1)
    n_pages = len(lengths) * max_pages
    kp = (torch.randn(n_pages, n_kv, 64, D, generator=g) * .5
          ).bfloat16().to(DEV)
    vp = (torch.randn(n_pages, n_kv, 64, D, generator=g) * .5
          ).bfloat16().to(DEV)
    table = torch.randperm(n_pages, generator=g).to(torch.int32).reshape(
        len(lengths), max_pages).to(DEV)
    T = sum(lengths)
    q = (torch.randn(T, H, D, generator=g) * .5).bfloat16().to(DEV)
    work, _, _ = prefill_work([(s, 0, n) for s, n in enumerate(lengths)], DEV)
    o = prefill_attention_paged(q, kp, vp, table, work, scale)
    ref = reference.prefill_attention_paged(q, kp, vp, table, work, scale)
    err = (o.float() - ref.float()).abs().max().item()
    assert err < 3e-2, err
    res = ab_rounds({"attn_prefill_paged": lambda: prefill_attention_paged(
        q, kp, vp, table, work, scale, out=o)})
    report(f"ragged: chunks {lengths} ({T} rows, {work.shape[0]} blocks), "
           f"max err vs fp32 twin {err:.2e}", res)


def engine(model_name, chunk):
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.generate import build_inference_model
    from trainingjob_operator_amd.models.paged import PagedEngine, pages_for
    cfg = CONFIGS[model_name]
    m = build_inference_model(cfg, torch.device(DEV))
    lengths = [37, 128, 300, 512, 64, 700, 200, 450]
    new = 64
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).to(DEV)
               for n in lengths]
    need = max(pages_for(n + new) for n in lengths)

    def run(**kw):
        eng = PagedEngine(m, max_slots=8, n_pages=need * 8,
                          max_pages_per_seq=need, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reqs = [eng.submit_request(p, new) for p in prompts]
        first = {}
        with torch.no_grad():
            while not eng.idle:
                eng.step()                 # ends in a host sync (argmax)
                now = time.perf_counter() - t0
                for r in reqs:
                    if r.n_new > 0 and r.id not in first:
                        first[r.id] = now
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return ([r.tokens for r in reqs], len(prompts) * new / dt,
                [first[r.id] for r in reqs])

    sides = {"contiguous": {}, "paged": {"prefill": "paged",
                                        "prefill_chunk": chunk}}
    toks = {name: run(**kw)[0] for name, kw in sides.items()}   # warmup
    same = sum(int(x == y) for a, b in zip(toks["contiguous"], toks["paged"])
               for x, y in zip(a, b)) / sum(len(a) for a in toks["paged"])
    print(f"{model_name}: 8 ragged requests (prompts {lengths}, {new} new "
          f"each), prefill_chunk {chunk}, token agreement paged vs "
          f"contiguous prefill {same:.3f}")
    res = {name: [] for name in sides}
    for _ in range(5):
        for name, kw in sides.items():
            res[name].append(run(**kw)[1:])
    for name, rs in res.items():
        tps = [r[0] for r in rs]
        ttft = [statistics.median(r[1][i] for r in rs) * 1e3
                for i in range(len(lengths))]
        print(f"  {name:<12} median {statistics.median(tps):8.1f} tok/s   "
              f"spread {min(tps):.1f}..{max(tps):.1f}  ({len(tps)} rounds)")
        print(f"  {'':<12} first token after ms (median, per request): "
              + " ".join(f"{t:.0f}" for t in ttft)
              + f"   mean {statistics.mean(ttft):.0f}")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "prefillbench needs a GPU"
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "kernels":
        kernels()
    elif mode == "engine":
        engine(sys.argv[2] if len(sys.argv) > 2 else "llama3-8b",
               int(sys.argv[3]) if len(sys.argv) > 3 else 512)
    else:
        sys.exit(f"unknown mode {mode!r}")
