#!/usr/bin/env python3
"""Validate + time the hipGraph decode path (AITJ_DECODE_GRAPH=1).

Run via gpurun under an explicit `timeout`: hipGraph capture hung on a
large training step on ROCm 7.2, so the graph path is exercised here, not
in the driver-run GPU suite.

  python scripts/graphcheck.py            # correctness on llama-smoke
  python scripts/graphcheck.py bench      # llama3-8b b1/b8 decode tok/s
  python scripts/graphcheck.py --paged    # captured paged engine step
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def tokens_per_sec(model, batch, prompt_len, new_tokens):
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.generate import generate
    from trainingjob_operator_amd.training import build_model
    cfg = CONFIGS[model]
    m = build_model(cfg, torch.device("cuda:0"))
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, cfg.vocab_size, (batch, prompt_len),
                           generator=g).to("cuda:0")
    generate(m, prompt, max_new_tokens=8)          # warmup (+graph capture)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = generate(m, prompt, max_new_tokens=new_tokens)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert out.shape == (batch, prompt_len + new_tokens)
    return batch * new_tokens / dt, dt * 1e3 / new_tokens


def check():
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.generate import (
        build_inference_model, generate,
    )
    for name in ("llama-smoke", "moe-mid"):
        cfg = CONFIGS[name]
        m = build_inference_model(cfg, torch.device("cuda:0"))
        g = torch.Generator().manual_seed(3)
        prompt = torch.randint(0, cfg.vocab_size, (2, 16),
                               generator=g).to("cuda:0")
        os.environ["AITJ_DECODE_GRAPH"] = "0"
        ref = generate(m, prompt, max_new_tokens=24)
        os.environ["AITJ_DECODE_GRAPH"] = "1"
        got = generate(m, prompt, max_new_tokens=24)
        match = (ref == got).float().mean().item()
        print(f"{name}: token agreement graph vs eager: {match:.3f} "
              f"({ref.shape[1]} positions)")
        assert match > 0.95, (name, ref, got)
        del m
        torch.cuda.empty_cache()
    print("graphcheck OK")


def bench():
    os.environ["AITJ_DECODE_GRAPH"] = "1"
    for b in (1, 8):
        tps, ms = tokens_per_sec("llama3-8b", b, 512, 128)
        print(f"llama3-8b b{b} graph decode: {tps:.1f} tok/s, "
              f"{ms:.2f} ms/token")


def session():
    """DecodeSession: capture once, serve many requests (correctness on
    llama-smoke + amortized timing on llama3-8b)."""
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.decode_graph import DecodeSession
    from trainingjob_operator_amd.models.generate import (
        build_inference_model, generate,
    )
    cfg = CONFIGS["llama-smoke"]
    m = build_inference_model(cfg, torch.device("cuda:0"))
    ses = DecodeSession(m, batch=2, max_len=256)
    g = torch.Generator().manual_seed(5)
    for i in range(3):                     # 3 requests, one capture
        prompt = torch.randint(0, cfg.vocab_size, (2, 12 + i),
                               generator=g).to("cuda:0")
        got = ses.generate(prompt, max_new_tokens=16)
        os.environ["AITJ_DECODE_GRAPH"] = "0"
        ref = generate(m, prompt, max_new_tokens=16)
        match = (ref == got).float().mean().item()
        print(f"request {i}: agreement {match:.3f}")
        assert match > 0.95
    del m
    torch.cuda.empty_cache()

    cfg = CONFIGS["llama3-8b"]
    m = build_inference_model(cfg, torch.device("cuda:0"))
    ses = DecodeSession(m, batch=1, max_len=1024)
    prompt = torch.randint(0, cfg.vocab_size, (1, 512),
                           generator=g).to("cuda:0")
    ses.generate(prompt, max_new_tokens=8)           # capture + warmup
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ses.generate(prompt, max_new_tokens=128)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"llama3-8b b1 session decode (no capture in-request): "
          f"{128 / dt:.1f} tok/s, {dt * 1e3 / 128:.2f} ms/token")


def paged():
    """PagedEngine(graph=True): _step_paged captured once at max_slots and
    replayed while requests of different lengths come and go, against the
    same engine run eagerly (llama-smoke)."""
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.generate import (
        build_inference_model,
    )
    from trainingjob_operator_amd.models.paged import PagedEngine
    cfg = CONFIGS["llama-smoke"]
    m = build_inference_model(cfg, torch.device("cuda:0"))
    g = torch.Generator().manual_seed(9)
    lengths = [5, 64, 130, 33, 70, 12]
    news = [24, 9, 30, 17, 40, 8]
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g)
               for n in lengths]
    outs = {}
    for graph in (False, True):
        eng = PagedEngine(m, max_slots=4, n_pages=16, max_pages_per_seq=3,
                          graph=graph)
        ids = [eng.submit(p, n) for p, n in zip(prompts, news)]
        done = {}
        t0 = time.perf_counter()
        while not eng.idle:
            for r in eng.step():
                done[r.id] = r.tokens
            eng.cache.check_block_table()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert eng.cache.pages_free == eng.cache.n_pages
        assert eng.graph_mode == graph
        outs[graph] = [done[i] for i in ids]
        print(f"paged engine graph={graph}: {eng.steps} steps, "
              f"{sum(news) / dt:.1f} tok/s (capture included)")
    same = sum(a == b for x, y in zip(outs[False], outs[True])
               for a, b in zip(x, y))
    total = sum(len(x) for x in outs[False])
    print(f"paged: token agreement graph vs eager: {same / total:.3f} "
          f"({total} positions)")
    assert all(len(x) == len(y) for x, y in zip(outs[False], outs[True]))
    assert same / total > 0.95, outs
    print("graphcheck paged OK")


if __name__ == "__main__":
    if "--paged" in sys.argv[1:]:
        paged()
    elif len(sys.argv) > 1 and sys.argv[1] == "bench":
        bench()
    elif len(sys.argv) > 1 and sys.argv[1] == "session":
        session()
    else:
        check()
