#!/usr/bin/env python3
"""Paged decode microbench: the paged kernels against the contiguous ones
on identical contents (pages shuffled), and the continuous-batching
engine against one-request-at-a-time generate().

  python scripts/pagedbench.py kernels           # attn_decode / rope_cache
  python scripts/pagedbench.py engine [model]    # ragged mix, tok/s

Both sides of every comparison run in this process, alternating round by
round; a round is N back-to-back calls between two device events. Printed
per side: median over the rounds and the min..max spread. The times are
CALL times (launches included), not kernel times.
"""
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

DEV = "cuda:0"
ROUNDS, CALLS = 9, 200


def ab_rounds(sides, rounds=ROUNDS, calls=CALLS):
    """sides: {name: fn}. Alternates the sides each round; returns
    {name: [us per call, one per round]}."""
    for fn in sides.values():                  # warm every shape
        for _ in range(10):
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
        print(f"  {name:<18} median {statistics.median(xs):8.2f} us/call   "
              f"spread {min(xs):.2f}..{max(xs):.2f}  ({len(xs)} rounds)")


def paged_case(B, n_kv, D, max_pages, fill, seed):
    """Pools with B*max_pages shuffled pages and the SAME rows as a
    contiguous [B, n_kv, max_pages*64, D] cache."""
    g = torch.Generator().manual_seed(seed)
    n_pages = B * max_pages
    kp = (torch.randn(n_pages, n_kv, 64, D, generator=g) * .5).bfloat16()
    vp = (torch.randn(n_pages, n_kv, 64, D, generator=g) * .5).bfloat16()
    table = torch.randperm(n_pages, generator=g).reshape(B, max_pages)

    def contig(pool):
        return pool[table].permute(0, 2, 1, 3, 4).reshape(
            B, n_kv, max_pages * 64, D).contiguous().to(DEV)

    kc, vc = contig(kp), contig(vp)
    pos = torch.full((B,), fill - 1, dtype=torch.int64, device=DEV)
    return (kp.to(DEV), vp.to(DEV), table.to(torch.int32).to(DEV), pos,
            kc, vc)


def kernels():
    from trainingjob_operator_amd.ops import (
        decode_attention, decode_attention_paged, make_inv_freq, native,
        rope_cache_paged,
    )
    lib = native.load(require=True)
    B, H, n_kv, D = 8, 32, 8, 128
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)
    q = (torch.randn(B, H, 1, D, device=DEV) * .5).bfloat16()
    for rows, fill in ((2048, 2048), (8192, 512)):
        kp, vp, table, pos, kc, vc = paged_case(B, n_kv, D, rows // 64,
                                                fill, seed=rows)
        pos1 = pos[:1].clone()
        a = decode_attention(q, kc, vc, pos1, scale)
        b = decode_attention_paged(q, kp, vp, table, pos, scale)
        assert torch.equal(a, b), "paged != contiguous"
        res = ab_rounds({
            "attn_decode": lambda: decode_attention(q, kc, vc, pos1, scale),
            "attn_decode_paged": lambda: decode_attention_paged(
                q, kp, vp, table, pos, scale),
        })
        report(f"attention B={B} H={H} n_kv={n_kv} fill {fill} in a "
               f"{rows}-row cache (bit-equal outputs)", res)
        del kp, vp, kc, vc

    nh = H
    kp, vp, table, pos, kc, vc = paged_case(B, n_kv, D, 32, 1000, seed=5)
    pos1 = pos[:1].clone()
    inv_freq = make_inv_freq(D, 500000.0, device=DEV)
    qkv = (torch.randn(B, (nh + 2 * n_kv) * D, device=DEV) * .5).bfloat16()
    qo = torch.empty(B, nh, D, dtype=torch.bfloat16, device=DEV)

    def contiguous_rope():
        rc = lib.rope_cache(native.stream_ptr(), qkv.data_ptr(),
                            qo.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                            inv_freq.data_ptr(), pos1.data_ptr(), B, nh,
                            n_kv, kc.shape[2], D)
        assert rc == 0
        return qo

    qp2 = torch.empty_like(qo)

    def paged_rope():          # the raw launcher too: same host work
        rc = lib.rope_cache_paged(native.stream_ptr(), qkv.data_ptr(),
                                  qp2.data_ptr(), kp.data_ptr(),
                                  vp.data_ptr(), inv_freq.data_ptr(),
                                  table.data_ptr(), pos.data_ptr(), B, nh,
                                  n_kv, kp.shape[0], table.shape[1], D)
        assert rc == 0
        return qp2

    qp = rope_cache_paged(qkv, kp, vp, inv_freq, table, pos, nh, n_kv)
    assert torch.equal(qp, contiguous_rope())
    assert torch.equal(qp, paged_rope())
    res = ab_rounds({"rope_cache": contiguous_rope,
                     "rope_cache_paged": paged_rope})
    report(f"rope + cache write B={B} nh={nh} nkv={n_kv} D={D}", res)


def engine(model_name):
    from trainingjob_operator_amd.models.config import CONFIGS
    from trainingjob_operator_amd.models.generate import (
        build_inference_model, generate,
    )
    from trainingjob_operator_amd.models.paged import generate_ragged
    cfg = CONFIGS[model_name]
    m = build_inference_model(cfg, torch.device(DEV))
    lengths = [37, 128, 300, 512, 64, 700, 200, 450]
    new = 64
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).to(DEV)
               for n in lengths]

    def ragged():
        return generate_ragged(m, prompts, new, max_slots=8)

    def one_by_one():
        return [generate(m, p[None], new)[0] for p in prompts]

    a, b = ragged(), one_by_one()              # warmup + agreement
    agree = sum(int((x == y).sum()) for x, y in zip(a, b)) \
        / sum(x.numel() for x in a)
    print(f"{model_name}: 8 ragged requests (prompts {lengths}, {new} new "
          f"each), token agreement engine vs generate {agree:.3f}")
    res = {"engine": [], "one by one": []}
    for _ in range(3):
        for name, fn in (("engine", ragged), ("one by one", one_by_one)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[name].append(len(prompts) * new
                             / (time.perf_counter() - t0))
    for name, xs in res.items():
        print(f"  {name:<12} median {statistics.median(xs):8.1f} tok/s   "
              f"spread {min(xs):.1f}..{max(xs):.1f}  ({len(xs)} rounds, "
              "prefill included)")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "pagedbench needs a GPU"
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "kernels":
        kernels()
    elif mode == "engine":
        engine(sys.argv[2] if len(sys.argv) > 2 else "llama3-8b")
    else:
        sys.exit(f"unknown mode {mode!r}")
