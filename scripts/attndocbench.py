#!/usr/bin/env python3
"""Per-kernel time of document-masked attention against the causal entries.

    python scripts/attndocbench.py [--repeats 7] [--inner 10] [--out FILE]

One process, B=1 H=32 HKV=8 S=4096 D=128 bf16. Cases: the causal entries
(attn_fwd_strided and the causal dq/dv/dk launches, under the ownership the
library picks for the shape), and the document kernels on one document of
4096, 4 x 1024, 16 x 256 and one fixed unaligned mix. Each of fwd, dq, dv
and dk is launched alone (the backward kernels through attn_bwd_part, with
the case's own lse and delta as inputs), warmed, then timed with device
events around `inner` launches. The cases are interleaved: one repeat walks
all cases and kernels, and the repeats give the run-to-run spread. Prints
one JSON line per (case, kernel): mean, min, max and standard deviation of
the per-launch time over the repeats, in us, and a last line with the
comparisons profiles/r10_doc_attention.md reports."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, H, HKV, S, D = 1, 32, 8, 4096, 128
MIX = [1000, 37, 1500, 300, 1259]
CASES = [("causal", None), ("doc_1x4096", [4096]), ("doc_4x1024", [1024] * 4),
         ("doc_16x256", [256] * 16), ("doc_mix", MIX)]
KERNELS = ("fwd", "dq", "dv", "dk")
PART = {"dq": 1, "dv": 2, "dk": 4}
WARM = 3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.repeats >= 2 and args.inner >= 1

    import torch
    assert torch.cuda.is_available(), "attndocbench needs a GPU"
    from trainingjob_operator_amd.ops import native
    from trainingjob_operator_amd.ops.attention import flash_attention_delta
    from trainingjob_operator_amd.ops.docmask import doc_bounds_from_lengths
    lib = native.load(require=True)
    dev = "cuda"
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)

    def rnd(h):
        return (torch.randn(B, h, S, D, device=dev) * .5).bfloat16()
    q, k, v, gout = rnd(H), rnd(HKV), rnd(HKV), rnd(H)
    dq = torch.empty_like(q)
    dk, dv = torch.empty_like(k), torch.empty_like(v)

    def tri(t):
        return (t.stride(0), t.stride(1), t.stride(2))

    state = {}
    for name, lengths in CASES:
        assert lengths is None or sum(lengths) == S
        bounds = None if lengths is None else doc_bounds_from_lengths(
            [lengths] * B, device=dev)
        out = torch.empty_like(q)
        lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
        state[name] = dict(bounds=bounds, out=out, lse=lse)

    def launch(name, kernel):
        st_ = state[name]
        bounds, out, lse = st_["bounds"], st_["out"], st_["lse"]
        bptr = None if bounds is None else bounds.data_ptr()
        if kernel == "fwd":
            st = native.stride_array(tri(q), tri(k), tri(v), tri(out))
            if bounds is None:
                rc = lib.attn_fwd_strided(
                    native.stream_ptr(), q.data_ptr(), k.data_ptr(),
                    v.data_ptr(), out.data_ptr(), lse.data_ptr(), st,
                    B, H, HKV, S, scale)
            else:
                rc = lib.attn_doc_fwd_strided(
                    native.stream_ptr(), q.data_ptr(), k.data_ptr(),
                    v.data_ptr(), out.data_ptr(), lse.data_ptr(), bptr, st,
                    B, H, HKV, S, scale)
        else:
            st = native.stride_array(tri(q), tri(k), tri(v), tri(out),
                                     tri(gout), tri(dq), tri(dk), tri(dv))
            rc = lib.attn_bwd_part(
                native.stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
                gout.data_ptr(), lse.data_ptr(), st_["delta"].data_ptr(),
                dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), bptr, st,
                B, H, HKV, S, scale, PART[kernel])
        native.check_rc(rc, f"{name}/{kernel}")

    # every case's own lse and delta, then a warm-up of every launch
    for name, _ in CASES:
        launch(name, "fwd")
        state[name]["delta"] = flash_attention_delta(state[name]["out"], gout)
    for name, _ in CASES:
        for kernel in KERNELS:
            for _ in range(WARM):
                launch(name, kernel)
    torch.cuda.synchronize()

    times = {(n, kn): [] for n, _ in CASES for kn in KERNELS}
    for _ in range(args.repeats):
        for name, _lengths in CASES:
            for kernel in KERNELS:
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _i in range(args.inner):
                    launch(name, kernel)
                e1.record()
                e1.synchronize()
                times[(name, kernel)].append(
                    e0.elapsed_time(e1) * 1e3 / args.inner)

    lines = []
    stat = {}
    for (name, kernel), t in times.items():
        stat[(name, kernel)] = dict(mean=statistics.mean(t), min=min(t),
                                    max=max(t), sd=statistics.stdev(t))
        lines.append(json.dumps(dict(
            case=name, kernel=kernel, repeats=args.repeats, inner=args.inner,
            **{k_: round(v_, 1) for k_, v_ in stat[(name, kernel)].items()})))
    summary = {}
    for kernel in KERNELS:
        m = {n: stat[(n, kernel)] for n, _ in CASES}
        spread = max(s["max"] - s["min"] for s in m.values())
        summary[kernel] = dict(
            spread_us=round(spread, 1),
            skip_16_lt_4=m["doc_16x256"]["mean"] + spread
            < m["doc_4x1024"]["mean"],
            skip_4_lt_1=m["doc_4x1024"]["mean"] + spread
            < m["doc_1x4096"]["mean"],
            one_doc_minus_causal_us=round(
                m["doc_1x4096"]["mean"] - m["causal"]["mean"], 1),
            causal_spread_us=round(m["causal"]["max"] - m["causal"]["min"],
                                   1))
    lines.append(json.dumps(dict(summary=summary)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
