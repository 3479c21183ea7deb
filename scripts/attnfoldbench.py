#!/usr/bin/env python3
"""dv + dk time by strip ownership (AITJ_ATTN_BWD_FOLD 0 | 1 | 2).

Run it under the profiler, then read the trace back:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- \\
        python scripts/attnfoldbench.py run
    python scripts/attnfoldbench.py read OUT

`run` walks the cells below in one process: causal fwd+bwd at H=32 HKV=8
S=4096, B in 1 2 4 8, unsplit under each ownership and (B=1, 2) split under
the identity, the whole list twice so that the modes alternate. Each cell
is WARM + TIMED calls; the knobs are read on every launch, so the process
switches them through its environment. It prints the cell list. `read`
takes the i-th dv and the i-th dk dispatch of the kernel trace (whatever
the kernel is called under that ownership) as call i of that list and
prints one JSON line per cell: average and standard deviation, us, over
the timed calls."""
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, HKV, S, D = 32, 8, 4096, 128
WARM, TIMED = 2, 8
REPS = 2


def cells():
    out = []
    for rep in range(REPS):
        for B in (1, 2, 4, 8):
            for fold in ("0", "1", "2"):
                out.append(dict(rep=rep, B=B, split="0", fold=fold))
            if B <= 2:
                out.append(dict(rep=rep, B=B, split="1", fold="0"))
    return out


def run():
    import torch
    from trainingjob_operator_amd.ops.attention import flash_attention
    for cell in cells():
        B = cell["B"]
        os.environ["AITJ_ATTN_BWD_SPLIT"] = cell["split"]
        os.environ["AITJ_ATTN_BWD_FOLD"] = cell["fold"]
        torch.manual_seed(0)

        def rnd(h):
            return (torch.randn(B, h, S, D, device="cuda") * .5).bfloat16()
        q, k, v = (rnd(h).requires_grad_() for h in (H, HKV, HKV))
        gout = rnd(H)
        for _ in range(WARM + TIMED):
            flash_attention(q, k, v).backward(gout)
            q.grad = k.grad = v.grad = None
        torch.cuda.synchronize()
        print(json.dumps(cell), flush=True)


def read(outdir):
    paths = glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"),
                      recursive=True)
    assert len(paths) == 1, paths
    rows = list(csv.DictReader(open(paths[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = {}
    for tag in ("attn_bwd_dv", "attn_bwd_dk", "attn_bwd_reduce"):
        per[tag] = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                    for r in rows if tag in r["Kernel_Name"]]
    n = WARM + TIMED
    cs = cells()
    assert len(per["attn_bwd_dv"]) == len(per["attn_bwd_dk"]) == n * len(cs)
    red = iter(per["attn_bwd_reduce"])
    for i, cell in enumerate(cs):
        res = dict(cell)
        for tag in ("attn_bwd_dv", "attn_bwd_dk"):
            t = per[tag][i * n + WARM:(i + 1) * n]
            res[tag[-2:]] = round(statistics.mean(t), 1)
            res[tag[-2:] + "_sd"] = round(statistics.stdev(t), 1)
        res["reduce"] = 0.0
        if cell["split"] == "1":
            t = [next(red) for _ in range(n)][WARM:]
            res["reduce"] = round(statistics.mean(t), 1)
        res["sum"] = round(res["dv"] + res["dk"] + res["reduce"], 1)
        print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "read":
        read(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    else:
        sys.exit(__doc__)
