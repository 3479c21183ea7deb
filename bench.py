#!/usr/bin/env python3
"""Flagship benchmark: managed Llama-3-8B training throughput on MI355X.

Measures the metric BASELINE.json names — tokens/sec of Llama-3-8B at
1/2/4/8 MI355X GPUs (DDP over RCCL/xGMI) on synthetic data with
random-init weights.

Single GPU:   python bench.py --gpus 1 --steps 10 --warmup 3
Multi GPU:    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
                  --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times --steps steps and prints the result
line; nothing else. --dump-outputs DIR also writes what the last timed
step computed as DIR/<name>.npy (same arguments -> same inputs, so two
builds can be compared output for output). --full is reserved for any
measurement beyond the headline figure; there is none at present.

Rank 0 prints exactly ONE JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time


def log(msg: str) -> None:
    print(msg, file=sys.stderr, flush=True)


TUNABLEOP_CSV = os.path.join(
    os.path.dirname(os.path.abspath(__file__)),
    "trainingjob_operator_amd", "data", "tunableop_gfx950.csv")


def stage_tunableop() -> None:
    """Use the committed hipBLASLt/rocBLAS GEMM tuning results when present
    (tuned once on MI355X; torch appends the device ordinal to the
    filename, so stage one copy per potential device). Must run before
    torch is imported."""
    if os.environ.get("PYTORCH_TUNABLEOP_ENABLED"):
        return  # user controls it
    if not os.path.exists(TUNABLEOP_CSV):
        return
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="tunableop_")
    for i in range(16):
        shutil.copy(TUNABLEOP_CSV, os.path.join(d, f"tunableop{i}.csv"))
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = os.path.join(d, "tunableop.csv")
    os.environ["PYTORCH_TUNABLEOP_VERBOSE"] = "0"


DUMP_SAMPLE_ELEMS = 1 << 22   # 16 MB of float32 — far under the 64 MB cap
DUMP_SAMPLE_SEED = 20240521


def dump_outputs(out_dir: str, trainer, last_loss) -> None:
    """Write what the last timed train_step() handed its caller: the loss
    it returned and the weights it left behind. The flat weight buffer of
    the 8B model is 16 GB, so a fixed, seeded, sorted sample of its
    elements is written (all of it when it is small enough)."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    if last_loss is not None:
        np.save(os.path.join(out_dir, "loss.npy"),
                last_loss.detach().float().cpu().reshape(1).numpy())
    flat = trainer.store.flat_param
    if flat.numel() > DUMP_SAMPLE_ELEMS:
        g = torch.Generator(device="cpu").manual_seed(DUMP_SAMPLE_SEED)
        idx = torch.randint(0, flat.numel(), (DUMP_SAMPLE_ELEMS,),
                            generator=g).sort().values
        flat = flat.index_select(0, idx.to(flat.device))
    np.save(os.path.join(out_dir, "params_sample.npy"),
            flat.detach().float().cpu().numpy())
    log(f"[bench] wrote loss.npy and params_sample.npy to {out_dir}")


def main() -> None:
    ap =argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default=None,
                    help="model config (default: llama3-8b on GPU, "
                         "llama-tiny on CPU)")
    ap.add_argument("--micro-batch", type=int, default=2)
    ap.add_argument("--grad-accum", type=int, default=2)
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--checkpoint-activations", action="store_true")
    ap.add_argument("--bucket-mb", type=int, default=128)
    ap.add_argument("--tp", type=int, default=1,
                    help="tensor-parallel degree (world = dp x tp)")
    ap.add_argument("--fp8", action="store_true",
                    help="fp8 (e4m3fn) forward projection GEMMs — opt-in; "
                         "the headline bench stays bf16")
    ap.add_argument("--graphs", action="store_true",
                    help="EXPERIMENTAL: hipGraph step capture (replay of "
                         "large-seq graphs currently faults in the ROCm "
                         "runtime — validated only at small scale)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step computed (its loss and a fixed seeded sample "
                         "of the updated weights) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run whatever the benchmark measures beyond "
                         "the headline figure (nothing at present: a plain "
                         "run already does only setup, warmup, the timed "
                         "steps and the result line)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1 (it is the number of timed "
                 "steps that ms_per_step averages over)")

    if os.environ.get("BENCH_DEBUG"):
        import faulthandler
        faulthandler.dump_traceback_later(
            int(os.environ.get("BENCH_DEBUG_TIMEOUT", "150")), exit=True)

    stage_tunableop()
    import torch
    import torch.distributed as dist

    from trainingjob_operator_amd.parallel import dist_ctx
    from trainingjob_operator_amd.training import TrainConfig, Trainer

    on_gpu = torch.cuda.is_available()
    model = args.model or ("llama3-8b" if on_gpu else "llama-tiny")
    seq_len = args.seq_len if on_gpu else min(args.seq_len, 128)

    ctx = dist_ctx.from_env()
    if "RANK" not in os.environ and args.gpus == 1:
        ctx.world_size = 1
    dist_ctx.init_process_group(ctx)
    n_gpus = ctx.world_size if ctx.is_distributed else 1

    cfg = TrainConfig(
        model=model,
        micro_batch=args.micro_batch,
        grad_accum=args.grad_accum,
        seq_len=seq_len,
        checkpoint_activations=args.checkpoint_activations,
        bucket_bytes=args.bucket_mb << 20,
        use_graphs=on_gpu and args.graphs,
        fp8_projections=on_gpu and args.fp8,
        tp_size=args.tp,
    )
    log(f"[bench] rank {ctx.rank}/{n_gpus} model={model} "
        f"mb={cfg.micro_batch} ga={cfg.grad_accum} seq={cfg.seq_len} "
        f"device={'cuda:%d' % ctx.local_rank if on_gpu else 'cpu'}")

    t_build = time.perf_counter()
    trainer = Trainer(cfg, ctx)
    log(f"[bench] built in {time.perf_counter() - t_build:.1f}s "
        f"({cfg.model_config.n_params / 1e9:.2f}B params)")

    for i in range(args.warmup):
        try:
            loss = trainer.train_step()
        except Exception as e:
            if cfg.use_graphs and trainer._graph is None:
                log(f"[bench] graph capture failed ({e!r}); eager fallback")
                cfg.use_graphs = False
                loss = trainer.train_step()
            else:
                raise
        log(f"[bench] warmup {i}: loss={loss.item():.4f} "
            f"graphs={trainer._graph is not None}")

    if ctx.is_distributed:
        dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last_loss = None
    for i in range(args.steps):
        last_loss = trainer.train_step()
        if os.environ.get("BENCH_DEBUG"):
            log(f"[bench] step {i} queued")
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if ctx.is_distributed:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=trainer.device if on_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        dist.barrier()

    if args.dump_outputs and ctx.rank == 0:
        dump_outputs(args.dump_outputs, trainer, last_loss)

    # with TP, tp ranks share one replica: whole-job tokens count replicas
    n_replicas = n_gpus // max(args.tp, 1)
    tokens_per_step_rank = cfg.tokens_per_step_per_rank()
    total_tokens = tokens_per_step_rank * n_replicas * args.steps
    tokens_per_sec = total_tokens / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if ctx.rank == 0:
        result = {
            "metric": "tokens_per_sec_llama3_8b" if model == "llama3-8b"
                      else f"tokens_per_sec_{model}",
            "value": round(tokens_per_sec, 1),
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 1),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "model": model,
                "global_batch": (cfg.micro_batch * cfg.grad_accum
                                 * (n_gpus // max(args.tp, 1))),
                "seq_len": cfg.seq_len,
                "parallelism": (f"dp{n_gpus // max(args.tp, 1)}"
                                + (f"tp{args.tp}" if args.tp > 1 else "")),
                "micro_batch": cfg.micro_batch,
                "grad_accum": cfg.grad_accum,
                "checkpoint_activations": cfg.checkpoint_activations,
            },
        }
        print(json.dumps(result), flush=True)

    dist_ctx.destroy_process_group()


if __name__ == "__main__":
    main()
