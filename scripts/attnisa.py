#!/usr/bin/env python3
"""Per-kernel ISA summary of the attention source, and its comparison.

  attnisa.py dump OUT.json [--src attention.hip]
  attnisa.py diff A.json B.json [--pair A_SUBSTRING=B_SUBSTRING ...]

dump compiles the attention source to gfx950 assembly with the flags of
native.build_ops (device side only, no GPU needed) and writes, per kernel
symbol: VGPR and SGPR counts, scratch and LDS bytes, the instruction count,
a hash of the instruction stream with comments and local labels stripped,
and the histogram of mnemonics. diff prints `identical` per kernel, or the
metadata and histogram entries that changed. Kernels pair by mangled symbol;
one that was renamed, or whose template or argument list changed, is named
with --pair, e.g. --pair attn_bwd_dq_kernelILb1E=attn_bwd_dq_kernelILi1E.
To compare a branch with its parent, dump each from its own checkout (`git
worktree add DIR REV`, then
`--src DIR/trainingjob_operator_amd/ops/hip/attention.hip`).

The compiler version decides the output, so this is a tool, not a test.
"""
from __future__ import annotations

import argparse
import collections
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SRC = os.path.join(ROOT, "trainingjob_operator_amd", "ops", "hip",
                           "attention.hip")
NATIVE_PY = os.path.join(ROOT, "trainingjob_operator_amd", "ops", "native.py")


def build_flags() -> list:
    """The compile flags of native.build_ops, read from its command list
    (native.py is parsed, not imported: the package pulls in torch)."""
    with open(NATIVE_PY) as f:
        src = f.read()
    m = re.search(r"cmd = \[(.*?)\]", src, re.S)
    if not m:
        raise SystemExit("no command list found in native.build_ops")
    words = re.findall(r'"([^"]+)"', m.group(1))
    return [w for w in words
            if w.startswith("-") and w not in ("-shared", "-fPIC", "-o")]


META_KEYS = {
    "vgpr": "vgpr_count",
    "sgpr": "sgpr_count",
    "scratch_bytes": "private_segment_fixed_size",
    "lds_bytes": "group_segment_fixed_size",
}


def assemble(src: str) -> str:
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "attention.s")
        subprocess.run(["hipcc", *build_flags(), "--cuda-device-only", "-S",
                        src, "-o", out], check=True)
        with open(out) as f:
            return f.read()


def kernel_meta(text: str) -> dict:
    """name -> register and memory figures from the amdhsa.kernels notes."""
    notes = text[text.index("amdhsa.kernels:"):]
    # one list item per kernel, at the indentation of the first "- "
    indent = re.search(r"^( *)- ", notes, re.M).group(1)
    meta = {}
    for blk in re.split(r"^" + indent + r"- ", notes, flags=re.M)[1:]:
        def field(key):
            return re.search(r"^\s*\." + key + r":\s*(\S+)", blk,
                             re.M).group(1)
        if not re.search(r"^\s*\.name:", blk, re.M):
            continue
        meta[field("name")] = {k: int(field(v)) for k, v in META_KEYS.items()}
    return meta


def kernel_stream(text: str, name: str) -> list:
    """The instructions of one kernel, comments and local labels stripped."""
    m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end",
                  text, re.S | re.M)
    if not m:
        raise SystemExit(f"no body found for kernel {name}")
    stream = []
    for line in m.group(1).splitlines():
        line = re.sub(r"\.L\w+", "L", line.split(";")[0]).strip()
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        stream.append(" ".join(line.split()))
    return stream


def summarise(text: str) -> dict:
    kernels = {}
    for name, meta in sorted(kernel_meta(text).items()):
        stream = kernel_stream(text, name)
        hist = collections.Counter(ins.split()[0] for ins in stream)
        kernels[name] = dict(
            meta, instructions=len(stream),
            stream_sha256=hashlib.sha256(
                "\n".join(stream).encode()).hexdigest(),
            histogram=dict(sorted(hist.items())))
    return kernels


def dump(args) -> int:
    kernels = summarise(assemble(args.src))
    with open(args.out, "w") as f:
        json.dump(kernels, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(kernels)} kernels -> {args.out}")
    return 0


def only_match(kernels: dict, sub: str, side: str) -> str:
    """The one kernel symbol of a dump that contains sub."""
    names = [n for n in kernels if sub in n]
    if len(names) != 1:
        raise SystemExit(f"--pair: {sub!r} matches {len(names)} kernels of "
                         f"{side}: {' '.join(sorted(names)) or 'none'}")
    return names[0]


def diff(args) -> int:
    with open(args.a) as f:
        a = json.load(f)
    with open(args.b) as f:
        b = json.load(f)
    renamed = {}                     # name in A -> name in B
    for spec in args.pair:
        sub_a, _, sub_b = spec.partition("=")
        na, nb = only_match(a, sub_a, "A"), only_match(b, sub_b, "B")
        if na in b or nb in a:
            raise SystemExit(f"--pair {spec}: {na if na in b else nb} "
                             "is in both dumps already")
        renamed[na] = nb
    total = len(set(a) | set(b)) - len(renamed)
    changed = 0
    for name in sorted((set(a) | set(b)) - set(renamed.values())):
        other = renamed.get(name, name)
        if name not in a or other not in b:
            print(f"{name}: only in {'A' if name in a else 'B'}")
            changed += 1
            continue
        ka, kb = a[name], b[other]
        label = name if other == name else f"{name} -> {other}"
        if ka["stream_sha256"] == kb["stream_sha256"] and all(
                ka[k] == kb[k] for k in META_KEYS):
            print(f"{label}: identical")
            continue
        changed += 1
        print(f"{label}: DIFFERENT")
        for k in (*META_KEYS, "instructions"):
            mark = "" if ka[k] == kb[k] else "   <--"
            print(f"    {k:14s} {ka[k]:6d} -> {kb[k]:6d}{mark}")
        ha, hb = ka["histogram"], kb["histogram"]
        for mn in sorted(set(ha) | set(hb)):
            if ha.get(mn, 0) != hb.get(mn, 0):
                print(f"    {mn:30s} {ha.get(mn, 0):5d} -> {hb.get(mn, 0):5d}")
    print(f"{total} kernels, {changed} differ")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump", help="compile and summarise every kernel")
    d.add_argument("out")
    d.add_argument("--src", default=DEFAULT_SRC)
    d.set_defaults(fn=dump)
    c = sub.add_parser("diff", help="compare two dumps kernel by kernel")
    c.add_argument("a")
    c.add_argument("b")
    c.add_argument("--pair", action="append", default=[],
                   metavar="A_SUBSTRING=B_SUBSTRING",
                   help="compare the one kernel of A whose symbol contains "
                        "A_SUBSTRING with the one of B that contains "
                        "B_SUBSTRING (a renamed kernel); repeatable")
    c.set_defaults(fn=diff)
    args = ap.parse_args()
    return args.fn(args)


if __name__ == "__main__":
    sys.exit(main())
