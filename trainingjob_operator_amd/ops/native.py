"""ctypes bindings to the in-tree gfx950 HIP library (libhipops.so).

The library is built by ``build_ops()`` (one direct hipcc invocation,
``--offload-arch=gfx950`` — no hipify, no compatibility layers) and loaded
from the package directory so the ``.so`` travels with the repo snapshot.

Policy: on a GPU box these bindings are REQUIRED — ops fail loudly if the
extension is missing rather than silently falling back to eager PyTorch.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Optional

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "libhipops.so")
SRC_PATH = os.path.join(_PKG_DIR, "hip", "ops.hip")
ATTN_SRC_PATH = os.path.join(_PKG_DIR, "hip", "attention.hip")

_lib: Optional[ctypes.CDLL] = None


class HipOpsUnavailable(RuntimeError):
    pass


def build_ops(verbose: bool = False) -> str:
    """Compile ops.hip -> libhipops.so in-tree for gfx950."""
    cmd = [
        "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
        "-shared", "-fPIC", SRC_PATH, ATTN_SRC_PATH, "-o", LIB_PATH,
    ]
    if verbose:
        print("+", " ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


def _sig(fn, argtypes, restype=None):
    fn.argtypes = argtypes
    fn.restype = restype


def load(require: bool = True) -> Optional[ctypes.CDLL]:
    """Load (and memoize) the HIP ops library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if require:
            raise HipOpsUnavailable(
                f"{LIB_PATH} not built — run trainingjob_operator_amd.ops."
                "native.build_ops() (or __graft_entry__.build())")
        return None
    lib = ctypes.CDLL(LIB_PATH)
    vp, l, i, f = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float
    # every launcher returns int: 0 = launched, nonzero = unsupported shape
    # (callers raise via check_rc — no silent no-op launches)
    _sig(lib.hipops_arch_check, [], i)
    _sig(lib.rmsnorm_fwd, [vp, vp, vp, vp, vp, vp, vp, l, i, f], i)
    _sig(lib.rmsnorm_bwd, [vp, vp, vp, vp, vp, vp, vp, vp, l, i], i)
    _sig(lib.rmsnorm_bwd_partials, [l, i], l)
    _sig(lib.rmsnorm_dw_reduce, [vp, vp, l, vp, i], i)
    _sig(lib.rope, [vp, vp, vp, vp, l, i, i, i, f], i)
    _sig(lib.rope_at, [vp, vp, vp, vp, l, i, i, i, f, i], i)
    _sig(lib.rope_at_dev, [vp, vp, vp, vp, l, i, i, i, f, vp], i)
    _sig(lib.rope_packed, [vp, vp, vp, vp, l, i, l, l, i, i, f], i)
    # rope_packed + (seg_len, pos_a, pos_b): rows at shard positions
    _sig(lib.rope_packed_at, [vp, vp, vp, vp, l, i, l, l, i, i, f, i, i, i],
         i)
    _sig(lib.gemv_bf16, [vp, vp, vp, vp, i, i, i], i)
    _sig(lib.gemv_swiglu, [vp, vp, vp, vp, i, i, i], i)
    _sig(lib.gemv_moe_swiglu, [vp, vp, vp, vp, vp, vp, i, i, i, i], i)
    _sig(lib.gemv_moe, [vp, vp, vp, vp, vp, i, i, i, i], i)
    _sig(lib.attn_decode, [vp, vp, vp, vp, vp, vp, vp,
                           i, i, i, i, i, f], i)
    _sig(lib.rope_cache, [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i], i)
    # paged decode: (q, k_pool, v_pool, block_table int32 [B, max_pages],
    # pos int64 [B], partial, o, B, H, n_kv, n_pages, max_pages, scale)
    _sig(lib.attn_decode_paged, [vp, vp, vp, vp, vp, vp, vp, vp,
                                 i, i, i, i, i, f], i)
    # (qkv, qout, k_pool, v_pool, inv_freq, block_table, pos, B, nh, nkv,
    # n_pages, max_pages, D)
    _sig(lib.rope_cache_paged, [vp, vp, vp, vp, vp, vp, vp, vp,
                                i, i, i, i, i, i], i)
    # paged prefill: (qkv, qout, k_pool, v_pool, inv_freq, block_table,
    # tok_slot int32 [T], tok_pos int64 [T], T, B, nh, nkv, n_pages,
    # max_pages, D)
    _sig(lib.rope_cache_paged_rows, [vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                     i, i, i, i, i, i, i], i)
    # (q [T,H,128], k_pool, v_pool, out, block_table, work int32 [n, 4],
    # n_blocks, T, H, n_kv, B, n_pages, max_pages, scale)
    _sig(lib.attn_prefill_paged, [vp, vp, vp, vp, vp, vp, vp,
                                  i, i, i, i, i, i, i, f], i)
    # clamp of one work row (host callable): (io int[4], T, B, max_pages)
    _sig(lib.attn_prefill_work_decode, [ctypes.POINTER(ctypes.c_int),
                                        i, i, i], i)
    _sig(lib.swiglu_fwd, [vp, vp, vp, vp, l], i)
    _sig(lib.swiglu_bwd, [vp, vp, vp, vp, vp, vp, l], i)
    _sig(lib.swiglu_packed_fwd, [vp, vp, vp, l, i], i)
    _sig(lib.swiglu_packed_bwd, [vp, vp, vp, vp, l, i], i)
    _sig(lib.ce_fwd, [vp, vp, vp, vp, vp, l, i, i], i)
    _sig(lib.ce_bwd, [vp, vp, vp, vp, vp, vp, l, i, i], i)
    _sig(lib.l2normsq, [vp, vp, l, vp, i, vp], i)
    _sig(lib.rows_gather, [vp, vp, vp, vp, l, i], i)
    _sig(lib.rows_scatter, [vp, vp, vp, vp, l, i], i)
    _sig(lib.rows_scatter_add_f32, [vp, vp, vp, vp, l, i], i)
    _sig(lib.moe_combine, [vp, vp, vp, vp, vp, l, i, i], i)
    _sig(lib.moe_combine_bwd, [vp, vp, vp, vp, vp, vp, vp, l, i, i], i)
    _sig(lib.adamw_step, [vp, vp, vp, vp, vp, vp, vp, l,
                          f, f, f, f, f, f, f, f, f, vp], i)
    _sig(lib.adamw_step_bf16mom, [vp, vp, vp, vp, vp, vp, vp, l,
                                  f, f, f, f, f, f, f, f, f, vp], i)
    _sig(lib.mfma_probe, [vp, vp, vp, vp])
    _sig(lib.attn_fwd, [vp, vp, vp, vp, vp, vp,
                        l, l, l, l, l, l, l, l, l, i, i, i, i, f], i)
    _sig(lib.attn_fwd_v5, [vp, vp, vp, vp, vp, vp,
                           l, l, l, l, l, l, l, l, l, i, i, i, f], i)
    _sig(lib.attn_fwd_nw8, [vp, vp, vp, vp, vp, vp,
                            l, l, l, l, l, l, l, l, l, i, i, i, i, f], i)
    _sig(lib.attn_fwd_v7, [vp, vp, vp, vp, vp, vp,
                           l, l, l, l, l, l, l, l, l, i, i, i, i, f], i)
    _sig(lib.attn_bwd, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                        l, l, l, l, l, l, l, l, l, i, i, i, i, f], i)
    # strided entries: stride triples (batch, head, row) as a host long[]
    # (see stride_array): q, k, v, out | q, k, v, out, dout, dq, dk, dv
    lp = ctypes.POINTER(ctypes.c_long)
    _sig(lib.attn_fwd_strided, [vp, vp, vp, vp, vp, vp, lp, i, i, i, i, f], i)
    _sig(lib.attn_bwd_strided, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                lp, i, i, i, i, f], i)
    # ring-attention block entries (causal flag last); stride triples:
    # q, k, v, out | out, dout | q, k, v, dout, dq, dk, dv | o_blk
    _sig(lib.attn_block_fwd, [vp, vp, vp, vp, vp, vp, lp,
                              i, i, i, i, f, i], i)
    _sig(lib.attn_delta, [vp, vp, vp, vp, lp, i, i, i], i)
    _sig(lib.attn_block_bwd, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, lp,
                              i, i, i, i, f, i], i)
    _sig(lib.attn_merge, [vp, vp, vp, vp, vp, lp, i, i, i], i)
    # backward with a caller-owned workspace (ws, ws_bytes last); the size
    # comes from attn_bwd_ws_bytes(B, H, HKV, S, causal), 0 = none needed
    _sig(lib.attn_bwd_ws_bytes, [i, i, i, i, i], l)
    _sig(lib.attn_bwd_ws, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                           l, l, l, l, l, l, l, l, l, i, i, i, i, f,
                           vp, l], i)
    _sig(lib.attn_bwd_strided_ws, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                   vp, lp, i, i, i, i, f, vp, l], i)
    _sig(lib.attn_block_bwd_ws, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, lp,
                                 i, i, i, i, f, i, vp, l], i)
    # rectangular non-causal blocks: (S_q, S_kv) in place of S; lse and delta
    # are [B,H,S_q], dk/dv and the workspace rows follow S_kv
    _sig(lib.attn_block_fwd_rect, [vp, vp, vp, vp, vp, vp, lp,
                                   i, i, i, i, i, f, i], i)
    _sig(lib.attn_block_bwd_rect, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, lp,
                                   i, i, i, i, i, f, i], i)
    _sig(lib.attn_block_bwd_rect_ws, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                      lp, i, i, i, i, i, f, i, vp, l], i)
    _sig(lib.attn_bwd_ws_bytes_rect, [i, i, i, i, i, i], l)
    # block-id decode of the scheduled attention kernels (host callable):
    # (sched 0 legacy | 1 balanced, id, row blocks, heads, batch) ->
    # rank, head, batch
    ip = ctypes.POINTER(ctypes.c_int)
    _sig(lib.attn_sched_decode, [i, i, i, i, i, ip, ip, ip], i)
    # strip ownership of the dv/dk workgroups (host callable): (fold 0
    # identity | 1 fold, workgroup rank, wave, row blocks) -> the wave's
    # first kv row, the workgroup's first q tile
    _sig(lib.attn_bwd_strips_decode, [i, i, i, i, ip, ip], i)
    # pair ownership of the causal unsplit dv/dk workgroups (host callable):
    # (workgroup rank, phase 0 heavy | 1 light, wave, row blocks) -> first kv
    # row, first q tile, sub computed, [ds0, ds1) accumulated, partner wave
    _sig(lib.attn_bwd_pair_decode, [i, i, i, i, ip, ip, ip, ip, ip, ip], i)
    # (batch, heads, kv heads, S, causal, split, kernel 0 dv | 1 dk) -> the
    # ownership a launch gets now: 0 identity, 1 fold, 2 pair
    _sig(lib.attn_bwd_fold_mode, [i, i, i, i, i, i, i], i)
    # document-masked entries: bounds (device int32 [2,B,S]) before the
    # stride triples q, k, v, out | q, k, v, out, dout, dq, dk, dv; the
    # backward runs delta, dq, dv, dk and takes no workspace
    _sig(lib.attn_doc_fwd_strided, [vp, vp, vp, vp, vp, vp, vp, lp,
                                    i, i, i, i, f], i)
    _sig(lib.attn_doc_bwd_strided, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                    vp, vp, lp, i, i, i, i, f], i)
    # one backward kernel alone (part 1 dq | 2 dv | 4 dk, last), for timing:
    # q, k, v, dout, lse, delta, dq, dk, dv, bounds (null = causal), strides
    _sig(lib.attn_bwd_part, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, lp,
                             i, i, i, i, f, i], i)
    # clamped tile ranges of the document kernels (host callable): (kind 0
    # fwd/dq | 1 dv/dk, start or end, row block, S) -> first, last tile
    _sig(lib.attn_doc_tiles_decode, [i, i, i, i, ip, ip], i)
    _sig(lib.mfma_probe32, [vp, vp, vp, vp])
    assert lib.hipops_arch_check() == 950
    _lib = lib
    return lib


def check_rc(rc: int, op: str, detail: str = "") -> None:
    """Raise on a nonzero launcher status (unsupported shape)."""
    if rc != 0:
        raise RuntimeError(
            f"hipops {op}: unsupported shape ({detail}) — the kernel "
            f"launcher refused to launch (rc={rc})")


def stride_array(*triples):
    """Pack (batch, head, row) stride triples for the *_strided launchers."""
    flat = [int(x) for t in triples for x in t]
    assert len(flat) == 3 * len(triples)
    return (ctypes.c_long * len(flat))(*flat)


def available() -> bool:
    return os.path.exists(LIB_PATH)


def stream_ptr() -> ctypes.c_void_p:
    """Current torch HIP stream as a raw handle."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def tr_probe_maps(device="cuda"):
    """Dump ds_read_b64_tr_b16 lane/elem -> LDS element mappings."""
    import torch
    lib = load()
    lib.tr_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_int, ctypes.c_int]
    results = {}
    for mode in (0, 1, 2, 3):
        out = torch.empty(64, 4, dtype=torch.int16, device=device)
        lib.tr_probe(stream_ptr(), ctypes.c_void_p(out.data_ptr()), 0, mode)
        torch.cuda.synchronize()
        results[mode] = out.to(torch.int32).cpu() & 0xFFFF
    return results
