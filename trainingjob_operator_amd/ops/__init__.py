"""MI355X-native op library: CDNA4 HIP kernels + autograd wrappers.

GPU path: hand-written gfx950 kernels in hip/ops.hip (bf16x8 vectorized,
wave64 reductions), loaded from the in-tree libhipops.so. CPU path: the
fp32 PyTorch reference (reference.py). The two are cross-checked by the
numerics tests in tests/test_ops_gpu.py.
"""
from .functional import (
    apply_rope,
    decode_attention,
    decode_attention_paged,
    decode_attention_paged_fp8,
    decode_linear,
    decode_linear_fp8,
    decode_moe_fp8,
    decode_moe_swiglu_fp8,
    decode_swiglu,
    decode_swiglu_fp8,
    fused_cross_entropy,
    fused_rmsnorm,
    dispatch_rows,
    gather_rows,
    make_inv_freq,
    moe_combine,
    prefill_attention_paged,
    prefill_work,
    rope_cache_paged,
    rope_cache_paged_fp8,
    rope_cache_paged_rows,
    swiglu,
    swiglu_packed,
    verify_attention_paged,
)
from .native import HipOpsUnavailable, available, build_ops, load

__all__ = [
    "apply_rope",
    "decode_attention",
    "decode_attention_paged",
    "decode_attention_paged_fp8",
    "decode_linear",
    "decode_linear_fp8",
    "decode_moe_fp8",
    "decode_moe_swiglu_fp8",
    "decode_swiglu",
    "decode_swiglu_fp8",
    "dispatch_rows",
    "gather_rows",
    "moe_combine",
    "fused_cross_entropy",
    "fused_rmsnorm",
    "make_inv_freq",
    "prefill_attention_paged",
    "prefill_work",
    "rope_cache_paged",
    "rope_cache_paged_fp8",
    "rope_cache_paged_rows",
    "swiglu",
    "verify_attention_paged",
    "available",
    "build_ops",
    "load",
    "HipOpsUnavailable",
]
