"""Weight-only fp8 for the decode GEMVs: quantise once, offline, into the
layout the kernel streams (hip/ops.hip gemv_fp8_kernel).

Values are OCP e4m3fn with one fp32 scale per output row, and the scale is
a power of two, 2**ceil(log2(amax_row / 448)). e4m3 has 3 mantissa bits and
bf16 has 7, so q * scale is a bf16 value: the dequantised weight can be
written back into the bf16 module exactly, and the bf16 and fp8 routes then
compute the same model.

Packed layout (uint8), tile-major:
    [M/16 tiles][K/64 k-blocks][64 lanes][16 bytes]
lane l of a k-block holds row (l % 16), k = block * 64 + (l // 16) * 16 +
0..15: a wave-wide 16-byte load is one contiguous KB, and a lane's bytes are
its A operands of two 16x16x32 MFMAs. A gate|up weight [2F, K] is packed as
[F/16][2][K/64][64][16], gate tile t next to up tile t.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

E4M3_MAX = 448.0


def _pack(q: torch.Tensor) -> torch.Tensor:
    """[M, K] uint8 -> [M/16, K/64, 64, 16] in the kernel's lane order."""
    M, K = q.shape
    # row = tile*16 + r, k = blk*64 + kg*16 + i  ->  [tile, blk, kg, r, i]
    t = q.reshape(M // 16, 16, K // 64, 4, 16).permute(0, 2, 3, 1, 4)
    return t.reshape(M // 16, K // 64, 64, 16)


def _unpack(p: torch.Tensor) -> torch.Tensor:
    """Inverse of _pack: [T, K/64, 64, 16] -> [T*16, K]."""
    T, B = p.shape[:2]
    t = p.reshape(T, B, 4, 16, 16).permute(0, 3, 1, 2, 4)
    return t.reshape(T * 16, B * 64)


@dataclass
class Fp8Weight:
    packed: torch.Tensor          # uint8, the kernel's layout
    scale: torch.Tensor           # [M] fp32 powers of two
    M: int
    K: int
    gate_up: bool = False         # [2F, K] gate|up, tiles interleaved

    def to(self, device) -> "Fp8Weight":
        return Fp8Weight(self.packed.to(device), self.scale.to(device),
                         self.M, self.K, self.gate_up)

    def dequant(self) -> torch.Tensor:
        """The row-major [M, K] fp32 values the kernel multiplies by."""
        p = self.packed
        if self.gate_up:
            q = torch.cat([_unpack(p[:, 0]), _unpack(p[:, 1])], dim=0)
        else:
            q = _unpack(p)
        q = q.contiguous().view(torch.float8_e4m3fn).float()
        return q * self.scale[:, None].to(q.device)


@dataclass
class Fp8ExpertTables:
    """What the routed fp8 GEMVs (hip/ops.hip gemv_moe_fp8_kernel) read for
    one weight of every expert of an MoE layer: device int64 [E] tables of
    the experts' packed bytes and of their scales. The Fp8Weights are held
    here so that the pointers stay valid as long as the tables do."""
    experts: List[Fp8Weight]
    w: torch.Tensor               # int64 [E]: packed.data_ptr()
    s: torch.Tensor               # int64 [E]: scale.data_ptr()
    M: int
    K: int
    gate_up: bool


def expert_tables(experts: List[Fp8Weight]) -> Fp8ExpertTables:
    """Tables over same-shaped Fp8Weights living on one device."""
    e0 = experts[0]
    assert all((e.M, e.K, e.gate_up) == (e0.M, e0.K, e0.gate_up)
               and e.packed.device == e0.packed.device
               and e.packed.is_contiguous() and e.scale.is_contiguous()
               for e in experts)
    dev = e0.packed.device
    w = torch.tensor([e.packed.data_ptr() for e in experts],
                     dtype=torch.int64, device=dev)
    s = torch.tensor([e.scale.data_ptr() for e in experts],
                     dtype=torch.int64, device=dev)
    return Fp8ExpertTables(list(experts), w, s, e0.M, e0.K, e0.gate_up)


def quantize_rows(weight: torch.Tensor,
                  gate_up: bool = False) -> Optional[Fp8Weight]:
    """[M, K] bf16 or fp32 weight -> Fp8Weight, or None for a shape the
    kernel does not take (M % 16, K % 512; a gate|up weight needs F % 16)."""
    if weight.dim() != 2:
        return None
    M, K = weight.shape
    if M == 0 or K == 0 or K % 512 != 0 or M % (32 if gate_up else 16) != 0:
        return None
    w = weight.detach().float()
    amax = w.abs().amax(dim=1)
    # 2**ceil(log2(amax / 448)) from the exponent, with no rounding of a log
    mant, exp = torch.frexp(amax / E4M3_MAX)          # v = mant * 2**exp
    exp = torch.where(mant == 0.5, exp - 1, exp)
    scale = torch.ldexp(torch.ones_like(amax), exp)
    scale = torch.where(amax > 0, scale, torch.ones_like(scale))
    q = (w / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX)
    q = q.to(torch.float8_e4m3fn).view(torch.uint8)
    if gate_up:
        F = M // 2
        packed = torch.stack([_pack(q[:F]), _pack(q[F:])], dim=1)
    else:
        packed = _pack(q)
    return Fp8Weight(packed.contiguous(), scale.contiguous(), M, K, gate_up)
