"""Weight-only MXFP4 for the decode GEMVs: quantise once, offline, into the
layout the kernel streams (hip/ops.hip gemv_mx4_kernel).

OCP MXFP4: e2m1 values (0, 0.5, 1, 1.5, 2, 3, 4, 6 with a sign; code = sign
<< 3 | index into that list) and one e8m0 scale byte b, 2**(b - 127), per
(row, 32 consecutive k): 4.25 bits per weight. The scale is
2**ceil(log2(amax_block / 6)), so nothing saturates; an all-zero block gets
scale 1; the exponent is floored at -125 so that the smallest nonzero
product, 0.5 * scale, is a normal bf16 and fp32, and byte 255 never occurs.
Rounding is to nearest, ties to the even code. e2m1 has one mantissa bit and
bf16 has 7, so q * scale is a bf16 value: the dequantised weight can be
written back into the bf16 module exactly, and the bf16 and MXFP4 routes
then compute the same model.

Packed values (uint8, two per byte, the low nibble is the even k),
tile-major:
    [M/16 tiles][K/128 k-blocks][64 lanes][16 bytes]
lane l of a k-block holds row (l % 16), k = block * 128 + (l // 16) * 32 +
0..31: a wave-wide 16-byte load is one contiguous KB, a lane's 16 bytes are
exactly one MX block (one scale for its 16 conversions), and its four words
are the A operands of four 16x16x32 MFMAs.
Scale bytes, one dword per lane per 512-wide chunk:
    [M/16 tiles][K/512 chunks][64 lanes][4 bytes]
byte i of lane l is the scale of row (l % 16) at k = chunk * 512 + i * 128 +
(l // 16) * 32, the block that lane loads from k-block 4 * chunk + i.
A gate|up weight [2F, K] is packed as [F/16][2][...] in both images, gate
tile t next to up tile t.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E2M1_MAX = 6.0
MX_BLOCK = 32
MIN_EXP = -125                  # 0.5 * 2**-125 is the smallest normal


def _pack(b: torch.Tensor) -> torch.Tensor:
    """[M, K/2] value bytes -> [M/16, K/128, 64, 16] in the lane order."""
    M, K2 = b.shape
    # row = tile*16 + r, byte = blk*64 + kg*16 + i  ->  [tile, blk, kg, r, i]
    t = b.reshape(M // 16, 16, K2 // 64, 4, 16).permute(0, 2, 3, 1, 4)
    return t.reshape(M // 16, K2 // 64, 64, 16)


def _unpack(p: torch.Tensor) -> torch.Tensor:
    """Inverse of _pack: [T, K/128, 64, 16] -> [T*16, K/2]."""
    T, B = p.shape[:2]
    t = p.reshape(T, B, 4, 16, 16).permute(0, 3, 1, 2, 4)
    return t.reshape(T * 16, B * 64)


def _pack_scale(s: torch.Tensor) -> torch.Tensor:
    """[M, K/32] scale bytes -> [M/16, K/512, 64, 4] in the lane order."""
    M, B = s.shape
    # row = tile*16 + r, block = c*16 + i*4 + kg  ->  [tile, c, kg, r, i]
    t = s.reshape(M // 16, 16, B // 16, 4, 4).permute(0, 2, 4, 1, 3)
    return t.reshape(M // 16, B // 16, 64, 4)


def _unpack_scale(p: torch.Tensor) -> torch.Tensor:
    """Inverse of _pack_scale: [T, K/512, 64, 4] -> [T*16, K/32]."""
    T, C = p.shape[:2]
    t = p.reshape(T, C, 4, 16, 4).permute(0, 3, 1, 4, 2)
    return t.reshape(T * 16, C * 16)


@dataclass
class Mx4Weight:
    packed: torch.Tensor          # uint8 e2m1 pairs, the kernel's layout
    scale: torch.Tensor           # uint8 e8m0, the kernel's lane-major image
    M: int
    K: int
    gate_up: bool = False         # [2F, K] gate|up, tiles interleaved

    def to(self, device) -> "Mx4Weight":
        return Mx4Weight(self.packed.to(device), self.scale.to(device),
                         self.M, self.K, self.gate_up)

    def scales(self) -> torch.Tensor:
        """Row-major [M, K/32] fp32 block scales."""
        s = self.scale
        if self.gate_up:
            s = torch.cat([_unpack_scale(s[:, 0]), _unpack_scale(s[:, 1])])
        else:
            s = _unpack_scale(s)
        return torch.ldexp(torch.ones(s.shape, device=s.device),
                           s.to(torch.int32) - 127)

    def dequant(self) -> torch.Tensor:
        """The row-major [M, K] fp32 values the kernel multiplies by."""
        p = self.packed
        if self.gate_up:
            b = torch.cat([_unpack(p[:, 0]), _unpack(p[:, 1])], dim=0)
        else:
            b = _unpack(p)
        code = torch.stack([b & 15, b >> 4], dim=-1).reshape(self.M, self.K)
        grid = torch.tensor(E2M1_GRID, device=b.device)
        q = grid[(code & 7).long()]
        q = torch.where(code >= 8, -q, q)
        return q * self.scales().repeat_interleave(MX_BLOCK, dim=1)


@dataclass
class Mx4ExpertTables:
    """What the routed MXFP4 GEMVs (hip/ops.hip gemv_moe_mx4_kernel) read for
    one weight of every expert of an MoE layer: device int64 [E] tables of
    the experts' packed values and of their scale images. The Mx4Weights are
    held here so that the pointers stay valid as long as the tables do."""
    experts: List[Mx4Weight]
    w: torch.Tensor               # int64 [E]: packed.data_ptr()
    s: torch.Tensor               # int64 [E]: scale.data_ptr()
    M: int
    K: int
    gate_up: bool


def mx4_expert_tables(experts: List[Mx4Weight]) -> Mx4ExpertTables:
    """Tables over same-shaped Mx4Weights living on one device."""
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
    return Mx4ExpertTables(list(experts), w, s, e0.M, e0.K, e0.gate_up)


def quantize_mx4(weight: torch.Tensor,
                 gate_up: bool = False) -> Optional[Mx4Weight]:
    """[M, K] bf16 or fp32 weight -> Mx4Weight, or None for a shape the
    kernel does not take (M % 16, K % 512; a gate|up weight needs F % 16)."""
    if weight.dim() != 2:
        return None
    M, K = weight.shape
    if M == 0 or K == 0 or K % 512 != 0 or M % (32 if gate_up else 16) != 0:
        return None
    w = weight.detach().float().reshape(M, K // MX_BLOCK, MX_BLOCK)
    amax = w.abs().amax(dim=2)
    # ceil(log2(amax / 6)) from the exponent, with no division and no log:
    # amax = m * 2**e with m in [0.5, 1), and amax / 6 = (m / 0.75) * 2**(e-3)
    mant, exp = torch.frexp(amax)
    exp = torch.where(mant > 0.75, exp - 2, exp - 3)
    exp = torch.where(amax > 0, exp, torch.zeros_like(exp)).clamp(MIN_EXP, 127)
    v = torch.ldexp(w.abs(), -exp[:, :, None]).clamp(max=E2M1_MAX)
    # nearest grid value, ties to the even code: the grid's step is 0.5 below
    # 2, 1 below 4 and 2 above, and torch.round is half-to-even
    step = torch.where(v < 2, 0.5, torch.where(v < 4, 1.0, 2.0))
    q = torch.round(v / step) * step
    code = torch.where(q < 2, q * 2, torch.where(q < 4, q + 2, q / 2 + 4))
    code = code.to(torch.uint8) | (((w < 0) & (q > 0)).to(torch.uint8) << 3)
    code = code.reshape(M, K)
    b = code[:, 0::2] | (code[:, 1::2] << 4)
    s = (exp + 127).to(torch.uint8)
    if gate_up:
        F = M // 2
        packed = torch.stack([_pack(b[:F]), _pack(b[F:])], dim=1)
        scale = torch.stack([_pack_scale(s[:F]), _pack_scale(s[F:])], dim=1)
    else:
        packed, scale = _pack(b), _pack_scale(s)
    return Mx4Weight(packed.contiguous(), scale.contiguous(), M, K, gate_up)
