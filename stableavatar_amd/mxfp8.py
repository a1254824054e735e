"""MXFP8 as the fp8 FFN mode uses it -- the definition the HIP kernels (csrc/mxfp8.h) match bit for bit.

Blocks of 32 consecutive elements along the last (K) dimension; elements are OCP `e4m3fn` bytes; one E8M0 scale byte
`s` per block, the block's values being `2^(s - 127) * element`.  Quantising a block with absolute maximum `amax`:
`e` = the smallest integer with `amax * 2^-e <= 448` (0 for an all-zero block), `s = clamp(e + 127, 0, 254)`, each
element `RNE(x * 2^-e)`: the scaling is exact and nothing saturates.  NaN / Inf are out of contract.
Plain torch, runs on the CPU.
"""
from __future__ import annotations

import torch

BLOCK = 32
E4M3_MAX = 448.0


def block_exponent(amax: torch.Tensor) -> torch.Tensor:
    """e (int32) per block for fp32 `amax` >= 0: minimal with amax * 2^-e <= 448; 0 where amax == 0."""
    amax = amax.float()
    # frexp: amax = m * 2^x, m in [0.5, 1); 448 = 0.875 * 2^9, so e = x - 9, one more where m > 0.875.  Exact at
    # every power of two (no log2 rounding): amax = 448 * 2^j -> j, amax = 256 * 2^j -> j.
    m, x = torch.frexp(amax)
    e = x.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)
    return torch.where(amax == 0, torch.zeros_like(e), e)


def quantize(x: torch.Tensor):
    """x [..., K] (bf16 or fp32, K % 32 == 0) -> (q uint8 [..., K] e4m3fn bit patterns, s uint8 [..., K / 32])."""
    K = x.shape[-1]
    if K % BLOCK:
        raise ValueError(f"mxfp8.quantize: K = {K} is not a multiple of {BLOCK}")
    xb = x.float().reshape(*x.shape[:-1], K // BLOCK, BLOCK)
    e = block_exponent(xb.abs().amax(-1))
    s = (e + 127).clamp(0, 254)
    inv = torch.ldexp(torch.ones((), dtype=torch.float32), 127 - s)  # 2^-e for the stored (clamped) scale
    q = (xb * inv.unsqueeze(-1)).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.reshape(x.shape), s.to(torch.uint8)


def dequantize(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """(q uint8 [..., K], s uint8 [..., K / 32]) -> fp32 [..., K] (exact)."""
    K = q.shape[-1]
    v = q.contiguous().view(torch.float8_e4m3fn).float().reshape(*q.shape[:-1], K // BLOCK, BLOCK)
    scale = torch.ldexp(torch.ones((), dtype=torch.float32), s.to(torch.int32) - 127)
    return (v * scale.unsqueeze(-1)).reshape(q.shape)


def fake_quant(x: torch.Tensor) -> torch.Tensor:
    """dequantize(quantize(x)) in fp32: what an MXFP8 GEMM operand stands for."""
    return dequantize(*quantize(x))
