"""MXFP8 without a GPU: the format's definition (stableavatar_amd/mxfp8.py), the C ABI's argument checks, and the CPU
oracle with the FFN Linears emulated in MXFP8 against the plain oracle (the reason the fp8 mode starts at the FFN)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from mxfp8_util import cos, rel, small_case  # noqa: E402

from stableavatar_amd import _lib, mxfp8  # noqa: E402


def _blocks(seed=0, rows=64, nblk=12):
    """bf16 [rows, nblk * 32]: block magnitudes 2^-20 .. 2^10, both signs, every eighth member 2^-14 .. 2^-17 of its
    block's size (e4m3 subnormals and underflow once scaled)"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.randint(-20, 11, (rows, nblk), generator=g).float())
    x = torch.randn(rows, nblk * 32, generator=g) * mag.repeat_interleave(32, 1)
    x[:, 3::8] *= torch.exp2(-torch.randint(14, 18, (rows, nblk * 4), generator=g).float())
    return x.bfloat16()


def _e(s):
    return s.to(torch.int32) - 127


def test_scale_is_minimal():
    x = _blocks()
    _, s = mxfp8.quantize(x)
    amax = x.float().reshape(64, -1, 32).abs().amax(-1).double()
    assert (amax > 0).all()
    e = _e(s).double()
    assert (amax * torch.exp2(-e) <= 448).all()
    assert (amax * torch.exp2(-(e - 1)) > 448).all()


@pytest.mark.parametrize("top,byte", [(448.0, 0x7E), (256.0, 0x78)])
def test_amax_at_exact_powers(top, byte):
    """amax = 448 * 2^j and 256 * 2^j: e = j exactly (no log2 rounding), the top element lands on `top`"""
    js = list(range(-20, 11))
    x = torch.zeros(len(js), 32)
    for i, j in enumerate(js):
        x[i, i % 32] = -top * 2.0 ** j if i % 2 else top * 2.0 ** j
        x[i, (i + 1) % 32] = 0.3 * 2.0 ** j
    q, s = mxfp8.quantize(x.bfloat16())
    assert _e(s)[:, 0].tolist() == js
    for i in range(len(js)):
        assert (q[i, i % 32] & 0x7F) == byte and (q[i, i % 32] >> 7) == i % 2


def test_zero_block_and_grid_round_trip():
    x = torch.zeros(4, 64).bfloat16()
    q, s = mxfp8.quantize(x)
    assert (s == 127).all() and (q == 0).all()
    # every finite e4m3 value at several scales, the block's maximum pinned to 448 so that e is the chosen one
    codes = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8)
    vals = codes.view(torch.float8_e4m3fn).float()
    vals = torch.cat([vals, torch.full((256 - len(vals),), 448.0)]).reshape(8, 32)
    vals[:, 0] = 448.0
    for j in (-9, 0, 5):
        xb = (vals * 2.0 ** j).bfloat16()
        assert torch.equal(xb.float(), vals * 2.0 ** j)  # 4 significant bits: exact in bf16
        q, s = mxfp8.quantize(xb)
        assert (_e(s) == j).all()
        assert torch.equal(mxfp8.dequantize(q, s), xb.float())


def test_error_is_at_most_half_a_step():
    x = _blocks(seed=1)
    q, s = mxfp8.quantize(x)
    d = mxfp8.dequantize(q, s).double().reshape(64, -1, 32)
    xs = x.double().reshape(64, -1, 32)
    scale = torch.exp2(_e(s).double()).unsqueeze(-1)
    # e4m3 step at the scaled magnitude: 2^(floor(log2 |v|) - 3), 2^-9 in the subnormal range
    v = (xs / scale).abs()
    ex = torch.floor(torch.log2(v.clamp_min(2.0 ** -6))).clamp_min(-6)
    step = torch.exp2(ex - 3)
    assert ((d - xs).abs() <= 0.5 * step * scale).all()
    assert (v > 0).logical_and(v < 2.0 ** -6).any()  # the subnormal range is exercised


def test_abi_rejects_bad_arguments_without_gpu_work():
    """every check precedes the first HIP call: rc 1 with no device"""
    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    L = _lib.lib()
    one = 256  # a non-null, 16-byte aligned host address: rejected before it is dereferenced

    def gemm(A=one, As=one, W=one, Ws=one, C=one, Cs=one, M=64, N=64, K=128, epi=2, res=None):
        return L.sa_gemm_mxfp8(A, K, As, K // 32 if K >= 32 else 4, W, K, Ws, K // 32 if K >= 32 else 4, None, C, N, Cs,
                               N // 32 if N >= 32 else 1, M, N, K, epi, res, N, None, 0, 0, None)

    assert gemm(A=None) == 1 and gemm(As=None) == 1 and gemm(W=None) == 1 and gemm(Ws=None) == 1 and gemm(C=None) == 1
    assert gemm(K=192) == 1                    # K % 128
    assert gemm(epi=8, N=48) == 1              # SA_EPI_GELU_TANH_MXFP8 with N % 32 != 0
    assert gemm(epi=8, Cs=None) == 1
    assert gemm(epi=3) == 1                    # gated residual without a residual
    for epi in (4, 5, 6, 7, 9, -1):            # epilogues of sa_gemm_bf16 this kernel does not have, unknown codes
        assert gemm(epi=epi) == 1
    assert L.sa_mxfp8_quant(None, 64, one, 64, one, 2, 4, 64, None) == 1
    assert L.sa_mxfp8_quant(one, 64, None, 64, one, 2, 4, 64, None) == 1
    assert L.sa_mxfp8_quant(one, 64, one, 64, None, 2, 4, 64, None) == 1
    assert L.sa_mxfp8_quant(one, 48, one, 48, one, 2, 4, 48, None) == 1            # K % 32
    assert L.sa_layernorm_mod_mxfp8(None, 64, 0, one, 64, one, 2, None, None, None, None, 0, 0, 4, 64, 1e-6, None) == 1
    assert L.sa_layernorm_mod_mxfp8(one, 64, 0, one, 64, None, 2, None, None, None, None, 0, 0, 4, 64, 1e-6, None) == 1
    assert L.sa_layernorm_mod_mxfp8(one, 48, 0, one, 48, one, 2, None, None, None, None, 0, 0, 4, 48, 1e-6, None) == 1
    assert L.sa_layernorm_mod_mxfp8(one, 64, 2, one, 64, one, 2, None, None, None, None, 0, 0, 4, 64, 1e-6, None) == 1


@pytest.mark.parametrize("case", ["full", "short", "wide"])
def test_oracle_ffn_in_mxfp8_stays_inside_the_bf16_bar(case):
    """the site choice: quantising only the FFN Linears' operands moves the oracle's output by less than the
    project's bf16 bar (measured 0.70e-2 / 0.99998 on 'full')"""
    _, _, plain = small_case(case, False)
    _, _, emu = small_case(case, True)
    r, c = rel(emu, plain), cos(emu, plain)
    print(f"DIT_SMALL {case}: FFN in MXFP8 vs plain oracle rel-L2 {r:.3e} cosine {c:.6f}")
    assert r > 0  # the patch took effect
    assert r < 2e-2 and c > 0.9995, (r, c)
