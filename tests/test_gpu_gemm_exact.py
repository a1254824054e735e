"""The GEMM epilogues of csrc/gemm.hip with every element pinned.  Small-integer operands (x, w in [-3, 3], bias in
[-50, 50], K <= 256) make every product and every partial sum exact in fp32 whatever the order, so the only rounding
left is the documented bf16 one and each assertion is torch.equal against a CPU integer reference
(dit_ref.int_gemm / gated_residual, pinned by test_dit_ref_cpu.py): a misplaced element, a bias or gate row taken
from the wrong column or batch row, a residual read through the wrong stride all change integers.  The activation
epilogues get operands that make the pre-activation an exact multiple of 1/8 in [-8, 8] and are held to the rounding
of the activation alone.  Outputs live in larger allocations pre-filled with a sentinel."""
import functools

import pytest
import torch

import aux_ref as A
import dit_ref as R
from stableavatar_amd import ops
from stableavatar_amd._lib import call
from stableavatar_amd.kbench import vt_layout

pytestmark = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")
SENT = 7.5  # not an integer: no exact result equals it

KERNELS = [0, 1, 2, 3, ops.GEMM_S9, ops.GEMM_S9_192]
KERNEL_IDS = ["auto", "pingpong", "persistent", "persistent192", "s9", "s9_192"]
T_KERNELS = [0, 2, 3, ops.GEMM_S9, ops.GEMM_S9_192]  # the transposed epilogues are not on the ping-pong kernel
T_KERNEL_IDS = ["auto", "persistent", "persistent192", "s9", "s9_192"]


def _ks(kernel):
    """K = 192 (no multiple of 128) exists on auto and ping-pong only"""
    return (128, 256, 192) if kernel in (0, 1) else (128, 256)


def _sync():
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    """(x, w, bias, acc = x w^T exactly, in fp32) on the CPU, computed once per shape"""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    x = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-3, 4, (N, K), generator=g).float()
    b = torch.randint(-50, 51, (N,), generator=g).float()
    return x, w, b, x @ w.t()  # integers below 2^24: the fp32 product is exact (test_int_gemm_is_exact_in_fp32)


def _out(M, N, dtype, pad=8):
    """([M, N] view, its [M + 1, N + pad] allocation full of the sentinel)"""
    big = torch.full((M + 1, N + pad), SENT, device=dev, dtype=dtype)
    return big[:M, :N], big


def _pads_kept(big, M, N):
    return bool((big[:M, N:] == SENT).all() and (big[M] == SENT).all())


def _strided(t, dtype=torch.bfloat16, pad=8):
    """t on the GPU as rows of a wider allocation with NaN in the pad"""
    big = torch.full((t.shape[0], t.shape[1] + pad), NAN, device=dev, dtype=dtype)
    big[:, :t.shape[1]] = t.to(dev)
    return big[:, :t.shape[1]]


# ------------------------------------------------------------------------------------------------ EPI_F32 / EPI_BF16

@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("M,N", [(1000, 1536), (777, 640), (513, 520), (4, 8)])
def test_gemm_f32_exact(kernel, M, N):
    """EPI_F32 with and without bias (and EPI_BF16 with, for the kernels test_gemm_bf16_epilogue_exact leaves out),
    every kernel, K = 128 / 256 (+ 192 where it exists): interior tiles, ragged last row and column tiles, a
    matrix smaller than one tile.  x rows strided with NaN in the pad, C rows strided with the sentinel."""
    for K in _ks(kernel):
        x, w, b, acc = _operands(M, N, K)
        xd, wd, bd = _strided(x), w.to(dev).bfloat16(), b.to(dev)
        for bias in (bd, None):
            out, big = _out(M, N, torch.float32)
            ops.linear(xd, wd, bias, ops.EPI_F32, out=out, kernel=kernel)
            _sync()
            assert torch.equal(out.cpu(), acc + b if bias is not None else acc), (K, bias is not None)
            assert _pads_kept(big, M, N), K
        out, big = _out(M, N, torch.bfloat16)
        ops.linear(xd, wd, bd, ops.EPI_BF16, out=out, kernel=kernel)
        _sync()
        assert torch.equal(out.cpu(), (acc + b).bfloat16()), K
        assert _pads_kept(big, M, N), K


# ------------------------------------------------------------------------------------------------ EPI_RES_F32

@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("M,rpb", [(600, 200), (512, 256), (513, 1000)], ids=["rpb200", "rpb256-M512", "rpb>M"])
def test_gemm_gated_residual_exact(kernel, M, rpb):
    """out = res + bf16(acc + bias) * gate[row // rows_per_batch], integer gate in [-2, 2] and residual in [-100,
    100]: exact.  N = 520: two interior 256-column tiles (the accumulator-path epilogue, which takes the gate per
    tile when the tile's rows share a batch row and per row otherwise) and a ragged one (the LDS-strip path).
    rows_per_batch 200 at M = 600 puts a batch boundary inside a 256-row and a 192-row tile and leaves tile 0 of
    the 192-row kernel on the per-tile path; 256 at M = 512 puts it on the 256-row tile edge (per-tile path in
    both tiles) but inside the second 192-row tile; 1000 > M is the single batch row.  Residual aliasing C, and in a
    tensor of its own with ldr != ldc; gate = None; gate rows strided (gate_bstride > N, NaN between)."""
    N = 520
    B = -(-M // rpb)
    for K in _ks(kernel):
        x, w, b, acc = _operands(M, N, K)
        g = torch.Generator().manual_seed(K + rpb)
        res = torch.randint(-100, 101, (M, N), generator=g).float()
        gate = torch.randint(-2, 3, (B, N), generator=g).float()
        xd, wd, bd = _strided(x), w.to(dev).bfloat16(), b.to(dev)
        ref = R.gated_residual(acc + b, res, gate, rpb).float()
        ref1 = R.gated_residual(acc + b, res, None, rpb).float()
        gd = gate.to(dev)
        # the residual aliases C
        out, big = _out(M, N, torch.float32)
        out.copy_(res.to(dev))
        ops.linear(xd, wd, bd, ops.EPI_RES_F32, out=out, residual=out, gate=gd, rows_per_batch=rpb, kernel=kernel)
        _sync()
        assert torch.equal(out.cpu(), ref), (K, "alias")
        assert _pads_kept(big, M, N), K
        # the residual in its own tensor, ldr = N + 16 != ldc = N + 8 (NaN in its pad), strided gate rows
        rd = _strided(res, torch.float32, pad=16)
        gs = _strided(gate, torch.float32, pad=24)
        out, big = _out(M, N, torch.float32)
        ops.linear(xd, wd, bd, ops.EPI_RES_F32, out=out, residual=rd, gate=gs, rows_per_batch=rpb, kernel=kernel)
        _sync()
        assert torch.equal(out.cpu(), ref), (K, "own residual")
        assert torch.equal(rd.cpu(), res), K
        assert _pads_kept(big, M, N), K
        # no gate
        out, big = _out(M, N, torch.float32)
        ops.linear(xd, wd, bd, ops.EPI_RES_F32, out=out, residual=rd, kernel=kernel)
        _sync()
        assert torch.equal(out.cpu(), ref1), (K, "no gate")
        assert _pads_kept(big, M, N), K


# ------------------------------------------------------------------------------------------------ transposed epilogues

@pytest.mark.parametrize("kernel", T_KERNELS, ids=T_KERNEL_IDS)
@pytest.mark.parametrize("M,N", [(1000, 384), (516, 130)])
def test_gemm_transposed_exact(kernel, M, N):
    """EPI_BF16_T: C^T[n, m] = the exact row result bf16(acc + bias)[m, n]; EPI_BF16_TP32: kbench.vt_layout of it
    (the rows of each 32-row chunk in the attention's P order).  The columns past M keep the sentinel -- for P32
    that includes the unwritten positions of a last chunk that M (= 8 or 4 mod 32) leaves partial."""
    for K in (128, 256):
        x, w, b, acc = _operands(M, N, K)
        xd, wd, bd = _strided(x), w.to(dev).bfloat16(), b.to(dev)
        y = (acc + b).bfloat16()
        Rv = (M + 63) // 64 * 64 + 64
        out = torch.full((N + 1, Rv), SENT, device=dev, dtype=torch.bfloat16)
        ops.linear(xd, wd, bd, ops.EPI_BF16_T, out=out[:N], kernel=kernel)
        _sync()
        assert torch.equal(out[:N, :M].t().cpu(), y), K
        assert (out[:N, M:] == SENT).all() and (out[N] == SENT).all(), K
        outp = torch.full((N + 1, Rv), SENT, device=dev, dtype=torch.bfloat16)
        ops.linear(xd, wd, bd, ops.EPI_BF16_TP32, out=outp[:N], kernel=kernel)
        _sync()
        want = vt_layout(y, 3)  # [N, Rv], zeros where no row lands
        written = vt_layout(torch.ones_like(y), 3) == 1
        assert want.shape == (N, Rv)
        assert torch.equal(outp[:N].cpu(), torch.where(written, want, torch.full_like(want, SENT))), K
        assert (outp[N] == SENT).all(), K


# ------------------------------------------------------------------------------------------------ batched

@pytest.mark.parametrize("kernel", [0, 1], ids=["auto", "pingpong"])
def test_gemm_batched_exact(kernel):
    """sa_gemm_bf16_ex with batch = 3 and batch strides larger than the matrices: NaN between the A slabs and
    between the W slabs, the sentinel between the C slabs; EPI_F32 (ops.bmm_nt's epilogue) and EPI_BF16, both with
    a bias (shared by the batch)"""
    Z, M, N, K = 3, 100, 72, 128
    g = torch.Generator().manual_seed(kernel)
    a = torch.randint(-3, 4, (Z, M, K), generator=g).float()
    w = torch.randint(-3, 4, (Z, N, K), generator=g).float()
    b = torch.randint(-50, 51, (N,), generator=g).float()
    ref = R.int_gemm(a, w, b)
    lda, ldw, ldc = K + 8, K + 16, N + 8
    sA, sW, sC = M * lda + 64, N * ldw + 128, M * ldc + 32
    ab = torch.full((Z * sA,), NAN, device=dev, dtype=torch.bfloat16)
    wb = torch.full((Z * sW,), NAN, device=dev, dtype=torch.bfloat16)
    for z in range(Z):
        ab[z * sA:z * sA + M * lda].view(M, lda)[:, :K] = a[z].to(dev)
        wb[z * sW:z * sW + N * ldw].view(N, ldw)[:, :K] = w[z].to(dev)
    bd = b.to(dev)
    for epi, dt in ((ops.EPI_F32, torch.float32), (ops.EPI_BF16, torch.bfloat16)):
        cb = torch.full((Z * sC,), SENT, device=dev, dtype=dt)
        call("sa_gemm_bf16_ex", ab.data_ptr(), lda, sA, wb.data_ptr(), ldw, sW, bd.data_ptr(), cb.data_ptr(), ldc, sC,
             M, N, K, Z, epi, 0, 0, 0, 0, 0, 0, kernel, 0, ops._stream())
        _sync()
        slabs = cb.view(Z, sC)
        got = slabs[:, :M * ldc].view(Z, M, ldc)
        assert torch.equal(got[:, :, :N].double().cpu(), ref if epi == ops.EPI_F32 else A.rbf(ref)), epi
        assert (got[:, :, N:] == SENT).all() and (slabs[:, M * ldc:] == SENT).all(), epi
    # the same through ops.bmm_nt (strided 3-D views, no bias)
    av = ab.view(Z, sA)[:, :M * lda].view(Z, M, lda)[:, :, :K]
    wv = wb.view(Z, sW)[:, :N * ldw].view(Z, N, ldw)[:, :, :K]
    cb = torch.full((Z * sC,), SENT, device=dev)
    cv = cb.view(Z, sC)[:, :M * ldc].view(Z, M, ldc)[:, :, :N]
    ops.bmm_nt(av, wv, cv, kernel=kernel)
    _sync()
    assert torch.equal(cv.double().cpu(), R.int_gemm(a, w))
    assert (cb.view(Z, sC)[:, M * ldc:] == SENT).all()


# ------------------------------------------------------------------------------------------------ activations

def _act_operands(M, N, K, seed):
    """x in {-1, 0, 1}, w in {-1, 0, 1} / 8, bias in multiples of 1/8 in [-1, 1]: the pre-activation is an exact
    multiple of 1/8.  The first 8 rows of x are one +-1 pattern s and column n < 130 of w is +-s / 8 on its first
    n % 65 entries (bias 0), so those outputs are +-(n % 65) / 8: every point of the grid in [-8, 8]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (M, K), generator=g).float()
    w = torch.randint(-1, 2, (N, K), generator=g).float() / 8
    b = torch.randint(-8, 9, (N,), generator=g).float() / 8
    s = torch.randint(0, 2, (K,), generator=g).float() * 2 - 1
    x[:8] = s
    for n in range(min(N, 130)):
        c = min(n % 65, K)
        w[n] = 0
        w[n, :c] = s[:c] / 8 * (1 if n < 65 else -1)
        b[n] = 0
    pre = R.int_gemm(x, w, b)
    assert pre.abs().max() <= 8 and torch.equal(pre * 8, torch.round(pre * 8))
    return x, w, b, pre


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("M,N", [(513, 520), (300, 256)])
def test_gemm_activations(kernel, M, N):
    """the activation epilogues on pre-activations that are exact multiples of 1/8 in [-8, 8] (exact in bf16, so
    the rounding the bf16-output epilogues apply before the activation changes nothing), all 129 grid points
    present.  GELU(tanh) -> bf16: one bf16 ulp (2^-7 |ref|, + 1e-30: nothing absolute) and at most 1 % of the
    elements off the once-rounded reference (an fp32 evaluation: none, test_dit_ref_cpu.py).  GELU(erf) -> bf16:
    2^-7 |ref| + 2^-23 |x| -- `1 + erf` cancels for x < -3, so no relative bound holds there, and no share cap
    either (a correct fp32 evaluation is off on 23 % of a uniform grid).  SiLU -> fp32: relative 2^-20.
    Measured on the MI355X: GELU(tanh) off the reference on no element, GELU(erf) on at most 0.27 %, SiLU's worst
    relative error 4.13e-07 = 0.43 of the bound."""
    for K in ((64, 128) if kernel in (0, 1) else (128,)):
        x, w, b, pre = _act_operands(M, N, K, K + M)
        assert len(torch.unique(pre)) == 129
        xd, wd, bd = _strided(x), w.to(dev).bfloat16(), b.to(dev)
        out, big = _out(M, N, torch.bfloat16)
        ops.linear(xd, wd, bd, ops.EPI_GELU_TANH_BF16, out=out, kernel=kernel)
        _sync()
        ref, got = A.rbf(R.gelu_tanh(pre)), out.double().cpu()
        share = (got != ref).double().mean().item()
        print(f"K={K} GELU(tanh): {share:.4%} of the elements differ from the reference")
        assert A.within_bf16_ulp(got, ref, 1e-30).all(), K
        assert share <= 0.01, K
        assert _pads_kept(big, M, N), K
        out, big = _out(M, N, torch.bfloat16)
        ops.linear(xd, wd, bd, ops.EPI_GELU_ERF_BF16, out=out, kernel=kernel)
        _sync()
        ref, got = A.rbf(R.gelu_erf(pre)), out.double().cpu()
        print(f"K={K} GELU(erf): {(got != ref).double().mean().item():.4%} of the elements differ from the reference")
        assert ((got - ref).abs() <= 2.0 ** -7 * ref.abs() + 2.0 ** -23 * pre.abs()).all(), K
        assert _pads_kept(big, M, N), K
        out, big = _out(M, N, torch.float32)
        ops.linear(xd, wd, bd, ops.EPI_SILU_F32, out=out, kernel=kernel)
        _sync()
        ref, got = R.silu(pre), out.double().cpu()
        print(f"K={K} SiLU: worst relative error {((got - ref).abs() / ref.abs().clamp(min=1e-300)).max().item():.3g}")
        assert ((got - ref).abs() <= 2.0 ** -20 * ref.abs()).all(), K
        assert _pads_kept(big, M, N), K
