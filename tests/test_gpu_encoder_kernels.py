"""Every entry point of csrc/encoders.hip on its own against the fp64 references of tests/aux_ref.py (pinned on
the CPU by test_aux_ref_cpu.py), through the C ABI, at the shapes and argument combinations the encoders never
pass: bf16 input of the T5 norm, batch > 1 / no bucket / no mask / ragged and maximal n of the T5 softmax, every
bf16 gate of the GEGLU, clamped taps / H != W / up- and down-scaling / identity of the CLIP resize.  Outputs are
written into larger, pre-filled allocations, and strided inputs carry NaN where the kernel must not read."""
import pytest
import torch
import torch.nn.functional as F

import aux_ref as R
from stableavatar_amd import ops
from stableavatar_amd._lib import KernelError, call

pytestmark = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ sa_t5_rmsnorm

@pytest.mark.parametrize("M,C", [(5, 72), (3, 256), (4, 1000), (2, 4096)])
@pytest.mark.parametrize("in_f32", [0, 1], ids=["bf16in", "f32in"])
def test_t5_rmsnorm(M, C, in_f32):
    """bf16(bf16(w) * bf16(x * rsqrt(mean(x^2) + eps))): every element within one bf16 ulp of the fp64 reference
    (the project's bound, 2^-7 |ref| + 1e-6) and at most 1 % of the elements different at all -- an fp32
    evaluation differs on <= 0.03 %, one without the inner rounding on a quarter (test_aux_ref_cpu.py; the kernel
    on the MI355X: on none at these shapes).  Strided input (NaN in the pad) and output (sentinel in the pad), one
    all-zero row."""
    g = torch.Generator().manual_seed(C + in_f32)
    x = torch.randn(M, C, generator=g) * 3
    x[:, ::7] *= 20
    x[1] = 0
    w = torch.randn(C, generator=g).to(dev)
    ldx, ldy = C + 8, C + 24
    xin = torch.full((M, ldx), NAN, device=dev, dtype=torch.float32 if in_f32 else torch.bfloat16)
    xin[:, :C] = x.to(dev)
    y = torch.full((M + 1, ldy), 7.0, device=dev, dtype=torch.bfloat16)
    call("sa_t5_rmsnorm", xin.data_ptr(), ldx, in_f32, y.data_ptr(), ldy, w.data_ptr(), M, C, 1e-6, ops._stream())
    _sync()
    ref = R.t5_rmsnorm(xin[:, :C], w, 1e-6)
    got = y[:M, :C].double().cpu()
    share = (got != ref).double().mean().item()
    print(f"in_f32={in_f32} M={M} C={C}: {share:.4%} of the elements differ from the reference")
    assert R.within_bf16_ulp(got, ref, 1e-6).all()
    assert share <= 0.01
    assert (got[1] == 0).all()
    assert (y[:M, C:] == 7.0).all() and (y[M] == 7.0).all()


# ------------------------------------------------------------------------------------------------ sa_t5_softmax_bias

def _softmax_case(batch, heads, rph, n, seed):
    g = torch.Generator().manual_seed(seed)
    rows = batch * heads * rph
    s = torch.randn(rows, n, generator=g) * 10  # unscaled T5 logits: about +-30
    bucket = torch.randint(0, 32, (rph, n), generator=g, dtype=torch.int32)
    emb = torch.randn(32, heads, generator=g).bfloat16()
    mask = (torch.rand(batch, n, generator=g) < 0.7).to(torch.int32)  # a different mask per batch row
    mask[:, 1] = 1
    if batch == 2 and n == 257:
        mask[1] = 0  # a fully masked batch row: uniform 1 / n
    return s, bucket, emb, mask


@pytest.mark.parametrize("batch,heads,rph,n", [(2, 3, 5, 100), (1, 2, 4, 256), (2, 2, 3, 257), (1, 1, 2, 2048)])
@pytest.mark.parametrize("use_bucket", [1, 0], ids=["bucket", "nobucket"])
@pytest.mark.parametrize("use_mask", [1, 0], ids=["mask", "nomask"])
def test_t5_softmax_bias(batch, heads, rph, n, use_bucket, use_mask):
    """P = softmax(bf16(bf16(s) + bias)) within one bf16 ulp of the fp64 reference (2^-7 |ref|, + 1e-36: where
    fp32 flushes its subnormals); masked keys exactly 0 in a row that has a valid key, a fully masked batch row
    uniform; per-batch masks (batch 2: the second row's mask is what tells b apart); n ragged against the 64-lane
    wave and the 256-thread block, and at the LDS array's limit; ld_s, ld_p > n with the pad of P untouched"""
    s, bucket, emb, mask = _softmax_case(batch, heads, rph, n, n + batch)
    rows = batch * heads * rph
    ld_s, ld_p = n + 3, n + 5
    sb = torch.full((rows, ld_s), NAN, device=dev)
    sb[:, :n] = s.to(dev)
    p = torch.full((rows + 1, ld_p), 7.0, device=dev, dtype=torch.bfloat16)
    bk, em, mk = bucket.to(dev), emb.to(dev), mask.to(dev)
    call("sa_t5_softmax_bias", sb.data_ptr(), ld_s, p.data_ptr(), ld_p, batch, heads, rph, n,
         bk.data_ptr() if use_bucket else 0, em.data_ptr() if use_bucket else 0, mk.data_ptr() if use_mask else 0,
         ops._stream())
    _sync()
    ref, _ = R.t5_softmax_bias(s, batch, heads, rph, bucket if use_bucket else None, emb if use_bucket else None,
                               mask if use_mask else None)
    got = p[:rows, :n].double().cpu()
    assert torch.isfinite(got).all()
    assert R.within_bf16_ulp(got, ref, 1e-36).all()
    if use_mask:
        g4 = got.view(batch, heads, rph, n)
        for b in range(batch):
            if mask[b].any():
                assert (g4[b][:, :, mask[b] == 0] == 0).all()
            else:
                assert R.within_bf16_ulp(g4[b], torch.full_like(g4[b], 1.0 / n), 0).all()
    assert (p[:rows, n:] == 7.0).all() and (p[rows] == 7.0).all()


def test_t5_softmax_bias_rejects():
    """n past the LDS row buffer (2048), and a bucket table without its embedding or the reverse"""
    s = torch.zeros(2, 2049, device=dev)
    p = torch.zeros(2, 2049, device=dev, dtype=torch.bfloat16)
    bk = torch.zeros(1, 2049, device=dev, dtype=torch.int32)
    em = torch.zeros(32, 2, device=dev, dtype=torch.bfloat16)
    st = ops._stream()
    with pytest.raises(KernelError, match="bad argument"):
        call("sa_t5_softmax_bias", s.data_ptr(), 2049, p.data_ptr(), 2049, 1, 2, 1, 2049, 0, 0, 0, st)
    with pytest.raises(KernelError, match="bad argument"):
        call("sa_t5_softmax_bias", s.data_ptr(), 2049, p.data_ptr(), 2049, 1, 2, 1, 64, bk.data_ptr(), 0, 0, st)
    with pytest.raises(KernelError, match="bad argument"):
        call("sa_t5_softmax_bias", s.data_ptr(), 2049, p.data_ptr(), 2049, 1, 2, 1, 64, 0, em.data_ptr(), 0, st)
    _sync()


# ------------------------------------------------------------------------------------------------ sa_t5_geglu

@pytest.mark.parametrize("fc1_kind", ["random", "ones"])
def test_t5_geglu_every_bf16_gate(fc1_kind):
    """the gate half holds all 65 280 finite bf16 bit patterns (M = 255, N = 256, ld_in = 2 N + 8): every output
    is a member of the reference's neighbour set (the bf16 tanh value moved by -1 / 0 / +1 place before the rest
    of the chain of bf16 ops -- `1 + tanh` cancels, so no ulp bound on the output holds), at most 0.1 % differ
    from its centre value, none is NaN"""
    M, N = 255, 256
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    gate = bits[torch.isfinite(bits.float())].view(M, N)
    g = torch.Generator().manual_seed(7)
    fc1 = torch.randn(M, N, generator=g).bfloat16() if fc1_kind == "random" else torch.ones(M, N).bfloat16()
    ld_in, ld_out = 2 * N + 8, N + 8
    inp = torch.full((M, ld_in), NAN, device=dev, dtype=torch.bfloat16)
    inp[:, :N] = gate.to(dev)
    inp[:, N:2 * N] = fc1.to(dev)
    out = torch.full((M + 1, ld_out), 7.0, device=dev, dtype=torch.bfloat16)
    call("sa_t5_geglu", inp.data_ptr(), ld_in, out.data_ptr(), ld_out, M, N, ops._stream())
    _sync()
    got = out[:M, :N].double().cpu()
    nb = R.t5_geglu_neighbours(gate, fc1)
    assert not torch.isnan(got).any()
    inside = (got[None] == nb).any(0)
    off = (got != nb[1]).double().mean().item()
    print(f"fc1 {fc1_kind}: {int((got != nb[1]).sum())} of {M * N} outputs off the centre value")
    assert inside.all(), gate[~inside]
    assert off <= 1e-3
    assert (out[:M, N:] == 7.0).all() and (out[M] == 7.0).all()


# ------------------------------------------------------------------------------------------------ sa_clip_preprocess

def _clip_run(img, S):
    C, H, W = img.shape
    buf = torch.full((C * H * W + 512,), NAN, device=dev)  # NaN before and after the planes
    src = buf[256:256 + C * H * W]
    src.copy_(img.to(dev).flatten())
    out = torch.full((C * S * S + 64,), NAN, device=dev)
    mean, std = torch.tensor(R.CLIP_MEAN, device=dev), torch.tensor(R.CLIP_STD, device=dev)
    call("sa_clip_preprocess", src.data_ptr(), C, H, W, out.data_ptr(), S, mean.data_ptr(), std.data_ptr(),
         ops._stream())
    _sync()
    assert torch.isnan(out[C * S * S:]).all()
    return out[:C * S * S].view(C, S, S).double().cpu()


@pytest.mark.parametrize("H,W,S", [(20, 36, 14), (9, 7, 14), (30, 52, 28)])
def test_clip_preprocess_resize(H, W, S):
    """down-scaling, up-scaling (clamped taps over most of the image) and H != W against F.interpolate(bicubic) in
    fp64.  The bound is measured, not fixed: torch's own fp32 F.interpolate pipeline on the GPU at the same input
    against the same reference, times 4 (the kernel sums its taps in another order).  Both are printed.  Measured on
    the MI355X, max abs error at outputs of magnitude ~2.5, kernel / torch fp32: (20, 36) -> 14: 3.81e-06 /
    3.81e-06; (9, 7) -> 14: 1.21e-06 / 1.09e-06; (30, 52) -> 28: 1.15e-05 / 1.15e-05 (the fp32 source coordinate
    dominates both)."""
    g = torch.Generator().manual_seed(H * 100 + W)
    img = torch.rand(3, H, W, generator=g) * 2 - 1
    ref = R.clip_preprocess(img, S)
    got = _clip_run(img, S)
    x = F.interpolate(img.to(dev)[None], size=(S, S), mode="bicubic", align_corners=False)[0]
    x = x * 0.5 + 0.5
    x = (x - torch.tensor(R.CLIP_MEAN, device=dev).view(3, 1, 1)) / torch.tensor(R.CLIP_STD, device=dev).view(3, 1, 1)
    e_torch = (x.double().cpu() - ref).abs().max().item()
    e_kernel = (got - ref).abs().max().item()
    print(f"({H},{W})->{S}: kernel max abs err {e_kernel:.3g}, torch fp32 {e_torch:.3g}")
    assert torch.isfinite(got).all()
    assert e_kernel <= 4 * e_torch


def test_clip_preprocess_identity():
    """S == H == W: the taps' weights are exactly (0, 1, 0, 0), so the output is (x * 0.5 + 0.5 - mean) / std to
    fp32 rounding: three roundings (the scale-and-shift, the subtraction, the division) of 2^-24 relative each on
    intermediates <= 1 in magnitude, divided by std >= 0.26, and the result <= 2.7: 2^-24 (1 + 1) / 0.26 + 2^-24
    2.7 < 11 * 2^-24 = 6.6e-07 (measured on the MI355X: 1.57e-07)"""
    S = 14
    g = torch.Generator().manual_seed(14)
    img = torch.rand(3, S, S, generator=g) * 2 - 1
    got = _clip_run(img, S)
    m = torch.tensor(R.CLIP_MEAN, dtype=torch.float32).double().view(3, 1, 1)
    s = torch.tensor(R.CLIP_STD, dtype=torch.float32).double().view(3, 1, 1)
    plain = (img.double() * 0.5 + 0.5 - m) / s
    e = (got - plain).abs().max().item()
    print(f"identity: max abs err {e:.3g}")
    assert e <= 11 * 2.0 ** -24
    assert (got - R.clip_preprocess(img, S)).abs().max().item() <= 11 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ sa_clip_patch_im2col

@pytest.mark.parametrize("S,P,Kpad", [(28, 14, 592), (42, 14, 640)])
def test_clip_patch_im2col(S, P, Kpad):
    """exactly the indexed reference: row 1 + py g + px, column (c, ky, kx); row 0 and the pad columns zero"""
    C = 3
    g = torch.Generator().manual_seed(S)
    img = torch.randn(C, S, S, generator=g)
    n = 1 + (S // P) ** 2
    cols = torch.full((n * Kpad + 64,), 7.0, device=dev, dtype=torch.bfloat16)
    im = img.to(dev)
    call("sa_clip_patch_im2col", im.data_ptr(), C, S, P, cols.data_ptr(), Kpad, ops._stream())
    _sync()
    got = cols[:n * Kpad].view(n, Kpad).cpu()
    assert torch.equal(got.view(torch.int16), R.clip_patch_im2col(img, P, Kpad).view(torch.int16))
    assert (got[0] == 0).all() and (got[:, C * P * P:] == 0).all()
    assert (cols[n * Kpad:] == 7.0).all()


def test_clip_patch_im2col_rejects():
    im = torch.zeros(3, 28, 28, device=dev)
    cols = torch.zeros(5, 592, device=dev, dtype=torch.bfloat16)
    with pytest.raises(KernelError, match="bad argument"):  # S % P
        call("sa_clip_patch_im2col", im.data_ptr(), 3, 27, 14, cols.data_ptr(), 592, ops._stream())
    with pytest.raises(KernelError, match="bad argument"):  # Kpad < C P P
        call("sa_clip_patch_im2col", im.data_ptr(), 3, 28, 14, cols.data_ptr(), 584, ops._stream())
    _sync()


# ------------------------------------------------------------------------------------------------ sa_cast_bf16_f32

def test_cast_bf16_f32():
    n = 1000
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(n, generator=g) * 100).bfloat16().to(dev)
    out = torch.full((n + 24,), 7.0, device=dev)
    call("sa_cast_bf16_f32", x.data_ptr(), out.data_ptr(), n, ops._stream())
    _sync()
    assert torch.equal(out[:n], x.float())
    assert (out[n:] == 7.0).all()
