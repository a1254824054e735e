"""The kernels of csrc/vae.hip that test_gpu_vae_conv_dma.py leaves out, each on its own through the C ABI against
the references of tests/aux_ref.py (pinned on the CPU by test_aux_ref_cpu.py) or, for sa_conv3d_cl, that file's
fp32 torch _ref: the register-staged conv with a ragged last M tile, the two down convs, the generic RMS_norm +
SiLU kernel, the row softmax, the batched transpose and the input / output / latent layout kernels.  Outputs are
written into larger, pre-filled allocations, and inputs carry NaN where the kernel must not read."""
import os

import pytest
import torch

import aux_ref as R
from stableavatar_amd import ops
from stableavatar_amd._lib import KernelError, call
from test_gpu_vae_conv_dma import CASES, _ref

pytestmark = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")
TAIL = 256


def _sync():
    torch.cuda.synchronize()


def _nan_tail(t, pad=4):
    """t's values followed by `pad` leading-dim slices of NaN in the same allocation (as _nan_tail of
    test_gpu_kernels.py)"""
    big = torch.full((t.shape[0] + pad, *t.shape[1:]), NAN, device=dev, dtype=t.dtype)
    big[:t.shape[0]] = t.to(dev)
    return big[:t.shape[0]]


# ------------------------------------------------------------------------------------------------ sa_conv3d_cl

def _conv_tail(x, T, H, W, cin, w, b, cout, cout_pad, k, dma, residual, upsample, out_f32, interleave, prev):
    """sa_conv3d_cl into an allocation with TAIL sentinel elements behind the output; returns (output, tail)"""
    kt, kh, kw = k
    shape = (2 * T, H, W, interleave) if interleave else (T, H, W, cout)
    n = shape[0] * shape[1] * shape[2] * shape[3]
    buf = torch.full((n + TAIL,), 7.0, device=dev, dtype=torch.float32 if out_f32 else torch.bfloat16)
    os.environ["SA_CONV_DMA"] = str(dma)
    try:
        call("sa_conv3d_cl", x.data_ptr(), T, H, W, cin, int(upsample), w.data_ptr(), b.data_ptr(), cout, cout_pad,
             kt, kh, kw, 0 if residual is None else residual.data_ptr(), buf.data_ptr(), int(out_f32), interleave,
             0 if prev is None else prev.data_ptr(), ops._stream())
    finally:
        os.environ.pop("SA_CONV_DMA", None)
    _sync()
    return buf[:n].view(shape), buf[n:]


@pytest.mark.parametrize("H,W", [(6, 10), (10, 12)])
@pytest.mark.parametrize("case", range(8))
def test_conv3d_register_staged_ragged_tile(case, H, W):
    """every option row of test_gpu_vae_conv_dma.CASES (prev, residual, upsample, out_f32, interleave, 1x1, Cout
    4 / 96 / 192 / 384) where H W % 128 != 0, so the last 128-row M tile is ragged (and a tile spans frames): the
    launcher must take the register-staged kernel whatever SA_CONV_DMA says (0 and 2 bit-identical), rel-L2 < 1e-2
    against the fp32 torch conv, nothing written behind the output.  (The real 480 x 832 clip's lowest resolution,
    60 x 104, is such a size.)"""
    T, _, _, cin, cout, k, o = CASES[case]
    assert (H * W) % 128 and (T * H * W) % 128 and T <= 3
    g = torch.Generator(device=dev).manual_seed(100 + case)
    up = o.get("upsample", False)
    Hin, Win = (H // 2, W // 2) if up else (H, W)
    cout_pad = 16 if cout <= 16 else (192 * ((cout + 191) // 192) if cout > 96 else 96)
    kvol = k[0] * k[1] * k[2]
    x = _nan_tail(torch.randn(T, Hin, Win, cin, device=dev, generator=g).bfloat16(), 1)
    w = (torch.randn(cout_pad, kvol * cin, device=dev, generator=g) / (kvol * cin) ** 0.5).bfloat16()
    b = torch.randn(cout_pad, device=dev, generator=g)
    prev = torch.randn(k[0] - 1, Hin, Win, cin, device=dev, generator=g).bfloat16() if o.get("prev") else None
    il = o.get("interleave", 0)
    res = torch.randn(T, H, W, cout, device=dev, generator=g).bfloat16() if o.get("residual") else None
    kw = dict(residual=res, upsample=up, out_f32=o.get("out_f32", False), interleave=il, prev=prev)
    y0, tail0 = _conv_tail(x, T, H, W, cin, w, b, cout, cout_pad, k, 0, **kw)
    y2, tail2 = _conv_tail(x, T, H, W, cin, w, b, cout, cout_pad, k, 2, **kw)
    assert torch.equal(y0, y2)
    assert (tail0 == 7.0).all() and (tail2 == 7.0).all()
    ref = _ref(x, T, H, W, cin, w, b, cout, k, residual=res, upsample=up, interleave=il, prev=prev)
    err = ((y0.float() - ref).norm() / ref.norm()).item()
    assert err < 1e-2, err


# ------------------------------------------------------------------------------------------------ sa_conv3d_cl_down

def _down(x, T_out, H_in, W_in, cin, mode, w, b, cout, cout_pad, shape):
    n = shape[0] * shape[1] * shape[2] * shape[3]
    buf = torch.full((n + TAIL,), 7.0, device=dev, dtype=torch.bfloat16)
    call("sa_conv3d_cl_down", x.data_ptr(), T_out, H_in, W_in, cin, mode, w.data_ptr(), b.data_ptr(), cout, cout_pad,
         buf.data_ptr(), ops._stream())
    _sync()
    assert (buf[n:] == 7.0).all()
    return buf[:n].view(shape)


def _down_weights(cout, K, g):
    cout_pad = 192 * ((cout + 191) // 192) if cout > 96 else 96
    w = (torch.randn(cout_pad, K, generator=g) / K ** 0.5).bfloat16()
    b = torch.randn(cout_pad, generator=g)
    return w, b, cout_pad


@pytest.mark.parametrize("T,H_in,W_in,cin,cout", [(2, 12, 20, 96, 96), (1, 16, 16, 96, 192), (2, 6, 10, 192, 384)])
def test_conv_down2d(T, H_in, W_in, cin, cout):
    """mode 1, Resample 'downsample*': ZeroPad2d((0, 1, 0, 1)) + 3x3 stride-2 conv per frame, against F.pad +
    F.conv2d: the pad row / column must read as zero, not as the next row, the next frame or (last frame) the NaN
    behind the input"""
    g = torch.Generator().manual_seed(H_in * W_in + cout)
    x = torch.randn(T, H_in, W_in, cin, generator=g).bfloat16()
    w, b, cout_pad = _down_weights(cout, 9 * cin, g)
    y = _down(_nan_tail(x, 1), T, H_in, W_in, cin, 1, w.to(dev), b.to(dev), cout, cout_pad,
              (T, H_in // 2, W_in // 2, cout))
    ref = R.conv_down2d(x, w, b, cout)
    assert torch.isfinite(y.float()).all()
    err = R.rel(y, ref)
    assert err < 1e-2, err


@pytest.mark.parametrize("T_out,H,W,C", [(2, 6, 10, 192), (3, 8, 16, 96)])
def test_conv_down_time(T_out, H, W, C):
    """mode 2, the (3, 1, 1) stride-2 time_conv without padding: output frame t reads input frames 2t .. 2t + 2
    of the 2 T_out + 1 given, against F.conv3d"""
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(2 * T_out + 1, H, W, C, generator=g).bfloat16()
    w, b, cout_pad = _down_weights(C, 3 * C, g)
    y = _down(_nan_tail(x, 1), T_out, H, W, C, 2, w.to(dev), b.to(dev), C, cout_pad, (T_out, H, W, C))
    ref = R.conv_down_time(x, w, b, C)
    assert torch.isfinite(y.float()).all()
    err = R.rel(y, ref)
    assert err < 1e-2, err


def test_conv_down_rejects():
    x = torch.zeros(2, 12, 20, 96, device=dev, dtype=torch.bfloat16)
    w = torch.zeros(96, 9 * 96, device=dev, dtype=torch.bfloat16)
    b = torch.zeros(96, device=dev)
    y = torch.zeros(2 * 12 * 20 * 96, device=dev, dtype=torch.bfloat16)
    for T_out, H_in, W_in, mode in [(2, 11, 20, 1), (2, 12, 19, 1), (2, 12, 20, 3), (2, 12, 20, 0), (0, 12, 20, 1)]:
        with pytest.raises(KernelError, match="bad argument"):
            call("sa_conv3d_cl_down", x.data_ptr(), T_out, H_in, W_in, 96, mode, w.data_ptr(), b.data_ptr(), 96, 96,
                 y.data_ptr(), ops._stream())
    _sync()


# ------------------------------------------------------------------------------------------------ sa_vae_rmsnorm_silu

@pytest.mark.parametrize("C", [8, 32, 128, 256, 512])
@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("silu", [0, 1])
def test_rmsnorm_silu_generic(C, rows, silu):
    """rmsnorm_silu_kernel<16 / 32 / 64> (C outside 96 / 192 / 384: 1, 4 and 16 of 16 lanes, 32 of 32, 64 of 64
    holding channels) with a row count that leaves a partial workgroup, against F.normalize * sqrt(C) * gamma
    (+ SiLU) in fp64: rel-L2 < 1e-2 and within one bf16 ulp (2^-7 |ref| + 1e-6); an all-zero row gives zeros"""
    g = torch.Generator().manual_seed(C + rows + silu)
    x = (torch.randn(rows, C, generator=g) * 3).bfloat16()
    if rows > 5:
        x[5] = 0
    gamma = torch.rand(C, generator=g) + 0.5
    xd = _nan_tail(x, 1)
    y = torch.full((rows + 1, C), 7.0, device=dev, dtype=torch.bfloat16)
    gd = gamma.to(dev)
    call("sa_vae_rmsnorm_silu", xd.data_ptr(), y.data_ptr(), gd.data_ptr(), rows, C, silu, ops._stream())
    _sync()
    ref = R.vae_rmsnorm_silu(x, gamma, silu)
    got = y[:rows].double().cpu()
    assert R.rel(got, ref) < 1e-2
    assert R.within_bf16_ulp(got, ref, 1e-6).all()
    if rows > 5:
        assert (got[5] == 0).all()
    assert (y[rows] == 7.0).all()


# ------------------------------------------------------------------------------------------------ sa_softmax_rows

@pytest.mark.parametrize("rows,n,ld_p", [(5, 60, 64), (3, 256, 256), (2, 1000, 1024)])
@pytest.mark.parametrize("scale", [384 ** -0.5, 1.0])
def test_softmax_rows(rows, n, ld_p, scale):
    """softmax(scale * s) with scale * s reaching +-40, within one bf16 ulp of fp64 (2^-7 |ref|, + 1e-36: where
    fp32 flushes its subnormals); the pad columns n .. ld_p, which the attention block zeroes once and then relies
    on, stay zero; strided input with NaN in its pad"""
    g = torch.Generator().manual_seed(n)
    s = torch.randn(rows, n, generator=g)
    s = s / s.abs().max() * (40.0 / scale)
    ld_s = n + 4
    sb = torch.full((rows, ld_s), NAN, device=dev)
    sb[:, :n] = s.to(dev)
    p = torch.zeros(rows + 1, ld_p, device=dev, dtype=torch.bfloat16)
    p[rows] = 7.0
    call("sa_softmax_rows", sb.data_ptr(), ld_s, p.data_ptr(), ld_p, rows, n, scale, ops._stream())
    _sync()
    ref = R.softmax_rows(s, float(torch.tensor(scale, dtype=torch.float32)))
    got = p[:rows, :n].double().cpu()
    assert torch.isfinite(got).all()
    assert R.within_bf16_ulp(got, ref, 1e-36).all()
    assert (p[:rows, n:] == 0).all() and (p[rows] == 7.0).all()


# ------------------------------------------------------------------------------------------------ sa_transpose_bf16

@pytest.mark.parametrize("rows,cols,batch", [(33, 31, 3), (64, 96, 1), (1, 5, 2)])
def test_transpose_bf16(rows, cols, batch):
    """exact; the input is the last column third of a wider tensor (V out of q | k | v, as the attention block
    passes it) whose other columns are NaN; ld_out > rows with the sentinel between the rows intact"""
    g = torch.Generator().manual_seed(rows)
    v = torch.randn(batch, rows, cols, generator=g).bfloat16()
    qkv = torch.full((batch, rows, 3 * cols), NAN, device=dev, dtype=torch.bfloat16)
    qkv[:, :, 2 * cols:] = v.to(dev)
    vin = qkv[:, :, 2 * cols:]
    ld_out = rows + 3
    out = torch.full((batch * cols * ld_out + TAIL,), 7.0, device=dev, dtype=torch.bfloat16)
    call("sa_transpose_bf16", vin.data_ptr(), vin.stride(1), vin.stride(0), out.data_ptr(), ld_out, cols * ld_out,
         rows, cols, batch, ops._stream())
    _sync()
    o = out[:batch * cols * ld_out].view(batch, cols, ld_out)
    assert torch.equal(o[:, :, :rows].cpu().view(torch.int16), R.transpose_batched(v).view(torch.int16))
    assert (o[:, :, rows:] == 7.0).all() and (out[batch * cols * ld_out:] == 7.0).all()


# ------------------------------------------------------------------------------------------------ layout kernels

THW, CZ, CP, CS = 77, 16, 32, 36


def _mean_std(g):
    return torch.randn(CZ, generator=g), torch.rand(CZ, generator=g) + 0.5


def test_vae_input():
    """z * std + mean -> channels-last bf16, the channels past Cz zero: the bf16 rounding of the fp64 value, where
    the fp64 value may move by the fp32 roundings of the product and the sum (2^-23 (|z std| + |mean|))"""
    g = torch.Generator().manual_seed(11)
    z = torch.randn(CZ, THW, generator=g)
    mean, std = _mean_std(g)
    out = torch.full((THW * CP + TAIL,), 7.0, device=dev, dtype=torch.bfloat16)
    zd, md, sd = z.to(dev), mean.to(dev), std.to(dev)
    call("sa_vae_input", zd.data_ptr(), CZ, THW, md.data_ptr(), sd.data_ptr(), out.data_ptr(), CP, ops._stream())
    _sync()
    ref, mag = R.vae_input(z, mean, std, CP)
    got = out[:THW * CP].view(THW, CP).double().cpu()
    e = mag * 2.0 ** -23
    assert ((R.rbf(ref - e) <= got) & (got <= R.rbf(ref + e))).all()
    assert (got[:, CZ:] == 0).all()
    assert (out[THW * CP:] == 7.0).all()


@pytest.mark.parametrize("post", [0, 1])
def test_vae_output(post):
    """channels-last fp32 (stride 36, the columns past C NaN) -> [3, THW], clamp(-1, 1) exactly; with post,
    / 2 + 0.5 is one fp32 rounding of a value in [0, 1]: within 2^-24"""
    g = torch.Generator().manual_seed(12)
    x = torch.randn(THW, CS, generator=g) * 2  # beyond +-1
    x[:, 3:] = NAN
    out = torch.full((3 * THW + TAIL,), 7.0, device=dev)
    xd = x.to(dev)
    call("sa_vae_output", xd.data_ptr(), CS, 3, THW, out.data_ptr(), post, ops._stream())
    _sync()
    ref = R.vae_output(x, 3, post)
    got = out[:3 * THW].view(3, THW).double().cpu()
    assert (x[:, :3].abs() > 1).any()
    if post:
        assert (got - ref).abs().max().item() <= 2.0 ** -24
        assert got.min().item() == 0.0 and got.max().item() == 1.0
    else:
        assert torch.equal(got, ref)
    assert (out[3 * THW:] == 7.0).all()


def test_vae_latent_out():
    """channels-last fp32 [THW][36] (mu | log_var | 4 NaN columns) -> [32][THW]: (mu - mean) * (1 / std) to fp32
    rounding (the reciprocal, the difference and the product: 3 * 2^-24 < 1e-6 relative), log_var exactly"""
    g = torch.Generator().manual_seed(13)
    x = torch.randn(THW, CS, generator=g)
    x[:, 2 * CZ:] = NAN
    mean, std = _mean_std(g)
    out = torch.full((2 * CZ * THW + TAIL,), 7.0, device=dev)
    xd, md, sd = x.to(dev), mean.to(dev), std.to(dev)
    call("sa_vae_latent_out", xd.data_ptr(), CS, CZ, THW, md.data_ptr(), sd.data_ptr(), out.data_ptr(), ops._stream())
    _sync()
    ref = R.vae_latent_out(x, CZ, mean, std)
    got = out[:2 * CZ * THW].view(2 * CZ, THW).double().cpu()
    assert ((got[:CZ] - ref[:CZ]).abs() <= ref[:CZ].abs() * 1e-6).all()
    assert torch.equal(got[CZ:], ref[CZ:])
    assert (out[2 * CZ * THW:] == 7.0).all()


# ------------------------------------------------------------------------------------------------ argument checks

def test_empty_sizes_are_bad_arguments():
    """rows, THW or a dimension <= 0 used to reach the launch with an empty grid (a launch failure, or a silent
    no-op) instead of SA_ERR_ARG; C = 520 / 20 of the RMS_norm were rejected before.  Every call here is refused
    by the launcher's argument check: none launches."""
    f = torch.zeros(64 * 36, device=dev)
    h = torch.zeros(64 * 36, device=dev, dtype=torch.bfloat16)
    st = ops._stream()
    bad = [
        ("sa_vae_rmsnorm_silu", (h.data_ptr(), h.data_ptr(), f.data_ptr(), 0, 32, 1, st)),
        ("sa_vae_rmsnorm_silu", (h.data_ptr(), h.data_ptr(), f.data_ptr(), -3, 32, 1, st)),
        ("sa_vae_rmsnorm_silu", (h.data_ptr(), h.data_ptr(), f.data_ptr(), 4, 0, 1, st)),
        ("sa_vae_rmsnorm_silu", (h.data_ptr(), h.data_ptr(), f.data_ptr(), 4, 520, 1, st)),
        ("sa_vae_rmsnorm_silu", (h.data_ptr(), h.data_ptr(), f.data_ptr(), 4, 20, 1, st)),
        ("sa_vae_input", (f.data_ptr(), 16, 0, f.data_ptr(), f.data_ptr(), h.data_ptr(), 32, st)),
        ("sa_vae_input", (f.data_ptr(), 0, 8, f.data_ptr(), f.data_ptr(), h.data_ptr(), 32, st)),
        ("sa_vae_input", (f.data_ptr(), 16, 8, f.data_ptr(), f.data_ptr(), h.data_ptr(), 8, st)),
        ("sa_vae_output", (f.data_ptr(), 4, 3, 0, f.data_ptr(), 0, st)),
        ("sa_vae_output", (f.data_ptr(), 4, 0, 8, f.data_ptr(), 0, st)),
        ("sa_vae_output", (f.data_ptr(), 2, 3, 8, f.data_ptr(), 0, st)),
        ("sa_vae_latent_out", (f.data_ptr(), 36, 16, 0, f.data_ptr(), f.data_ptr(), f.data_ptr(), st)),
        ("sa_vae_latent_out", (f.data_ptr(), 36, 0, 8, f.data_ptr(), f.data_ptr(), f.data_ptr(), st)),
        ("sa_vae_latent_out", (f.data_ptr(), 30, 16, 8, f.data_ptr(), f.data_ptr(), f.data_ptr(), st)),
        ("sa_transpose_bf16", (h.data_ptr(), 8, 64, h.data_ptr(), 8, 64, 0, 8, 1, st)),
        ("sa_transpose_bf16", (h.data_ptr(), 8, 64, h.data_ptr(), 8, 64, 8, 0, 1, st)),
        ("sa_transpose_bf16", (h.data_ptr(), 8, 64, h.data_ptr(), 8, 64, 8, 8, 0, st)),
        ("sa_softmax_rows", (f.data_ptr(), 8, h.data_ptr(), 8, 0, 8, 1.0, st)),
    ]
    for name, args in bad:
        with pytest.raises(KernelError, match="bad argument"):
            call(name, *args)
    _sync()
