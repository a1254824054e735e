"""Pins the references of tests/aux_ref.py (what the per-kernel GPU tests of encoders.hip, wav2vec.hip and vae.hip
compare against) on the CPU, each against an independent evaluation: oracle/encoders.py and oracle/vae.py where
they have the op, torch's own bf16 op sequence for the roundings, hand-indexed sums for the convolutions.  Also the
two cap conditions of the GPU tests (share of elements that may differ from the reference), which the reference
must leave room for: an fp32 restatement of the kernel's arithmetic has to meet them with a wide margin, and a
restatement with the rounding the cap is there to catch left out has to miss them."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_ref as R
from oracle import encoders as oenc
from oracle import vae as ovae


def _all_finite_bf16():
    b = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    return b[torch.isfinite(b.float())]


# ------------------------------------------------------------------------------------------------ helpers

def test_rbf_is_round_to_nearest_even_bf16():
    """fp32 -> bf16 is one rounding in torch, so rbf must reproduce it exactly: random values over the whole
    exponent range (subnormals included), every exact tie, and overflow"""
    g = torch.Generator().manual_seed(0)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (200000,), generator=g, dtype=torch.int64).to(torch.int32)
    x = bits.view(torch.float32)
    x = x[torch.isfinite(x)]
    fin = _all_finite_bf16().float()
    ties = ((fin[:-1].double() + R.bf16_step(fin[:-1], 1)) / 2).float()  # midpoints: exact in fp32
    x = torch.cat([x, fin, ties, torch.tensor([3.3961775e38, -3.4e38, 0.0, -0.0, 1e-45])])
    assert torch.equal(R.rbf(x), x.bfloat16().double())
    # and in one rounding from fp64: just above a tie goes up, though fp32 would first round it onto the tie
    assert R.rbf(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)).item() == 1.0 + 2.0 ** -7
    assert R.rbf(torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64)).item() == 1.0


def test_bf16_step_walks_the_grid():
    fin = _all_finite_bf16()
    s = torch.sort(fin.double().unique()).values  # -0 and +0 fold into one
    nz = s != 0
    up = R.bf16_step(s[:-1].bfloat16(), 1)
    dn = R.bf16_step(s[1:].bfloat16(), -1)
    # (stepping off a zero lands on the subnormal of that zero's sign side twice; skip the zero itself)
    assert torch.equal(up[nz[:-1]], s[1:][nz[:-1]])
    assert torch.equal(dn[nz[1:]], s[:-1][nz[1:]])


# ------------------------------------------------------------------------------------------------ umT5

def _t5_norm_inputs(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * 3
    x[:, ::7] *= 20
    w = torch.randn(C, generator=g)
    return x, w


def _t5_norm_kernel_fp32(x, w, eps, inner_rounding=True):
    """sa_t5_rmsnorm's arithmetic in fp32 torch (the sum's order aside)"""
    x = x.float()
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    if inner_rounding:
        n = n.bfloat16().float()
    return (w.bfloat16().float() * n).bfloat16()


@pytest.mark.parametrize("C", [72, 256, 1000, 4096])
@pytest.mark.parametrize("in_bf16", [False, True])
def test_t5_rmsnorm_reference_and_cap(C, in_bf16):
    """reference vs T5LayerNorm.forward's own torch op sequence on a bf16 weight; vs oracle.encoders._t5_norm
    (no roundings: three bf16 roundings apart); and the cap of the GPU test: <= 1 % of the elements of an fp32
    evaluation differ from the fp64 reference (measured <= 0.022 %), while without the inner rounding about a
    quarter do (measured 25.5 .. 26.3 %; asserted > 10 %)"""
    x, w = _t5_norm_inputs(64, C, C)
    if in_bf16:
        x = x.bfloat16()
    ref = R.t5_rmsnorm(x, w, 1e-6)
    # T5LayerNorm.forward, weight in bf16
    wb = w.bfloat16()
    t = x * torch.rsqrt(x.float().pow(2).mean(dim=-1, keepdim=True) + 1e-6)
    t = wb * t.type_as(wb)
    assert t.dtype == torch.bfloat16
    share = (t.double() != ref).double().mean().item()
    print(f"C={C}: torch bf16 sequence differs from the fp64 reference on {share:.5%}")
    assert share <= 0.01
    assert R.within_bf16_ulp(t, ref, 1e-30).all()
    # the oracle on the same bf16 weight: no rounding; n and the product each round by <= 2^-8 relative
    o = oenc._t5_norm(x.double(), wb.double())
    assert ((ref - o).abs() <= o.abs() * 2.1 * 2.0 ** -8).all()
    # cap
    share = (_t5_norm_kernel_fp32(x, w, 1e-6).double() != ref).double().mean().item()
    print(f"C={C}: fp32 restatement differs on {share:.5%}")
    assert share <= 0.01
    share_no = (_t5_norm_kernel_fp32(x, w, 1e-6, inner_rounding=False).double() != ref).double().mean().item()
    print(f"C={C}: without the inner rounding {share_no:.2%}")
    assert share_no > 0.1


def test_t5_rmsnorm_zero_row():
    x, w = _t5_norm_inputs(3, 72, 1)
    x[1] = 0
    assert (R.t5_rmsnorm(x, w, 1e-6)[1] == 0).all()


@pytest.mark.parametrize("use_bucket,use_mask", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_t5_softmax_reference(use_bucket, use_mask):
    """vs T5Attention.forward's torch op sequence in bf16 (attn_bias built in bf16, masked_fill with
    finfo(bf16).min, einsum output + attn_bias in bf16, softmax in fp32), with oracle.encoders' bucket table;
    a fully masked batch row gives uniform 1 / n"""
    b, N, L = 2, 3, 37
    g = torch.Generator().manual_seed(5)
    s = torch.randn(b, N, L, L, generator=g) * 10
    bucket = oenc.t5_relative_bucket(L, L, 32)
    emb = torch.randn(32, N, generator=g).bfloat16()
    mask = torch.ones(b, L, dtype=torch.int32)
    mask[0, 20:] = 0
    mask[1] = 0
    attn_bias = torch.zeros(b, N, L, L, dtype=torch.bfloat16)
    if use_bucket:
        attn_bias += emb[bucket].permute(2, 0, 1).unsqueeze(0)
    if use_mask:
        attn_bias.masked_fill_(mask.view(b, 1, 1, -1) == 0, torch.finfo(torch.bfloat16).min)
    attn = s.bfloat16() + attn_bias
    p_t = F.softmax(attn.float(), dim=-1)
    p, t = R.t5_softmax_bias(s.view(-1, L), b, N, L, bucket if use_bucket else None, emb if use_bucket else None,
                             mask if use_mask else None)
    assert torch.equal(t, attn.double().view(-1, L))
    assert (p - p_t.double().view(-1, L)).abs().max().item() < 1e-6
    if use_mask:
        pm = p.view(b, N, L, L)
        assert (pm[0, :, :, 20:] == 0).all()
        assert torch.allclose(pm[1], torch.full_like(pm[1], 1.0 / L), rtol=1e-12)


def _gelu_kernel_fp32(x):
    """t5_gelu_bf16 of encoders.hip in fp32 torch (fp32 tanh, every step rounded to bf16)"""
    r = lambda v: v.bfloat16().float()  # noqa: E731
    x = x.float()
    half_x = r(0.5 * x)
    x3 = r(x * x * x)
    inner = r(x + r(torch.tensor(0.044715, dtype=torch.float32) * x3))
    th = r(torch.tanh(r(torch.tensor(0.7978845608028654, dtype=torch.float32) * inner)))
    return r(half_x * r(1.0 + th))


def test_t5_gelu_chain_all_bf16_inputs():
    """over all 65 280 finite bf16 inputs: torch's own bf16 op sequence (GELU.forward copied) and the fp32
    restatement of the kernel each leave the reference's centre value on <= 0.1 % of the inputs (measured: 7 and
    0 of 65 280), always inside the neighbour set -- though some of those differ by far more than one ulp of the
    result (up to 100 % of it), since `1 + tanh` cancels: the reason the GPU test uses the neighbour set and no
    ulp bound"""
    x = _all_finite_bf16()
    assert x.numel() == 65280
    one = torch.ones_like(x)
    nb = R.t5_geglu_neighbours(x, one)
    assert not torch.isnan(nb).any()
    t = 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))
    assert t.dtype == torch.bfloat16
    for name, got in (("torch bf16 sequence", t.double()), ("fp32 restatement", _gelu_kernel_fp32(x).double())):
        off = got != nb[1]
        inside = (got[None] == nb).any(0)
        worst = ((got - nb[1]).abs() / nb[1].abs().clamp(min=1e-300))[off].max().item() if off.any() else 0.0
        print(f"{name}: {int(off.sum())} of {x.numel()} off the centre value, worst relative difference {worst:.3g}")
        assert off.double().mean().item() <= 1e-3
        assert inside.all(), x[~inside]
    # the oracle's unrounded GELU: the chain's roundings stay within 2^-5 |x|
    o = oenc._t5_gelu(x.double())
    fin = torch.isfinite(o)  # x^3 overflows fp64 nowhere, but keep the guard
    assert ((nb[1] - o).abs()[fin] <= x.double().abs()[fin] * 2.0 ** -5 + 1e-30).all()


def test_t5_geglu_reference_rounds_the_product():
    """fc1 * GELU(gate) is one more bf16 op: torch's bf16 multiply of fc1 and the chain's value.  (The chain itself
    is pinned above; torch's CPU pow(x, 3.0) on bf16 rounds x * x before the second multiply, which the kernel's
    exact fp32 cube and the reference do not, so gates are not compared through torch's pow here.)"""
    g = torch.Generator().manual_seed(2)
    gate = (torch.randn(1000, generator=g) * 3).bfloat16()
    fc1 = torch.randn(1000, generator=g).bfloat16()
    nb = R.t5_geglu_neighbours(gate, fc1)
    for k in (-1, 0, 1):
        ge = R.t5_gelu_chain(gate, k)
        assert torch.equal(ge.bfloat16().double(), ge)  # a bf16 value
        assert torch.equal((fc1 * ge.bfloat16()).double(), nb[k + 1])
    assert (nb[0] != nb[2]).any()


# ------------------------------------------------------------------------------------------------ CLIP

def _bicubic_taps(img, S, dt):
    """clip_preprocess_kernel's tap formula in numpy at precision dt: A = -0.75, source index
    (o + 0.5) * (in / S) - 0.5, four clamped taps per axis, rows first"""
    img = np.asarray(img, dtype=dt)
    C, H, W = img.shape
    A = dt(-0.75)

    def c1(x):
        return ((A + dt(2)) * x - (A + dt(3))) * x * x + dt(1)

    def c2(x):
        return ((A * x - dt(5) * A) * x + dt(8) * A) * x - dt(4) * A

    def axis(n_in):
        sc = dt(n_in) / dt(S)
        f = (np.arange(S).astype(dt) + dt(0.5)) * sc - dt(0.5)
        i = np.floor(f).astype(np.int64)
        t = (f - i.astype(dt)).astype(dt)
        wts = np.stack([c2(t + dt(1)), c1(t), c1(dt(1) - t), c2(dt(2) - t)]).astype(dt)  # [4, S]
        idx = np.clip(i[None] - 1 + np.arange(4)[:, None], 0, n_in - 1)  # [4, S]
        return wts, idx

    wy, iy = axis(H)
    wx, ix = axis(W)
    acc = np.zeros((C, S, S), dtype=dt)
    for ky in range(4):
        row = np.zeros((C, S, S), dtype=dt)
        for kx in range(4):
            row = row + img[:, iy[ky]][:, :, ix[kx]] * wx[kx][None, None, :]
        acc = acc + row * wy[ky][None, :, None]
    mean = np.asarray(R.CLIP_MEAN, dtype=np.float32).astype(dt)[:, None, None]
    std = np.asarray(R.CLIP_STD, dtype=np.float32).astype(dt)[:, None, None]
    return ((acc * dt(0.5) + dt(0.5)) - mean) / std


@pytest.mark.parametrize("H,W,S", [(20, 36, 14), (9, 7, 14), (14, 14, 14), (30, 52, 28)])
def test_clip_preprocess_reference(H, W, S):
    """F.interpolate(bicubic) in fp64 vs the kernel's tap formula restated in numpy, in fp64 (same function:
    1e-12) and in fp32 (the figure the GPU tolerance is about: printed), and vs oracle.encoders.clip_preprocess
    (fp32 torch).  fp32 bound: the source coordinate (up to 52) carries 2^-24 relative error, i.e. 3e-6 of a pixel,
    times the interpolant's slope (<= ~4 per pixel for taps of |x| <= 1, weights' slopes <= 1.5), / 2 / std
    (0.26) -> < 1e-4"""
    g = torch.Generator().manual_seed(H * 100 + W)
    img = (torch.rand(3, H, W, generator=g) * 2 - 1)
    ref = R.clip_preprocess(img, S)
    t64 = _bicubic_taps(img.numpy(), S, np.float64)
    assert np.abs(t64 - ref.numpy()).max() < 1e-12
    t32 = _bicubic_taps(img.numpy(), S, np.float32)
    e32 = np.abs(t32.astype(np.float64) - ref.numpy()).max()
    eo = (oenc.clip_preprocess(img[:, None], S)[0].double() - ref).abs().max().item()
    print(f"({H},{W})->{S}: fp32 tap formula max abs err {e32:.3g}, fp32 F.interpolate {eo:.3g}")
    assert e32 < 1e-4 and eo < 1e-4
    if (H, W) == (S, S):
        plain = (img.double() * 0.5 + 0.5 - torch.tensor(R.CLIP_MEAN, dtype=torch.float32).double().view(3, 1, 1)) \
            / torch.tensor(R.CLIP_STD, dtype=torch.float32).double().view(3, 1, 1)
        assert (ref - plain).abs().max().item() < 1e-14


@pytest.mark.parametrize("S,P,Kpad", [(28, 14, 592), (42, 14, 640)])
def test_clip_patch_im2col_reference(S, P, Kpad):
    """the indexed rows times a flattened Conv2d weight are the patch convolution (oracle.encoders.clip_visual's
    first line); row 0 and the pad columns are zero"""
    g = torch.Generator().manual_seed(S)
    img = torch.randn(3, S, S, generator=g)
    cols = R.clip_patch_im2col(img, P, Kpad)
    assert cols.shape == (1 + (S // P) ** 2, Kpad) and cols.dtype == torch.bfloat16
    assert (cols[0] == 0).all() and (cols[:, 3 * P * P:] == 0).all()
    w = torch.randn(5, 3, P, P, generator=g, dtype=torch.float64)
    conv = F.conv2d(img.bfloat16().double()[None], w, stride=P).flatten(2).permute(0, 2, 1)[0]
    assert (cols[1:, :3 * P * P].double() @ w.flatten(1).t() - conv).abs().max().item() < 1e-10


# ------------------------------------------------------------------------------------------------ wav2vec2

@pytest.mark.parametrize("T", [1, 7, 300])
def test_w2v_conv0_reference(T):
    """vs a hand-written evaluation: windows by unfold, biased variance over time, 0.5 x (1 + erf(x / sqrt 2))"""
    C, k, stride = 5, 10, 5
    g = torch.Generator().manual_seed(T)
    audio = torch.randn((T - 1) * stride + k + 3, generator=g, dtype=torch.float64) + 50
    w = torch.randn(C, k, generator=g, dtype=torch.float64)
    gw, gb = torch.randn(C, generator=g).double(), torch.randn(C, generator=g).double()
    ref = R.w2v_conv0_gn_gelu(audio, w, stride, gw, gb, 1e-5, T)
    win = audio.unfold(0, k, stride)[:T]  # [T, k]
    y = win @ w.t()  # [T, C]
    y = (y - y.mean(0)) / torch.sqrt(y.var(0, unbiased=False) + 1e-5) * gw + gb
    y = 0.5 * y * (1 + torch.erf(y / math.sqrt(2)))
    assert ref.shape == (T, C)
    assert (ref - y).abs().max().item() < 1e-9
    if T == 1:  # one sample per channel: the normalised value is 0, leaving gelu(bias)
        assert torch.allclose(ref[0], F.gelu(gb), atol=1e-12)


@pytest.mark.parametrize("form", ["feature", "positional"])
def test_conv1d_im2col_reference(form):
    """the gathered rows times the flattened weight are F.conv1d (grouped, padded) of the channel slice"""
    if form == "feature":
        groups, cg, k, stride, pad, T_in, ldx, col0 = 1, 16, 3, 2, 0, 37, 24, 8
        T_out, Kpad = (T_in - k) // stride + 1, k * cg
    else:
        groups, cg, k, stride, pad, T_in, ldx, col0 = 4, 8, 16, 1, 8, 19, 40, 8
        T_out, Kpad = 19, k * cg + 8
    g = torch.Generator().manual_seed(k)
    x = torch.randn(T_in + 2, ldx, generator=g).bfloat16()
    cols = R.conv1d_im2col(x, T_in, col0, groups, cg, k, stride, pad, T_out, Kpad)
    assert cols.shape == (groups, T_out, Kpad) and (cols[:, :, k * cg:] == 0).all()
    cout_g = 3
    w = torch.randn(groups * cout_g, cg, k, generator=g, dtype=torch.float64)
    xs = x[:T_in, col0:col0 + groups * cg].double().t()[None]  # [1, C, T]
    conv = F.conv1d(xs, w, stride=stride, padding=pad, groups=groups)[0][:, :T_out]  # [groups cout_g, T_out]
    for gi in range(groups):
        wg = w[gi * cout_g:(gi + 1) * cout_g].permute(0, 2, 1).reshape(cout_g, k * cg)  # column order (j, c)
        got = cols[gi, :, :k * cg].double() @ wg.t()
        assert (got.t() - conv[gi * cout_g:(gi + 1) * cout_g]).abs().max().item() < 1e-10


def test_add_f32_bf16_reference():
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(7, 100, generator=g), torch.randn(7, 100, generator=g).bfloat16()
    assert torch.equal(R.add_f32_bf16(x, y), x + y.float())


# ------------------------------------------------------------------------------------------------ VAE

@pytest.mark.parametrize("silu", [0, 1])
def test_vae_rmsnorm_silu_reference(silu):
    """vs oracle.vae.rms_norm (channels on dim 1) + torch's SiLU"""
    g = torch.Generator().manual_seed(silu)
    x = torch.randn(37, 32, generator=g, dtype=torch.float64) * 3
    x[4] = 0
    gamma = torch.rand(32, generator=g, dtype=torch.float64) + 0.5
    o = ovae.rms_norm(x.t()[None, :, :, None, None], gamma.view(1, -1, 1, 1, 1))[0, :, :, 0, 0].t()
    o = o * torch.sigmoid(o) if silu else o
    ref = R.vae_rmsnorm_silu(x, gamma, silu)
    assert (ref - o).abs().max().item() < 1e-12
    assert (ref[4] == 0).all()


def test_vae_elementwise_references():
    """input de-normalise / output clamp / latent split vs the expressions of wan_vae.py on [C, T, H, W] tensors"""
    g = torch.Generator().manual_seed(3)
    Cz, Cp, THW, Cs = 16, 32, 77, 36
    mean, std = torch.randn(Cz, generator=g).double(), (torch.rand(Cz, generator=g) + 0.5).double()
    z = torch.randn(Cz, THW, generator=g).double()
    out, mag = R.vae_input(z, mean, std, Cp)
    scale = [mean.view(-1, 1), 1.0 / std.view(-1, 1)]  # decode: z / scale[1] + scale[0] with scale[1] = 1 / std
    assert (out[:, :Cz].t() - (z / scale[1] + scale[0])).abs().max().item() < 1e-12
    assert (out[:, Cz:] == 0).all() and (mag >= out.abs() - 1e-12).all()
    x = torch.randn(THW, Cs, generator=g).double() * 2
    assert torch.equal(R.vae_output(x, 3, 0), x[:, :3].t().clamp_(-1, 1))
    assert torch.equal(R.vae_output(x, 3, 1), (x[:, :3].t().clamp_(-1, 1) / 2 + 0.5).clamp(0, 1))
    assert R.vae_output(x, 3, 1).min().item() == 0.0 and R.vae_output(x, 3, 1).max().item() == 1.0
    lo = R.vae_latent_out(x, Cz, mean, std)
    mu, log_var = x[:, :2 * Cz].t().chunk(2, dim=0)
    mu = (mu - scale[0]) * scale[1]  # encode: (mu - mean) * (1 / std)
    assert (lo - torch.cat([mu, log_var])).abs().max().item() < 1e-12


def test_softmax_and_transpose_references():
    g = torch.Generator().manual_seed(4)
    s = torch.randn(5, 60, generator=g) * 100
    sc = 384 ** -0.5
    p = R.softmax_rows(s, sc)
    e = torch.exp((s.double() - s.double().max(-1, keepdim=True).values) * sc)
    assert (p - e / e.sum(-1, keepdim=True)).abs().max().item() < 1e-14
    x = torch.randn(3, 33, 31, generator=g).bfloat16()
    t = R.transpose_batched(x)
    assert t.shape == (3, 31, 33) and all(t[b, c, r] == x[b, r, c] for b, r, c in [(0, 0, 0), (2, 32, 30), (1, 5, 17)])


def test_down_conv_references():
    """vs tap-by-tap sums indexed as the kernel's comments state them (2h + dh, 2w + dw with the right / bottom
    zero pad; frames 2t .. 2t + 2), with weights packed by the product's own packer from torch-layout weights;
    and vs oracle.vae.resample_down, which chains the two"""
    from stableavatar_amd.vae import _pack_conv
    g = torch.Generator().manual_seed(6)
    T, H, W, cin, cout = 5, 6, 10, 32, 32  # (the oracle's Resample has cin == cout)
    x = torch.randn(T, H, W, cin, generator=g).bfloat16()
    w2 = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    b2 = torch.randn(cout, generator=g)
    pk = _pack_conv(w2, b2)
    wp = pk.w.double().view(-1, 1, 3, 3, cin)
    y = R.conv_down2d(x, pk.w, pk.b, cout)
    assert y.shape == (T, H // 2, W // 2, cout)
    xp = torch.zeros(T, H + 1, W + 1, cin, dtype=torch.float64)
    xp[:, :H, :W] = x.double()
    hand = pk.b.double()[:cout].expand(T, H // 2, W // 2, cout).clone()
    for dh in range(3):
        for dw in range(3):
            hand += xp[:, dh:dh + H:2, dw:dw + W:2][:, :H // 2, :W // 2] @ wp[:cout, 0, dh, dw].t()
    assert (y - hand).abs().max().item() < 1e-10
    # time conv on the (bf16-rounded) result, cin == cout here
    yb = y.bfloat16()
    w3 = torch.randn(cout, cout, 3, 1, 1, generator=g) / (3 * cout) ** 0.5
    b3 = torch.randn(cout, generator=g)
    pk3 = _pack_conv(w3, b3)
    To = (T - 1) // 2
    z = R.conv_down_time(yb, pk3.w, pk3.b, cout)
    assert z.shape == (To, H // 2, W // 2, cout)
    w3p = pk3.w.double().view(-1, 3, cout)
    hand = pk3.b.double()[:cout].expand(To, H // 2, W // 2, cout).clone()
    for dt in range(3):
        hand += yb.double()[dt:dt + 2 * To:2] @ w3p[:cout, dt].t()
    assert (z - hand).abs().max().item() < 1e-10
    # oracle / torch on the torch-layout weights (bf16-rounded, as the packer stores them)
    P = {"q.resample.1.weight": w2.bfloat16().double(), "q.resample.1.bias": b2.double()}
    o = ovae.resample_down(P, "q", x.double().permute(3, 0, 1, 2)[None], False)[0].permute(1, 2, 3, 0)
    assert (y - o).abs().max().item() < 1e-10
    o3 = F.conv3d(yb.double().permute(3, 0, 1, 2)[None], w3.bfloat16().double(), b3.double(),
                  stride=(2, 1, 1))[0].permute(1, 2, 3, 0)
    assert (z - o3).abs().max().item() < 1e-10
