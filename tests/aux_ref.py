"""Shared by the per-kernel tests of encoders.hip, wav2vec.hip and the lower half of vae.hip: one plain fp64 (or
exact integer-indexing) torch function per operation, restating the reference's arithmetic with its bf16 roundings
where it has them.  They run on the CPU; tests/test_aux_ref_cpu.py pins each against an independent evaluation."""
import math

import torch
import torch.nn.functional as F

BF16_MIN = float(torch.finfo(torch.bfloat16).min)
BF16_MAX = float(torch.finfo(torch.bfloat16).max)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def f64(x):
    return torch.as_tensor(x).detach().cpu().double()


def rbf(x):
    """fp64 -> nearest bf16 value (ties to even) -> fp64, in one rounding (torch's own double -> bfloat16 cast goes
    through fp32 and rounds twice).  bf16: 8 significant bits, normal exponents down to 2^-126, subnormals below."""
    x = f64(x)
    _, e = torch.frexp(x)  # |x| = m 2^e, m in [0.5, 1)
    q = torch.ldexp(torch.ones_like(x), e.clamp(min=-125) - 8)
    y = torch.round(x / q) * q  # torch.round: half to even; x / q and the product are exact (q a power of two)
    y = torch.where(y.abs() > BF16_MAX, torch.copysign(torch.full_like(y, math.inf), x), y)
    return torch.where(torch.isfinite(x), y, x)


def bf16_step(x, k):
    """the bf16 value k places above (k > 0) or below x on the bf16 grid; x holds bf16 values (any float dtype)"""
    b = torch.as_tensor(x).detach().cpu().to(torch.bfloat16).view(torch.int16).to(torch.int32)
    o = torch.where(b >= 0, b, -(b & 0x7FFF)) + k  # sign-magnitude -> ordered
    b = torch.where(o >= 0, o, (-o) | 0x8000)
    b = torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16)
    return b.view(torch.bfloat16).double()


def within_bf16_ulp(got, ref, atol):
    """the project's one-ulp bound (test_qk_rmsnorm_rope_pair_matches_generic): |d| <= 2^-7 |ref| + atol"""
    got, ref = f64(got), f64(ref)
    return (got - ref).abs() <= ref.abs() * 2.0 ** -7 + atol


def rel(a, b):
    a, b = f64(a), f64(b)
    return ((a - b).norm() / b.norm()).item()


# ------------------------------------------------------------------------------------------------ umT5

def t5_rmsnorm(x, w, eps):
    """T5LayerNorm.forward with a bf16 weight: bf16(bf16(w) * bf16(x * rsqrt(mean(x^2) + eps))); x [M, C]"""
    x = f64(x)
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))
    return rbf(rbf(w) * rbf(n))


def t5_softmax_bias(s, batch, heads, rows_per_head, bucket=None, emb=None, key_mask=None):
    """T5Attention.forward's softmax.  s [batch * heads * rows_per_head, n] scores, bucket [rows_per_head, n]
    indices into emb [num_buckets, heads] (bf16 values), key_mask [batch, n] (0 = padded key).
    t = bf16(bf16(s) + bias), bias = the bucket embedding, or finfo(bf16).min where the key is masked;
    returns (softmax of t in fp64, t)"""
    n = s.shape[-1]
    bias = torch.zeros(batch, heads, rows_per_head, n, dtype=torch.float64)
    if bucket is not None:
        bias = bias + f64(emb)[bucket.cpu().long()].permute(2, 0, 1)[None]
    if key_mask is not None:
        bias = bias.masked_fill(key_mask.cpu().view(batch, 1, 1, n) == 0, BF16_MIN)
    t = rbf(rbf(s).view(batch, heads, rows_per_head, n) + bias).view(-1, n)
    return torch.softmax(t, -1), t


def t5_gelu_chain(x, th_shift=0):
    """GELU.forward of the reference on a bf16 tensor, every torch op rounded to bf16:
    0.5 * x * (1.0 + tanh(sqrt(2/pi) * (x + 0.044715 * x^3))); th_shift moves the bf16 tanh value by that many
    bf16 places before the rest of the chain"""
    x = f64(x)
    half_x = rbf(0.5 * x)
    x3 = rbf(x * x * x)
    inner = rbf(x + rbf(0.044715 * x3))
    th = rbf(torch.tanh(rbf(math.sqrt(2.0 / math.pi) * inner)))
    if th_shift:
        th = bf16_step(th, th_shift)
    return rbf(half_x * rbf(1.0 + th))


def t5_geglu(gate, fc1, th_shift=0):
    """T5FeedForward: bf16(fc1 * GELU(gate)), both bf16"""
    return rbf(f64(fc1) * t5_gelu_chain(gate, th_shift))


def t5_geglu_neighbours(gate, fc1):
    """[3, ...]: t5_geglu with the bf16 tanh value moved by -1, 0, +1 bf16 places (index 1 is the centre).  tanh
    is the one transcendental of the chain, and `1 + tanh` cancels for negative gates, so a last-place difference
    of two correct tanh implementations can move the output by many of its own ulps."""
    return torch.stack([t5_geglu(gate, fc1, k) for k in (-1, 0, 1)])


# ------------------------------------------------------------------------------------------------ CLIP

def clip_preprocess(img, S, mean=CLIP_MEAN, std=CLIP_STD):
    """CLIPModel.forward preprocessing of img [C, H, W] in [-1, 1] -> [C, S, S] fp64; mean / std taken at their
    fp32 values, as torchvision's Normalize makes them for an fp32 image"""
    x = F.interpolate(f64(img)[None], size=(S, S), mode="bicubic", align_corners=False)[0]
    x = x * 0.5 + 0.5
    m = torch.tensor(mean, dtype=torch.float32).double().view(-1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).double().view(-1, 1, 1)
    return (x - m) / s


def clip_patch_im2col(img, P, Kpad):
    """img [C, S, S] -> [1 + (S/P)^2, Kpad] bf16: row 1 + py * g + px, column (c, ky, kx) = img[c, py P + ky,
    px P + kx]; row 0 (class token) and the columns past C P P zero"""
    C, S, _ = img.shape
    g = S // P
    out = torch.zeros(1 + g * g, Kpad, dtype=torch.bfloat16)
    out[1:, :C * P * P] = img.cpu().view(C, g, P, g, P).permute(1, 3, 0, 2, 4).reshape(g * g, C * P * P).bfloat16()
    return out


# ------------------------------------------------------------------------------------------------ wav2vec2

def w2v_conv0_gn_gelu(audio, w, stride, gn_w, gn_b, eps, T):
    """feature-encoder layer 0: Conv1d(1, C, k, stride, bias=False) on the first (T - 1) stride + k samples,
    GroupNorm(C groups, C channels), exact GELU -> [T, C] fp64"""
    C, k = w.shape
    a = f64(audio)[:(T - 1) * stride + k]
    y = F.conv1d(a[None, None], f64(w)[:, None], stride=stride)
    if T == 1:  # F.group_norm refuses one value per channel; its formula gives (y - y) * rsqrt(0 + eps) * w + b
        y = (y - y) * f64(gn_w)[None, :, None] + f64(gn_b)[None, :, None]
    else:
        y = F.group_norm(y, C, f64(gn_w), f64(gn_b), eps)
    return F.gelu(y)[0].t()


def conv1d_im2col(x, T_in, col0, groups, cg, k, stride, pad, T_out, Kpad):
    """x [>= T_in, ld] channels-last -> [groups, T_out, Kpad]: column j cg + c = x[t stride + j - pad, col0 + g cg
    + c], zero outside [0, T_in) and past k cg.  Zero padding + an index gather, no arithmetic."""
    x = x.cpu()
    need = (T_out - 1) * stride + k  # padded rows the gather reaches
    xp = torch.zeros(max(need, pad + T_in), groups * cg, dtype=x.dtype)
    xp[pad:pad + T_in] = x[:T_in, col0:col0 + groups * cg]
    rows = torch.arange(T_out)[:, None] * stride + torch.arange(k)[None]  # [T_out, k]
    out = torch.zeros(groups, T_out, Kpad, dtype=x.dtype)
    for g in range(groups):
        out[g, :, :k * cg] = xp[rows][:, :, g * cg:(g + 1) * cg].reshape(T_out, k * cg)
    return out


def add_f32_bf16(x, y):
    """x (f32) + y (bf16) in fp32: one rounding, so the fp64 sum rounded to fp32 is the same number"""
    return (f64(x) + f64(y)).float()


# ------------------------------------------------------------------------------------------------ VAE

def vae_rmsnorm_silu(x, gamma, silu):
    """RMS_norm (F.normalize(x, dim=channels) * sqrt(C) * gamma) (+ SiLU); x [rows, C] -> fp64"""
    x = f64(x)
    y = x / x.norm(dim=-1, keepdim=True).clamp(min=1e-12) * math.sqrt(x.shape[-1]) * f64(gamma)
    return F.silu(y) if silu else y


def vae_input(z, mean, std, Cp):
    """z [Cz, THW] -> channels-last [THW, Cp] fp64: z * std + mean, the channels past Cz zero.  Also returns the
    magnitude |z std| + |mean| each element's fp32 roundings scale with."""
    z, mean, std = f64(z), f64(mean), f64(std)
    out = torch.zeros(z.shape[1], Cp, dtype=torch.float64)
    mag = torch.zeros_like(out)
    out[:, :z.shape[0]] = (z * std[:, None] + mean[:, None]).t()
    mag[:, :z.shape[0]] = ((z * std[:, None]).abs() + mean[:, None].abs()).t()
    return out, mag


def vae_output(x, C, post):
    """channels-last [THW, C_stride] -> [C, THW]: clamp(-1, 1) (+ / 2 + 0.5, clamp(0, 1)); fp64"""
    v = f64(x)[:, :C].t().clamp(-1, 1)
    return (v / 2 + 0.5).clamp(0, 1) if post else v


def vae_latent_out(x, Cz, mean, std):
    """channels-last [THW, C_stride] (mu | log_var) -> [2 Cz, THW]: (mu - mean) * (1 / std) | log_var; fp64"""
    v = f64(x)[:, :2 * Cz].t().clone()
    v[:Cz] = (v[:Cz] - f64(mean)[:, None]) * (1.0 / f64(std)[:, None])
    return v


def softmax_rows(s, scale):
    return torch.softmax(f64(s) * scale, -1)


def transpose_batched(x):
    """[batch, rows, cols] -> [batch, cols, rows]"""
    return x.cpu().transpose(1, 2).contiguous()


def _conv_weight(w, cout, kt, kh, kw, cin):
    """the packed layout [Cout_pad][kt][kh][kw][Cin] of the implicit-GEMM convs (as _ref of
    test_gpu_vae_conv_dma.py unpacks it) -> torch's [Cout, Cin, kt, kh, kw]"""
    return f64(w)[:cout].reshape(cout, kt, kh, kw, cin).permute(0, 4, 1, 2, 3)


def conv_down2d(x, w, b, cout):
    """Resample 'downsample*': ZeroPad2d((0, 1, 0, 1)) + Conv2d(3x3, stride 2) per frame;
    x channels-last [T, H_in, W_in, Cin] -> [T, H_in / 2, W_in / 2, Cout] fp64"""
    cin = x.shape[-1]
    xc = F.pad(f64(x).permute(0, 3, 1, 2), (0, 1, 0, 1))
    wt = _conv_weight(w, cout, 1, 3, 3, cin)[:, :, 0]
    return F.conv2d(xc, wt, f64(b)[:cout], stride=2).permute(0, 2, 3, 1)


def conv_down_time(x, w, b, cout):
    """Resample 'downsample3d' time_conv: Conv3d((3, 1, 1), stride (2, 1, 1), no padding);
    x channels-last [2 T_out + 1, H, W, C] -> [T_out, H, W, Cout] fp64"""
    cin = x.shape[-1]
    xc = f64(x).permute(3, 0, 1, 2)[None]
    wt = _conv_weight(w, cout, 3, 1, 1, cin)
    return F.conv3d(xc, wt, f64(b)[:cout], stride=(2, 1, 1))[0].permute(1, 2, 3, 0)
