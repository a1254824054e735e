"""Shared by the per-kernel tests of norm.hip, elementwise.hip and the GEMM epilogues: one plain fp64 (or exact
integer-indexing) torch function per operation, implementing what include/stableavatar_hip.h documents for it, with a
single bf16 rounding where the output is bf16.  They run on the CPU; tests/test_dit_ref_cpu.py pins each against an
independent evaluation.  The magnitudes some of them return next to the value are what an fp32 evaluation's rounding
errors scale with; the GPU tests' fp32 bounds are stated in them."""
import math

import torch

from aux_ref import f64, rbf


def f32c(v):
    """a Python number as the fp32 value a `float` argument of the C ABI carries, in fp64"""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ norm.hip

def layernorm_mod(x, eps, w=None, b=None, shift=None, scale=None, gate=None, rows_per_batch=0, out_bf16=False):
    """LayerNorm (biased variance) -> affine -> y (1 + scale[b]) + shift[b] -> x + y gate[b], b = row //
    rows_per_batch; x [M, C], w / b [C], shift / scale / gate [B, C].  Returns (y, T): T = |n| |w| + |b|, then
    T |1 + scale| + |shift|, then |x| + |gate| T -- the sum of the magnitudes of the terms y is made of."""
    x = f64(x)
    M = x.shape[0]
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    y = (x - mean) * torch.rsqrt(var + f32c(eps))
    T = y.abs()
    if w is not None:
        y, T = y * f64(w), T * f64(w).abs()
        if b is not None:
            y, T = y + f64(b), T + f64(b).abs()
    if scale is not None or gate is not None:
        bi = torch.arange(M) // rows_per_batch
    if scale is not None:
        sc, sh = f64(scale)[bi], f64(shift)[bi]
        y, T = y * (1 + sc) + sh, T * (1 + sc).abs() + sh.abs()
    if gate is not None:
        g = f64(gate)[bi]
        y, T = x + y * g, x.abs() + g.abs() * T
    return (rbf(y) if out_bf16 else y), T


def rope_positions(M, grid, tok_offset, rows_per_batch):
    """token t = tok_offset + row % rows_per_batch -> (rotated [M] bool, frame, height, width index [M])"""
    Fr, H, W = grid
    t = tok_offset + torch.arange(M) % rows_per_batch
    return t < Fr * H * W, t // (H * W), (t // W) % H, t % W


def qk_rmsnorm_rope(x, w, eps, table=None, head_dim=128, grid=(1, 1, 1), tok_offset=0, rows_per_batch=1, nf=0, nh=0,
                    rounded=True):
    """WanRMSNorm over the whole row, then the 3-D RoPE on (even, odd) column pairs: pair p = (c % head_dim) / 2
    takes its angle from the frame index for p < nf, the height index for p < nf + nh, else the width index;
    (cos, sin) = table[index, p] as the fp32 table holds them; rows whose token is past F H W stay unrotated.
    x [M, C] -> (bf16 values [M, C] in fp64 (rounded=False: the values before that rounding), |re| + |im| of each
    element's normalised pair [M, C])"""
    rnd = rbf if rounded else (lambda v: v)
    x = f64(x)
    M, C = x.shape
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + f32c(eps)) * f64(w)
    re, im = n[:, 0::2], n[:, 1::2]
    mag = (re.abs() + im.abs()).repeat_interleave(2, 1)
    if table is None:
        return rnd(n), mag
    rot, fi, hi, wi = rope_positions(M, grid, tok_offset, rows_per_batch)
    p = (torch.arange(0, C, 2) % head_dim) // 2  # [C / 2]
    pos = torch.where(p[None] < nf, fi[:, None], torch.where(p[None] < nf + nh, hi[:, None], wi[:, None]))
    cs_sn = f64(table)[pos, p[None].expand_as(pos)]  # [M, C / 2, 2]
    cs, sn = cs_sn[..., 0], cs_sn[..., 1]
    out = torch.stack([re * cs - im * sn, re * sn + im * cs], -1).reshape(M, C)
    return rnd(torch.where(rot[:, None], out, n)), mag


# ------------------------------------------------------------------------------------------------ elementwise.hip

def timestep_embed(t, dim):
    """sinusoidal_embedding_1d: [cos(t f_i) | sin(t f_i)], f_i = 10000^(-i / (dim / 2)); t fp32 values -> [B, dim]"""
    half = dim // 2
    i = torch.arange(half, dtype=torch.float64)
    s = f64(t)[:, None] * torch.exp(-math.log(10000.0) * i / half)[None]
    return torch.cat([torch.cos(s), torch.sin(s)], 1)


def silu(x):
    x = f64(x)
    return x / (1 + torch.exp(-x))


def gelu_tanh(x):
    """nn.GELU(approximate='tanh'): 0.5 x (1 + tanh u) = x / (1 + exp(-2 u)), u = sqrt(2 / pi) (x + 0.044715 x^3),
    in the second form: `1 + tanh u` cancels for negative x (to 0 in fp64 below x = -7), the quotient does not"""
    x = f64(x)
    return x / (1 + torch.exp(-2 * math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_erf(x):
    x = f64(x)
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def small_linear(x, W, b=None, act_in=0, act_out=0):
    """act_out(act_in(x) W^T + b), act = SiLU where 1.  Returns (value, S, pre): S = sum_k |act_in(x_k) w_k| + |b|,
    pre the value before act_out"""
    xa = silu(x) if act_in else f64(x)
    W = f64(W)
    pre = xa @ W.t()
    S = xa.abs() @ W.abs().t()
    if b is not None:
        pre, S = pre + f64(b), S + f64(b).abs()
    return (silu(pre) if act_out else pre), S, pre


def mod_add(mod, e):
    """out[l, b, j, c] = mod[l, j, c] + e[b, j, c] (e [B, C]: broadcast over j), one fp32 addition"""
    mod, e = mod.cpu().float(), e.cpu().float()
    if e.dim() == 2:
        e = e[:, None]
    return mod[:, None] + e[None]


def gather_rows(inp, idx):
    """out[r] = inp[idx[r]] for idx[r] >= 0, else a zero row"""
    inp, idx = inp.cpu(), idx.cpu().long()
    out = inp[idx.clamp(min=0)].clone()
    out[idx < 0] = 0
    return out


def patch_im2col(x, y, B, Fr, H, W, Kpad, Lpad, x_frame_offset=0, x_batch_broadcast=False):
    """cat(x[:, :, off:off + F], y[:, :, :F], channels) [B, c, F, H, W] -> [B, Lpad, Kpad]: row (f, h / 2, w / 2),
    column 4 c + 2 (h % 2) + w % 2; the rows past F (H / 2) (W / 2) and the columns past 4 c zero"""
    x = x.cpu()[:, :, x_frame_offset:x_frame_offset + Fr]
    if x_batch_broadcast:
        x = x[:1].expand(B, -1, -1, -1, -1)
    z = x[:B] if y is None else torch.cat([x[:B], y.cpu()[:B, :, :Fr]], 1)
    c = z.shape[1]
    hp, wp = H // 2, W // 2
    cols = z.reshape(B, c, Fr, hp, 2, wp, 2).permute(0, 2, 3, 5, 1, 4, 6).reshape(B, Fr * hp * wp, 4 * c)
    out = torch.zeros(B, Lpad, Kpad, dtype=z.dtype)
    out[:, :Fr * hp * wp, :4 * c] = cols
    return out


def unpatchify(head, Lpad, B, C, Fr, H, W):
    """head [B * Lpad, >= 4 C] -> [B, C, F, H, W]: out[b, c, f, h, w] = head[b Lpad + (f, h / 2, w / 2),
    (2 (h % 2) + w % 2) C + c]"""
    hp, wp = H // 2, W // 2
    u = head.cpu()[:, :4 * C].reshape(B, Lpad, 4 * C)[:, :Fr * hp * wp].reshape(B, Fr, hp, wp, 2, 2, C)
    return u.permute(0, 6, 1, 2, 4, 3, 5).reshape(B, C, Fr, H, W)


def flow_step(lat, pred, noise, start, dsigma, audio_scale, text_scale, overlap=0, prev_end=0, weights=None,
              blend=False):
    """One sampler step of one window on pred [1, C, T, H, W] (a new tensor is returned): CFG combine, Euler step,
    overlap blend, scatter to the frames (start + f) % T.  Not an fp64 chain: every op is the fp32 torch op on
    bf16-representable inputs followed by a .bfloat16() cast, in the order of the kernel (the reference computes on
    bf16 tensors: each op rounds once from the exact fp32 result, which an fp64 value rounded by rbf per op
    reproduces only up to double rounding).  The two guidance scales are Python floats in the reference and enter
    as fp32 values; the step size is a 0-d fp32 tensor there, which torch casts to the bf16 of the tensor it
    multiplies."""
    bf = lambda v: v.bfloat16().float()
    lat, pred, noise = lat.cpu(), pred.cpu().clone(), noise.cpu()
    T, Fw = lat.shape[2], noise.shape[2]
    a, t, ds = (torch.tensor(s, dtype=torch.float32) for s in (audio_scale, text_scale, dsigma))
    if noise.shape[0] == 3:
        u, d, c = (n.float() for n in noise)
        t1 = bf(bf(d - u) * a)
        t2 = bf(bf(c - d) * t)
        v = bf(bf(u + t1) + t2)
    else:
        v = noise[0].float()
    fa = (start + torch.arange(Fw)) % T
    x1 = bf(lat[0][:, fa].float() + bf(bf(ds) * v))
    if blend:
        w = bf(weights.cpu().float()[:overlap]).view(1, overlap, 1, 1)
        fp = (prev_end - overlap + torch.arange(overlap)) % T
        a1 = bf(x1[:, :overlap] * w)
        a2 = bf(pred[0][:, fp].float() * bf(1.0 - w))
        x1[:, :overlap] = bf(a1 + a2)
    pred[0][:, fa] = x1.bfloat16()
    return pred


# ------------------------------------------------------------------------------------------------ GEMM epilogues

def int_gemm(x, w, bias=None):
    """x [.., M, K] @ w [.., N, K]^T + bias on small-integer operands, in fp64: exact (|sum| < 2^24, so fp32 is too)"""
    y = f64(x) @ f64(w).transpose(-1, -2)
    return y if bias is None else y + f64(bias)


def gated_residual(acc, res, gate, rows_per_batch):
    """res + bf16(acc) * gate[row // rows_per_batch] (gate None: 1); acc already holds the bias"""
    y = rbf(acc)
    if gate is not None:
        y = y * f64(gate)[torch.arange(acc.shape[0]) // rows_per_batch]
    return f64(res) + y


# ------------------------------------------------------------------------------------------------ fp32 restatements
# The same formulas in plain fp32 torch ops, in another order than the kernels'.  The GPU tests measure their
# distance from the fp64 references at the same inputs (the ratio r of the fp32-output bounds), and
# test_dit_ref_cpu.py checks that they leave the once-rounded bf16 value on far fewer elements than the tests' cap.

def _seq_mean(v):
    """row means by a plain left-to-right fp32 loop (torch's own mean sums in a cascade)"""
    s = torch.zeros(v.shape[0], dtype=torch.float32)
    for c in range(v.shape[1]):
        s = s + v[:, c]
    return (s / v.shape[1])[:, None]


def layernorm_mod_f32(x, eps, w=None, b=None, shift=None, scale=None, gate=None, rows_per_batch=0, seq=False):
    """seq: the two row sums by a plain sequential loop instead of torch's cascade"""
    x = x.cpu().float()
    mean = _seq_mean(x) if seq else x.mean(-1, keepdim=True)
    var = _seq_mean((x - mean).pow(2)) if seq else (x - mean).pow(2).mean(-1, keepdim=True)
    y = (x - mean) * torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    if w is not None:
        y = y * w.cpu().float()
        if b is not None:
            y = y + b.cpu().float()
    if scale is not None or gate is not None:
        bi = torch.arange(x.shape[0]) // rows_per_batch
    if scale is not None:
        y = y * (1 + scale.cpu().float()[bi]) + shift.cpu().float()[bi]
    if gate is not None:
        y = x + y * gate.cpu().float()[bi]
    return y


def qk_rmsnorm_rope_f32(x, w, eps, table=None, head_dim=128, grid=(1, 1, 1), tok_offset=0, rows_per_batch=1, nf=0,
                        nh=0):
    x = x.cpu().float()
    M, C = x.shape
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + torch.tensor(eps, dtype=torch.float32)) * w.cpu().float()
    if table is None:
        return n
    rot, fi, hi, wi = rope_positions(M, grid, tok_offset, rows_per_batch)
    p = (torch.arange(0, C, 2) % head_dim) // 2
    pos = torch.where(p[None] < nf, fi[:, None], torch.where(p[None] < nf + nh, hi[:, None], wi[:, None]))
    cs_sn = table.cpu().float()[pos, p[None].expand_as(pos)]
    re, im, cs, sn = n[:, 0::2], n[:, 1::2], cs_sn[..., 0], cs_sn[..., 1]
    out = torch.stack([re * cs - im * sn, re * sn + im * cs], -1).reshape(M, C)
    return torch.where(rot[:, None], out, n)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs

def ln_inputs(M, C, B, seed, bf16_in=False):
    """x = randn * 3 + 1 with every 7th column scaled by 20 and one constant row (variance 0); w, b [C]; shift,
    scale, gate [B, C]"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * 3 + 1
    x[:, ::7] *= 20
    x[M // 2] = 2.5
    if bf16_in:
        x = x.bfloat16()
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    shift, scale, gate = (torch.randn(B, C, generator=g) for _ in range(3))
    return x, w, b, shift, scale, gate


def qk_inputs(M, C, seed):
    """the q | k | v columns of a QKV GEMM output [M, 3 C] (bf16) and the two norm weights"""
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(M, 3 * C, generator=g) * 2).bfloat16()
    return qkv, torch.randn(C, generator=g), torch.randn(C, generator=g)


def rope_split(head_dim):
    """(pairs on the frame axis, pairs on the height axis) of self.freqs' split"""
    c = head_dim // 2
    return c - 2 * (c // 3), c // 3


GELU_GRID = torch.arange(-64, 65, dtype=torch.float64) / 8  # the pre-activations of the GEMM activation tests

# sa_qk_rmsnorm_rope cases: (id, C, head_dim, with k, with RoPE, tok_offset).  Every case: grid (F, H, W) = QK_GRID (60
# tokens, all three sizes different), QK_RPB rows per batch row, QK_M rows = two batch rows, not a multiple of the 4
# rows of a workgroup.  tok_offset 0 / 37: every token of a batch row inside the grid; 50: tokens 50 .. 72, so the
# first padded (unrotated) token is row 10 of each batch row, inside the launch.
QK_GRID, QK_RPB, QK_M = (3, 4, 5), 23, 46
QK_CASES = [
    ("pair", 1536, 128, True, True, 0),
    ("pair-off37", 1536, 128, True, True, 37),
    ("pair-off50", 1536, 128, True, True, 50),
    ("w1536-q-rope", 1536, 128, False, True, 37),
    ("w1536-q-norope", 1536, 128, False, False, 0),
    ("w5120", 5120, 128, True, True, 0),
    ("w5120-off50", 5120, 128, True, True, 50),
    ("w640-d64", 640, 64, True, True, 0),
    ("w640-d64-off50", 640, 64, True, True, 50),
    ("w72-q-norope", 72, 8, False, False, 0),
]
# sa_layernorm_mod: the widths and row counts of the GPU test
LN_WIDTHS, LN_ROWS = (1536, 5120, 1280, 72, 8), (1, 5, 21, 1037)

# sa_flow_step cases (R, start, Fw, overlap, prev_end, blend) on T = FLOW_T frames: the pipeline's use (the blended
# frames are the window's own first frames), a window that wraps past T, a wrapping prev_end - overlap that names
# frames outside the window, overlap == Fw, and R == 1.  The frames read for the blend are either the ones the same
# element writes or outside the window, as in the pipeline (the kernel reads and writes pred in one pass).
FLOW_T, FLOW_C, FLOW_HW = 30, 5, (3, 7)
FLOW_CASES = [
    (3, 6, 21, 0, 0, False),
    (1, 6, 21, 0, 0, False),
    (3, 6, 21, 15, 21, True),
    (1, 6, 21, 15, 21, True),
    (3, 20, 21, 0, 0, False),
    (3, 20, 21, 5, 25, True),
    (3, 28, 10, 5, 33, True),
    (3, 4, 10, 5, 32, True),
    (3, 9, 7, 7, 16, True),
    (1, 9, 7, 7, 16, True),
]


def flow_inputs(R_, Fw, seed=0):
    """latents / pred [1, C, T, H, W], noise [R, C, Fw, H, W] (bf16), overlap weights (fp32, not bf16 values)"""
    g = torch.Generator().manual_seed(seed + R_ + Fw)
    shp = (1, FLOW_C, FLOW_T) + FLOW_HW
    lat, pred = torch.randn(shp, generator=g).bfloat16(), torch.randn(shp, generator=g).bfloat16()
    noise = torch.randn((R_, FLOW_C, Fw) + FLOW_HW, generator=g).bfloat16()
    wts = torch.linspace(0, 1, Fw) ** 1.3
    return lat, pred, noise, wts
