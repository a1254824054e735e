"""The references of tests/dit_ref.py against independent evaluations (oracle/dit.py, torch.nn.functional in fp64,
explicit loops, torch's own bf16 op sequence), and the conditions the GPU tests' caps rest on: a correct fp32
evaluation must leave the once-rounded bf16 reference on far fewer elements than the 1 % the GPU tests allow."""
import math

import pytest
import torch
import torch.nn.functional as F

import aux_ref as A
import dit_ref as R
from oracle import dit as odit


def _table(head_dim):
    """the fp32 (cos, sin) table of transformer.rope_table, from the oracle's complex128 frequencies"""
    fr = odit.model_freqs(head_dim)
    return torch.stack([fr.real, fr.imag], -1).float().contiguous()


# ------------------------------------------------------------------------------------------------ layernorm_mod

@pytest.mark.parametrize("C", [1536, 72])
def test_layernorm_mod_vs_functional(C):
    """F.layer_norm in fp64, the oracle's fp32 layer_norm, and the modulate / gate formulas written out"""
    M, B, rpb = 21, 2, 11
    x, w, b, shift, scale, gate = R.ln_inputs(M, C, B, 1)
    y, T = R.layernorm_mod(x, 1e-5, w, b)
    ln = F.layer_norm(x.double(), (C,), w.double(), b.double(), A.f64(torch.tensor(1e-5)).item())
    assert (y - ln).abs().max() <= 1e-12 * T.max()
    # fp32: the error of the mean reaches every element of a row, so the bound is per tensor, not per element
    assert (y - odit.layer_norm(x, 1e-5, w, b).double()).abs().max() <= 2.0 ** -20 * T.max()
    y, _ = R.layernorm_mod(x, 1e-6, w)
    ln0 = F.layer_norm(x.double(), (C,), None, None, R.f32c(1e-6))
    assert (y - ln0 * w.double()).abs().max() <= 1e-12 * T.max()
    bi = torch.arange(M) // rpb
    mod = ln0 * (1 + scale.double()[bi]) + shift.double()[bi]
    y, T = R.layernorm_mod(x, 1e-6, shift=shift, scale=scale, rows_per_batch=rpb)
    assert (y - mod).abs().max() <= 1e-12 * T.max()
    y, T = R.layernorm_mod(x, 1e-6, shift=shift, scale=scale, gate=gate, rows_per_batch=rpb)
    assert (y - (x.double() + mod * gate.double()[bi])).abs().max() <= 1e-12 * T.max()
    assert (T >= y.abs() * (1 - 1e-12)).all()  # the term magnitude bounds the value
    assert torch.isfinite(y[M // 2]).all()  # the constant row
    yb, _ = R.layernorm_mod(x, 1e-6, shift=shift, scale=scale, rows_per_batch=rpb, out_bf16=True)
    assert torch.equal(yb, A.rbf(mod))


def test_layernorm_mod_fp32_restatement_share():
    """the cap condition of test_gpu_norm_kernels.test_layernorm_mod (bf16 output: at most 1 % of the elements off
    the reference): the fp32 restatement, rounded to bf16, is within one ulp of the once-rounded reference and
    differs from it on at most 0.007 % of the elements of the test's own inputs (pooled over the widths and modes:
    the narrow widths have so few elements that one is 0.012 %; no single case above 0.1 %)"""
    total = diff = 0
    for C in R.LN_WIDTHS:
        M, B, rpb = 1037, 2, 528
        for bf16_in in (False, True):
            x, w, b, shift, scale, gate = R.ln_inputs(M, C, B, C, bf16_in)
            for kw in (dict(w=w, b=b), dict(w=w), dict(shift=shift, scale=scale, rows_per_batch=rpb)):
                ref, _ = R.layernorm_mod(x, 1e-6, out_bf16=True, **kw)
                got = R.layernorm_mod_f32(x, 1e-6, **kw).bfloat16().double()
                assert A.within_bf16_ulp(got, ref, 1e-6).all()
                n = int((got != ref).sum())
                print(f"C={C} bf16_in={bf16_in} {sorted(kw)}: {n} of {ref.numel()}")
                assert n <= 1e-3 * ref.numel()
                total += ref.numel()
                diff += n
    print(f"fp32 restatement off the reference: {diff} of {total} = {diff / total:.4%}")
    assert diff / total <= 7e-5


# ------------------------------------------------------------------------------------------------ qk_rmsnorm_rope

@pytest.mark.parametrize("head_dim,C", [(128, 1536), (64, 640)])
def test_qk_rmsnorm_rope_vs_oracle(head_dim, C):
    """oracle/dit.py's rms_norm + rope_apply (complex multiplication by self.freqs) on two batch rows with padded
    tokens; the pair magnitude bounds both elements of the pair"""
    grid = R.QK_GRID
    L = grid[0] * grid[1] * grid[2] + 5
    nf, nh = R.rope_split(head_dim)
    qkv, wq, _ = R.qk_inputs(2 * L, C, 3)
    x = qkv[:, :C]
    got, mag = R.qk_rmsnorm_rope(x, wq, 1e-6, _table(head_dim), head_dim, grid, 0, L, nf, nh, rounded=False)
    n = odit.rms_norm(x.double(), wq.double(), R.f32c(1e-6))  # .float() inside: fp32 from here on
    ref = odit.rope_apply(n.view(2, L, C // head_dim, head_dim), [grid, grid], odit.model_freqs(head_dim))
    assert ((got - ref.reshape(2 * L, C).double()).abs() <= 2.0 ** -20 * mag + 1e-30).all()
    assert (got.abs() <= mag * (1 + 1e-6)).all()
    unrot, _ = R.qk_rmsnorm_rope(x, wq, 1e-6, rounded=False)
    assert torch.equal(got[L - 5:L], unrot[L - 5:L]) and not torch.equal(got[:L - 5], unrot[:L - 5])
    # a token offset is a shift of the rows of one batch row
    off, _ = R.qk_rmsnorm_rope(x[7:L], wq, 1e-6, _table(head_dim), head_dim, grid, 7, L, nf, nh, rounded=False)
    assert torch.equal(off, got[7:L])


def test_rope_table_is_the_oracle_frequencies():
    from stableavatar_amd.transformer import rope_table
    for d in (128, 64):
        assert torch.equal(rope_table(d), _table(d))


def test_qk_rmsnorm_rope_fp32_restatement_bound_and_share():
    """the conditions of test_gpu_norm_kernels.test_qk_rmsnorm_rope at its own inputs: the fp32 restatement is
    within 2^-7 |ref| + 2^-20 (|re| + |im|) of the reference, also with the project's plain 1e-6 term, and differs
    from it on at most 0.008 % of the elements at C = 1536 / 5120 / 640"""
    total = diff = 0
    for name, C, hd, with_k, rope, off in R.QK_CASES:
        qkv, wq, wk = R.qk_inputs(R.QK_M, C, C + off)
        nf, nh = R.rope_split(hd)
        tab = _table(hd) if rope else None
        for col, w in ((0, wq), (C, wk))[:2 if with_k else 1]:
            x = qkv[:, col:col + C]
            ref, mag = R.qk_rmsnorm_rope(x, w, 1e-6, tab, hd, R.QK_GRID, off, R.QK_RPB, nf, nh)
            got = R.qk_rmsnorm_rope_f32(x, w, 1e-6, tab, hd, R.QK_GRID, off, R.QK_RPB, nf, nh).bfloat16().double()
            assert ((got - ref).abs() <= 2.0 ** -7 * ref.abs() + 2.0 ** -20 * mag).all(), name
            assert A.within_bf16_ulp(got, ref, 1e-6).all(), name
            if C in (1536, 5120, 640):
                total += ref.numel()
                diff += int((got != ref).sum())
    print(f"fp32 restatement off the reference: {diff} of {total} = {diff / total:.4%}")
    assert diff / total <= 8e-5


# ------------------------------------------------------------------------------------------------ small ops

def test_timestep_embed_vs_oracle():
    t = torch.tensor([0.0, 24.41, 995.87, 1000.0])
    for dim in (2, 256, 2048):
        ref = odit.sinusoidal_embedding_1d(dim, t)
        assert (R.timestep_embed(t, dim) - ref).abs().max() <= 1e-11  # exp(-i ln 10000 / half) vs pow, angle <= 1000


def test_activations_vs_functional():
    x = torch.cat([R.GELU_GRID, torch.randn(1000, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 4])
    assert (R.silu(x) - F.silu(x)).abs().max() <= 1e-14
    assert (R.gelu_tanh(x) - F.gelu(x, approximate="tanh")).abs().max() <= 1e-14  # absolute: see gelu_tanh
    assert (R.gelu_erf(x) - F.gelu(x)).abs().max() <= 1e-14


def test_gelu_tanh_fp32_restatement_on_the_grid():
    """the cap condition of test_gpu_gemm_exact's GELU(tanh) test: on the 1/8 grid of its pre-activations an fp32
    evaluation rounds to the reference's bf16 value everywhere"""
    x = R.GELU_GRID.float()
    u = math.sqrt(2 / math.pi) * (x + 0.044715 * x * x * x)
    g32 = (x / (1 + torch.exp(-2 * u))).bfloat16().double()
    assert torch.equal(g32, A.rbf(R.gelu_tanh(R.GELU_GRID)))
    # torch's own fp32 form 0.5 x (1 + tanh u) cancels to -0 below x = -4 or so, where the value is not 0
    t32 = F.gelu(x, approximate="tanh").bfloat16().double()
    assert (t32[x < -6] == 0).all() and (g32[x < -6] < 0).all()


@pytest.mark.parametrize("act_in,act_out", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_small_linear_vs_functional(act_in, act_out):
    g = torch.Generator().manual_seed(5)
    x, W, b = torch.randn(3, 256, generator=g), torch.randn(6, 256, generator=g).bfloat16(), torch.randn(6, generator=g)
    xa = F.silu(x.double()) if act_in else x.double()
    ref = F.linear(xa, W.double(), b.double())
    ref = F.silu(ref) if act_out else ref
    y, S, pre = R.small_linear(x, W, b, act_in, act_out)
    assert (y - ref).abs().max() <= 1e-12 * S.max()
    assert (S >= pre.abs() * (1 - 1e-12)).all()
    y0, S0, _ = R.small_linear(x, W, None, act_in, act_out)
    ref0 = F.linear(xa, W.double())
    assert (y0 - (F.silu(ref0) if act_out else ref0)).abs().max() <= 1e-12 * S.max()
    # the slope of SiLU the GPU test lets a pre-activation error grow by: at most 1.1
    v = torch.linspace(-20, 20, 400001, dtype=torch.float64, requires_grad=True)
    slope, = torch.autograd.grad(F.silu(v).sum(), v)
    assert slope.abs().max() <= 1.1


def test_exact_index_ops_vs_loops():
    g = torch.Generator().manual_seed(9)
    # patch_im2col: Conv3d(k = s = (1, 2, 2)) of cat(x, y) with one-hot kernels picks the columns
    B, Fr, H, W, cx, cy, off = 2, 2, 4, 6, 3, 2, 1
    x = torch.randn(1, cx, Fr + off + 1, H, W, generator=g).bfloat16()
    y = torch.randn(B, cy, Fr + 2, H, W, generator=g).bfloat16()
    K = 4 * (cx + cy)
    got = R.patch_im2col(x, y, B, Fr, H, W, K + 8, Fr * 6 + 3, off, True)
    z = torch.cat([x[:, :, off:off + Fr].expand(B, -1, -1, -1, -1), y[:, :, :Fr]], 1).float()
    onehot = torch.eye(K).view(K, cx + cy, 1, 2, 2)
    ref = F.conv3d(z, onehot, stride=(1, 2, 2)).flatten(2).transpose(1, 2)
    assert torch.equal(got[:, :Fr * 6, :K].float(), ref)
    assert (got[:, Fr * 6:] == 0).all() and (got[:, :, K:] == 0).all()
    gx = R.patch_im2col(y, None, B, Fr, H, W, 4 * cy, Fr * 6)
    assert torch.equal(gx.float(), F.conv3d(y[:, :, :Fr].float(), torch.eye(4 * cy).view(4 * cy, cy, 1, 2, 2),
                                            stride=(1, 2, 2)).flatten(2).transpose(1, 2))
    # unpatchify: the reference's einsum
    C, Lp = 5, Fr * 6 + 3
    head = torch.randn(B * Lp, 4 * C + 8, generator=g).bfloat16()
    got = R.unpatchify(head, Lp, B, C, Fr, H, W)
    for b_ in range(B):
        u = head[b_ * Lp:b_ * Lp + Fr * 6, :4 * C].view(Fr, H // 2, W // 2, 1, 2, 2, C)
        assert torch.equal(got[b_], torch.einsum("fhwpqrc->cfphqwr", u).reshape(C, Fr, H, W))
    # mod_add and gather_rows: loops
    mod, e = torch.randn(2, 3, 8, generator=g), torch.randn(2, 3, 8, generator=g)
    got = R.mod_add(mod, e)
    for l in range(2):
        for b_ in range(2):
            assert torch.equal(got[l, b_], mod[l] + e[b_])
    assert torch.equal(R.mod_add(mod, e[:, 0]), mod[:, None] + e[None, :, :1])
    src, idx = torch.randn(5, 7, generator=g), torch.tensor([3, -1, 0, 4, -7])
    got = R.gather_rows(src, idx)
    for r, i in enumerate(idx.tolist()):
        assert torch.equal(got[r], src[i] if i >= 0 else torch.zeros(7))


# ------------------------------------------------------------------------------------------------ flow_step

def _torch_flow_step(lat, pred, noise, start, dsigma, a, t, overlap, prev_end, wts, blend):
    """the pipeline's lines on bf16 tensors, as torch evaluates them (oracle/pipeline.py:103-113): the guidance
    scales Python floats, the step size a 0-d fp32 tensor (a difference of two entries of the sigma table)"""
    T = lat.shape[2]
    idx = [ii % T for ii in range(start, start + noise.shape[2])]
    x = lat[:, :, idx].clone()
    if noise.shape[0] == 3:
        u, d, c = noise.chunk(3)
        v = u + a * (d - u) + t * (c - d)
    else:
        v = noise
    x = (x.float() + torch.tensor(dsigma, dtype=torch.float32) * v).to(v.dtype)
    if blend:
        w = wts[:overlap].view(1, 1, overlap, 1, 1).to(x.dtype)
        oi = list(range(overlap))
        pi = [ii % T for ii in range(prev_end - overlap, prev_end)]
        x[:, :, oi] = x[:, :, oi] * w + pred[:, :, pi] * (1 - w)
    out = pred.clone()
    for k in range(noise.shape[2]):
        out[:, :, (start + k) % T] = x[:, :, k]
    return out


@pytest.mark.parametrize("R_,start,Fw,overlap,prev_end,blend", R.FLOW_CASES)
def test_flow_step_equals_torch_bf16_sequence(R_, start, Fw, overlap, prev_end, blend):
    lat, pred, noise, wts = R.flow_inputs(R_, Fw)
    args = (start, -0.0042, 5.3, 3.1, overlap, prev_end, wts, blend)
    ref = _torch_flow_step(lat, pred, noise, *args)
    got = R.flow_step(lat, pred, noise, *args)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    assert not torch.equal(got, pred)


def test_flow_step_fp64_chain_is_not_the_reference():
    """why flow_step is not written as an fp64 chain with one rbf per op: that chain is off torch's own sequence
    on about 1 % of the elements (double rounding: fp64 -> bf16 in one step vs the fp32 result -> bf16)"""
    lat, pred, noise, _ = R.flow_inputs(3, 21)
    u, d, c = (A.f64(n) for n in noise)
    v = A.rbf(A.rbf(u + A.rbf(A.rbf(d - u) * R.f32c(5.3))) + A.rbf(A.rbf(c - d) * R.f32c(3.1)))
    x = A.rbf(A.f64(lat[0][:, 6:27]) + A.rbf(A.rbf(R.f32c(-0.0042)) * v))
    ref = R.flow_step(lat, pred, noise, 6, -0.0042, 5.3, 3.1)[0][:, 6:27].double()
    share = (x != ref).double().mean().item()
    print(f"fp64 chain off the fp32 chain on {share:.3%}")
    assert 0 < share < 0.05


# ------------------------------------------------------------------------------------------------ GEMM references

def test_int_gemm_is_exact_in_fp32():
    """the largest sums of the exact GEMM tests (K = 256, |x|, |w| <= 3, |bias| <= 50) stay below 2^24, so an fp32
    accumulation in any order is exact and equals the fp64 reference"""
    assert 256 * 9 + 50 < 2 ** 24
    g = torch.Generator().manual_seed(2)
    x = torch.randint(-3, 4, (64, 256), generator=g).float()
    w = torch.randint(-3, 4, (48, 256), generator=g).float()
    b = torch.randint(-50, 51, (48,), generator=g).float()
    ref = R.int_gemm(x, w, b)
    assert torch.equal(ref, (x @ w.t() + b).double())
    assert torch.equal(ref, torch.round(ref))
    res = torch.randint(-100, 101, (64, 48), generator=g).float()
    gate = torch.randint(-2, 3, (2, 48), generator=g).float()
    out = R.gated_residual(ref, res, gate, 40)
    bi = torch.arange(64) // 40
    assert torch.equal(out, res.double() + (x @ w.t() + b).bfloat16().double() * gate.double()[bi])
    assert torch.equal(out, out.float().double())  # fp32 holds it exactly
