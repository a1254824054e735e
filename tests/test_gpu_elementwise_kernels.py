"""Every entry point of csrc/elementwise.hip on its own against the references of tests/dit_ref.py (pinned on the CPU
by test_dit_ref_cpu.py), through ops / the C ABI, at the argument combinations the DiT never passes together: the
indexing ops bit for bit, the time embedding and the fp32 Linear against fp64 within stated rounding bounds, the
sampler step bit for bit against the reference's chain of bf16 ops.  Outputs are written into larger allocations
pre-filled with a sentinel, strided inputs carry NaN where the kernel must not read."""
import pytest
import torch

import aux_ref as A
import dit_ref as R
from stableavatar_amd import ops
from stableavatar_amd._lib import KernelError, call

pytestmark = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")
SENT = 7.0


def _sync():
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ exact ops

@pytest.mark.parametrize("broadcast", [True, False], ids=["broadcast", "perbatch"])
@pytest.mark.parametrize("with_y", [True, False], ids=["xy", "xonly"])
@pytest.mark.parametrize("off", [0, 2])
def test_patch_im2col(broadcast, with_y, off):
    """cat(x, y) -> im2col, bit for bit: batch broadcast of x or one x per batch row, y = None, a frame offset into
    x, Kpad at least 16 columns wider than 4 (xcn + ycn) and Lpad 5 rows more than the tokens (both pads zero), y with more
    frames than F; the allocation past [B, Lpad, Kpad] keeps its sentinel"""
    B, Fr, H, W, cx, cy = 3, 2, 6, 10, 5, 3
    g = torch.Generator().manual_seed(off + 2 * with_y)
    x = torch.randn(1 if broadcast else B, cx, Fr + off + 1, H, W, generator=g).bfloat16()
    y = torch.randn(B, cy, Fr + 2, H, W, generator=g).bfloat16() if with_y else None
    Kpad = (4 * (cx + (cy if with_y else 0)) + 7) // 8 * 8 + 16
    Lpad = Fr * (H // 2) * (W // 2) + 5
    buf = torch.full((B * Lpad * Kpad + 64,), SENT, device=dev, dtype=torch.bfloat16)
    out = buf[:B * Lpad * Kpad].view(B, Lpad, Kpad)
    ops.patch_im2col(x.to(dev), None if y is None else y.to(dev), B, Fr, H, W, out, Kpad, Lpad, x_frame_offset=off,
                     x_batch_broadcast=broadcast)
    _sync()
    ref = R.patch_im2col(x, y, B, Fr, H, W, Kpad, Lpad, off, broadcast)
    assert torch.equal(_bits(out.cpu()), _bits(ref))
    assert (out[:, Lpad - 5:] == 0).all() and (out[:, :, Kpad - 16:] == 0).all()
    assert (buf[B * Lpad * Kpad:] == SENT).all()


@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_unpatchify(odt):
    """Head output rows of stride ld_in = 4 C + 8 (NaN in the pad, NaN rows past each batch row's tokens) ->
    [B, C, F, H, W] in fp32 and in bf16, bit for bit"""
    B, C, Fr, H, W = 2, 5, 3, 4, 6
    Lp = Fr * (H // 2) * (W // 2) + 3
    g = torch.Generator().manual_seed(1)
    head = torch.full((B * Lp, 4 * C + 8), NAN).bfloat16()
    head.view(B, Lp, -1)[:, :Lp - 3, :4 * C] = torch.randn(B, Lp - 3, 4 * C, generator=g).bfloat16()
    n = B * C * Fr * H * W
    buf = torch.full((n + 64,), SENT, device=dev, dtype=odt)
    out = buf[:n].view(B, C, Fr, H, W)
    ops.unpatchify(head.to(dev), Lp, B, C, Fr, H, W, out)
    _sync()
    ref = R.unpatchify(head, Lp, B, C, Fr, H, W)
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(out.cpu(), ref.to(odt))
    assert (buf[n:] == SENT).all()


@pytest.mark.parametrize("jstride0", [False, True], ids=["e3d", "e2d-jstride0"])
def test_mod_add(jstride0):
    """mod [L, J, C] + e [B, J, C], and e [B, C] broadcast over j (e_jstride = 0, Head.forward); e rows strided
    with NaN between them"""
    L, B, J, C = 3, 2, 6, 100
    g = torch.Generator().manual_seed(2)
    mod = torch.randn(L, J, C, generator=g)
    if jstride0:
        ebuf = torch.full((B, C + 4), NAN)
        ebuf[:, :C] = torch.randn(B, C, generator=g)
        e = ebuf[:, :C]
    else:
        ebuf = torch.full((B, J * C + 4), NAN)
        ebuf[:, :J * C] = torch.randn(B, J * C, generator=g)
        e = ebuf[:, :J * C].unflatten(1, (J, C))
    n = L * B * J * C
    buf = torch.full((n + 64,), SENT, device=dev)
    out = buf[:n].view(L, B, J, C)
    ed = ebuf.to(dev)
    ev = ed[:, :C] if jstride0 else ed[:, :J * C].unflatten(1, (J, C))
    ops.mod_add(mod.to(dev), ev, out, e_jstride=0 if jstride0 else None)
    _sync()
    assert torch.equal(out.cpu(), R.mod_add(mod, e).expand(L, B, J, C))
    assert (buf[n:] == SENT).all()


def test_gather_rows():
    """negative indices give zero rows; a row of 1100 bytes (not a multiple of the 1024 a workgroup copies per
    pass), source and destination row strides larger than the row (NaN / sentinel in the pads)"""
    cols, rows = 275, 10
    g = torch.Generator().manual_seed(3)
    src = torch.full((rows, cols + 5), NAN)
    src[:, :cols] = torch.randn(rows, cols, generator=g)
    idx = torch.tensor([3, -1, 0, 9, -5, 9, 4], dtype=torch.int32)
    out = torch.full((len(idx) + 1, cols + 9), SENT, device=dev)
    ops.gather_rows(src.to(dev)[:, :cols], idx.to(dev), out[:len(idx), :cols])
    _sync()
    assert torch.equal(out[:len(idx), :cols].cpu(), R.gather_rows(src[:, :cols], idx))
    assert (out[:len(idx), cols:] == SENT).all() and (out[len(idx)] == SENT).all()
    call("sa_gather_rows", out.data_ptr(), 16, idx.to(dev).data_ptr(), 0, out.data_ptr(), 16, 16, ops._stream())  # no rows
    _sync()
    assert torch.equal(out[:len(idx), :cols].cpu(), R.gather_rows(src[:, :cols], idx)) and (out[len(idx)] == SENT).all()


@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_fill_and_cast(n):
    """sa_fill_f32 and sa_cast_f32_bf16 around the 256-thread block: exactly n elements written, the cast round to
    nearest even (aux_ref.rbf), ties and values past bf16's largest included"""
    buf = torch.full((n + 64,), SENT, device=dev)
    ops.fill_(buf[:n], -2.5)
    _sync()
    assert (buf[:n] == -2.5).all() and (buf[n:] == SENT).all()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 100
    x[::5] = (torch.randint(-300, 300, (len(x[::5]),), generator=g).float() * 2 + 1) * 2.0 ** -8  # ties of [1, 2)'s grid
    x[0] = 3.4e38
    ob = torch.full((n + 64,), SENT, device=dev, dtype=torch.bfloat16)
    ops.cast_bf16(x.to(dev), ob[:n])
    _sync()
    assert torch.equal(ob[:n].double().cpu(), A.rbf(x))
    assert (ob[n:] == SENT).all()
    call("sa_fill_f32", buf.data_ptr(), 0, 1.0, ops._stream())  # n == 0 stays a success
    call("sa_cast_f32_bf16", buf.data_ptr(), ob.data_ptr(), 0, ops._stream())
    _sync()
    assert (buf[n:] == SENT).all() and (ob[n:] == SENT).all()


# ------------------------------------------------------------------------------------------------ sa_timestep_embed

@pytest.mark.parametrize("dim", [2, 256, 2048])
def test_timestep_embed(dim):
    """the kernel computes cos / sin in fp64 and rounds once to fp32: |got - ref| <= 2^-24, one fp32 rounding of a
    value in [-1, 1] (ulp / 2 at most 2^-25, plus the fp64 evaluation's own error at angles up to 1000).  Measured on
    the MI355X: 2.98e-08 = 2^-25."""
    t = torch.tensor([0.0, 24.41, 995.87, 1000.0])
    out = torch.full((t.numel() + 1, dim), SENT, device=dev)
    ops.timestep_embed(t.to(dev), dim, out)
    _sync()
    e = (out[:4].double().cpu() - R.timestep_embed(t, dim)).abs().max().item()
    print(f"dim={dim}: max abs err {e:.3g}")
    assert e <= 2.0 ** -24
    assert (out[4] == SENT).all()


# ------------------------------------------------------------------------------------------------ sa_small_linear_f32

@pytest.mark.parametrize("act_in,act_out", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["plain", "silu-in", "silu-out", "both"])
@pytest.mark.parametrize("M,K,N", [(1, 8, 1), (3, 256, 6), (8, 1536, 6), (3, 1536, 9216), (1, 256, 9216), (8, 8, 6)])
def test_small_linear_f32(M, K, N, act_in, act_out):
    """|got - ref| <= (K + 8) 2^-24 S, S = sum_k |act(x_k) w_k| + |b|: the bound of a K-term fp32 dot product summed
    in any order, with room for the activations' own rounding; with act_out the bound holds for the pre-activation
    and grows by SiLU's slope (<= 1.1, test_dit_ref_cpu.py).  M = 1 / 3 / 8 rows, K below, at and above the 512
    columns a wave covers per pass, N = 1 (three idle waves) / 6 / 9216; with and without bias; ldi > K and ldo > N
    (NaN / sentinel in the pads).  Measured on the MI355X: at most 0.113 of the bound."""
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g).bfloat16()
    b = torch.randn(N, generator=g)
    xin = torch.full((M, K + 4), NAN, device=dev)
    xin[:, :K] = x.to(dev)
    Wd, bd = W.to(dev), b.to(dev)
    for bias in (b, None):
        out = torch.full((M + 1, N + 3), SENT, device=dev)
        ops.small_linear_f32(xin[:, :K], Wd, bd if bias is not None else None, out[:M, :N], act_in=act_in,
                             act_out=act_out)
        _sync()
        ref, S, _ = R.small_linear(x, W, bias, act_in, act_out)
        bound = (K + 8) * 2.0 ** -24 * S * (1.1 if act_out else 1.0)
        e = (out[:M, :N].double().cpu() - ref).abs()
        print(f"M={M} K={K} N={N} bias={bias is not None}: worst error / bound {(e / bound).max().item():.3g}")
        assert (e <= bound).all()
        assert (out[:M, N:] == SENT).all() and (out[M] == SENT).all()


# ------------------------------------------------------------------------------------------------ sa_flow_step

@pytest.mark.parametrize("R_,start,Fw,overlap,prev_end,blend", R.FLOW_CASES)
def test_flow_step(R_, start, Fw, overlap, prev_end, blend):
    """bit-equal to dit_ref.flow_step, the chain of fp32 ops each rounded to bf16 that equals torch's own bf16
    sequence of the pipeline's lines on the CPU (test_dit_ref_cpu.py): R = 1 and 3, blend on and off, a window
    that wraps past T (T = 30, start = 20, Fw = 21), a wrapping prev_end - overlap, overlap == Fw, scales (5.3,
    3.1, -0.0042) and blend weights that are not bf16 values; the frames outside the window and the latents
    untouched.
    This test found two deviations of the kernel from that sequence, both fixed with it: the compiler contracted
    the blend's x1 * w + a2 into an fma, which dropped the bf16 rounding of the first product (316 of the 1575
    blended elements of the first blend case one bf16 place off, torch's own ops on the MI355X agreeing with the
    chain), and the step size entered the Euler step as an fp32 value where torch casts the 0-d sigma difference
    to bf16 before it multiplies a bf16 tensor."""
    lat, pred, noise, wts = R.flow_inputs(R_, Fw)
    args = (start, -0.0042, 5.3, 3.1, overlap, prev_end)
    ld, pd, nd = lat.to(dev), pred.to(dev), noise.to(dev)
    ops.flow_step(ld, pd, nd, *args, wts.to(dev) if blend else None, blend)
    _sync()
    ref = R.flow_step(lat, pred, noise, *args, wts, blend)
    got = pd.cpu()
    assert torch.equal(_bits(got), _bits(ref))
    outside = [f for f in range(R.FLOW_T) if f not in {(start + k) % R.FLOW_T for k in range(Fw)}]
    assert torch.equal(got[:, :, outside], pred[:, :, outside])
    assert torch.equal(ld.cpu(), lat) and torch.equal(nd.cpu(), noise)


# ------------------------------------------------------------------------------------------------ argument checks

def test_elementwise_empty_sizes_are_bad_arguments():
    """a non-positive B, dim, N, K, L, J, C, F, Fw, HW, T, a negative nrows / n used to reach the launch with an empty
    (or wrapped) grid instead of SA_ERR_ARG; sa_flow_step took a negative start and, blending, prev_end < overlap,
    both of which index frames before the tensor.  Every call here is refused by the launcher's argument check:
    none launches."""
    f = torch.zeros(4096, device=dev)
    h = torch.zeros(4096, device=dev, dtype=torch.bfloat16)
    i32 = torch.zeros(16, device=dev, dtype=torch.int32)
    F_, H_, I_, st = f.data_ptr(), h.data_ptr(), i32.data_ptr(), ops._stream()
    O_ = F_ + 8192  # outputs of the valid calls at the end: the second half of f
    im2col = lambda B=1, Fr=1, H=4, W=4, Kpad=16, Lpad=4, xcn=2, ycn=2: (
        "sa_patch_im2col", (H_, 0, 16, 16, xcn, H_, 0, 16, 16, ycn, B, Fr, H, W, H_, Kpad, Lpad, st))
    unp = lambda Lpad=4, B=1, C=2, Fr=1, H=4, W=4: ("sa_unpatchify", (H_, 8, Lpad, B, C, Fr, H, W, F_, 0, st))
    lin = lambda M=1, N=4, K=8: ("sa_small_linear_f32", (F_, 8, M, H_, 8, F_, O_, 8, N, K, 0, 0, st))
    madd = lambda L=1, B=1, J=1, C=8: ("sa_mod_add", (F_, F_, 8, 8, O_, L, B, J, C, st))
    flow = lambda C=1, T=4, Fw=2, HW=4, start=0, overlap=0, prev_end=0, blend=0: (
        "sa_flow_step", (H_, H_, H_, 1, C, T, Fw, HW, start, 0.1, 0.0, 0.0, overlap, prev_end, F_, blend, st))
    bad = [
        im2col(B=0), im2col(Fr=0), im2col(H=0), im2col(W=-2), im2col(Kpad=0, xcn=0, ycn=0), im2col(Lpad=0, Fr=0),
        im2col(xcn=0), im2col(ycn=-1, Kpad=8),
        unp(Lpad=0), unp(B=0), unp(C=0), unp(Fr=-1), unp(H=0), unp(W=0),
        ("sa_timestep_embed", (F_, 0, 8, F_, st)), ("sa_timestep_embed", (F_, 2, 0, F_, st)),
        ("sa_timestep_embed", (F_, 2, -2, F_, st)),
        lin(M=0), lin(N=0), lin(N=-4), lin(K=0), lin(K=-8),
        madd(L=0), madd(B=0), madd(J=-1), madd(C=0),
        flow(C=0), flow(T=0, Fw=0), flow(Fw=0), flow(Fw=-1), flow(HW=0), flow(start=-1),
        flow(overlap=2, prev_end=1, blend=1), flow(overlap=0, blend=1), flow(Fw=5),
        ("sa_gather_rows", (F_, 16, I_, -1, F_, 16, 16, st)), ("sa_gather_rows", (F_, 16, I_, 2, F_, 16, 0, st)),
        ("sa_fill_f32", (F_, -1, 0.0, st)), ("sa_cast_f32_bf16", (F_, H_, -1, st)),
    ]
    for name, args in bad:
        with pytest.raises(KernelError, match="bad argument"):
            call(name, *args)
    _sync()
    # the same calls with valid sizes pass the check (so each refusal above is its bad value's)
    for name, args in (im2col(), unp(), ("sa_timestep_embed", (F_, 2, 8, O_, st)), lin(), madd(), flow(),
                       flow(overlap=2, prev_end=2, blend=1), ("sa_gather_rows", (F_, 16, I_, 2, F_, 16, 16, st))):
        call(name, *args)
    _sync()
