"""The fp8 FFN mode on the GPU: the quantiser and the fused LayerNorm bit-exact against the definition
(stableavatar_amd/mxfp8.py), the MXFP8 GEMM exact on integer data (lane map, scale bytes, K pipeline, ragged
tiles) and within the fp32-accumulation bound on random data, its MXFP8 epilogue bit-exact, and the DiT with
enable_fp8_ffn() against the CPU oracle with the same two Linears emulated (single GPU, qfloat8 weights, SP)."""
import functools
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from mp_util import collect  # noqa: E402
from mxfp8_util import cos, full_dims_case, rel, small_case  # noqa: E402

from stableavatar_amd import mxfp8, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mx(q, s):
    return ops.Mx8(q.to(DEV), s.to(DEV))


def _quant_data(M, K, seed):
    """bf16 [M, K]: block magnitudes 2^-20 .. 2^10, negatives, all-zero blocks, blocks with amax = 448 * 2^j and
    256 * 2^j exactly, and members 2^-14 .. 2^-17 of their block's size (e4m3 subnormals / underflow to +-0)"""
    g = torch.Generator().manual_seed(seed)
    nb = K // 32
    jb = torch.randint(-20, 11, (M, nb), generator=g)
    x = torch.randn(M, K, generator=g) * torch.exp2(jb.float()).repeat_interleave(32, 1)
    x[:, 3::8] *= torch.exp2(-torch.randint(14, 18, (M, K // 8), generator=g).float())
    xb = x.reshape(M, nb, 32)
    kind = torch.arange(M * nb).reshape(M, nb) % 5
    xb[kind == 1] = 0
    for k, top in ((2, 448.0), (3, 256.0)):
        sel = kind == k
        xb[sel] *= 0.2 / xb[sel].abs().amax(-1, keepdim=True).clamp_min(1e-30) * torch.exp2(jb[sel].float())[:, None]
        t = xb[sel]
        t[:, 7] = -top * torch.exp2(jb[sel].float())
        xb[sel] = t
    return xb.reshape(M, K).bfloat16()


@pytest.mark.parametrize("K", [128, 1536])
@pytest.mark.parametrize("M", [1, 33, 300])
def test_quant_bit_exact(M, K):
    x = _quant_data(M, K, 7 * M + K)
    buf = torch.zeros(M, K + 64, dtype=torch.bfloat16, device=DEV)
    buf[:, :K] = x.to(DEV)
    out = ops.mxfp8_quant(buf[:, :K])
    q, s = mxfp8.quantize(x)
    assert torch.equal(out.s.cpu(), s)
    assert torch.equal(out.q.cpu(), q)
    if M >= 33:  # the data is what it claims
        e = s.to(torch.int32) - 127
        assert (s == 127).any() and e.min() < -15 and e.max() > 0 and (q == 0x80).any()


@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["modulate", "affine"])
def test_layernorm_mxfp8_bit_exact(mode, in_dtype):
    M, C, rpb = 300, 1536, 100
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(M, C, generator=g) * 3 + 0.5).to(in_dtype).to(DEV)
    kw = dict(rows_per_batch=rpb)
    if mode == "modulate":
        mod = (torch.randn(3, 2, C, generator=g) * 0.5).to(DEV)
        kw.update(shift=mod[:, 0], scale=mod[:, 1])
    else:
        kw.update(weight=(1 + 0.3 * torch.randn(C, generator=g)).to(DEV), bias=(0.2 * torch.randn(C, generator=g)).to(DEV))
    ref_bf = ops.layernorm_mod(x, torch.empty(M, C, dtype=torch.bfloat16, device=DEV), 1e-6, **kw)
    ref = ops.mxfp8_quant(ref_bf)
    out = ops.layernorm_mod_mxfp8(x, ops.Mx8.empty(M, C, DEV), 1e-6, **kw)
    assert torch.equal(out.s, ref.s) and torch.equal(out.q, ref.q)


def _int_operand(rows, K, seed, identity=False):
    """integer elements in [-8, 8] as e4m3 bytes and block scales 2^j, j in [-3, 3], varying per row and per block;
    returns (q uint8, s uint8, the values times 8 as int64).  Asymmetric in row and column.  Two of every three
    elements are in [-1, 1] so that every partial sum of a product stays below 2^24 units (asserted by the test)."""
    r = torch.arange(rows)[:, None]
    k = torch.arange(K)[None, :]
    if identity:
        v = torch.where(k == r % K, (r % 8) + 1, 0) * torch.where(r % 2 == 0, 1, -1)
    else:
        big = (r * 7 + k * 3 + seed) % 17 - 8
        small = (r * 5 + k * 11 + seed) % 3 - 1
        v = torch.where((r + 2 * k + seed) % 3 == 0, big, small)
    j = (r * 3 + (k // 32) * 5 + seed) % 7 - 3
    q = v.float().to(torch.float8_e4m3fn).view(torch.uint8)
    s = (j[:, ::32] + 127).to(torch.uint8)
    return q.contiguous(), s.contiguous(), (v * torch.exp2((j + 3).float()).long()).long()


@pytest.mark.parametrize("K", [128, 256, 1536])
@pytest.mark.parametrize("N", [32, 160, 288])
@pytest.mark.parametrize("M", [16, 257, 300])
@pytest.mark.parametrize("a_identity", [False, True], ids=["pattern", "identity"])
def test_gemm_exact_integers(a_identity, M, N, K):
    """products and sums of small integers times powers of two are exact in fp32: the result must equal the int64
    reference exactly -- a wrong lane map, scale byte, dropped K step or ragged-tile error cannot hide"""
    aq, as_, a8 = _int_operand(M, K, 1, identity=a_identity)
    wq, ws, w8 = _int_operand(N, K, 2)
    assert (a8.abs() @ w8.abs().T).max() < 2 ** 24  # every partial sum, in units of 2^-6
    ref = (a8 @ w8.T).double() / 64
    out = ops.linear_mxfp8(_mx(aq, as_), _mx(wq, ws), None, ops.EPI_F32)
    assert torch.equal(out.double().cpu(), ref), (out.double().cpu() - ref).abs().max()


@functools.lru_cache(maxsize=None)
def _random_problem():
    """operands, bias, the fp64 product of the dequantised operands and the fp32-accumulation bound
    K 2^-23 (|A| |W|^T): products of two e4m3 values (times powers of two) are exact in fp32, so only the
    accumulation contributes"""
    M, N, K = 300, 288, 1536
    g = torch.Generator().manual_seed(3)
    a = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    aq, as_ = mxfp8.quantize(a)
    wq, ws = mxfp8.quantize(w)
    ad, wd = mxfp8.dequantize(aq, as_).double(), mxfp8.dequantize(wq, ws).double()
    bias = torch.randn(N, generator=g) * 0.5
    return _mx(aq, as_), _mx(wq, ws), bias, ad @ wd.T, K * 2.0 ** -23 * (ad.abs() @ wd.abs().T)


def _bf16_round(x):
    return x.float().bfloat16().double()


def _rounded_linear(a, w, bias, lin, bound):
    """The bf16 rounding of the Linear output that the bf16 epilogues consume.  Any fp32 value within the accumulation
    bound of the fp64 product is a legitimate Linear output, so every bf16 value x in [bf16(lin - bound),
    bf16(lin + bound)] is a legitimate rounding (the bound spans a few bf16 steps), and an epilogue is right if it
    matches the emulation for one of them.  The witness tried is the rounding of the kernel's own fp32 output
    (SA_EPI_F32, the same accumulators and bias add); it is first checked to lie in that window."""
    x = ops.linear_mxfp8(a, w, bias.to(DEV), ops.EPI_F32).bfloat16().double().cpu()
    assert (x >= _bf16_round(lin - bound)).all() and (x <= _bf16_round(lin + bound)).all()
    return x


def _gelu_tanh64(t):
    """nn.GELU('tanh') in fp64 as t * sigmoid(2u), u = sqrt(2/pi) (t + 0.044715 t^3): the same function as
    0.5 t (1 + tanh u) without its cancellation for t << 0 (where 1 + tanh u loses every digit, in fp64 too)"""
    u = 0.7978845608028654 * (t + 0.044715 * t ** 3)
    return t * torch.sigmoid(2 * u)


def _with_bias():
    """_random_problem with the bias added: one more fp32 addition in the bound"""
    a, w, bias, lin, bound = _random_problem()
    K = a.shape[1]
    return a, w, bias, lin + bias.double(), (bound + 2.0 ** -23 * bias.abs().double()) * (K + 1) / K


def test_gemm_random_f32():
    a, w, _, lin, bound = _random_problem()
    out = ops.linear_mxfp8(a, w, None, ops.EPI_F32).double().cpu()
    err = (out - lin).abs()
    print(f"EPI_F32: max err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()


def test_gemm_random_gelu_bf16():
    a, w, bias, lin, bound = _with_bias()
    out = ops.linear_mxfp8(a, w, bias.to(DEV), ops.EPI_GELU_TANH_BF16).double().cpu()
    x = _rounded_linear(a, w, bias, lin, bound)
    ref = _gelu_tanh64(x)
    # one bf16 rounding of the output: 2^-8 |ref|.  The kernels form x / (1 + exp2(z)) in fp32 (common.h gelu_tanh,
    # the bf16 GEMM's too): exp2 overflows at 2^128, so an output below |x| 2^-128 is zero -- |x| 2^-127 absolute
    err = (out - ref).abs()
    nz = ref.abs() > 2.0 ** -100
    print(f"EPI_GELU_TANH_BF16: max err / |ref| {(err[nz] / ref.abs()[nz]).max():.3e} (2^-8 = {2.0 ** -8:.3e})")
    assert (err <= 2.0 ** -8 * ref.abs() + x.abs() * 2.0 ** -127).all()


def test_gemm_random_res_f32_in_place():
    a, w, bias, lin, bound = _with_bias()
    M, N = lin.shape
    g = torch.Generator().manual_seed(4)
    res = torch.randn(M, N, generator=g)
    gate = torch.randn(3, N, generator=g)
    x = res.clone().to(DEV)
    ops.linear_mxfp8(a, w, bias.to(DEV), ops.EPI_RES_F32, out=x, residual=x, gate=gate.to(DEV), rows_per_batch=100)
    out = x.double().cpu()
    gr = gate.double().repeat_interleave(100, 0)
    tg = _rounded_linear(a, w, bias, lin, bound) * gr
    ref = res.double() + tg
    # the fp32 product t g and the sum r + t g: half an ulp each, 2^-24 (|t g| + |r + t g|)
    tol = 2.0 ** -24 * 1.001 * (res.abs().double() + 2 * tg.abs())
    err = (out - ref).abs()
    print(f"EPI_RES_F32 in place: max err / tol {(err / tol).max():.3f}")
    assert (err <= tol).all()


@pytest.mark.parametrize("N", [288, 8960])
def test_gemm_gelu_mxfp8_epilogue_bit_exact(N):
    M, K = 300, 1536
    g = torch.Generator().manual_seed(N)
    rows = torch.exp2(torch.randint(-4, 3, (M, 1), generator=g).float())  # output blocks over several scales
    a = ops.mxfp8_quant((torch.randn(M, K, generator=g) * 2 * rows).bfloat16().to(DEV))
    w = ops.mxfp8_quant((torch.randn(N, K, generator=g) * 0.04).bfloat16().to(DEV))
    bias = (torch.randn(N, generator=g) * 0.5).to(DEV)
    ref = ops.mxfp8_quant(ops.linear_mxfp8(a, w, bias, ops.EPI_GELU_TANH_BF16))
    out = ops.linear_mxfp8(a, w, bias, ops.EPI_GELU_TANH_MXFP8)
    assert torch.equal(out.s, ref.s) and torch.equal(out.q, ref.q)
    assert len(torch.unique(out.s)) > 3


# ------------------------------------------------------------------------------------------------ the DiT

def _make(cfg, P, qfloat8=False):
    from test_gpu_dit import make_model
    m = make_model(cfg, {k: v.clone() for k, v in P.items()})
    if qfloat8:
        for name, p in m.named_parameters():
            if "modulation" not in name:
                p.data = p.data.to(torch.float8_e4m3fn)
    return m


def test_dit_small_fp8_ffn():
    from golden_cases import DIT_SMALL
    from test_gpu_dit import run
    P, inp, emu = small_case("full", True)
    fresh = run(_make(DIT_SMALL, P), inp)
    m = _make(DIT_SMALL, P)
    off0 = run(m, inp)  # packs the bf16 weights first: the toggle must re-pack
    m.enable_fp8_ffn()
    on = run(m, inp)
    r, c = rel(on, emu), cos(on, emu)
    print(f"DIT_SMALL fp8 FFN vs emulated oracle: rel-L2 {r:.3e} cosine {c:.6f}; vs mode off {rel(on, off0):.3e}")
    assert r < 2e-2 and c > 0.9995, (r, c)
    assert not torch.equal(on, off0)
    m.enable_fp8_ffn(False)
    assert torch.equal(run(m, inp), fresh) and torch.equal(off0, fresh)


def test_dit_full_dims_fp8_ffn():
    """30 layers, ffn 8960 at a tiny grid (as test_dit_full_dims_vs_oracle)"""
    from test_gpu_dit import run
    cfg, P, inp, emu = full_dims_case()
    m = _make(cfg, P)
    m.enable_fp8_ffn()
    on = run(m, inp)
    r, c = rel(on, emu), cos(on, emu)
    print(f"CONFIG_1_3B fp8 FFN vs emulated oracle: rel-L2 {r:.3e} cosine {c:.6f}")
    assert r < 2e-2 and c > 0.9995, (r, c)


def test_dit_qfloat8_weights_fp8_ffn():
    from golden_cases import DIT_SMALL
    from test_gpu_dit import run
    P, inp, emu = small_case("full", True, True)
    m = _make(DIT_SMALL, small_case("full", False)[0], qfloat8=True)
    m.enable_fp8_ffn()
    on = run(m, inp)
    r, c = rel(on, emu), cos(on, emu)
    assert r < 2e-2 and c > 0.9995, (r, c)


def _sp_worker(rank, world, port, qret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    import torch.distributed as dist
    sys.path.insert(0, HERE)
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        from golden_cases import DIT_SMALL
        from test_gpu_dit import run
        P, inp, emu = small_case("full", True)
        m = _make(DIT_SMALL, P)
        m.enable_fp8_ffn()
        single = run(m, inp)
        m.enable_multi_gpus_inference()
        par = run(m, inp)
        qret.put((rank, rel(par, emu), cos(par, emu), rel(par, single), bool(torch.isfinite(par).all())))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sp_world2_fp8_ffn():
    """gloo world 2 sharing the GPU, the default exchange schedule (per-row streams: _sp_block_streams), as
    tests/test_gpu_sp.py drives it and with its tolerances"""
    from test_gpu_sp import _rendezvous_file
    world = 2
    ctx = mp.get_context("spawn")
    qret = ctx.Queue()
    port = _rendezvous_file()
    procs = [ctx.Process(target=_sp_worker, args=(r, world, port, qret)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, qret, world, timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, e_emu, c_emu, e_single, finite in res:
        print(f"rank {rank}: vs emulated oracle rel {e_emu:.2e} cos {c_emu:.6f}, vs single-GPU {e_single:.1e}")
        assert finite
        assert e_emu < 2e-2 and c_emu > 0.9995, (rank, e_emu, c_emu)
        assert e_single < 1e-3, (rank, e_single)
