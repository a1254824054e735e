"""Every entry point of csrc/wav2vec.hip on its own against the references of tests/aux_ref.py (pinned on the
CPU by test_aux_ref_cpu.py), through the C ABI: the fused conv 0 + GroupNorm + GELU at time lengths around its
256-thread block, the im2col in both forms the encoder uses it in, the f32 += bf16 add.  Outputs are written into
larger, pre-filled allocations, and inputs carry NaN where the kernel must not read."""
import pytest
import torch

import aux_ref as R
from stableavatar_amd import ops
from stableavatar_amd._lib import KernelError, call

pytestmark = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ sa_w2v_conv0_gn_gelu

C0, K0, STRIDE0 = 5, 10, 5


@pytest.mark.parametrize("T", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("variant", ["exact", "spare", "dc"])
def test_w2v_conv0_gn_gelu(T, variant):
    """Conv1d(1, C, 10, stride 5) + GroupNorm(C, C) + exact GELU against F.conv1d + F.group_norm + F.gelu in fp64:
    rel-L2 < 1e-2 and every element within one bf16 ulp + 1e-3.  n_samples exactly (T - 1) stride + k (NaN
    behind the last sample) or with spare samples (which must not count); an input with a DC offset of 50 on unit
    noise, which a one-pass variance would lose; T = 1 leaves gelu(bias)."""
    g = torch.Generator().manual_seed(T)
    need = (T - 1) * STRIDE0 + K0
    n_samples = need + (13 if variant == "spare" else 0)
    audio = torch.randn(n_samples, generator=g) + (50.0 if variant == "dc" else 0.0)
    w = torch.randn(C0, K0, generator=g) * 0.3
    gw = torch.randn(C0, generator=g)
    gb = torch.randn(C0, generator=g)
    buf = torch.full((n_samples + 64,), NAN, device=dev)
    buf[:n_samples] = audio.to(dev)
    out = torch.full((T + 1, C0), 7.0, device=dev, dtype=torch.bfloat16)
    wd, gwd, gbd = w.to(dev), gw.to(dev), gb.to(dev)
    call("sa_w2v_conv0_gn_gelu", buf.data_ptr(), n_samples, wd.data_ptr(), C0, K0, STRIDE0, gwd.data_ptr(),
         gbd.data_ptr(), 1e-5, out.data_ptr(), T, ops._stream())
    _sync()
    ref = R.w2v_conv0_gn_gelu(audio, w, STRIDE0, gw, gb, float(torch.tensor(1e-5, dtype=torch.float32)), T)
    got = out[:T].double().cpu()
    d = (got - ref).abs()
    print(f"T={T} {variant}: rel-L2 {R.rel(got, ref):.3g}, max |d| - 2^-7 |ref| = "
          f"{(d - ref.abs() * 2.0 ** -7).max().item():.3g}")
    assert torch.isfinite(got).all()
    assert R.rel(got, ref) < 1e-2
    assert R.within_bf16_ulp(got, ref, 1e-3).all()
    if T == 1:
        assert R.within_bf16_ulp(got[0], torch.nn.functional.gelu(gb.double()), 1e-3).all()
    assert (out[T] == 7.0).all()


def test_w2v_conv0_rejects():
    T = 8
    need = (T - 1) * STRIDE0 + K0
    audio = torch.zeros(need + 64, device=dev)
    w = torch.zeros(C0, 65, device=dev)
    gw, gb = torch.ones(C0, device=dev), torch.zeros(C0, device=dev)
    out = torch.zeros(T, C0, device=dev, dtype=torch.bfloat16)
    st = ops._stream()
    with pytest.raises(KernelError, match="bad argument"):  # one sample short
        call("sa_w2v_conv0_gn_gelu", audio.data_ptr(), need - 1, w.data_ptr(), C0, K0, STRIDE0, gw.data_ptr(),
             gb.data_ptr(), 1e-5, out.data_ptr(), T, st)
    with pytest.raises(KernelError, match="bad argument"):  # the taps' LDS array holds 64
        call("sa_w2v_conv0_gn_gelu", audio.data_ptr(), need + 64, w.data_ptr(), C0, 65, STRIDE0, gw.data_ptr(),
             gb.data_ptr(), 1e-5, out.data_ptr(), 1, st)
    _sync()


# ------------------------------------------------------------------------------------------------ sa_conv1d_im2col

FORMS = {
    # groups, cg, k, stride, pad, T_in, ldx, col0, T_out, Kpad
    "feature": (1, 16, 3, 2, 0, 37, 24, 8, 18, 48),       # feature-encoder convs 1-6: a column slice, no padding
    "positional": (4, 8, 16, 1, 8, 19, 40, 8, 19, 136),  # grouped positional conv: zero rows both sides, Kpad > k cg
}


@pytest.mark.parametrize("form", list(FORMS))
def test_conv1d_im2col(form):
    """bit-exact against zero padding + an index gather; the columns outside [col0, col0 + groups cg) and the rows
    past T_in are NaN, the pad columns of the output zero, the allocation behind the output untouched"""
    groups, cg, k, stride, pad, T_in, ldx, col0, T_out, Kpad = FORMS[form]
    g = torch.Generator().manual_seed(k)
    x = torch.full((T_in + 4, ldx), NAN, dtype=torch.bfloat16)
    x[:T_in, col0:col0 + groups * cg] = torch.randn(T_in, groups * cg, generator=g).bfloat16()
    xd = x.to(dev)
    n = groups * T_out * Kpad
    out = torch.full((n + 64,), 7.0, device=dev, dtype=torch.bfloat16)
    call("sa_conv1d_im2col", xd.data_ptr(), ldx, T_in, col0, groups, cg, k, stride, pad, out.data_ptr(), T_out, Kpad,
         ops._stream())
    _sync()
    ref = R.conv1d_im2col(x, T_in, col0, groups, cg, k, stride, pad, T_out, Kpad)
    got = out[:n].view(groups, T_out, Kpad).cpu()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    assert (got[:, :, k * cg:] == 0).all()
    assert (out[n:] == 7.0).all()


def test_conv1d_im2col_rejects_misalignment():
    """each condition of the launcher's list on its own: the kernel moves 16-byte vectors"""
    groups, cg, k, stride, pad, T_in, ldx, col0, T_out, Kpad = FORMS["feature"]
    x = torch.zeros(T_in + 4, 32, device=dev, dtype=torch.bfloat16)
    out = torch.zeros(groups * T_out * 64 + 64, device=dev, dtype=torch.bfloat16)
    ok = dict(x=x.data_ptr(), ldx=ldx, T_in=T_in, col0=col0, groups=groups, cg=cg, k=k, stride=stride, pad=pad,
              out=out.data_ptr(), T_out=T_out, Kpad=Kpad)
    bad = [dict(cg=12), dict(Kpad=52), dict(Kpad=40), dict(ldx=28), dict(col0=4), dict(col0=16),
           dict(x=x.data_ptr() + 2), dict(out=out.data_ptr() + 2), dict(x=x.data_ptr() + 8),
           dict(T_in=0), dict(T_out=0), dict(groups=0), dict(k=0), dict(stride=0), dict(pad=-1)]
    for b in bad:
        a = dict(ok, **b)
        with pytest.raises(KernelError, match="bad argument"):
            call("sa_conv1d_im2col", a["x"], a["ldx"], a["T_in"], a["col0"], a["groups"], a["cg"], a["k"], a["stride"],
                 a["pad"], a["out"], a["T_out"], a["Kpad"], ops._stream())
    call("sa_conv1d_im2col", *[ok[n] for n in ("x", "ldx", "T_in", "col0", "groups", "cg", "k", "stride", "pad", "out",
                                               "T_out", "Kpad")], ops._stream())  # the unmodified call is accepted
    _sync()


# ------------------------------------------------------------------------------------------------ sa_add_f32_bf16

def test_add_f32_bf16():
    M, N, ldx, ldy = 7, 100, 104, 108
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(M, N, generator=g)
    y0 = torch.randn(M, N, generator=g).bfloat16()
    x = torch.full((M + 1, ldx), 7.0, device=dev)
    x[:M, :N] = x0.to(dev)
    y = torch.full((M, ldy), NAN, device=dev, dtype=torch.bfloat16)
    y[:, :N] = y0.to(dev)
    call("sa_add_f32_bf16", x.data_ptr(), ldx, y.data_ptr(), ldy, M, N, ops._stream())
    _sync()
    assert torch.equal(x[:M, :N].cpu(), R.add_f32_bf16(x0, y0))
    assert torch.equal(x[:M, :N].cpu(), x0 + y0.float())
    assert (x[:M, N:] == 7.0).all() and (x[M] == 7.0).all()
