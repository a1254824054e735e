"""sa_layernorm_mod and sa_qk_rmsnorm_rope (csrc/norm.hip), every element against the fp64 references of
tests/dit_ref.py (pinned on the CPU by test_dit_ref_cpu.py), through every kernel the launchers dispatch to: the
one-row-per-wave LayerNorm at its fixed (1536, 5120) and generic widths, the shared-modulation kernel with 8 and 16
rows per workgroup (SA_LN_SHARED, read per call) including its idle waves and its fall-back when a workgroup would
span two batch rows, the q+k pair kernel and the generic RMSNorm + RoPE kernel at widths 1536 / 5120 / any.  Outputs
are written into larger allocations pre-filled with a sentinel, strided inputs carry NaN where the kernel must not
read.

Bounds.  bf16 output: one bf16 ulp of the reference (2^-7 |ref| + 1e-6) on every element and at most 1 % of the
elements different at all (a correct fp32 evaluation: <= 0.007 % / 0.008 %, test_dit_ref_cpu.py).  fp32 output of the
LayerNorm: |got - ref| <= 4 r T with T the magnitude of the terms the value is summed from and r the largest
|fp32 restatement - ref| / T that a plain fp32 torch evaluation reaches at the same inputs (printed; 4 = the project's
margin for an fp32 evaluation in another order).  r is taken over two restatements that differ in how they sum a row
(torch's cascade, and a plain left-to-right loop): the largest ratio sits at the element whose normalised value is
closest to 0, where T vanishes and the error is the row mean's, so one evaluation's r is one draw of that row's mean
error and can be almost 0 by luck (with torch's sum alone, two of the 320 fp32 launches of test_layernorm_mod were
4.5 and 10.6 times their r on the MI355X, at C = 5120 where a lane adds 80 values in sequence)."""
import os

import pytest
import torch

import aux_ref as A
import dit_ref as R
from stableavatar_amd import ops
from stableavatar_amd._lib import KernelError, call
from stableavatar_amd.transformer import rope_table

pytestmark = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")
SENT = 7.0


def _sync():
    torch.cuda.synchronize()


def _shared(nw):
    """SA_LN_SHARED for the calls inside the `with`"""
    class _Env:
        def __enter__(self):
            self.old = os.environ.get("SA_LN_SHARED")
            os.environ["SA_LN_SHARED"] = str(nw)

        def __exit__(self, *a):
            if self.old is None:
                os.environ.pop("SA_LN_SHARED", None)
            else:
                os.environ["SA_LN_SHARED"] = self.old
    return _Env()


def _bits(t):
    """a view whose equality is bit equality (NaN pads included)"""
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ sa_layernorm_mod

def _ln_modes(w, b, shift, scale, gate, rpb, out_f32):
    d = lambda t: None if t is None else t.to(dev)
    modes = [("affine", dict(w=w, b=b)), ("affine-nobias", dict(w=w)),
             ("modulate", dict(shift=shift, scale=scale, rows_per_batch=rpb))]
    if out_f32:
        modes.append(("modulate-gate", dict(shift=shift, scale=scale, gate=gate, rows_per_batch=rpb)))
    return [(n, kw, dict(weight=d(kw.get("w")), bias=d(kw.get("b")), shift=d(kw.get("shift")), scale=d(kw.get("scale")),
                         gate=d(kw.get("gate")), rows_per_batch=kw.get("rows_per_batch", 0))) for n, kw in modes]


def _ln_check(got, x_cpu, eps, kw, out_f32, tag):
    """the bound of the module docstring; returns the share of differing elements (bf16) or r (fp32)"""
    ref, T = R.layernorm_mod(x_cpu, eps, out_bf16=not out_f32, **kw)
    got = got.double().cpu()
    assert torch.isfinite(got).all(), tag
    if not out_f32:
        share = (got != ref).double().mean().item()
        print(f"{tag}: {share:.4%} of the elements differ from the reference")
        assert A.within_bf16_ulp(got, ref, 1e-6).all(), tag
        assert share <= 0.01, tag
        return share
    r = 0.0
    for seq in (False, True):
        e32 = (R.layernorm_mod_f32(x_cpu, eps, seq=seq, **kw).double() - ref).abs()
        r = max(r, (e32[T > 0] / T[T > 0]).max().item() if (T > 0).any() else 0.0)
    e = (got - ref).abs()
    worst = (e[T > 0] / T[T > 0]).max().item() if (T > 0).any() else 0.0
    print(f"{tag}: r = {r:.3g} (fp32 restatement), kernel {worst:.3g}")
    assert (e <= 4 * r * T).all(), tag
    return r


@pytest.mark.parametrize("in_bf16,out_f32", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["f32-bf16", "f32-f32", "bf16-bf16",
                                                                                  "bf16-f32"])
@pytest.mark.parametrize("M", R.LN_ROWS)
@pytest.mark.parametrize("C", R.LN_WIDTHS)
def test_layernorm_mod(C, M, in_bf16, out_f32):
    """every width class (FIXED = 3, 10, generic with a partial 512-column chunk, a single partial chunk, one lane)
    x row counts that leave idle waves in the 4-, 8- and 16-row workgroups x the four dtype pairs, in four modes:
    affine with and without bias, AdaLN modulate, modulate + gated residual (fp32 output only); at C = 1536 each
    with SA_LN_SHARED = 0 / 8 / 16 (rows_per_batch = 16 for M > 16: two batch rows and a short last one).  ldx, ldo
    > C; the constant row (variance 0) must come out finite.
    Measured on the MI355X: bf16 output off the reference on at most 0.066 % of a case's elements (one element of
    a narrow case; the fp32 restatements: 0.0040 % pooled); fp32 output: the kernel's largest error / T at most
    1.55 r.  The r of the 320 fp32 launches, median / largest per mode over the widths 8, 72, 1280, 1536, 5120 (next
    to it the kernel's largest error / T): affine 1.1e-7 .. 1.6e-5 / 3.7e-4 (5.6e-5); affine without bias 2.2e-7 ..
    1.5e-2 / 24.6 (1.0); modulate 1.3e-7 .. 1.4e-4 / 1.1e-3 (5.4e-5); modulate + gate 7.5e-8 .. 1.5e-6 / 3.5e-6
    (2.9e-7).  Without a bias or a residual T vanishes where the normalised value does, the ratio there is the row
    mean's error over almost nothing, and r (set by the sequential restatement at C = 5120) is far above fp32's
    2^-24: on those elements the bound is loose, on all others it is a few 2^-24 T.  A launch that is one constant
    row has r = 0 and must be exact."""
    B = 2 if M > 16 else 1
    rpb = 16 if M > 16 else M
    if M > 1000:
        B, rpb = 2, 528
    x, w, b, shift, scale, gate = R.ln_inputs(M, C, B, C + M, in_bf16)
    ldx, ldo = C + 8, C + 24
    xin = torch.full((M, ldx), NAN, device=dev, dtype=x.dtype)
    xin[:, :C] = x.to(dev)
    odt = torch.float32 if out_f32 else torch.bfloat16
    for name, kw, gkw in _ln_modes(w, b, shift, scale, gate, rpb, out_f32):
        for nw in ((0, 8, 16) if C == 1536 else (8,)):
            out = torch.full((M + 16, ldo), SENT, device=dev, dtype=odt)
            with _shared(nw):
                ops.layernorm_mod(xin[:, :C], out[:M, :C], 1e-6, **gkw)
            _sync()
            _ln_check(out[:M, :C], x, 1e-6, kw, out_f32, f"C={C} M={M} {name} shared={nw}")
            assert (out[:M, C:] == SENT).all() and (out[M:] == SENT).all(), (name, nw)


@pytest.mark.parametrize("rpb", [528, 520, 519, 1040], ids=["rpb%16", "rpb%8", "rpb-odd", "rpb>M"])
@pytest.mark.parametrize("nw", [0, 8, 16])
def test_layernorm_mod_batch_rows(rpb, nw):
    """C = 1536, M = 1037: rows_per_batch divisible by 16 (both shared kernels), by 8 only (16 rows per workgroup
    must fall back to the per-wave kernel: a workgroup would span the batch boundary), by neither (both fall back),
    and larger than M; the last batch row is short in the first three.  The batch row decides which modulation
    vectors an element sees, so a wrong one is far outside the bound.  fp32 input, bf16 and fp32 (gated) output;
    also mod_bstride == 0 (one vector for every batch row)."""
    M, C = 1037, 1536
    B = -(-M // rpb)
    x, w, b, shift, scale, gate = R.ln_inputs(M, C, B, rpb)
    xin = x.to(dev)
    sh, sc, gt = shift.to(dev), scale.to(dev), gate.to(dev)
    for out_f32 in (0, 1):
        out = torch.full((M + 16, C), SENT, device=dev, dtype=torch.float32 if out_f32 else torch.bfloat16)
        kw = dict(shift=shift, scale=scale, rows_per_batch=rpb)
        with _shared(nw):
            ops.layernorm_mod(xin, out[:M], 1e-6, shift=sh, scale=sc, gate=gt if out_f32 else None, rows_per_batch=rpb)
        _sync()
        if out_f32:
            kw["gate"] = gate
        _ln_check(out[:M], x, 1e-6, kw, out_f32, f"rpb={rpb} shared={nw} f32={out_f32}")
        assert (out[M:] == SENT).all()
    # mod_bstride == 0: row 1 of the vectors, seen by every batch row
    out = torch.full((M + 16, C), SENT, device=dev, dtype=torch.bfloat16)
    with _shared(nw):
        ops.layernorm_mod(xin, out[:M], 1e-6, shift=sh[B - 1:].expand(B, C), scale=sc[B - 1:].expand(B, C),
                          rows_per_batch=rpb)
    _sync()
    _ln_check(out[:M], x, 1e-6, dict(shift=shift[B - 1:], scale=scale[B - 1:], rows_per_batch=M), 0,
              f"rpb={rpb} shared={nw} bstride=0")
    assert (out[M:] == SENT).all()


@pytest.mark.parametrize("C,nw", [(1536, 0), (1536, 8), (1536, 16), (1280, 8), (72, 8)])
@pytest.mark.parametrize("mode", ["f32", "f32-gate", "bf16"])
def test_layernorm_mod_in_place(C, nw, mode):
    """out == x, as the vocal projector, the encoders and wav2vec call it: fp32 -> fp32 affine, fp32 -> fp32
    modulate + gated residual (which reads x twice), bf16 -> bf16 affine.  A row is loaded whole before any of it
    is stored, so the result is the out-of-place one; the NaN pad columns and the rows past M stay as they were."""
    M, B, rpb = 21, 2, 16
    x, w, b, shift, scale, gate = R.ln_inputs(M, C, B, C + 1, mode == "bf16")
    ld = C + 8
    buf = torch.full((M + 16, ld), NAN, device=dev, dtype=x.dtype)
    buf[:M, :C] = x.to(dev)
    v = buf[:M, :C]
    if mode == "f32-gate":
        kw = dict(shift=shift, scale=scale, gate=gate, rows_per_batch=rpb)
        gkw = dict(shift=shift.to(dev), scale=scale.to(dev), gate=gate.to(dev), rows_per_batch=rpb)
    else:
        kw, gkw = dict(w=w, b=b), dict(weight=w.to(dev), bias=b.to(dev))
    with _shared(nw):
        ops.layernorm_mod(v, v, 1e-5, **gkw)
    _sync()
    _ln_check(v, x, 1e-5, kw, mode != "bf16", f"in place C={C} shared={nw} {mode}")
    assert torch.isnan(buf[:M, C:]).all() and torch.isnan(buf[M:]).all()


def test_layernorm_mod_rejects():
    x = torch.zeros(4, 1536, device=dev)
    o = torch.zeros(4, 1536, device=dev, dtype=torch.bfloat16)
    v = torch.zeros(1, 1536, device=dev)
    with pytest.raises(KernelError, match="bad argument"):  # gate needs fp32 output
        ops.layernorm_mod(x, o, 1e-6, shift=v, scale=v, gate=v, rows_per_batch=4)
    with pytest.raises(KernelError, match="bad argument"):  # scale without rows_per_batch
        ops.layernorm_mod(x, o, 1e-6, shift=v, scale=v)
    with pytest.raises(KernelError, match="bad argument"):  # C % 8
        ops.layernorm_mod(x[:, :1532], o[:, :1532], 1e-6)
    _sync()


# ------------------------------------------------------------------------------------------------ sa_qk_rmsnorm_rope

def _qk_run(qkv, wq, wk, C, hd, with_k, rope, off, ldx_pad=8, split_k=False):
    """the launch on a [QK_M + 1, 3 C + pad] buffer (NaN pad, one row past M); returns (buffer before, after).
    split_k: q and k by two q-only calls (the generic kernel by dispatch)"""
    M = qkv.shape[0]
    buf = torch.full((M + 1, 3 * C + ldx_pad), NAN, device=dev, dtype=torch.bfloat16)
    buf[:M, :3 * C] = qkv.to(dev)
    before = buf.clone()
    nf, nh = R.rope_split(hd)
    kw = dict(rope=rope_table(hd).to(dev) if rope else None, rows_per_batch=R.QK_RPB, tok_offset=off, grid=R.QK_GRID,
              head_dim=hd, n_frame_pairs=nf, n_height_pairs=nh, M=M)
    wq, wk = wq.to(dev), wk.to(dev)
    if split_k:
        ops.qk_rmsnorm_rope(buf, 0, -1, wq, None, C, 1e-6, **kw)
        ops.qk_rmsnorm_rope(buf, C, -1, wk, None, C, 1e-6, **kw)
    else:
        ops.qk_rmsnorm_rope(buf, 0, C if with_k else -1, wq, wk if with_k else None, C, 1e-6, **kw)
    _sync()
    return before, buf


def _qk_check(buf, before, qkv, wq, wk, C, hd, with_k, rope, off, tag):
    """q (and k) within 2^-7 |ref| + 2^-20 (|re| + |im|) of the reference, at most 1 % different; everything else
    in the buffer bit for bit as before"""
    M = qkv.shape[0]
    nf, nh = R.rope_split(hd)
    tab = rope_table(hd) if rope else None
    done = C * (2 if with_k else 1)
    for col, w in ((0, wq), (C, wk))[:2 if with_k else 1]:
        ref, mag = R.qk_rmsnorm_rope(qkv[:, col:col + C], w, 1e-6, tab, hd, R.QK_GRID, off, R.QK_RPB, nf, nh)
        got = buf[:M, col:col + C].double().cpu()
        share = (got != ref).double().mean().item()
        print(f"{tag} col {col}: {share:.4%} of the elements differ from the reference")
        assert torch.isfinite(got).all(), tag
        assert ((got - ref).abs() <= 2.0 ** -7 * ref.abs() + 2.0 ** -20 * mag).all(), tag
        assert share <= 0.01, tag
    assert torch.equal(_bits(buf[:M, done:]), _bits(before[:M, done:])), tag  # (k,) v and the pad columns
    assert torch.equal(_bits(buf[M]), _bits(before[M])), tag


@pytest.mark.parametrize("name,C,hd,with_k,rope,off", R.QK_CASES, ids=[c[0] for c in R.QK_CASES])
def test_qk_rmsnorm_rope(name, C, hd, with_k, rope, off):
    """every kernel of the launcher: the q+k pair kernel (C = 1536, head_dim 128, RoPE), qk_rmsnorm_rope_kernel<3>
    with q only (the cross-attention norms), <10> (the 14B width), <0> (640 with head_dim 64; 72 without RoPE).
    46 rows = two batch rows of 23 (not a multiple of the 4 rows of a workgroup), grid 3 x 4 x 5 so that a swapped
    axis moves an angle, token offsets 0 / 37 and 50 (the first unrotated token in the middle of the launch).
    Measured on the MI355X: at most 0.0071 % of a case's elements off the reference (the fp32 restatement: 0.0020 %
    pooled)."""
    qkv, wq, wk = R.qk_inputs(R.QK_M, C, C + off)
    before, buf = _qk_run(qkv, wq, wk, C, hd, with_k, rope, off)
    _qk_check(buf, before, qkv, wq, wk, C, hd, with_k, rope, off, name)


@pytest.mark.parametrize("off", [0, 37, 50])
def test_qk_pair_kernel_vs_generic_kernel(off):
    """qk_rmsnorm_rope_pair_kernel against qk_rmsnorm_rope_kernel<3> without the environment: one call with q_col =
    0, k_col = C takes the pair kernel, two calls with k_col = -1 (the q columns, then the k columns with wk) take
    the generic one by dispatch.  Both satisfy the reference bound, and they agree to one bf16 ulp (on the MI355X
    they are bit-identical at these inputs)."""
    C, hd = 1536, 128
    qkv, wq, wk = R.qk_inputs(R.QK_M, C, 11 + off)
    outs = []
    for split in (False, True):
        before, buf = _qk_run(qkv, wq, wk, C, hd, True, True, off, split_k=split)
        _qk_check(buf, before, qkv, wq, wk, C, hd, True, True, off, f"off={off} generic={split}")
        outs.append(buf[:R.QK_M, :2 * C].double().cpu())
    assert A.within_bf16_ulp(outs[0], outs[1], 1e-6).all()
    print(f"off={off}: pair and generic differ on {(outs[0] != outs[1]).double().mean().item():.4%}")


def _qk_same_columns(x, wq, wk, off, two_calls=False):
    """q_col == k_col == 0 on a copy of x [M, C] (C = 1536): one launch, or the two q-only launches (wq, then wk)
    that take qk_rmsnorm_rope_kernel<3> by dispatch.  Returns the [M + 1, C + 8] buffer."""
    M, C = x.shape
    buf = torch.full((M + 1, C + 8), NAN, device=dev, dtype=torch.bfloat16)
    buf[:M, :C] = x.to(dev)
    nf, nh = R.rope_split(128)
    kw = dict(rope=rope_table(128).to(dev), rows_per_batch=R.QK_RPB, tok_offset=off, grid=R.QK_GRID, head_dim=128,
              n_frame_pairs=nf, n_height_pairs=nh, M=M)
    wq, wk = wq.to(dev), wk.to(dev)
    if two_calls:
        ops.qk_rmsnorm_rope(buf, 0, -1, wq, None, C, 1e-6, **kw)
        ops.qk_rmsnorm_rope(buf, 0, -1, wk, None, C, 1e-6, **kw)
    else:
        ops.qk_rmsnorm_rope(buf, 0, 0, wq, wk, C, 1e-6, **kw)
    _sync()
    return buf


@pytest.mark.parametrize("off", [0, 50])
def test_qk_generic_switch_is_read_per_call(off, monkeypatch):
    """SA_QK_GENERIC changes the kernel of sa_qk_rmsnorm_rope at the next call of the same process.  At the DiT's
    arguments the pair and the generic kernel give the same bytes (test_qk_pair_kernel_vs_generic_kernel), so the
    choice is made visible by a launch on which they must differ: k_col == q_col.  The pair kernel loads q and k
    (the same columns) before it stores either and stores k last, so a row ends as norm_rope(x, wk); the generic
    kernel normalises the columns in place with wq and then what it stored with wk, norm_rope(norm_rope(x, wq), wk)
    -- the bytes of two q-only launches, which are generic by dispatch.  Each lane reads back only columns it
    wrote itself, so both are deterministic.  Without the variable the launch gives the first, with it the
    second, without it again the first.
    Only this launcher's reading of the switch is observed: sa_qk_rmsnorm_rope_mxfp8 and sa_qkv_pack call the same
    helper, but neither writes q back into x, so their pair and generic kernels give the same bytes on every input
    and no test can tell which one ran."""
    C, hd = 1536, 128
    nf, nh = R.rope_split(hd)
    qkv, wq, wk = R.qk_inputs(R.QK_M, C, 5 + off)
    x = qkv[:, :C]
    monkeypatch.delenv("SA_QK_GENERIC", raising=False)
    pair = _qk_same_columns(x, wq, wk, off)
    gen = _qk_same_columns(x, wq, wk, off, two_calls=True)
    # what each is: the pair kernel's against the reference of norm_rope(x, wk) ...
    ref, mag = R.qk_rmsnorm_rope(x, wk, 1e-6, rope_table(hd), hd, R.QK_GRID, off, R.QK_RPB, nf, nh)
    got = pair[:R.QK_M, :C].double().cpu()
    assert ((got - ref).abs() <= 2.0 ** -7 * ref.abs() + 2.0 ** -20 * mag).all()
    # ... and the generic kernel's far from it: normalised and rotated twice
    differ = (_bits(gen[:R.QK_M, :C]) != _bits(pair[:R.QK_M, :C])).double().mean().item()
    print(f"off={off}: k_col == q_col, pair and generic kernel differ on {differ:.1%} of the elements")
    assert differ > 0.5
    monkeypatch.setenv("SA_QK_GENERIC", "1")
    switched = _qk_same_columns(x, wq, wk, off)
    monkeypatch.delenv("SA_QK_GENERIC")
    back = _qk_same_columns(x, wq, wk, off)
    assert torch.equal(_bits(switched), _bits(gen))
    assert torch.equal(_bits(back), _bits(pair))
    assert not torch.equal(_bits(switched), _bits(back))


def test_qk_rmsnorm_rope_rejects():
    x = torch.zeros(8, 3 * 1536, device=dev, dtype=torch.bfloat16)
    w = torch.zeros(1536, device=dev)
    rope = rope_table(128).to(dev)
    with pytest.raises(KernelError, match="bad argument"):  # k without its weight
        ops.qk_rmsnorm_rope(x, 0, 1536, w, None, 1536, 1e-6)
    with pytest.raises(KernelError, match="bad argument"):  # RoPE without rows_per_batch
        ops.qk_rmsnorm_rope(x, 0, 1536, w, w, 1536, 1e-6, rope=rope, grid=(1, 2, 2))
    with pytest.raises(KernelError, match="bad argument"):  # an empty grid axis
        ops.qk_rmsnorm_rope(x, 0, 1536, w, w, 1536, 1e-6, rope=rope, rows_per_batch=8, grid=(1, 0, 2))
    with pytest.raises(KernelError, match="bad argument"):  # M == 0
        ops.qk_rmsnorm_rope(x, 0, 1536, w, w, 1536, 1e-6, M=0)
    _sync()
