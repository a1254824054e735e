"""The fp8 q/k/v mode on the GPU: the three kernels that write the fp8 attention's operands where their values are made,
each bit-exact against the pair of calls it replaces (and, for the V^T GEMM, against the definition on the CPU and an
exact-integer product); the DiT with enable_fp8_qkv() against the CPU oracle with the same Linears emulated; the fused
chain byte-identical to the unfused one; all three fp8 modes together; sequence parallel; the CLI flag."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from fp8_qkv_util import cos, full_dims_case, oracle_forward, rel, small_case  # noqa: E402
from mp_util import collect  # noqa: E402

from stableavatar_amd import mxfp8_attn, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128
BAR = dict(rel=2e-2, cos=0.9995)  # the project's bar for a quantised mode against its emulated oracle


def _tables(segs):
    vcol0, Rv = ops.attn_vcol0(segs)
    return (torch.tensor(segs, dtype=torch.int32, device=DEV), torch.tensor(vcol0, dtype=torch.int32, device=DEV), Rv,
            max(s[1] for s in segs), max(s[3] for s in segs))


# ------------------------------------------------------------------------------------------------ sa_gemm_mxfp8_vt

GUARD = 0xA5


def _vt_buf(M, N, rps, nseg):
    """operand buffers with one 128-column guard band past the segments' columns, every byte preset"""
    c128 = mxfp8_attn.ceil128(rps)
    buf = ops.AttnMx8(M, M, N // D, nseg * c128 + 128, nseg, DEV)
    buf.vq.fill_(GUARD)
    buf.vs.fill_(GUARD)
    return buf, c128


def _check_vt(buf, v_rows, rps, nseg, c128, what):
    """every byte and scale of every segment's ceil128 columns against mxfp8_attn.quant_vt of its bf16 rows"""
    vq, vs = buf.vq.cpu(), buf.vs.cpu()
    for s in range(nseg):
        wq, wsc = mxfp8_attn.quant_vt(v_rows[s * rps:(s + 1) * rps])
        assert torch.equal(vs[:, s * c128 // 32:(s + 1) * c128 // 32], wsc), (what, s, "scales")
        assert torch.equal(vq[:, s * c128:(s + 1) * c128], wq), (what, s, "bytes")
    assert (vq[:, nseg * c128:] == GUARD).all() and (vs[:, nseg * c128 // 32:] == GUARD).all()  # nothing past them


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("rps", [128, 300, 513])
def test_gemm_vt_bit_exact(rps, nseg, N, K):
    """the witness is the kernel's own bf16 output (sa_gemm_mxfp8 SA_EPI_BF16, the same accumulators): V^T must be the
    definition's quantisation of exactly those rows, zero padding and zero-block scales included"""
    M = rps * nseg
    g = torch.Generator().manual_seed(rps + 7 * nseg + N + K)
    rows = torch.exp2(torch.randint(-5, 4, (M, 1), generator=g).float())  # a V^T block mixes keys of several scales
    a = ops.mxfp8_quant((torch.randn(M, K, generator=g) * rows).bfloat16().to(DEV))
    w = ops.mxfp8_quant((torch.randn(N, K, generator=g) * 0.1).bfloat16().to(DEV))
    bias = (torch.randn(N, generator=g) * 0.5).to(DEV)
    v = ops.linear_mxfp8(a, w, bias, ops.EPI_BF16).cpu()
    buf, c128 = _vt_buf(M, N, rps, nseg)
    ops.linear_mxfp8_vt(a, w, bias, rps, nseg, buf)
    torch.cuda.synchronize()
    _check_vt(buf, v, rps, nseg, c128, (rps, nseg, N, K))
    if rps % 128:  # keys past the segment's end: zero bytes
        pad = mxfp8_attn.KEY_OF_POS >= rps - (c128 - 128)
        assert (buf.vq[:, c128 - 128:c128].cpu()[:, pad] == 0).all()
    assert len(torch.unique(buf.vs[:, :nseg * c128 // 32])) > 3


def test_gemm_vt_exact_integers():
    """small integers, unit scales: the fp32 product is exact, so V^T must be the fp64 product put through the
    definition -- a wrong lane map, key position or segment tiling cannot hide behind the witness"""
    rps, nseg, N, K = 300, 2, 256, 256
    M = rps * nseg
    r, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    av = torch.where((r + 2 * k) % 3 == 0, (r * 7 + k * 3) % 17 - 8, (r * 5 + k * 11) % 3 - 1)
    n = torch.arange(N)[:, None]
    wv = torch.where((n + k) % 4 == 0, (n * 3 + k * 5) % 9 - 4, (n + k * 7) % 3 - 1)
    e4 = lambda t: t.float().to(torch.float8_e4m3fn).view(torch.uint8).contiguous().to(DEV)  # noqa: E731
    unit = lambda rows: torch.full((rows, K // 32), 127, dtype=torch.uint8, device=DEV)  # noqa: E731
    prod = av.double() @ wv.double().T
    assert (av.abs().double() @ wv.abs().double().T).max() < 2 ** 24
    buf, c128 = _vt_buf(M, N, rps, nseg)
    ops.linear_mxfp8_vt(ops.Mx8(e4(av), unit(M)), ops.Mx8(e4(wv), unit(N)), None, rps, nseg, buf)
    torch.cuda.synchronize()
    _check_vt(buf, prod.float().bfloat16(), rps, nseg, c128, "integers")


# ------------------------------------------------------------------------------------------------ RMSNorm + RoPE -> Q

@pytest.mark.parametrize("C,with_rope", [(1536, True), (384, True), (5120, True), (1536, False)],
                         ids=["pair1536", "generic384", "fixed5120", "norope1536"])
def test_qk_rmsnorm_rope_mxfp8_bit_exact(C, with_rope):
    """= sa_qk_rmsnorm_rope on a copy, then the Q third of the pack; K byte-identical to the in-place kernel's; q and v
    of the buffer untouched.  37 rows (not a multiple of the 4 rows per workgroup), 19 per batch row, a 16-token
    grid: rows with t >= 16 go unrotated"""
    from stableavatar_amd.transformer import rope_table
    M, rpb, heads = 37, 19, C // D
    g = torch.Generator().manual_seed(C)
    mag = torch.exp2(torch.randint(-4, 4, (M, 3 * C // 32), generator=g).float()).repeat_interleave(32, 1)
    x = (torch.randn(M, 3 * C, generator=g) * mag).bfloat16().to(DEV)
    wq = (1 + 0.3 * torch.randn(C, generator=g)).to(DEV)
    wk = (1 + 0.3 * torch.randn(C, generator=g)).to(DEV)
    kw = dict(rows_per_batch=rpb, tok_offset=0, grid=(4, 2, 2), head_dim=D, n_frame_pairs=D // 2 - 2 * (D // 6),
              n_height_pairs=D // 6)
    if with_rope:
        kw["rope"] = rope_table(D).to(DEV)
    segs = [[0, M, 0, M]]
    st, vc, Rv, mq, mk = _tables(segs)
    ref_x = x.clone()
    ops.qk_rmsnorm_rope(ref_x, 0, C, wq, wk, C, 1e-6, **kw)
    ref = ops.AttnMx8(M, M, heads, Rv, 1, DEV)
    ops.attn_pack_mxfp8(ref_x[:, :C], ref_x[:, C:2 * C], ref_x[:, 2 * C:], st, vc, 1, mq, mk, heads, ref)
    new_x = x.clone()
    buf = ops.AttnMx8(M, M, heads, Rv, 1, DEV)
    buf.qq.fill_(GUARD), buf.qs.fill_(GUARD)
    ops.qk_rmsnorm_rope_mxfp8(new_x, 0, C, wq, wk, C, 1e-6, buf, **kw)
    torch.cuda.synchronize()
    assert torch.equal(buf.qs, ref.qs) and torch.equal(buf.qq, ref.qq)
    assert torch.equal(new_x[:, C:2 * C], ref_x[:, C:2 * C])          # K as the in-place kernel leaves it
    assert torch.equal(new_x[:, :C], x[:, :C]) and torch.equal(new_x[:, 2 * C:], x[:, 2 * C:])  # q not stored back
    assert not torch.equal(ref_x[:, :C], x[:, :C]) and len(torch.unique(buf.qs)) > 3
    if with_rope:  # the data is what it claims: on a 32-token grid (same h, w) exactly the rows with t >= 16 change
        wide = x.clone()
        ops.qk_rmsnorm_rope(wide, 0, C, wq, wk, C, 1e-6, **{**kw, "grid": (8, 2, 2)})
        same = (wide[:, :C] == ref_x[:, :C]).all(1).cpu()
        t = torch.arange(M) % rpb
        assert same[t < 16].all() and not same[t >= 16].any()


# ------------------------------------------------------------------------------------------------ the K pack

@pytest.mark.parametrize("use_mean", [False, True])
@pytest.mark.parametrize("heads", [1, 3])
def test_attn_pack_k_bit_exact(heads, use_mean):
    C = heads * D
    g = torch.Generator().manual_seed(heads)
    segs, q0, k0 = [], 0, 0
    for ql, kl in [(77, 300), (33, 129)]:
        segs.append([q0, ql, k0, kl])
        q0, k0 = q0 + ql, k0 + kl
    mag = torch.exp2(torch.randint(-6, 5, (3, k0, C // 32), generator=g).float()).repeat_interleave(32, 2)
    x = torch.randn(3, k0, C, generator=g) * mag
    x[1] += 2 * torch.randn(C, generator=g)
    qkv = torch.zeros(k0, 3 * C, dtype=torch.bfloat16, device=DEV)  # column slices of one buffer
    qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:] = (t.bfloat16().to(DEV) for t in x)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    st, vc, Rv, mq, mk = _tables(segs)
    km = mxfp8_attn.k_mean(k.cpu(), segs).to(DEV) if use_mean else None
    ref = ops.AttnMx8(k0, k0, heads, Rv, 2, DEV)
    ops.attn_pack_mxfp8(q, k, v, st, vc, 2, mq, mk, heads, ref, kmean=km)
    buf = ops.AttnMx8(k0, k0, heads, Rv, 2, DEV)
    for t in (buf.qq, buf.qs, buf.kq, buf.ks, buf.vq, buf.vs):
        t.fill_(GUARD)
    ops.attn_pack_k_mxfp8(k, st, 2, mk, heads, buf, km)
    torch.cuda.synchronize()
    assert torch.equal(buf.ks, ref.ks) and torch.equal(buf.kq, ref.kq)
    for t in (buf.qq, buf.qs, buf.vq, buf.vs):  # the K third alone
        assert (t == GUARD).all()


# ------------------------------------------------------------------------------------------------ the DiT

def _make(cfg, P):
    from test_gpu_dit import make_model
    return make_model(cfg, {k: v.clone() for k, v in P.items()})


def _inside_the_bar(out, emu, what):
    r, c = rel(out, emu), cos(out, emu)
    print(f"{what} vs emulated oracle: rel-L2 {r:.3e} cosine {c:.6f}")
    assert r < BAR["rel"] and c > BAR["cos"], (what, r, c)


@pytest.mark.parametrize("case", ["full", "short"])
def test_dit_small_fp8_qkv(case):
    from golden_cases import DIT_SMALL
    from test_gpu_dit import run
    P, inp, emu = small_case(case, True)
    fresh = run(_make(DIT_SMALL, P), inp)
    m = _make(DIT_SMALL, P)
    off0 = run(m, inp)  # packs the bf16 weights first: the toggle must re-pack
    m.enable_fp8_qkv()
    on = run(m, inp)
    _inside_the_bar(on, emu, f"DIT_SMALL {case} fp8 q/k/v")
    print(f"  vs mode off {rel(on, off0):.3e}")
    assert not torch.equal(on, off0)
    m.enable_fp8_qkv(False)
    assert torch.equal(run(m, inp), fresh) and torch.equal(off0, fresh)


def _fused_and_unfused(m, run, inp, monkeypatch):
    """the outputs of the two chains with fp8 q/k/v + fp8 attention on, and how often each chain's own calls ran"""
    calls = {"vt": 0, "pack": 0}
    vt, pack = ops.linear_mxfp8_vt, ops.attn_pack_mxfp8

    def count_vt(*a, **kw):
        calls["vt"] += 1
        return vt(*a, **kw)

    def count_pack(*a, **kw):
        calls["pack"] += 1
        return pack(*a, **kw)

    monkeypatch.setattr(ops, "linear_mxfp8_vt", count_vt)
    monkeypatch.setattr(ops, "attn_pack_mxfp8", count_pack)
    m.enable_fp8_qkv()
    m.enable_fp8_attention()
    m._fp8_qkv_fused = True
    fused = run(m, inp)
    n_fused = dict(calls)
    m._fp8_qkv_fused = False
    unfused = run(m, inp)
    return fused, unfused, n_fused, {k: calls[k] - n_fused[k] for k in calls}


@pytest.mark.parametrize("case", ["full", "short"])
def test_fused_chain_equals_unfused(case, monkeypatch):
    """every new kernel is bit-identical to what it replaces, so the two chains give the same bytes; both cases have
    row lengths that are no multiple of 128 (80 tokens), 'short' with unrotated padding rows"""
    from golden_cases import DIT_SMALL
    from test_gpu_dit import run
    P, inp, _ = small_case(case, False)
    assert inp["seq_len"] % 128 != 0
    m = _make(DIT_SMALL, P)
    fused, unfused, nf, nu = _fused_and_unfused(m, run, inp, monkeypatch)
    L = DIT_SMALL["num_layers"]
    assert nf == {"vt": L, "pack": 0} and nu == {"vt": 0, "pack": L}  # each run took its own chain
    assert torch.equal(fused, unfused)


def test_fused_chain_equals_unfused_dim5120(monkeypatch):
    """the dim-5120 class: the <10> RoPE instantiation, 40 heads, 20 column tiles of the V GEMM"""
    from golden_cases import DIT14_SMALL, dit14_inputs
    from stableavatar_amd import synthetic
    from stableavatar_amd.transformer import WanTransformer3DFantasy14BModel, param_shapes
    from test_gpu_dit14 import _run
    cfg = dict(DIT14_SMALL, vocal="14B")
    P = synthetic.fill_state_dict(param_shapes(cfg), cfg["seed"])
    m = WanTransformer3DFantasy14BModel(**{k: v for k, v in cfg.items() if k not in ("seed", "vocal")})
    m.load_state_dict(P)
    m = m.cuda()
    inp = dit14_inputs(cfg)
    off = _run(m, inp)
    fused, unfused, nf, nu = _fused_and_unfused(m, _run, inp, monkeypatch)
    assert nf == {"vt": 1, "pack": 0} and nu == {"vt": 0, "pack": 1}
    assert torch.equal(fused, unfused) and not torch.equal(fused, off)


def test_dit_small_all_three_modes():
    from golden_cases import DIT_SMALL
    from test_gpu_dit import run
    P, inp, emu = small_case("full", True, True, True)
    m = _make(DIT_SMALL, P)
    m.enable_fp8_qkv(), m.enable_fp8_attention(), m.enable_fp8_ffn()
    _inside_the_bar(run(m, inp), emu, "DIT_SMALL fp8 q/k/v + attention + FFN")


def test_dit_full_dims_all_three_modes():
    """30 layers at the 1.3B widths on a tiny grid"""
    from test_gpu_dit import run
    cfg, P, inp, emu = full_dims_case()
    m = _make(cfg, P)
    m.enable_fp8_qkv(), m.enable_fp8_attention(), m.enable_fp8_ffn()
    _inside_the_bar(run(m, inp), emu, "CONFIG_1_3B fp8 q/k/v + attention + FFN")


def _sp_worker(rank, world, port, qret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    import torch.distributed as dist
    sys.path.insert(0, HERE)
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        from golden_cases import DIT_SMALL
        from test_gpu_dit import run
        P, inp, emu = small_case("full", True, True)
        m = _make(DIT_SMALL, P)
        m.enable_fp8_qkv()
        m.enable_fp8_attention()
        single = run(m, inp)
        m.enable_multi_gpus_inference()
        par = run(m, inp)
        qret.put((rank, rel(par, emu), cos(par, emu), rel(par, single), bool(torch.equal(par, single))))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sp_world2_fp8_qkv_with_fp8_attention():
    """gloo world 2 sharing the GPU, the default exchange schedule (per-row streams: _sp_block_streams), as
    tests/test_gpu_fp8_attn.py::test_sp_world2_fp8_attention drives it: the sequence-parallel sites use the mode for
    the GEMM only, and the output is bit-identical to the single-GPU (fused) one"""
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
    for rank, e_emu, c_emu, e_single, same in res:
        print(f"rank {rank}: vs emulated oracle rel {e_emu:.2e} cos {c_emu:.6f}, vs single-GPU {e_single:.1e}")
        assert e_emu < BAR["rel"] and c_emu > BAR["cos"], (rank, e_emu, c_emu)
        assert same, (rank, e_single)


class _Stop(Exception):
    pass


@pytest.mark.timeout(300)
def test_cli_fp8_qkv_flag(tmp_path, monkeypatch):
    """--fp8_qkv is accepted and the model the CLI builds has the mode on (the tree test_gpu_inference_cli.py writes;
    the run stops at the pipeline call)"""
    from stableavatar_amd.inference import main
    from stableavatar_amd.pipeline import WanI2VTalkingInferenceLongPipeline
    from test_gpu_inference_cli import _write_tree
    root = str(tmp_path)
    _write_tree(root)
    seen = []

    def spy(self, *a, **kw):
        t = self.transformer
        seen.append((t._fp8_qkv, t._fp8_attn, t._fp8_ffn))
        raise _Stop

    monkeypatch.setattr(WanI2VTalkingInferenceLongPipeline, "__call__", spy)
    base = ["--config_path", os.path.join(root, "config.yaml"), "--pretrained_model_name_or_path", root,
            "--transformer_path", os.path.join(root, "transformer3d-square.pt"),
            "--pretrained_wav2vec_path", os.path.join(root, "wav2vec"),
            "--validation_reference_path", os.path.join(root, "reference.png"),
            "--validation_driven_audio_path", os.path.join(root, "audio.wav"),
            "--output_dir", os.path.join(root, "output"), "--validation_prompts", "a woman is singing", "--seed", "42",
            "--ulysses_degree", "1", "--ring_degree", "1", "--motion_frame", "25", "--sample_steps", "2",
            "--width", "64", "--height", "64", "--overlap_window_length", "2", "--clip_sample_n_frames", "17",
            "--GPU_memory_mode", "model_full_load"]
    with pytest.raises(_Stop):
        main(base + ["--fp8_qkv"])
    with pytest.raises(_Stop):
        main(base + ["--fp8_qkv", "--fp8_attn"])
    with pytest.raises(_Stop):
        main(base)
    assert seen == [(True, False, False), (True, True, False), (False, False, False)]
