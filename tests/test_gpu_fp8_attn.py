"""The fp8 attention mode on the GPU: the K means within the fp32-sum bound, the operand pack bit-exact against the
definition (stableavatar_amd/mxfp8_attn.py), the flash kernel exact on the selection / uniform inputs (lane maps of
both products, key permutation, scale bytes, ragged tail, o_rows) and within the definition's own error on random
data, and the DiT with enable_fp8_attention() against the CPU oracle with the definition in its place."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from fp8_attn_util import cos, full_dims_case, oracle_forward, rel, selection_input, small_case, uniform_input  # noqa: E402
from mp_util import collect  # noqa: E402

from stableavatar_amd import mxfp8_attn, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128


def _tables(segs):
    vcol0, Rv = ops.attn_vcol0(segs)
    return (torch.tensor(segs, dtype=torch.int32, device=DEV), torch.tensor(vcol0, dtype=torch.int32, device=DEV), Rv,
            max(s[1] for s in segs), max(s[3] for s in segs))


def _gpu_attention(q, k, v, segs, heads, k_mean=True, o_rows=None, out_rows=None):
    st, vc, Rv, mq, mk = _tables(segs)
    buf = ops.AttnMx8(q.shape[0], k.shape[0], heads, Rv, len(segs), DEV)
    out = torch.zeros(out_rows or q.shape[0], heads * D, dtype=torch.bfloat16, device=DEV)
    o_rows = None if o_rows is None else o_rows.to(DEV)
    if torch.is_tensor(k_mean):  # given means instead of sa_attn_kmean's
        ops.attn_pack_mxfp8(q.to(DEV), k.to(DEV), v.to(DEV), st, vc, len(segs), mq, mk, heads, buf,
                            kmean=k_mean.to(DEV))
        ops.attn_fwd_mxfp8(buf, out, st, vc, len(segs), mq, heads, o_rows)
    else:
        ops.attention_mxfp8(q.to(DEV), k.to(DEV), v.to(DEV), out, st, len(segs), mq, heads, vc, mk, buf,
                            o_rows=o_rows, k_mean=k_mean)
    torch.cuda.synchronize()
    return out.cpu()


def _gpu_kmean(k, segs, heads):
    out = torch.empty(len(segs), heads * D, device=DEV)
    ops.attn_kmean(k.to(DEV), torch.tensor(segs, dtype=torch.int32, device=DEV), len(segs), heads, out)
    return out.cpu()


# ------------------------------------------------------------------------------------------------ the K means

@pytest.mark.parametrize("kv_len", [1, 31, 300])
def test_kmean_within_the_fp32_sum_bound(kv_len):
    heads = 3
    g = torch.Generator().manual_seed(kv_len)
    segs = [[0, 1, 0, kv_len], [1, 1, kv_len + 5, 2 * kv_len + 1]]
    rows = segs[1][2] + segs[1][3]
    k = (torch.randn(rows, heads * D, generator=g) + 3 * torch.randn(heads * D, generator=g)).bfloat16()
    buf = torch.zeros(rows, heads * D + 64, dtype=torch.bfloat16, device=DEV)  # a strided view
    buf[:, :heads * D] = k.to(DEV)
    out = torch.empty(2, heads * D, device=DEV)
    ops.attn_kmean(buf[:, :heads * D], torch.tensor(segs, dtype=torch.int32, device=DEV), 2, heads, out)
    again = torch.empty_like(out)
    ops.attn_kmean(buf[:, :heads * D], torch.tensor(segs, dtype=torch.int32, device=DEV), 2, heads, again)
    assert torch.equal(out, again)  # deterministic
    for i, (_, _, k0, kl) in enumerate(segs):
        x = k[k0:k0 + kl].double()
        err = (out[i].double().cpu() - x.mean(0)).abs()
        bound = kl * 2.0 ** -24 * x.abs().mean(0)  # the worst case of an fp32 sum of kl terms
        print(f"kmean kv_len {kl}: max err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ the pack

PACK_SHAPES = [[(1, 1), (33, 31)], [(257, 129), (1, 128)], [(33, 300), (257, 31)]]


def _pack_data(shapes, heads, seed):
    g = torch.Generator().manual_seed(seed)
    segs, q0, k0 = [], 0, 0
    for ql, kl in shapes:
        segs.append([q0, ql, k0, kl])
        q0, k0 = q0 + ql, k0 + kl
    C = heads * D
    rows = max(q0, k0)
    # magnitudes over several binades per 32-column block, a per-channel offset on k
    mag = torch.exp2(torch.randint(-6, 5, (3, rows, C // 32), generator=g).float()).repeat_interleave(32, 2)
    x = torch.randn(3, rows, C, generator=g) * mag
    x[1] += 2 * torch.randn(C, generator=g)
    return [t.bfloat16() for t in x], segs, q0, k0


@pytest.mark.parametrize("use_mean", [False, True])
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("heads", [1, 3])
def test_pack_bit_exact(heads, sliced, use_mean):
    C = heads * D
    for si, shapes in enumerate(PACK_SHAPES):
        (q, k, v), segs, nq, nk = _pack_data(shapes, heads, 10 * si + heads)
        q, k, v = q[:nq], k[:nk], v[:nk]
        if sliced:  # column slices of one [rows, 3 * heads * 128] buffer (every tensor padded to the same rows)
            rows = max(nq, nk)
            qkv = torch.zeros(rows, 3 * C, dtype=torch.bfloat16, device=DEV)
            qkv[:nq, :C], qkv[:nk, C:2 * C], qkv[:nk, 2 * C:] = q.to(DEV), k.to(DEV), v.to(DEV)
            qd, kd, vd = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        else:
            qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
        st, vc, Rv, mq, mk = _tables(segs)
        assert vc[1].item() != segs[1][2]  # the second segment's V^T columns do not start at its kv_row0
        km = mxfp8_attn.k_mean(k, segs) if use_mean else None
        buf = ops.AttnMx8(qd.shape[0], kd.shape[0], heads, Rv, 2, DEV)
        for t in (buf.qq, buf.qs, buf.kq, buf.ks, buf.vq):
            t.zero_()
        buf.vs.fill_(127)
        ops.attn_pack_mxfp8(qd, kd, vd, st, vc, 2, mq, mk, heads, buf, kmean=None if km is None else km.to(DEV))
        want = mxfp8_attn.pack(q, k, v, segs, heads, D ** -0.5, km)
        got = (buf.qq[:nq], buf.qs[:nq], buf.kq[:nk], buf.ks[:nk], buf.vq, buf.vs)
        for name, a, b in zip(("Q", "Q scales", "K", "K scales", "V^T", "V^T scales"), got, want):
            assert torch.equal(a.cpu(), b), (shapes, name)
        # V^T columns between kv_len and ceil128(kv_len): zero bytes; a whole padded block carries the zero-block scale
        for (_, _, _, kl), c0 in zip(segs, want[6]):
            pad = mxfp8_attn.KEY_OF_POS >= kl - (mxfp8_attn.ceil128(kl) - 128)
            last = buf.vq[:, c0 + mxfp8_attn.ceil128(kl) - 128:c0 + mxfp8_attn.ceil128(kl)].cpu()
            assert (last[:, pad] == 0).all()
            if kl == 1:  # positions 32 .. 127 hold no key at all
                assert (buf.vs[:, c0 // 32 + 1:c0 // 32 + 4] == 127).all()


# ------------------------------------------------------------------------------------------------ the kernel, exact

@pytest.mark.parametrize("use_mean", [False, True])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("shapes", [[(77, 300), (33, 129)], [(257, 129), (77, 300)], [(33, 1000), (257, 1)]])
def test_kernel_selects_exactly(shapes, heads, use_mean):
    q, k, v, segs, want = selection_input(shapes, heads)
    assert torch.equal(mxfp8_attn.attention(q, k, v, segs, heads,
                                            kmean=mxfp8_attn.k_mean(k, segs) if use_mean else None), want)
    out = _gpu_attention(q, k, v, segs, heads, k_mean=use_mean)
    assert torch.equal(out, want)


def test_kernel_selects_exactly_through_a_shuffled_row_map():
    heads = 3
    q, k, v, segs, want = selection_input([(77, 300), (257, 129)], heads)
    n = q.shape[0]
    perm = torch.randperm(n + 9, generator=torch.Generator().manual_seed(1))[:n].int()
    out = _gpu_attention(q, k, v, segs, heads, o_rows=perm, out_rows=n + 9)
    ref = torch.zeros(n + 9, heads * D, dtype=torch.bfloat16)
    ref[perm.long()] = want
    assert torch.equal(out, ref)  # the rows the map does not name stay untouched


def test_kernel_uniform_exact_at_256_keys():
    q, k, v, segs, mean = uniform_input(256, 40, heads=3)
    out = _gpu_attention(q, k, v, segs, 3)
    assert torch.equal(out, mean.float().bfloat16().expand(40, -1))


def test_kernel_uniform_within_one_ulp_at_300_keys():
    q, k, v, segs, mean = uniform_input(300, 40, heads=3)
    out = _gpu_attention(q, k, v, segs, 3).double()
    ulp = torch.exp2(torch.floor(torch.log2(mean.abs().clamp_min(2.0 ** -126))) - 7)  # bf16: 8 significant bits
    assert ((out - mean).abs() <= ulp).all()


def test_kernel_empty_segment_gives_zeros():
    q, k, v, segs, want = selection_input([(77, 300), (40, 5)], heads=1)
    segs[1][3] = 0
    st, vc, Rv, mq, mk = _tables(segs)
    buf = ops.AttnMx8(q.shape[0], k.shape[0], 1, Rv, 2, DEV)
    out = torch.full((q.shape[0], D), 5.0, dtype=torch.bfloat16, device=DEV)
    ops.attention_mxfp8(q.to(DEV), k.to(DEV), v.to(DEV), out, st, 2, mq, 1, vc, mk, buf)
    assert torch.equal(out[:77].cpu(), want[:77]) and (out[77:] == 0).all()


# ------------------------------------------------------------------------------------------------ the kernel, random

def _softmax64(qd, kd, vd, heads):
    h = lambda t: t.double().reshape(t.shape[0], heads, D).transpose(0, 1)  # noqa: E731
    s = h(qd) @ h(kd).transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return ((p @ h(vd)) / p.sum(-1, keepdim=True)).transpose(0, 1).reshape(qd.shape[0], heads * D)


@pytest.mark.parametrize("variant", ["plain", "sharp", "k_offset"])
@pytest.mark.parametrize("shape", [(257, 1000), (40, 300)])
def test_kernel_random_within_the_definitions_error(shape, variant):
    heads, (ql, kl) = 3, shape
    g = torch.Generator().manual_seed(ql + len(variant))
    q, k, v = (torch.randn(n, heads * D, generator=g) for n in (ql, kl, kl))
    if variant == "sharp":
        q = q * 4
    if variant == "k_offset":
        k = k + 3 * torch.randn(heads * D, generator=g)
    q, k, v = q.bfloat16(), k.bfloat16(), v.bfloat16()
    segs = [[0, ql, 0, kl]]
    km = _gpu_kmean(k, segs, heads)  # the means the kernel's own first pass gives, for both sides
    scale = D ** -0.5
    # R: fp64 softmax attention on the dequantised operands (isolates P's rounding and the accumulation order);
    # X: on the unquantised inputs (q prescaled the same way; the K mean cancels in exact arithmetic)
    R = _softmax64(*mxfp8_attn.dequant_operands(q, k, v, scale, km[0]), heads)
    X = _softmax64(q.double() * float(mxfp8_attn.prescale(scale)), k.double(), v.double(), heads)
    want = mxfp8_attn.attention(q, k, v, segs, heads, scale, km)
    out = _gpu_attention(q, k, v, segs, heads, k_mean=km)
    eR, dR, eX, dX = rel(out, R), rel(want, R), rel(out, X), rel(want, X)
    print(f"{variant} {shape}: vs R kernel {eR:.3e} definition {dR:.3e} ratio {eR / dR:.3f}; "
          f"vs exact kernel {eX:.3e} definition {dX:.3e} ratio {eX / dX:.3f}")
    assert eR <= 1.5 * dR + 2.0 ** -8
    assert eX <= 1.5 * dX


# ------------------------------------------------------------------------------------------------ the DiT

BAR = dict(rel=2e-2, cos=0.9995)  # the project's bar for a quantised mode against its emulated oracle


def _make(cfg, P):
    from test_gpu_dit import make_model
    return make_model(cfg, {k: v.clone() for k, v in P.items()})


def _inside_the_bar(out, emu, what):
    r, c = rel(out, emu), cos(out, emu)
    print(f"{what} vs emulated oracle: rel-L2 {r:.3e} cosine {c:.6f}")
    assert r < BAR["rel"] and c > BAR["cos"], (what, r, c)


def test_dit_small_fp8_attention():
    from golden_cases import DIT_SMALL
    from test_gpu_dit import run
    P, inp, emu = small_case("full", True)
    fresh = run(_make(DIT_SMALL, P), inp)
    m = _make(DIT_SMALL, P)
    off0 = run(m, inp)
    m.enable_fp8_attention()
    on = run(m, inp)
    _inside_the_bar(on, emu, "DIT_SMALL fp8 attention")
    print(f"  vs mode off {rel(on, off0):.3e}")
    assert not torch.equal(on, off0)
    m.enable_fp8_attention(False)
    assert torch.equal(run(m, inp), fresh) and torch.equal(off0, fresh)


def test_dit_small_short_rows_fp8_attention():
    """the ragged case: the row length is no multiple of 128"""
    from golden_cases import DIT_SMALL
    from test_gpu_dit import run
    P, inp, emu = small_case("short", True)
    assert inp["seq_len"] % 128 != 0
    m = _make(DIT_SMALL, P)
    m.enable_fp8_attention()
    _inside_the_bar(run(m, inp), emu, "DIT_SMALL short fp8 attention")


def test_dit_full_dims_fp8_attention():
    """30 layers at the 1.3B widths on a tiny grid"""
    from test_gpu_dit import run
    cfg, P, inp, emu = full_dims_case()
    m = _make(cfg, P)
    m.enable_fp8_attention()
    _inside_the_bar(run(m, inp), emu, "CONFIG_1_3B fp8 attention")


def test_dit_small_fp8_attention_with_fp8_ffn():
    from golden_cases import DIT_SMALL
    from test_gpu_dit import run
    P, inp, emu = small_case("full", True, True)
    m = _make(DIT_SMALL, P)
    m.enable_fp8_attention()
    m.enable_fp8_ffn()
    _inside_the_bar(run(m, inp), emu, "DIT_SMALL fp8 attention + fp8 FFN")


def test_dit14_small_fp8_attention():
    """the dim-5120 class (head_dim 128 as well) goes through the same call site"""
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
    inp.setdefault("n_frames", 81)
    off = _run(m, inp)
    m.enable_fp8_attention()
    on = _run(m, inp)
    assert not torch.equal(on, off)
    _inside_the_bar(on, oracle_forward(P, cfg, inp, True), "14B-class DiT fp8 attention")


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
        m.enable_fp8_attention()
        single = run(m, inp)
        m.enable_multi_gpus_inference()
        par = run(m, inp)
        qret.put((rank, rel(par, emu), cos(par, emu), rel(par, single), bool(torch.isfinite(par).all())))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sp_world2_fp8_attention():
    """gloo world 2 sharing the GPU, the default exchange schedule (per-row streams: _sp_block_streams), as
    tests/test_gpu_mxfp8.py::test_sp_world2_fp8_ffn drives it"""
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
        assert e_emu < BAR["rel"] and c_emu > BAR["cos"], (rank, e_emu, c_emu)
        assert e_single < 1e-3, (rank, e_single)


class _Stop(Exception):
    pass


@pytest.mark.timeout(300)
def test_cli_fp8_attn_flag(tmp_path, monkeypatch):
    """--fp8_attn is accepted and the model the CLI builds has the mode on (the tree test_gpu_inference_cli.py
    writes; the run stops at the pipeline call)"""
    from stableavatar_amd.inference import main
    from stableavatar_amd.pipeline import WanI2VTalkingInferenceLongPipeline
    from test_gpu_inference_cli import _write_tree
    root = str(tmp_path)
    _write_tree(root)
    seen = []

    def spy(self, *a, **kw):
        seen.append((self.transformer._fp8_attn, self.transformer._fp8_ffn))
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
        main(base + ["--fp8_attn"])
    with pytest.raises(_Stop):
        main(base)
    assert seen == [(True, False), (False, False)]
