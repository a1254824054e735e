"""The fp8 self-O mode on the GPU: the two flash entry points that write the O-projection's MXFP8 operand, byte-exact
against the bf16 entry point followed by the quantiser (guard bytes around everything they may write) and against the
definition on an exact input; the DiT with enable_fp8_o() against the CPU oracle with the same Linear emulated, alone
and with the other three modes; fused against unfused; the mode toggled off; sequence parallel."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from fp8_o_util import cos, oracle_forward, rel, small_case  # noqa: E402
from mp_util import collect  # noqa: E402

from stableavatar_amd import mxfp8, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128
GUARD = 0xA5
BAR = dict(rel=2e-2, cos=0.9995)  # the project's bar for a quantised mode against its emulated oracle


# ------------------------------------------------------------------------------------------------ the kernels

def _inputs(shapes, heads, seed):
    """segments of (q_len, kv_len) on random q, k; v scaled per 32-column block by 2^randint(-5, 4) with one block of
    columns all zero, so the four blocks of a head take different scale bytes and one of them 127"""
    g = torch.Generator().manual_seed(seed)
    C = heads * D
    segs, q0, k0 = [], 0, 0
    for ql, kl in shapes:
        segs.append([q0, ql, k0, kl])
        q0, k0 = q0 + ql, k0 + max(kl, 1)  # a segment without keys still names a row
    q, k = torch.randn(q0, C, generator=g), torch.randn(k0, C, generator=g)
    mag = torch.exp2(torch.randint(-5, 5, (C // 32,), generator=g).float())
    mag[1 % (C // 32)] = 0.0
    v = torch.randn(k0, C, generator=g) * mag.repeat_interleave(32)
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), segs


def _packed(q, k, v, segs, heads):
    vcol0, Rv = ops.attn_vcol0(segs)
    st = torch.tensor(segs, dtype=torch.int32, device=DEV)
    vc = torch.tensor(vcol0, dtype=torch.int32, device=DEV)
    mq, mk = max(s[1] for s in segs), max(s[3] for s in segs)
    buf = ops.AttnMx8(q.shape[0], k.shape[0], heads, Rv, len(segs), DEV)
    kd = k.to(DEV)
    km = ops.attn_kmean(kd, st, len(segs), heads, buf.kmean, buf.kmean_work)
    ops.attn_pack_mxfp8(q.to(DEV), kd, v.to(DEV), st, vc, len(segs), mq, mk, heads, buf, kmean=km)
    return buf, st, vc, mq


def _witness_and_o8(q, k, v, segs, heads, o_rows=None, out_rows=None, split_tiles=0):
    """-> (bf16 rows of the existing entry point, their mxfp8_quant, the o8 entry point's byte and scale buffers with
    128 guard columns / 4 guard scale columns, the mask of rows a query maps to)"""
    C, n = heads * D, q.shape[0]
    out_rows = out_rows or n
    buf, st, vc, mq = _packed(q, k, v, segs, heads)
    om = None if o_rows is None else o_rows.to(DEV)
    ref = torch.zeros(out_rows, C, dtype=torch.bfloat16, device=DEV)
    ops.attn_fwd_mxfp8(buf, ref, st, vc, len(segs), mq, heads, om, split_tiles=split_tiles)
    want = ops.mxfp8_quant(ref)
    qbig = torch.full((out_rows, C + 128), GUARD, dtype=torch.uint8, device=DEV)
    sbig = torch.full((out_rows, heads * 4 + 4), GUARD, dtype=torch.uint8, device=DEV)
    ops.attn_fwd_mxfp8(buf, ops.Mx8(qbig[:, :C], sbig[:, :heads * 4]), st, vc, len(segs), mq, heads, om,
                       split_tiles=split_tiles)
    torch.cuda.synchronize()
    written = torch.zeros(out_rows, dtype=torch.bool)
    for q0, ql, _, _ in segs:
        rows = torch.arange(q0, q0 + ql)
        written[rows if o_rows is None else o_rows[rows].long()] = True
    return ref.cpu(), ops.Mx8(want.q.cpu(), want.s.cpu()), qbig.cpu(), sbig.cpu(), written


def _check_bytes(want, qbig, sbig, written, heads, what):
    C = heads * D
    assert torch.equal(sbig[written, :heads * 4], want.s[written]), (what, "scales")
    assert torch.equal(qbig[written, :C], want.q[written]), (what, "bytes")
    # nothing else is touched: rows no query maps to, the columns past the heads, the scale columns past the heads
    assert (qbig[~written] == GUARD).all() and (sbig[~written] == GUARD).all(), (what, "rows")
    assert (qbig[:, C:] == GUARD).all() and (sbig[:, heads * 4:] == GUARD).all(), (what, "columns")


O8_CASES = {
    "one_segment": [(300, 1000)],
    "two_segments": [(37, 129), (300, 513)],
    "no_keys": [(77, 300), (40, 0), (300, 257)],
}


@pytest.mark.parametrize("case", list(O8_CASES))
def test_o8_is_the_bf16_kernel_followed_by_the_quantiser(case):
    heads, shapes = 3, O8_CASES[case]
    q, k, v, segs = _inputs(shapes, heads, seed=len(case))
    n = q.shape[0]
    ref, want, qbig, sbig, written = _witness_and_o8(q, k, v, segs, heads, out_rows=n + 9)
    assert written.sum() == n and not written[n:].any()
    _check_bytes(want, qbig, sbig, written, heads, case)
    used = sbig[written, :heads * 4]
    assert len(torch.unique(used)) > 3 and (used == 127).any()  # several binades, and an all-zero block
    if case == "no_keys":  # zeros, scale byte 127 -- whatever the witness says
        q0, ql = segs[1][0], segs[1][1]
        assert (qbig[q0:q0 + ql, :heads * D] == 0).all() and (sbig[q0:q0 + ql, :heads * 4] == 127).all()


def test_o8_through_a_shuffled_row_map():
    heads = 3
    q, k, v, segs = _inputs([(77, 300), (257, 129)], heads, seed=2)
    n = q.shape[0]
    perm = torch.randperm(n + 9, generator=torch.Generator().manual_seed(1))[:n].int()
    ref, want, qbig, sbig, written = _witness_and_o8(q, k, v, segs, heads, o_rows=perm, out_rows=n + 9)
    assert written.sum() == n
    _check_bytes(want, qbig, sbig, written, heads, "o_rows")


def _exact_input(kv_len, q_len, heads, seed=11):
    """Q = 0: a uniform P; V = small integers times a power of two per key and one per 32-column block: with a
    power-of-two key count every sum is exact, so O is the mean of V exactly.  -> q, k, v, segs, the mean in fp64"""
    g = torch.Generator().manual_seed(seed)
    C = heads * D
    k = torch.randn(kv_len, C, generator=g).bfloat16()
    col = torch.exp2(torch.randint(-5, 5, (C // 32,), generator=g).float())
    col[2] = 0.0
    v = (torch.randint(-7, 8, (kv_len, C), generator=g).float()
         * torch.exp2(torch.randint(-3, 4, (kv_len, 1), generator=g).float()) * col.repeat_interleave(32)).bfloat16()
    return torch.zeros(q_len, C).bfloat16(), k, v, [[0, q_len, 0, kv_len]], v.double().mean(0)


@pytest.mark.parametrize("split", [False, True], ids=["o8", "split_o8"])
def test_o8_exact_against_the_definition(split):
    """no witness from the GPU: the bytes are mxfp8.quantize of the value computed on the CPU, so a wrong lane-to-column
    map or block grouping shows"""
    heads, ql = 3, 40
    q, k, v, segs, mean = _exact_input(256, ql, heads)
    wq, ws = mxfp8.quantize(mean.float().bfloat16().expand(ql, -1).contiguous())
    ref, _, qbig, sbig, written = _witness_and_o8(q, k, v, segs, heads, split_tiles=heads if split else 0)
    assert torch.equal(ref, mean.float().bfloat16().expand(ql, -1))
    assert torch.equal(sbig[:, :heads * 4], ws) and torch.equal(qbig[:, :heads * D], wq)
    assert len(torch.unique(ws)) > 3 and (ws == 127).any()
    assert len(torch.unique(wq[0])) > 16  # the columns differ: a permutation would show


@pytest.mark.parametrize("all_tiles", [False, True], ids=["split1", "split_all"])
@pytest.mark.parametrize("q_len", [300, 600])
def test_split_o8_is_the_bf16_split_followed_by_the_quantiser(q_len, all_tiles):
    """the key-split launch: whole tiles through the flash kernel's epilogue, split tiles through the merge; a segment
    whose second half is empty (100 keys) and one without keys among them"""
    heads = 3
    shapes = [(q_len, 1000), (40, 100), (33, 0)]
    q, k, v, segs = _inputs(shapes, heads, seed=q_len)
    nt = len(segs) * heads * -(-q_len // 256)
    n = q.shape[0]
    ref, want, qbig, sbig, written = _witness_and_o8(q, k, v, segs, heads, out_rows=n + 9,
                                                     split_tiles=nt if all_tiles else 1)
    assert written.sum() == n
    _check_bytes(want, qbig, sbig, written, heads, (q_len, all_tiles))
    q0, ql = segs[2][0], segs[2][1]
    assert (qbig[q0:q0 + ql, :heads * D] == 0).all() and (sbig[q0:q0 + ql, :heads * 4] == 127).all()
    assert len(torch.unique(sbig[written, :heads * 4])) > 3


# ------------------------------------------------------------------------------------------------ the DiT

def _make(cfg, P):
    from test_gpu_dit import make_model
    return make_model(cfg, {k: v.clone() for k, v in P.items()})


def _inside_the_bar(out, emu, what):
    r, c = rel(out, emu), cos(out, emu)
    print(f"{what} vs emulated oracle: rel-L2 {r:.3e} cosine {c:.6f}")
    assert r < BAR["rel"] and c > BAR["cos"], (what, r, c)


def _all_four(m):
    m.enable_fp8_o(), m.enable_fp8_qkv(), m.enable_fp8_attention(), m.enable_fp8_ffn()
    return m


@pytest.mark.parametrize("case", ["full", "short"])
def test_dit_small_fp8_o_alone_and_toggled_off(case):
    """the mode alone: bf16 attention, the quantiser, the MXFP8 GEMM; off again, the bytes of a model never toggled"""
    from golden_cases import DIT_SMALL
    from test_gpu_dit import run
    P, inp, emu = small_case(case, True)
    fresh = run(_make(DIT_SMALL, P), inp)
    m = _make(DIT_SMALL, P)
    off0 = run(m, inp)  # packs the bf16 weight first: the toggle must re-pack
    m.enable_fp8_o()
    on = run(m, inp)
    _inside_the_bar(on, emu, f"DIT_SMALL {case} fp8 self-O")
    print(f"  vs mode off {rel(on, off0):.3e}")
    assert not torch.equal(on, off0)
    m.enable_fp8_o(False)
    assert torch.equal(run(m, inp), fresh) and torch.equal(off0, fresh)


@pytest.mark.parametrize("case", ["full", "short"])
def test_dit_small_all_four_modes_fused_equals_unfused(case, monkeypatch):
    """all four modes against the oracle with all four emulations; the flash kernel writing the operand gives the
    bytes of the bf16 output through the quantiser, and each run took its own path"""
    from golden_cases import DIT_SMALL
    from test_gpu_dit import run
    P, inp, emu = small_case(case, True, True, True, True)
    m = _all_four(_make(DIT_SMALL, P))
    calls = []
    quant = ops.mxfp8_quant
    monkeypatch.setattr(ops, "mxfp8_quant", lambda *a, **kw: (calls.append(1), quant(*a, **kw))[1])
    m._fp8_o_fused = True
    fused = run(m, inp)
    n_fused = len(calls)
    m._fp8_o_fused = False
    unfused = run(m, inp)
    _inside_the_bar(fused, emu, f"DIT_SMALL {case} fp8 self-O + q/k/v + attention + FFN")
    # the weights are quantised at pack time (before the first run's blocks), the activations once per layer, unfused
    assert len(calls) - n_fused == DIT_SMALL["num_layers"]
    assert torch.equal(fused, unfused)
    three = _make(DIT_SMALL, P)
    three.enable_fp8_qkv(), three.enable_fp8_attention(), three.enable_fp8_ffn()
    assert not torch.equal(run(three, inp), fused)


def test_dit14_small_all_four_modes():
    """the dim-5120 class (40 heads) goes through the same sites"""
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
    m.enable_fp8_qkv(), m.enable_fp8_attention(), m.enable_fp8_ffn()
    three = _run(m, inp)
    m.enable_fp8_o()
    on = _run(m, inp)
    assert not torch.equal(on, three)
    _inside_the_bar(on, oracle_forward(P, cfg, inp, True, True, True, True), "14B-class DiT, all four modes")


def _sp_worker(rank, world, port, qret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    import torch.distributed as dist
    sys.path.insert(0, HERE)
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        from golden_cases import DIT_SMALL
        from test_gpu_dit import run
        P, inp, emu = small_case("full", True, True, True, True)
        m = _all_four(_make(DIT_SMALL, P))
        single = run(m, inp)
        m.enable_multi_gpus_inference()
        par = run(m, inp)
        qret.put((rank, rel(par, emu), cos(par, emu), rel(par, single), bool(torch.equal(par, single))))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sp_world2_all_four_modes():
    """gloo world 2 sharing the GPU, the default exchange schedule, as tests/test_gpu_fp8_qkv.py drives it: each bf16
    column panel is quantised into its columns of the operand, whose bytes are then the single-GPU ones -- the output
    is bit-identical to the single-GPU (fused) forward"""
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
