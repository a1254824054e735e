"""The key-split launch of the fp8 attention mode on the GPU (sa_attn_fwd_mxfp8_split): its argument checks, whole tiles
and empty second halves bit for bit the unsplit kernel's, exact on the selection / uniform inputs with every tile
split and at the split rule's own count (the tile decode), zeros for a segment without keys, within the split
definition's error on random data, and the DiT under sequence parallelism with every tile split."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from fp8_attn_split_util import RANDOM_SHAPES, SELECT_SHAPES, VARIANTS, n_tiles, random_case  # noqa: E402
from fp8_attn_util import cos, rel, selection_input, small_case, uniform_input  # noqa: E402
from mp_util import collect  # noqa: E402

from stableavatar_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128
WORK_PER_TILE = 2 * 256 * (D + 2)  # floats


def _tables(segs):
    vcol0, Rv = ops.attn_vcol0(segs)
    return (torch.tensor(segs, dtype=torch.int32, device=DEV), torch.tensor(vcol0, dtype=torch.int32, device=DEV), Rv,
            max(s[1] for s in segs), max(s[3] for s in segs))


def _packed(q, k, v, segs, heads, k_mean=True):
    """the operands of one launch: (AttnMx8, segs, vcol0, max_q_len); k_mean: True = sa_attn_kmean's, a tensor = given"""
    st, vc, Rv, mq, mk = _tables(segs)
    buf = ops.AttnMx8(q.shape[0], k.shape[0], heads, Rv, len(segs), DEV)
    if torch.is_tensor(k_mean):
        km = k_mean.to(DEV)
    else:
        km = ops.attn_kmean(k.to(DEV), st, len(segs), heads, buf.kmean, buf.kmean_work) if k_mean else None
    ops.attn_pack_mxfp8(q.to(DEV), k.to(DEV), v.to(DEV), st, vc, len(segs), mq, mk, heads, buf, kmean=km)
    return buf, st, vc, mq


def _split_attention(q, k, v, segs, heads, split_tiles, k_mean=True, o_rows=None, out_rows=None):
    buf, st, vc, mq = _packed(q, k, v, segs, heads, k_mean)
    buf.split_work = torch.full((split_tiles * WORK_PER_TILE,), float("nan"), device=DEV)
    out = torch.zeros(out_rows or q.shape[0], heads * D, dtype=torch.bfloat16, device=DEV)
    ops.attn_fwd_mxfp8(buf, out, st, vc, len(segs), mq, heads, None if o_rows is None else o_rows.to(DEV),
                       split_tiles=split_tiles)
    torch.cuda.synchronize()
    return out.cpu()


# ------------------------------------------------------------------------------------------------ argument checks

def test_split_rejects_bad_arguments_and_touches_nothing():
    heads = 1
    q, k, v, segs, _ = selection_input([(300, 257)], heads)
    buf, st, vc, mq = _packed(q, k, v, segs, heads)
    nt = n_tiles(segs, heads)
    assert nt == 2
    out = torch.full((q.shape[0], heads * D + 8), 7.0, dtype=torch.bfloat16, device=DEV)
    work = torch.full((nt * WORK_PER_TILE + 4,), -3.0, device=DEV)
    L = _lib.lib()
    ok = dict(q=buf.qq.data_ptr(), qs=buf.qs.data_ptr(), k=buf.kq.data_ptr(), ks=buf.ks.data_ptr(),
              vt=buf.vq.data_ptr(), vts=buf.vs.data_ptr(), Rv=buf.Rv, o=out.data_ptr(), os=out.stride(0),
              segs=st.data_ptr(), vcol0=vc.data_ptr(), nseg=1, mq=mq, heads=heads, hd=128, orows=None, split=nt,
              work=work.data_ptr(), wb=nt * WORK_PER_TILE * 4, stream=None)
    order = list(ok)

    def rc(**kw):
        return L.sa_attn_fwd_mxfp8_split(*[dict(ok, **kw)[n] for n in order])

    for name in ("q", "qs", "k", "ks", "vt", "vts", "o", "segs", "vcol0", "work"):
        assert rc(**{name: None}) == 1, name
    assert rc(hd=64) == 1
    assert rc(os=out.stride(0) + 4) == 1                       # o_stride % 8
    for name in ("q", "k", "vt", "o", "work"):                 # 16-byte accesses
        assert rc(**{name: ok[name] + 8}) == 1, name
    for name in ("qs", "ks", "vts"):                           # dword scale loads
        assert rc(**{name: ok[name] + 2}) == 1, name
    assert rc(split=0) == 1 and rc(split=-1) == 1 and rc(split=nt + 1) == 1
    assert rc(wb=ok["wb"] - 4) == 1 and rc(split=1, wb=WORK_PER_TILE * 4 - 1) == 1
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (work == -3.0).all()


# ------------------------------------------------------------------------------------------------ whole tiles

@pytest.mark.parametrize("shapes,split_tiles", [([(257, 300), (77, 129)], 1), ([(257, 300), (77, 129)], 5),
                                                ([(257, 300), (77, 129)], 12),
                                                ([(257, 300), (77, 129), (40, 128), (33, 1)], 24)])
def test_whole_tiles_and_empty_second_halves_are_the_unsplit_kernels_bytes(shapes, split_tiles):
    """heads 3, two query blocks: 6 tiles a segment (the second block of every segment but the first holds no query).
    Soft rows, so every key weighs in and a tile with keys in both halves does change."""
    heads, nqb = 3, 2
    q, k, v, segs, _ = selection_input(shapes, heads, seed=9)
    g = torch.Generator().manual_seed(4)
    q = (q.float() * 0.02 + torch.randn(q.shape, generator=g)).bfloat16()
    nt = n_tiles(segs, heads)
    assert nt == 6 * len(shapes) and split_tiles <= nt
    buf, st, vc, mq = _packed(q, k, v, segs, heads)
    n = q.shape[0]
    perm = torch.randperm(n + 9, generator=torch.Generator().manual_seed(1))[:n].int()
    whole = torch.full((n + 9, heads * D), 5.0, dtype=torch.bfloat16, device=DEV)
    ops.attn_fwd_mxfp8(buf, whole, st, vc, len(segs), mq, heads, perm.to(DEV))
    out = torch.full((n + 9, heads * D), 5.0, dtype=torch.bfloat16, device=DEV)
    need = split_tiles * WORK_PER_TILE
    buf.split_work = torch.full((need + 64,), -3.0, device=DEV)
    ops.attn_fwd_mxfp8(buf, out, st, vc, len(segs), mq, heads, perm.to(DEV), split_tiles=split_tiles)
    torch.cuda.synchronize()
    assert (buf.split_work[need:] == -3.0).all()               # nothing past the required bytes
    out, whole = out.cpu(), whole.cpu()
    named = torch.zeros(n + 9, dtype=torch.bool)
    named[perm.long()] = True
    assert (out[~named] == 5.0).all() and (whole[~named] == 5.0).all()
    assert torch.isfinite(out.float()).all()
    changed = 0
    for i, (q0, ql, _, kl) in enumerate(segs):
        for h in range(heads):
            for qb in range(nqb):
                rows = perm[q0 + qb * 256:q0 + min(ql, (qb + 1) * 256)].long()
                a, b = out[rows, h * D:(h + 1) * D], whole[rows, h * D:(h + 1) * D]
                if (i * heads + h) * nqb + qb < nt - split_tiles or kl <= 128:
                    assert torch.equal(a, b), (i, h, qb)
                else:
                    changed += int(not torch.equal(a, b))
    assert changed > 0 or split_tiles == 1  # the last tile of all holds no query


# ------------------------------------------------------------------------------------------------ exact inputs

@pytest.mark.parametrize("use_mean", [False, True])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("shapes", SELECT_SHAPES + [[(40, 128)], [(40, 1)], [(300, 257)]])
def test_split_kernel_selects_exactly(shapes, heads, use_mean):
    q, k, v, segs, want = selection_input(shapes, heads)
    out = _split_attention(q, k, v, segs, heads, n_tiles(segs, heads), k_mean=use_mean)
    assert torch.equal(out, want)


def test_split_kernel_selects_exactly_through_a_shuffled_row_map():
    heads = 3
    q, k, v, segs, want = selection_input([(77, 300), (257, 129)], heads)
    n = q.shape[0]
    perm = torch.randperm(n + 9, generator=torch.Generator().manual_seed(1))[:n].int()
    out = _split_attention(q, k, v, segs, heads, n_tiles(segs, heads), o_rows=perm, out_rows=n + 9)
    ref = torch.zeros(n + 9, heads * D, dtype=torch.bfloat16)
    ref[perm.long()] = want
    assert torch.equal(out, ref)  # the rows the map does not name stay untouched


@pytest.mark.parametrize("kv_len", [256, 512])
def test_split_kernel_uniform_exact(kv_len):
    q, k, v, segs, mean = uniform_input(kv_len, 40, heads=3)
    out = _split_attention(q, k, v, segs, 3, n_tiles(segs, 3))
    assert torch.equal(out, mean.float().bfloat16().expand(40, -1))


def test_split_kernel_uniform_within_one_ulp_at_300_keys():
    q, k, v, segs, mean = uniform_input(300, 40, heads=3)
    out = _split_attention(q, k, v, segs, 3, n_tiles(segs, 3)).double()
    ulp = torch.exp2(torch.floor(torch.log2(mean.abs().clamp_min(2.0 ** -126))) - 7)  # bf16: 8 significant bits
    assert ((out - mean).abs() <= ulp).all()


def test_split_kernel_zero_key_segment_gives_zeros():
    q, k, v, segs, want = selection_input([(77, 300), (40, 5), (300, 5)], heads=1)
    segs[1][3] = segs[2][3] = 0
    buf, st, vc, mq = _packed(q, k, v, segs, 1)
    nt = n_tiles(segs, 1)
    buf.split_work = torch.full((nt * WORK_PER_TILE,), float("nan"), device=DEV)
    out = torch.full((q.shape[0], D), 5.0, dtype=torch.bfloat16, device=DEV)
    ops.attn_fwd_mxfp8(buf, out, st, vc, 3, mq, 1, split_tiles=nt)
    out = out.cpu()
    assert torch.equal(out[:77], want[:77]) and (out[77:] == 0).all()


# ------------------------------------------------------------------------------------------------ random data

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", RANDOM_SHAPES[:3])
def test_split_kernel_random_within_the_split_definitions_error(shape, variant):
    """every tile split; the project's bounds for this kernel, against the split definition on the same K means"""
    heads = 3
    c = random_case(shape, variant, heads)
    out = _split_attention(c["q"], c["k"], c["v"], c["segs"], heads, n_tiles(c["segs"], heads), k_mean=c["km"])
    eR, dR, eX, dX = rel(out, c["R"]), c["split_R"], rel(out, c["X"]), c["split_X"]
    print(f"{variant} {shape}: vs R kernel {eR:.3e} split definition {dR:.3e} ratio {eR / dR:.3f}; "
          f"vs exact kernel {eX:.3e} split definition {dX:.3e} ratio {eX / dX:.3f}")
    assert eR <= 1.5 * dR + 2.0 ** -8
    assert eX <= 1.5 * dX


# ------------------------------------------------------------------------------------------------ the rule's count

def test_split_kernel_exact_at_the_rules_own_count():
    """the Ulysses N = 8 rank launch's tile table with short keys: 3 segments x 3 heads x 42 query blocks = 378 tiles,
    the last 378 % CUs of them split (122 on 256 CUs): whole tiles through the XCD remap of a count that is no
    multiple of 8, halves behind them"""
    heads = 3
    nt = 3 * heads * 42
    split = ops.attn_tail_split(0, nt, torch.device(DEV))
    if split == 0:
        pytest.skip("the rule gives no split on this device")
    q, k, v, segs, want = selection_input([(10752, 300)] * 3, heads)
    assert n_tiles(segs, heads) == nt
    out = _split_attention(q, k, v, segs, heads, split)
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ the DiT under SP

BAR = dict(rel=2e-2, cos=0.9995)  # the project's bar for a quantised mode against its emulated oracle


def _sp_worker(rank, world, port, qret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    import torch.distributed as dist
    sys.path.insert(0, HERE)
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        from golden_cases import DIT_SMALL
        from test_gpu_dit import make_model, run
        P, inp, emu = small_case("full", True)
        m = make_model(DIT_SMALL, {k: v.clone() for k, v in P.items()})
        m.enable_fp8_attention()
        m.enable_multi_gpus_inference()
        calls = []
        real_call, real_rule = ops.call, ops.attn_tail_split

        def counting(name, *a):
            calls.append(name)
            return real_call(name, *a)

        ops.call = counting
        res = []
        for ov in ("1", "0"):  # the default schedule (one stream per CFG row), one batched launch per layer
            os.environ["SA_SP_OVERLAP"] = ov
            for every in (True, False):
                ops.attn_tail_split = (lambda before, n, dev: n) if every else (lambda before, n, dev: 0)
                del calls[:]
                par = run(m, inp)
                res.append((ov, every, calls.count("sa_attn_fwd_mxfp8_split"), calls.count("sa_attn_fwd_mxfp8"),
                            rel(par, emu), cos(par, emu), bool(torch.isfinite(par).all()),
                            par.contiguous().numpy().tobytes()))
        ops.call, ops.attn_tail_split = real_call, real_rule
        qret.put((rank, DIT_SMALL["num_layers"], inp["x"].shape[0], res))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sp_world2_fp8_attention_with_every_tile_split():
    """gloo world 2 sharing the GPU, as tests/test_gpu_fp8_attn.py::test_sp_world2_fp8_attention drives it, in the
    default schedule and the one-stream one, ops.attn_tail_split patched to split every tile and to split none"""
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
    outs = {}
    for rank, layers, B, rows in res:
        for ov, every, n_split, n_whole, e_emu, c_emu, finite, par in rows:
            print(f"rank {rank} overlap {ov} split {every}: {n_split} split / {n_whole} unsplit launches, vs emulated "
                  f"oracle rel {e_emu:.2e} cos {c_emu:.6f}")
            # the batched launch splits: once per layer.  The per-row launches of the default schedule stay unsplit
            # in this mode whatever the rule says (measured slower split: profiles/r10, DESIGN.md "fp8 attention")
            launches = layers * (B if ov == "1" else 1)
            split_here = every and ov == "0"
            assert (n_split, n_whole) == ((launches, 0) if split_here else (0, launches)), (rank, ov, every)
            assert finite
            assert e_emu < BAR["rel"] and c_emu > BAR["cos"], (rank, ov, every, e_emu, c_emu)
            outs.setdefault((ov, every), []).append(par)
    for key, (a, b) in outs.items():
        assert a == b, key  # the two ranks agree bit for bit
