"""The block-sparse self-attention on the MI355X: sa_attn_fwd_sparse (kernels 1 and 3) byte for byte against the dense
kernels -- on the full list, and per query tile against the dense kernel run over gathered copies of the listed key
blocks -- and against tests/attn_ref.py's ulp contract on those gathered problems; unlisted blocks never read (NaN),
empty lists, guard bytes; then the DiT forward with enable_sparse_attention against the masked oracle, against the
mode off at a window of all frames, and under sequence parallelism (gloo, world 2 on one GPU).

Shapes: 2 heads, two segments with gaps between their query and key rows, q_len 300 (two query tiles, the second 44
rows), kv_len 6 x 64 + 40 (seven key blocks, the last ragged).  The lists have 7, 1, 1, 3, 2, 4 and 0 entries: the
first-block path alone, both halves of the unrolled loop, its two exits, the tail block first, last and absent."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import attn_ref as A  # noqa: E402
import sparse_attn_util as U  # noqa: E402
from mp_util import collect  # noqa: E402

from stableavatar_amd import _lib, ops, sparse_attn  # noqa: E402
from stableavatar_amd.kbench import vt_layout  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, HEADS, C = A.D, 2, 2 * A.D
QL, KL, NKB = 300, 6 * 64 + 40, 7
Q0, K0 = (0, 307), (0, 480)  # 7 unnamed query rows and 56 unnamed key rows between the segments; 480 = 15 x 32
NQ, NK = Q0[1] + QL, K0[1] + KL
TILES = ((0, 256), (256, 44))  # (first query, rows) of a segment's two tiles
ALL = list(range(NKB))
TABLES = {"full": (ALL, ALL), "all_0": (ALL, [0]), "tail_025": ([6], [0, 2, 5]), "16_0123": ([1, 6], [0, 1, 2, 3]),
          "empty_all": ([], ALL)}
NAN = float("nan")


def _table(name):
    a, b = TABLES[name]
    ptr = torch.tensor([0, len(a), len(a) + len(b)], dtype=torch.int32)
    idx = torch.tensor(a + b, dtype=torch.int32)
    sparse_attn.validate(ptr, idx, QL, KL)
    return ptr, idx


def _key_rows(blocks):
    """the key rows (relative to the segment) of the listed blocks, ascending"""
    return torch.cat([torch.arange(kb * 64, min(kb * 64 + 64, KL)) for kb in blocks]) if blocks else torch.zeros(0).long()


_PROBLEMS = {}


def problem(family, table):
    """q / k / v rows of the two segments (NaN in the rows no segment names) and, per (segment, tile), the expectation
    on the gathered problem: `selection` -- K rows +-1, each query 16 x one key row drawn from its tile's listed blocks,
    expected V of that key exactly (attn_ref.selection's recipe, its score gap asserted over the listed keys);
    `int` -- attn_ref.integer_scores' recipe (Q in {0, +-8}, K in {-1, 0, 1}, scale INT_SCALE), expected the fp64
    softmax attention over the listed keys and its a_abs.  K and V do not depend on the table."""
    key = (family, table)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    g = torch.Generator().manual_seed(31 if family == "selection" else 37)
    scale = D ** -0.5 if family == "selection" else A.INT_SCALE
    q = torch.full((NQ, C), NAN, dtype=torch.bfloat16)
    k = torch.full((NK, C), NAN, dtype=torch.bfloat16)
    v = torch.full((NK, C), NAN, dtype=torch.bfloat16)
    exact = family == "selection"
    want = torch.zeros(NQ, C, dtype=torch.bfloat16 if exact else torch.float64)
    a_abs = None if exact else torch.zeros(NQ, C, dtype=torch.float64)
    for s in range(2):
        if exact:
            ks = (torch.randint(0, 2, (KL, C), generator=g) * 2 - 1).float().bfloat16()
        else:
            ks = torch.randint(-1, 2, (KL, C), generator=g).float().bfloat16()
        vs = A._v_rows(KL, C, g)
        k[K0[s]:K0[s] + KL], v[K0[s]:K0[s] + KL] = ks, vs
        for (t0, tl), blocks in zip(TILES, TABLES[table]):
            rows = _key_rows(blocks)
            sl = slice(Q0[s] + t0, Q0[s] + t0 + tl)
            if exact:
                if len(rows) == 0:
                    q[sl] = (torch.randint(0, 2, (tl, C), generator=g) * 2 - 1).float().bfloat16()
                    continue
                pi = rows[torch.randint(0, len(rows), (tl,), generator=g)]
                q[sl] = (A.SELECT_A * ks[pi].float()).bfloat16()
                sc = A._heads(A.scaled_q(q[sl], scale), HEADS) @ A._heads(ks[rows].double(), HEADS).transpose(-1, -2)
                top2 = sc.topk(min(2, len(rows)), -1).values
                assert (rows[sc.argmax(-1)] == pi).all()
                assert len(rows) == 1 or (top2[..., 0] - top2[..., 1]).min() >= A.SELECT_MIN_GAP
                want[sl] = vs[pi]
            else:
                qt = torch.zeros(tl, HEADS, D)
                at = torch.rand(tl, HEADS, D, generator=g).argsort(-1)[..., :8]
                qt.scatter_(-1, at, (torch.randint(0, 2, at.shape, generator=g) * 16 - 8).float())
                q[sl] = qt.reshape(tl, C).bfloat16()
                if len(rows):
                    qd = A.scaled_q(q[sl], scale)
                    assert torch.equal(qd, q[sl].double() / 8)
                    want[sl], a_abs[sl] = A.softmax64(qd, ks[rows], vs[rows], HEADS, with_abs=True)
    owned = torch.zeros(NQ, dtype=torch.bool)
    for s in range(2):
        owned[Q0[s]:Q0[s] + QL] = True
    _PROBLEMS[key] = dict(q=q, k=k, v=v, want=want, a_abs=a_abs, owned=owned, scale=scale)
    return _PROBLEMS[key]


SEGS = [[Q0[s], QL, K0[s], KL] for s in range(2)]


def _strided(t, fill=NAN, pad=64, extra=8):
    big = torch.full((t.shape[0] + extra, t.shape[1] + pad), fill, dtype=t.dtype, device=DEV)
    big[:t.shape[0], :t.shape[1]] = t.to(DEV)
    return big[:t.shape[0], :t.shape[1]]


def _o_rows(seed=5):
    """a shuffled output row map into an allocation 9 rows longer, as attn_ref's shared_keys layout"""
    return torch.randperm(NQ + 9, generator=torch.Generator().manual_seed(seed))[:NQ].int()


def _unlisted_nan(t, table):
    """t (key rows) with the blocks that neither tile of `table` lists filled with NaN"""
    t = t.clone()
    listed = set(TABLES[table][0]) | set(TABLES[table][1])
    for s in range(2):
        for kb in range(NKB):
            if kb not in listed:
                t[K0[s] + kb * 64:K0[s] + min(kb * 64 + 64, KL)] = NAN
    return t


def _vt(v):
    """kernel 3's V^T of the key rows v: the unnamed rows inside a segment's last 64-key block hold zeros (the kernel's
    contract: finite through that block); kbench.vt_layout's permuted order"""
    v = v.clone()
    for s in range(2):
        v[K0[s] + KL:min(K0[s] + NKB * 64, NK)] = 0
    return vt_layout(v.to(DEV), 3)


def _gathered(p, table, kernel):
    """the dense problem of one segment per (segment, tile): copies of the listed key blocks one after the other from a
    64-row boundary -> (k_g, v_g or V^T_g, segs_g); an empty list is a segment without keys"""
    kk, vv = p["k"], p["v"]
    segs, kparts, row = [], [], 0
    for s in range(2):
        for (t0, tl), blocks in zip(TILES, TABLES[table]):
            rows = _key_rows(blocks)
            segs.append([Q0[s] + t0, tl, row, len(rows)])
            kparts.append((row, K0[s] + rows, K0[s], blocks))
            row += -(-len(rows) // 64) * 64
    k_g = torch.full((row + 64, C), NAN, dtype=torch.bfloat16)
    v_g = torch.full((row + 64, C), NAN, dtype=torch.bfloat16)
    for r0, src, _, _ in kparts:
        k_g[r0:r0 + len(src)], v_g[r0:r0 + len(src)] = kk[src], vv[src]
    if kernel != 3:
        return _strided(k_g), _strided(v_g), segs
    vt = _vt(vv)
    vt_g = torch.zeros(C, row + 64, dtype=torch.bfloat16, device=DEV)
    for r0, _, k0, blocks in kparts:  # by 64-column blocks: the per-32 permutation travels with them
        for j, kb in enumerate(blocks):
            vt_g[:, r0 + 64 * j:r0 + 64 * j + 64] = vt[:, k0 + 64 * kb:k0 + 64 * kb + 64]
    return _strided(k_g), vt_g, segs


def _launch(p, kernel, segs, k, v, max_q, o_rows, base, blocks=None):
    """-> the output rows on the CPU, after asserting that the guard rows and columns around them are intact"""
    n = NQ + (9 if o_rows is not None else 0)
    big = torch.full((n + 8, C + 64), A.SENTINEL, dtype=torch.bfloat16, device=DEV)
    if base is not None:
        big[:n, :C] = base.to(DEV)
    before = big.clone()
    own = p["owned"] if o_rows is None else torch.zeros(n, dtype=torch.bool).index_fill_(0, o_rows.long()[p["owned"]], True)
    kw = {} if blocks is None else dict(blocks=tuple(t.to(DEV) for t in blocks))
    ops.attention(_strided(p["q"]), k, v, big[:n, :C], torch.tensor(segs, dtype=torch.int32, device=DEV), len(segs),
                  max_q, HEADS, scale=p["scale"], accumulate=base is not None, kernel=kernel,
                  o_rows=None if o_rows is None else o_rows.to(DEV), **kw)
    torch.cuda.synchronize()
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[:n, :C][own.to(DEV)] = False
    assert torch.equal(big[keep], before[keep]), "rows or columns outside the segments' output changed"
    return big[:n, :C].cpu()


def _sparse(p, table, kernel, o_rows=None, base=None, nan_unlisted=False):
    k, v = p["k"], p["v"]
    if nan_unlisted:
        k, v = _unlisted_nan(k, table), _unlisted_nan(v, table)
    vd = _vt(v) if kernel == 3 else _strided(v)
    return _launch(p, kernel, SEGS, _strided(k), vd, QL, o_rows, base, blocks=_table(table))


def _dense(p, kernel, o_rows=None, base=None):
    vd = _vt(p["v"]) if kernel == 3 else _strided(p["v"])
    return _launch(p, kernel, SEGS, _strided(p["k"]), vd, QL, o_rows, base)


def _dense_gathered(p, table, kernel, o_rows=None, base=None):
    k_g, v_g, segs = _gathered(p, table, kernel)
    return _launch(p, kernel, segs, k_g, v_g, 256, o_rows, base)


def _base(n, seed=9):
    return (3 * torch.randn(n, C, generator=torch.Generator().manual_seed(seed))).bfloat16()


COMBOS = [(False, False), (True, False), (False, True), (True, True)]  # (o_rows, accumulate)


def _combo(use_map, acc):
    o_rows = _o_rows() if use_map else None
    return o_rows, (_base(NQ + (9 if use_map else 0)) if acc else None)


def _case(p, o_rows, base):
    """attn_ref.Case of the gathered problem on the launch's output rows (accumulate: onto `base`, selection only)"""
    n = NQ + (9 if o_rows is not None else 0)
    rows = torch.arange(NQ) if o_rows is None else o_rows.long()
    want = torch.zeros(n, C, dtype=p["want"].dtype)
    want[rows] = p["want"]
    owned = torch.zeros(n, dtype=torch.bool)
    owned[rows] = p["owned"]
    a_abs = None
    if p["a_abs"] is not None:
        a_abs = torch.zeros(n, C, dtype=torch.float64)
        a_abs[rows] = p["a_abs"]
    if base is not None:
        want[owned] = A.bf16_add(base[owned], want[owned])
    return A.Case(p["q"], p["k"], p["v"], SEGS, o_rows, want, owned, a_abs, p["scale"])


@pytest.mark.parametrize("family", ["selection", "int"])
@pytest.mark.parametrize("kernel", [0, 1, 3])
def test_full_list_is_the_dense_kernel_byte_for_byte(kernel, family):
    p = problem(family, "full")
    for use_map, acc in COMBOS:
        o_rows, base = _combo(use_map, acc)
        got, want = _sparse(p, "full", kernel, o_rows, base), _dense(p, kernel or 1, o_rows, base)
        A.assert_equal_rows(got, want, SEGS, o_rows, what=f"full list, kernel {kernel}, map {use_map}, accumulate {acc}")
        if not acc:
            w = A.check(_case(p, o_rows, None), got, f"full list {family} kernel {kernel}")
            print(f"full list, {family}, kernel {kernel}, map {use_map}: worst ulp {w}")


@pytest.mark.parametrize("family", ["selection", "int"])
@pytest.mark.parametrize("table", [t for t in TABLES if t != "full"])
@pytest.mark.parametrize("kernel", [1, 3])
def test_lists_are_the_dense_kernel_on_gathered_blocks(kernel, table, family):
    """per-tile lists: byte-identical to the dense kernel over gathered copies of the listed blocks (one segment per
    query tile), inside the header's ulp contract on those gathered problems, unchanged with NaN in every unlisted
    block of K and V; an empty list writes zeros and adds nothing"""
    p = problem(family, table)
    for use_map, acc in COMBOS:
        o_rows, base = _combo(use_map, acc)
        what = f"{table} {family} kernel {kernel}, map {use_map}, accumulate {acc}"
        got = _sparse(p, table, kernel, o_rows, base)
        A.assert_equal_rows(got, _dense_gathered(p, table, kernel, o_rows, base), SEGS, o_rows, what=what + " vs gathered")
        A.assert_equal_rows(_sparse(p, table, kernel, o_rows, base, nan_unlisted=True), got, SEGS, o_rows,
                            what=what + " with NaN in the unlisted blocks")
        if not acc or family == "selection":
            w = A.check(_case(p, o_rows, base), got, what)
            print(f"{what}: worst ulp {w}")
        for s in range(2):  # the tiles with an empty list: zeros, or the base untouched
            for (t0, tl), blocks in zip(TILES, TABLES[table]):
                if not blocks:
                    rows = torch.arange(Q0[s] + t0, Q0[s] + t0 + tl)
                    rows = rows if o_rows is None else o_rows.long()[rows]
                    assert torch.equal(got[rows], base[rows] if acc else torch.zeros(tl, C, dtype=torch.bfloat16)), what


def test_entry_refuses_a_table_of_another_tile_count():
    p = problem("selection", "full")
    ptr, idx = _table("full")
    for bad in (ptr[:2].contiguous(), torch.cat([ptr, ptr[-1:]])):  # one tile short, one too many
        out = torch.zeros(NQ, C, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(_lib.KernelError, match="bad argument"):
            ops.attention(_strided(p["q"]), _strided(p["k"]), _strided(p["v"]), out,
                          torch.tensor(SEGS, dtype=torch.int32, device=DEV), 2, QL, HEADS, kernel=1,
                          blocks=(bad.to(DEV), idx.to(DEV)))
        torch.cuda.synchronize()
        assert not out.any()


# ------------------------------------------------------------------------------------------------ the DiT forward

def _model(peak=False):
    from golden_cases import DIT_SMALL
    from test_gpu_dit import make_model
    return make_model(DIT_SMALL, U.params(peak))


def _run(m, inp):
    from test_gpu_dit import run
    return run(m, inp)


def _count_launches(monkeypatch):
    names = []
    real = _lib.call

    def rec(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(ops, "call", rec)
    return names


@pytest.mark.parametrize("case", ["full", "short"])
def test_forward_golden_grids_vs_masked_oracle(case, monkeypatch):
    """DIT_SMALL's golden grids with enable_sparse_attention(1) against the masked oracle, the forward bar of
    tests/test_gpu_dit.py.  On these grids every window lists every block (tests/test_sparse_attn_cpu.py shows it), so
    this checks the sparse launch path of the forward, not the mask; the tall grid below checks the mask."""
    _, inp, emu = U.small_case(case, 1)
    m = _model()
    m.enable_sparse_attention(window_frames=1)
    names = _count_launches(monkeypatch)
    out = _run(m, inp)
    assert names.count("sa_attn_fwd_sparse") == 2  # one self-attention launch per layer
    r, c = U.rel(out, emu), U.cos(out, emu)
    print(f"DIT_SMALL {case}, window 1: vs masked oracle rel-L2 {r:.3e} cosine {c:.6f}")
    assert r < 2e-2 and c > 0.9995, (r, c)


@pytest.mark.parametrize("rows_kernel", [False, True], ids=["vt_site", "rows_site"])
@pytest.mark.parametrize("window", [1, 0])
def test_forward_tall_grid_vs_masked_oracle(window, rows_kernel):
    """the grid at which the table leaves tiles out (sparse_attn_util.TALL, sharper scores): the forward with the mode
    on is inside the forward bar around the masked oracle, and the dense forward is outside it, so the table took
    effect; both bf16 call sites (V^T kernel 3, and _self_attn's row-major kernel with attn_kernel = 1)"""
    _, inp, emu = U.small_case(U.TALL, window, 1, True)
    m = _model(peak=True)
    if rows_kernel:
        m.attn_kernel = 1
    dense = _run(m, inp)
    m.enable_sparse_attention(window_frames=window)
    out = _run(m, inp)
    r, c = U.rel(out, emu), U.cos(out, emu)
    rd, cd = U.rel(dense, emu), U.cos(dense, emu)
    print(f"tall, window {window}, {'rows' if rows_kernel else 'V^T'} site: vs masked oracle rel-L2 {r:.3e} cosine "
          f"{c:.6f}; the dense forward vs the masked oracle rel-L2 {rd:.3e} cosine {cd:.6f}")
    assert r < 2e-2 and c > 0.9995, (r, c)
    assert not (rd < 2e-2 and cd > 0.9995), (rd, cd)


@pytest.mark.parametrize("case", ["full", U.TALL])
def test_forward_window_of_all_frames_is_the_mode_off_byte_for_byte(case, monkeypatch):
    from golden_cases import DIT_SMALL
    inp = U.inputs(DIT_SMALL, case)
    m = _model()
    off = _run(m, inp)
    names = _count_launches(monkeypatch)
    off2 = _run(m, inp)
    seq_off = list(names)
    m.enable_sparse_attention(window_frames=5)  # five latent frames: every frame within the window
    names.clear()
    on = _run(m, inp)
    assert names.count("sa_attn_fwd_sparse") == 2  # one self-attention launch per layer, nothing else changed
    assert ["sa_attn_fwd_map" if n == "sa_attn_fwd_sparse" else n for n in names] == seq_off
    assert torch.equal(on, off) and torch.equal(off2, off)
    m.enable_sparse_attention(5, enabled=False)
    names.clear()
    again = _run(m, inp)
    assert names == seq_off and "sa_attn_fwd_sparse" not in names  # off again: the launches made before
    assert torch.equal(again, off)


def _sp_worker(rank, world, port, qret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    import torch.distributed as dist
    sys.path.insert(0, HERE)
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        from golden_cases import DIT_SMALL
        inp = U.inputs(DIT_SMALL, U.TALL)
        m = _model()
        m.enable_sparse_attention(window_frames=0)
        res = []
        single = _run(m, inp)
        m.enable_sparse_attention(0, enabled=False)
        dense = _run(m, inp)
        m.enable_sparse_attention(window_frames=0)
        m.enable_multi_gpus_inference()
        for ov in ("0", "2", "3", "4"):
            os.environ["SA_SP_OVERLAP"] = ov
            par = _run(m, inp)
            res.append((ov, bool(torch.equal(par, single)), ((par - single).norm() / single.norm()).item(),
                        ((single - dense).norm() / dense.norm()).item()))
        qret.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sequence_parallel_world_2_is_the_single_gpu_bit_for_bit():
    """gloo, world 2 on one GPU, every exchange schedule, window 0 on the tall grid (4 of 10 tiles left out): the same
    table on every rank, bit-identical to the single GPU with the mode on"""
    import tempfile
    ctx = mp.get_context("spawn")
    qret = ctx.Queue()
    port = os.path.join(tempfile.mkdtemp(prefix="sa_rdv_"), "store")
    procs = [ctx.Process(target=_sp_worker, args=(r, 2, port, qret)) for r in range(2)]
    for p in procs:
        p.start()
    res = collect(procs, qret, 2, timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, rows in res:
        for ov, same, err, moved in rows:
            print(f"world 2 rank {rank} overlap {ov}: bit-identical to one GPU {same} (rel {err:.1e}); the mode moved "
                  f"the single-GPU output by {moved:.2e}")
            assert moved > 1e-3  # the table left tiles out
            assert same, (rank, ov, err)
