"""The bf16 attention kernels of csrc/attention.hip element by element, against tests/attn_ref.py: inputs whose result
is known exactly (selection, uniform), inputs with integer scores held to one bf16 ulp of the fp64 softmax, and Gaussian
inputs held to the definition's own error -- through every entry point (sa_attn_fwd_map kernels 0-3, the key split and
its merge, sa_attn_cross3 in both wave counts, sa_attn_small in both kernels and its split, and the drop-in seam).

Every launch writes into a larger allocation filled with a sentinel, reads strided views with NaN in the pad columns,
and finds NaN in the K / V rows between and after its segments (V^T, kernel 3: NaN only past the 64-key block a
segment's last block stages, which the kernel's contract wants finite).  Every table holds one segment without keys.
tests/test_attn_ref_cpu.py shows on the CPU that the expectations hold under any block order and rescale policy, and
that the assertions used here reject a dropped / doubled / shifted key, shifted query rows, swapped V rows, swapped
heads, a neighbour's keys, swapped merge weights and a vocal frame off by one."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import attn_ref as A  # noqa: E402

from stableavatar_amd import ops  # noqa: E402
from stableavatar_amd.kbench import vt_layout  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = A.D
NAN = float("nan")
SETS = [("a", 3), ("b", 1), ("c", 3)]


@functools.lru_cache(maxsize=None)
def _case(family, name, heads, layout, kalign=1, d=D, round_q=True):
    return A.build(family, A.SHAPE_SETS[name], heads, layout, d=d, kalign=kalign, round_q=round_q)


def _families(name):
    return A.FAMILIES if name == "a" else A.FAMILIES[:-1]  # the ladder needs 5 key blocks: the 300-key segments of "a"


def _strided(t, stride_pad=64, extra_rows=8, fill=NAN):
    """t on the GPU as a view of a wider and longer allocation filled with `fill` -> (allocation, view)"""
    big = torch.full((t.shape[0] + extra_rows, t.shape[1] + stride_pad), fill, dtype=t.dtype, device=DEV)
    big[:t.shape[0], :t.shape[1]] = t.to(DEV)
    return big, big[:t.shape[0], :t.shape[1]]


def _segs_dev(segs):
    return torch.tensor(segs, dtype=torch.int32, device=DEV)


def _reach_zeroed(v, segs):
    """V for the V^T kernel: the rows past a segment's keys inside its last 64-key block hold zeros unless another
    segment owns them (the kernel's contract: finite through that block); every other unnamed row stays NaN"""
    v = v.clone()
    owned = torch.zeros(v.shape[0] + 64, dtype=torch.bool)
    reach = torch.zeros_like(owned)
    for _, _, k0, kl in segs:
        owned[k0:k0 + kl] = True
        reach[k0:k0 + (kl + 63) // 64 * 64] = True
    fix = (reach & ~owned)[:v.shape[0]]
    v[fix] = 0
    return v


def _launch(case, heads, out, kernel=0, split_tiles=0, accumulate=False, vt=None, q_pad=64):
    """one ops.attention launch of `case` into the view `out`"""
    _, q = _strided(case.q, q_pad)
    _, k = _strided(case.k)
    if vt is None:
        _, v = _strided(case.v)
    else:
        v = vt
    o_rows = None if case.o_rows is None else case.o_rows.to(DEV)
    ops.attention(q, k, v, out, _segs_dev(case.segs), len(case.segs), max(s[1] for s in case.segs), heads,
                  scale=case.scale, accumulate=accumulate, kernel=kernel, o_rows=o_rows, split_tiles=split_tiles)
    torch.cuda.synchronize()


def _run(case, heads, base=None, **kw):
    """-> the output rows on the CPU, after asserting that nothing outside the owned rows and columns changed"""
    C = heads * D
    n = case.want.shape[0]
    big = torch.full((n + 8, C + 64), A.SENTINEL, dtype=torch.bfloat16, device=DEV)
    if base is not None:
        big[:n, :C] = base.to(DEV)
    before = big.clone()
    _launch(case, heads, big[:n, :C], **kw)
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[:n, :C][case.owned.to(DEV)] = False
    assert torch.equal(big[keep], before[keep]), "rows or columns outside the segments' output changed"
    return big[:n, :C].cpu()


def _check_all(case, out, family, what, d=D):
    w = A.check(case, out, what, d=d)
    if family == "uniform":
        A.check_uniform_exact(case, out, what)
    return w


# ------------------------------------------------------------------------------------------------ sa_attn_fwd_map

@pytest.mark.parametrize("layout", A.LAYOUTS)
@pytest.mark.parametrize("name,heads", SETS)
def test_self_attention_kernels(name, heads, layout):
    """kernels 0 (auto), 1 (8 waves) and 2 (4 waves): selection and uniform exact, integer scores (nz 8 and 128, the
    ladder over both sides of each rescale threshold) within 1 ulp; 1 and 2 bit-identical, as the header states.
    shared_keys goes through a shuffled o_rows."""
    worst = {}
    for family in _families(name):
        case = _case(family, name, heads, layout)
        outs = {kern: _run(case, heads, kernel=kern) for kern in (0, 1, 2)}
        for kern, out in outs.items():
            worst[family] = max(worst.get(family, 0.0), _check_all(case, out, family, f"{family} kernel {kern}"))
        A.assert_equal_rows(outs[2], outs[1], case.segs, case.o_rows, what=f"{family}: kernel 2 vs kernel 1")
    print(f"sa_attn_fwd_map kernels 0/1/2, {name} x {heads} heads, {layout}: worst ulp {worst}")


@pytest.mark.parametrize("kernel", [1, 2, 3])
@pytest.mark.parametrize("layout", A.LAYOUTS)
def test_accumulate_onto_a_bf16_output_is_exact_on_selection(layout, kernel):
    """out = bf16(out + bf16(attention)): one rounding per addition; the segment without keys adds nothing"""
    heads, kalign = 3, 32 if kernel == 3 else 1
    case = _case("selection", "a", heads, layout, kalign)
    g = torch.Generator().manual_seed(9)
    base = (3 * torch.randn(case.want.shape, generator=g)).bfloat16()
    want = base.clone()
    want[case.owned] = A.bf16_add(base[case.owned], case.want[case.owned])
    vt = vt_layout(_reach_zeroed(case.v, case.segs).to(DEV), 3) if kernel == 3 else None
    out = _run(case, heads, base=base, kernel=kernel, accumulate=True, vt=vt)
    A.assert_equal_rows(out, want, case.segs, case.o_rows, what=f"accumulate kernel {kernel}")


def test_two_tables_with_q_row0_zero_write_disjoint_rows_of_one_output():
    """the per-row cross-attention tables of transformer.py: each launch's table starts at q_row0 = 0 of its own Q view
    and writes through its own o_rows (indexed by query row, so two such segments cannot share a launch)"""
    heads = 3
    case = _case("selection", "a", heads, "contiguous")
    n = case.q.shape[0]
    perm = torch.randperm(n + 9, generator=torch.Generator().manual_seed(4))[:n].int()
    big = torch.full((n + 9 + 8, heads * D + 64), A.SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = big[:n + 9, :heads * D]
    _, q = _strided(case.q)
    _, k = _strided(case.k)
    _, v = _strided(case.v)
    for kern, (q0, ql, k0, kl) in zip((1, 2, 1, 2, 0), case.segs):
        ops.attention(q[q0:], k, v, out, _segs_dev([[0, ql, k0, kl]]), 1, ql, heads, kernel=kern,
                      o_rows=perm[q0:q0 + ql].contiguous().to(DEV))
    torch.cuda.synchronize()
    want = torch.full((n + 9, heads * D), A.SENTINEL, dtype=torch.bfloat16)
    want[perm.long()] = case.want
    A.assert_equal_rows(out.cpu(), want, what="per-row tables")
    assert (big[:, heads * D:] == A.SENTINEL).all() and (big[n + 9:] == A.SENTINEL).all()


# ------------------------------------------------------------------------------------------------ kernel 3 (V^T)

@pytest.mark.parametrize("layout", A.LAYOUTS)
@pytest.mark.parametrize("name,heads", SETS)
def test_vt_kernel_with_v_through_vt_layout(name, heads, layout):
    """ATTN_VT_P32: key ranges on 32-key boundaries, V^T in P's permuted key order by kbench.vt_layout"""
    worst = {}
    for family in _families(name):
        case = _case(family, name, heads, layout, 32)
        vt = vt_layout(_reach_zeroed(case.v, case.segs).to(DEV), 3)
        out = _run(case, heads, kernel=ops.ATTN_VT_P32, vt=vt)
        worst[family] = _check_all(case, out, family, f"{family} kernel 3")
    print(f"sa_attn_fwd_map kernel 3, {name} x {heads} heads, {layout}: worst ulp {worst}")


@pytest.mark.parametrize("family", ["selection", "int8"])
@pytest.mark.parametrize("layout", A.LAYOUTS)
def test_vt_kernel_with_v_from_the_gemm_epilogue(layout, family):
    """the chain GEMM -> attention: V^T written by ops.linear(EPI_BF16_TP32) from a signed permutation weight (each
    output column is +- one input column of its head: exact), read by kernel 3"""
    heads = 3
    C = heads * D
    case = _case(family, "a", heads, layout, 32)
    g = torch.Generator().manual_seed(8)
    perm = torch.cat([h * D + torch.randperm(D, generator=g) for h in range(heads)])
    sign = (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    w = torch.zeros(C, C)
    w[torch.arange(C), perm] = sign
    x = _reach_zeroed(case.v, case.segs)
    x = torch.cat([x, torch.zeros(-x.shape[0] % 4, C, dtype=x.dtype)])  # EPI_BF16_T(P32): M % 4 == 0
    _, xd = _strided(x, fill=0.0)
    vt = ops.linear(xd, w.bfloat16().to(DEV), None, ops.EPI_BF16_TP32)
    out = _run(case, heads, kernel=ops.ATTN_VT_P32, vt=vt)
    moved = case._replace(want=(case.want[:, perm] * sign.to(case.want.dtype)),
                          a_abs=None if case.a_abs is None else case.a_abs[:, perm])
    print(f"GEMM(EPI_BF16_TP32) -> kernel 3, {family}, {layout}: worst ulp {A.check(moved, out, family)}")


# ------------------------------------------------------------------------------------------------ the key split

def _n_tiles(case, heads):
    return len(case.segs) * heads * -(-max(s[1] for s in case.segs) // 256)


@pytest.mark.parametrize("layout", A.LAYOUTS)
@pytest.mark.parametrize("name,heads", SETS)
def test_key_split(name, heads, layout):
    """sa_attn_fwd_split with 1, about half and all of the tiles split: the merge's weights exact on selection and
    uniform (at power-of-two key counts), integer scores within 1 ulp; tiles whose second half is empty (kv_len 1, 17,
    63, 64), a half with a single key (65), tiles without queries, and a split tile of the segment without keys, which
    gives zeros.  Regression: the merge divided 0 by 0 for that segment and wrote NaN (attn_split_merge_kernel)."""
    worst = {}
    nt = _n_tiles(_case("selection", name, heads, layout), heads)
    for family in _families(name):
        case = _case(family, name, heads, layout)
        for split in (1, nt // 2, nt):
            w = _check_all(case, _run(case, heads, split_tiles=split), family, f"{family} split {split}/{nt}")
            worst[family] = max(worst.get(family, 0.0), w)
    print(f"sa_attn_fwd_split, {name} x {heads} heads, {layout}: worst ulp {worst}")


def test_key_split_uniform_exact_at_power_of_two_key_counts():
    """both halves hold keys (128 + 128, 64 + 64): equal maxima, weights 1, and 1 / l exact"""
    heads, shapes = 3, [(300, 256), (33, 0), (40, 128)]
    case = A.build("uniform", shapes, heads, "gaps_descending")
    out = _run(case, heads, split_tiles=_n_tiles(case, heads))
    A.check_uniform_exact(case, out, "uniform split")
    assert all(kl & (kl - 1) == 0 for _, kl in shapes)


@pytest.mark.parametrize("layout", A.LAYOUTS)
def test_key_split_accumulates_through_the_merge(layout):
    heads = 3
    case = _case("selection", "c", heads, layout)
    g = torch.Generator().manual_seed(10)
    base = (3 * torch.randn(case.want.shape, generator=g)).bfloat16()
    want = base.clone()
    want[case.owned] = A.bf16_add(base[case.owned], case.want[case.owned])
    out = _run(case, heads, base=base, split_tiles=_n_tiles(case, heads), accumulate=True)
    A.assert_equal_rows(out, want, case.segs, case.o_rows, what="split accumulate")


# ------------------------------------------------------------------------------------------------ sa_attn_cross3

def _cross3(c, kw):
    C = kw["heads"] * D
    bufs = []
    for k, v in ((c.kt, c.vt), (c.ki, c.vi), (c.kv, c.vv)):  # K | V column slices of one buffer, NaN rows after
        _, kv = _strided(torch.cat([k, v], 1))
        bufs += [kv[:, :C], kv[:, C:]]
    _, q = _strided(c.q)
    n = kw["batch"] * kw["q_len"]
    big = torch.full((n + 8, C + 64), A.SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.attention_cross3(q, bufs[0], bufs[1], kw["t_len"], bufs[2], bufs[3], kw["i_len"], bufs[4], bufs[5], kw["nper"],
                         kw["tpf"], kw["n_frames"], big[:n, :C], kw["batch"], kw["q_len"], kw["heads"],
                         tok_offset=kw["tok_offset"], scale=c.scale)
    torch.cuda.synchronize()
    assert (big[n:] == A.SENTINEL).all() and (big[:, C:] == A.SENTINEL).all()
    return big[:n, :C].cpu()


@pytest.mark.parametrize("w4", ["1", "0"], ids=["w4", "w8"])
@pytest.mark.parametrize("ci", [0, 1])
def test_cross3(ci, w4, monkeypatch):
    """selection in the three sources at once (the exact bf16 three-way sum, the vocal key inside the query's frame),
    then each source alone on integer scores (nz 8, and 128 where the rescale fires) within 1 ulp"""
    monkeypatch.setenv("SA_X3_W4", w4)
    kw = A.X3_CASES[ci]
    c = A.cross3_selection(**kw)
    A.assert_equal_rows(_cross3(c, kw), c.want, what="cross3 selection")
    worst = {}
    for source in range(3):
        for nz in (8, 128):
            c = A.cross3_integer(source, nz=nz, **kw)
            worst[("text", "image", "vocal")[source], nz] = A.assert_within_ulps(
                _cross3(c, kw), c.want, c.a_abs, what=f"cross3 source {source} nz {nz}")
    print(f"sa_attn_cross3 SA_X3_W4={w4} case {ci}: worst ulp {worst}")


# ------------------------------------------------------------------------------------------------ sa_attn_small

def _small(case, heads, d, nsplit, q_pad=64, max_kv=None):
    C = heads * d
    n = case.want.shape[0]
    _, q = _strided(case.q, q_pad)
    _, k = _strided(case.k)
    _, v = _strided(case.v)
    big = torch.full((n + 8, C + 64), A.SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.attention_small(q, k, v, big[:n, :C], _segs_dev(case.segs), len(case.segs), max(s[1] for s in case.segs),
                        max_kv or max(s[3] for s in case.segs), heads, d, scale=case.scale, nsplit=nsplit)
    torch.cuda.synchronize()
    out = big[:n, :C].cpu()
    assert (big[n:] == A.SENTINEL).all() and (big[:, C:] == A.SENTINEL).all() and \
        (out[~case.owned] == A.SENTINEL).all()
    return out


@pytest.mark.parametrize("d", [64, 80, 192, 256, 640])
def test_small_attention(d):
    """the tiled kernel (d <= 256) unsplit, with the automatic split, 3 and 16 splits (16 > the key chunks: clamped) and
    its combine kernel; the one-wave-per-query kernel (d = 640).  Q' and P stay fp32 here."""
    heads, worst = 2, {}
    for family in ("selection", "uniform", "int8"):
        case = _case(family, "a", heads, "gaps_descending", 1, d, False)
        for nsplit in ((1, None, 3, 16) if d <= 256 else (1,)):
            w = _check_all(case, _small(case, heads, d, nsplit), family, f"{family} d {d} nsplit {nsplit}", d)
            worst[family] = max(worst.get(family, 0.0), w)
    print(f"sa_attn_small d {d}: worst ulp {worst}")


def test_small_attention_one_wave_kernel_by_alignment():
    """a Q row stride that is no multiple of 8 elements: sm2_applies rejects it, the one-wave-per-query kernel runs"""
    heads, d, worst = 2, 64, {}
    for family in ("selection", "uniform", "int8"):
        case = _case(family, "a", heads, "gaps_descending", 1, d, False)
        worst[family] = _check_all(case, _small(case, heads, d, 1, q_pad=4), family, family, d)
    print(f"sa_attn_small one-wave kernel (d 64, unaligned Q rows): worst ulp {worst}")


@pytest.mark.parametrize("nsplit", [1, None])
def test_small_attention_past_4096_keys(nsplit):
    """2 queries over 4097 keys: the tiled kernel's online softmax past the one-wave kernel's 4096-key score row"""
    heads, d, shapes = 2, 64, [(2, 4097), (1, 0)]
    for family in ("selection", "int8"):
        case = A.build(family, shapes, heads, "contiguous", d=d, round_q=False)
        w = A.check(case, _small(case, heads, d, nsplit), f"{family} 4097 keys", d=d)
        print(f"sa_attn_small 4097 keys nsplit {nsplit} {family}: worst ulp {w}")


# ------------------------------------------------------------------------------------------------ the drop-in seam

def test_drop_in_attention_on_selection_with_a_float32_input():
    from stableavatar_amd.attention import attention
    heads, B, ql, kl = 3, 2, 33, 65
    case = A.build("selection", [(ql, kl)] * B, heads)
    q, k, v = (t.float().view(B, -1, heads, D).to(DEV) for t in (case.q, case.k, case.v))
    out = attention(q, k, v)
    assert out.dtype == torch.float32 and out.shape == (B, ql, heads, D)
    A.assert_equal_rows(out.cpu().view(B * ql, heads * D), case.want.float(), case.segs, what="drop-in attention")


# ------------------------------------------------------------------------------------------------ Gaussian data

def _tile_rel(a, b, rows, cols):
    a, b = a[rows][:, cols].double(), b[rows][:, cols].double()
    return ((a - b).norm() / b.norm()).item()


def _gauss(variant, shapes, heads, d, seed):
    g = torch.Generator().manual_seed(seed + len(variant))
    nq, nk = sum(s[0] for s in shapes), sum(s[1] for s in shapes)
    q, k, v = (torch.randn(n, heads * d, generator=g) for n in (nq, nk, nk))
    if variant == "sharp":
        q = q * 4
    if variant == "k_offset":
        k = k + 3 * torch.randn(heads * d, generator=g)
    segs, q0, k0 = [], 0, 0
    for ql, kl in shapes:
        segs.append([q0, ql, k0, kl])
        q0, k0 = q0 + ql, k0 + kl
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), segs


def _assert_within_the_definitions_error(out, want, R, X, segs, heads, d, what):
    """per (segment, head): eR <= 1.5 dR + 2^-8 against the fp64 softmax on the prescaled Q, eX <= 1.5 dX against the
    fp64 softmax on the exact inputs (the rule and factor of tests/test_gpu_fp8_attn.py)"""
    for si, (q0, ql, _, _) in enumerate(segs):
        for h in range(heads):
            rows, cols = slice(q0, q0 + ql), slice(h * d, (h + 1) * d)
            eR, dR = _tile_rel(out, R, rows, cols), _tile_rel(want, R, rows, cols)
            eX, dX = _tile_rel(out, X, rows, cols), _tile_rel(want, X, rows, cols)
            print(f"{what} segment {si} head {h}: eR {eR:.3e} dR {dR:.3e} ({eR / dR:.3f}); eX {eX:.3e} dX {dX:.3e} "
                  f"({eX / dX:.3f})")
            assert eR <= 1.5 * dR + 2.0 ** -8, (what, si, h, eR, dR)
            assert eX <= 1.5 * dX, (what, si, h, eX, dX)


def _refs(q, k, v, segs, heads, d, round_q):
    scale = d ** -0.5
    R, X = (torch.zeros(q.shape, dtype=torch.float64) for _ in range(2))
    for q0, ql, k0, kl in segs:
        qs, ks, vs = q[q0:q0 + ql], k[k0:k0 + kl], v[k0:k0 + kl]
        R[q0:q0 + ql] = A.softmax64(A.scaled_q(qs, scale, round_q), ks, vs, heads)
        X[q0:q0 + ql] = A.softmax64(qs.double() * (scale * A.LOG2E), ks, vs, heads)
    return R, X


GAUSS_SHAPES = [(257, 300), (40, 65), (129, 1000)]


@pytest.mark.parametrize("variant", ["plain", "sharp", "k_offset"])
@pytest.mark.parametrize("entry", ["kernel1", "kernel2", "kernel3", "split"])
def test_gaussian_within_the_definitions_error(entry, variant):
    """what the structured inputs cannot see: exp2 at non-integer arguments and P's rounding"""
    heads = 3
    shapes = [(ql, -(-kl // 32) * 32 if entry == "kernel3" else kl) for ql, kl in GAUSS_SHAPES]
    q, k, v, segs = _gauss(variant, shapes, heads, D, 30)
    want = A.attention(q, k, v, segs, heads)
    R, X = _refs(q, k, v, segs, heads, D, True)
    case = A.Case(q, k, v, segs, None, want, torch.ones(q.shape[0], dtype=torch.bool), None, D ** -0.5)
    kw = dict(split_tiles=_n_tiles(case, heads)) if entry == "split" else dict(kernel=int(entry[-1]))
    if entry == "kernel3":
        kw["vt"] = vt_layout(v.to(DEV), 3)
    out = _run(case, heads, **kw)
    _assert_within_the_definitions_error(out, want, R, X, segs, heads, D, f"{entry} {variant}")


@pytest.mark.parametrize("variant", ["plain", "sharp", "k_offset"])
@pytest.mark.parametrize("d,q_pad", [(64, 64), (64, 4), (640, 64)], ids=["tiled", "one_wave_unaligned", "one_wave_640"])
def test_small_attention_gaussian_within_the_definitions_error(d, q_pad, variant):
    heads = 2
    q, k, v, segs = _gauss(variant, [(33, 300), (17, 65)], heads, d, 40)
    want = A.attention_small(q, k, v, segs, heads)
    R, X = _refs(q, k, v, segs, heads, d, False)
    case = A.Case(q, k, v, segs, None, want, torch.ones(q.shape[0], dtype=torch.bool), None, d ** -0.5)
    for nsplit in ((1, 3) if d <= 256 and q_pad == 64 else (1,)):
        out = _small(case, heads, d, nsplit, q_pad)
        _assert_within_the_definitions_error(out, want, R, X, segs, heads, d, f"small d {d} nsplit {nsplit} {variant}")


@pytest.mark.parametrize("variant", ["plain", "sharp", "k_offset"])
@pytest.mark.parametrize("w4", ["1", "0"], ids=["w4", "w8"])
def test_cross3_gaussian_within_the_definitions_error(w4, variant, monkeypatch):
    """per (batch row, head), against the exact sum of the three fp64 softmax attentions"""
    monkeypatch.setenv("SA_X3_W4", w4)
    kw = A.X3_CASES[0]
    B, Lq, heads, tl, il, nper, F = kw["batch"], kw["q_len"], kw["heads"], kw["t_len"], kw["i_len"], kw["nper"], \
        kw["n_frames"]
    g = torch.Generator().manual_seed(50 + len(variant))
    C, scale = heads * D, D ** -0.5
    q = torch.randn(B * Lq, C, generator=g) * (4 if variant == "sharp" else 1)
    src = [torch.randn(n, 2 * C, generator=g) for n in (B * tl, B * il, B * F * nper)]
    if variant == "k_offset":
        for s in src:
            s[:, :C] += 3 * torch.randn(C, generator=g)
    q, src = q.bfloat16(), [s.bfloat16() for s in src]
    c = A.Cross3Case(q, *(t for s in src for t in (s[:, :C], s[:, C:])), None, None, scale)
    args = (nper, kw["tpf"], F, B, Lq, heads, kw["tok_offset"])
    want = A.cross3(q, c.kt, c.vt, tl, c.ki, c.vi, il, c.kv, c.vv, *args, scale)
    R, X = (torch.zeros(q.shape, dtype=torch.float64) for _ in range(2))
    for b in range(B):
        for r0 in range(0, Lq, kw["tpf"]):
            rows = slice(b * Lq + r0, b * Lq + min(Lq, r0 + kw["tpf"]))
            f = (kw["tok_offset"] + r0) // kw["tpf"]
            for (kk, vv), (k0, n) in zip(((c.kt, c.vt), (c.ki, c.vi), (c.kv, c.vv)),
                                         ((b * tl, tl), (b * il, il), ((b * F + f) * nper, nper))):
                R[rows] += A.softmax64(A.scaled_q(q[rows], scale), kk[k0:k0 + n], vv[k0:k0 + n], heads)
                X[rows] += A.softmax64(q[rows].double() * (scale * A.LOG2E), kk[k0:k0 + n], vv[k0:k0 + n], heads)
    out = _cross3(c, kw)
    segs = [[b * Lq, Lq, 0, 0] for b in range(B)]
    _assert_within_the_definitions_error(out, want, R, X, segs, heads, D, f"cross3 SA_X3_W4={w4} {variant}")
