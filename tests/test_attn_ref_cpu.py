"""tests/attn_ref.py on the CPU: the definition against fp64 SDPA; the expectations of the exact inputs under an fp32
block-wise emulation of the flash loop, in both key-block orders and under both running-max policies (so they rest on
no order or policy the kernel is free to choose); and the two assertion helpers against deliberately wrong outputs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_ref as A  # noqa: E402

KVB = 64


# ------------------------------------------------------------------------------------------------ the definition

def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("ql,kl,heads,sharp", [(40, 300, 3, 1.0), (129, 65, 1, 4.0)])
def test_definition_agrees_with_fp64_sdpa(ql, kl, heads, sharp):
    """Its roundings: Q' to bf16 (2^-9 per element, ~2^-9 |S| ln 2 / sqrt(3) on a weight), P to bf16 (2^-9, averaging
    out over the keys) and the output to bf16 (2^-9 / sqrt(3) rms relative): well inside 2^-7 of the norm in all, and
    never below the output rounding alone."""
    g = torch.Generator().manual_seed(ql)
    q, k, v = (torch.randn(n, heads * A.D, generator=g).bfloat16() for n in (ql, kl, kl))
    q = (q.float() * sharp).bfloat16()
    segs = [[0, ql, 0, kl]]
    out = A.attention(q, k, v, segs, heads)
    sdpa = torch.nn.functional.scaled_dot_product_attention(
        *(t.double().view(-1, heads, A.D).transpose(0, 1) for t in (q, k, v))).transpose(0, 1).reshape(ql, -1)
    mine = A.softmax64(q.double() * A.prescale(A.D ** -0.5), k, v, heads)
    assert _rel(mine, sdpa) < 1e-6  # c is an fp32 product: 2^-24 relative on the scores
    e = _rel(out, sdpa)
    print(f"definition vs fp64 SDPA ({ql} x {kl}, q x {sharp}): {e:.3e}")
    assert 2.0 ** -11 < e < 2.0 ** -7
    small = A.attention_small(q, k, v, segs, heads)
    assert 2.0 ** -11 < _rel(small, sdpa) < 2.0 ** -8.5  # the output rounding alone


def test_accumulate_and_row_map():
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(n, A.D, generator=g).bfloat16() for n in (20, 30, 30))
    segs = [[0, 7, 0, 30], [7, 13, 3, 0]]
    base = torch.randn(25, A.D, generator=g).bfloat16()
    rows = torch.randperm(25, generator=g)[:20].int()
    plain = A.attention(q, k, v, segs, 1)
    assert (plain[7:] == 0).all()
    acc = A.attention(q, k, v, segs, 1, out=base, accumulate=True, o_rows=rows)
    want = base.clone()
    want[rows[:7].long()] = (base[rows[:7].long()].float() + plain[:7].float()).bfloat16()
    assert torch.equal(acc, want)  # the segment without keys adds nothing; unnamed rows keep their value


# ------------------------------------------------------------------------------------------------ the emulation

def emulate(q, k, v, segs, heads, scale, order, policy, out=None, o_rows=None, round_q=True):
    """The flash loop in fp32: 64-key blocks in `order` (fwd | rev), P = bf16(exp2(S - m)), l from the rounded P, O and l
    in fp32, o = bf16(O * (1 / l)).  policy lazy7: m = block max + 7 at the first block, and moved (for every row whose
    block max + 7 passes it) when some P >= 2; blockmax: m = the running row max after every block."""
    d = q.shape[1] // heads
    c = torch.tensor(A.prescale(scale), dtype=torch.float32)
    out = torch.zeros(q.shape[0], q.shape[1], dtype=torch.bfloat16) if out is None else out.clone()
    for q0, ql, k0, kl in segs:
        rows = torch.arange(q0, q0 + ql) if o_rows is None else o_rows[q0:q0 + ql].long()
        if kl == 0:
            out[rows] = 0
            continue
        qs = q[q0:q0 + ql].float() * c
        qs = A._heads(qs.bfloat16().float() if round_q else qs, heads)
        kh, vh = A._heads(k[k0:k0 + kl].float(), heads), A._heads(v[k0:k0 + kl].float(), heads)
        O = torch.zeros(heads, ql, d)
        L = torch.zeros(heads, ql, 1)
        m = None
        blocks = list(range(0, kl, KVB))
        for b0 in (blocks if order == "fwd" else blocks[::-1]):
            S = qs @ kh[:, b0:b0 + KVB].transpose(-1, -2)
            bm = S.amax(-1, keepdim=True)
            if policy == "lazy7":
                if m is None:
                    m_new = bm + 7
                elif (torch.exp2(S - m).bfloat16().float() >= 2).any():
                    m_new = torch.maximum(m, bm + 7)
                else:
                    m_new = m
            else:
                m_new = bm if m is None else torch.maximum(m, bm)
            if m is not None:
                alpha = torch.exp2(m - m_new)
                O, L = O * alpha, L * alpha
            m = m_new
            P = torch.exp2(S - m).bfloat16().float()
            L = L + P.sum(-1, keepdim=True)
            O = O + P @ vh[:, b0:b0 + KVB]
        o = (O * (1.0 / L)).bfloat16()
        out[rows] = o.transpose(0, 1).reshape(ql, -1)
    return out


WAYS = [(o, p) for o in ("fwd", "rev") for p in ("lazy7", "blockmax")]


def _emulated(case, heads, order, policy, round_q=True):
    base = torch.full(case.want.shape, A.SENTINEL, dtype=torch.bfloat16)
    out = emulate(case.q, case.k, case.v, case.segs, heads, case.scale, order, policy, base, case.o_rows, round_q)
    assert (out[~case.owned] == A.SENTINEL).all()
    return out


@pytest.mark.parametrize("layout", A.LAYOUTS)
@pytest.mark.parametrize("name,heads", [("a", 3), ("b", 1), ("c", 3)])
def test_expectations_hold_under_any_order_and_policy(name, heads, layout):
    shapes = A.SHAPE_SETS[name]
    worst = {}
    for family in A.FAMILIES if name == "a" else A.FAMILIES[:-1]:
        case = A.build(family, shapes, heads, layout)
        for order, policy in WAYS:
            out = _emulated(case, heads, order, policy)
            w = A.check(case, out, f"{family} {order} {policy}")
            worst[family] = max(worst.get(family, 0.0), w)
            if family == "uniform":
                A.check_uniform_exact(case, out, f"uniform {order} {policy}")
        # and the definition itself (per-row max)
        A.check(case, A.attention(case.q, case.k, case.v, case.segs, heads, case.scale,
                                  torch.full(case.want.shape, A.SENTINEL, dtype=torch.bfloat16), o_rows=case.o_rows),
                f"{family} definition")
    print(f"{name} {layout}: worst ulp {worst}")


def test_uniform_is_exact_at_power_of_two_key_counts():
    """the key-split test's case: 256 and 128 keys"""
    case = A.build("uniform", [(300, 256), (33, 0), (40, 128)], 3, "gaps_descending")
    for order, policy in WAYS:
        A.check_uniform_exact(case, _emulated(case, 3, order, policy), f"{order} {policy}")


@pytest.mark.parametrize("d", [64, 80, 192, 256, 640])
def test_small_attention_expectations(d):
    """the small-attention form (Q' and P in fp32) at the head dims and shapes of the GPU test"""
    for family, shapes in [(f, A.SHAPE_SETS["a"]) for f in ("selection", "uniform", "int8")] + (
            [(f, [(2, 4097), (1, 0)]) for f in ("selection", "int8")] if d == 64 else []):
        case = A.build(family, shapes, 2, "gaps_descending" if len(shapes) > 2 else "contiguous", d=d, round_q=False)
        out = A.attention(case.q, case.k, case.v, case.segs, 2, case.scale,
                          torch.full(case.want.shape, A.SENTINEL, dtype=torch.bfloat16), round_q=False, round_p=False)
        A.check(case, out, f"{family} d {d}")
        A.check(case, _emulated(case, 2, "fwd", "blockmax", round_q=False), f"{family} d {d} emulated")


def test_ladder_reaches_both_sides_of_each_threshold():
    """the ladder queries' scores are the levels, so consecutive block maxima differ by 7, 8, 9 and 156"""
    case = A.build("ladder", A.SHAPE_SETS["a"], 3)
    for seg, levels in A.LADDERS.items():
        q0, _, k0, kl = case.segs[seg]
        s = A._heads(A.scaled_q(case.q[q0:q0 + 2], case.scale), 3) @ A._heads(case.k[k0:k0 + kl].double(), 3).transpose(
            -1, -2)
        want = torch.tensor([levels[j // KVB] for j in range(kl)], dtype=torch.float64)
        assert torch.equal(s[:, 0], want.expand(3, kl)) and torch.equal(s[:, 1], -want.expand(3, kl))
    rises = lambda lv: [b - a for a, b in zip(lv, lv[1:])]  # noqa: E731
    assert rises(A.LADDER) == [7, 8, 9, 156] and rises(A.LADDER8)[0] == 8


# ------------------------------------------------------------------------------------------------ the key split

def split_partials(q, k, v, heads, scale, kper):
    """the two key halves' (O, m, l) in fp64 on the rounded operands (m = the half's row max)"""
    parts = []
    for kk, vv in ((k[:kper], v[:kper]), (k[kper:], v[kper:])):
        s = A._heads(A.scaled_q(q, scale), heads) @ A._heads(kk.double(), heads).transpose(-1, -2)
        m = s.amax(-1, keepdim=True)
        p = torch.exp2(s - m).float().bfloat16().double()
        parts.append((p @ A._heads(vv.double(), heads), m, p.sum(-1, keepdim=True)))
    return parts


def merge(parts, swap=False):
    (O0, m0, l0), (O1, m1, l1) = parts
    M = torch.maximum(m0, m1)
    w0, w1 = torch.exp2(m0 - M), torch.exp2(m1 - M)
    if swap:
        w0, w1 = w1, w0
    o = (w0 * O0 + w1 * O1) / (w0 * l0 + w1 * l1)
    return o.transpose(0, 1).reshape(o.shape[1], -1).bfloat16()


# ------------------------------------------------------------------------------------------------ mutants

MUT_SHAPES = [(33, 300), (40, 256), (129, 300)]  # the mutants act on segment 1 (a power-of-two kv_len: uniform exact)
MUT_HEADS = 3


def _mutant(name, case):
    """a deliberately wrong output for `case` (contiguous layout): the definition with one thing off in segment 1"""
    q, k, v, segs = case.q, case.k, case.v, [list(s) for s in case.segs]
    q0, ql, k0, kl = segs[1]
    run = lambda q_, k_, v_, s_: A.attention(q_, k_, v_, s_, MUT_HEADS, case.scale)  # noqa: E731
    if name == "last_key_dropped":
        segs[1][3] -= 1
    elif name == "key_counted_twice":
        dup = k0 + 37
        k = torch.cat([k[:k0 + kl], k[dup:dup + 1], k[k0 + kl:]])
        v = torch.cat([v[:k0 + kl], v[dup:dup + 1], v[k0 + kl:]])
        segs[1][3] += 1
        segs[2][2] += 1
    elif name == "key_range_shifted":
        segs[1][2] += 1
    elif name == "query_rows_shifted":
        out = run(q, k, v, segs)
        out[q0:q0 + ql - 1] = out[q0 + 1:q0 + ql].clone()
        return out
    elif name == "v_rows_swapped_in_a_chunk":
        v = v.clone()
        v[[k0 + 67, k0 + 84]] = v[[k0 + 84, k0 + 67]]  # keys 3 and 20 of the 32-key chunk 2: two lane groups
    elif name == "heads_swapped":
        out = run(q, k, v, segs)
        out[q0:q0 + ql, :2 * A.D] = torch.cat([out[q0:q0 + ql, A.D:2 * A.D], out[q0:q0 + ql, :A.D]], 1)
        return out
    elif name == "keys_of_the_next_segment":
        segs[1][2], segs[1][3] = segs[2][2], min(kl, segs[2][3])
    elif name == "merge_weights_swapped":
        out = run(q, k, v, segs)
        kper = ((kl + 1) // 2 + KVB - 1) // KVB * KVB - KVB  # unequal halves: 64 and 192 keys
        out[q0:q0 + ql] = merge(split_partials(q[q0:q0 + ql], k[k0:k0 + kl], v[k0:k0 + kl], MUT_HEADS, case.scale,
                                               kper), swap=True)
        return out
    else:
        raise KeyError(name)
    return run(q, k, v, segs)


# which family is meant to see which mutant.  False = cannot: uniform weighs every key alike, so it is blind to where
# a V row sits, to which query a row belongs and to the merge weights (equal maxima: both are 1); selection sees a
# dropped, doubled, moved or shifted-out key only where it is some query's match (it finds its key by content, wherever
# the row sits: a 40-query segment over 256 keys rarely picks the one key a mutant touches; a doubled match carries
# the same V twice) and is blind to them otherwise
SEES = {
    "last_key_dropped":          dict(selection=False, uniform=True, int8=True, int128=True),
    "key_counted_twice":         dict(selection=False, uniform=True, int8=True, int128=True),
    "key_range_shifted":         dict(selection=False, uniform=True, int8=True, int128=True),
    "query_rows_shifted":        dict(selection=True, uniform=False, int8=True, int128=True),
    "v_rows_swapped_in_a_chunk": dict(selection=False, uniform=False, int8=True, int128=True),
    "heads_swapped":             dict(selection=True, uniform=True, int8=True, int128=True),
    "keys_of_the_next_segment":  dict(selection=True, uniform=True, int8=True, int128=True),
    "merge_weights_swapped":     dict(selection=True, uniform=False, int8=True, int128=True),
}


def _rejected(case, out, family=""):
    try:
        A.check(case, out)
        if family == "uniform":
            A.check_uniform_exact(case, out)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", list(SEES))
def test_mutants_are_rejected(name):
    seen = {}
    for family, meant in SEES[name].items():
        case = A.build(family, MUT_SHAPES, MUT_HEADS)
        assert not _rejected(case, A.attention(case.q, case.k, case.v, case.segs, MUT_HEADS, case.scale), family), family
        seen[family] = _rejected(case, _mutant(name, case), family)
        if meant:
            assert seen[family], f"{family} accepts the mutant {name}"
    print(f"{name}: rejected by {[f for f, s in seen.items() if s]}; not seen by {[f for f, s in seen.items() if not s]}")
    assert any(seen.values())


def test_v_swap_of_a_selected_key_is_rejected_by_selection():
    """selection sees a V swap where a swapped key is some query's match: with 300 queries over 96 keys every key is"""
    case = A.build("selection", [(300, 96)], 1)
    v = case.v.clone()
    v[[3, 20]] = v[[20, 3]]
    assert _rejected(case, A.attention(case.q, case.k, v, case.segs, 1, case.scale))


def test_vocal_frame_off_by_one_is_rejected():
    for kw in A.X3_CASES:
        args = (kw["nper"], kw["tpf"], kw["n_frames"], kw["batch"], kw["q_len"], kw["heads"], kw["tok_offset"])
        for c in (A.cross3_selection(**kw), A.cross3_integer(2, **kw)):
            good, bad = (A.cross3(c.q, c.kt, c.vt, kw["t_len"], c.ki, c.vi, kw["i_len"], c.kv, c.vv, *args, c.scale,
                                  frame_shift=s) for s in (0, 1))
            if c.a_abs is None:
                A.assert_equal_rows(good, c.want)
                with pytest.raises(AssertionError, match="first at"):
                    A.assert_equal_rows(bad, c.want)
            else:
                A.assert_within_ulps(good, c.want, c.a_abs)
                with pytest.raises(AssertionError, match="past 1 ulp"):
                    A.assert_within_ulps(bad, c.want, c.a_abs)


def test_helpers_name_the_first_wrong_element():
    case = A.build("selection", MUT_SHAPES, MUT_HEADS)
    out = case.want.clone()
    out[33 + 5, A.D + 7] += 1
    with pytest.raises(AssertionError, match="segment 1 head 1 row 5 column 7"):
        A.assert_equal_rows(out, case.want, case.segs)
    case = A.build("int8", MUT_SHAPES, MUT_HEADS)
    out = case.want.float().bfloat16()
    out[2, 3] = float("nan")
    with pytest.raises(AssertionError, match="segment 0 head 0 row 2 column 3"):
        A.assert_within_ulps(out, case.want, case.a_abs, segs=case.segs)
