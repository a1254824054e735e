"""The definition of the bf16 attention family (csrc/attention.hip) in plain torch, the inputs whose result is known
exactly, and the two assertions the CPU and GPU tests share.  No GPU and no kernel code.

The contract (include/stableavatar_hip.h, next to sa_attn_fwd):
  * c = fp32(scale) * fp32(log2 e); Q' = bf16(fp32(Q) * c)  (sa_attn_small: Q' = fp32(Q) * c, not rounded);
  * S = Q' K^T accumulated in fp32;  P = bf16(exp2(S - m))  (sa_attn_small: P stays fp32);
  * l = the sum of the rounded P;  O = (P V) / l accumulated in fp32, rounded to bf16 once;
  * accumulate and the three-source sum of sa_attn_cross3 add bf16 values with one bf16 rounding per addition:
    (bf16(text) + bf16(img)) + bf16(vocal).
The kernels move the running max m lazily; here m is the row maximum.  tests/test_attn_ref_cpu.py shows that the
expectations of the exact inputs below hold under either choice and in either key-block order.
Everything is computed in float64 apart from the roundings listed above."""
import math
from typing import NamedTuple

import torch

D = 128
LOG2E = 1.4426950408889634
SENTINEL = 12288.0  # a bf16 value no test output reaches
INT_SCALE = math.log(2.0) / 8  # c = 1/8 to within an fp32 ulp: bf16(+-8 c) = +-1 exactly


def prescale(scale):
    """c as sa_attn_fwd forms it: the fp32 product of fp32(scale) and fp32(log2 e)  -> a python float"""
    return float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


def scaled_q(q, scale, round_q=True):
    """Q' in float64: fp32(Q) * c in fp32, rounded to bf16 unless round_q is False (the small-attention form)"""
    x = q.float() * torch.tensor(prescale(scale), dtype=torch.float32)
    return (x.bfloat16() if round_q else x).double()


def _heads(t, heads):
    return t.reshape(t.shape[0], heads, -1).transpose(0, 1)  # [heads, rows, d]


def softmax64(qd, kd, vd, heads, with_abs=False):
    """fp64 softmax attention (base 2) on the operands as given: qd already carries c.  -> [q rows, heads * d] fp64;
    with_abs: also the softmax-weighted mean of |v| per row and column (the scale of an fp32 accumulation's error)"""
    s = _heads(qd.double(), heads) @ _heads(kd.double(), heads).transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    back = lambda t: t.transpose(0, 1).reshape(qd.shape[0], -1)  # noqa: E731
    o = back(p @ _heads(vd.double(), heads))
    return (o, back(p @ _heads(vd.double().abs(), heads))) if with_abs else o


def attend(q, k, v, heads, scale, round_q=True, round_p=True):
    """the definition on one segment's rows -> fp64 [q rows, heads * d] before the final bf16 rounding"""
    if k.shape[0] == 0:
        return torch.zeros(q.shape[0], q.shape[1], dtype=torch.float64)
    s = _heads(scaled_q(q, scale, round_q), heads) @ _heads(k.double(), heads).transpose(-1, -2)
    s = s.float().double()  # the fp32 score accumulator
    p = torch.exp2(s - s.amax(-1, keepdim=True)).float()
    p = (p.bfloat16() if round_p else p).double()
    o = (p @ _heads(v.double(), heads)) / p.sum(-1, keepdim=True)
    return o.transpose(0, 1).reshape(q.shape[0], -1)


def bf16_add(a, b):
    """bf16 + bf16 with one rounding (accumulate; the cross-attention's sum of sources)"""
    return (a.float() + b.float()).bfloat16()


def attention(q, k, v, segs, heads, scale=None, out=None, accumulate=False, o_rows=None, round_q=True, round_p=True):
    """sa_attn_fwd_map's definition: bf16 rows of `out` (zeros [q rows] when None) named by the segment table, through
    o_rows when given; rows no segment names keep their value.  A segment with kv_len == 0 writes zeros (adds nothing
    when accumulating)."""
    d = q.shape[1] // heads
    scale = d ** -0.5 if scale is None else scale
    out = torch.zeros(q.shape[0], q.shape[1], dtype=torch.bfloat16) if out is None else out.clone()
    for q0, ql, k0, kl in segs:
        o = attend(q[q0:q0 + ql], k[k0:k0 + kl], v[k0:k0 + kl], heads, scale, round_q, round_p).bfloat16()
        rows = torch.arange(q0, q0 + ql) if o_rows is None else o_rows[q0:q0 + ql].long()
        out[rows] = bf16_add(out[rows], o) if accumulate else o
    return out


def attention_small(q, k, v, segs, heads, scale=None):
    """sa_attn_small's definition: Q' and P stay fp32"""
    return attention(q, k, v, segs, heads, scale, round_q=False, round_p=False)


def vocal_frame(tok_offset, i, tokens_per_frame):
    return (tok_offset + i) // tokens_per_frame


def cross3(q, kt, vt, t_len, ki, vi, i_len, kv, vv, nper, tokens_per_frame, n_frames, batch, q_len, heads, tok_offset=0,
           scale=None, frame_shift=0):
    """sa_attn_cross3's definition: (bf16(text) + bf16(img)) + bf16(vocal), the vocal keys those of the query's latent
    frame.  frame_shift: the mutant of tests/test_attn_ref_cpu.py (the frame index off by that much)"""
    scale = D ** -0.5 if scale is None else scale
    out = torch.zeros(batch * q_len, heads * D, dtype=torch.bfloat16)
    for b in range(batch):
        qq = q[b * q_len:(b + 1) * q_len]
        t = attend(qq, kt[b * t_len:(b + 1) * t_len], vt[b * t_len:(b + 1) * t_len], heads, scale).bfloat16()
        im = attend(qq, ki[b * i_len:(b + 1) * i_len], vi[b * i_len:(b + 1) * i_len], heads, scale).bfloat16()
        vo = torch.zeros_like(t)
        r0 = r1 = 0
        while r1 < q_len:
            r0, r1 = r1, min(q_len, r1 + tokens_per_frame - (tok_offset + r1) % tokens_per_frame)
            f = (vocal_frame(tok_offset, r0, tokens_per_frame) + frame_shift) % n_frames
            rows = slice((b * n_frames + f) * nper, (b * n_frames + f + 1) * nper)
            vo[r0:r1] = attend(qq[r0:r1], kv[rows], vv[rows], heads, scale).bfloat16()
        out[b * q_len:(b + 1) * q_len] = bf16_add(bf16_add(t, im), vo)
    return out


# ------------------------------------------------------------------------------------------------ segment tables

class Case(NamedTuple):
    """one launch: q / k / v rows (NaN in the rows no segment names), the table, the output row map (None: the query's
    own row), the expected rows of the output and which of them the launch owns, the scale, and for the integer-score
    and uniform families the fp64 reference's accumulation scale a_abs (else None)"""
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    segs: list
    o_rows: object
    want: torch.Tensor
    owned: torch.Tensor
    a_abs: object
    scale: float


LAYOUTS = ("contiguous", "gaps_descending", "shared_keys")


def kv_of(shapes, layout):
    """which segment's keys each segment reads: itself, but under shared_keys the first two segments with the same
    non-zero kv_len share the first one's key rows"""
    src = list(range(len(shapes)))
    if layout == "shared_keys":
        for j in range(len(shapes)):
            for i in range(j):
                if shapes[i][1] == shapes[j][1] > 0 and src[i] == i:
                    src[j] = i
                    return src
        raise ValueError("shared_keys needs two segments with the same kv_len")
    return src


def place(pieces, shapes, layout, kalign=1, seed=0):
    """Rows for the segments' pieces [(q_i, k_i, v_i, want_i, a_abs_i or None)] under one of LAYOUTS:
      contiguous       segments one after the other (key ranges on multiples of kalign);
      gaps_descending  the last segment first, 3 + i query rows and kalign + 5 key rows (rounded up to kalign) between;
      shared_keys      as gaps_descending, but two query segments read one key range, and the output goes through a
                       shuffled o_rows into an allocation 9 rows longer.
    Rows of q / k / v that no segment names are NaN; rows of the output no segment names are not owned."""
    n = len(shapes)
    src = kv_of(shapes, layout)
    order = list(range(n)) if layout == "contiguous" else list(range(n - 1, -1, -1))
    up = lambda x: -(-x // kalign) * kalign  # noqa: E731
    q0s, k0s, qn, kn = [0] * n, [0] * n, 0, 0
    for pos, i in enumerate(order):
        if layout != "contiguous":
            qn, kn = qn + 3 + pos, kn + kalign + 5
        q0s[i], qn = qn, qn + shapes[i][0]
        if src[i] == i:
            k0s[i] = kn = up(kn)
            kn += shapes[i][1]
    for i in range(n):
        k0s[i] = k0s[src[i]]
    C = pieces[0][0].shape[1]
    q = torch.full((qn, C), float("nan"), dtype=torch.bfloat16)
    k = torch.full((kn, C), float("nan"), dtype=torch.bfloat16)
    v = torch.full((kn, C), float("nan"), dtype=torch.bfloat16)
    exact = pieces[0][3].dtype == torch.bfloat16
    n_out = qn + (9 if layout == "shared_keys" else 0)
    o_rows = None
    if layout == "shared_keys":
        o_rows = torch.randperm(n_out, generator=torch.Generator().manual_seed(seed + 77))[:qn].int()
    want = torch.zeros(n_out, C, dtype=torch.bfloat16 if exact else torch.float64)
    a_abs = None if pieces[0][4] is None else torch.zeros(n_out, C, dtype=torch.float64)
    owned = torch.zeros(n_out, dtype=torch.bool)
    segs = []
    for i, (qi, ki, vi, wi, ai) in enumerate(pieces):
        ql, kl = shapes[i]
        q[q0s[i]:q0s[i] + ql] = qi
        k[k0s[i]:k0s[i] + kl], v[k0s[i]:k0s[i] + kl] = ki, vi
        rows = torch.arange(q0s[i], q0s[i] + ql) if o_rows is None else o_rows[q0s[i]:q0s[i] + ql].long()
        want[rows], owned[rows] = wi, True
        if a_abs is not None:
            a_abs[rows] = ai
        segs.append([q0s[i], ql, k0s[i], kl])
    return q, k, v, segs, o_rows, want, owned, a_abs


# ------------------------------------------------------------------------------------------------ exact inputs

def _v_rows(n, C, g):
    """V without a zero entry: odd integers of at most 3 bits times a power of two per key, so every fp32 sum of
    them -- weighted by powers of two -- is exact in any order"""
    odd = torch.randint(0, 4, (n, C), generator=g) * 2 + 1
    sign = torch.randint(0, 2, (n, C), generator=g) * 2 - 1
    return ((odd * sign).float() * torch.exp2(torch.randint(-3, 4, (n, 1), generator=g).float())).bfloat16()


SELECT_A = 16.0
SELECT_MIN_GAP = 64.0  # log2 units between the matching key's score and every other: > 24 (fp32) + 9 (the spread of
# |V|: 7 * 8 / 2^-3) + 13 (8192 keys), so every other key's contribution is below half an ulp of the match's, in O and l


def selection(shapes, heads, layout="contiguous", d=D, seed=3, kalign=1):
    """K rows +-1, Q[i] = SELECT_A * K[pi(i)] for a random pi with distinct key rows per segment: the matching score
    stands at least SELECT_MIN_GAP log2 units above every other (asserted), so under fp32 round-to-nearest every other
    key's term vanishes, whatever the key order and the rescale policy -- unlike the fp8 mode, bf16 P does not flush
    them to zero, so V holds no zero that could hide a misplaced key.  Expected: V[pi] exactly (zeros at kv_len 0)."""
    g = torch.Generator().manual_seed(seed)
    C, scale = heads * d, d ** -0.5
    src, pieces = kv_of(shapes, layout), []
    for i, (ql, kl) in enumerate(shapes):
        if src[i] != i:
            k, v = pieces[src[i]][1], pieces[src[i]][2]
        else:
            k = (torch.randint(0, 2, (kl, C), generator=g) * 2 - 1).float().bfloat16()
            v = _v_rows(kl, C, g)
        if kl == 0:
            q = (torch.randint(0, 2, (ql, C), generator=g) * 2 - 1).float().bfloat16()
            pieces.append((q, k, v, torch.zeros(ql, C, dtype=torch.bfloat16), None))
            continue
        pi = torch.randint(0, kl, (ql,), generator=g)
        q = (SELECT_A * k[pi].float()).bfloat16()
        s = _heads(scaled_q(q, scale), heads) @ _heads(k.double(), heads).transpose(-1, -2)  # [heads, ql, kl]
        top2 = s.topk(min(2, kl), -1).values
        assert (s.argmax(-1) == pi).all() and (kl == 1 or (top2[..., 0] - top2[..., 1]).min() >= SELECT_MIN_GAP)
        pieces.append((q, k, v, v[pi], None))
    return Case(*place(pieces, shapes, layout, kalign, seed), scale)


def uniform(shapes, heads, layout="contiguous", d=D, seed=11, kalign=1):
    """Q = 0: every key weighs the same.  Expected (fp64): the exact column mean of V, which is the exact result at a
    power-of-two kv_len (1 / l is exact) and within one bf16 ulp of it elsewhere."""
    g = torch.Generator().manual_seed(seed)
    C = heads * d
    src, pieces = kv_of(shapes, layout), []
    for i, (ql, kl) in enumerate(shapes):
        if src[i] != i:
            k, v = pieces[src[i]][1], pieces[src[i]][2]
        else:
            k, v = torch.randn(kl, C, generator=g).bfloat16(), _v_rows(kl, C, g)
        mean = v.double().mean(0) if kl else torch.zeros(C, dtype=torch.float64)
        amean = v.double().abs().mean(0) if kl else torch.zeros(C, dtype=torch.float64)
        pieces.append((torch.zeros(ql, C, dtype=torch.bfloat16), k, v, mean.expand(ql, C), amean.expand(ql, C)))
    return Case(*place(pieces, shapes, layout, kalign, seed), d ** -0.5)


# block maxima of the ladder's first query, one per 64-key block (its second query sees their negatives): a rise of
# 7 (below both rescale thresholds), 8 (P = 2: the self-attention moves; the cross-attention, whose max sits on the
# row maximum, sees 15 and moves), 9, and 156 (alpha = exp2(-163) = 0); the second query's first block stands far
# above every later one
LADDER = (-120, -113, -105, -96, 60)
# a rise of exactly 8 over the running max: the cross-attention stays (its test is > 8), the self-attention moves
LADDER8 = (-120, -112, -104, -97, 60)


def _ladder_keys(kl, C, levels, g):
    """one head's key rows [kl, C] in {-1, 0, 1} whose entries sum to levels[row // 64] exactly"""
    k = torch.zeros(kl, C)
    for r in range(kl):
        t = levels[min(r // 64, len(levels) - 1)]
        extra = int(torch.randint(0, (C - abs(t)) // 2 + 1, (1,), generator=g))
        cols = torch.randperm(C, generator=g)
        k[r, cols[:abs(t) + extra]] = 1.0 if t > 0 else -1.0
        k[r, cols[abs(t) + extra:abs(t) + 2 * extra]] = -1.0 if t > 0 else 1.0
    return k


def integer_scores(shapes, heads, nz=8, layout="contiguous", d=D, seed=5, kalign=1, ladder=None, round_q=True):
    """scale = INT_SCALE, Q in {0, +-8} with nz non-zeros per row and head, K in {-1, 0, 1}: every score is an exact
    integer and every P an exact power of two whatever the running max, so only the fp32 accumulations, the reciprocal
    and the final bf16 rounding are left.  ladder = {segment: levels}: that segment's keys have row sums levels[block]
    in every head, and its first two queries are all +8 / all -8 (scores +-levels[block] for every key of the block).
    Expected: the fp64 softmax attention and its a_abs."""
    g = torch.Generator().manual_seed(seed + nz)
    C = heads * d
    src, pieces = kv_of(shapes, layout), []
    ladder = ladder or {}
    for i, (ql, kl) in enumerate(shapes):
        if src[i] != i:
            k, v = pieces[src[i]][1], pieces[src[i]][2]
        else:
            if i in ladder:
                k = torch.cat([_ladder_keys(kl, d, ladder[i], g) for _ in range(heads)], 1).bfloat16()
            else:
                k = torch.randint(-1, 2, (kl, C), generator=g).float().bfloat16()
            v = _v_rows(kl, C, g)
        q = torch.zeros(ql, heads, d)
        idx = torch.rand(ql, heads, d, generator=g).argsort(-1)[..., :min(nz, d)]
        q.scatter_(-1, idx, (torch.randint(0, 2, idx.shape, generator=g) * 16 - 8).float())
        if i in ladder:
            q[0] = 8.0
            if ql > 1:
                q[1] = -8.0
        q = q.reshape(ql, C).bfloat16()
        if kl == 0:
            pieces.append((q, k, v, torch.zeros(ql, C, dtype=torch.float64), torch.zeros(ql, C, dtype=torch.float64)))
            continue
        qd = scaled_q(q, INT_SCALE, round_q)
        if round_q:
            assert torch.equal(qd, q.double() / 8)
        pieces.append((q, k, v, *softmax64(qd, k, v, heads, with_abs=True)))
    return Case(*place(pieces, shapes, layout, kalign, seed), INT_SCALE)


# ------------------------------------------------------------------------------------------------ assertions

def _where(i, j, segs, o_rows, width, d):
    """(segment, head, row in the segment, column in the head) of output element (i, j)"""
    for s, (q0, ql, _, _) in enumerate(segs or []):
        rows = list(range(q0, q0 + ql)) if o_rows is None else o_rows[q0:q0 + ql].tolist()
        if i in rows:
            return s, j // d, rows.index(i), j % d
    return None, j // d, i, j % d


def assert_equal_rows(out, want, segs=None, o_rows=None, d=D, what=""):
    """torch.equal; on failure the first wrong (segment, head, row, column)"""
    assert out.shape == want.shape and out.dtype == want.dtype, (what, out.shape, want.shape, out.dtype, want.dtype)
    if torch.equal(out, want):
        return
    bad = ~((out == want) | (out.isnan() & want.isnan()))
    i, j = (int(x) for x in bad.nonzero()[0])
    s, h, r, c = _where(i, j, segs, o_rows, out.shape[1], d)
    raise AssertionError(f"{what}: {int(bad.sum())} elements differ; first at segment {s} head {h} row {r} column {c} "
                         f"(output row {i}): got {out[i, j].item()} want {want[i, j].item()}")


def bf16_ulp(x):
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def assert_within_ulps(out, ref64, a_abs, n=1, segs=None, o_rows=None, d=D, what=""):
    """every element: |out - ref64| <= n * bf16_ulp(ref64) + 2^-20 * a_abs; -> the worst |out - ref64| / that bound's
    ulp part, i.e. the worst error in ulps after the cancellation allowance"""
    assert out.shape == ref64.shape, (what, out.shape, ref64.shape)
    err = (out.double() - ref64).abs()
    ulp = bf16_ulp(ref64)
    slack = 2.0 ** -20 * a_abs
    bad = ~(err <= n * ulp + slack)  # a NaN fails
    worst = float(((err - slack).clamp_min(0) / ulp).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    if bad.any():
        i, j = (int(x) for x in bad.nonzero()[0])
        s, h, r, c = _where(i, j, segs, o_rows, out.shape[1], d)
        raise AssertionError(f"{what}: {int(bad.sum())} elements past {n} ulp (worst {worst:.3f}); first at segment {s} "
                             f"head {h} row {r} column {c} (output row {i}): got {out[i, j].item()} "
                             f"ref {ref64[i, j].item()!r}")
    return worst


# ------------------------------------------------------------------------------------------------ the cases of the tests

# (q_len, kv_len) per segment: every q_len of {1, 33, 129, 257, 300} and kv_len of {1, 17, 63, 64, 65, 96, 257, 300},
# unequal segments (workgroups of the grid without rows), one segment without keys, two segments of one kv_len (the
# shared_keys layout)
SHAPE_SETS = {
    "a": [(33, 300), (300, 257), (5, 0), (129, 300), (1, 17)],
    "b": [(257, 63), (1, 1), (129, 0), (33, 64), (300, 63)],
    "c": [(300, 65), (33, 96), (1, 0), (257, 96), (129, 65)],
}
LADDERS = {0: LADDER, 3: LADDER8}  # on SHAPE_SETS["a"]: its two 300-key segments (5 key blocks)


def build(family, shapes, heads, layout="contiguous", d=D, kalign=1, round_q=True):
    """family: selection | uniform | int8 | int128 | ladder (nz = 128 with LADDERS; 300-key segments 0 and 3)"""
    if family == "selection":
        return selection(shapes, heads, layout, d, kalign=kalign)
    if family == "uniform":
        return uniform(shapes, heads, layout, d, kalign=kalign)
    nz = {"int8": 8, "int128": 128, "ladder": 128}[family]
    return integer_scores(shapes, heads, nz, layout, d, kalign=kalign, round_q=round_q,
                          ladder=LADDERS if family == "ladder" else None)


FAMILIES = ("selection", "uniform", "int8", "int128", "ladder")


def check(case, out, what="", n=1, d=D):
    """the family's assertion on the owned rows of `out` (bf16 [rows of case.want, C]): exact for selection, and for
    uniform segments with a power-of-two kv_len; else within n ulps.  -> the worst ulp figure (0.0 where exact)"""
    own = case.owned
    if case.want.dtype == torch.bfloat16:
        got = out.clone()
        got[~own] = case.want[~own]  # the rows no segment names are the caller's to check
        assert_equal_rows(got, case.want, case.segs, case.o_rows, d, what)
        return 0.0
    got = out.double()
    got[~own] = case.want[~own]
    return assert_within_ulps(got, case.want, case.a_abs, n, case.segs, case.o_rows, d, what)


def check_uniform_exact(case, out, what=""):
    """uniform: the rows of segments with a power-of-two kv_len (and of those without keys) equal bf16(mean) exactly"""
    for q0, ql, _, kl in case.segs:
        if kl & (kl - 1) == 0:
            rows = torch.arange(q0, q0 + ql) if case.o_rows is None else case.o_rows[q0:q0 + ql].long()
            assert_equal_rows(out[rows], case.want[rows].float().bfloat16(), what=f"{what} kv_len {kl}")


# --- sa_attn_cross3

class Cross3Case(NamedTuple):
    q: torch.Tensor
    kt: torch.Tensor
    vt: torch.Tensor
    ki: torch.Tensor
    vi: torch.Tensor
    kv: torch.Tensor
    vv: torch.Tensor
    want: torch.Tensor
    a_abs: object
    scale: float


X3_SELECT_A = 64.0


def _x3_rows(batch, q_len, t_len, i_len, nper, tpf, n_frames, tok_offset):
    """per source: the first key row of query row (b, i) and the keys it sees"""
    b = torch.arange(batch).repeat_interleave(q_len)
    f = (tok_offset + torch.arange(q_len).repeat(batch)) // tpf
    return [(b * t_len, t_len), (b * i_len, i_len), ((b * n_frames + f) * nper, nper)]


def cross3_selection(batch, q_len, heads, t_len, i_len, nper, tpf, n_frames, tok_offset, seed=21):
    """selection in the three sources at once: source s owns a third of every head's columns, its K rows are +-1 there
    and 0 elsewhere, and Q[i] = X3_SELECT_A * (Kt[pt(i)] + Ki[pi(i)] + Kv[pv(i)]) with the vocal key inside the query's
    frame.  Expected: the exact bf16 sum (Vt[pt] + Vi[pi]) + Vv[pv]."""
    g = torch.Generator().manual_seed(seed)
    C, scale = heads * D, D ** -0.5
    cols = [(torch.arange(C) % D >= lo) & (torch.arange(C) % D < hi) for lo, hi in ((0, 43), (43, 86), (86, 128))]
    rows = _x3_rows(batch, q_len, t_len, i_len, nper, tpf, n_frames, tok_offset)
    q = torch.zeros(batch * q_len, C)
    ks, vs, picks = [], [], []
    for (first, n), n_rows, m in zip(rows, (batch * t_len, batch * i_len, batch * n_frames * nper), cols):
        k = (torch.randint(0, 2, (n_rows, C), generator=g) * 2 - 1).float() * m
        pick = first + torch.randint(0, n, (batch * q_len,), generator=g)
        q += X3_SELECT_A * k[pick]
        ks.append(k.bfloat16()), vs.append(_v_rows(n_rows, C, g)), picks.append(pick)
    q = q.bfloat16()
    qd = scaled_q(q, scale)
    for k, (first, n), pick in zip(ks, rows, picks):  # the gap, per query row over the keys it sees
        for r in range(0, batch * q_len, 64):
            for f0 in first[r:r + 64].unique():
                sel = torch.arange(r, min(r + 64, batch * q_len))[first[r:r + 64] == f0]
                s = _heads(qd[sel], heads) @ _heads(k[f0:f0 + n].double(), heads).transpose(-1, -2)
                top2 = s.topk(min(2, n), -1).values
                assert (s.argmax(-1) + f0 == pick[sel]).all()
                assert n == 1 or (top2[..., 0] - top2[..., 1]).min() >= SELECT_MIN_GAP
    want = bf16_add(bf16_add(vs[0][picks[0]], vs[1][picks[1]]), vs[2][picks[2]])
    return Cross3Case(q, ks[0], vs[0], ks[1], vs[1], ks[2], vs[2], want, None, scale)


def cross3_integer(source, batch, q_len, heads, t_len, i_len, nper, tpf, n_frames, tok_offset, nz=8, seed=23):
    """integer scores in source `source` (0 text, 1 image, 2 vocal) alone: the other two sources' V are all zero, so
    they contribute exactly 0 and the bf16 sums are exact.  Expected: that source's fp64 softmax attention, a_abs."""
    g = torch.Generator().manual_seed(seed + source)
    C = heads * D
    rows = _x3_rows(batch, q_len, t_len, i_len, nper, tpf, n_frames, tok_offset)
    q = torch.zeros(batch * q_len, heads, D)
    idx = torch.rand(q.shape, generator=g).argsort(-1)[..., :nz]
    q.scatter_(-1, idx, (torch.randint(0, 2, idx.shape, generator=g) * 16 - 8).float())
    q = q.reshape(-1, C).bfloat16()
    ks, vs = [], []
    for s, n_rows in enumerate((batch * t_len, batch * i_len, batch * n_frames * nper)):
        ks.append(torch.randint(-1, 2, (n_rows, C), generator=g).float().bfloat16())
        vs.append(_v_rows(n_rows, C, g) if s == source else torch.zeros(n_rows, C, dtype=torch.bfloat16))
    first, n = rows[source]
    want = torch.zeros(batch * q_len, C, dtype=torch.float64)
    a_abs = torch.zeros_like(want)
    qd = scaled_q(q, INT_SCALE)
    for f0 in first.unique():
        sel = (first == f0).nonzero()[:, 0]
        want[sel], a_abs[sel] = softmax64(qd[sel], ks[source][f0:f0 + n], vs[source][f0:f0 + n], heads, with_abs=True)
    return Cross3Case(q, ks[0], vs[0], ks[1], vs[1], ks[2], vs[2], want, a_abs, INT_SCALE)


# t_len in {64, 512}, i_len 257, nper 17, 2 to 3 frames of 256 tokens, tok_offset 0 and 256; q_len ends inside a frame
X3_CASES = [dict(batch=2, q_len=300, heads=3, t_len=64, i_len=257, nper=17, tpf=256, n_frames=2, tok_offset=0),
            dict(batch=1, q_len=449, heads=1, t_len=512, i_len=257, nper=17, tpf=256, n_frames=3, tok_offset=256)]
