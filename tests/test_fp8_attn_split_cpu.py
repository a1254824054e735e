"""The key split of the fp8 attention mode without a GPU: the split definition (stableavatar_amd/mxfp8_attn.py,
attend_split) exact on the selection and uniform inputs -- and not exact without its drop rule --, no less accurate than
the unsplit definition on random data, bit-identical wherever nothing is split, and the plumbing of the new entry."""
import inspect
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fp8_attn_split_util import RANDOM_SHAPES, SELECT_SHAPES, VARIANTS, n_tiles, random_case  # noqa: E402
from fp8_attn_util import selection_input, uniform_input  # noqa: E402

from stableavatar_amd import _lib, mxfp8_attn, ops  # noqa: E402

D = 128


def _merge_without_the_drop_rule(qd, kd, vd):
    """attend_split's merge as plain log-sum-exp: w_h = exp2(m_h - M) whatever the gap"""
    kper = mxfp8_attn.split_point(kd.shape[-2])
    if kper >= kd.shape[-2]:
        return mxfp8_attn.attend(qd, kd, vd)
    m0, O0, l0 = mxfp8_attn.attend_half(qd, kd[..., :kper, :], vd[..., :kper, :])
    m1, O1, l1 = mxfp8_attn.attend_half(qd, kd[..., kper:, :], vd[..., kper:, :])
    M = torch.maximum(m0, m1)
    w0, w1 = torch.exp2(m0 - M)[..., None], torch.exp2(m1 - M)[..., None]
    return (w0 * O0 + w1 * O1) / (w0 * l0[..., None] + w1 * l1[..., None])


@pytest.mark.parametrize("use_mean", [False, True])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("shapes", SELECT_SHAPES)
def test_split_selection_is_exact_and_needs_the_drop_rule(shapes, heads, use_mean, monkeypatch):
    q, k, v, segs, want = selection_input(shapes, heads)
    km = mxfp8_attn.k_mean(k, segs) if use_mean else None
    nt = n_tiles(segs, heads)
    assert torch.equal(mxfp8_attn.attention(q, k, v, segs, heads, kmean=km, split_tiles=nt), want)
    # without the rule the other half's 2^-95-weighted O shows wherever the selected V is 0
    monkeypatch.setattr(mxfp8_attn, "attend_split", _merge_without_the_drop_rule)
    loose = mxfp8_attn.attention(q, k, v, segs, heads, kmean=km, split_tiles=nt)
    assert not torch.equal(loose, want)
    bad = loose != want
    assert (want[bad] == 0).all() and (loose[bad].float().abs() < 2.0 ** -60).all()


@pytest.mark.parametrize("kv_len", [256, 300, 512])
def test_split_uniform_is_the_mean_of_v(kv_len):
    q, k, v, segs, mean = uniform_input(kv_len, 40, heads=3)
    out = mxfp8_attn.attention(q, k, v, segs, 3, kmean=mxfp8_attn.k_mean(k, segs), split_tiles=n_tiles(segs, 3))
    assert torch.equal(out, mean.float().bfloat16().expand(40, -1))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_split_random_is_no_less_accurate_than_the_unsplit_definition(shape, variant):
    """Every tile split against the unsplit definition, both measured against R (fp64 attention on the dequantised
    operands) and X (fp64 attention on the inputs); the split may cost at most 5 %.  Measured over the 12 cases:
    against R 0.795-0.999, against X 0.991-1.004 (the ratios are printed)."""
    c = random_case(shape, variant)
    rR, rX = c["split_R"] / c["whole_R"], c["split_X"] / c["whole_X"]
    print(f"{variant} {shape}: split / unsplit definition vs R {c['split_R']:.3e} / {c['whole_R']:.3e} = {rR:.3f}, "
          f"vs X {c['split_X']:.3e} / {c['whole_X']:.3e} = {rX:.3f}")
    assert rR <= 1.05
    assert rX <= 1.05


def _mixed():
    """segments (257, 300), (77, 129), (40, 128), (33, 1): heads 3, nqb 2 -> 24 tiles, four of them without a query"""
    q, k, v, segs, _ = selection_input([(257, 300), (77, 129), (40, 128), (33, 1)], 3, seed=9)
    g = torch.Generator().manual_seed(4)
    q = (q.float() * 0.02 + torch.randn(q.shape, generator=g)).bfloat16()  # soft rows: every key weighs in
    return q, k, v, segs


def test_split_tiles_zero_is_todays_function():
    q, k, v, segs = _mixed()
    km = mxfp8_attn.k_mean(k, segs)
    whole = mxfp8_attn.attention(q, k, v, segs, 3, kmean=km)
    assert torch.equal(mxfp8_attn.attention(q, k, v, segs, 3, kmean=km, split_tiles=0), whole)
    assert torch.equal(mxfp8_attn.attention(q, k, v, segs, 3, kmean=km, split_tiles=0, max_q_len=257), whole)
    assert torch.isfinite(whole.float()).all()


@pytest.mark.parametrize("split_tiles", [1, 7, 14, 24])
def test_rows_outside_the_split_tiles_and_short_segments_keep_their_bits(split_tiles):
    q, k, v, segs = _mixed()
    heads, nqb = 3, 2
    km = mxfp8_attn.k_mean(k, segs)
    whole = mxfp8_attn.attention(q, k, v, segs, heads, kmean=km)
    out = mxfp8_attn.attention(q, k, v, segs, heads, kmean=km, split_tiles=split_tiles)
    nt = n_tiles(segs, heads)
    assert nt == 24
    changed = 0
    for i, (q0, ql, _, kl) in enumerate(segs):
        for h in range(heads):
            for qb in range(nqb):
                rows = slice(q0 + qb * 256, q0 + min(ql, (qb + 1) * 256))
                a, b = out[rows, h * D:(h + 1) * D], whole[rows, h * D:(h + 1) * D]
                is_split = (i * heads + h) * nqb + qb >= nt - split_tiles
                if not is_split or kl <= 128:
                    assert torch.equal(a, b), (i, h, qb)
                else:
                    changed += int(not torch.equal(a, b))
    # the split is a different rounding of P: tiles with keys in both halves do not all come out bit-identical
    # (the last 12 tiles belong to the two short segments)
    assert changed > 0 if split_tiles > 12 else changed == 0


def test_split_tiles_out_of_range_is_an_error():
    q, k, v, segs = _mixed()
    with pytest.raises(ValueError):
        mxfp8_attn.attention(q, k, v, segs, 3, split_tiles=25)


def test_plumbing_of_the_split_entry():
    header = _lib.HEADER.read_text()
    m = re.search(r"^\s*int\s+sa_attn_fwd_mxfp8_split\s*\(([^;]*)\)\s*;", header, flags=re.M)
    assert m, "include/stableavatar_hip.h does not declare sa_attn_fwd_mxfp8_split"
    assert "sa_attn_fwd_mxfp8_split" in _lib.header_symbols()
    sig = _lib.SIGNATURES["sa_attn_fwd_mxfp8_split"]
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(sig) == 20
    for a, c in zip(args, sig):  # pointers, int64_t and int line up
        assert c == ("p" if "*" in a else "l" if a.startswith("int64_t") else "i"), (a, c)
    for fn in (ops.attention_mxfp8, ops.attn_fwd_mxfp8):
        p = inspect.signature(fn).parameters
        assert "split_tiles" in p and p["split_tiles"].default == 0
    p = inspect.signature(mxfp8_attn.attention).parameters
    assert p["split_tiles"].default == 0 and p["max_q_len"].default is None


def test_split_abi_rejects_bad_arguments_without_gpu_work():
    """every check precedes the first HIP call: rc 1 with no device"""
    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    L = _lib.lib()
    one = 256  # a non-null, 16-byte aligned host address: rejected before it is dereferenced
    need = 2 * 256 * 130 * 4  # bytes of work per split tile

    def fwd(q=one, qs=one, k=one, ks=one, vt=one, vts=one, Rv=128, o=one, os_=128, segs=one, vcol0=one, hd=128,
            split=1, work=one, wb=None, mq=16):
        return L.sa_attn_fwd_mxfp8_split(q, qs, k, ks, vt, vts, Rv, o, os_, segs, vcol0, 1, mq, 1, hd, None, split,
                                         work, split * need if wb is None else wb, None)

    for name in ("q", "qs", "k", "ks", "vt", "vts", "o", "segs", "vcol0", "work"):
        assert fwd(**{name: None}) == 1, name
    assert fwd(hd=64) == 1 and fwd(hd=256) == 1
    assert fwd(Rv=192) == 1 and fwd(Rv=0) == 1
    assert fwd(os_=132) == 1 and fwd(os_=64) == 1
    assert fwd(q=264) == 1 and fwd(k=264) == 1 and fwd(vt=264) == 1 and fwd(o=264) == 1
    assert fwd(ks=258) == 1
    assert fwd(work=264) == 1                            # 16-byte partial stores
    assert fwd(split=0) == 1 and fwd(split=-1) == 1
    assert fwd(split=2) == 1                             # one tile in all
    assert fwd(split=3, mq=513, wb=3 * need - 4) == 1    # three tiles; work four bytes short
    assert fwd(wb=need - 1) == 1 and fwd(wb=0) == 1
