"""The fp8 attention mode without a GPU: its definition (stableavatar_amd/mxfp8_attn.py) -- the key permutation of the
V^T operand, exact selection and the exact uniform mean -- the C ABI's argument checks, and the CPU oracle with every
block's self-attention replaced by the definition against the plain oracle (the site choice)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fp8_attn_util import cos, rel, selection_input, small_case, uniform_input  # noqa: E402

from stableavatar_amd import _lib, mxfp8, mxfp8_attn  # noqa: E402


def test_key_permutation_is_the_accumulator_to_operand_map():
    kp = mxfp8_attn.KEY_OF_POS
    assert sorted(kp.tolist()) == list(range(128))
    # score accumulator (key tile t, lane group g, element e) holds key 16 t + 4 g + e and packs into operand VGPR t,
    # byte e of lane group g, i.e. reduction position 64 (t / 4) + 16 g + 4 (t % 4) + e
    seen = set()
    for t in range(8):
        for g in range(4):
            for e in range(4):
                pos = mxfp8_attn.acc_to_operand_pos(t, g, e)
                assert kp[pos] == 16 * t + 4 * g + e
                # the operand lane map: group g supplies bytes 16 g .. 16 g + 15 and 64 + 16 g .. 64 + 16 g + 15
                assert pos % 64 // 16 == g and pos // 64 == t // 4
                seen.add(pos)
    assert len(seen) == 128
    assert mxfp8_attn.P_SHIFT + mxfp8_attn.LAG <= 8  # 2^8 = 256 < 448: P never saturates


def test_vt_layout_round_trip():
    """quant_vt stores key KEY_OF_POS[p] of each block at position p, pads with zero bytes, and dequant_v inverts it"""
    g = torch.Generator().manual_seed(0)
    v = (torch.randint(-7, 8, (300, 256), generator=g).float() * 0.25).bfloat16()  # exact in e4m3 at any block scale
    vq, vs = mxfp8_attn.quant_vt(v)
    assert vq.shape == (256, 384) and vs.shape == (256, 12)
    assert torch.equal(mxfp8_attn.dequant_v(vq, vs, 300), v.float())
    vt = mxfp8.dequantize(vq, vs)
    for p in (0, 5, 17, 64, 127):
        assert torch.equal(vt[:, 128 + p], v[128 + int(mxfp8_attn.KEY_OF_POS[p])].float())
    pad = mxfp8_attn.KEY_OF_POS >= 300 - 256  # positions of the last block whose key is past kv_len
    assert (vq[:, 256:][:, pad] == 0).all()


@pytest.mark.parametrize("use_mean", [False, True])
def test_selection_is_exact(use_mean):
    q, k, v, segs, want = selection_input([(77, 300)], heads=2)
    km = mxfp8_attn.k_mean(k, segs) if use_mean else None
    out = mxfp8_attn.attention(q, k, v, segs, 2, kmean=km)
    assert torch.equal(out, want)


def test_uniform_is_the_mean_of_v():
    q, k, v, segs, mean = uniform_input(256, 5, heads=1)
    out = mxfp8_attn.attention(q, k, v, segs, 1, kmean=mxfp8_attn.k_mean(k, segs))
    vhat = mxfp8_attn.dequant_v(*mxfp8_attn.quant_vt(v), 256)
    assert torch.equal(vhat, v.float())  # the data quantises exactly, so the mean of V^ is the mean of V
    assert torch.equal(out, mean.float().bfloat16().expand(5, -1))


def test_empty_segment_gives_zeros():
    q, k, v, _, _ = selection_input([(3, 5)], heads=1)
    out = mxfp8_attn.attention(q, k, v, [[0, 3, 0, 0]], 1)
    assert (out == 0).all()


def test_abi_rejects_bad_arguments_without_gpu_work():
    """every check precedes the first HIP call: rc 1 with no device"""
    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    L = _lib.lib()
    one = 256  # a non-null, 16-byte aligned host address: rejected before it is dereferenced

    def fwd(q=one, qs=one, k=one, ks=one, vt=one, vts=one, Rv=128, o=one, os_=128, segs=one, vcol0=one, hd=128):
        return L.sa_attn_fwd_mxfp8(q, qs, k, ks, vt, vts, Rv, o, os_, segs, vcol0, 1, 16, 1, hd, None, None)

    for name in ("q", "qs", "k", "ks", "vt", "vts", "o", "segs", "vcol0"):
        assert fwd(**{name: None}) == 1, name
    assert fwd(hd=64) == 1 and fwd(hd=256) == 1
    assert fwd(Rv=192) == 1 and fwd(Rv=0) == 1          # Rv % 128
    assert fwd(os_=132) == 1 and fwd(os_=64) == 1       # vector stores; narrower than the heads
    assert fwd(q=264) == 1 and fwd(vt=264) == 1         # 16-byte operand loads
    assert fwd(ks=258) == 1                             # dword scale loads

    def pack(q=one, k=one, v=one, segs=one, vcol0=one, outs=(one,) * 6, st=(128, 128, 128), Rv=128, hd=128, km=None):
        return L.sa_attn_pack_mxfp8(q, st[0], k, st[1], v, st[2], segs, vcol0, 1, 16, 16, 1, hd, 0.1, km, *outs, Rv,
                                    None)

    for name in ("q", "k", "v", "segs", "vcol0"):
        assert pack(**{name: None}) == 1, name
    for i in range(6):
        assert pack(outs=tuple(None if j == i else one for j in range(6))) == 1
    assert pack(hd=64) == 1
    assert pack(Rv=100) == 1
    for i in range(3):                                  # a stride that breaks the 16-byte loads, one too narrow
        assert pack(st=tuple(132 if j == i else 128 for j in range(3))) == 1
        assert pack(st=tuple(64 if j == i else 128 for j in range(3))) == 1
    assert pack(q=264) == 1 and pack(v=264) == 1

    assert L.sa_attn_kmean(None, 128, one, 1, 1, 128, one, one, None) == 1
    assert L.sa_attn_kmean(one, 128, None, 1, 1, 128, one, one, None) == 1
    assert L.sa_attn_kmean(one, 128, one, 1, 1, 128, None, one, None) == 1
    assert L.sa_attn_kmean(one, 128, one, 1, 1, 128, one, None, None) == 1
    assert L.sa_attn_kmean(one, 128, one, 1, 1, 64, one, one, None) == 1
    assert L.sa_attn_kmean(one, 132, one, 1, 1, 128, one, one, None) == 1  # 16-byte row loads


@pytest.mark.parametrize("case,peak", [("full", False), ("short", False), ("wide", False), ("full", True)])
def test_oracle_self_attention_in_mxfp8_stays_inside_the_bf16_bar(case, peak):
    """the site choice: the definition in place of every block's self-attention moves the oracle's output by less than
    the project's bar for a quantised mode; `peak`: every norm_q weight x 4 (scores four times as sharp)"""
    _, _, plain = small_case(case, False, False, peak)
    _, _, emu = small_case(case, True, False, peak)
    r, c = rel(emu, plain), cos(emu, plain)
    print(f"DIT_SMALL {case}{' peaky' if peak else ''}: self-attention in MXFP8 vs plain oracle rel-L2 {r:.3e} "
          f"cosine {c:.6f}")
    assert r > 0  # the patch took effect
    assert r < 2e-2 and c > 0.9995, (r, c)
