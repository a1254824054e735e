"""The fp8 self-O mode without a GPU: the site choice on the CPU oracle (the self-attention output projection emulated
in MXFP8 against the plain oracle, alone and on top of the other three emulations; why cross_attn.o stays bf16; the
30-layer case), the argument checks of the two flash entry points that write the projection's operand, and the mode's
validation and CLI flag."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fp8_o_util import CROSS_O_LINEAR, cos, full_dims_case, rel, small_case  # noqa: E402

from stableavatar_amd import _lib  # noqa: E402
from stableavatar_amd.transformer import WanTransformer3DFantasyModel  # noqa: E402

MODE = WanTransformer3DFantasyModel.enable_fp8_o  # the mode whose numerics the oracle patch defines

BAR = dict(rel=2e-2, cos=0.9995)  # the project's bar (tests/test_gpu_fp8_attn.py BAR, tests/test_gpu_mxfp8.py)
NONE = (False, False, False, False)  # (o, q/k/v, attention, FFN)
ALL = (True, True, True, True)


@pytest.mark.parametrize("case", ["full", "short", "wide"])
def test_oracle_self_o_in_mxfp8_stays_inside_the_bar(case):
    """the site choice: quantising the operands of self_attn.o moves the oracle's output by far less than the
    project's bar (measured 4.12e-3 / 4.84e-3 rel-L2 on full / short)"""
    assert "mxfp8.quantize" in MODE.__doc__  # the definition the patch restates
    _, _, plain = small_case(case, *NONE)
    _, _, emu = small_case(case, True)
    r, c = rel(emu, plain), cos(emu, plain)
    print(f"DIT_SMALL {case}: self-O in MXFP8 vs plain oracle rel-L2 {r:.3e} cosine {c:.6f}")
    assert r > 0  # the patch took effect
    assert r < BAR["rel"] and c > BAR["cos"], (r, c)


@pytest.mark.parametrize("case", ["full", "short", "wide"])
def test_oracle_all_four_in_mxfp8_stay_inside_the_bar(case):
    """self-O on top of q/k/v + attention + FFN (measured 8.60e-3 / 9.29e-3 on full / short), and the four patches
    compose: the result differs from any three of them"""
    _, _, plain = small_case(case, *NONE)
    _, _, all4 = small_case(case, *ALL)
    r, c = rel(all4, plain), cos(all4, plain)
    print(f"DIT_SMALL {case}: self-O + q/k/v + attention + FFN in MXFP8 vs plain oracle rel-L2 {r:.3e} cosine {c:.6f}")
    for i in range(4):
        three = tuple(j != i for j in range(4))
        assert rel(all4, small_case(case, *three)[2]) > 0, three
    assert r < BAR["rel"] and c > BAR["cos"], (r, c)


@pytest.mark.parametrize("case", ["full", "short"])
def test_oracle_cross_o_in_mxfp8_is_outside_the_bar(case):
    """why cross_attn.o stays bf16: that one site alone moves the output past the bar's rel-L2 (measured 2.59e-2 /
    2.63e-2 on full / short)"""
    _, _, plain = small_case(case, *NONE)
    _, _, emu = small_case(case, True, site=CROSS_O_LINEAR)
    r, c = rel(emu, plain), cos(emu, plain)
    print(f"DIT_SMALL {case}: cross_attn.o in MXFP8 vs plain oracle rel-L2 {r:.3e} cosine {c:.6f}")
    assert r > BAR["rel"], r


def test_oracle_30_layers_all_four_stay_inside_the_bar():
    """30 layers at the 1.3B widths on a tiny grid, all four emulations against the plain oracle (measured 1.625e-2 /
    0.999868)"""
    _, _, _, plain = full_dims_case(NONE)
    _, _, _, all4 = full_dims_case(ALL)
    r, c = rel(all4, plain), cos(all4, plain)
    print(f"CONFIG_1_3B, 30 layers: all four emulations vs plain oracle rel-L2 {r:.3e} cosine {c:.6f}")
    assert r < BAR["rel"] and c > BAR["cos"], (r, c)


# ------------------------------------------------------------------------------------------------ the C ABI

ONE = 256  # a non-null, 16-byte aligned host address: rejected before it is dereferenced
NAMES = {"sa_attn_fwd_mxfp8_o8", "sa_attn_fwd_mxfp8_split_o8"}


def _lib_or_skip():
    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    return _lib.lib()


def test_new_entry_points_are_declared_bound_and_exported():
    assert NAMES <= set(_lib.header_symbols()) and NAMES <= set(_lib.SIGNATURES)
    assert _lib.SIGNATURES["sa_attn_fwd_mxfp8_o8"] == "pppppplplplppiiiipp"
    assert _lib.SIGNATURES["sa_attn_fwd_mxfp8_split_o8"] == "pppppplplplppiiiipiplp"
    L = _lib_or_skip()
    for n in NAMES:
        assert getattr(L, n) is not None


def _call(L, split, q=ONE, qs=ONE, k=ONE, ks=ONE, vt=ONE, vts=ONE, Rv=128, oq=ONE, ldo=None, osc=ONE, ldos=None,
          segs=ONE, vcol0=ONE, nseg=1, mq=16, heads=2, hd=128, tiles=1, work=ONE, wb=1 << 30):
    ldo = heads * 128 if ldo is None else ldo
    ldos = heads * 4 if ldos is None else ldos
    head = (q, qs, k, ks, vt, vts, Rv, oq, ldo, osc, ldos, segs, vcol0, nseg, mq, heads, hd, None)
    if split:
        return L.sa_attn_fwd_mxfp8_split_o8(*head, tiles, work, wb, None)
    return L.sa_attn_fwd_mxfp8_o8(*head, None)


@pytest.mark.parametrize("split", [False, True], ids=["o8", "split_o8"])
def test_o8_entry_points_reject_bad_arguments_without_gpu_work(split):
    L = _lib_or_skip()
    bad = lambda **kw: _call(L, split, **kw)  # noqa: E731
    # the parent's checks
    for n in ("q", "qs", "k", "ks", "vt", "vts", "segs", "vcol0"):
        assert bad(**{n: None}) == 1, n
    assert bad(nseg=0) == 1 and bad(heads=0) == 1 and bad(mq=0) == 1
    assert bad(hd=64) == 1                               # head_dim 128 only
    assert bad(Rv=0) == 1 and bad(Rv=192) == 1           # Rv a positive multiple of 128
    for n in ("q", "k", "vt"):
        assert bad(**{n: ONE + 8}) == 1, n               # 16-byte operand loads
    for n in ("qs", "ks", "vts"):
        assert bad(**{n: ONE + 2}) == 1, n               # dword scale loads
    # the output operand
    assert bad(oq=None) == 1 and bad(osc=None) == 1
    assert bad(ldo=128) == 1 and bad(ldo=255) == 1       # a row shorter than heads * 128
    assert bad(ldos=4) == 1 and bad(ldos=7) == 1         # a scale row shorter than heads * 4
    assert bad(ldo=258) == 1 and bad(ldos=10) == 1       # ldo % 4, ldos % 4
    assert bad(oq=ONE + 2) == 1 and bad(osc=ONE + 1) == 1  # dword stores
    if split:
        assert bad(work=None) == 1 and bad(work=ONE + 8) == 1
        assert bad(tiles=0) == 1 and bad(tiles=3) == 1   # 1 segment x 2 heads x 1 query block = 2 tiles
        assert bad(wb=2 * 256 * 130 * 4 - 1) == 1        # one split tile's partials do not fit


# ------------------------------------------------------------------------------------------------ the mode

def _model(**kw):
    cfg = dict(dim=256, ffn_dim=256, num_heads=2, num_layers=1, text_dim=64, freq_dim=64, text_len=8)
    cfg.update(kw)
    return WanTransformer3DFantasyModel(**cfg)


def test_enable_fp8_o_validates_and_drops_packed_state():
    m = _model()
    assert m._fp8_o is False and m._fp8_o_fused in (True, False)
    m._packed, m._ws = object(), {"k": 1}
    m.enable_fp8_o(False)  # no change: nothing dropped
    assert m._packed is not None and m._ws
    m.enable_fp8_o()
    assert m._fp8_o and m._packed is None and m._ws == {}
    assert not m._fp8_ffn and not m._fp8_attn and not m._fp8_qkv  # independent of the other three modes
    m._packed, m._ws = object(), {"k": 1}
    m.enable_fp8_o(False)
    assert not m._fp8_o and m._packed is None and m._ws == {}
    for ffn in (False, True):
        for attn in (False, True):
            for qkv in (False, True):
                m.enable_fp8_ffn(ffn), m.enable_fp8_attention(attn), m.enable_fp8_qkv(qkv), m.enable_fp8_o()
                assert (m._fp8_ffn, m._fp8_attn, m._fp8_qkv, m._fp8_o) == (ffn, attn, qkv, True)


def test_enable_fp8_o_rejects_widths_off_the_k_tile():
    m = _model()
    m.dim = 1600  # no constructible model has such a width at head_dim 128: the check is the mode's own
    with pytest.raises(ValueError, match="128"):
        m.enable_fp8_o()
    assert not m._fp8_o
    m.enable_fp8_o(False)  # turning it off is always accepted


def test_cli_flag_parses_and_defaults_to_off():
    from stableavatar_amd.inference import parse_args
    base = ["--pretrained_model_name_or_path", "ckpt"]
    assert parse_args(base).fp8_o is False
    a = parse_args(base + ["--fp8_o"])
    assert a.fp8_o is True and a.fp8_ffn is False and a.fp8_attn is False and a.fp8_qkv is False
    a = parse_args(base + ["--fp8_o", "--fp8_qkv", "--fp8_attn", "--fp8_ffn"])
    assert a.fp8_o and a.fp8_qkv and a.fp8_attn and a.fp8_ffn
