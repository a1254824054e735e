"""The fp8 q/k/v mode without a GPU: the site choice on the CPU oracle (the q, k and v Linears of the self-attention
emulated in MXFP8 against the plain oracle, alone and with the FFN), the argument checks of the three entry points
that write the fp8 attention's operands where their values are made, and the mode's validation and CLI flag."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fp8_qkv_util import cos, rel, small_case  # noqa: E402

from stableavatar_amd import _lib  # noqa: E402
from stableavatar_amd.transformer import WanTransformer3DFantasyModel  # noqa: E402

MODE = WanTransformer3DFantasyModel.enable_fp8_qkv  # the mode whose numerics the oracle patch below defines

BAR = dict(rel=2e-2, cos=0.9995)  # the project's bar (tests/test_gpu_fp8_attn.py BAR, tests/test_gpu_mxfp8.py)


@pytest.mark.parametrize("case", ["full", "short", "wide"])
def test_oracle_qkv_in_mxfp8_stays_inside_the_bar(case):
    """the site choice: quantising the operands of self-attention q/k/v moves the oracle's output by far less than the
    project's bar (measured 3.23e-3 / 3.79e-3 / 3.07e-3 rel-L2 on full / short / wide)"""
    assert "mxfp8.quantize" in MODE.__doc__  # the definition the patch restates
    _, _, plain = small_case(case, False)
    _, _, emu = small_case(case, True)
    r, c = rel(emu, plain), cos(emu, plain)
    print(f"DIT_SMALL {case}: q/k/v in MXFP8 vs plain oracle rel-L2 {r:.3e} cosine {c:.6f}")
    assert r > 0  # the patch took effect
    assert r < BAR["rel"] and c > BAR["cos"], (r, c)


@pytest.mark.parametrize("case", ["full", "short", "wide"])
def test_oracle_qkv_and_ffn_in_mxfp8_stay_inside_the_bar(case):
    """both GEMM modes together (measured 7.5e-3 .. 7.7e-3 / 0.99997), and the two patches compose: the result differs
    from either one alone"""
    _, _, plain = small_case(case, False)
    _, _, qkv = small_case(case, True)
    _, _, ffn = small_case(case, False, False, True)
    _, _, both = small_case(case, True, False, True)
    r, c = rel(both, plain), cos(both, plain)
    print(f"DIT_SMALL {case}: q/k/v + FFN in MXFP8 vs plain oracle rel-L2 {r:.3e} cosine {c:.6f}")
    assert rel(both, qkv) > 0 and rel(both, ffn) > 0
    assert r < BAR["rel"] and c > BAR["cos"], (r, c)


def test_oracle_patches_compose_with_fp8_attention():
    """all three emulations in one forward differ from any two of them"""
    _, _, all3 = small_case("full", True, True, True)
    for two in ((False, True, True), (True, False, True), (True, True, False)):
        assert rel(all3, small_case("full", *two)[2]) > 0, two


# ------------------------------------------------------------------------------------------------ the C ABI

ONE = 256  # a non-null, 16-byte aligned host address: rejected before it is dereferenced


def _lib_or_skip():
    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    return _lib.lib()


def test_new_entry_points_are_declared_bound_and_exported():
    names = {"sa_gemm_mxfp8_vt", "sa_qk_rmsnorm_rope_mxfp8", "sa_attn_pack_k_mxfp8"}
    assert names <= set(_lib.header_symbols()) and names <= set(_lib.SIGNATURES)
    L = _lib_or_skip()
    for n in names:
        assert getattr(L, n) is not None


def test_gemm_vt_rejects_bad_arguments_without_gpu_work():
    L = _lib_or_skip()

    def vt(A=ONE, As=ONE, W=ONE, Ws=ONE, out=ONE, outs=ONE, Rv=256, N=128, K=128, rps=100, nseg=2, M=None):
        M = nseg * rps if M is None else M
        return L.sa_gemm_mxfp8_vt(A, K, As, max(K // 32, 4), W, K, Ws, max(K // 32, 4), None, out, outs, Rv, M, N, K,
                                  rps, nseg, None)

    for kw in (dict(A=None), dict(As=None), dict(W=None), dict(Ws=None), dict(out=None), dict(outs=None)):
        assert vt(**kw) == 1, kw
    assert vt(K=192) == 1                 # K % 128
    assert vt(N=192) == 1                 # N % 128
    assert vt(Rv=128) == 1                # two segments of ceil128(100) = 128 columns need 256
    assert vt(Rv=320) == 1                # Rv % 128
    assert vt(rps=129, Rv=256) == 1       # ceil128(129) = 256 per segment
    assert vt(rps=0, M=128) == 1 and vt(rps=-4, M=128) == 1
    assert vt(nseg=0, M=128) == 1
    assert vt(M=199) == 1                 # M != nseg * rows_per_seg
    assert vt(out=ONE + 8) == 1           # 16-byte stores
    assert vt(A=ONE + 8) == 1


def test_qk_rmsnorm_rope_mxfp8_rejects_bad_arguments_without_gpu_work():
    L = _lib_or_skip()

    def rr(x=ONE, wq=ONE, wk=ONE, qo=ONE, qs=ONE, C=256, hd=128, k_col=256, ldq=None, ldqs=None, rope=None, rpb=0):
        return L.sa_qk_rmsnorm_rope_mxfp8(x, 3 * C, 0, k_col, wq, wk, 8, C, hd, 1e-6, rope, rpb, 0, 1, 1, 1, 0, 0, qo,
                                          C if ldq is None else ldq, qs, C // 32 if ldqs is None else ldqs, 0.1, None)

    for kw in (dict(x=None), dict(wq=None), dict(wk=None), dict(qo=None), dict(qs=None)):
        assert rr(**kw) == 1, kw
    assert rr(hd=64) == 1 and rr(hd=256) == 1     # head_dim 128 only
    assert rr(C=192, k_col=192) == 1              # C % 128
    assert rr(C=5248) == 1                        # past the kernels' 5120 columns
    assert rr(ldq=128) == 1 and rr(ldqs=4) == 1   # the outputs' rows are too short
    assert rr(rope=ONE, rpb=0) == 1               # a RoPE table needs rows_per_batch
    assert rr(qo=ONE + 4) == 1                    # 8-byte stores


def test_attn_pack_k_rejects_bad_arguments_without_gpu_work():
    L = _lib_or_skip()

    def pk(k=ONE, ks=256, segs=ONE, nseg=1, mkv=8, heads=2, km=None, ko=ONE, kso=ONE):
        return L.sa_attn_pack_k_mxfp8(k, ks, segs, nseg, mkv, heads, km, ko, kso, None)

    for kw in (dict(k=None), dict(segs=None), dict(ko=None), dict(kso=None)):
        assert pk(**kw) == 1, kw
    assert pk(nseg=0) == 1 and pk(heads=0) == 1 and pk(mkv=-1) == 1
    assert pk(ks=128) == 1 and pk(ks=260) == 1    # a row shorter than heads * 128; not a multiple of 8
    assert pk(k=ONE + 8) == 1 and pk(km=ONE + 2) == 1
    # the full pack keeps its own checks
    assert L.sa_attn_pack_mxfp8(ONE, 256, ONE, 256, ONE, 256, ONE, ONE, 1, 8, 8, 2, 128, 0.1, None, None, ONE, ONE, ONE,
                                ONE, ONE, 128, None) == 1


# ------------------------------------------------------------------------------------------------ the mode

def _model(**kw):
    cfg = dict(dim=256, ffn_dim=256, num_heads=2, num_layers=1, text_dim=64, freq_dim=64, text_len=8)
    cfg.update(kw)
    return WanTransformer3DFantasyModel(**cfg)


def test_enable_fp8_qkv_validates_and_drops_packed_state():
    m = _model()
    assert m._fp8_qkv is False and m._fp8_qkv_fused in (True, False)
    m._packed, m._ws = object(), {"k": 1}
    m.enable_fp8_qkv(False)  # no change: nothing dropped
    assert m._packed is not None and m._ws
    m.enable_fp8_qkv()
    assert m._fp8_qkv and m._packed is None and m._ws == {}
    assert not m._fp8_ffn and not m._fp8_attn  # independent of the other two modes
    m._packed, m._ws = object(), {"k": 1}
    m.enable_fp8_qkv(False)
    assert not m._fp8_qkv and m._packed is None and m._ws == {}
    for ffn in (False, True):
        for attn in (False, True):
            m.enable_fp8_ffn(ffn), m.enable_fp8_attention(attn), m.enable_fp8_qkv()
            assert (m._fp8_ffn, m._fp8_attn, m._fp8_qkv) == (ffn, attn, True)


def test_enable_fp8_qkv_rejects_widths_off_the_k_tile():
    m = _model()
    m.dim = 1600  # no constructible model has such a width at head_dim 128: the check is the mode's own
    with pytest.raises(ValueError, match="128"):
        m.enable_fp8_qkv()
    assert not m._fp8_qkv
    m.enable_fp8_qkv(False)  # turning it off is always accepted


def test_cli_flag_parses_and_defaults_to_off():
    from stableavatar_amd.inference import parse_args
    base = ["--pretrained_model_name_or_path", "ckpt"]
    assert parse_args(base).fp8_qkv is False
    a = parse_args(base + ["--fp8_qkv"])
    assert a.fp8_qkv is True and a.fp8_ffn is False and a.fp8_attn is False
    a = parse_args(base + ["--fp8_qkv", "--fp8_attn", "--fp8_ffn"])
    assert a.fp8_qkv and a.fp8_attn and a.fp8_ffn
