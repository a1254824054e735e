"""Shared by the fp8 self-O tests: the CPU oracle with the output projection of every DiT block's self-attention
emulated in MXFP8 (the definition of what enable_fp8_o() computes, up to bf16 noise).  The patch goes through
oracle.dit.linear and wraps whatever is installed there, as fp8_qkv_util._QkvLinear does, so it composes with the q/k/v
patch, with mxfp8_util's FFN patch and with fp8_attn_util's oracle.dit.self_attn (which hands its bf16-rounded output
to oracle.dit.linear for `o`).  The same wrapper with another pattern measures the sites that stay bf16."""
import functools
import os
import re
import sys

import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import fp8_attn_util  # noqa: E402
import fp8_qkv_util  # noqa: E402
from mxfp8_util import cos, rel  # noqa: E402,F401

O_LINEAR = re.compile(r"^blocks\.\d+\.self_attn\.o$")
CROSS_O_LINEAR = re.compile(r"^blocks\.\d+\.cross_attn\.o$")  # stays bf16: the CPU test records why


class _SiteLinear:
    """oracle.dit.linear with the Linears whose name matches `site` seeing their input (after bf16 rounding) and their
    (bf16) weight quantised to MXFP8 along the row and back.  Every other name goes to the wrapped function."""

    def __init__(self, inner, site):
        self.inner, self.site = inner, site

    def __call__(self, P_, name, x):
        from stableavatar_amd import mxfp8
        if not self.site.match(name):
            return self.inner(P_, name, x)
        w = mxfp8.fake_quant(P_[name + ".weight"].bfloat16())
        return F.linear(mxfp8.fake_quant(x.bfloat16()).to(x.dtype), w.to(x.dtype), P_.get(name + ".bias"))


def oracle_forward(P, cfg, inp, fp8_o=True, fp8_qkv=False, fp8_attn=False, fp8_ffn=False, site=O_LINEAR):
    """oracle.dit.forward with any combination of the four emulations (fp8_o: the Linears matching `site`)"""
    from oracle import dit as odit
    orig = odit.linear
    if fp8_o:
        odit.linear = _SiteLinear(orig, site)
    try:
        return fp8_qkv_util.oracle_forward(P, cfg, inp, fp8_qkv, fp8_attn, fp8_ffn)
    finally:
        odit.linear = orig


@functools.lru_cache(maxsize=None)
def small_case(case, fp8_o=True, fp8_qkv=False, fp8_attn=False, fp8_ffn=False, site=O_LINEAR):
    """(P, inputs, oracle output) of DIT_SMALL's golden case `case`"""
    from golden_cases import DIT_SMALL, dit_inputs
    P = fp8_qkv_util.small_params()
    inp = dit_inputs(DIT_SMALL, case)
    return P, inp, oracle_forward(P, DIT_SMALL, inp, fp8_o, fp8_qkv, fp8_attn, fp8_ffn, site)


@functools.lru_cache(maxsize=None)
def full_dims_case(modes=(True, True, True, True)):
    """(cfg, P, inputs, oracle output with the emulations `modes` = (o, q/k/v, attention, FFN)) at the 1.3B layer dims
    (30 layers) on a tiny grid: mxfp8_util.full_dims_case's geometry"""
    cfg, P, inp, _ = fp8_attn_util._full_dims_inputs()
    return cfg, P, inp, oracle_forward(P, cfg, inp, *modes)
