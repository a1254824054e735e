"""Shared by the fp8 q/k/v tests: the CPU oracle with the q, k and v Linears of every DiT block's self-attention
emulated in MXFP8 (the definition of what enable_fp8_qkv() computes, up to bf16 noise).  The patch goes through
oracle.dit.linear, as mxfp8_util's FFN patch does, and wraps whatever is installed there, so it composes with that patch
and with fp8_attn_util's oracle.dit.self_attn (which calls oracle.dit.linear for q, k and v)."""
import functools
import os
import re
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import fp8_attn_util  # noqa: E402
from mxfp8_util import cos, rel  # noqa: E402,F401

QKV_LINEAR = re.compile(r"^blocks\.\d+\.self_attn\.[qkv]$")


class _QkvLinear:
    """oracle.dit.linear with blocks.N.self_attn.{q,k,v} seeing their input (after bf16 rounding) and their (bf16)
    weight quantised to MXFP8 and back.  Every other name goes to the function found in the module at call time --
    mxfp8_util installs its FFN patch after this one and takes this one as its `orig`, so both apply."""

    def __init__(self, inner):
        self.inner = inner

    def __call__(self, P_, name, x):
        from stableavatar_amd import mxfp8
        if not QKV_LINEAR.match(name):
            return self.inner(P_, name, x)
        w = mxfp8.fake_quant(P_[name + ".weight"].bfloat16())
        return F.linear(mxfp8.fake_quant(x.bfloat16()).to(x.dtype), w.to(x.dtype), P_.get(name + ".bias"))


def oracle_forward(P, cfg, inp, fp8_qkv=True, fp8_attn=False, fp8_ffn=False):
    """oracle.dit.forward with any combination of the three emulations"""
    from oracle import dit as odit
    orig = odit.linear
    if fp8_qkv:
        odit.linear = _QkvLinear(orig)
    try:
        return fp8_attn_util.oracle_forward(P, cfg, inp, fp8_attn, fp8_ffn)
    finally:
        odit.linear = orig


@functools.lru_cache(maxsize=None)
def small_params():
    from golden_cases import DIT_SMALL
    from stableavatar_amd import synthetic
    from stableavatar_amd.transformer import param_shapes
    return synthetic.fill_state_dict(param_shapes(DIT_SMALL), DIT_SMALL["seed"])


@functools.lru_cache(maxsize=None)
def small_case(case, fp8_qkv=True, fp8_attn=False, fp8_ffn=False):
    """(P, inputs, oracle output) of DIT_SMALL's golden case `case`"""
    from golden_cases import DIT_SMALL, dit_inputs
    P = small_params()
    inp = dit_inputs(DIT_SMALL, case)
    return P, inp, oracle_forward(P, DIT_SMALL, inp, fp8_qkv, fp8_attn, fp8_ffn)


@functools.lru_cache(maxsize=None)
def full_dims_case():
    """(cfg, P, inputs, oracle output with all three emulations) at the 1.3B layer dims (30 layers) on a tiny grid:
    mxfp8_util.full_dims_case's geometry"""
    cfg, P, inp, _ = fp8_attn_util._full_dims_inputs()
    return cfg, P, inp, oracle_forward(P, cfg, inp, True, True, True)
