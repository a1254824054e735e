"""Shared by the MXFP8 tests: the CPU oracle with the blocks' FFN Linears emulated in MXFP8 (the definition of what
enable_fp8_ffn() computes, up to bf16 noise), computed once per case."""
import functools
import os
import re
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

FFN_LINEAR = re.compile(r"^blocks\.\d+\.ffn\.[02]$")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm()).item()


def cos(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm())).item()


def oracle_forward(P, cfg, inp, fp8_ffn):
    """oracle.dit.forward; fp8_ffn: oracle.dit.linear patched so that ffn.0 / ffn.2 of every DiT block see their
    input (after bf16 rounding) and their (bf16) weight quantised to MXFP8 and back."""
    from oracle import dit as odit
    from stableavatar_amd import mxfp8
    orig = odit.linear

    def linear(P_, name, x):
        if not FFN_LINEAR.match(name):
            return orig(P_, name, x)
        w = mxfp8.fake_quant(P_[name + ".weight"].bfloat16())
        return F.linear(mxfp8.fake_quant(x.bfloat16()).to(x.dtype), w.to(x.dtype), P_.get(name + ".bias"))

    if fp8_ffn:
        odit.linear = linear
    try:
        with torch.no_grad():
            return odit.forward(P, cfg, inp["x"], inp["t"], inp["context"], inp["seq_len"], inp["clip_fea"], inp["y"],
                                inp["vocal"], inp["n_frames"])
    finally:
        odit.linear = orig


@functools.lru_cache(maxsize=None)
def small_case(case, fp8_ffn, qfloat8=False):
    """(P, inputs, oracle output) of DIT_SMALL's golden case; qfloat8: every parameter but the modulations rounded
    to float8_e4m3fn first (the reference's qfloat8 memory mode)"""
    from golden_cases import DIT_SMALL, dit_inputs
    from stableavatar_amd import synthetic
    from stableavatar_amd.transformer import param_shapes
    P = synthetic.fill_state_dict(param_shapes(DIT_SMALL), DIT_SMALL["seed"])
    if qfloat8:
        P = {k: (v if "modulation" in k else v.to(torch.float8_e4m3fn).float()) for k, v in P.items()}
    inp = dit_inputs(DIT_SMALL, case)
    return P, inp, oracle_forward(P, DIT_SMALL, inp, fp8_ffn)


@functools.lru_cache(maxsize=None)
def full_dims_case():
    """(cfg, P, inputs, emulated oracle output) at the 1.3B layer dims (30 layers, ffn 8960) on a tiny grid"""
    from golden_cases import dit_inputs
    from oracle import dit as odit
    from stableavatar_amd import synthetic
    cfg = dict(odit.CONFIG_1_3B, seed=5)
    P = synthetic.fill_state_dict(odit.param_shapes(cfg), cfg["seed"])
    inp = dit_inputs(dict(cfg, text_dim=4096), "full")
    return cfg, P, inp, oracle_forward(P, cfg, inp, True)
