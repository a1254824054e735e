"""Shared by the fp8 attention tests: the CPU oracle with every DiT block's self-attention replaced by the mode's
definition (stableavatar_amd/mxfp8_attn.py), computed once per case, and the exact inputs of the kernel tests."""
import functools
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import mxfp8_util  # noqa: E402
from mxfp8_util import cos, rel  # noqa: E402,F401

D = 128


def oracle_forward(P, cfg, inp, fp8_attn=True, fp8_ffn=False):
    """oracle.dit.forward with oracle.dit.self_attn patched, for the length of this call, to the definition: q and k
    after RMSNorm and RoPE and v, rounded to bf16 as the QKV buffer holds them, through mxfp8_attn (K means on)"""
    from oracle import dit as odit
    from stableavatar_amd import mxfp8_attn
    orig = odit.self_attn

    def self_attn(P_, pre, x, grid_sizes, freqs, heads, eps=1e-6):
        b, s, dim = x.shape
        d = dim // heads
        q = odit.rms_norm(odit.linear(P_, pre + ".q", x), P_[pre + ".norm_q.weight"], eps).view(b, s, heads, d)
        k = odit.rms_norm(odit.linear(P_, pre + ".k", x), P_[pre + ".norm_k.weight"], eps).view(b, s, heads, d)
        v = odit.linear(P_, pre + ".v", x).view(b, s, heads, d)
        o = mxfp8_attn.self_attention_bshd(odit.rope_apply(q, grid_sizes, freqs), odit.rope_apply(k, grid_sizes, freqs),
                                           v)
        return odit.linear(P_, pre + ".o", o.to(x.dtype).flatten(2))

    if fp8_attn:
        odit.self_attn = self_attn
    try:
        return mxfp8_util.oracle_forward(P, cfg, inp, fp8_ffn)
    finally:
        odit.self_attn = orig


def peaky(P, factor=4.0):
    """every self-attention's norm_q weight times `factor`: scores `factor` times as sharp"""
    return {k: (v * factor if k.endswith("self_attn.norm_q.weight") else v) for k, v in P.items()}


@functools.lru_cache(maxsize=None)
def small_case(case, fp8_attn, fp8_ffn=False, peak=False):
    """(P, inputs, oracle output) of DIT_SMALL's golden case `case`"""
    from golden_cases import DIT_SMALL, dit_inputs
    from stableavatar_amd import synthetic
    from stableavatar_amd.transformer import param_shapes
    P = synthetic.fill_state_dict(param_shapes(DIT_SMALL), DIT_SMALL["seed"])
    if peak:
        P = peaky(P)
    inp = dit_inputs(DIT_SMALL, case)
    return P, inp, oracle_forward(P, DIT_SMALL, inp, fp8_attn, fp8_ffn)


@functools.lru_cache(maxsize=None)
def full_dims_case():
    """(cfg, P, inputs, emulated oracle output) at the 1.3B layer dims (30 layers) on a tiny grid"""
    cfg, P, inp, _ = _full_dims_inputs()
    return cfg, P, inp, oracle_forward(P, cfg, inp, True, False)


def _full_dims_inputs():
    from golden_cases import dit_inputs
    from oracle import dit as odit
    from stableavatar_amd import synthetic
    cfg = dict(odit.CONFIG_1_3B, seed=5)
    P = synthetic.fill_state_dict(odit.param_shapes(cfg), cfg["seed"])
    return cfg, P, dit_inputs(dict(cfg, text_dim=4096), "full"), None


# ------------------------------------------------------------------------------------------------ kernel inputs

SELECT_SEED = 3


def selection_input(shapes, heads, seed=SELECT_SEED):
    """Segments of (q_len, kv_len): K rows random +-1, Q row i = 8 K[pi(i)] for a random pi per segment, V = small
    integers times a per-key power of two.  The matching score stands ~95 exp2 units above every other, so every other
    P^ rounds to 0 and the output is V[pi] exactly.  -> (q, k, v bf16 rows, segs, expected bf16 [q rows, heads*128])"""
    g = torch.Generator().manual_seed(seed)
    C = heads * D
    qs, ks, vs, es, segs = [], [], [], [], []
    q0 = k0 = 0
    for ql, kl in shapes:
        k = (torch.randint(0, 2, (kl, C), generator=g) * 2 - 1).float()
        pi = torch.randint(0, kl, (ql,), generator=g)
        v = torch.randint(-7, 8, (kl, C), generator=g).float() * torch.exp2(
            torch.randint(-3, 4, (kl, 1), generator=g).float())
        qs.append(8 * k[pi]), ks.append(k), vs.append(v), es.append(v[pi])
        segs.append([q0, ql, k0, kl])
        q0, k0 = q0 + ql, k0 + kl
    cat = lambda ts: torch.cat(ts).bfloat16()  # noqa: E731
    return cat(qs), cat(ks), cat(vs), segs, cat(es)


def uniform_input(kv_len, q_len, heads, seed=11):
    """Q = 0: every key weighs the same; V as selection_input's, so the fp32 sums are exact in any order.
    -> (q, k, v, segs, the exact mean of V per column in float64)"""
    g = torch.Generator().manual_seed(seed)
    C = heads * D
    k = torch.randn(kv_len, C, generator=g).bfloat16()
    v = (torch.randint(-7, 8, (kv_len, C), generator=g).float() * torch.exp2(
        torch.randint(-3, 4, (kv_len, 1), generator=g).float())).bfloat16()
    q = torch.zeros(q_len, C).bfloat16()
    return q, k, v, [[0, q_len, 0, kv_len]], v.double().mean(0)
