"""Shared by the sparse self-attention tests: the CPU oracle with every DiT block's self-attention masked by the
mode's table (stableavatar_amd/sparse_attn.py), computed once per case, and the inputs of a grid at which the
frame-window table leaves blocks out."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from fp8_attn_util import peaky  # noqa: E402
from mxfp8_util import cos, rel  # noqa: E402,F401

# DIT_SMALL's golden grids are 16 and 24 tokens per frame with at most 120 tokens: one 256-query tile whose five frames
# reach into both 64-key blocks, so every frame window lists every block there and the emulated oracle is the plain one.
# "tall" is the smallest grid of the same model at which the block rule bites: a 16 x 16 latent -> 64 tokens per frame
# (one key block per frame), 5 latent frames -> 320 tokens: two query tiles, frames 0-3 and frame 4, five key blocks.
# With the synthetic weights as they are the scores are nearly flat and two blocks of ten move the output by 0.7e-2,
# inside the forward bar; with every norm_q weight x 4 (fp8_attn_util.peaky, the fp8 attention tests' sharper scores)
# the same table moves it by 3.8e-2 (window 1) and 7.2e-2 (window 0), so a forward that ignored the table fails the bar
TALL = "tall"


def inputs(cfg, case):
    """golden_cases.dit_inputs, and for `tall` the same recipe on a 16 x 16 latent"""
    from golden_cases import dit_inputs
    from stableavatar_amd import synthetic
    if case != TALL:
        return dit_inputs(cfg, case)
    B, H, W, Fw, n_frames = 3, 16, 16, 5, 17
    lat = synthetic.seeded_normal((1, 16, Fw, H, W), 111)
    y = synthetic.seeded_normal((B, 20, Fw, H, W), 112)
    neg = synthetic.seeded_normal((20, cfg["text_dim"]), 103)
    pos = synthetic.seeded_normal((25, cfg["text_dim"]), 104)
    clip = synthetic.seeded_normal((1, 257, 1280), 105).expand(3, -1, -1).contiguous()
    a = synthetic.seeded_normal((1, 39, 768), 106)
    return dict(x=torch.cat([lat] * 3), y=y, context=[neg, neg, pos], clip_fea=clip,
                vocal=torch.cat([torch.zeros_like(a), a, a]), t=torch.full((3,), 937.5),
                seq_len=Fw * (H // 2) * (W // 2), n_frames=n_frames)


def table_for(inp, window_frames, sink_frames=1):
    """the (blk_ptr, blk_idx) a single-GPU forward of `inp` builds: the grid's frames and tokens per frame, seq_len
    queries and keys"""
    from stableavatar_amd import sparse_attn
    Fw, H, W = inp["y"].shape[2], inp["x"].shape[3] // 2, inp["x"].shape[4] // 2
    S = inp["seq_len"]
    return sparse_attn.frame_window_table(Fw, H * W, S, S, window_frames, sink_frames)


def oracle_forward(P, cfg, inp, window_frames=None, sink_frames=1):
    """oracle.dit.forward; with window_frames, oracle.dit.self_attn is patched for the length of this call to softmax
    attention under sparse_attn.expand of the table the model builds for this grid (table_for)"""
    from oracle import dit as odit
    from stableavatar_amd import sparse_attn
    orig = odit.self_attn

    def self_attn(P_, pre, x, grid_sizes, freqs, heads, eps=1e-6):
        b, s, dim = x.shape
        d = dim // heads
        q = odit.rms_norm(odit.linear(P_, pre + ".q", x), P_[pre + ".norm_q.weight"], eps).view(b, s, heads, d)
        k = odit.rms_norm(odit.linear(P_, pre + ".k", x), P_[pre + ".norm_k.weight"], eps).view(b, s, heads, d)
        v = odit.linear(P_, pre + ".v", x).view(b, s, heads, d)
        fr, h, w = (int(g) for g in grid_sizes[0])
        mask = sparse_attn.expand(*sparse_attn.frame_window_table(fr, h * w, s, s, window_frames, sink_frames), s, s)
        q, k = odit.rope_apply(q, grid_sizes, freqs), odit.rope_apply(k, grid_sizes, freqs)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=mask)
        return odit.linear(P_, pre + ".o", o.transpose(1, 2).contiguous().flatten(2))

    if window_frames is not None:
        odit.self_attn = self_attn
    try:
        with torch.no_grad():
            return odit.forward(P, cfg, inp["x"], inp["t"], inp["context"], inp["seq_len"], inp["clip_fea"], inp["y"],
                                inp["vocal"], inp["n_frames"])
    finally:
        odit.self_attn = orig


@functools.lru_cache(maxsize=None)
def params(peak=False):
    """DIT_SMALL's synthetic parameters; peak: every norm_q weight x 4"""
    from golden_cases import DIT_SMALL
    from stableavatar_amd import synthetic
    from stableavatar_amd.transformer import param_shapes
    P = synthetic.fill_state_dict(param_shapes(DIT_SMALL), DIT_SMALL["seed"])
    return peaky(P) if peak else P


@functools.lru_cache(maxsize=None)
def small_case(case, window_frames=None, sink_frames=1, peak=False):
    """(P, inputs, oracle output) of DIT_SMALL on golden case `case` or TALL; window_frames None: the plain oracle"""
    from golden_cases import DIT_SMALL
    P, inp = params(peak), inputs(DIT_SMALL, case)
    return P, inp, oracle_forward(P, DIT_SMALL, inp, window_frames, sink_frames)
