"""Shared by the key-split fp8 attention tests (CPU and GPU): the shape sets, the random cases with their fp64
references and the definition's errors, each computed once."""
import functools
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fp8_attn_util import rel  # noqa: E402

from stableavatar_amd import mxfp8_attn  # noqa: E402

D = 128
# the three shape sets of tests/test_gpu_fp8_attn.py::test_kernel_selects_exactly
SELECT_SHAPES = [[(77, 300), (33, 129)], [(257, 129), (77, 300)], [(33, 1000), (257, 1)]]
VARIANTS = ["plain", "sharp", "k_offset"]
RANDOM_SHAPES = [(257, 1000), (40, 300), (40, 129), (300, 257)]


def n_tiles(segs, heads, max_q_len=None):
    mq = max(s[1] for s in segs) if max_q_len is None else max_q_len
    return len(segs) * heads * ((mq + mxfp8_attn.QB - 1) // mxfp8_attn.QB)


def softmax64(qd, kd, vd, heads):
    h = lambda t: t.double().reshape(t.shape[0], heads, D).transpose(0, 1)  # noqa: E731
    s = h(qd) @ h(kd).transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return ((p @ h(vd)) / p.sum(-1, keepdim=True)).transpose(0, 1).reshape(qd.shape[0], heads * D)


def random_input(shape, variant, heads=3):
    """the data of tests/test_gpu_fp8_attn.py::test_kernel_random_within_the_definitions_error"""
    ql, kl = shape
    g = torch.Generator().manual_seed(ql + len(variant))
    q, k, v = (torch.randn(n, heads * D, generator=g) for n in (ql, kl, kl))
    if variant == "sharp":
        q = q * 4
    if variant == "k_offset":
        k = k + 3 * torch.randn(heads * D, generator=g)
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), [[0, ql, 0, kl]]


@functools.lru_cache(maxsize=None)
def random_case(shape, variant, heads=3):
    """-> dict: q, k, v, segs, km (the definition's K means), R (fp64 softmax attention on the dequantised operands),
    X (on the inputs), whole / split (the definition unsplit and with every tile split) and their errors"""
    q, k, v, segs = random_input(shape, variant, heads)
    km = mxfp8_attn.k_mean(k, segs)
    scale = D ** -0.5
    R = softmax64(*mxfp8_attn.dequant_operands(q, k, v, scale, km[0]), heads)
    X = softmax64(q.double() * float(mxfp8_attn.prescale(scale)), k.double(), v.double(), heads)
    whole = mxfp8_attn.attention(q, k, v, segs, heads, scale, km)
    split = mxfp8_attn.attention(q, k, v, segs, heads, scale, km, split_tiles=n_tiles(segs, heads))
    return dict(q=q, k=k, v=v, segs=segs, km=km, R=R, X=X, whole=whole, split=split,
                whole_R=rel(whole, R), whole_X=rel(whole, X), split_R=rel(split, R), split_X=rel(split, X))
