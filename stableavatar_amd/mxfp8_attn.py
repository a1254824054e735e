"""MXFP8 self-attention as the fp8 attention mode computes it -- the definition the HIP kernels
(csrc/attention_mxfp8.hip) are held to.  Plain torch, runs on the CPU.  `quantize` is mxfp8.quantize, head_dim is 128.

Operands (sa_attn_pack_mxfp8 writes exactly these bytes; with the fp8 q/k/v mode on as well, sa_qk_rmsnorm_rope_mxfp8
writes Q, sa_attn_pack_k_mxfp8 K and sa_gemm_mxfp8_vt V^T, the same bytes):
  Q    quantize(fp32(q) * c) along D (four blocks per head), c = float32(scale) * 1.4426950408889634f: the log2(e)
       prescale is folded in before quantising, so the scores come out of the MFMA in exp2 units.
  K    quantize(fp32(k) - k_mean[seg][column]) along D.  k_mean is fp32 [nseg][heads * 128] (None: no subtraction).
       Every query of a segment sees the same keys, so subtracting a per-channel constant from K moves every score of
       a row by the same amount and leaves the softmax unchanged in exact arithmetic; it removes the per-channel
       offset of K that would otherwise use up the e4m3 mantissa.
  V^T  [heads * 128][Rv] e4m3 bytes + [heads * 128][Rv / 32] scale bytes.  Segment s owns columns vcol0[s] ..
       vcol0[s] + ceil128(kv_len_s) (vcol0 in multiples of 128).  Inside each 128-key block the keys sit at the
       positions KEY_OF_POS gives (below); quantisation blocks are 32 consecutive positions of a d-row; keys at or
       past kv_len are zeros.

The position order is the one in which the P^T operand of the PV product falls out of the score accumulators with no
lane exchange.  S^T = K Q^T on the 16x16 MFMA leaves lane (query l % 16, group g = l / 16) holding keys 16 t + 4 g + e
(e = 0..3) of key tile t = 0..7; the scaled MFMA's operand lane (row l % 16, group g) supplies reduction bytes
16 g .. 16 g + 15 and 64 + 16 g .. 64 + 16 g + 15.  Packing the lane's tile t into bytes 4 (t % 4) + e of its half
t / 4 puts key 16 t + 4 g + e at position 64 (t / 4) + 16 g + 4 (t % 4) + e.

Scores and P: s = Q^ K^ in fp32; p = exp2(s - m), m the row's maximum; P^ = e4m3(RNE(p * 2^P_SHIFT)), every block's
scale byte 127 - P_SHIFT.  The kernel keeps a running maximum that lags the true one by at most LAG (its deferred
rescale), so its P^ reach 2^(P_SHIFT + LAG) <= 256 < 448.  o = (P^ V^) / sum(P^) with the sum over the rounded P in
fp32: the weights sum to one whatever the rounding did, and a one-hot P returns its V row exactly.  kv_len == 0
gives zeros.

Key split (sa_attn_fwd_mxfp8_split): the last split_tiles (segment, head, 256-query block) tiles of a launch take their
keys in two halves, each half the definition above on its own keys, merged by attend_split.
"""
from __future__ import annotations

import torch

from . import mxfp8

D = 128
KB = 128  # keys per block of the V^T layout
P_SHIFT = 4
LAG = 4
assert P_SHIFT + LAG <= 8
LOG2E_F32 = torch.tensor(1.4426950408889634, dtype=torch.float32)


def key_of_pos() -> torch.Tensor:
    """int64 [128]: the key (within its 128-key block) stored at each position of a V^T row"""
    p = torch.arange(KB)
    hi, g, t, e = p // 64, (p % 64) // 16, (p % 16) // 4, p % 4
    return (4 * hi + t) * 16 + 4 * g + e


KEY_OF_POS = key_of_pos()


def acc_to_operand_pos(t: int, g: int, e: int) -> int:
    """position of the score accumulator element (key tile t, lane group g, element e) in the P^T operand: VGPR
    4 (t / 4) + t % 4 of the lane, byte e; VGPRs 0-3 hold reduction bytes 16 g.., VGPRs 4-7 bytes 64 + 16 g.."""
    return 64 * (t // 4) + 16 * g + 4 * (t % 4) + e


def ceil128(n: int) -> int:
    return (n + KB - 1) // KB * KB


def make_vcol0(segs):
    """host side of the layout: (vcol0 list, Rv) for a list of {q_row0, q_len, kv_row0, kv_len} rows"""
    out, c = [], 0
    for s in segs:
        out.append(c)
        c += ceil128(int(s[3]))
    return out, max(c, KB)


def prescale(scale: float) -> torch.Tensor:
    return torch.tensor(scale, dtype=torch.float32) * LOG2E_F32


def quant_q(q: torch.Tensor, scale: float):
    """q [rows, heads * 128] -> (bytes, scales [rows, heads * 4])"""
    return mxfp8.quantize(q.float() * prescale(scale))


def quant_k(k: torch.Tensor, mean_row=None):
    """k [rows, heads * 128] of one segment, mean_row fp32 [heads * 128] or None"""
    k = k.float()
    return mxfp8.quantize(k if mean_row is None else k - mean_row.float())


def quant_vt(v: torch.Tensor):
    """v [kv_len, heads * 128] of one segment -> V^T (bytes [heads * 128, ceil128], scales [heads * 128, ceil128 / 32])
    in position order"""
    n, C = v.shape
    n128 = ceil128(n)
    vp = torch.zeros(n128, C, dtype=torch.float32)
    vp[:n] = v.float()
    vp = vp.reshape(n128 // KB, KB, C)[:, KEY_OF_POS]  # [block, position, column]
    return mxfp8.quantize(vp.reshape(n128, C).t().contiguous())


def dequant_v(vq: torch.Tensor, vs: torch.Tensor, n: int) -> torch.Tensor:
    """inverse of quant_vt up to the rounding: fp32 [n, heads * 128] in key order"""
    vt = mxfp8.dequantize(vq, vs)  # [C, n128]
    C, n128 = vt.shape
    vp = vt.t().reshape(n128 // KB, KB, C)
    out = torch.empty_like(vp)
    out[:, KEY_OF_POS] = vp
    return out.reshape(n128, C)[:n]


def k_mean(k: torch.Tensor, segs) -> torch.Tensor:
    """fp32 [nseg, heads * 128]: column means of k over each segment's keys (what sa_attn_kmean computes, up to the
    order of the fp32 sum)"""
    out = torch.zeros(len(segs), k.shape[1], dtype=torch.float32)
    for i, s in enumerate(segs):
        if s[3] > 0:
            out[i] = k[s[2]:s[2] + s[3]].double().mean(0).float()
    return out


def pack(q, k, v, segs, heads, scale, kmean=None):
    """The six outputs of sa_attn_pack_mxfp8 for row-major q, k, v [rows, heads * 128]: (Q bytes, Q scales, K bytes,
    K scales, V^T bytes, V^T scales, vcol0).  Rows outside every segment stay zero bytes (the kernel leaves them
    untouched)."""
    C = heads * D
    vcol0, Rv = make_vcol0(segs)
    qq = torch.zeros(q.shape[0], C, dtype=torch.uint8)
    qs = torch.zeros(q.shape[0], C // 32, dtype=torch.uint8)
    kq = torch.zeros(k.shape[0], C, dtype=torch.uint8)
    ks = torch.zeros(k.shape[0], C // 32, dtype=torch.uint8)
    vq = torch.zeros(C, Rv, dtype=torch.uint8)
    vs = torch.full((C, Rv // 32), 127, dtype=torch.uint8)
    for i, (q0, ql, k0, kl) in enumerate(segs):
        qq[q0:q0 + ql], qs[q0:q0 + ql] = quant_q(q[q0:q0 + ql], scale)
        if kl <= 0:
            continue
        kq[k0:k0 + kl], ks[k0:k0 + kl] = quant_k(k[k0:k0 + kl], None if kmean is None else kmean[i])
        n128 = ceil128(kl)
        vq[:, vcol0[i]:vcol0[i] + n128], vs[:, vcol0[i] // 32:(vcol0[i] + n128) // 32] = quant_vt(v[k0:k0 + kl])
    return qq, qs, kq, ks, vq, vs, vcol0


def dequant_operands(q, k, v, scale, mean_row=None):
    """(Q^, K^, V^) fp32 of one segment and all heads, in row / key order: what the two products multiply"""
    return (mxfp8.dequantize(*quant_q(q, scale)), mxfp8.dequantize(*quant_k(k, mean_row)),
            dequant_v(*quant_vt(v), v.shape[0]))


def attend(qd, kd, vd):
    """the definition's softmax attention on dequantised operands [.., L, 128] (leading dims batch): fp32"""
    s = qd @ kd.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    ph = torch.ldexp(p, torch.tensor(P_SHIFT)).to(torch.float8_e4m3fn).float()
    return (ph @ vd) / ph.sum(-1, keepdim=True)


QB = 256  # queries per tile of the key-split launch
DROP_GAP = 10 + P_SHIFT  # exp2(-DROP_GAP) * 2^P_SHIFT = 2^-10 is the e4m3 rounding boundary: half the least subnormal


def split_point(kv_len: int) -> int:
    """kper: the first half of a split tile is keys [0, kper), whole 128-key blocks; the second the rest"""
    return ceil128((kv_len + 1) // 2)


def attend_half(qd, kd, vd):
    """one key half by the definition on its own keys: (m its row maximum [.., L], O = P^ V^ unnormalised [.., L, 128],
    l = sum P^ [.., L]), fp32"""
    s = qd @ kd.transpose(-1, -2)
    m = s.amax(-1)
    ph = torch.ldexp(torch.exp2(s - m[..., None]), torch.tensor(P_SHIFT)).to(torch.float8_e4m3fn).float()
    return m, ph @ vd, ph.sum(-1)


def attend_split(qd, kd, vd):
    """attend() with the keys in two halves at split_point, as sa_attn_fwd_mxfp8_split runs a split tile: each half is
    the definition on its own keys (its own row maximum), merged with w_h = exp2(m_h - M), M = max(m_0, m_1):
    o = (w_0 O_0 + w_1 O_1) / (w_0 l_0 + w_1 l_1).  A half whose maximum stands more than DROP_GAP below M gets
    w_h = 0: each of its P, taken against the row's maximum as attend() takes it, rounds to zero (the flash loop's own
    drop rule, FLUSH_GAP, across halves), so a one-hot P still returns its V row exactly.  An empty second half has
    w = 0 and the result is attend()'s."""
    kper = split_point(kd.shape[-2])
    if kper >= kd.shape[-2]:
        return attend(qd, kd, vd)
    m0, O0, l0 = attend_half(qd, kd[..., :kper, :], vd[..., :kper, :])
    m1, O1, l1 = attend_half(qd, kd[..., kper:, :], vd[..., kper:, :])
    M = torch.maximum(m0, m1)
    w0 = torch.where(M - m0 > DROP_GAP, torch.zeros_like(M), torch.exp2(m0 - M))[..., None]
    w1 = torch.where(M - m1 > DROP_GAP, torch.zeros_like(M), torch.exp2(m1 - M))[..., None]
    return (w0 * O0 + w1 * O1) / (w0 * l0[..., None] + w1 * l1[..., None])


def split_mask(segs, heads, split_tiles, max_q_len=None):
    """bool [nseg][heads, q_len]: the queries in the last split_tiles tiles of the launch.  Tile = (segment, head,
    256-query block), numbered (seg * heads + h) * nqb + qb with nqb = ceil(max_q_len / 256) (sa_attn_fwd_split's
    order); tiles that hold no query count."""
    if max_q_len is None:
        max_q_len = max(int(s[1]) for s in segs)
    nqb = (max_q_len + QB - 1) // QB
    ntiles = len(segs) * heads * nqb
    if not 0 <= split_tiles <= ntiles:
        raise ValueError(f"split_tiles = {split_tiles} of {ntiles} tiles")
    out = []
    for i, s in enumerate(segs):
        tile = (i * heads + torch.arange(heads)[:, None]) * nqb + torch.arange(int(s[1]))[None, :] // QB
        out.append(tile >= ntiles - split_tiles)
    return out


def attention(q, k, v, segs, heads, scale=None, kmean=None, o_rows=None, out=None, split_tiles=0, max_q_len=None):
    """The mode's self-attention over a segment table, row-major q, k, v [rows, heads * 128] -> bf16 [rows, heads * 128]
    (row r's output at row o_rows[r] when given).  split_tiles > 0: the last split_tiles tiles of the launch
    (split_mask; max_q_len as the launch is given it, default the longest segment) by attend_split."""
    if scale is None:
        scale = D ** -0.5
    if out is None:
        out = torch.zeros(q.shape[0], heads * D, dtype=torch.bfloat16)
    mask = split_mask(segs, heads, split_tiles, max_q_len) if split_tiles else None
    for i, (q0, ql, k0, kl) in enumerate(segs):
        rows = torch.arange(q0, q0 + ql)
        if o_rows is not None:
            rows = torch.as_tensor(o_rows)[rows].long()
        if kl <= 0:
            out[rows] = 0
            continue
        qd, kd, vd = dequant_operands(q[q0:q0 + ql], k[k0:k0 + kl], v[k0:k0 + kl], scale,
                                      None if kmean is None else kmean[i])
        h = lambda t: t.reshape(t.shape[0], heads, D).transpose(0, 1)  # noqa: E731
        o = attend(h(qd), h(kd), h(vd))
        if mask is not None and mask[i].any():
            o = torch.where(mask[i][..., None], attend_split(h(qd), h(kd), h(vd)), o)
        out[rows] = o.transpose(0, 1).reshape(ql, heads * D).bfloat16()
    return out


def self_attention_bshd(q, k, v, use_kmean=True):
    """q, k, v [B, L, heads, 128] (after RMSNorm and RoPE; rounded to bf16 as the QKV buffer holds them) -> fp32
    [B, L, heads, 128]: one segment per batch row, as the DiT blocks' self-attention runs it"""
    B, L, H, _ = q.shape
    f = lambda t: t.bfloat16().reshape(B * L, H * D)  # noqa: E731
    qf, kf, vf = f(q), f(k), f(v)
    segs = [[b * L, L, b * L, L] for b in range(B)]
    km = k_mean(kf, segs) if use_kmean else None
    return attention(qf, kf, vf, segs, H, D ** -0.5, km).float().reshape(B, L, H, D)
