"""Block lists for the opt-in block-sparse self-attention (sa_attn_fwd_sparse, ops.attention(..., blocks=)).  Host only.

A table is a CSR pair of int32 tensors: blk_ptr [nqb + 1] and blk_idx.  Query block qb -- the 256-query tile qb of a
segment -- attends the 64-key blocks blk_idx[blk_ptr[qb] : blk_ptr[qb + 1]] of its segment (strictly ascending, each
< ceil(kv_len / 64)) and no other key.  One table serves every segment and head of a launch.

The frame-window pattern (frame_window_table) is the one the DiT offers (enable_sparse_attention).  Tokens are
frame-major, as forward_window orders them: token t lies in latent frame min(t // tokens_per_frame, n_frames - 1)
(the pads past the last frame, which the dense path attends as keys, count as its last frame's).
  token rule: a query in frame fq sees a key in frame fk iff |fq - fk| <= window_frames or fk < sink_frames;
  block rule: tile (qb, kb) is listed iff some (query, key) pair in it passes the token rule.
The block rule is the mode's definition: a listed tile is attended whole, so where frames do not fill whole tiles
(tokens_per_frame not a multiple of 256) a query also sees the rest of the tiles its frame window touches.  At 512 x 512
a frame is 1024 tokens -- 4 query tiles, 16 key blocks -- and the two rules coincide.  sink_frames = 1 (every query
keeps the first latent frame) is a convention borrowed from attention-sink practice, not a measured choice; quality on
real checkpoints is unmeasured at any window.

The C entry cannot see device memory, so tables are validated here (validate) before they are uploaded.
"""
from __future__ import annotations

import numpy as np
import torch

QB = 256  # queries per tile (the 8-wave kernels' workgroup)
KVB = 64  # keys per block


def _frames(t0: int, t1: int, tokens_per_frame: int, n_frames: int):
    """first and last frame of tokens [t0, t1)"""
    return min(t0 // tokens_per_frame, n_frames - 1), min((t1 - 1) // tokens_per_frame, n_frames - 1)


def validate(blk_ptr, blk_idx, q_len: int, kv_len: int) -> None:
    """ValueError unless (blk_ptr, blk_idx) is a table for q_len queries and kv_len keys per segment: int32, one
    pointer per 256-query tile plus one, pointers from 0 up to len(blk_idx) and never falling, every list strictly
    ascending within [0, ceil(kv_len / 64))."""
    for name, t in (("blk_ptr", blk_ptr), ("blk_idx", blk_idx)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1:
            raise ValueError(f"{name}: a 1-D int32 tensor is needed")
    if q_len <= 0 or kv_len < 0:
        raise ValueError(f"q_len {q_len} / kv_len {kv_len}")
    nqb, nkb = -(-q_len // QB), -(-kv_len // KVB)
    p, x = blk_ptr.cpu().numpy().astype(np.int64), blk_idx.cpu().numpy().astype(np.int64)
    if p.size != nqb + 1:
        raise ValueError(f"blk_ptr has {p.size} entries, {nqb + 1} needed for q_len {q_len}")
    if p[0] != 0 or p[-1] != x.size or (np.diff(p) < 0).any():
        raise ValueError("blk_ptr must rise from 0 to len(blk_idx) without falling")
    if x.size and (x.min() < 0 or x.max() >= nkb):
        raise ValueError(f"blk_idx out of range [0, {nkb})")
    inner = np.ones(x.size, dtype=bool)  # positions that continue a list (not a list's first entry)
    inner[p[:-1][p[:-1] < x.size]] = False
    if x.size and (np.diff(x)[inner[1:]] <= 0).any():
        raise ValueError("blk_idx must be strictly ascending within each query block")


def frame_window_table(n_frames: int, tokens_per_frame: int, q_len: int, kv_len: int, window_frames: int,
                       sink_frames: int = 1, q_offset: int = 0):
    """(blk_ptr, blk_idx), CPU int32, of the frame-window pattern's block rule (module docstring) for q_len queries --
    tokens q_offset .. q_offset + q_len - 1 of the sequence -- and keys 0 .. kv_len - 1."""
    if min(n_frames, tokens_per_frame, q_len) <= 0 or kv_len < 0 or window_frames < 0 or sink_frames < 0 or q_offset < 0:
        raise ValueError("frame_window_table: sizes must be positive, window_frames / sink_frames / q_offset >= 0")
    nqb, nkb = -(-q_len // QB), -(-kv_len // KVB)
    klo = np.empty(nkb, dtype=np.int64)
    khi = np.empty(nkb, dtype=np.int64)
    for kb in range(nkb):
        klo[kb], khi[kb] = _frames(kb * KVB, min(kb * KVB + KVB, kv_len), tokens_per_frame, n_frames)
    ptr, idx = [0], []
    for qb in range(nqb):
        qlo, qhi = _frames(q_offset + qb * QB, q_offset + min(qb * QB + QB, q_len), tokens_per_frame, n_frames)
        # frames are contiguous in a tile and in a block: some pair is within the window iff the ranges, the queries'
        # widened by it, overlap; the sink admits a block that holds a key of a sink frame
        seen = ((klo <= qhi + window_frames) & (khi >= qlo - window_frames)) | (klo < sink_frames)
        idx.append(np.nonzero(seen)[0])
        ptr.append(ptr[-1] + idx[-1].size)
    blk_ptr = torch.tensor(ptr, dtype=torch.int32)
    blk_idx = torch.from_numpy(np.concatenate(idx).astype(np.int32)) if nkb else torch.zeros(0, dtype=torch.int32)
    validate(blk_ptr, blk_idx, q_len, kv_len)
    return blk_ptr, blk_idx


def expand(blk_ptr, blk_idx, q_len: int, kv_len: int) -> torch.Tensor:
    """The boolean token mask [q_len, kv_len] a table stands for: query i sees key j iff block j // 64 is on the list
    of tile i // 256."""
    validate(blk_ptr, blk_idx, q_len, kv_len)
    nqb, nkb = -(-q_len // QB), -(-kv_len // KVB)
    tiles = torch.zeros(nqb, nkb, dtype=torch.bool)
    p = blk_ptr.tolist()
    for qb in range(nqb):
        tiles[qb, blk_idx[p[qb]:p[qb + 1]].long()] = True
    return tiles.repeat_interleave(QB, 0)[:q_len].repeat_interleave(KVB, 1)[:, :kv_len]


def density(blk_ptr, blk_idx, q_len: int, kv_len: int) -> float:
    """listed (tile, block) pairs over all pairs"""
    return blk_idx.numel() / max(-(-q_len // QB) * -(-kv_len // KVB), 1)
