"""Drop-in WanTransformer3DFantasyModel for MI355X (reference:
wan/models/wan_fantasy_transformer3d_1B.py + wan/models/vocal_projector_fantasy_1B.py).

Same constructor arguments, state_dict keys, `from_pretrained(...)` and
`forward(x, t, context, seq_len, clip_fea, y, cond_flag, vocal_embeddings, is_clip_level_modeling,
video_sample_n_frames)` as the reference; every op of the forward runs as a HIP kernel from
libstableavatar_hip.so (there is no eager/CPU fallback).

Residual stream is kept in fp32 ([B*L, dim], rows = batch-major tokens), GEMM operands in bf16,
norms/softmax/RoPE in fp32.  Weights are re-packed once per load into fused layouts:
self-attn QKV [3*dim, dim]; cross-attn text/img/vocal K|V [2*dim, dim]; patch embedding as a
[dim, 192] GEMM (K padded from 144).  Step-invariant cross-attention K/V of the text and image
context are cached across forwards (they depend only on the prompt and reference image).
"""
from __future__ import annotations

import glob
import json
import math
import os
from contextlib import contextmanager
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import ops, sp, sparse_attn


def rope_params(max_seq_len: int, dim: int, theta: float = 10000.0) -> torch.Tensor:
    """Angles of rope_params (1B:223-231) in fp64: [max_seq_len, dim/2]."""
    return torch.outer(torch.arange(max_seq_len, dtype=torch.float64),
                       1.0 / torch.pow(theta, torch.arange(0, dim, 2, dtype=torch.float64).div(dim)))


def riflex_params(max_seq_len: int, dim: int, k: int, L_test: int, L_test_scale=None,
                  theta: float = 10000.0) -> torch.Tensor:
    """Angles of get_1d_rotary_pos_embed_riflex (1B:236-291) in fp64: rope_params with the k-th
    intrinsic frequency replaced by 0.9 * 2 pi / L_test (then divided by L_test_scale)."""
    freqs = 1.0 / torch.pow(theta, torch.arange(0, dim, 2, dtype=torch.float64).div(dim))
    freqs[k - 1] = 0.9 * 2 * math.pi / L_test
    if L_test_scale is not None:
        freqs[k - 1] = freqs[k - 1] / L_test_scale
    return torch.outer(torch.arange(max_seq_len, dtype=torch.float64), freqs)


def rope_table(head_dim: int = 128, max_seq_len: int = 1024, riflex=None) -> torch.Tensor:
    """fp32 (cos, sin) table [max_seq_len, head_dim/2, 2] of the concatenated frame/height/width
    frequencies of self.freqs (1B:855-862), computed in fp64 like the reference.  riflex = (k, L_test,
    L_test_scale) swaps the frame axis for RIFLEx's frequencies (enable_riflex, 1B:890-905)."""
    d = head_dim
    df = d - 4 * (d // 6)
    frame = rope_params(max_seq_len, df) if riflex is None else riflex_params(max_seq_len, df, *riflex)
    ang = torch.cat([frame, rope_params(max_seq_len, 2 * (d // 6)), rope_params(max_seq_len, 2 * (d // 6))], dim=1)
    return torch.stack([torch.cos(ang), torch.sin(ang)], -1).float().contiguous()


def split_audio_sequence(audio_proj_length, num_frames=81):
    """vocal_projector_fantasy.py:39-78 (same integer arithmetic)."""
    tokens_per_frame = audio_proj_length / num_frames
    half = int(tokens_per_frame * 4 / 2)
    pos = []
    for i in range(int((num_frames - 1) / 4) + 1):
        if i == 0:
            pos.append(0)
        else:
            st = tokens_per_frame * ((i - 1) * 4 + 1)
            en = tokens_per_frame * (i * 4 + 1)
            pos.append(int((st + en) / 2) - 1)
    ranges = [[p - half, p + half] for p in pos]
    ranges[0] = [-(half * 2 - ranges[1][0]), ranges[1][0]]
    return ranges


def split_rows(audio_len, num_frames, expand_length=4):
    """Gather table of split_tensor_with_padding (vocal_projector_fantasy.py:81-131): per latent
    frame the source token rows, then -1 (zero rows) for front AND back padding, both appended."""
    rows = []
    for s, e in split_audio_sequence(audio_len, num_frames):
        s, e = s - expand_length, e + expand_length
        mx = audio_len - 1
        pad = max(-s, 0) + max(e - mx, 0)
        vs, ve = max(s, 0), min(e, mx)
        rows.append((list(range(vs, ve + 1)) if vs <= ve else []) + [-1] * pad)
    return rows


def vocal_dim(cfg: dict) -> int:
    """width of the vocal projector: 1536 for the 1.3B model (1B:872), the DiT width for 14B (14B:866)"""
    return cfg["dim"] if cfg.get("vocal", "1B") == "14B" else 1536


def param_shapes(cfg: dict) -> dict:
    """{state_dict key: shape} of the reference WanTransformer3DFantasyModel (1B:829-872), or of
    WanTransformer3DFantasy14BModel (14B:823-866) with cfg["vocal"] = "14B"."""
    dim, ffn, L = cfg["dim"], cfg["ffn_dim"], cfg["num_layers"]
    S = {"patch_embedding.weight": (dim, cfg["in_dim"], 1, 2, 2), "patch_embedding.bias": (dim,),
         "text_embedding.0.weight": (dim, cfg["text_dim"]), "text_embedding.0.bias": (dim,),
         "text_embedding.2.weight": (dim, dim), "text_embedding.2.bias": (dim,),
         "time_embedding.0.weight": (dim, cfg["freq_dim"]), "time_embedding.0.bias": (dim,),
         "time_embedding.2.weight": (dim, dim), "time_embedding.2.bias": (dim,),
         "time_projection.1.weight": (6 * dim, dim), "time_projection.1.bias": (6 * dim,)}
    for i in range(L):
        p = f"blocks.{i}"
        S[p + ".modulation"] = (1, 6, dim)
        for n in ("q", "k", "v", "o"):
            S[f"{p}.self_attn.{n}.weight"] = (dim, dim)
            S[f"{p}.self_attn.{n}.bias"] = (dim,)
        S[p + ".self_attn.norm_q.weight"] = (dim,)
        S[p + ".self_attn.norm_k.weight"] = (dim,)
        S[p + ".norm3.weight"] = (dim,)
        S[p + ".norm3.bias"] = (dim,)
        for n in ("q", "k", "v", "o", "k_img", "v_img", "k_vocal", "v_vocal"):
            S[f"{p}.cross_attn.{n}.weight"] = (dim, dim)
            S[f"{p}.cross_attn.{n}.bias"] = (dim,)
        for n in ("norm_q", "norm_k", "norm_k_img"):
            S[f"{p}.cross_attn.{n}.weight"] = (dim,)
        S[p + ".ffn.0.weight"] = (ffn, dim)
        S[p + ".ffn.0.bias"] = (ffn,)
        S[p + ".ffn.2.weight"] = (dim, ffn)
        S[p + ".ffn.2.bias"] = (dim,)
    S["head.modulation"] = (1, 2, dim)
    S["head.head.weight"] = (cfg["out_dim"] * 4, dim)
    S["head.head.bias"] = (cfg["out_dim"] * 4,)
    if cfg.get("model_type", "i2v") == "i2v":
        S.update({"img_emb.proj.0.weight": (1280,), "img_emb.proj.0.bias": (1280,),
                  "img_emb.proj.1.weight": (1280, 1280), "img_emb.proj.1.bias": (1280,),
                  "img_emb.proj.3.weight": (dim, 1280), "img_emb.proj.3.bias": (dim,),
                  "img_emb.proj.4.weight": (dim,), "img_emb.proj.4.bias": (dim,)})
    vp = "vocal_projector"
    # 1.3B: FantasyTalkingVocalCondition1BModel(audio_proj_dim=1536) (1B:872, vocal_projector_fantasy_1B.py:
    # 389-431); 14B: audio_proj_dim = dim and a two-layer audio projection 768 -> 2048 -> dim (14B:866,
    # vocal_projector_fantasy_14B.py:385-425); both: 2 blocks of 8 heads, ffn 2 x width, final head
    vd = vocal_dim(cfg)
    if cfg.get("vocal", "1B") == "14B":
        S[vp + ".proj_model.proj_1.weight"] = (2048, 768)
        S[vp + ".proj_model.norm_1.weight"] = (2048,)
        S[vp + ".proj_model.norm_1.bias"] = (2048,)
        S[vp + ".proj_model.proj_2.weight"] = (vd, 2048)
        S[vp + ".proj_model.norm_2.weight"] = (vd,)
        S[vp + ".proj_model.norm_2.bias"] = (vd,)
    else:
        S[vp + ".proj_model.proj.weight"] = (vd, 768)
        S[vp + ".proj_model.norm.weight"] = (vd,)
        S[vp + ".proj_model.norm.bias"] = (vd,)
    for i in range(2):
        bp = f"{vp}.blocks.{i}"
        S[bp + ".modulation"] = (1, 6, vd)
        S[bp + ".norm3.weight"] = (vd,)
        S[bp + ".norm3.bias"] = (vd,)
        for n in ("q", "o"):
            S[f"{bp}.cross_attn.{n}.weight"] = (vd, vd)
            S[f"{bp}.cross_attn.{n}.bias"] = (vd,)
        for n in ("k", "v"):
            S[f"{bp}.cross_attn.{n}.weight"] = (vd, dim)
            S[f"{bp}.cross_attn.{n}.bias"] = (vd,)
        S[bp + ".cross_attn.norm_q.weight"] = (vd,)
        S[bp + ".cross_attn.norm_k.weight"] = (vd,)
        S[bp + ".ffn.0.weight"] = (2 * vd, vd)
        S[bp + ".ffn.0.bias"] = (2 * vd,)
        S[bp + ".ffn.2.weight"] = (vd, 2 * vd)
        S[bp + ".ffn.2.bias"] = (vd,)
    S[vp + ".final_head.modulation"] = (1, 2, vd)
    S[vp + ".final_head.final_proj.weight"] = (vd, vd)
    S[vp + ".final_head.final_proj.bias"] = (vd,)
    return S


def _register_tree(root: nn.Module, shapes: dict, dtype):
    for name, shp in shapes.items():
        *path, leaf = name.split(".")
        mod = root
        for p in path:
            if not hasattr(mod, p) or not isinstance(getattr(mod, p), nn.Module):
                mod.add_module(p, nn.Module())
            mod = getattr(mod, p)
        mod.register_parameter(leaf, nn.Parameter(torch.empty(shp, dtype=dtype), requires_grad=False))


class _Seg:
    """Cache of device segment tables {q_row0, q_len, kv_row0, kv_len} for sa_attn_fwd."""

    def __init__(self):
        self._c = {}
        self._rows = {}  # id(table) -> its host rows (the tables live as long as the cache)
        self._vt = {}  # id(table) -> (vcol0 device int32, Rv, max kv_len): the fp8 attention's V^T layout

    def get(self, key, rows, device):
        t = self._c.get(key)
        if t is None or t.device != device:
            t = torch.tensor(rows, dtype=torch.int32).reshape(-1, 4).to(device)
            self._c[key] = t
            self._rows[id(t)] = [list(r) for r in torch.tensor(rows).reshape(-1, 4).tolist()]
            self._vt.pop(id(t), None)
        return t

    def blocks(self, key, build, device):
        """Device (blk_ptr, blk_idx) of a block-sparse table, built on the host by build() once per key"""
        t = self._c.get(key)
        if t is None or t[0].device != device:
            t = self._c[key] = tuple(x.to(device) for x in build())
        return t

    def vt_layout(self, table):
        """(vcol0, Rv, max kv_len) of a table this cache handed out: each segment's first V^T column (host-computed,
        multiples of 128) for ops.attention_mxfp8"""
        lay = self._vt.get(id(table))
        if lay is None:
            rows = self._rows[id(table)]
            vcol0, Rv = ops.attn_vcol0(rows)
            lay = (torch.tensor(vcol0, dtype=torch.int32).to(table.device), Rv, max(r[3] for r in rows))
            self._vt[id(table)] = lay
        return lay


SP_BATCHED, SP_ROWS, SP_ROWS_X, SP_STREAMS = "0", "2", "3", "4"  # the exchange schedules, by their SA_SP_OVERLAP value


def sp_schedule(overlap: str, B: int, wg_row: int, n_cu: int, gpu: bool) -> str:
    """The sequence-parallel exchange schedule of the DiT blocks for SA_SP_OVERLAP = `overlap`: 0 one synchronous
    batched exchange per direction; 2 per-row exchanges and per-row attention; 3 per-row Q/K/V exchanges, batched
    attention; 4 every CFG row through the whole block on its own HIP stream (more than one row, on a GPU); 1 = auto:
    4, else 2 when per-row attention launches add no waves over the CUs -- a row's launch has wg_row = ceil(Lq / 256)
    x hg workgroups and B serial launches must not need more rounds than the batched one -- else 3 (N = 8: 63
    workgroups per row would leave most CUs idle, but the Q/K/V exchange of row b can still travel under the QKV GEMMs
    of rows b+1..; per-row GEMMs there take as many rounds over the CUs as the batched one).  With a single row 3 and
    4 are the batched schedule."""
    if overlap == "1":
        if B > 1 and gpu:
            # one stream per CFG row through the whole block: its compute alone matches the best of the
            # other schedules at every degree (per-rank forward with the transfers stubbed out, N = 2 / 4 / 8:
            # 197.2 / 103.3 / 59.3 ms vs 198.5 / 103.8 / 59.0 ms, profiles/r04/sp_rank_compute_r4s.jsonl)
            # and every transfer travels under the other rows' work
            return SP_STREAMS
        return SP_ROWS if B * -(-wg_row // n_cu) <= -(-(B * wg_row) // n_cu) else SP_ROWS_X
    if overlap == SP_ROWS or (overlap == SP_ROWS_X and B > 1) or (overlap == SP_STREAMS and B > 1 and gpu):
        return overlap
    return SP_BATCHED


class WanTransformer3DFantasyModel(nn.Module):
    """Audio-driven Wan-2.1 DiT (1B:741-1184) on HIP kernels."""

    VOCAL = "1B"  # vocal projector family (param_shapes)

    def __init__(self, model_type="i2v", patch_size=(1, 2, 2), text_len=512, in_dim=16, dim=2048, ffn_dim=8192,
                 freq_dim=256, text_dim=4096, out_dim=16, num_heads=16, num_layers=32, window_size=(-1, -1),
                 qk_norm=True, cross_attn_norm=True, eps=1e-6, in_channels=16, hidden_size=2048, **_):
        super().__init__()
        assert model_type in ("t2v", "i2v")
        if tuple(patch_size) != (1, 2, 2) or not qk_norm or not cross_attn_norm:
            raise ValueError("the StableAvatar path uses patch (1,2,2), qk_norm and cross_attn_norm (1B:1234-1237)")
        if tuple(window_size) != (-1, -1):
            raise ValueError("windowed attention is not part of the inference path")
        assert dim % num_heads == 0 and dim // num_heads == 128, "HIP attention kernel is built for head_dim 128"
        self.model_type = model_type
        self.patch_size = tuple(patch_size)
        self.text_len, self.in_dim, self.dim, self.ffn_dim = text_len, in_dim, dim, ffn_dim
        self.freq_dim, self.text_dim, self.out_dim = freq_dim, text_dim, out_dim
        self.num_heads, self.num_layers, self.eps = num_heads, num_layers, eps
        self.d = dim // num_heads
        self.config = SimpleNamespace(model_type=model_type, patch_size=self.patch_size, text_len=text_len,
                                      in_dim=in_dim, dim=dim, ffn_dim=ffn_dim, freq_dim=freq_dim, text_dim=text_dim,
                                      out_dim=out_dim, num_heads=num_heads, num_layers=num_layers,
                                      window_size=window_size, qk_norm=qk_norm, cross_attn_norm=cross_attn_norm,
                                      eps=eps, in_channels=in_channels, hidden_size=hidden_size)
        self._cfg = dict(model_type=model_type, dim=dim, ffn_dim=ffn_dim, freq_dim=freq_dim, text_dim=text_dim,
                         in_dim=in_dim, out_dim=out_dim, num_heads=num_heads, num_layers=num_layers,
                         text_len=text_len, vocal=self.VOCAL)
        self.vd = vocal_dim(self._cfg)
        _register_tree(self, param_shapes(self._cfg), torch.float32)
        self.sp_world_size, self.sp_world_rank, self.sp_group = 1, 0, None
        self.teacache = None  # enable_teacache() (1B:867)
        self._riflex = None  # enable_riflex() (1B:890-905)
        self.attn_kernel = 0  # self-attention schedule (sa_attn_fwd_ex; 0 = auto), for in-situ A/B
        self._fp8_ffn = False  # enable_fp8_ffn(): the blocks' FFN GEMMs on MXFP8 operands
        self._fp8_attn = False  # enable_fp8_attention(): the blocks' self-attention on MXFP8 operands
        self._sparse = None  # enable_sparse_attention(): (window_frames, sink_frames) of the frame-window block lists
        self._fp8_qkv = False  # enable_fp8_qkv(): the blocks' self-attention q/k/v Linears on MXFP8 operands
        # with _fp8_qkv and _fp8_attn both on, the single-GPU sites write the attention operands where their values are
        # made (_self_attention_rows); False: the mode's GEMM, then _self_attn -- the same output bytes (for the A/B)
        self._fp8_qkv_fused = True
        self._fp8_o = False  # enable_fp8_o(): the blocks' self-attention O-projection on MXFP8 operands
        # with _fp8_o and _fp8_attn both on, the single-GPU sites have the flash kernel write the O-projection's operand
        # (_self_attention_rows); False: bf16 attention output, then the quantiser -- the same bytes (for the A/B)
        self._fp8_o_fused = True
        self._rstreams = None  # _row_streams(): the HIP streams of the per-CFG-row sequence-parallel schedule
        self._packed = None
        self._ws = {}
        self._ctx_cache = None
        self._segs = _Seg()
        self._sp_ex = None
        self._split_cache = {}
        self._events = None  # optional list to record (start, end) events around self-attention
        self._sp_enabled = False
        self._sp_loopback = False

    # ------------------------------------------------------------------ loading

    @classmethod
    def from_config(cls, config, **kw):
        import inspect
        p = set(inspect.signature(cls.__init__).parameters) - {"self"}
        return cls(**{k: v for k, v in {**config, **kw}.items() if k in p})

    @classmethod
    def from_pretrained(cls, pretrained_model_path, subfolder=None, transformer_additional_kwargs={},
                        low_cpu_mem_usage=False, torch_dtype=torch.bfloat16):
        """Same directory contract as 1B:1210-1339: config.json + diffusion_pytorch_model
        .bin/.safetensors or sharded *.safetensors; dict_mapping; forced patch/qk/cross norms;
        size-mismatched keys skipped; patch_embedding in_dim widening zero-filled."""
        if subfolder is not None:
            pretrained_model_path = os.path.join(pretrained_model_path, subfolder)
        cfg_file = os.path.join(pretrained_model_path, "config.json")
        if not os.path.isfile(cfg_file):
            raise RuntimeError(f"{cfg_file} does not exist")
        with open(cfg_file) as f:
            config = json.load(f)
        kw = dict(transformer_additional_kwargs)
        for key, target in kw.pop("dict_mapping", {}).items():
            kw[target] = config[key]
        kw.update(patch_size=(1, 2, 2), qk_norm=True, window_size=(-1, -1), cross_attn_norm=True)
        model = cls.from_config(config, **kw)
        bin_file = os.path.join(pretrained_model_path, "diffusion_pytorch_model.bin")
        st_file = bin_file.replace(".bin", ".safetensors")
        if os.path.exists(bin_file):
            sd = torch.load(bin_file, map_location="cpu", weights_only=True)
        else:
            from safetensors.torch import load_file
            files = [st_file] if os.path.exists(st_file) else sorted(
                glob.glob(os.path.join(pretrained_model_path, "*.safetensors")))
            sd = {}
            for fn in files:
                sd.update(load_file(fn))
        own = model.state_dict()
        pe = "patch_embedding.weight"
        if pe in sd and sd[pe].shape != own[pe].shape and sd[pe].shape[1] < own[pe].shape[1]:
            w = torch.zeros(own[pe].shape, dtype=sd[pe].dtype)
            w[:, :sd[pe].shape[1]] = sd[pe]
            sd[pe] = w
        sd = {k: v for k, v in sd.items() if k in own and own[k].shape == v.shape}
        model.load_state_dict(sd, strict=False)
        return model.to(torch_dtype)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        self._packed = None
        self._ctx_cache = None
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def _apply(self, fn, recurse=True):
        self._packed = None
        self._ctx_cache = None
        self._ws = {}
        return super()._apply(fn, recurse)

    def enable_riflex(self, k=6, L_test=66, L_test_scale=4.886):
        """1B:890-905: RIFLEx frame frequencies for length extrapolation."""
        self._riflex = (k, L_test, L_test_scale)
        self._set_rope()

    def disable_riflex(self):
        """1B:907-916."""
        self._riflex = None
        self._set_rope()

    def _set_rope(self):
        if self._packed is not None:
            self._packed.rope = rope_table(self.d, riflex=self._riflex).to(self._packed.rope.device)

    def enable_teacache(self, coefficients, num_steps: int, rel_l1_thresh: float, num_skip_start_steps: int = 0,
                        offload: bool = True):
        """1B:874-885 (inference.py:526-535)."""
        from .teacache import TeaCache
        self.teacache = TeaCache(coefficients, num_steps, rel_l1_thresh=rel_l1_thresh,
                                 num_skip_start_steps=num_skip_start_steps, offload=offload)

    def disable_teacache(self):
        self.teacache = None

    def enable_fp8_ffn(self, enabled=True):
        """MI355X addition (no counterpart in the reference; changes numerics): the FFN of every DiT block --
        norm2 + modulate, ffn.0 + GELU, ffn.2 + gated residual (1B:687-691) -- runs its two GEMMs on MXFP8 operands
        (stableavatar_amd/mxfp8.py; block-scaled e4m3 MFMA, fp32 accumulation).  Everything else, the vocal
        projector's FFN included, stays bf16.  Toggling drops the packed weights and the workspace: the next forward
        re-packs (ffn.0 / ffn.2 quantised from the same bf16 weights the bf16 path packs)."""
        enabled = bool(enabled)
        if enabled and (self.dim % 128 or self.ffn_dim % 128):
            raise ValueError(f"enable_fp8_ffn: dim {self.dim} and ffn_dim {self.ffn_dim} must be multiples of 128")
        if enabled != self._fp8_ffn:
            self._fp8_ffn = enabled
            self._packed = None
            self._ws = {}

    def enable_fp8_attention(self, enabled=True):
        """MI355X addition (no counterpart in the reference; changes numerics): the self-attention of every DiT block
        (1B:383-413) runs both its products, Q K^T and P V, on MXFP8 operands (stableavatar_amd/mxfp8_attn.py is the
        definition; block-scaled e4m3 MFMA, fp32 softmax and accumulation).  Cross-attention, the vocal projector's
        attention and every GEMM are untouched; combines with enable_fp8_ffn().  Off, the calls made are the bf16
        path's.  Toggling drops the workspace (the operand buffers live there); the packed weights stay."""
        enabled = bool(enabled)
        if enabled and self.d != 128:
            raise ValueError(f"enable_fp8_attention: head_dim {self.d} != 128")
        if enabled and self._sparse is not None:
            raise NotImplementedError("enable_fp8_attention: the MXFP8 flash kernel has no block-sparse form")
        if enabled != self._fp8_attn:
            self._fp8_attn = enabled
            self._ws = {}

    def enable_fp8_qkv(self, enabled=True):
        """MI355X addition (no counterpart in the reference; changes numerics): the q, k and v Linears of every DiT
        block's self-attention (1B:383-413) run on MXFP8 operands -- the bf16 norm1 + modulate output and the bf16
        weights quantised by mxfp8.quantize, fp32 accumulation, bias, bf16 rounding; RMSNorm, RoPE and the attention
        see that bf16 result as before.  The vocal projector and cross-attention are untouched; independent of
        enable_fp8_ffn() and enable_fp8_attention(), every combination works.  With the mode on the single-GPU sites
        keep V in rows: sa_gemm_mxfp8 has no SA_EPI_BF16_TP32, so the bf16 V^T attention kernel 3 is not used.  Together
        with enable_fp8_attention() those sites write the attention's operands where the values are made (V^T from
        the V GEMM's epilogue, Q from the RMSNorm + RoPE kernel), bit-identical to the separate pack.  The
        sequence-parallel sites use the mode for the GEMM only (the exchange carries bf16).  Toggling drops the packed
        weights and the workspace, as enable_fp8_ffn does."""
        enabled = bool(enabled)
        if enabled and self.dim % 128:
            raise ValueError(f"enable_fp8_qkv: dim {self.dim} must be a multiple of 128")
        if enabled != self._fp8_qkv:
            self._fp8_qkv = enabled
            self._packed = None
            self._ws = {}

    def enable_fp8_o(self, enabled=True):
        """MI355X addition (no counterpart in the reference; changes numerics): the output projection of every DiT
        block's self-attention (blocks.N.self_attn.o, 1B:413) runs on MXFP8 operands.  Its input is the attention output
        after its bf16 rounding, quantised by mxfp8.quantize along the row (32-column blocks, four per 128-wide head, none
        straddling a head); its weight is the bf16 weight quantised by mxfp8.quantize along K; the product is
        accumulated in fp32; bias, gate and residual follow SA_EPI_RES_F32 as in the bf16 path.  cross_attn.o,
        cross_attn.q and the vocal projector stay bf16.  Independent of enable_fp8_ffn(), enable_fp8_attention() and
        enable_fp8_qkv(), every combination works.  With enable_fp8_attention() the single-GPU sites have the flash
        kernel write the operand itself (sa_attn_fwd_mxfp8_o8: the bytes of the bf16 output quantised, so O never goes
        to memory as bf16); without it, and at the sequence-parallel sites (whose exchange and panels stay bf16), the
        bf16 attention output goes through the quantiser first -- one more pass over it, kept so that every combination
        is correct and not expected to be faster than the bf16 projection.  The operand bytes are the same on every
        layout.  Toggling drops the packed weights and the workspace, as enable_fp8_qkv does."""
        enabled = bool(enabled)
        if enabled and self.dim % 128:
            raise ValueError(f"enable_fp8_o: dim {self.dim} must be a multiple of 128")
        if enabled != self._fp8_o:
            self._fp8_o = enabled
            self._packed = None
            self._ws = {}

    def enable_sparse_attention(self, window_frames, sink_frames=1, enabled=True):
        """MI355X addition (no counterpart in the reference; changes the function computed): the self-attention of
        every DiT block (1B:383-413) attends, per 256-query tile, only the 64-key blocks of the frame-window pattern
        (stableavatar_amd/sparse_attn.py is the definition: latent frames within window_frames of the query's, plus
        the first sink_frames frames, at tile granularity) through sa_attn_fwd_sparse on the bf16 flash kernels.  The
        tables depend on the grid and the sequence length alone and are cached with the segment tables; the same table
        serves every CFG row, head and layer, and under sequence parallelism every rank (each attends the whole
        sequence for its heads; no launch is key-split while the mode is on).  Cross-attention and the vocal projector
        are untouched.  A window that covers every frame lists every block and reproduces the dense output byte for
        byte.  sink_frames = 1 is a convention, not a measured choice, and quality on real checkpoints is unmeasured at
        any window.  Not combined with enable_fp8_attention() (NotImplementedError).  Off, the calls made are the
        dense path's."""
        if not enabled:
            self._sparse = None
            return
        if self._fp8_attn:
            raise NotImplementedError("enable_sparse_attention: the MXFP8 flash kernel has no block-sparse form")
        if self.d != 128:
            raise ValueError(f"enable_sparse_attention: head_dim {self.d} != 128")
        window_frames, sink_frames = int(window_frames), int(sink_frames)
        if window_frames < 0 or sink_frames < 0:
            raise ValueError("enable_sparse_attention: window_frames and sink_frames must be >= 0")
        self._sparse = (window_frames, sink_frames)

    def _self_attn(self, f, q, k, v, out, segs, kernel=0, split_tiles=0):
        """One self-attention launch of a DiT block over the segment table `segs` (f: the forward's state, whose Lq,
        hg and omap are the launch's query rows per segment, heads and output row map): ops.attention, or with
        enable_fp8_attention() the K means, the operand pack and the MXFP8 flash kernel (ops.attention_mxfp8; `out` may
        then be an ops.Mx8, the fp8 self-O mode's operand);
        split_tiles (ops.attn_tail_split, given by the sequence-parallel sites alone; in fp8 mode by the batched one
        alone, see _sp_block_streams) goes to either.  The operand buffers and the split's scratch live in the
        workspace, one set per segment table (the per-row streams run concurrently, each on its own table), allocated
        on first use."""
        nseg = segs.shape[0]
        if not self._fp8_attn:
            if f.blocks is not None:
                return ops.attention(q, k, v, out, segs, nseg, f.Lq, f.hg, kernel=kernel, o_rows=f.omap,
                                     split_tiles=split_tiles, blocks=f.blocks)
            return ops.attention(q, k, v, out, segs, nseg, f.Lq, f.hg, kernel=kernel, o_rows=f.omap,
                                 split_tiles=split_tiles)
        vcol0, Rv, max_kv = self._segs.vt_layout(segs)
        key = (id(segs), q.shape[0], k.shape[0], f.hg)
        buf = f.ws.attn8.get(key)
        if buf is None:
            buf = f.ws.attn8[key] = ops.AttnMx8(q.shape[0], k.shape[0], f.hg, Rv, nseg, q.device)
        return ops.attention_mxfp8(q, k, v, out, segs, nseg, f.Lq, f.hg, vcol0, max_kv, buf, o_rows=f.omap,
                                   split_tiles=split_tiles)

    def enable_multi_gpus_inference(self, group=None, loopback=None):
        """Ulysses sequence parallelism over torch.distributed (RCCL); replaces the xfuser path
        installed at 1B:918-923 with single-GPU semantics.  loopback=True (default: env
        SA_SP_LOOPBACK=1) also sends this rank's own token chunk through the point-to-point transport (a transfer
        to itself), so at degree 1 every exchange of the layer runs on RCCL; the output is unchanged."""
        import torch.distributed as dist
        self.sp_group = group
        self.sp_world_size = dist.get_world_size(group)
        self.sp_world_rank = dist.get_rank(group)
        self._sp_enabled = True  # the exchange path runs even at degree 1 (pack + row-mapped attention + panels)
        self._sp_loopback = (os.environ.get("SA_SP_LOOPBACK", "0") == "1") if loopback is None else bool(loopback)

    def disable_multi_gpus_inference(self):
        """back to single-GPU forwards (every rank its own clip)"""
        self.sp_group, self.sp_world_size, self.sp_world_rank = None, 1, 0
        self._sp_enabled = False

    # ------------------------------------------------------------------ packing

    def _pack(self):
        if self._packed is not None:
            return self._packed
        dev = self.patch_embedding.weight.device
        if dev.type != "cuda":
            raise RuntimeError("WanTransformer3DFantasyModel runs on the MI355X HIP kernels: move it to 'cuda'")
        # parameters stored as float8_e4m3fn by the reference's qfloat8 memory mode
        # (wan/utils/fp8_optimization.py:29-43, inference.py:517-518) are upcast exactly before packing
        fp8 = (torch.float8_e4m3fn, torch.float8_e5m2)
        P = {k: (v.detach().float() if v.dtype in fp8 else v) for k, v in self.named_parameters()}
        bf = lambda n: P[n].detach().to(torch.bfloat16).contiguous()  # noqa: E731
        f32 = lambda n: P[n].detach().float().contiguous()  # noqa: E731
        cat_bf = lambda *ns: torch.cat([P[n].detach() for n in ns], 0).to(torch.bfloat16).contiguous()  # noqa: E731
        cat_f = lambda *ns: torch.cat([P[n].detach() for n in ns], 0).float().contiguous()  # noqa: E731
        dim = self.dim
        pk = SimpleNamespace()
        kin = self.in_dim * 4
        pk.kpad = ((kin + 63) // 64) * 64
        wpe = torch.zeros(dim, pk.kpad, device=dev, dtype=torch.bfloat16)
        wpe[:, :kin] = P["patch_embedding.weight"].detach().reshape(dim, kin).to(torch.bfloat16)
        pk.w_pe, pk.b_pe = wpe, f32("patch_embedding.bias")
        tkpad = ((self.text_dim + 63) // 64) * 64
        pk.text_kpad = tkpad
        w0 = torch.zeros(dim, tkpad, device=dev, dtype=torch.bfloat16)
        w0[:, :self.text_dim] = P["text_embedding.0.weight"].detach().to(torch.bfloat16)
        pk.w_t0, pk.b_t0 = w0, f32("text_embedding.0.bias")
        pk.w_t2, pk.b_t2 = bf("text_embedding.2.weight"), f32("text_embedding.2.bias")
        pk.w_te0, pk.b_te0 = bf("time_embedding.0.weight"), f32("time_embedding.0.bias")
        pk.w_te2, pk.b_te2 = bf("time_embedding.2.weight"), f32("time_embedding.2.bias")
        pk.w_tp, pk.b_tp = bf("time_projection.1.weight"), f32("time_projection.1.bias")
        pk.mod = torch.cat([P[f"blocks.{i}.modulation"].detach() for i in range(self.num_layers)], 0).float().contiguous()
        pk.layers = []
        # per-frame vocal K|V weights of every block stacked [layers * 2 * dim, vd]: the vocal context is the same for
        # all blocks of a forward, so one GEMM forms every block's vocal keys and values (L.w_kv_v are views)
        pk.w_kv_v_all = torch.cat([P[f"blocks.{i}.cross_attn.{n}_vocal.weight"].detach() for i in range(self.num_layers)
                                   for n in ("k", "v")], 0).to(torch.bfloat16).contiguous()
        pk.b_kv_v_all = torch.cat([P[f"blocks.{i}.cross_attn.{n}_vocal.bias"].detach() for i in range(self.num_layers)
                                   for n in ("k", "v")], 0).float().contiguous()
        for i in range(self.num_layers):
            p = f"blocks.{i}."
            L = SimpleNamespace(i=i)  # i: the block's index (its rows of the per-forward context and vocal K|V)
            L.w_qkv = cat_bf(p + "self_attn.q.weight", p + "self_attn.k.weight", p + "self_attn.v.weight")
            L.b_qkv = cat_f(p + "self_attn.q.bias", p + "self_attn.k.bias", p + "self_attn.v.bias")
            if self._fp8_qkv:  # quantised along K on the GPU (= mxfp8.quantize), the bf16 copy dropped
                L.w_qkv = ops.mxfp8_quant(L.w_qkv)
            # views for the single-GPU V^T path: q|k rows into the QKV rows, v into V^T (EPI_BF16_TP32, or with
            # enable_fp8_qkv() + enable_fp8_attention() sa_gemm_mxfp8_vt)
            L.w_qk, L.b_qk = L.w_qkv[:2 * self.dim], L.b_qkv[:2 * self.dim]
            L.w_v, L.b_v = L.w_qkv[2 * self.dim:], L.b_qkv[2 * self.dim:]
            L.nq, L.nk = f32(p + "self_attn.norm_q.weight"), f32(p + "self_attn.norm_k.weight")
            L.w_o, L.b_o = bf(p + "self_attn.o.weight"), f32(p + "self_attn.o.bias")
            if self._fp8_o:  # quantised along K on the GPU (= mxfp8.quantize), the bf16 copy dropped
                L.w_o = ops.mxfp8_quant(L.w_o)
            L.n3w, L.n3b = f32(p + "norm3.weight"), f32(p + "norm3.bias")
            c = p + "cross_attn."
            L.w_cq, L.b_cq = bf(c + "q.weight"), f32(c + "q.bias")
            L.cnq, L.cnk, L.cnki = f32(c + "norm_q.weight"), f32(c + "norm_k.weight"), f32(c + "norm_k_img.weight")
            L.w_kv_t, L.b_kv_t = cat_bf(c + "k.weight", c + "v.weight"), cat_f(c + "k.bias", c + "v.bias")
            L.w_kv_i, L.b_kv_i = cat_bf(c + "k_img.weight", c + "v_img.weight"), cat_f(c + "k_img.bias", c + "v_img.bias")
            L.w_kv_v, L.b_kv_v = pk.w_kv_v_all[2 * dim * i:2 * dim * (i + 1)], pk.b_kv_v_all[2 * dim * i:2 * dim * (i + 1)]
            L.w_co, L.b_co = bf(c + "o.weight"), f32(c + "o.bias")
            L.w_f0, L.b_f0 = bf(p + "ffn.0.weight"), f32(p + "ffn.0.bias")
            L.w_f2, L.b_f2 = bf(p + "ffn.2.weight"), f32(p + "ffn.2.bias")
            if self._fp8_ffn:  # the bf16 weights quantised on the GPU (= mxfp8.quantize), the bf16 copies dropped
                L.w_f0, L.w_f2 = ops.mxfp8_quant(L.w_f0), ops.mxfp8_quant(L.w_f2)
            pk.layers.append(L)
        pk.head_mod = f32("head.modulation").reshape(1, 2, dim)
        pk.w_head, pk.b_head = bf("head.head.weight"), f32("head.head.bias")
        if self.model_type == "i2v":
            pk.ie0w, pk.ie0b = f32("img_emb.proj.0.weight"), f32("img_emb.proj.0.bias")
            pk.w_ie1, pk.b_ie1 = bf("img_emb.proj.1.weight"), f32("img_emb.proj.1.bias")
            pk.w_ie3, pk.b_ie3 = bf("img_emb.proj.3.weight"), f32("img_emb.proj.3.bias")
            pk.ie4w, pk.ie4b = f32("img_emb.proj.4.weight"), f32("img_emb.proj.4.bias")
        vp = "vocal_projector."
        V = SimpleNamespace()
        if self.VOCAL == "14B":  # two-layer audio projection (vocal_projector_fantasy_14B.py:385-398)
            V.proj = [(bf(vp + "proj_model.proj_1.weight"), f32(vp + "proj_model.norm_1.weight"),
                       f32(vp + "proj_model.norm_1.bias")),
                      (bf(vp + "proj_model.proj_2.weight"), f32(vp + "proj_model.norm_2.weight"),
                       f32(vp + "proj_model.norm_2.bias"))]
        else:
            V.proj = [(bf(vp + "proj_model.proj.weight"), f32(vp + "proj_model.norm.weight"),
                       f32(vp + "proj_model.norm.bias"))]
        V.mod = torch.cat([P[f"{vp}blocks.{i}.modulation"].detach() for i in range(2)], 0).float().contiguous()
        V.blocks = []
        for i in range(2):
            b = f"{vp}blocks.{i}."
            B_ = SimpleNamespace()
            B_.n3w, B_.n3b = f32(b + "norm3.weight"), f32(b + "norm3.bias")
            B_.w_q, B_.b_q = bf(b + "cross_attn.q.weight"), f32(b + "cross_attn.q.bias")
            B_.w_kv = cat_bf(b + "cross_attn.k.weight", b + "cross_attn.v.weight")
            B_.b_kv = cat_f(b + "cross_attn.k.bias", b + "cross_attn.v.bias")
            B_.nq, B_.nk = f32(b + "cross_attn.norm_q.weight"), f32(b + "cross_attn.norm_k.weight")
            B_.w_o, B_.b_o = bf(b + "cross_attn.o.weight"), f32(b + "cross_attn.o.bias")
            B_.w_f0, B_.b_f0 = bf(b + "ffn.0.weight"), f32(b + "ffn.0.bias")
            B_.w_f2, B_.b_f2 = bf(b + "ffn.2.weight"), f32(b + "ffn.2.bias")
            V.blocks.append(B_)
        V.fmod = f32(vp + "final_head.modulation").reshape(1, 2, self.vd)
        V.w_fp, V.b_fp = bf(vp + "final_head.final_proj.weight"), f32(vp + "final_head.final_proj.bias")
        pk.vocal = V
        pk.rope = rope_table(self.d, riflex=self._riflex).to(dev)
        self._packed = pk
        return pk

    # ------------------------------------------------------------------ workspace

    def _workspace(self, M, dev):
        key = (M, dev)
        ws = self._ws.get(key)
        if ws is None:
            dim = self.dim
            ws = SimpleNamespace(
                x=torch.empty(M, dim, device=dev, dtype=torch.float32),
                mod=torch.empty(M, dim, device=dev, dtype=torch.bfloat16),
                qkv=torch.empty(M, 3 * dim, device=dev, dtype=torch.bfloat16),
                att=torch.empty(M, dim, device=dev, dtype=torch.bfloat16),
                ffn=torch.empty(M, self.ffn_dim, device=dev, dtype=torch.bfloat16) if not self._fp8_ffn else None,
                vt=None,  # V^T [dim, M rounded up to 64] of the single-GPU self-attention, allocated on first use
                attn8={},  # enable_fp8_attention(): ops.AttnMx8 operand buffers per segment table (_self_attn)
            )
            if self._fp8_ffn or self._fp8_qkv:  # a LayerNorm output as MXFP8 (the FFN's or the q/k/v Linears' input)
                ws.modq = ops.Mx8.empty(M, dim, dev)
            if self._fp8_ffn:  # the FFN's hidden activations as MXFP8
                ws.ffn = ops.Mx8.empty(M, self.ffn_dim, dev)
            if self._fp8_o:  # the self-attention output as MXFP8 (the O-projection's input)
                ws.attq = ops.Mx8.empty(M, dim, dev)
            self._ws = {key: ws}  # keep one shape at a time
        return ws

    def _vt_attention(self, Lp, dev) -> bool:
        """the single-GPU self-attention reads V as V^T written by the QKV GEMM's transposed epilogue (attention
        kernel 3: 6.20 vs 6.41 ms per config-2 launch, bit-identical, profiles/r05/attn_ab_v6_v6t_v12_r5b.jsonl)
        when the batch rows start on 32-key boundaries; SA_ATTN_VT=0 or an explicit attn_kernel keeps V in rows"""
        return (dev.type == "cuda" and self.attn_kernel == 0 and Lp % 32 == 0
                and os.environ.get("SA_ATTN_VT", "1") != "0")

    # ------------------------------------------------------------------ context (step-invariant)

    def invalidate_context(self):
        """drop the cached text / image K/V (the pipeline calls this at the start of every denoise)"""
        self._ctx_cache = None

    def _sp_exchange(self, plan, B, Lc, dev):
        """the sequence-parallel exchange buffers (attention inputs, send slabs, output / panel buffer, pack
        table, output row map) for this shape, kept across layers, steps and calls (one shape at a time)"""
        key = (plan, B, Lc, self.d, str(dev), id(self.sp_group), self._sp_loopback)
        ex = self._sp_ex
        if ex is None or ex[0] != key:
            self._sp_ex = None  # free the previous shape's buffers first
            ex = self._sp_ex = (key, sp.UlyssesExchange(plan, B, Lc, self.d, dev, self.sp_group,
                                                        loopback=self._sp_loopback))
        return ex[1]

    @staticmethod
    def _ctx_key(context, clip_fea):
        """(tensor, version) of every context input.  The cache holds the tensors themselves and matches
        by identity, so a hit cannot come from a new tensor the caching allocator placed at a freed
        address (an address key could return the previous call's prompt / image K/V)."""
        return tuple((c, c._version) for c in context) + (((clip_fea, clip_fea._version),)
                                                          if clip_fea is not None else ())

    def _context(self, pk, context, clip_fea, B, dev):
        key = self._ctx_key(context, clip_fea)
        if self._ctx_cache is not None:
            old = self._ctx_cache[0]
            if len(old) == len(key) and all(a is c and va == vc for (a, va), (c, vc) in zip(old, key)):
                return self._ctx_cache[1]
            self._ctx_cache = None  # release the previous call's tensors and K/V before building new ones
        dim, tl = self.dim, self.text_len
        # text: pad each prompt to text_len with zeros (the pads are attended, 1B:993-999)
        tin = torch.zeros(B, tl, pk.text_kpad, device=dev, dtype=torch.bfloat16)
        for b, c in enumerate(context):
            tin[b, :c.shape[0], :c.shape[1]] = c.to(device=dev, dtype=torch.bfloat16)
        h = ops.linear(tin.view(B * tl, pk.text_kpad), pk.w_t0, pk.b_t0, ops.EPI_GELU_TANH_BF16)
        ctx_t = ops.linear(h, pk.w_t2, pk.b_t2, ops.EPI_BF16)
        # image: MLPProj (1B:726-738): LN(1280) -> Linear -> GELU(erf) -> Linear -> LN(dim)
        ni = 0
        if self.model_type == "i2v":
            ni = clip_fea.shape[1]
            cf = clip_fea.to(device=dev, dtype=torch.float32).reshape(B * ni, -1).contiguous()
            cn = torch.empty(B * ni, cf.shape[1], device=dev, dtype=torch.bfloat16)
            ops.layernorm_mod(cf, cn, 1e-5, weight=pk.ie0w, bias=pk.ie0b)
            h1 = ops.linear(cn, pk.w_ie1, pk.b_ie1, ops.EPI_GELU_ERF_BF16)
            h3 = ops.linear(h1, pk.w_ie3, pk.b_ie3, ops.EPI_F32)
            ctx_i = torch.empty(B * ni, dim, device=dev, dtype=torch.bfloat16)
            ops.layernorm_mod(h3, ctx_i, 1e-5, weight=pk.ie4w, bias=pk.ie4b)
        kv = []
        for L in pk.layers:
            kvt = ops.linear(ctx_t, L.w_kv_t, L.b_kv_t, ops.EPI_BF16)      # [B*tl, 2dim] = k | v
            ops.qk_rmsnorm_rope(kvt, 0, -1, L.cnk, None, dim, self.eps)
            kvi = None
            if ni:
                kvi = ops.linear(ctx_i, L.w_kv_i, L.b_kv_i, ops.EPI_BF16)
                ops.qk_rmsnorm_rope(kvi, 0, -1, L.cnki, None, dim, self.eps)
            kv.append((kvt, kvi))
        out = SimpleNamespace(kv=kv, text_len=tl, img_len=ni)
        self._ctx_cache = (key, out)
        return out

    # ------------------------------------------------------------------ vocal projector

    def _vocal(self, pk, vocal_embeddings, n_frames, lat_bf16, Lq, e0_row, e_row, frames=None):
        """FantasyTalkingVocalCondition{1B,14B}Model.forward (vocal_projector_fantasy_1B.py:433-450,
        _14B.py:431-449) for one audio row; lat_bf16 = patch-embedded tokens of that row [Lq, dim].
        Returns [F*n, vd] bf16 (vd = 1536 for 1.3B, the DiT width for 14B).
        frames = (f0, nf): latent frames f0 .. f0+nf-1 only (lat_bf16 then holds just their tokens, and the result is
        [nf*n, vd]).  Every op of the projector is per row except the attention, whose queries of frame f attend only
        to frame f's tokens (:259-270), so these rows equal those of the whole projector bit for bit: a
        sequence-parallel rank computes the frames its token chunk covers."""
        V, vd, dev = pk.vocal, self.vd, lat_bf16.device
        hdv = vd // 8  # 8 heads: D = 192 (1.3B) or 640 (14B)
        feat = vocal_embeddings.to(device=dev, dtype=torch.bfloat16).contiguous()
        Na = feat.shape[0]
        for j, (w, nw, nb) in enumerate(V.proj):  # Linear (no bias) + LayerNorm, once or twice
            f = ops.linear(feat, w, None, ops.EPI_F32)
            last = j == len(V.proj) - 1
            feat = ops.layernorm_mod(f, f if last else torch.empty(Na, f.shape[1], device=dev, dtype=torch.bfloat16),
                                     1e-5, weight=nw, bias=nb)
        key = (Na, n_frames)
        rows = self._split_cache.get(key)
        if rows is None:
            r = split_rows(Na, n_frames)
            rows = (torch.tensor([i for row in r for i in row], dtype=torch.int32, device=dev), len(r), len(r[0]))
            self._split_cache[key] = rows
        idx, Fn, nper = rows
        f0, nf = (0, Fn) if frames is None else frames
        Mv = nf * nper
        x = torch.empty(Mv, vd, device=dev, dtype=torch.float32)
        ops.gather_rows(feat, idx[f0 * nper:(f0 + nf) * nper], x)
        em = torch.empty(2, 1, 6, vd, device=dev, dtype=torch.float32)
        ops.mod_add(V.mod, e0_row, em)
        hb = torch.empty(Mv, vd, device=dev, dtype=torch.bfloat16)
        G = Lq // Fn
        assert lat_bf16.shape[0] == nf * G
        segs = self._segs.get(("vp", nf, nper, G), [[f * nper, nper, f * G, G] for f in range(nf)], dev)
        for i, B_ in enumerate(V.blocks):
            e = em[i, 0]
            # "self-attention" branch is x + modulate(LN(x))*e2 (vocal_projector_fantasy_1B.py:345-347)
            ops.layernorm_mod(x, x, 1e-6, shift=e[0:1], scale=e[1:2], gate=e[2:3], rows_per_batch=Mv)
            ops.layernorm_mod(x, hb, 1e-6, weight=B_.n3w, bias=B_.n3b)
            q = ops.linear(hb, B_.w_q, B_.b_q, ops.EPI_BF16)
            ops.qk_rmsnorm_rope(q, 0, -1, B_.nq, None, vd, 1e-6)
            kv = ops.linear(lat_bf16, B_.w_kv, B_.b_kv, ops.EPI_BF16)
            ops.qk_rmsnorm_rope(kv, 0, -1, B_.nk, None, vd, 1e-6)
            o = torch.empty(Mv, vd, device=dev, dtype=torch.bfloat16)
            ops.attention_small(q, kv[:, :vd], kv[:, vd:], o, segs, nf, nper, G, 8, hdv)
            ops.linear(o, B_.w_o, B_.b_o, ops.EPI_RES_F32, out=x, residual=x)
            ops.layernorm_mod(x, hb, 1e-6, shift=e[3:4], scale=e[4:5], rows_per_batch=Mv)
            h = ops.linear(hb, B_.w_f0, B_.b_f0, ops.EPI_GELU_TANH_BF16)
            ops.linear(h, B_.w_f2, B_.b_f2, ops.EPI_RES_F32, out=x, residual=x, gate=e[5:6], rows_per_batch=Mv)
        ef = torch.empty(1, 1, 2, vd, device=dev, dtype=torch.float32)
        ops.mod_add(V.fmod, e_row, ef, e_jstride=0)
        ops.layernorm_mod(x, hb, 1e-6, shift=ef[0, 0, 0:1], scale=ef[0, 0, 1:2], rows_per_batch=Mv)
        return ops.linear(hb, V.w_fp, V.b_fp, ops.EPI_BF16), Fn, nper

    # ------------------------------------------------------------------ the steps of a DiT block
    # Each takes the forward's state f (forward_window), the layer's packed weights L, the layer's modulation em
    # [B, 6, dim] where it reads one, and a row selector b: None = all B CFG rows in one launch, b = CFG row b alone.
    # The selector resolves to R = f.all or f.row[b]: the rows' range, workspace views and tables (_plan_blocks).

    def _row_streams(self, B, dev):
        """B HIP streams (one per CFG row) for the SP_OVERLAP=4 layer schedule, kept per device"""
        st = self._rstreams
        if st is None or len(st) < B or st[0].device != dev:
            st = self._rstreams = [torch.cuda.Stream(dev) for _ in range(B)]
        return st[:B]

    @staticmethod
    def _sel(f, b, em=None):
        """row selector -> (the rows' views and tables R, their modulation [rows, 6, dim])"""
        if b is None:
            return f.all, em
        return f.row[b], None if em is None else em[b:b + 1]

    def _norm1(self, f, R, e):
        """norm1 + modulate (1B:675) of the rows R of the residual stream: bf16 ws.mod, or
        with enable_fp8_qkv() MXFP8 ws.modq (bf16 output followed by the quantiser, in one kernel)"""
        ln, out = (ops.layernorm_mod_mxfp8, R.modq) if self._fp8_qkv else (ops.layernorm_mod, R.mod)
        return ln(R.x, out, self.eps, shift=e[:, 0], scale=e[:, 1], rows_per_batch=f.Lc)

    def _qkv(self, f, L, R, e, normed=False):
        """The q|k|v Linears of a block's self-attention (1B:383-390) for the rows R of the residual stream: norm1 +
        modulate (unless `normed`: _norm1 already ran), then the fused QKV GEMM into their ws.qkv rows as bf16.  With
        enable_fp8_qkv() the LayerNorm writes MXFP8 and the GEMM runs on the block-scaled fp8 MFMA; off, exactly the
        bf16 calls."""
        if not normed:
            self._norm1(f, R, e)
        lin, mod = (ops.linear_mxfp8, R.modq) if self._fp8_qkv else (ops.linear, R.mod)
        return lin(mod, L.w_qkv, L.b_qkv, ops.EPI_BF16, out=R.qkv)

    def _sp_send_qkv(self, f, L, em, b, normed=False):
        """Self-attention inputs (1B:675-676) of the selected rows and their Q/K/V exchange (wan_xfuser.py:102-107): QKV
        GEMM, RMSNorm + RoPE packed into the send slabs / attention inputs, the transfers issued; returns the Pending"""
        R, e = self._sel(f, b, em)
        self._qkv(f, L, R, e, normed=normed)
        ops.qkv_pack(R.qkv, L.nq, L.nk, self.dim, self.eps, b_offset=R.rows.start, **f.pack_kw, **f.rope_kw)
        return f.ex.heads(R.rows)

    def _sp_attend(self, f, b, pend, kernel, split_tiles):
        """Ulysses: once the Q/K/V transfers `pend` have arrived, full-sequence attention of this rank's (query part,
        head group) for the selected rows, outputs written to the owners' send slabs / this rank's own O-projection
        panel, then heads -> tokens issued.  Returns the Pending."""
        for p_ in pend:
            p_.wait()
        R, ex = self._sel(f, b)[0], f.ex
        with self._span(rows=len(R.rows), batch=f.B):
            self._self_attn(f, ex.q, f.k, f.v, ex.obuf, R.self_attn, kernel=kernel, split_tiles=split_tiles)
        return ex.tokens(R.rows)

    def _o_proj(self, f, L, R, e, att):
        """The O-projection + gated residual (1B:677-679) of the rows R: bf16 `att` through the bf16 GEMM, or with
        enable_fp8_o() the MXFP8 GEMM on R.attq -- `att` quantised into it first, or att = None: it already holds the
        operand (the flash kernel, or _sp_o_proj's panels, wrote it)"""
        if not self._fp8_o:
            return ops.linear(att, L.w_o, L.b_o, ops.EPI_RES_F32, out=R.x, residual=R.x, gate=e[:, 2],
                              rows_per_batch=f.Lc)
        if att is not None:
            ops.mxfp8_quant(att, out=R.attq)
        return ops.linear_mxfp8(R.attq, L.w_o, L.b_o, ops.EPI_RES_F32, out=R.x, residual=R.x, gate=e[:, 2],
                                rows_per_batch=f.Lc)

    def _sp_o_proj(self, f, L, em, b, back):
        """the head outputs `back` of the selected rows received, their O-projection over the column panels +
        gated residual (1B:677-679).  With enable_fp8_o() each bf16 panel (whole heads) is quantised into its columns
        of R.attq -- the single-GPU operand's bytes -- and the MXFP8 GEMM reads that one matrix"""
        R, e = self._sel(f, b, em)
        back.wait()
        a0, pnl = f.ex.panels(R.rows)
        if not self._fp8_o:
            return ops.linear(a0, L.w_o, L.b_o, ops.EPI_RES_F32, out=R.x, residual=R.x, gate=e[:, 2],
                              rows_per_batch=f.Lc, a_panels=pnl)
        pc, ps = pnl
        for p in range(self.dim // pc):
            panel = a0.as_strided(a0.shape, a0.stride(), a0.storage_offset() + p * ps)
            ops.mxfp8_quant(panel, out=R.attq.cols(p * pc, (p + 1) * pc))
        self._o_proj(f, L, R, e, None)

    def _self_attention_rows(self, f, L, em, b=None, normed=False):
        """The self-attention half of a block (1B:675-679) on the single-GPU layout, for all CFG rows or row 0 (the
        shared first block): LN + modulate (unless `normed`), q|k (+ v as V^T for kernel 3, or q|k|v rows), RMSNorm +
        RoPE, attention, O-projection + gated residual into x.  With enable_fp8_qkv() and enable_fp8_attention() (and
        _fp8_qkv_fused) the fused chain: q|k GEMM, the V GEMM writing the V^T operand, RMSNorm + RoPE writing the Q
        operand, K means, K pack, the MXFP8 flash kernel.  With enable_fp8_o() and enable_fp8_attention() (and
        _fp8_o_fused) either flash launch writes the O-projection's MXFP8 operand instead of bf16 rows."""
        dim, H_, ws, Lc, Lp = self.dim, self.num_heads, f.ws, f.Lc, f.Lp
        R, e = self._sel(f, b, em)
        nb, segs, mod, qkv, att = len(R.rows), R.self_attn, R.mod, R.qkv, R.att
        o8 = self._fp8_o and self._fp8_attn and self._fp8_o_fused
        if o8:
            att = R.attq
        if not normed:
            self._norm1(f, R, e)
        if self._fp8_qkv and self._fp8_attn and self._fp8_qkv_fused:
            assert Lc == Lp and not f.use_vt
            vcol0, Rv, max_kv = self._segs.vt_layout(segs)
            key = (id(segs), nb * Lc, nb * Lc, H_)
            buf = ws.attn8.get(key)
            if buf is None:
                buf = ws.attn8[key] = ops.AttnMx8(nb * Lc, nb * Lc, H_, Rv, nb, f.dev)
            modq = R.modq
            ops.linear_mxfp8(modq, L.w_qk, L.b_qk, ops.EPI_BF16, out=qkv[:, :2 * dim])
            ops.linear_mxfp8_vt(modq, L.w_v, L.b_v, Lp, nb, buf)
            ops.qk_rmsnorm_rope_mxfp8(qkv, 0, dim, L.nq, L.nk, dim, self.eps, buf, **f.rope_kw)
            with self._span(rows=nb, batch=f.B):
                km = ops.attn_kmean(qkv[:, dim:2 * dim], segs, nb, H_, buf.kmean, buf.kmean_work)
                ops.attn_pack_k_mxfp8(qkv[:, dim:2 * dim], segs, nb, max_kv, H_, buf, km)
                ops.attn_fwd_mxfp8(buf, att, segs, vcol0, nb, Lp, H_)
        elif f.use_vt:
            # q|k into the QKV rows, v straight into V^T (keys in P's order per 32) for attention kernel 3
            ops.linear(mod, L.w_qk, L.b_qk, ops.EPI_BF16, out=qkv[:, :2 * dim])
            ops.linear(mod, L.w_v, L.b_v, ops.EPI_BF16_TP32, out=ws.vt)
            ops.qk_rmsnorm_rope(qkv, 0, dim, L.nq, L.nk, dim, self.eps, **f.rope_kw)
            with self._span(rows=nb, batch=f.B):
                if f.blocks is not None:
                    ops.attention(qkv[:, :dim], qkv[:, dim:2 * dim], ws.vt, att, segs, nb, Lp, H_,
                                  kernel=ops.ATTN_VT_P32, blocks=f.blocks)
                else:
                    ops.attention(qkv[:, :dim], qkv[:, dim:2 * dim], ws.vt, att, segs, nb, Lp, H_,
                                  kernel=ops.ATTN_VT_P32)
        else:
            self._qkv(f, L, R, e, normed=True)
            ops.qk_rmsnorm_rope(qkv, 0, dim, L.nq, L.nk, dim, self.eps, **f.rope_kw)
            with self._span(rows=nb, batch=f.B):
                self._self_attn(f, qkv[:, :dim], qkv[:, dim:2 * dim], qkv[:, 2 * dim:], att, segs,
                                kernel=self.attn_kernel)
        self._o_proj(f, L, R, e, None if o8 else att)

    def _cross_attention(self, f, L, b):
        """cross-attention of the selected rows: text + image + per-frame vocal (1B:534-605, 684), its output
        projection added to the residual stream.  A row alone reads its own rows of the text / image / vocal K|V
        (cross3), or the shared K|V through its own segment tables (the three launches)."""
        dim, H_, eps, ctx = self.dim, self.num_heads, self.eps, f.ctx
        R = self._sel(f, b)[0]
        nb, xr, mod, att = len(R.rows), R.x, R.mod, R.att
        ops.layernorm_mod(xr, mod, eps, weight=L.n3w, bias=L.n3b)
        qc = R.qkv[:, :dim]
        ops.linear(mod, L.w_cq, L.b_cq, ops.EPI_BF16, out=qc)
        ops.qk_rmsnorm_rope(qc, 0, -1, L.cnq, None, dim, eps)
        (kvt, kvi), kvv = ctx.kv[L.i], f.kvv[L.i]
        if f.use_cross3:  # text + image + vocal in one launch, bf16 sum as 1B:602
            if b is not None:
                tl, ni, nv = ctx.text_len, ctx.img_len, f.n_fr * f.nper
                kvt, kvi, kvv = kvt[b * tl:(b + 1) * tl], kvi[b * ni:(b + 1) * ni], kvv[b * nv:(b + 1) * nv]
            ops.attention_cross3(qc, kvt[:, :dim], kvt[:, dim:], ctx.text_len, kvi[:, :dim], kvi[:, dim:],
                                 ctx.img_len, kvv[:, :dim], kvv[:, dim:], f.nper, f.G, f.n_fr, att, nb, f.Lc, H_,
                                 tok_offset=f.rank * f.Lc)
        else:
            ops.attention(qc, kvt[:, :dim], kvt[:, dim:], att, R.txt, nb, f.Lc, H_)
            if kvi is not None:
                ops.attention(qc, kvi[:, :dim], kvi[:, dim:], att, R.img, nb, f.Lc, H_, accumulate=True)
            ops.attention(qc, kvv[:, :dim], kvv[:, dim:], att, R.voc, R.voc_n, R.voc_q, H_, accumulate=True)
        ops.linear(att, L.w_co, L.b_co, ops.EPI_RES_F32, out=xr, residual=xr)

    def _ffn(self, f, L, em, b):
        """The FFN third of a block (1B:687-691) on the selected rows of the residual stream: norm2 +
        modulate, ffn.0 + GELU, ffn.2 + gated residual into x.  With enable_fp8_ffn() the LayerNorm writes MXFP8,
        ffn.0's epilogue hands ffn.2 its operand as MXFP8 and both GEMMs run on the block-scaled fp8 MFMA."""
        R, e = self._sel(f, b, em)
        x, ffn, Lc = R.x, R.ffn, f.Lc
        if self._fp8_ffn:
            ln, lin, mod, gelu = ops.layernorm_mod_mxfp8, ops.linear_mxfp8, R.modq, ops.EPI_GELU_TANH_MXFP8
        else:
            ln, lin, mod, gelu = ops.layernorm_mod, ops.linear, R.mod, ops.EPI_GELU_TANH_BF16
        ln(x, mod, self.eps, shift=e[:, 3], scale=e[:, 4], rows_per_batch=Lc)
        lin(mod, L.w_f0, L.b_f0, gelu, out=ffn)
        lin(ffn, L.w_f2, L.b_f2, ops.EPI_RES_F32, out=x, residual=x, gate=e[:, 5], rows_per_batch=Lc)

    # ------------------------------------------------------------------ the schedules of a DiT block (1B:650-695)

    def _shared_first_block(self, f, L, em):
        """The first block's self-attention half (1B:675-679) for CFG row 0 alone -- under sequence parallelism through
        the Ulysses exchange (its Q/K/V and head outputs only, unsplit), on the current stream -- the residual stream
        then copied to rows 1..B-1: the CFG rows enter the block identical (shared_rows), every rank takes this path"""
        if f.ex is None:
            self._self_attention_rows(f, L, em, 0)
        else:
            back = self._sp_attend(f, 0, [self._sp_send_qkv(f, L, em, 0)], self.attn_kernel, 0)
            self._sp_o_proj(f, L, em, 0, back)
        x, Lc = f.ws.x, f.Lc
        for b in range(1, f.B):
            x[b * Lc:(b + 1) * Lc].copy_(x[:Lc])
        if f.schedule == SP_STREAMS:
            for st in f.streams:
                st.wait_stream(f.main)

    def _sp_self_attention(self, f, L, em):
        """The self-attention half of a block (norm1 done) under the one-stream Ulysses schedules."""
        # one exchange per direction for all rows, or per-row Q/K/V exchanges issued as each row's QKV GEMM + pack
        # lands (they travel under the later rows' GEMMs)
        sent = [None] if f.schedule == SP_BATCHED else range(f.B)
        pend = [self._sp_send_qkv(f, L, em, b, normed=True) for b in sent]
        if f.schedule == SP_ROWS:
            # Ulysses pipelined over the CFG rows: row b's attention waits only on its own exchange, and row b's output
            # exchange travels under the next rows' attention and the earlier rows' O-projections.  No launch is split
            back = [self._sp_attend(f, b, [pend[b]], self.attn_kernel, 0) for b in sent]
            for b in sent:
                self._sp_o_proj(f, L, em, b, back[b])
            return
        # one batched attention once all have arrived, its tiles past the last full round over the CUs as key halves
        split = (ops.attn_tail_split(0, f.B * f.hg * -(-f.Lq // 256), f.dev)
                 if self.attn_kernel == 0 and f.blocks is None else 0)
        self._sp_o_proj(f, L, em, None, self._sp_attend(f, None, pend, self.attn_kernel, split))

    def _sp_block_streams(self, f, L, em, sa):
        """One DiT block (1B:650-695) with Ulysses sequence parallelism, each CFG row on its own stream
        (SA_SP_OVERLAP=4): row b's Q/K/V exchange (wan_xfuser.py:102-107) travels while the other rows compute
        (their QKV GEMMs, attention, O-projection, cross-attention and FFN), and its head-output exchange travels
        under the other rows' attention and FFN.  The host issues the phases of the three rows interleaved
        (QKV+pack+send for every row, then attention+send back for every row, then the rest of the block), so the
        transport sees the same order of transfers on every rank.  Per-row kernels are the batched ones applied to
        row slices: the output is bit-identical to the batched schedule.  sa=False: the self-attention half already
        ran (_shared_first_block), the block starts at its cross-attention."""
        # the rows' attention launches run concurrently: the tiles past their last full round over the CUs (in the
        # last row's launch) run as key halves (ops.attn_tail_split), all rows on the 8-wave kernel then.  Not in
        # the fp8 attention mode: there the three concurrent launches measured 3 % slower with the last row's tail
        # split than without (profiles/r10/fp8_attn_split.jsonl), so its key split serves the batched launch alone
        n_row = f.hg * -(-f.Lq // 256)
        splits = [ops.attn_tail_split(b * n_row, n_row, f.dev)
                  if self.attn_kernel == 0 and not self._fp8_attn and f.blocks is None else 0 for b in range(f.B)]
        akern = 1 if any(splits) else self.attn_kernel
        pend, back = [], []
        for b, st in enumerate(f.streams if sa else []):  # self-attention inputs (1B:675-676) and the Q/K/V exchange
            with torch.cuda.stream(st):
                pend.append(self._sp_send_qkv(f, L, em, b))
        for b, st in enumerate(f.streams if sa else []):  # attention over every key, head outputs back to the owners
            with torch.cuda.stream(st):
                back.append(self._sp_attend(f, b, [pend[b]], akern, splits[b]))
        for b, st in enumerate(f.streams):  # O-projection + gated residual, cross-attention, FFN (1B:677-691)
            with torch.cuda.stream(st):
                if sa:
                    self._sp_o_proj(f, L, em, b, back[b])
                self._cross_attention(f, L, b)
                self._ffn(f, L, em, b)

    def _blocks(self, f, emod):
        """the layer loop (1B:650-695 for every block) in the forward's schedule"""
        streams = f.schedule == SP_STREAMS
        if streams:  # every CFG row through the whole layer on its own HIP stream; rows are independent
            for st in f.streams:
                st.wait_stream(f.main)
        for L in f.pk.layers:
            em = emod[L.i]  # [B, 6, dim]
            # the CFG rows enter the first block identical (shared_rows): its self-attention half for
            # row 0 only, then the residual stream copied to the other rows
            sa = not (L.i == 0 and f.dedup)
            if not sa:
                self._shared_first_block(f, L, em)
            if streams:
                self._sp_block_streams(f, L, em, sa)
                continue
            if sa:  # self-attention (1B:675-679)
                self._norm1(f, f.all, em)
                if f.ex is None:
                    self._self_attention_rows(f, L, em, normed=True)
                else:
                    self._sp_self_attention(f, L, em)
            self._cross_attention(f, L, None)
            self._ffn(f, L, em, None)  # FFN (1B:687-691)
        if streams:
            for st in f.streams:
                f.main.wait_stream(st)

    # ------------------------------------------------------------------ timing hooks (bench.py)

    @contextmanager
    def _span(self, rows, batch):
        """While self._events is a list: HIP events on the current stream (the one the attention kernel is launched
        on) around a self-attention launch, appended to it; `rows` of the `batch` CFG rows ran in the span."""
        if self._events is None:
            yield
            return
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        yield
        ev1.record()
        self._events.append((ev0, ev1, rows / batch))

    # ------------------------------------------------------------------ the parts of a forward

    def _patch_embed(self, f, lat, y, frame_offset, broadcast):
        """patch embedding (1B:972-983): im2col + GEMM, padding rows zero; with SP every rank embeds
        the whole sequence (the vocal projector reads it, 1B:1004-1009) and keeps its chunk (1B:1019).  Returns the
        whole sequence's embedding [B * Lp, dim] fp32 (without SP the residual stream itself)."""
        pk, ws, dev, B, Lp, Lc, dim = f.pk, f.ws, f.dev, f.B, f.Lp, f.Lc, self.dim
        Fw, Hh, Ww = f.fhw
        real = math.prod(f.grid)
        cols = torch.empty(B, Lp, pk.kpad, device=dev, dtype=torch.bfloat16)
        ops.patch_im2col(lat, y, B, Fw, Hh, Ww, cols, pk.kpad, Lp, x_frame_offset=frame_offset,
                         x_batch_broadcast=broadcast)
        xfull = ws.x if not self._sp_enabled else torch.empty(B * Lp, dim, device=dev, dtype=torch.float32)
        call_gemm_batched(cols, pk.w_pe, pk.b_pe, xfull, B, real, Lp, dim, pk.kpad)
        if real < Lp:
            for b in range(B):
                ops.fill_(xfull[b * Lp + real:(b + 1) * Lp], 0.0)
        if self._sp_enabled:
            ws.x.view(B, Lc, dim).copy_(xfull.view(B, Lp, dim)[:, f.rank * Lc:(f.rank + 1) * Lc])
        return xfull

    def _time_modulation(self, f, t):
        """time embedding (fp32, 1B:986-990).  Returns e [B, dim], e0 [B, 6, dim], the blocks' modulation
        [layers, B, 6, dim] and the head's [1, B, 2, dim]."""
        pk, dev, B, dim = f.pk, f.dev, f.B, self.dim
        tt = t.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if tt.numel() == 1:
            tt = tt.expand(B).contiguous()
        sin = torch.empty(B, self.freq_dim, device=dev, dtype=torch.float32)
        ops.timestep_embed(tt, self.freq_dim, sin)
        h1 = torch.empty(B, dim, device=dev, dtype=torch.float32)
        ops.small_linear_f32(sin, pk.w_te0, pk.b_te0, h1, act_out=1)
        e = torch.empty(B, dim, device=dev, dtype=torch.float32)
        ops.small_linear_f32(h1, pk.w_te2, pk.b_te2, e)
        e0 = torch.empty(B, 6 * dim, device=dev, dtype=torch.float32)
        ops.small_linear_f32(e, pk.w_tp, pk.b_tp, e0, act_in=1)
        e0 = e0.view(B, 6, dim)
        emod = torch.empty(self.num_layers, B, 6, dim, device=dev, dtype=torch.float32)
        ops.mod_add(pk.mod, e0, emod)
        hmod = torch.empty(1, B, 2, dim, device=dev, dtype=torch.float32)
        ops.mod_add(pk.head_mod, e, hmod, e_jstride=0)
        return e, e0, emod, hmod

    def _vocal_context(self, f, xfull, vocal_embeddings, n_video_frames, e0, e):
        """vocal context (1B:1004-1009) and every block's per-frame vocal K|V of it; sets f.n_fr, f.G (latent frames,
        tokens per frame), f.nper (context rows per frame) and f.kvv."""
        pk, dev, B, S, Lp, Lc, rank, dim = f.pk, f.dev, f.B, f.S, f.Lp, f.Lc, f.rank, self.dim
        n_fr = (n_video_frames - 1) // 4 + 1
        if S % n_fr:
            raise ValueError("seq_len must split evenly into latent frames for the per-frame audio attention")
        G = S // n_fr
        # the latent frames this rank's tokens belong to (SP pads past S join the last frame): the only vocal
        # context rows its cross-attention reads (sp.vocal_segments); without SP every frame
        if self._sp_enabled:
            t0, t1 = rank * Lc, min((rank + 1) * Lc, S)
            vf0 = min(t0 // G, n_fr - 1)
            vnf = min(max(t1 - 1, t0) // G, n_fr - 1) - vf0 + 1
        else:
            vf0, vnf = 0, n_fr
        lat_row = torch.empty(vnf * G, dim, device=dev, dtype=torch.bfloat16)
        if vocal_embeddings.shape[0] == 1 and B != 1:
            raise ValueError("a single audio row drives a batch of 1 (1B:1008-1009); CFG batches pass 3 rows")
        # 1.3B: the projector runs on the last (full-condition) row only, the unconditional row gets
        # zeros (1B:1004-1009); 14B: every row through the projector with its own audio (14B:1008)
        rows_v = B if (self.VOCAL == "14B" or vocal_embeddings.shape[0] == 1) else 1
        voc_rows = []
        for r in range(rows_v):
            src = B - 1 if rows_v == 1 else r
            ops.cast_bf16(xfull[src * Lp + vf0 * G:src * Lp + (vf0 + vnf) * G], lat_row)
            vv, Fn, nper = self._vocal(pk, vocal_embeddings[src], n_video_frames, lat_row, S, e0[src:src + 1],
                                       e[src:src + 1], frames=(vf0, vnf))
            if self.vd != dim:
                raise ValueError("vocal context width must equal the DiT width")
            voc_rows.append(vv)
        assert Fn == n_fr
        vr = slice(vf0 * nper, (vf0 + vnf) * nper)  # the computed frames' rows of each CFG row's context
        if rows_v == 1 and vnf == n_fr:
            vctx = torch.zeros(B, Fn * nper, dim, device=dev, dtype=torch.bfloat16)
            for b in range(1, B):
                vctx[b].copy_(voc_rows[0])
        elif vnf == n_fr:
            vctx = torch.stack(voc_rows)
        else:
            vctx = torch.zeros(B, Fn * nper, dim, device=dev, dtype=torch.bfloat16)
            for b in range(B):
                if rows_v == B or b >= 1:
                    vctx[b, vr].copy_(voc_rows[b if rows_v == B else 0])
        vctx = vctx.view(B * Fn * nper, dim)
        # per-frame vocal K|V of every block in one GEMM [B * n_fr * nper, layers * 2 * dim] (1B:575-578: the
        # block's k_vocal / v_vocal of the shared vocal context); under SP only the rows of the frames this rank's
        # queries read (the others are never read)
        kvv_all = torch.empty(B * n_fr * nper, pk.w_kv_v_all.shape[0], device=dev, dtype=torch.bfloat16)
        if vnf == n_fr:
            ops.linear(vctx, pk.w_kv_v_all, pk.b_kv_v_all, ops.EPI_BF16, out=kvv_all)
        else:
            for b in range(B):
                r0 = b * n_fr * nper + vf0 * nper
                ops.linear(vctx[r0:r0 + vnf * nper], pk.w_kv_v_all, pk.b_kv_v_all, ops.EPI_BF16,
                           out=kvv_all[r0:r0 + vnf * nper])
        f.n_fr, f.G, f.nper = n_fr, G, nper
        f.kvv = [kvv_all[:, 2 * dim * i:2 * dim * (i + 1)] for i in range(self.num_layers)]  # each block's k | v

    def _plan_blocks(self, f, shared):
        """The tables and the schedule of the layer loop.  Under sequence parallelism: the exchange (f.ex, f.omap,
        f.pack_kw, f.k, f.v; f.Lq, f.hg become this rank's query part and head group) and its schedule (f.schedule,
        with f.streams and f.main for the per-row streams).  f.all and f.row[b]: the workspace views of all CFG rows
        and of row b, with their segment tables (a row's where the schedule launches it alone); f.use_cross3,
        f.use_vt; f.dedup: the CFG rows are equal (`shared`) and the first block's self-attention half runs once."""
        dev, B, S, Lp, Lc, rank, ctx, n_fr, nper = f.dev, f.B, f.S, f.Lp, f.Lc, f.rank, f.ctx, f.n_fr, f.nper
        tl, ni, get, ws = ctx.text_len, ctx.img_len, self._segs.get, f.ws

        def views(rows):  # the workspace rows of the CFG rows `rows`, sliced once per forward
            rs = slice(rows.start * Lc, rows.stop * Lc)
            return SimpleNamespace(rows=rows, x=ws.x[rs], mod=ws.mod[rs], qkv=ws.qkv[rs], att=ws.att[rs],
                                   ffn=ws.ffn[rs], modq=ws.modq[rs] if hasattr(ws, "modq") else None,
                                   attq=ws.attq[rs] if hasattr(ws, "attq") else None)
        f.all, f.row = views(range(B)), [views(range(b, b + 1)) for b in range(B)]
        if self._sp_enabled:
            plan = sp.make_plan(f.NS, rank, self.num_heads)
            ex = f.ex = self._sp_exchange(plan, B, Lc, dev)
            f.Lq, f.hg, f.omap = plan.G * Lc, plan.hg, ex.omap
            f.k, f.v = ex.kv[:, :plan.hg * self.d], ex.kv[:, plan.hg * self.d:]
            f.pack_kw = dict(table=ex.table, G=plan.G, R=plan.R, my_part=plan.part)
            gpu = dev.type == "cuda"
            f.schedule = sp_schedule(os.environ.get("SA_SP_OVERLAP", "1"), B, -(-f.Lq // 256) * f.hg,
                                     ops._n_cu(dev) if gpu else 256, gpu)
            if f.schedule == SP_STREAMS:
                f.streams, f.main = self._row_streams(B, dev), torch.cuda.current_stream(dev)
        # shared rows: the single-GPU layout, or the one-stream and per-row-stream Ulysses schedules
        f.dedup = shared and B > 1 and f.schedule in (None, SP_BATCHED, SP_STREAMS)
        # self-attention keys: the S tokens of the single-GPU sequence (the SP pads past S are queries only, their
        # outputs are never read), so any degree reproduces the single-GPU forward
        Lq, self_rows = f.Lq, [[b * f.Lq, f.Lq, b * Lp, S] for b in range(B)]
        voc_list = sp.vocal_segments(B, S, Lc, rank, n_fr, nper)
        vars(f.all).update(self_attn=get(("self", B, Lp, Lq, S), self_rows, dev),
                           txt=get(("txt", B, Lc, tl), sp.local_segments(B, Lc, tl), dev),
                           img=get(("img", B, Lc, ni), sp.local_segments(B, Lc, ni), dev),
                           voc=get(("voc", B, S, Lc, rank, n_fr, nper), voc_list, dev),
                           voc_n=len(voc_list), voc_q=max(s_[1] for s_ in voc_list))
        for b, t in enumerate(f.row[:B if f.schedule in (SP_ROWS, SP_STREAMS) else int(f.dedup)]):
            t.self_attn = get(("self_row", b, Lp, Lq, S), self_rows[b:b + 1], dev)
            if f.schedule == SP_STREAMS:
                # the row's cross-attention tables (query rows relative to the row's chunk, key rows absolute in the
                # shared text / image / vocal K|V buffers) for the three-launch path
                vl = [[q0 - b * Lc, ql, k0, kl] for q0, ql, k0, kl in voc_list if b * Lc <= q0 < (b + 1) * Lc]
                t.txt = get(("rtxt", b, Lc, tl), [[0, Lc, b * tl, tl]], dev)
                t.img = get(("rimg", b, Lc, ni), [[0, Lc, b * ni, ni]], dev)
                t.voc = get(("rvoc", b, Lc, tuple(map(tuple, vl))), vl, dev)
                t.voc_n, t.voc_q = len(vl), max(s_[1] for s_ in vl)
        if self._sparse is not None:
            # the block lists of every self-attention launch of this forward: f.Lq queries -- under sequence parallelism
            # this rank's query part, tokens part * Lq onwards -- against the S keys of a row
            (Fw, Hg, Wg), (win, sink) = f.grid, self._sparse
            q0 = f.Lq * sp.make_plan(f.NS, rank, self.num_heads).part if self._sp_enabled else 0
            f.blocks = self._segs.blocks(
                ("blocks", Fw, Hg * Wg, Lq, S, win, sink, q0),
                lambda: sparse_attn.frame_window_table(Fw, Hg * Wg, Lq, S, win, sink, q_offset=q0), dev)
        f.use_cross3 = (ni > 0 and f.G % 256 == 0 and (rank * Lc) % 256 == 0 and (rank + 1) * Lc <= S
                        and os.environ.get("SA_CROSS3", "1") != "0")
        f.use_vt = not self._sp_enabled and not self._fp8_attn and not self._fp8_qkv and self._vt_attention(Lp, dev)
        if f.use_vt and f.ws.vt is None:
            # zero-filled once: the pad columns past B * Lp are read (as P = 0 keys) by a partial last block, which
            # stages a whole 64-key block: up to (B-1)*Lp + ceil64(Lp) <= ceil64(M) + 64 columns
            f.ws.vt = torch.zeros(self.dim, (f.ws.x.shape[0] + 63) // 64 * 64 + 64, device=dev, dtype=torch.bfloat16)

    def _head(self, f, hm, out):
        """head (1B:715-723) + unpatchify (1B:1161-1184)"""
        ws, B, Lc = f.ws, f.B, f.Lc
        Fw, Hh, Ww = f.fhw
        ops.layernorm_mod(ws.x, ws.mod, self.eps, shift=hm[:, 0], scale=hm[:, 1], rows_per_batch=Lc)
        ho = ops.linear(ws.mod, f.pk.w_head, f.pk.b_head, ops.EPI_BF16)
        if self._sp_enabled:  # every rank gets the whole prediction (1B:1150-1152)
            ho = sp.gather_tokens(ho, B, Lc, f.NS, self.sp_group)
        if out is None:
            out = torch.empty(B, self.out_dim, Fw, Hh, Ww, device=f.dev, dtype=torch.bfloat16)
        ops.unpatchify(ho, f.Lp, B, self.out_dim, Fw, Hh, Ww, out)
        return out

    # ------------------------------------------------------------------ forward

    def forward(self, x, t, context, seq_len, clip_fea=None, y=None, cond_flag=True, vocal_embeddings=None,
                is_clip_level_modeling=False, video_sample_n_frames=81):
        """1B:928-1159.  x, y: [B, C, F, H, W] tensors (or lists of [C, F, H, W]); context: list of
        [L_i, text_dim]; t: [B]; vocal_embeddings: [B, N_audio, 768].  Returns [B, out_dim, F, H, W]
        (bf16)."""
        if isinstance(x, (list, tuple)):
            x = torch.stack(list(x))
        if isinstance(y, (list, tuple)):
            y = torch.stack(list(y))
        return self.forward_window(x, 0, False, x.shape[0], t, context, seq_len, clip_fea, y, vocal_embeddings,
                                   video_sample_n_frames, is_clip_level_modeling, cond_flag=cond_flag)

    def forward_window(self, lat, frame_offset, broadcast, B, t, context, seq_len, clip_fea, y, vocal_embeddings,
                       video_sample_n_frames=81, is_clip_level_modeling=False, out=None, cond_flag=True,
                       shared_rows=False):
        """Forward on frames [frame_offset, frame_offset + Fw) of `lat` ([B|1, C, T, H, W]); with
        broadcast=True one latent row feeds all B CFG rows (the pipeline's torch.cat([latents]*3)).
        shared_rows=True (with broadcast): the caller guarantees the B rows of y are equal too, as the pipeline's
        CFG batch has them (y tripled at wan_inference_long_pipeline.py:693-700, x at :730, t expanded at :733) --
        then every row's input to the first block's self-attention half (patch embedding, time modulation) is the
        same, and that half (1B:675-679) runs for one row and is copied to the others: bit-identical output."""
        if is_clip_level_modeling:
            raise NotImplementedError("clip-level audio modeling is a training mode (1B:1011-1015)")
        if self.model_type == "i2v":
            assert clip_fea is not None and y is not None
        # the patch-embedding Conv3d runs under the pipeline's bf16 autocast (pipeline:738): bf16 operands
        if lat.dtype != torch.bfloat16:
            lat = lat.to(torch.bfloat16)
        if y is not None and y.dtype != torch.bfloat16:
            y = y.to(torch.bfloat16)
        pk = self._pack()
        dev, d = pk.w_pe.device, self.d
        Fw = y.shape[2] if y is not None else lat.shape[2] - frame_offset
        Hh, Ww = lat.shape[3], lat.shape[4]
        grid = (Fw, Hh // 2, Ww // 2)
        NS, rank = self.sp_world_size, self.sp_world_rank  # at NS = 1 the SP path has no transfer, the same kernels
        S = int(seq_len)  # the single-GPU sequence (1B:983): these keys are attended, SP's extra pads are not
        Lp = sp.padded_len(S, NS)
        assert math.prod(grid) <= S, "seq_len smaller than the token count"
        Lc = Lp // NS  # tokens of each CFG row held by this rank (all of them without SP)
        # the forward's state: what every step of every layer needs and no layer changes (_vocal_context adds the
        # vocal K|V and frame geometry, _plan_blocks the tables and the schedule); Lq, hg: the whole row's at first
        f = SimpleNamespace(
            pk=pk, ws=self._workspace(B * Lc, dev), dev=dev, B=B, S=S, Lp=Lp, Lc=Lc, NS=NS, rank=rank,
            fhw=(Fw, Hh, Ww), grid=grid,
            rope_kw=dict(rope=pk.rope, rows_per_batch=Lc, tok_offset=rank * Lc, grid=grid, head_dim=d,
                         n_frame_pairs=d // 2 - 2 * (d // 6), n_height_pairs=d // 6),
            ex=None, omap=None, schedule=None, Lq=Lp, hg=self.num_heads, blocks=None)

        xfull = self._patch_embed(f, lat, y, frame_offset, broadcast)
        e, e0, emod, hmod = self._time_modulation(f, t)
        f.ctx = self._context(pk, context, clip_fea, B, dev)
        # TeaCache (1B:1021-1044): optional, decided on e0 before any block work
        tc = self.teacache
        if tc is not None and not tc.decide(e0, cond_flag):  # 1B:1048-1050: reuse the last computed residual
            f.ws.x.add_(tc.residual(cond_flag, dev))
        else:
            x_in = f.ws.x.clone() if tc is not None else None
            self._vocal_context(f, xfull, vocal_embeddings, video_sample_n_frames, e0, e)
            self._plan_blocks(f, shared_rows and broadcast)
            self._blocks(f, emod)
            if tc is not None:  # 1B:1096-1099
                tc.store(f.ws.x - x_in, cond_flag)
                del x_in
        return self._head(f, hmod[0], out)


class WanTransformer3DFantasy14BModel(WanTransformer3DFantasyModel):
    """WanTransformer3DFantasy14BModel (wan_fantasy_transformer3d_14B.py:735-1178): the same DiT at the 14B
    widths (wan_civitai 14B: dim 5120, 40 heads, 40 layers, ffn 13824) with the 14B vocal projector
    (two-layer audio projection, width = dim, 8 heads of 640, run on every CFG row with its own audio,
    14B:1008).  The reference's forward has no video_sample_n_frames (its vocal path hard-codes 81 video /
    21 latent frames, 14B:1008-1010, vocal_projector_fantasy_14B.py:254), which is why its long pipeline
    cannot drive it; here forward also accepts the 1.3B keyword and requires 81."""

    VOCAL = "14B"

    def forward_window(self, lat, frame_offset, broadcast, B, t, context, seq_len, clip_fea, y, vocal_embeddings,
                       video_sample_n_frames=81, is_clip_level_modeling=False, out=None, cond_flag=True,
                       shared_rows=False):
        if video_sample_n_frames != 81:
            raise ValueError("the 14B vocal path is built for 81-frame windows (21 latent frames, 14B:1008-1010)")
        return super().forward_window(lat, frame_offset, broadcast, B, t, context, seq_len, clip_fea, y,
                                      vocal_embeddings, 81, is_clip_level_modeling, out=out, cond_flag=cond_flag,
                                      shared_rows=shared_rows)


def call_gemm_batched(cols, w, bias, xout, B, real, Lp, dim, kpad):
    """patch-embedding GEMM per batch row over its real tokens only (pads stay zero, 1B:983)."""
    from ._lib import call
    call("sa_gemm_bf16", cols.data_ptr(), kpad, Lp * kpad, w.data_ptr(), kpad, 0, bias.data_ptr(), xout.data_ptr(),
         dim, Lp * dim, real, dim, kpad, B, ops.EPI_F32, 0, 0, 0, 0, 0, 0, ops._stream())
