"""The opt-in block-sparse self-attention on the CPU: the frame-window table against a brute-force evaluation of its
token rule, the validation, the C entry's argument checks, the enable / CLI plumbing, the two self-attention call sites
with the mode off and on (ops recorded, no kernel runs), and the distance between the masked and the plain oracle that
the GPU forward tests rely on."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sparse_attn_util as U  # noqa: E402

from stableavatar_amd import _lib, ops, sparse_attn  # noqa: E402
from stableavatar_amd.transformer import WanTransformer3DFantasyModel  # noqa: E402


# ------------------------------------------------------------------------------------------------ the generator

def token_rule(n_frames, tpf, q_len, kv_len, window, sink, q_offset=0):
    """query i sees key j iff |frame(i) - frame(j)| <= window or frame(j) < sink, evaluated for every pair"""
    fq = ((q_offset + torch.arange(q_len)) // tpf).clamp(max=n_frames - 1)[:, None]
    fk = (torch.arange(kv_len) // tpf).clamp(max=n_frames - 1)[None, :]
    return ((fq - fk).abs() <= window) | (fk < sink)


def block_rule(tok, q_len, kv_len):
    """tile (qb, kb) is seen iff any of its pairs passes the token rule -> the token mask of whole tiles"""
    out = torch.zeros_like(tok)
    for q0 in range(0, q_len, 256):
        for k0 in range(0, kv_len, 64):
            out[q0:q0 + 256, k0:k0 + 64] = bool(tok[q0:q0 + 256, k0:k0 + 64].any())
    return out


GRIDS = {
    # name: (n_frames, tokens_per_frame, q_len, kv_len, q_offset)
    "aligned": (3, 1024, 3072, 3072, 0),          # a frame = 4 query tiles = 16 key blocks
    "unaligned_240x416": (4, 390, 1560, 1560, 0),  # 15 x 26 tokens per frame: frames straddle tiles and blocks
    "ragged_kv": (4, 390, 1560, 1500, 0),          # keys end inside a block and inside the last frame
    "padded": (3, 100, 520, 520, 0),               # 220 pad tokens past the last frame count as its tokens
    "query_part": (4, 390, 780, 1560, 780),        # the second half of the queries (a sequence-parallel query part)
}


@pytest.mark.parametrize("sink", [0, 1, 2])
@pytest.mark.parametrize("window", [0, 1, 2, 4, 7])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_table_is_the_block_rule_of_the_token_rule(grid, window, sink):
    nf, tpf, ql, kl, q0 = GRIDS[grid]
    ptr, idx = sparse_attn.frame_window_table(nf, tpf, ql, kl, window, sink, q_offset=q0)
    assert ptr.dtype == idx.dtype == torch.int32 and ptr.numel() == -(-ql // 256) + 1
    tok = token_rule(nf, tpf, ql, kl, window, sink, q0)
    got = sparse_attn.expand(ptr, idx, ql, kl)
    assert torch.equal(got, block_rule(tok, ql, kl))
    assert (got | ~tok).all()  # the table never hides a pair the token rule admits
    if grid == "aligned":
        assert torch.equal(got, tok)  # whole frames per tile and block: the two rules coincide
    if window >= nf:
        assert idx.numel() == -(-ql // 256) * -(-kl // 64) and sparse_attn.density(ptr, idx, ql, kl) == 1.0
    if window == 0 and sink == 0 and grid == "aligned":
        assert sparse_attn.density(ptr, idx, ql, kl) == pytest.approx(1 / 3)


def test_table_rejects_bad_sizes():
    for bad in (dict(n_frames=0), dict(tokens_per_frame=0), dict(q_len=0), dict(window_frames=-1), dict(sink_frames=-1),
                dict(kv_len=-1)):
        kw = dict(n_frames=2, tokens_per_frame=64, q_len=128, kv_len=128, window_frames=0, sink_frames=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            sparse_attn.frame_window_table(**kw)


def _t(*xs):
    return torch.tensor(xs, dtype=torch.int32)


def test_validation_errors():
    ok = (_t(0, 2, 3), _t(0, 5, 6))  # 2 query tiles (q_len 300), 7 key blocks (kv_len 424)
    sparse_attn.validate(*ok, 300, 424)
    sparse_attn.validate(_t(0, 0, 0), torch.zeros(0, dtype=torch.int32), 300, 424)  # empty lists are a valid table
    sparse_attn.validate(_t(0, 0, 2), _t(3, 4), 300, 424)                            # an empty list before a full one
    bad = {
        "descending": (_t(0, 2, 3), _t(5, 0, 6)),
        "repeated": (_t(0, 2, 3), _t(5, 5, 6)),
        "past the last block": (_t(0, 2, 3), _t(0, 7, 6)),
        "negative": (_t(0, 2, 3), _t(-1, 5, 6)),
        "pointer falls": (_t(0, 3, 2), _t(0, 5, 6)),
        "pointer does not start at 0": (_t(1, 2, 3), _t(0, 5, 6)),
        "pointer does not end at len": (_t(0, 2, 4), _t(0, 5, 6)),
        "too few pointers": (_t(0, 3), _t(0, 5, 6)),
        "too many pointers": (_t(0, 1, 2, 3), _t(0, 5, 6)),
    }
    for what, (p, x) in bad.items():
        with pytest.raises(ValueError):
            sparse_attn.validate(p, x, 300, 424)
            pytest.fail(what)
    with pytest.raises(ValueError):
        sparse_attn.validate(ok[0].long(), ok[1], 300, 424)
    with pytest.raises(ValueError):
        sparse_attn.expand(_t(0, 2, 3), _t(5, 0, 6), 300, 424)
    # ascending across a list boundary is not required: tile 0 = {5, 6}, tile 1 = {0}
    sparse_attn.validate(_t(0, 2, 3), _t(5, 6, 0), 300, 424)


# ------------------------------------------------------------------------------------------------ the C entry

def test_abi_is_declared_bound_and_rejects_bad_arguments_without_gpu_work():
    assert "sa_attn_fwd_sparse" in _lib.header_symbols() and "sa_attn_fwd_sparse" in _lib.SIGNATURES
    L = _lib.lib()
    one = 256  # a non-null, 16-byte aligned host address: rejected before it is dereferenced

    def fwd(q=one, k=one, v=one, o=one, segs=one, max_q=300, hd=128, vs=128, kernel=1, ptr=one, idx=one, nqb=2):
        return L.sa_attn_fwd_sparse(q, k, v, o, segs, 1, max_q, 2, hd, 256, 256, vs, 256, 1.0, 0, kernel, None, ptr, idx,
                                    nqb, None)

    for name in ("q", "k", "v", "o", "segs", "ptr", "idx"):
        assert fwd(**{name: None}) == 1, name
    assert fwd(ptr=258) == 1 and fwd(idx=257) == 1            # int32 tables on 4-byte boundaries
    assert fwd(nqb=1) == 1 and fwd(nqb=3) == 1 and fwd(max_q=512, nqb=3) == 1  # ceil(max_q_len / 256) exactly
    for kern in (2, 4, -1):                                   # 0, 1 and 3 only
        assert fwd(kernel=kern) == 1, kern
    assert fwd(hd=64) == 1 and fwd(q=264) == 1
    assert fwd(kernel=3, vs=96) == 1 and fwd(kernel=3, v=320) == 1  # kernel 3's V^T rows: whole 64-key blocks


# ------------------------------------------------------------------------------------------------ the plumbing

def _model(**kw):
    cfg = dict(dim=256, ffn_dim=256, num_heads=2, num_layers=1, text_dim=64, freq_dim=64, text_len=8)
    cfg.update(kw)
    return WanTransformer3DFantasyModel(**cfg)


def test_enable_validates_and_refuses_fp8_attention_either_way():
    m = _model()
    assert m._sparse is None
    m.enable_sparse_attention(2)
    assert m._sparse == (2, 1)
    m.enable_sparse_attention(0, sink_frames=0)
    assert m._sparse == (0, 0)
    with pytest.raises(ValueError):
        m.enable_sparse_attention(-1)
    with pytest.raises(NotImplementedError):
        m.enable_fp8_attention()          # the mode is on: fp8 attention cannot join it
    assert not m._fp8_attn
    m.enable_sparse_attention(3, enabled=False)
    assert m._sparse is None
    m.enable_fp8_attention()
    with pytest.raises(NotImplementedError):
        m.enable_sparse_attention(1)      # fp8 attention is on: raises at enable time
    assert m._sparse is None
    m.enable_sparse_attention(1, enabled=False)  # turning it off is always accepted
    m.enable_fp8_attention(False)
    for ffn in (False, True):             # the other fp8 modes combine
        m.enable_fp8_ffn(ffn), m.enable_fp8_qkv(ffn), m.enable_fp8_o(ffn), m.enable_sparse_attention(1)
        assert m._sparse == (1, 1)


def test_cli_flags_parse_and_default_to_off():
    from stableavatar_amd.inference import parse_args
    base = ["--pretrained_model_name_or_path", "ckpt"]
    a = parse_args(base)
    assert a.attn_window_frames is None and a.attn_sink_frames == 1
    a = parse_args(base + ["--attn_window_frames", "2"])
    assert a.attn_window_frames == 2 and a.attn_sink_frames == 1
    a = parse_args(base + ["--attn_window_frames", "0", "--attn_sink_frames", "3"])
    assert a.attn_window_frames == 0 and a.attn_sink_frames == 3


def test_ops_attention_refuses_blocks_with_a_key_split_or_the_4_wave_kernel():
    z = torch.zeros(4, 128, dtype=torch.bfloat16)  # the refusal precedes every use of the tensors
    blocks = (_t(0, 1), _t(0))
    for kw in (dict(split_tiles=1), dict(kernel=2), dict(kernel=4)):
        with pytest.raises(ValueError, match="block list"):
            ops.attention(z, z, z, z, z, 1, 4, 1, blocks=blocks, **kw)


class _Recorder:
    """stands in for the ops functions the self-attention half of a block calls; keeps (name, kwargs) per call"""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("linear", "qk_rmsnorm_rope", "layernorm_mod", "attention"):
            monkeypatch.setattr(ops, name, self._rec(name))

    def _rec(self, name):
        def f(*a, **kw):
            self.calls.append((name, len(a), kw))
        return f

    def attention(self):
        return [(n, kw) for name, n, kw in self.calls if name == "attention"]


def _state(use_vt, blocks):
    buf = torch.zeros(8, 768, dtype=torch.bfloat16)
    R = SimpleNamespace(rows=range(1), self_attn=torch.zeros(1, 4, dtype=torch.int32), mod=buf, qkv=buf, att=buf, x=buf,
                        modq=None, attq=None)
    f = SimpleNamespace(ws=SimpleNamespace(vt=buf), Lc=8, Lp=8, Lq=8, hg=2, B=1, omap="omap", all=R, row=[R],
                        use_vt=use_vt, blocks=blocks, rope_kw={}, dev="cpu")
    L = SimpleNamespace(**{n: None for n in ("w_qk", "b_qk", "w_v", "b_v", "w_qkv", "b_qkv", "nq", "nk", "w_o", "b_o")})
    return f, L, torch.zeros(1, 6, 256)


@pytest.mark.parametrize("use_vt", [True, False])
def test_mode_off_makes_the_attention_call_made_before_the_mode_existed(use_vt, monkeypatch):
    """the two bf16 self-attention sites, ops recorded: with the mode off (never on, or on and off again) the
    ops.attention call is the parent's -- 8 positional arguments, kernel 3 at the V^T site; kernel, o_rows and
    split_tiles at _self_attn -- with no `blocks` keyword; on, the same call plus blocks"""
    m = _model()
    rec = _Recorder(monkeypatch)
    want = {"kernel": ops.ATTN_VT_P32} if use_vt else {"kernel": 0, "o_rows": "omap", "split_tiles": 0}
    for toggle in (False, True):
        if toggle:
            m.enable_sparse_attention(1)
            m.enable_sparse_attention(1, enabled=False)
        rec.calls.clear()
        f, L, em = _state(use_vt, None)
        m._self_attention_rows(f, L, em, None, normed=True)
        assert rec.attention() == [(8, want)], rec.attention()
        names = [c[0] for c in rec.calls]
        assert names == (["linear", "linear", "qk_rmsnorm_rope", "attention", "linear"] if use_vt else
                         ["linear", "qk_rmsnorm_rope", "attention", "linear"])
    rec.calls.clear()
    f, L, em = _state(use_vt, "the table")
    m._self_attention_rows(f, L, em, None, normed=True)
    assert rec.attention() == [(8, dict(want, blocks="the table"))]


def test_sequence_parallel_site_passes_no_key_split_with_the_mode_on(monkeypatch):
    m = _model()
    rec = _Recorder(monkeypatch)
    f, _, _ = _state(False, None)
    seg = f.all.self_attn
    m._self_attn(f, seg, seg, seg, seg, seg, kernel=1, split_tiles=5)
    assert rec.attention() == [(8, {"kernel": 1, "o_rows": "omap", "split_tiles": 5})]
    rec.calls.clear()
    f.blocks = "the table"
    m._self_attn(f, seg, seg, seg, seg, seg, kernel=1, split_tiles=0)
    assert rec.attention() == [(8, {"kernel": 1, "o_rows": "omap", "split_tiles": 0, "blocks": "the table"})]


# ------------------------------------------------------------------------------------------------ the oracle

@pytest.mark.parametrize("case", ["full", "short"])
def test_golden_grids_list_every_block_at_any_window(case):
    """DIT_SMALL's golden grids have 16 tokens per frame and 80 tokens: one query tile whose frames reach into both
    key blocks, so under the block rule every window -- 0 included -- lists every block, and the masked oracle is the
    plain oracle.  The GPU forward tests on these grids therefore check the sparse launch path against a dense
    function; the grid below is the one that tells a masked forward from an unmasked one."""
    _, inp, plain = U.small_case(case)
    S = inp["seq_len"]
    for w in (1, 0):
        ptr, idx = U.table_for(inp, w)
        assert sparse_attn.density(ptr, idx, S, S) == 1.0
        assert sparse_attn.expand(ptr, idx, S, S).all()
    _, _, emu = U.small_case(case, 1)
    assert U.rel(emu, plain) < 1e-6


@pytest.mark.parametrize("window", [1, 0])
def test_masked_oracle_leaves_the_forward_bar_on_the_tall_grid(window):
    """64 tokens per frame, 5 frames, sharper scores: the table drops 2 (window 1) or 4 (window 0) of 10 tiles and the
    masked oracle stands outside the forward bar (rel-L2 < 2e-2 and cosine > 0.9995) around the plain oracle -- by
    1.5 times the rel-L2 bar at least, the dense HIP forward itself being 0.5e-2 from the plain oracle -- so the GPU
    forward test cannot pass with the table ignored"""
    _, inp, plain = U.small_case(U.TALL, None, 1, True)
    _, _, emu = U.small_case(U.TALL, window, 1, True)
    S = inp["seq_len"]
    ptr, idx = U.table_for(inp, window)
    assert ptr.tolist() == ([0, 5, 8] if window else [0, 4, 6])
    assert idx.tolist() == ([0, 1, 2, 3, 4, 0, 3, 4] if window else [0, 1, 2, 3, 0, 4])
    r, c = U.rel(emu, plain), U.cos(emu, plain)
    print(f"tall, window {window}: density {sparse_attn.density(ptr, idx, S, S):.2f}, masked vs plain oracle rel-L2 "
          f"{r:.3e} cosine {c:.6f}")
    assert r > 3e-2 and c < 0.9995, (r, c)
