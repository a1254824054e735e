"""sa_gemm_mxfp8_ks's split K step (kstep=2) against the one-tile kernel's one-barrier step (kernel=1, kstep=1), byte for
byte: both add each accumulator's K-tiles in the same order with one MFMA per K-tile and run the same epilogue, so every
output byte and every scale byte must be equal.  The shapes are the smallest at which a two-deep, region-freed pipeline
can go wrong -- no K-tile t + 1, no K-tile t + 2, the first step that ends on a counted vmcnt, both ring parities at the
drain, clamped rows re-read by the early DMA, the raster's short last run, the DiT's 12- and 70-step tiles, more tiles
than CUs.  The buffers carry guard rows and columns: a store past M or N shows as a changed guard.  The helpers are those
of tests/test_gpu_mxfp8_persistent.py."""
import functools
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from stableavatar_amd import mxfp8, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, GELU, F32, RES, GELU_MX = (ops.EPI_BF16, ops.EPI_GELU_TANH_BF16, ops.EPI_F32, ops.EPI_RES_F32,
                                 ops.EPI_GELU_TANH_MXFP8)
ALL = [BF16, GELU, F32, RES, GELU_MX]
EPI_ID = {BF16: "bf16", GELU: "gelu", F32: "f32", RES: "res", GELU_MX: "gelu_mx"}
GUARD_ROWS, GUARD_COLS = 8, 32


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """seeded bf16 data quantised by the definition: activations with per-row magnitudes 2^-3 .. 2^3, weights ~ 0.05,
    a bias, a residual and one gate row per 100 rows (the widest use)"""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    a = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    aq, as_ = mxfp8.quantize(a)
    wq, ws = mxfp8.quantize(w)
    return dict(a=ops.Mx8(aq.to(DEV), as_.to(DEV)), w=ops.Mx8(wq.to(DEV), ws.to(DEV)),
                bias=(torch.randn(N, generator=g) * 0.5).to(DEV), res=torch.randn(M, N, generator=g).to(DEV),
                gate=torch.randn(-(-M // 100) + 1, N, generator=g).to(DEV))


def _launch(p, epi, kstep, rows_per_batch=100, in_place=False):
    """one launch of the one-tile kernel under the given K step into guarded buffers; returns the whole buffers (output
    bytes, and scale bytes for epilogue 8)"""
    M, N = p["a"].shape[0], p["w"].shape[0]
    if epi == GELU_MX:
        q = torch.full((M + GUARD_ROWS, N + GUARD_COLS), 0xA5, dtype=torch.uint8, device=DEV)
        s = torch.full((M + GUARD_ROWS, N // 32 + 4), 0xA5, dtype=torch.uint8, device=DEV)
        ops.linear_mxfp8(p["a"], p["w"], p["bias"], epi, out=ops.Mx8(q[:M, :N], s[:M, :N // 32]), kernel=1, kstep=kstep)
        bufs = (q, s)
    else:
        dt = torch.float32 if epi in (F32, RES) else torch.bfloat16
        c = torch.full((M + GUARD_ROWS, N + GUARD_COLS), -7.0, dtype=dt, device=DEV)
        kw = {}
        if epi == RES:
            res = p["res"]
            if in_place:  # the residual aliases C, as the DiT's FFN-down runs
                c[:M, :N] = res
                res = c[:M, :N]
            kw = dict(residual=res, gate=p["gate"], rows_per_batch=rows_per_batch)
        ops.linear_mxfp8(p["a"], p["w"], p["bias"], epi, out=c[:M, :N], kernel=1, kstep=kstep, **kw)
        bufs = (c,)
    torch.cuda.synchronize()
    return bufs


def _guards_intact(bufs, M, N, epi):
    c = bufs[0]
    fill = 0xA5 if epi == GELU_MX else -7.0
    ok = bool((c[M:] == fill).all() and (c[:, N:] == fill).all())
    if epi == GELU_MX:
        s = bufs[1]
        ok = ok and bool((s[M:] == fill).all() and (s[:, N // 32:] == fill).all())
    return ok


def _check(M, N, K, epi, rows_per_batch=100, in_place=False):
    p = _problem(M, N, K)
    ref = _launch(p, epi, 1, rows_per_batch, in_place)
    out = _launch(p, epi, 2, rows_per_batch, in_place)
    assert _guards_intact(ref, M, N, epi) and _guards_intact(out, M, N, epi)
    for r, o in zip(ref, out):  # the output; the scales too for epilogue 8
        assert torch.equal(r, o), (M, N, K, epi, int((r != o).sum()))
    # the launch wrote: no live element still holds the fill
    live = out[0][:M, :N]
    assert not bool((live == (0xA5 if epi == GELU_MX else -7.0)).all())


@pytest.mark.parametrize("epi", ALL, ids=EPI_ID.get)
@pytest.mark.parametrize("K", [128, 256, 384, 512, 640])
def test_one_tile_one_to_five_k_tiles(K, epi):
    """nk = 1 (no K-tile t + 1), 2 (no K-tile t + 2), 3 (the first step that ends on a counted vmcnt), 4 and 5 (both
    ring parities at the drain); the file's first test, so a mismatched barrier shows on the cheapest launch"""
    _check(256, 256, K, epi)


@pytest.mark.parametrize("epi", ALL, ids=EPI_ID.get)
@pytest.mark.parametrize("K", [256, 384])
def test_ragged_rows_and_columns(K, epi):
    """4 tiles, three of them ragged: rows and columns clamped on load and masked on store"""
    _check(300, 320 if epi == GELU_MX else 288, K, epi)


@pytest.mark.parametrize("epi", ALL, ids=EPI_ID.get)
@pytest.mark.parametrize("K", [256, 384])
def test_one_partly_live_tile(K, epi):
    """M = N = 64: three quarters of the tile's rows are the clamped last row, which the early DMA reads again"""
    _check(64, 64, K, epi)


@pytest.mark.parametrize("epi", ALL, ids=EPI_ID.get)
def test_six_tiles(epi):
    _check(768, 512, 384, epi)


@pytest.mark.parametrize("M,epi", [(1280, BF16), (1280, RES), (2560, BF16), (2560, RES)],
                         ids=["gm8_one_run", "gm4_4+1", "gm8_8+2", "gm4_4+4+2"])
def test_group_m_raster_short_last_run(M, epi):
    """the raster's runs of group_m tile rows (8, or 4 for the gated residual): 5 and 10 tile rows"""
    _check(M, 768, 128, epi)


def test_gate_rows_across_tiles_in_place():
    """gate per batch row with rows_per_batch = 200 (no tile multiple: a tile spans two gate rows), residual = C"""
    _check(600, 512, 256, RES, rows_per_batch=200, in_place=True)


@pytest.mark.parametrize("K,epi", [(1536, GELU), (1536, GELU_MX), (8960, RES)], ids=["12_gelu", "12_gelu_mx", "70_res"])
def test_dit_k_tile_counts(K, epi):
    """the DiT's K = 1536 (12 steps: q/k/v, FFN-up) and K = 8960 (70 steps: FFN-down)"""
    _check(512, 512, K, epi)


@pytest.mark.parametrize("epi", [GELU_MX, RES], ids=EPI_ID.get)
def test_more_tiles_than_cus(epi):
    """272 tiles: workgroups start and finish beside each other at every phase of the step"""
    assert 17 * 16 > ops._n_cu(torch.device(DEV))
    _check(4352, 4096, 256, epi, in_place=epi == RES)


def test_exact_integers():
    """operands whose products and sums are exact in fp32 (test_gpu_mxfp8.py's lane-map witness): the split step against
    the integer result itself, 4 tiles of 3 K-tiles"""
    from test_gpu_mxfp8 import _int_operand
    M, N, K = 512, 512, 384
    aq, as_, a8 = _int_operand(M, K, 1)
    wq, ws, w8 = _int_operand(N, K, 2)
    assert (a8.abs() @ w8.abs().T).max() < 2 ** 24  # every partial sum, in units of 2^-6
    ref = (a8 @ w8.T).double() / 64
    out = ops.linear_mxfp8(ops.Mx8(aq.to(DEV), as_.to(DEV)), ops.Mx8(wq.to(DEV), ws.to(DEV)), None, F32, kstep=2)
    assert torch.equal(out.double().cpu(), ref), (out.double().cpu() - ref).abs().max()


def test_dit_small_under_the_environment_switch(tmp_path):
    """DIT_SMALL "full" with the three fp8 modes on, SA_MXGEMM_KSTEP=2 in one fresh process and unset in another
    (the variable is read once per process): the outputs are equal byte for byte"""
    child = os.path.join(HERE, "mxgemm_child.py")
    procs, paths = [], []
    for name, val in (("default", None), ("split", "2")):
        env = {k: v for k, v in os.environ.items() if k not in ("SA_MXGEMM_KSTEP", "SA_MXGEMM_KERNEL")}
        if val is not None:
            env["SA_MXGEMM_KSTEP"] = val
        paths.append(str(tmp_path / f"{name}.pt"))
        procs.append(subprocess.Popen([sys.executable, child, paths[-1]], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    for p in procs:
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, log[-3000:]
    a, b = (torch.load(p) for p in paths)
    assert a.abs().max() > 0 and torch.isfinite(a).all()
    assert torch.equal(a, b)
