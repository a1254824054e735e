"""sa_gemm_mxfp8_ks's split K step (kstep=2) against the one-tile kernel's one-barrier step (kernel=1, kstep=1), byte for
byte: both add each accumulator's K-tiles in the same order with one MFMA per K-tile and run the same epilogue, so every
output byte and every scale byte must be equal.  The shapes are the smallest at which a two-deep, region-freed pipeline
can go wrong -- no K-tile t + 1, no K-tile t + 2, the first step that ends on a counted vmcnt, both ring parities at the
drain, clamped rows re-read by the early DMA, the raster's short last run, the DiT's 12- and 70-step tiles, more tiles
than CUs.  The buffers carry guard rows and columns: a store past M or N shows as a changed guard.  The helpers are
tests/mxgemm_util.py's."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from mxgemm_util import ALL, BF16, DEV, EPI_ID, F32, GELU, GELU_MX, RES, guards_intact, launch, problem  # noqa: E402

from stableavatar_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(M, N, K, epi, rows_per_batch=100, in_place=False):
    p = problem(M, N, K)
    ref = launch(p, epi, 1, kstep=1, rows_per_batch=rows_per_batch, in_place=in_place)
    out = launch(p, epi, 1, kstep=2, rows_per_batch=rows_per_batch, in_place=in_place)
    assert guards_intact(ref, M, N, epi) and guards_intact(out, M, N, epi)
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
