"""sa_gemm_mxfp8_ex's persistent kernel (kernel=2) against the one-tile kernel (kernel=1), byte for byte: both add each
accumulator's K-tiles in the same order with one MFMA per K-tile and run the same epilogue, so every output byte and
every scale byte must be equal.  The shapes are the places a persistent loop can go wrong -- the seam between two tiles
of one workgroup with an even and an odd K-tile count (ring parity), uneven tile counts per workgroup, workgroups without
a tile, ragged tiles on either side of a seam, the raster's short last run, the gate's batch rows across a seam -- with
the grid capped at 1, 2, 3 workgroups so that a handful of tiles is enough.  The buffers carry guard rows and columns:
a store past M or N shows as a changed guard."""
import functools
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from mxgemm_util import ALL, BF16, DEV, EPI_ID, F32, GELU_MX, RES, guards_intact, launch, problem  # noqa: E402

from stableavatar_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _one_tile(M, N, K, epi, rows_per_batch=100, in_place=False):
    """the reference: the one-tile kernel's buffers, computed once per case and shared by the workgroup counts"""
    return launch(problem(M, N, K), epi, 1, 0, rows_per_batch=rows_per_batch, in_place=in_place)


def _check(M, N, K, epi, workgroups, rows_per_batch=100, in_place=False):
    ref = _one_tile(M, N, K, epi, rows_per_batch, in_place)
    out = launch(problem(M, N, K), epi, 2, workgroups, rows_per_batch=rows_per_batch, in_place=in_place)
    assert guards_intact(ref, M, N, epi) and guards_intact(out, M, N, epi)
    for r, o in zip(ref, out):  # the output; the scales too for epilogue 8
        assert torch.equal(r, o), (M, N, K, epi, workgroups, int((r != o).sum()))
    # the launch wrote: no live element still holds the fill
    live = out[0][:M, :N]
    assert not bool((live == (0xA5 if epi == GELU_MX else -7.0)).all())


@pytest.mark.parametrize("epi", ALL, ids=EPI_ID.get)
def test_one_tile_one_k_step(epi):
    """no ring turn, no seam"""
    _check(256, 256, 128, epi, 1)


@pytest.mark.parametrize("epi", ALL, ids=EPI_ID.get)
@pytest.mark.parametrize("workgroups", [1, 2])
@pytest.mark.parametrize("K", [256, 384])
def test_seam_even_and_odd_k_tiles(K, workgroups, epi):
    """6 tiles over 1 or 2 workgroups: with nk = 3 every second tile of a workgroup starts in ring stage 1"""
    _check(768, 512, K, epi, workgroups)


@pytest.mark.parametrize("epi", [BF16, RES], ids=EPI_ID.get)
def test_uneven_tiles_per_workgroup(epi):
    """6 tiles over 4 workgroups: 2, 2, 1, 1"""
    _check(768, 512, 384, epi, 4)


def test_more_workgroups_than_tiles():
    """2 tiles, a cap of 5: the grid is min(tiles, workgroups), nothing runs without a tile"""
    _check(256, 512, 256, BF16, 5)


@pytest.mark.parametrize("epi", ALL, ids=EPI_ID.get)
@pytest.mark.parametrize("workgroups", [1, 3])
def test_ragged_edges_around_a_seam(workgroups, epi):
    """4 tiles, three of them ragged: rows and columns clamped on load and masked on store, before and after a seam"""
    _check(300, 320 if epi == GELU_MX else 288, 256, epi, workgroups)


@pytest.mark.parametrize("M,epi", [(1280, BF16), (1280, RES), (2560, BF16)], ids=["gm8_one_run", "gm4_4+1", "gm8_8+2"])
def test_group_m_raster_short_last_run(M, epi):
    """the raster's runs of group_m tile rows.  group_m is not an argument of the entry point (8, or 4 for the gated
    residual): 5 tile rows are one short run under 8 and runs of 4 and 1 under 4, 10 tile rows are runs of 8 and 2"""
    _check(M, 768, 128, epi, 3)


def test_gate_rows_across_tiles_in_place():
    """gate per batch row with rows_per_batch = 200 (no tile multiple: a tile spans two gate rows), residual = C"""
    _check(600, 512, 256, RES, 2, rows_per_batch=200, in_place=True)


@pytest.mark.parametrize("epi", [GELU_MX, RES], ids=EPI_ID.get)
def test_default_grid_more_tiles_than_cus(epi):
    """workgroups = 0 (one per CU) with 272 tiles: the launch the DiT would make, seams included"""
    assert 17 * 16 > ops._n_cu(torch.device(DEV))
    _check(4352, 4096, 256, epi, 0, in_place=epi == RES)


def test_exact_integers_across_seams():
    """operands whose products and sums are exact in fp32 (test_gpu_mxfp8.py's lane-map witness): the persistent kernel
    against the integer result itself, 4 tiles of 3 K-tiles over 2 workgroups"""
    from test_gpu_mxfp8 import _int_operand
    M, N, K = 512, 512, 384
    aq, as_, a8 = _int_operand(M, K, 1)
    wq, ws, w8 = _int_operand(N, K, 2)
    assert (a8.abs() @ w8.abs().T).max() < 2 ** 24  # every partial sum, in units of 2^-6
    ref = (a8 @ w8.T).double() / 64
    out = ops.linear_mxfp8(ops.Mx8(aq.to(DEV), as_.to(DEV)), ops.Mx8(wq.to(DEV), ws.to(DEV)), None, F32, kernel=2,
                           workgroups=2)
    assert torch.equal(out.double().cpu(), ref), (out.double().cpu() - ref).abs().max()


def test_dit_small_under_the_environment_switch(tmp_path):
    """DIT_SMALL "full" with the three fp8 modes on, SA_MXGEMM_KERNEL=2 in one fresh process and unset in another
    (the variable is read once per process): the outputs are equal byte for byte"""
    child = os.path.join(HERE, "mxgemm_child.py")
    procs, paths = [], []
    for name, val in (("default", None), ("persistent", "2")):
        env = {k: v for k, v in os.environ.items() if k != "SA_MXGEMM_KERNEL"}
        if val is not None:
            env["SA_MXGEMM_KERNEL"] = val
        paths.append(str(tmp_path / f"{name}.pt"))
        procs.append(subprocess.Popen([sys.executable, child, paths[-1]], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    for p in procs:
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, log[-3000:]
    a, b = (torch.load(p) for p in paths)
    assert a.abs().max() > 0 and torch.isfinite(a).all()
    assert torch.equal(a, b)
