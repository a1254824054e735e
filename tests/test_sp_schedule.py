"""The sequence-parallel exchange schedule chosen for an SA_SP_OVERLAP value (transformer.sp_schedule), pinned to the
rule forward_window applied before the rule became a function: auto ("1") takes the per-row streams on a GPU with more
than one CFG row, else the per-row schedule when B serial per-row attention launches need no more rounds over the CUs
than the batched launch, else per-row exchanges with batched attention; the explicit values name themselves, and 3 / 4
fall back to the batched schedule with a single row."""
import pytest

from stableavatar_amd.transformer import SP_BATCHED, SP_ROWS, SP_ROWS_X, SP_STREAMS, sp_schedule

ANY = [(1, 256), (63, 256), (504, 256), (1000, 304)]  # (workgroups per row, CUs) where the rule ignores them


@pytest.mark.parametrize("wg_row,n_cu", ANY)
def test_auto_on_a_gpu(wg_row, n_cu):
    assert sp_schedule("1", 3, wg_row, n_cu, True) == SP_STREAMS
    assert sp_schedule("1", 1, wg_row, n_cu, True) == SP_ROWS


def test_auto_without_a_gpu_counts_rounds_over_the_cus():
    assert sp_schedule("1", 3, 504, 256, False) == SP_ROWS  # 3 * ceil(504 / 256) = 6 <= ceil(1512 / 256) = 6
    assert sp_schedule("1", 3, 63, 256, False) == SP_ROWS_X  # 3 * 1 > ceil(189 / 256) = 1


@pytest.mark.parametrize("wg_row,n_cu", ANY)
def test_explicit_values(wg_row, n_cu):
    for ov, want in (("0", SP_BATCHED), ("2", SP_ROWS), ("3", SP_ROWS_X), ("4", SP_STREAMS)):
        assert sp_schedule(ov, 3, wg_row, n_cu, True) == want
    assert sp_schedule("4", 1, wg_row, n_cu, True) == SP_BATCHED
    assert sp_schedule("3", 1, wg_row, n_cu, True) == SP_BATCHED


def test_schedules_are_distinct_names():
    assert len({SP_BATCHED, SP_ROWS, SP_ROWS_X, SP_STREAMS}) == 4
