"""sa_gemm_mxfp8_ex without a GPU: the kernel selector's and the grid cap's argument checks, and every check of
sa_gemm_mxfp8 re-driven through the _ex entry point under each kernel code -- all before the first HIP call (rc 1 with
no device)."""
import pytest

from stableavatar_amd import _lib

ONE = 256  # a non-null, 16-byte aligned host address: rejected before it is dereferenced


def _lib_or_skip():
    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    return _lib.lib()


def _gemm(L, A=ONE, As=ONE, W=ONE, Ws=ONE, C=ONE, Cs=ONE, M=64, N=64, K=128, epi=2, res=None, lda=None, ldas=None,
          ldc=None, gate=None, gstride=0, rpb=0, kernel=0, workgroups=0):
    lds = K // 32 if K >= 32 else 4
    return L.sa_gemm_mxfp8_ex(A, K if lda is None else lda, As, lds if ldas is None else ldas, W, K, Ws, lds, None, C,
                              N if ldc is None else ldc, Cs, N // 32 if N >= 32 else 1, M, N, K, epi, res, N, gate,
                              gstride, rpb, kernel, workgroups, None)


def test_entry_point_is_declared_and_bound():
    assert "sa_gemm_mxfp8_ex" in _lib.header_symbols()
    assert _lib.SIGNATURES["sa_gemm_mxfp8_ex"] == _lib.SIGNATURES["sa_gemm_mxfp8"][:-1] + "iip"


# (kernel, workgroups, bad): valid selector values must get past the selector check to the operand checks (driven here
# with a null A, still rc 1), so the table also pins which values are *not* what is being rejected
@pytest.mark.parametrize("kernel", [3, -1, 4, 100])
def test_unknown_kernel_is_rejected(kernel):
    L = _lib_or_skip()
    for wg in (0, 1, 256):
        assert _gemm(L, kernel=kernel, workgroups=wg) == 1


@pytest.mark.parametrize("kernel", [0, 1, 2])
@pytest.mark.parametrize("workgroups", [-1, -256, -2 ** 31])
def test_negative_workgroups_is_rejected(kernel, workgroups):
    L = _lib_or_skip()
    assert _gemm(L, kernel=kernel, workgroups=workgroups) == 1


@pytest.mark.parametrize("kernel,workgroups", [(0, 0), (1, 0), (2, 0), (2, 3), (1, 7)])
def test_every_check_of_sa_gemm_mxfp8_holds_through_ex(kernel, workgroups):
    """tests/test_mxfp8_cpu.py's cases, and the remaining operand checks of the entry point"""
    L = _lib_or_skip()
    kw = dict(kernel=kernel, workgroups=workgroups)
    for null in ("A", "As", "W", "Ws", "C"):
        assert _gemm(L, **{null: None}, **kw) == 1
    assert _gemm(L, K=192, **kw) == 1                   # K % 128
    assert _gemm(L, K=0, **kw) == 1 and _gemm(L, M=0, **kw) == 1 and _gemm(L, N=0, **kw) == 1
    assert _gemm(L, epi=8, N=48, **kw) == 1             # SA_EPI_GELU_TANH_MXFP8 with N % 32 != 0
    assert _gemm(L, epi=8, Cs=None, **kw) == 1
    assert _gemm(L, epi=3, **kw) == 1                   # gated residual without a residual
    assert _gemm(L, epi=3, res=ONE + 4, **kw) == 1      # residual not 16-byte aligned
    assert _gemm(L, epi=3, res=ONE, gate=ONE, rpb=0, **kw) == 1          # a gate needs rows_per_batch
    assert _gemm(L, epi=3, res=ONE, gate=ONE + 4, rpb=8, **kw) == 1      # gate alignment
    assert _gemm(L, epi=3, res=ONE, gate=ONE, gstride=6, rpb=8, **kw) == 1
    for epi in (4, 5, 6, 7, 9, -1):                     # epilogues this GEMM does not have, unknown codes
        assert _gemm(L, epi=epi, **kw) == 1
    assert _gemm(L, A=ONE + 8, **kw) == 1 and _gemm(L, W=ONE + 8, **kw) == 1     # operand alignment
    assert _gemm(L, As=ONE + 2, **kw) == 1              # scale rows are read a dword at a time
    assert _gemm(L, lda=120, **kw) == 1 and _gemm(L, lda=136, **kw) == 1         # lda < K, lda % 16
    assert _gemm(L, ldas=6, **kw) == 1                  # ldas % 4
    assert _gemm(L, ldc=62, **kw) == 1 and _gemm(L, ldc=66, **kw) == 1           # ldc < N, ldc % 4
    assert _gemm(L, C=ONE + 8, **kw) == 1
    assert _gemm(L, M=2 ** 24, K=128, **kw) == 1        # M * lda past the kernel's 32-bit offsets


def test_sa_gemm_mxfp8_still_rejects():
    """the plain entry point stays in the ABI and forwards: its own checks answer as before"""
    L = _lib_or_skip()
    assert L.sa_gemm_mxfp8(None, 128, ONE, 4, ONE, 128, ONE, 4, None, ONE, 64, ONE, 2, 64, 64, 128, 2, None, 64, None,
                           0, 0, None) == 1
    assert L.sa_gemm_mxfp8(ONE, 192, ONE, 6, ONE, 192, ONE, 6, None, ONE, 64, ONE, 2, 64, 64, 192, 2, None, 64, None,
                           0, 0, None) == 1


def test_ops_keywords_exist():
    import inspect

    from stableavatar_amd import ops
    p = inspect.signature(ops.linear_mxfp8).parameters
    assert p["kernel"].default == 0 and p["workgroups"].default == 0
