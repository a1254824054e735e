"""sa_gemm_mxfp8_ks without a GPU: the K-step selector's argument checks, its combinations with the kernel selector and
the grid cap, and every operand check of sa_gemm_mxfp8 re-driven through the _ks entry point under each step code -- all
before the first HIP call (rc 1 with no device)."""
import pytest

from stableavatar_amd import _lib

ONE = 256  # a non-null, 16-byte aligned host address: rejected before it is dereferenced


def _lib_or_skip():
    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    return _lib.lib()


def _gemm(L, A=ONE, As=ONE, W=ONE, Ws=ONE, C=ONE, Cs=ONE, M=64, N=64, K=128, epi=2, res=None, lda=None, ldas=None,
          ldc=None, gate=None, gstride=0, rpb=0, kernel=0, workgroups=0, kstep=0):
    lds = K // 32 if K >= 32 else 4
    return L.sa_gemm_mxfp8_ks(A, K if lda is None else lda, As, lds if ldas is None else ldas, W, K, Ws, lds, None, C,
                              N if ldc is None else ldc, Cs, N // 32 if N >= 32 else 1, M, N, K, epi, res, N, gate,
                              gstride, rpb, kernel, workgroups, kstep, None)


def test_entry_point_is_declared_and_bound():
    assert "sa_gemm_mxfp8_ks" in _lib.header_symbols()
    assert _lib.SIGNATURES["sa_gemm_mxfp8_ks"] == _lib.SIGNATURES["sa_gemm_mxfp8_ex"][:-1] + "ip"
    assert hasattr(_lib_or_skip(), "sa_gemm_mxfp8_ks")


# the selector checks are driven with operands that pass every other check (M = N = 64, K = 128, plain fp32 epilogue),
# so rc 1 here is the selector's answer: with no device the first HIP call would answer something else
@pytest.mark.parametrize("kstep", [3, -1, 100])
def test_unknown_kstep_is_rejected(kstep):
    L = _lib_or_skip()
    for kernel in (0, 1, 2):
        assert _gemm(L, kernel=kernel, kstep=kstep) == 1


def test_kstep_2_with_the_persistent_kernel_is_rejected():
    L = _lib_or_skip()
    assert _gemm(L, kernel=2, kstep=2) == 1
    assert _gemm(L, kernel=2, workgroups=3, kstep=2) == 1


@pytest.mark.parametrize("workgroups", [1, 256])
def test_kstep_2_with_a_grid_cap_is_rejected(workgroups):
    L = _lib_or_skip()
    for kernel in (0, 1):
        assert _gemm(L, kernel=kernel, workgroups=workgroups, kstep=2) == 1


@pytest.mark.parametrize("kernel", [3, -1, 4, 100])
@pytest.mark.parametrize("kstep", [0, 1, 2])
def test_unknown_kernel_is_rejected_under_every_kstep(kstep, kernel):
    L = _lib_or_skip()
    assert _gemm(L, kernel=kernel, kstep=kstep) == 1
    assert _gemm(L, kernel=1, workgroups=-1, kstep=kstep) == 1


@pytest.mark.parametrize("kstep,kernel,workgroups", [(0, 0, 0), (0, 2, 3), (1, 0, 0), (1, 1, 7), (1, 2, 0), (1, 2, 3),
                                                     (2, 0, 0), (2, 1, 0)])
def test_every_check_of_sa_gemm_mxfp8_holds_through_ks(kstep, kernel, workgroups):
    """tests/test_mxfp8_persistent_cpu.py's operand cases under every step code and the selections it may go with"""
    L = _lib_or_skip()
    kw = dict(kernel=kernel, workgroups=workgroups, kstep=kstep)
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


def test_ops_keyword_exists():
    import inspect

    from stableavatar_amd import ops
    p = inspect.signature(ops.linear_mxfp8).parameters
    assert p["kstep"].default == 0
    assert list(p)[-3:] == ["kernel", "workgroups", "kstep"]
