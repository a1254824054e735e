"""Shared by the MXFP8 GEMM kernel-against-kernel tests (test_gpu_mxfp8_persistent.py, test_gpu_mxfp8_kstep.py): the
seeded problem, one launch of a selected kernel into buffers that carry guard rows and columns, and the guard check."""
import functools

import torch

from stableavatar_amd import mxfp8, ops

DEV = "cuda"
BF16, GELU, F32, RES, GELU_MX = (ops.EPI_BF16, ops.EPI_GELU_TANH_BF16, ops.EPI_F32, ops.EPI_RES_F32,
                                 ops.EPI_GELU_TANH_MXFP8)
ALL = [BF16, GELU, F32, RES, GELU_MX]
EPI_ID = {BF16: "bf16", GELU: "gelu", F32: "f32", RES: "res", GELU_MX: "gelu_mx"}
GUARD_ROWS, GUARD_COLS = 8, 32


@functools.lru_cache(maxsize=None)
def problem(M, N, K):
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


def fill(epi):
    """what every element of a guarded buffer holds before the launch"""
    return 0xA5 if epi == GELU_MX else -7.0


def launch(p, epi, kernel, workgroups=0, kstep=0, rows_per_batch=100, in_place=False):
    """one launch of the selected kernel and K step into guarded buffers; returns the whole buffers (output bytes, and
    scale bytes for epilogue 8)"""
    M, N = p["a"].shape[0], p["w"].shape[0]
    sel = dict(kernel=kernel, workgroups=workgroups, kstep=kstep)
    if epi == GELU_MX:
        q = torch.full((M + GUARD_ROWS, N + GUARD_COLS), 0xA5, dtype=torch.uint8, device=DEV)
        s = torch.full((M + GUARD_ROWS, N // 32 + 4), 0xA5, dtype=torch.uint8, device=DEV)
        ops.linear_mxfp8(p["a"], p["w"], p["bias"], epi, out=ops.Mx8(q[:M, :N], s[:M, :N // 32]), **sel)
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
        ops.linear_mxfp8(p["a"], p["w"], p["bias"], epi, out=c[:M, :N], **sel, **kw)
        bufs = (c,)
    torch.cuda.synchronize()
    return bufs


def guards_intact(bufs, M, N, epi):
    c = bufs[0]
    ok = bool((c[M:] == fill(epi)).all() and (c[:, N:] == fill(epi)).all())
    if epi == GELU_MX:
        s = bufs[1]
        ok = ok and bool((s[M:] == fill(epi)).all() and (s[:, N // 32:] == fill(epi)).all())
    return ok
