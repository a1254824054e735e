"""Kernel micro-benchmarks at the config-2 (512x512x81f, CFG batch 3) shapes of the DiT.
python -m stableavatar_amd.kbench  -> one JSON line per kernel with TFLOP/s (random data).
Selectors: gemm, attn, gemmvar, attnvar, dit, ditvar, ...; gemmfp8 = the fp8 FFN mode's LayerNorm / ffn_up / ffn_down
against the bf16 kernels, ditfp8 = the whole forward with the mode off and on; attnfp8 = the config-2 self-attention
launch, bf16 against the fp8 attention mode's three kernels, ditfp8attn = the whole forward with that mode off, on, and
on together with the fp8 FFN; qkvfp8 = the self-attention's operand chain (LayerNorm .. operands ready) in bf16, with the
fp8 q/k/v mode unfused and fused, ditfp8qkv = the whole forward off / attn+ffn / attn+ffn+qkv unfused / fused;
ofp8 = the MXFP8 flash kernel + the self-attention O-projection in bf16 and with the fp8 self-O mode unfused and fused,
ditfp8o = the whole forward off / the three modes / the three + fp8 self-O unfused / fused;
attnfp8split = the Ulysses N = 8 rank's self-attention launch unsplit against its key-split launch, fp8 and bf16;
unipc = sa_unipc_step beside sa_flow_step at config 2's latent shape;
attnsparse = the config-2 self-attention launch on dense kernel 3, on sa_attn_fwd_sparse with every block listed and
with frame windows of a few widths (each table's density beside its time), ditsparse = the whole forward with
enable_sparse_attention() off and on at those windows.
gemmfp8 and qkvfp8 also time sa_gemm_mxfp8_ks's one-tile kernel (the baseline arm) against its persistent kernel and
against the one-tile kernel with the split K step (kstep=2) on their GEMM shapes, and ditfp8qkv has
variants that run every MXFP8 GEMM of the forward on the persistent kernel and on the one-barrier K step."""
from __future__ import annotations

import json
import sys

import torch

from . import ops


def _time(fn, iters=10, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def vt_layout(v, mode, rows_pad=64):
    """V^T in the layout self-attention kernels 3 / 4 read (sa_attn_fwd_map): [H*128, Rv] bf16, row h*128 + d = d of
    head h for every key row (rows padded with zeros to a multiple of rows_pad).  mode 3: the keys of each 32-key
    chunk in P's permuted order (position 8g + j <- key 4g + j for j < 4, 16 + 4g + j - 4 for j >= 4); mode 4: natural
    order.  Built by torch (tests / A-B only; the DiT's QKV GEMM writes it itself)."""
    R, HD = v.shape
    Rv = (R + rows_pad - 1) // rows_pad * rows_pad + 64  # + one 64-key block: a ragged last block stages all 64
    vt = torch.zeros(HD, Rv, device=v.device, dtype=v.dtype)
    vt[:, :R] = v.t()
    if mode == 3:
        p = torch.arange(32, device=v.device)
        perm = torch.where(p % 8 < 4, 4 * (p // 8) + p % 8, 16 + 4 * (p // 8) + p % 8 - 4)
        idx = (torch.arange(Rv, device=v.device) // 32) * 32 + perm[torch.arange(Rv, device=v.device) % 32]
        vt = vt[:, idx].contiguous()
    return vt


def main(which=("gemm", "attn")):
    dev = "cuda"
    torch.manual_seed(0)
    M = 3 * 21504
    res = []
    if "gemmvar" in which:  # A/B of the GEMM kernels in one process (rule: interleaved rounds)
        import os
        # spec "K" or "K:G": K = kernel (0 auto, 1 ping-pong, 2 persistent), G = tile-raster group_m
        gvars = tuple(os.environ.get("SA_KB_GVARS", "1,2").split(","))
        for (Mx, N, K, epi, name) in [(M, 4608, 1536, ops.EPI_BF16, "qkv"), (M, 1536, 1536, ops.EPI_RES_F32, "o_proj"),
                                      (M, 1536, 1536, ops.EPI_BF16, "cross_q"),
                                      (M, 8960, 1536, ops.EPI_GELU_TANH_BF16, "ffn_up"),
                                      (M, 1536, 8960, ops.EPI_RES_F32, "ffn_down"),
                                      (M, 1536, 8960, ops.EPI_BF16, "ffn_down_bf16"),
                                      (M, 1536, 1536, ops.EPI_BF16_TP32, "v_t"),
                                      (8192, 8192, 8192, ops.EPI_BF16, "sq8192")]:
            if os.environ.get("SA_KB_SHAPES") and name not in os.environ["SA_KB_SHAPES"].split(","):
                continue
            x = (torch.rand(Mx, K, device=dev) * 2 - 1).bfloat16()
            w = ((torch.rand(N, K, device=dev) * 2 - 1) / K ** 0.5).bfloat16()
            b = torch.randn(N, device=dev)
            if epi == ops.EPI_BF16_TP32:  # the V^T operand of self-attention: [N, M rounded up to 64]
                out = torch.empty(N, (Mx + 63) // 64 * 64, device=dev, dtype=torch.bfloat16)
            else:
                out = torch.empty(Mx, N, device=dev, dtype=torch.float32 if epi == ops.EPI_RES_F32 else torch.bfloat16)
            gate = torch.randn(3, N, device=dev)
            ref = None
            times = {v: [] for v in gvars}
            same = {}
            for rnd in range(3):
                for v in gvars:
                    vv, _, gm = v.partition(":")
                    kw = dict(kernel=int(vv), group_m=int(gm or 0))
                    if epi == ops.EPI_RES_F32:
                        out.zero_()
                        fn = lambda: ops.linear(x, w, b, epi, out=out, residual=out, gate=gate, rows_per_batch=21504,
                                                **kw)
                    else:
                        fn = lambda: ops.linear(x, w, b, epi, out=out, **kw)
                    times[v].append(_time(fn, iters=5, warmup=1))
                    if epi == ops.EPI_RES_F32:  # one clean launch on a zero residual for the comparison
                        out.zero_()
                        ops.linear(x, w, b, epi, out=out, residual=out, gate=gate, rows_per_batch=21504, **kw)
                    o = out.float()
                    if ref is None:
                        ref = o.clone()
                    if int(vv) >= 8 or os.environ.get("SA_KB_NOCHECK"):  # measurement kernels / builds
                        continue
                    err = ((o - ref).norm() / ref.norm()).item()
                    assert err < 1e-2, (name, v, err)
                    same.setdefault(v, True)
                    same[v] = same[v] and bool(torch.equal(o, ref))
            fl = 2.0 * Mx * N * K
            r = {"kernel": f"gemm_{name}", "M": Mx, "N": N, "K": K}
            ms_ref = _time(lambda: torch.nn.functional.linear(x, w), iters=5, warmup=1)
            r["torch_tflops"] = round(fl / ms_ref / 1e9, 1)
            for v in gvars:
                ms = sorted(times[v])[1]
                r[f"v{v}_ms"] = round(ms, 4)
                r[f"v{v}_tflops"] = round(fl / ms / 1e9, 1)
                r[f"v{v}_bitident"] = same.get(v)
            res.append(r)
            print(json.dumps(r), flush=True)
            del x, w, out
    if "gemmfp8" in which:  # the fp8 FFN mode's kernels against the bf16 ones they replace, interleaved rounds
        res.extend(bench_fp8_ffn(M))
        res.extend(bench_mxgemm_kernels(MXGEMM_FFN_SHAPES))
    if "attnvar" in which:
        import os
        L, H, D = 21504, 12, 128
        qkv = torch.randn(3 * L, 3 * H * D, device=dev).bfloat16()
        segs = torch.tensor([[b * L, L, b * L, L] for b in range(3)], dtype=torch.int32, device=dev)
        q, k, v_ = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
        outs = {}
        variants = tuple(int(v) for v in os.environ.get("SA_KB_AVARS", "1").split(","))
        vts = {m: vt_layout(v_, 3) for m in (3,) if m in variants}  # kernel 3 reads V^T
        times = {v: [] for v in variants}
        for rnd in range(3):
            for v in variants:
                o = torch.empty(3 * L, H * D, device=dev, dtype=torch.bfloat16)
                vin = vts.get(v, v_)
                times[v].append(_time(lambda: ops.attention(q, k, vin, o, segs, 3, L, H, kernel=v), iters=3, warmup=1))
                outs[v] = o.float()
        # fp32 reference on a sample of query rows of every head (batch row 2)
        qi = torch.arange(0, L, 997, device=dev)
        ref = torch.empty(len(qi), H * D, device=dev)
        for hh in range(H):
            sl = slice(hh * D, (hh + 1) * D)
            s_ = (q[2 * L + qi, sl].float() @ k[2 * L:, sl].float().t()) * D ** -0.5
            ref[:, sl] = torch.softmax(s_, -1) @ v_[2 * L:, sl].float()
        fl = 4.0 * 3 * H * L * L * D
        r = {"kernel": "attn_self"}
        for v in variants:
            ms = sorted(times[v])[1]
            r[f"err_v{v}_v{variants[0]}"] = ((outs[v] - outs[variants[0]]).norm() / outs[variants[0]].norm()).item()
            r[f"v{v}_bitident"] = bool(torch.equal(outs[v], outs[variants[0]]))
            r[f"err_v{v}_fp32"] = ((outs[v][2 * L + qi] - ref).norm() / ref.norm()).item()
            r[f"v{v}_ms"] = round(ms, 3)
            r[f"v{v}_tflops"] = round(fl / ms / 1e9, 1)
        res.append(r)
        print(json.dumps(r), flush=True)
    if "attnclip" in which:
        res.extend(attn_clip_inputs())
    if "cross3" in which:  # the fused text + image + per-frame vocal cross-attention at config 2
        L, H, D, B, nper, nfr = 21504, 12, 128, 3, 32, 21
        q = torch.randn(B * L, H * D, device=dev).bfloat16()
        kvt = torch.randn(B * 512, 2 * H * D, device=dev).bfloat16()
        kvi = torch.randn(B * 257, 2 * H * D, device=dev).bfloat16()
        kvv = torch.randn(B * nfr * nper, 2 * H * D, device=dev).bfloat16()
        o = torch.empty(B * L, H * D, device=dev, dtype=torch.bfloat16)
        fn = lambda: ops.attention_cross3(q, kvt[:, :H * D], kvt[:, H * D:], 512, kvi[:, :H * D], kvi[:, H * D:], 257,
                                          kvv[:, :H * D], kvv[:, H * D:], nper, L // nfr, nfr, o, B, L, H)
        ms = sorted(_time(fn, iters=20, warmup=3) for _ in range(5))[2]
        fl = 4.0 * B * H * L * D * (512 + 257 + nper)
        import hashlib
        r = {"kernel": "attn_cross3", "ms": round(ms, 4), "tflops": round(fl / ms / 1e9, 1),
             "out_sum": float(o.float().abs().sum()),
             "out_sha": hashlib.sha256(o.view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]}
        res.append(r)
        print(json.dumps(r), flush=True)
    if "gemm" in which:
        for (N, K, epi, name) in [(4608, 1536, ops.EPI_BF16, "qkv"), (1536, 1536, ops.EPI_RES_F32, "o_proj"),
                                  (8960, 1536, ops.EPI_GELU_TANH_BF16, "ffn_up"),
                                  (1536, 8960, ops.EPI_RES_F32, "ffn_down")]:
            x = torch.randn(M, K, device=dev).bfloat16()
            w = (torch.randn(N, K, device=dev) / K ** 0.5).bfloat16()
            b = torch.randn(N, device=dev)
            out = torch.empty(M, N, device=dev, dtype=torch.float32 if epi == ops.EPI_RES_F32 else torch.bfloat16)
            gate = torch.randn(3, N, device=dev)
            if epi == ops.EPI_RES_F32:
                fn = lambda: ops.linear(x, w, b, epi, out=out, residual=out, gate=gate, rows_per_batch=21504)
            else:
                fn = lambda: ops.linear(x, w, b, epi, out=out)
            ms = _time(fn)
            ms_ref = _time(lambda: torch.nn.functional.linear(x, w))
            fl = 2.0 * M * N * K
            res.append({"kernel": f"gemm_{name}", "M": M, "N": N, "K": K, "ms": round(ms, 4),
                        "tflops": round(fl / ms / 1e9, 1), "torch_ms": round(ms_ref, 4),
                        "torch_tflops": round(fl / ms_ref / 1e9, 1)})
            print(json.dumps(res[-1]), flush=True)
            del x, w, out
    if "attn" in which:
        L, H, D = 21504, 12, 128
        qkv = torch.randn(3 * L, 3 * H * D, device=dev).bfloat16()
        o = torch.empty(3 * L, H * D, device=dev, dtype=torch.bfloat16)
        segs = torch.tensor([[b * L, L, b * L, L] for b in range(3)], dtype=torch.int32, device=dev)
        q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
        fn = lambda: ops.attention(q, k, v, o, segs, 3, L, H)
        ms = _time(fn, iters=5)
        fl = 4.0 * 3 * H * L * L * D
        qh = q.view(3, L, H, D).transpose(1, 2)
        kh = k.view(3, L, H, D).transpose(1, 2)
        vh = v.view(3, L, H, D).transpose(1, 2)
        try:
            ms_ref = _time(lambda: torch.nn.functional.scaled_dot_product_attention(qh, kh, vh), iters=3)
        except Exception:  # noqa: BLE001
            ms_ref = float("nan")
        res.append({"kernel": "attn_self", "L": L, "ms": round(ms, 3), "tflops": round(fl / ms / 1e9, 1),
                    "torch_sdpa_ms": round(ms_ref, 3), "torch_tflops": round(fl / ms_ref / 1e9, 1)})
        print(json.dumps(res[-1]), flush=True)
    if "gemmsq" in which:  # square shapes of the guide's GEMM template figures (random [-1, 1) operands)
        for n in (4096, 8192):
            x = (torch.rand(n, n, device=dev) * 2 - 1).bfloat16()
            w = (torch.rand(n, n, device=dev) * 2 - 1).bfloat16()
            out = torch.empty(n, n, device=dev, dtype=torch.bfloat16)
            ms = _time(lambda: ops.linear(x, w, None, ops.EPI_BF16, out=out), iters=10, warmup=3)
            ms_ref = _time(lambda: torch.nn.functional.linear(x, w), iters=10, warmup=3)
            fl = 2.0 * n ** 3
            res.append({"kernel": f"gemm_sq{n}", "ms": round(ms, 4), "tflops": round(fl / ms / 1e9, 1),
                        "torch_tflops": round(fl / ms_ref / 1e9, 1)})
            print(json.dumps(res[-1]), flush=True)
            del x, w, out
    if "attn1" in which:  # 3 bare self-attention launches (PMC passes: FETCH_SIZE / WRITE_SIZE)
        L, H, D = 21504, 12, 128
        qkv = torch.randn(3 * L, 3 * H * D, device=dev).bfloat16()
        o = torch.empty(3 * L, H * D, device=dev, dtype=torch.bfloat16)
        segs = torch.tensor([[b * L, L, b * L, L] for b in range(3)], dtype=torch.int32, device=dev)
        for _ in range(3):
            ops.attention(qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:], o, segs, 3, L, H)
        torch.cuda.synchronize()
        res.append({"kernel": "attn_self_x3", "algorithmic_bytes_per_launch": 4 * 3 * L * H * D * 2})
        print(json.dumps(res[-1]), flush=True)
    if "gemm1" in which:  # one launch of each DiT GEMM shape (PMC passes)
        for (N, K, epi, name) in [(4608, 1536, ops.EPI_BF16, "qkv"), (1536, 1536, ops.EPI_RES_F32, "o_proj"),
                                  (8960, 1536, ops.EPI_GELU_TANH_BF16, "ffn_up"),
                                  (1536, 8960, ops.EPI_RES_F32, "ffn_down")]:
            x = torch.randn(M, K, device=dev).bfloat16()
            w = (torch.randn(N, K, device=dev) / K ** 0.5).bfloat16()
            b = torch.randn(N, device=dev)
            out = torch.zeros(M, N, device=dev, dtype=torch.float32 if epi == ops.EPI_RES_F32 else torch.bfloat16)
            if epi == ops.EPI_RES_F32:
                ops.linear(x, w, b, epi, out=out, residual=out)
            else:
                ops.linear(x, w, b, epi, out=out)
            torch.cuda.synchronize()
            del x, w, out
        res.append({"kernel": "gemm_x4"})
        print(json.dumps(res[-1]), flush=True)
    if "dit" in which:
        res.append(bench_dit())
        print(json.dumps(res[-1]), flush=True)
    if "dit14" in which:
        res.append(bench_dit14())
        print(json.dumps(res[-1]), flush=True)
    if "dit14full" in which:  # BASELINE config 4's model: one whole 40-layer forward at 720p x 81 frames
        res.append(bench_dit14(layer_counts=(40,)))
        print(json.dumps(res[-1]), flush=True)
    if "lnvar" in which:  # LayerNorm: one row per wave vs rows sharing the modulation through LDS (interleaved)
        import os
        x = torch.randn(M, 1536, device=dev)
        em = torch.randn(3, 6, 1536, device=dev)
        w, bb = torch.randn(1536, device=dev), torch.randn(1536, device=dev)
        ob = torch.empty(M, 1536, device=dev, dtype=torch.bfloat16)
        modes = {"adaln": dict(shift=em[:, 0], scale=em[:, 1], rows_per_batch=21504),
                 "affine": dict(weight=w, bias=bb)}
        nws = os.environ.get("SA_KB_LNVARS", "0,8,16").split(",")
        for name, kw in modes.items():
            times = {v: [] for v in nws}
            for rnd in range(3):
                for v in nws:
                    os.environ["SA_LN_SHARED"] = v
                    times[v].append(_time(lambda: ops.layernorm_mod(x, ob, 1e-6, **kw), iters=20, warmup=3))
            os.environ.pop("SA_LN_SHARED", None)
            r = {"kernel": f"layernorm_{name}", "M": M}
            for v in nws:
                ms = sorted(times[v])[1]
                r[f"rows{v}_us"] = round(ms * 1e3, 1)
                r[f"rows{v}_tbs"] = round(M * 1536 * 6 / ms / 1e9, 2)
            res.append(r)
            print(json.dumps(r), flush=True)
    if "ditenv" in which:  # in-situ A/B of an environment switch inside full DiT forwards (SA_KB_ENVVARS)
        import os
        res.append(bench_dit(env_variants=tuple(os.environ.get("SA_KB_ENVVARS", "SA_LN_SHARED=0,SA_LN_SHARED=8")
                                                .split(","))))
        print(json.dumps(res[-1]), flush=True)
    if "attnfp8" in which:  # the fp8 attention mode's kernels against the bf16 launch, interleaved rounds
        res.extend(bench_fp8_attn())
    if "attnfp8split" in which:  # the key-split launch at the Ulysses N = 8 rank shape, fp8 and bf16, interleaved
        res.extend(bench_fp8_attn_split())
    if "qkvfp8" in which:  # the fp8 q/k/v mode's operand chains against the bf16 one, interleaved rounds
        res.extend(bench_fp8_qkv())
        res.extend(bench_mxgemm_kernels(MXGEMM_QKV_SHAPES))
    if "ofp8" in which:  # flash kernel + self-attention O-projection: bf16 against the fp8 self-O mode, interleaved
        res.extend(bench_fp8_o())
    if "ditfp8o" in which:  # whole-forward A/B of enable_fp8_o() on top of the other three modes, interleaved
        res.append(bench_dit(fp8_o_ab=True))
        print(json.dumps(res[-1]), flush=True)
    if "ditfp8qkv" in which:  # whole-forward A/B of enable_fp8_qkv() on top of the other two modes, interleaved
        res.append(bench_dit(fp8_qkv_ab=True))
        print(json.dumps(res[-1]), flush=True)
    if "ditfp8attn" in which:  # whole-forward A/B of enable_fp8_attention() (and with enable_fp8_ffn()), interleaved
        res.append(bench_dit(fp8_attn_ab=True))
        print(json.dumps(res[-1]), flush=True)
    if "ditfp8" in which:  # whole-forward A/B of enable_fp8_ffn(), interleaved
        res.append(bench_dit(fp8_ab=True))
        print(json.dumps(res[-1]), flush=True)
    if "unipc" in which:  # the UniPC sampler step beside the Euler one at config 2's latent shape, interleaved
        res.extend(bench_unipc())
    if "attnsparse" in which:  # the block-sparse launch against dense kernel 3 at config 2, interleaved rounds
        res.extend(bench_sparse_attn())
    if "ditsparse" in which:  # whole-forward A/B of enable_sparse_attention(), interleaved
        res.append(bench_dit(sparse_ab=True))
        print(json.dumps(res[-1]), flush=True)
    if "ditvar" in which:  # in-situ A/B of attention variants inside full DiT forwards (interleaved)
        import os
        avars = tuple(int(v) for v in os.environ.get("SA_KB_AVARS", "1").split(","))
        res.append(bench_dit(attn_variants=avars))
        print(json.dumps(res[-1]), flush=True)
    return res


def _sclk_mhz():
    """the graphics clock right now, or None where the runtime cannot tell"""
    try:
        return int(torch.cuda.clock_rate())
    except Exception:  # noqa: BLE001
        return None


def bench_unipc(C=16, T=21, H=64, W=64, R=3, rounds=5):
    """sa_unipc_step (a middle step: corrector and predictor at order 2, all state read) beside sa_flow_step on one
    whole-clip window of config 2's latents [16, 21, 64, 64], R = 3 noise rows, same process, interleaved rounds,
    median of `rounds` with every round kept; 200 launches per timing so that a window is milliseconds, not one
    launch.  bytes = what each kernel has to move per launch: Euler 3 x 2 (noise) + 2 (x) + 2 (pred) = 10 B per
    element, UniPC + 3 x 4 (xhat, m0, m1) + 2 x 4 (new xhat, new m) = 30 B."""
    from .scheduler import FlowUniPCMultistepScheduler
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lat = torch.randn(1, C, T, H, W, device=dev, generator=g).bfloat16()
    pred = torch.empty_like(lat)
    noise = torch.randn(R, C, T, H, W, device=dev, generator=g).bfloat16()
    st = [torch.randn(1, C, T, H, W, device=dev, generator=g) for _ in range(5)]
    sched = FlowUniPCMultistepScheduler(1000, shift=5.0)
    sched.set_timesteps(50)
    k = sched.step_coefficients(25)
    assert (k.corrector, k.predictor) == (2, 2)
    dsig = float(sched.sigmas[26]) - float(sched.sigmas[25])
    fns = {"flow_step": lambda: ops.flow_step(lat, pred, noise, 0, dsig, 5.0, 3.0, 0, 0, None, False),
           "unipc_step": lambda: ops.unipc_step(lat, pred, noise, 0, k, 5.0, 3.0, 0, 0, None, False, *st)}
    times, clocks = {n: [] for n in fns}, []
    for _ in range(rounds):
        for n, fn in fns.items():
            times[n].append(_time(fn, iters=200, warmup=5))
        clocks.append(_sclk_mhz())
    n_el = C * T * H * W
    by = {"flow_step": (2 * R + 2 + 2) * n_el, "unipc_step": (2 * R + 2 + 2 + 3 * 4 + 2 * 4) * n_el}
    r = {"kernel": "sampler_step", "shape": [C, T, H, W], "noise_rows": R, "sclk_mhz": clocks}
    for n in fns:
        ms = sorted(times[n])[rounds // 2]
        r.update({f"{n}_us": round(1e3 * ms, 2), f"{n}_rounds_us": [round(1e3 * t, 2) for t in times[n]],
                  f"{n}_bytes": by[n], f"{n}_gbps": round(by[n] / ms / 1e6, 1)})
    print(json.dumps(r), flush=True)
    return [r]


SPARSE_WINDOWS = (8, 4, 2, 1, 0)  # frame windows of attnsparse / ditsparse, besides the window of all frames


def _table_stats(ptr, idx, q_len, kv_len):
    """density and the spread of the per-tile list lengths (the launch's imbalance: a tile's time follows its list)"""
    from . import sparse_attn
    n = (ptr[1:] - ptr[:-1]).float()
    return {"density": round(sparse_attn.density(ptr, idx, q_len, kv_len), 4), "list_min": int(n.min()),
            "list_mean": round(n.mean().item(), 1), "list_max": int(n.max())}


def bench_sparse_attn(L=21504, H=12, B=3, frames=21, rounds=5):
    """The config-2 self-attention launch (B = 3 rows of L = 21 504 tokens = 21 latent frames of 1024, 12 heads) on the
    V^T kernel 3, same process, interleaved rounds, median of `rounds` with every round kept: dense (sa_attn_fwd_map),
    sa_attn_fwd_sparse with every block listed (the price of the indirection; output compared byte for byte), and with
    the frame-window tables of SPARSE_WINDOWS (sink_frames = 1).  Per table: its density, the spread of its per-tile
    list lengths, and ms / (density x dense ms) -- 1.0 would be time proportional to the blocks visited."""
    from . import sparse_attn
    dev, D = "cuda", 128
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * L, 3 * H * D, device=dev, generator=g).bfloat16()
    q, k = qkv[:, :H * D], qkv[:, H * D:2 * H * D]
    vt = vt_layout(qkv[:, 2 * H * D:], 3)
    segs = torch.tensor([[b * L, L, b * L, L] for b in range(B)], dtype=torch.int32, device=dev)
    outs = {n: torch.empty(B * L, H * D, device=dev, dtype=torch.bfloat16) for n in ("dense", "full")}
    tabs = {"full": sparse_attn.frame_window_table(frames, L // frames, L, L, frames)}
    tabs.update({f"w{w}": sparse_attn.frame_window_table(frames, L // frames, L, L, w) for w in SPARSE_WINDOWS})
    dtabs = {n: tuple(x.to(dev) for x in t) for n, t in tabs.items()}
    o = outs["full"]
    fns = {"dense": lambda: ops.attention(q, k, vt, outs["dense"], segs, B, L, H, kernel=ops.ATTN_VT_P32)}
    for n in tabs:
        fns[n] = lambda n=n: ops.attention(q, k, vt, outs.get(n, o), segs, B, L, H, kernel=ops.ATTN_VT_P32,
                                           blocks=dtabs[n])
    times, clocks = {n: [] for n in fns}, []
    for _ in range(rounds):
        for n, fn in fns.items():
            times[n].append(_time(fn, iters=5, warmup=1))
        clocks.append(_sclk_mhz())
    fns["dense"](), fns["full"]()
    torch.cuda.synchronize()
    ms = {n: sorted(t)[rounds // 2] for n, t in times.items()}
    fl = 4.0 * B * H * L * L * D
    r = {"kernel": "attn_sparse_self", "L": L, "heads": H, "rows": B, "frames": frames, "sclk_mhz": clocks,
         "full_equals_dense": bool(torch.equal(outs["full"], outs["dense"])),
         "dense_ms": round(ms["dense"], 4), "dense_tflops": round(fl / ms["dense"] / 1e9, 1),
         "rounds_ms": {n: [round(t, 4) for t in times[n]] for n in fns}}
    for n, t in tabs.items():
        st = _table_stats(*t, L, L)
        r[n] = dict(st, ms=round(ms[n], 4), ratio_vs_dense=round(ms["dense"] / ms[n], 3),
                    ms_over_density_x_dense=round(ms[n] / (st["density"] * ms["dense"]), 3))
    print(json.dumps(r), flush=True)
    return [r]


def bench_fp8_attn(L=21504, H=12, B=3):
    """The config-2 self-attention launch (`kbench attn`'s: B = 3 rows of L = 21 504 tokens, 12 heads), same process,
    interleaved rounds, median of 3: the bf16 auto kernel against K means + operand pack + MXFP8 flash kernel
    (ops.attention_mxfp8), the flash kernel alone and the means + pack alone.  ratio = bf16 ms / fp8 ms (> 1: the fp8
    path is faster); the graphics clock is read after each round."""
    dev, D = "cuda", 128
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * L, 3 * H * D, device=dev, generator=g).bfloat16()
    o = torch.empty(B * L, H * D, device=dev, dtype=torch.bfloat16)
    o8 = torch.empty_like(o)
    rows = [[b * L, L, b * L, L] for b in range(B)]
    segs = torch.tensor(rows, dtype=torch.int32, device=dev)
    vcol0, Rv = ops.attn_vcol0(rows)
    vc = torch.tensor(vcol0, dtype=torch.int32, device=dev)
    buf = ops.AttnMx8(B * L, B * L, H, Rv, B, dev)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]

    def pack():
        km = ops.attn_kmean(k, segs, B, H, buf.kmean, buf.kmean_work)
        ops.attn_pack_mxfp8(q, k, v, segs, vc, B, L, L, H, buf, kmean=km)

    fns = {"bf16": lambda: ops.attention(q, k, v, o, segs, B, L, H),
           "fp8_total": lambda: ops.attention_mxfp8(q, k, v, o8, segs, B, L, H, vc, L, buf),
           "fp8_kernel": lambda: ops.attn_fwd_mxfp8(buf, o8, segs, vc, B, L, H),
           "fp8_pack": pack}
    times, clocks = {n: [] for n in fns}, []
    for _ in range(3):
        for n, fn in fns.items():
            times[n].append(_time(fn, iters=5, warmup=1))
        clocks.append(_sclk_mhz())
    ms = {n: sorted(t)[1] for n, t in times.items()}
    fl = 4.0 * B * H * L * L * D
    r = {"kernel": "fp8attn_self", "L": L, "heads": H, "rows": B, "sclk_mhz": clocks,
         "rel_l2_fp8_vs_bf16": round(((o8.float() - o.float()).norm() / o.float().norm()).item(), 5)}
    for n in fns:
        r[f"{n}_ms"] = round(ms[n], 4)
    r.update(ratio_total=round(ms["bf16"] / ms["fp8_total"], 3), ratio_kernel=round(ms["bf16"] / ms["fp8_kernel"], 3),
             bf16_tflops=round(fl / ms["bf16"] / 1e9, 1), fp8_kernel_tflops=round(fl / ms["fp8_kernel"] / 1e9, 1))
    print(json.dumps(r), flush=True)
    return [r]


def bench_fp8_attn_split(Lq=10752, Lk=21504, H=3, B=3, rounds=5):
    """The Ulysses N = 8 rank's self-attention launch at config 2 (3 segments x 3 heads, 10 752 queries and 21 504 keys
    each: 378 tiles), kernels alone on packed operands, same process, interleaved rounds, median of `rounds`: the
    MXFP8 flash kernel unsplit and with ops.attn_tail_split's tail as key halves, the bf16 8-wave kernel likewise, and
    the three per-row launches of the per-row-stream schedule on three streams, unsplit and with the last row's tail
    split.  Every round's time is kept (`*_rounds_ms`): the spread between rounds of one arm is what a difference
    between arms is read against.  ratio_* = unsplit ms / split ms (> 1: the split is faster)."""
    dev, D = "cuda", 128
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(B * Lq, H * D, device=dev, generator=g).bfloat16()
    k, v = (torch.randn(B * Lk, H * D, device=dev, generator=g).bfloat16() for _ in range(2))
    o, os_, o8, o8s, o8r = (torch.empty(B * Lq, H * D, device=dev, dtype=torch.bfloat16) for _ in range(5))
    rows = [[b * Lq, Lq, b * Lk, Lk] for b in range(B)]
    segs = torch.tensor(rows, dtype=torch.int32, device=dev)
    vcol0, Rv = ops.attn_vcol0(rows)
    vc = torch.tensor(vcol0, dtype=torch.int32, device=dev)
    buf = ops.AttnMx8(B * Lq, B * Lk, H, Rv, B, dev)
    ops.attn_pack_mxfp8(q, k, v, segs, vc, B, Lq, Lk, H, buf, kmean=ops.attn_kmean(k, segs, B, H, buf.kmean,
                                                                                  buf.kmean_work))
    n_row = H * -(-Lq // 256)
    split = ops.attn_tail_split(0, B * n_row, q.device)
    split_row = ops.attn_tail_split((B - 1) * n_row, n_row, q.device)
    # the per-row launches: one segment table, one operand set (and one split scratch) per row, one stream per row
    seg1 = torch.tensor([[0, Lq, 0, Lk]], dtype=torch.int32, device=dev)
    vc1 = torch.zeros(1, dtype=torch.int32, device=dev)
    bufs, streams = [], [torch.cuda.Stream() for _ in range(B)]
    for b in range(B):
        rb = ops.AttnMx8(Lq, Lk, H, ops.attn_vcol0(rows[:1])[1], 1, dev)
        kb = k[b * Lk:(b + 1) * Lk]
        ops.attn_pack_mxfp8(q[b * Lq:(b + 1) * Lq], kb, v[b * Lk:(b + 1) * Lk], seg1, vc1, 1, Lq, Lk, H, rb,
                            kmean=ops.attn_kmean(kb, seg1, 1, H, rb.kmean, rb.kmean_work))
        bufs.append(rb)

    def per_row(out, st):
        cur = torch.cuda.current_stream()
        for b in range(B):
            streams[b].wait_stream(cur)
            with torch.cuda.stream(streams[b]):
                ops.attn_fwd_mxfp8(bufs[b], out[b * Lq:(b + 1) * Lq], seg1, vc1, 1, Lq, H,
                                   split_tiles=st if b == B - 1 else 0)
        for s in streams:
            cur.wait_stream(s)

    fns = {"fp8": lambda: ops.attn_fwd_mxfp8(buf, o8, segs, vc, B, Lq, H),
           "fp8_split": lambda: ops.attn_fwd_mxfp8(buf, o8s, segs, vc, B, Lq, H, split_tiles=split),
           "bf16": lambda: ops.attention(q, k, v, o, segs, B, Lq, H, kernel=1),
           "bf16_split": lambda: ops.attention(q, k, v, os_, segs, B, Lq, H, split_tiles=split),
           "fp8_rows": lambda: per_row(o8, 0),
           "fp8_rows_split": lambda: per_row(o8r, split_row)}
    times, clocks = {n: [] for n in fns}, []
    for _ in range(rounds):
        for n, fn in fns.items():
            times[n].append(_time(fn, iters=20, warmup=3))
        clocks.append(_sclk_mhz())
    ms = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    rel = lambda a, b: round(((a.float() - b.float()).norm() / b.float().norm()).item(), 6)  # noqa: E731
    r = {"kernel": "fp8attn_split", "Lq": Lq, "Lk": Lk, "heads": H, "rows": B, "tiles": B * n_row,
         "cus": ops._n_cu(q.device), "split_tiles": split, "split_tiles_last_row": split_row, "sclk_mhz": clocks,
         "rel_l2_fp8_split_vs_fp8": rel(o8s, o8), "rel_l2_fp8_rows_split_vs_fp8": rel(o8r, o8),
         "rel_l2_bf16_split_vs_bf16": rel(os_, o), "rel_l2_fp8_vs_bf16": rel(o8, o)}
    for n in fns:
        r[f"{n}_ms"] = round(ms[n], 4)
        r[f"{n}_rounds_ms"] = [round(t, 4) for t in times[n]]
        r[f"{n}_spread"] = round((max(times[n]) - min(times[n])) / ms[n], 4)
    r.update(ratio_fp8=round(ms["fp8"] / ms["fp8_split"], 3), ratio_bf16=round(ms["bf16"] / ms["bf16_split"], 3),
             ratio_fp8_rows=round(ms["fp8_rows"] / ms["fp8_rows_split"], 3))
    print(json.dumps(r), flush=True)
    return [r]


def bench_fp8_qkv(L=21504, H=12, B=3):
    """The self-attention half of a config-2 block up to the point where the MXFP8 flash kernel's operands are ready
    (M = 3 x 21 504 rows, dim 1536, 12 heads; fp8 attention on in all three), same process, interleaved rounds, median
    of 3: the bf16 chain (LayerNorm, QKV GEMM, RMSNorm + RoPE, K means, pack), the fp8 q/k/v mode unfused (MXFP8
    LayerNorm and GEMM, then the same three) and fused (q|k GEMM, V GEMM writing V^T, RMSNorm + RoPE writing Q, K means,
    K pack).  One JSON line for the chains (ratio = bf16 ms / chain ms; whether the fused operands equal the unfused
    ones byte for byte) and one with every stage timed alone in the same rounds."""
    from .transformer import rope_table
    dev, D = "cuda", 128
    C, M = H * D, B * L
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, C, device=dev, generator=g)
    mod = torch.randn(B, 2, C, device=dev, generator=g) * 0.3
    w = (torch.randn(3 * C, C, device=dev, generator=g) / C ** 0.5).bfloat16()
    bias = torch.randn(3 * C, device=dev, generator=g) * 0.1
    nq, nk = 1 + 0.1 * torch.randn(C, device=dev, generator=g), 1 + 0.1 * torch.randn(C, device=dev, generator=g)
    wq8 = ops.mxfp8_quant(w)
    ln_bf, ln_mx = torch.empty(M, C, device=dev, dtype=torch.bfloat16), ops.Mx8.empty(M, C, dev)
    qkv = torch.empty(M, 3 * C, device=dev, dtype=torch.bfloat16)
    rows = [[b * L, L, b * L, L] for b in range(B)]
    segs = torch.tensor(rows, dtype=torch.int32, device=dev)
    vcol0, Rv = ops.attn_vcol0(rows)
    vc = torch.tensor(vcol0, dtype=torch.int32, device=dev)
    buf, buf_f = ops.AttnMx8(M, M, H, Rv, B, dev), ops.AttnMx8(M, M, H, Rv, B, dev)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    kw = dict(shift=mod[:, 0], scale=mod[:, 1], rows_per_batch=L)
    rope_kw = dict(rope=rope_table(D).to(dev), rows_per_batch=L, tok_offset=0, grid=(21, 32, 32), head_dim=D,
                   n_frame_pairs=D // 2 - 2 * (D // 6), n_height_pairs=D // 6)
    st = {
        "ln_bf16": lambda: ops.layernorm_mod(x, ln_bf, 1e-6, **kw),
        "ln_mxfp8": lambda: ops.layernorm_mod_mxfp8(x, ln_mx, 1e-6, **kw),
        "qkv_bf16": lambda: ops.linear(ln_bf, w, bias, ops.EPI_BF16, out=qkv),
        "qkv_mxfp8": lambda: ops.linear_mxfp8(ln_mx, wq8, bias, ops.EPI_BF16, out=qkv),
        "qk_mxfp8": lambda: ops.linear_mxfp8(ln_mx, wq8[:2 * C], bias[:2 * C], ops.EPI_BF16, out=qkv[:, :2 * C]),
        "v_mxfp8_vt": lambda: ops.linear_mxfp8_vt(ln_mx, wq8[2 * C:], bias[2 * C:], L, B, buf_f),
        "rope": lambda: ops.qk_rmsnorm_rope(qkv, 0, C, nq, nk, C, 1e-6, **rope_kw),
        "rope_mxfp8": lambda: ops.qk_rmsnorm_rope_mxfp8(qkv, 0, C, nq, nk, C, 1e-6, buf_f, **rope_kw),
        "kmean": lambda: ops.attn_kmean(k, segs, B, H, buf.kmean, buf.kmean_work),
        "pack": lambda: ops.attn_pack_mxfp8(q, k, v, segs, vc, B, L, L, H, buf, kmean=buf.kmean),
        "kmean_f": lambda: ops.attn_kmean(k, segs, B, H, buf_f.kmean, buf_f.kmean_work),
        "pack_k": lambda: ops.attn_pack_k_mxfp8(k, segs, B, L, H, buf_f, buf_f.kmean),
    }
    seq = {"bf16": ("ln_bf16", "qkv_bf16", "rope", "kmean", "pack"),
           "unfused": ("ln_mxfp8", "qkv_mxfp8", "rope", "kmean", "pack"),
           "fused": ("ln_mxfp8", "qk_mxfp8", "v_mxfp8_vt", "rope_mxfp8", "kmean_f", "pack_k")}

    def chain(name):
        def run():
            for s_ in seq[name]:
                st[s_]()
        return run

    fns = {n: chain(n) for n in seq}
    fns.update(st)
    times, clocks = {n: [] for n in fns}, []
    for _ in range(3):
        for n, fn in fns.items():
            times[n].append(_time(fn, iters=10, warmup=1))
        clocks.append(_sclk_mhz())
    ms = {n: sorted(t)[1] for n, t in times.items()}
    fns["unfused"]()
    fns["fused"]()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in ((buf.qq, buf_f.qq), (buf.qs, buf_f.qs), (buf.kq, buf_f.kq),
                                              (buf.ks, buf_f.ks), (buf.vq, buf_f.vq), (buf.vs, buf_f.vs)))
    r = {"kernel": "fp8qkv_chain", "M": M, "dim": C, "heads": H, "sclk_mhz": clocks, "fused_equals_unfused": same}
    for n in seq:
        r[f"{n}_ms"] = round(ms[n], 4)
    r.update(ratio_unfused=round(ms["bf16"] / ms["unfused"], 3), ratio_fused=round(ms["bf16"] / ms["fused"], 3),
             fused_vs_unfused=round(ms["unfused"] / ms["fused"], 3))
    print(json.dumps(r), flush=True)
    r2 = {"kernel": "fp8qkv_stages", "M": M}
    r2.update({f"{n}_ms": round(ms[n], 4) for n in st})
    print(json.dumps(r2), flush=True)
    return [r, r2]


def bench_fp8_o(L=21504, H=12, B=3):
    """The end of the self-attention half of a config-2 block (M = 3 x 21 504 rows, dim 1536, 12 heads; fp8 attention
    on in all three arms), same process, interleaved rounds, median of 3: the MXFP8 flash kernel writing bf16 + the bf16
    O-projection with its fp32 gated-residual epilogue (bf16: what the three existing modes run), the fp8 self-O mode
    unfused (the same flash launch, the quantiser, the MXFP8 GEMM) and fused (the flash kernel writing the GEMM's
    operand, the MXFP8 GEMM).  One JSON line for the chains, each timed as one sequence (ratio = bf16 ms / chain ms;
    whether the fused operand equals the unfused one byte for byte), and one with every stage timed alone in the same
    rounds, the MXFP8 O-projection also on the persistent kernel and on the split K step, and both projections in
    place (output = residual, as the forward calls them)."""
    dev, D = "cuda", 128
    C, M = H * D, B * L
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(M, 3 * C, device=dev, generator=g).bfloat16()
    x = torch.randn(M, C, device=dev, generator=g)
    xo, xi = torch.empty_like(x), x.clone()
    gate = torch.randn(B, C, device=dev, generator=g) * 0.3
    w = (torch.randn(C, C, device=dev, generator=g) / C ** 0.5).bfloat16()
    bias = torch.randn(C, device=dev, generator=g) * 0.1
    w8 = ops.mxfp8_quant(w)
    o = torch.empty(M, C, device=dev, dtype=torch.bfloat16)
    oq, oq_f = ops.Mx8.empty(M, C, dev), ops.Mx8.empty(M, C, dev)
    rows = [[b * L, L, b * L, L] for b in range(B)]
    segs = torch.tensor(rows, dtype=torch.int32, device=dev)
    vcol0, Rv = ops.attn_vcol0(rows)
    vc = torch.tensor(vcol0, dtype=torch.int32, device=dev)
    buf = ops.AttnMx8(M, M, H, Rv, B, dev)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    ops.attn_pack_mxfp8(q, k, v, segs, vc, B, L, L, H, buf, kmean=ops.attn_kmean(k, segs, B, H, buf.kmean,
                                                                                buf.kmean_work))
    epi = dict(out=xo, residual=x, gate=gate, rows_per_batch=L)
    inplace = dict(out=xi, residual=xi, gate=gate, rows_per_batch=L)  # as the forward calls it: x += gate * y
    st = {
        "flash_bf16": lambda: ops.attn_fwd_mxfp8(buf, o, segs, vc, B, L, H),
        "flash_o8": lambda: ops.attn_fwd_mxfp8(buf, oq_f, segs, vc, B, L, H),
        "quant": lambda: ops.mxfp8_quant(o, out=oq),
        "oproj_bf16": lambda: ops.linear(o, w, bias, ops.EPI_RES_F32, **epi),
        "oproj_mxfp8": lambda: ops.linear_mxfp8(oq, w8, bias, ops.EPI_RES_F32, **epi),
        "oproj_mxfp8_f": lambda: ops.linear_mxfp8(oq_f, w8, bias, ops.EPI_RES_F32, **epi),
        # the same GEMM on the MXFP8 GEMM's other kernels (auto is the one-tile kernel, one-barrier K step, at K = 1536)
        "oproj_mxfp8_persistent": lambda: ops.linear_mxfp8(oq, w8, bias, ops.EPI_RES_F32, kernel=2, **epi),
        "oproj_mxfp8_kstep2": lambda: ops.linear_mxfp8(oq, w8, bias, ops.EPI_RES_F32, kstep=2, **epi),
        "oproj_bf16_inplace": lambda: ops.linear(o, w, bias, ops.EPI_RES_F32, **inplace),
        "oproj_mxfp8_inplace": lambda: ops.linear_mxfp8(oq, w8, bias, ops.EPI_RES_F32, **inplace),
    }
    seq = {"bf16": ("flash_bf16", "oproj_bf16"), "unfused": ("flash_bf16", "quant", "oproj_mxfp8"),
           "fused": ("flash_o8", "oproj_mxfp8_f")}

    def chain(name):
        def run():
            for s_ in seq[name]:
                st[s_]()
        return run

    fns = {n: chain(n) for n in seq}
    fns.update(st)
    times, clocks = {n: [] for n in fns}, []
    for _ in range(3):
        for n, fn in fns.items():
            times[n].append(_time(fn, iters=10, warmup=1))
        clocks.append(_sclk_mhz())
    ms = {n: sorted(t)[1] for n, t in times.items()}
    fns["bf16"]()
    ref = xo.clone()
    fns["unfused"]()
    un = xo.clone()
    fns["fused"]()
    torch.cuda.synchronize()
    same = torch.equal(oq.q, oq_f.q) and torch.equal(oq.s, oq_f.s) and torch.equal(un, xo)
    r = {"kernel": "fp8o_chain", "M": M, "dim": C, "heads": H, "sclk_mhz": clocks, "fused_equals_unfused": same,
         "rel_l2_fp8_o_vs_bf16_o": round(((xo - ref).norm() / ref.norm()).item(), 6)}
    for n in seq:
        r[f"{n}_ms"] = round(ms[n], 4)
        r[f"{n}_rounds_ms"] = [round(t, 4) for t in times[n]]
    r.update(ratio_unfused=round(ms["bf16"] / ms["unfused"], 4), ratio_fused=round(ms["bf16"] / ms["fused"], 4),
             fused_vs_unfused=round(ms["unfused"] / ms["fused"], 4))
    print(json.dumps(r), flush=True)
    r2 = {"kernel": "fp8o_stages", "M": M}
    r2.update({f"{n}_ms": round(ms[n], 4) for n in st})
    r2.update({f"{n}_rounds_ms": [round(t, 4) for t in times[n]] for n in st})
    print(json.dumps(r2), flush=True)
    return [r, r2]


# (name, M, N, K, epilogue): config 2 (M = 3 x 21 504) and the Ulysses N = 8 rank (M = 3 x 2 688) FFN, config-2 q|k, qkv
MXGEMM_FFN_SHAPES = (("ffn_up", 64512, 8960, 1536, ops.EPI_GELU_TANH_MXFP8), ("ffn_down", 64512, 1536, 8960, ops.EPI_RES_F32),
                     ("ffn_up_rank8", 8064, 8960, 1536, ops.EPI_GELU_TANH_MXFP8),
                     ("ffn_down_rank8", 8064, 1536, 8960, ops.EPI_RES_F32))
MXGEMM_QKV_SHAPES = (("qk", 64512, 3072, 1536, ops.EPI_BF16), ("qkv", 64512, 4608, 1536, ops.EPI_BF16))


def bench_mxgemm_kernels(shapes, rounds=5):
    """sa_gemm_mxfp8_ks's one-tile kernel with the one-barrier K step (kernel=1, kstep=1: the baseline arm) against its
    persistent kernel (kernel=2, one workgroup per CU) and the one-tile kernel with the split K step (kernel=1, kstep=2)
    on random MXFP8 operands, same process, interleaved rounds, median of `rounds` per arm, every round kept, spread =
    (max - min) / median per arm, the graphics clock after each round.  ratio = one-tile ms / persistent ms and
    kstep_ratio = one-tile ms / split-step ms (> 1: the other arm is faster); `identical`: the three outputs (and
    scales) byte for byte."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    res = []
    for name, M, N, K, epi in shapes:
        x = ops.mxfp8_quant(torch.randn(M, K, device=dev, generator=g).bfloat16())
        w = ops.mxfp8_quant((torch.randn(N, K, device=dev, generator=g) / K ** 0.5).bfloat16())
        bias = torch.randn(N, device=dev, generator=g) * 0.1
        kw = {}
        if epi == ops.EPI_RES_F32:  # residual in its own buffer, so that repeated launches keep one input
            kw = dict(residual=torch.randn(M, N, device=dev, generator=g), gate=torch.randn(3, N, device=dev, generator=g),
                      rows_per_batch=M // 3)
        if epi == ops.EPI_GELU_TANH_MXFP8:
            outs = {k: ops.Mx8.empty(M, N, dev) for k in (1, 2, 3)}
        else:
            dt = torch.float32 if epi == ops.EPI_RES_F32 else torch.bfloat16
            outs = {k: torch.empty(M, N, device=dev, dtype=dt) for k in (1, 2, 3)}
        fns = {"one_tile": lambda: ops.linear_mxfp8(x, w, bias, epi, out=outs[1], kernel=1, kstep=1, **kw),
               "persistent": lambda: ops.linear_mxfp8(x, w, bias, epi, out=outs[2], kernel=2, **kw),
               "kstep2": lambda: ops.linear_mxfp8(x, w, bias, epi, out=outs[3], kernel=1, kstep=2, **kw)}
        times, clocks = {n: [] for n in fns}, []
        for _ in range(rounds):
            for n, fn in fns.items():
                times[n].append(_time(fn, iters=20, warmup=2))
            clocks.append(_sclk_mhz())
        torch.cuda.synchronize()
        if epi == ops.EPI_GELU_TANH_MXFP8:
            same = all(torch.equal(outs[1].q, outs[k].q) and torch.equal(outs[1].s, outs[k].s) for k in (2, 3))
        else:
            same = all(torch.equal(outs[1], outs[k]) for k in (2, 3))
        ms = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        r = {"kernel": f"mxgemm_{name}", "M": M, "N": N, "K": K, "epilogue": epi, "tiles": -(-M // 256) * -(-N // 256),
             "cus": ops._n_cu(x.q.device), "sclk_mhz": clocks, "identical": bool(same)}
        for n in fns:
            r[f"{n}_ms"] = round(ms[n], 4)
            r[f"{n}_tflops"] = round(2.0 * M * N * K / ms[n] / 1e9, 1)
            r[f"{n}_rounds_ms"] = [round(t, 4) for t in times[n]]
            r[f"{n}_spread"] = round((max(times[n]) - min(times[n])) / ms[n], 4)
        r["ratio"] = round(ms["one_tile"] / ms["persistent"], 4)
        r["kstep_ratio"] = round(ms["one_tile"] / ms["kstep2"], 4)
        res.append(r)
        print(json.dumps(r), flush=True)
        del x, w, outs, kw
    return res


def bench_fp8_ffn(M=3 * 21504, C=1536, FF=8960, rpb=21504):
    """The three kernels of a block's FFN at config 2 (M = 64 512 rows), bf16 (auto kernel) vs MXFP8, same process,
    interleaved rounds, median of 3: LayerNorm + modulate (bf16 out vs MXFP8 out), ffn_up (N 8960, K 1536, GELU;
    MXFP8 out in the fp8 mode) and ffn_down (N 1536, K 8960, gated residual in place).  One JSON line per pair
    and one for the sum; ratio = bf16 ms / MXFP8 ms (> 1: the fp8 kernel is faster)."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, C, device=dev, generator=g)
    mod = torch.randn(3, 2, C, device=dev, generator=g) * 0.3
    w0 = (torch.randn(FF, C, device=dev, generator=g) / C ** 0.5).bfloat16()
    w2 = (torch.randn(C, FF, device=dev, generator=g) / FF ** 0.5).bfloat16()
    b0, b2 = torch.randn(FF, device=dev, generator=g) * 0.1, torch.randn(C, device=dev, generator=g) * 0.1
    gate = torch.randn(3, C, device=dev, generator=g)
    w0q, w2q = ops.mxfp8_quant(w0), ops.mxfp8_quant(w2)
    ln_bf, ln_mx = torch.empty(M, C, device=dev, dtype=torch.bfloat16), ops.Mx8.empty(M, C, dev)
    h_bf, h_mx = torch.empty(M, FF, device=dev, dtype=torch.bfloat16), ops.Mx8.empty(M, FF, dev)
    out = torch.zeros(M, C, device=dev)
    kw = dict(shift=mod[:, 0], scale=mod[:, 1], rows_per_batch=rpb)
    pairs = {
        "layernorm": (lambda: ops.layernorm_mod(x, ln_bf, 1e-6, **kw), lambda: ops.layernorm_mod_mxfp8(x, ln_mx, 1e-6, **kw)),
        "ffn_up": (lambda: ops.linear(ln_bf, w0, b0, ops.EPI_GELU_TANH_BF16, out=h_bf),
                   lambda: ops.linear_mxfp8(ln_mx, w0q, b0, ops.EPI_GELU_TANH_MXFP8, out=h_mx)),
        "ffn_down": (lambda: ops.linear(h_bf, w2, b2, ops.EPI_RES_F32, out=out, residual=out, gate=gate, rows_per_batch=rpb),
                     lambda: ops.linear_mxfp8(h_mx, w2q, b2, ops.EPI_RES_F32, out=out, residual=out, gate=gate,
                                              rows_per_batch=rpb)),
    }
    res, tot = [], [0.0, 0.0]
    for name, fns in pairs.items():  # in data-flow order: each pair's inputs were written by the pair before
        times = ([], [])
        for _ in range(3):
            for i, fn in enumerate(fns):
                if name == "ffn_down":
                    out.zero_()
                times[i].append(_time(fn, iters=40, warmup=2))
        ms = [sorted(t)[1] for t in times]
        r = {"kernel": f"fp8ffn_{name}", "M": M, "bf16_ms": round(ms[0], 4), "mxfp8_ms": round(ms[1], 4),
             "ratio": round(ms[0] / ms[1], 3)}
        if name != "layernorm":
            fl = 2.0 * M * C * FF
            r.update(bf16_tflops=round(fl / ms[0] / 1e9, 1), mxfp8_tflops=round(fl / ms[1] / 1e9, 1))
        tot = [tot[0] + ms[0], tot[1] + ms[1]]
        res.append(r)
        print(json.dumps(r), flush=True)
    r = {"kernel": "fp8ffn_ln_up_down", "M": M, "bf16_ms": round(tot[0], 4), "mxfp8_ms": round(tot[1], 4),
         "ratio": round(tot[0] / tot[1], 3)}
    res.append(r)
    print(json.dumps(r), flush=True)
    return res


def bench_dit14(layer_counts=(1, 2)):
    """BASELINE config 4's model on one GPU: WanTransformer3DFantasy14BModel (dim 5120, 40 heads, ffn 13824)
    at 720x1280 (90x160 latent, 21 latent frames: L = 75 600 tokens, B = 3 CFG rows), forwards with 1 and 2
    layers; the difference is one block's time, the remainder the embeddings + 14B vocal projector + head."""
    from . import synthetic
    from .flops import dit_forward_flops
    from .transformer import WanTransformer3DFantasy14BModel, param_shapes
    cfg = dict(model_type="i2v", dim=5120, ffn_dim=13824, freq_dim=256, text_dim=4096, in_dim=36, out_dim=16,
               num_heads=40, text_len=512)
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lat = torch.randn(1, 16, 21, 90, 160, device=dev, generator=g).bfloat16()
    y = torch.randn(3, 20, 21, 90, 160, device=dev, generator=g).bfloat16()
    ctx = [torch.randn(n, 4096, device=dev, generator=g) for n in (120, 120, 60)]
    clip = torch.randn(3, 257, 1280, device=dev, generator=g)
    a = torch.randn(1, 161, 768, device=dev, generator=g)
    voc = torch.cat([torch.zeros_like(a), a, a])
    t = torch.tensor([990.0], device=dev)
    L = 21 * 45 * 80
    ms = {}
    for nl in layer_counts:
        m = WanTransformer3DFantasy14BModel(**cfg, num_layers=nl).to(dev)
        m.load_state_dict(synthetic.fill_state_dict(param_shapes(dict(cfg, num_layers=nl, vocal="14B")), 0,
                                                    backend="torch", device=dev))
        print(f"[kbench] dit14: {nl}-layer model loaded, timing", file=sys.stderr, flush=True)
        with torch.no_grad():
            ms[nl] = _time(lambda: m.forward_window(lat, 0, True, 3, t, ctx, L, clip, y, voc, 81), iters=2, warmup=1)
        del m
        torch.cuda.empty_cache()
    if tuple(layer_counts) == (40,):  # the whole 40-layer forward, measured
        fl_fwd = dit_forward_flops(B=3, L=L, dim=5120, ffn=13824, layers=40)
        return {"kernel": "dit14_forward_720p_40_layers", "L": L, "ms_forward": round(ms[40], 0),
                "tflop_per_forward": round(fl_fwd / 1e12, 0), "tflops": round(fl_fwd / ms[40] / 1e9, 1),
                "clip_s_projected_50_steps": round(50 * ms[40] / 1e3, 0)}
    per_layer = ms[2] - ms[1]
    fl_layer = dit_forward_flops(B=3, L=L, dim=5120, ffn=13824, layers=1) - dit_forward_flops(
        B=3, L=L, dim=5120, ffn=13824, layers=0)
    fl_fwd = dit_forward_flops(B=3, L=L, dim=5120, ffn=13824, layers=40)
    fwd40 = ms[1] - per_layer + 40 * per_layer
    return {"kernel": "dit14_forward_720p", "L": L, "ms_1_layer": round(ms[1], 1), "ms_2_layers": round(ms[2], 1),
            "ms_per_layer": round(per_layer, 1), "tflops_per_layer": round(fl_layer / per_layer / 1e9, 1),
            "ms_forward_40_layers_projected": round(fwd40, 0), "tflop_per_forward": round(fl_fwd / 1e12, 0),
            "tflops_forward_projected": round(fl_fwd / fwd40 / 1e9, 1)}


def attn_clip_inputs(layers=(0, 15, 29)):
    """The self-attention launches' operands of one config-2 DiT forward (random-init weights, bench_dit's
    inputs) against random operands of the same shapes: per captured layer, the launch time with q/k and V^T each
    from the forward or from randn (2 x 2), so a difference splits into the scores' side (rescale frequency) and
    the data's side (switching power)."""
    from . import ops as _ops
    captured, calls = [], [0]
    real = _ops.attention

    def spy(q, k, v, o, segs, B, L, H, **kw):
        if kw.get("kernel") == _ops.ATTN_VT_P32:
            if calls[0] in layers:
                captured.append((calls[0], q.clone(), k.clone(), v.clone(), segs.clone(), B, L, H))
            calls[0] += 1
        return real(q, k, v, o, segs, B, L, H, **kw)
    fwd = bench_dit(fwd_only=True)
    _ops.attention = spy
    try:
        with torch.no_grad():
            fwd()
    finally:
        _ops.attention = real
    torch.cuda.synchronize()
    out = []
    for (li, q, k, vt, segs, B, L, H) in captured:
        qr, kr = torch.randn_like(q.float()).bfloat16(), torch.randn_like(k.float()).bfloat16()
        vr = torch.randn_like(vt.float()).bfloat16()
        o = torch.empty(B * L, H * 128, device=q.device, dtype=torch.bfloat16)
        combos = {"qk_clip_v_clip": (q, k, vt), "qk_rand_v_clip": (qr, kr, vt), "qk_clip_v_rand": (q, k, vr),
                  "qk_rand_v_rand": (qr, kr, vr)}
        times = {c: [] for c in combos}
        for _ in range(3):
            for c, (a, b_, v) in combos.items():
                times[c].append(_time(lambda: real(a, b_, v, o, segs, B, L, H, kernel=_ops.ATTN_VT_P32), iters=3,
                                      warmup=1))
        # scaled score statistics on a sample of rows (head 0, batch row 0): spread of the row max, log2 units
        qs = q[:L:997, :128].float()
        sc = qs @ k[:L, :128].float().t() * (128 ** -0.5) * 1.4426950408889634
        r = {"kernel": "attn_clip_inputs", "layer": li, "q_rms": round(q.float().pow(2).mean().sqrt().item(), 3),
             "k_rms": round(k.float().pow(2).mean().sqrt().item(), 3),
             "row_max_log2_mean": round(sc.max(1).values.mean().item(), 2),
             "score_std_log2": round(sc.std().item(), 2)}
        for c in combos:
            r[f"{c}_ms"] = round(sorted(times[c])[1], 3)
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def bench_dit(iters=3, attn_variants=None, env_variants=None, fwd_only=False, fp8_ab=False, fp8_attn_ab=False,
              fp8_qkv_ab=False, fp8_o_ab=False, sparse_ab=False):
    """One full 30-layer DiT forward at config 2 (B=3 CFG, 21 latent frames at 64x64, L=21504).
    attn_variants: time the forward under each self-attention schedule, interleaved rounds.
    fp8_ab: the forward with enable_fp8_ffn() off and on (two models on the same weights), interleaved rounds,
    and the rel-L2 between their outputs.  fp8_attn_ab: the same for enable_fp8_attention() off, on, and on together
    with enable_fp8_ffn() (three models on the same weights), each output's rel-L2 against off, the graphics clock
    after each round.  fp8_qkv_ab: four variants on the same weights -- off; attention + FFN; those + enable_fp8_qkv()
    unfused; fused; fused with the MXFP8 GEMMs on their persistent kernel; and fused with every MXFP8 GEMM on the
    one-barrier K step -- each output's rel-L2 against off, whether fused equals unfused, and persistent and the
    one-barrier step equal fused, byte for byte.  fp8_o_ab: off; the three modes (attention + FFN + q/k/v); those +
    enable_fp8_o() unfused; fused -- every round kept, each output's rel-L2 against off, whether fused equals unfused.
    sparse_ab: one model with enable_sparse_attention() off, on at a window of all frames (every block listed: the
    output compared byte for byte with off) and on at SPARSE_WINDOWS -- every round kept, each table's density, each
    output's rel-L2 against off (synthetic weights: how far the function moved, not a quality figure)."""
    from . import synthetic
    from .transformer import WanTransformer3DFantasyModel, param_shapes
    cfg = dict(model_type="i2v", dim=1536, ffn_dim=8960, freq_dim=256, text_dim=4096, in_dim=36, out_dim=16,
               num_heads=12, num_layers=30, text_len=512)
    dev = "cuda"
    m = WanTransformer3DFantasyModel(**cfg)
    m.load_state_dict(synthetic.fill_state_dict(param_shapes(cfg), 0, backend="torch", device=dev))
    m = m.to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    lat = torch.randn(1, 16, 21, 64, 64, device=dev, generator=g).bfloat16()
    y = torch.randn(3, 20, 21, 64, 64, device=dev, generator=g).bfloat16()
    ctx = [torch.randn(n, 4096, device=dev, generator=g) for n in (120, 120, 60)]
    clip = torch.randn(3, 257, 1280, device=dev, generator=g)
    voc = torch.randn(3, 167, 768, device=dev, generator=g)
    t = torch.tensor([990.0], device=dev)

    def fwd():
        return m.forward_window(lat, 0, True, 3, t, ctx, 21504, clip, y, voc, 81)

    if fwd_only:
        return fwd
    from .flops import dit_forward_flops
    fl = dit_forward_flops()
    if fp8_ab:
        m8 = WanTransformer3DFantasyModel(**cfg)
        m8.load_state_dict(m.state_dict())
        m8 = m8.to(dev)
        m8.enable_fp8_ffn()
        fwds = {"bf16": fwd, "fp8_ffn": lambda: m8.forward_window(lat, 0, True, 3, t, ctx, 21504, clip, y, voc, 81)}
        times = {k: [] for k in fwds}
        with torch.no_grad():
            for _ in range(3):
                for k, f in fwds.items():
                    times[k].append(_time(f, iters=2, warmup=1))
            o, o8 = fwds["bf16"]().float(), fwds["fp8_ffn"]().float()
        r = {"kernel": "dit_forward_fp8_ffn_ab", "tflop": round(fl / 1e12, 1),
             "rel_l2_on_vs_off": round(((o8 - o).norm() / o.norm()).item(), 5)}
        for k in fwds:
            r[f"{k}_ms"] = round(sorted(times[k])[1], 2)
        r["ratio"] = round(r["bf16_ms"] / r["fp8_ffn_ms"], 4)
        return r
    if fp8_attn_ab:
        modes = {"off": m}
        for k in ("fp8_attn", "fp8_attn_ffn"):
            mm = WanTransformer3DFantasyModel(**cfg)
            mm.load_state_dict(m.state_dict())
            modes[k] = mm.to(dev)
            modes[k].enable_fp8_attention()
        modes["fp8_attn_ffn"].enable_fp8_ffn()
        times, clocks, outs = {k: [] for k in modes}, [], {}
        with torch.no_grad():
            for _ in range(3):
                for k, mm in modes.items():
                    f = lambda mm=mm: mm.forward_window(lat, 0, True, 3, t, ctx, 21504, clip, y, voc, 81)  # noqa: E731
                    times[k].append(_time(f, iters=2, warmup=1))
                    outs[k] = f().float()
                clocks.append(_sclk_mhz())
        r = {"kernel": "dit_forward_fp8_attn_ab", "tflop": round(fl / 1e12, 1), "sclk_mhz": clocks}
        for k in modes:
            r[f"{k}_ms"] = round(sorted(times[k])[1], 2)
            if k != "off":
                r[f"rel_l2_{k}_vs_off"] = round(((outs[k] - outs["off"]).norm() / outs["off"].norm()).item(), 5)
                r[f"ratio_{k}"] = round(r["off_ms"] / r[f"{k}_ms"], 4)
        return r
    if fp8_qkv_ab:
        modes = {"off": m}
        for k in ("attn_ffn", "attn_ffn_qkv_unfused", "attn_ffn_qkv_fused"):
            mm = WanTransformer3DFantasyModel(**cfg)
            mm.load_state_dict(m.state_dict())
            modes[k] = mm.to(dev)
            modes[k].enable_fp8_attention()
            modes[k].enable_fp8_ffn()
            if k != "attn_ffn":
                modes[k].enable_fp8_qkv()
                modes[k]._fp8_qkv_fused = k.endswith("_fused")
        # the fused variant again with every sa_gemm_mxfp8_ks launch on the persistent kernel (what SA_MXGEMM_KERNEL=2
        # does to a process; the variable is read once, so one process cannot hold both of its states), and once more
        # with every launch on the one-barrier K step (what SA_MXGEMM_KSTEP=1 does: the baseline arm of the K-step auto)
        import os
        pers, ks1 = "attn_ffn_qkv_fused_persistent", "attn_ffn_qkv_fused_kstep1"
        modes[pers] = modes[ks1] = modes["attn_ffn_qkv_fused"]
        one_tile_or_auto = ops.linear_mxfp8
        forced = {pers: lambda *a, **kw: one_tile_or_auto(*a, **dict(kw, kernel=2)),
                  ks1: lambda *a, **kw: one_tile_or_auto(*a, **dict(kw, kstep=1))}
        times, clocks, outs = {k: [] for k in modes}, [], {}
        with torch.no_grad():
            for _ in range(3):
                for k, mm in modes.items():
                    f = lambda mm=mm: mm.forward_window(lat, 0, True, 3, t, ctx, 21504, clip, y, voc, 81)  # noqa: E731
                    ops.linear_mxfp8 = forced.get(k, one_tile_or_auto)
                    try:
                        times[k].append(_time(f, iters=2, warmup=1))
                        outs[k] = f().float()
                    finally:
                        ops.linear_mxfp8 = one_tile_or_auto
                clocks.append(_sclk_mhz())
        r = {"kernel": "dit_forward_fp8_qkv_ab", "tflop": round(fl / 1e12, 1), "sclk_mhz": clocks,
             "SA_MXGEMM_KERNEL": os.environ.get("SA_MXGEMM_KERNEL"), "SA_MXGEMM_KSTEP": os.environ.get("SA_MXGEMM_KSTEP"),
             "fused_equals_unfused": bool(torch.equal(outs["attn_ffn_qkv_fused"], outs["attn_ffn_qkv_unfused"])),
             "persistent_equals_fused": bool(torch.equal(outs[pers], outs["attn_ffn_qkv_fused"])),
             "kstep1_equals_fused": bool(torch.equal(outs[ks1], outs["attn_ffn_qkv_fused"])),
             "rounds_ms": {k: [round(v, 2) for v in times[k]] for k in ("attn_ffn_qkv_fused", pers, ks1)}}
        for k in modes:
            r[f"{k}_ms"] = round(sorted(times[k])[1], 2)
            if k != "off":
                r[f"rel_l2_{k}_vs_off"] = round(((outs[k] - outs["off"]).norm() / outs["off"].norm()).item(), 5)
                r[f"ratio_{k}"] = round(r["off_ms"] / r[f"{k}_ms"], 4)
        for k in ("attn_ffn_qkv_unfused", "attn_ffn_qkv_fused", pers, ks1):
            r[f"ratio_{k}_vs_attn_ffn"] = round(r["attn_ffn_ms"] / r[f"{k}_ms"], 4)
        r["ratio_kstep_auto_vs_kstep1"] = round(r[f"{ks1}_ms"] / r["attn_ffn_qkv_fused_ms"], 4)
        return r
    if fp8_o_ab:
        modes = {"off": m}
        for k in ("three", "four_unfused", "four_fused"):
            mm = WanTransformer3DFantasyModel(**cfg)
            mm.load_state_dict(m.state_dict())
            modes[k] = mm.to(dev)
            modes[k].enable_fp8_attention(), modes[k].enable_fp8_ffn(), modes[k].enable_fp8_qkv()
            if k != "three":
                modes[k].enable_fp8_o()
                modes[k]._fp8_o_fused = k.endswith("_fused")
        times, clocks, outs = {k: [] for k in modes}, [], {}
        with torch.no_grad():
            for _ in range(3):
                for k, mm in modes.items():
                    f = lambda mm=mm: mm.forward_window(lat, 0, True, 3, t, ctx, 21504, clip, y, voc, 81)  # noqa: E731
                    times[k].append(_time(f, iters=2, warmup=1))
                    outs[k] = f().float()
                clocks.append(_sclk_mhz())
        r = {"kernel": "dit_forward_fp8_o_ab", "tflop": round(fl / 1e12, 1), "sclk_mhz": clocks,
             "fused_equals_unfused": bool(torch.equal(outs["four_fused"], outs["four_unfused"])),
             "rounds_ms": {k: [round(v, 2) for v in times[k]] for k in modes}}
        for k in modes:
            r[f"{k}_ms"] = round(sorted(times[k])[1], 2)
            if k != "off":
                r[f"rel_l2_{k}_vs_off"] = round(((outs[k] - outs["off"]).norm() / outs["off"].norm()).item(), 5)
                r[f"ratio_{k}"] = round(r["off_ms"] / r[f"{k}_ms"], 4)
        for k in ("four_unfused", "four_fused"):
            r[f"ratio_{k}_vs_three"] = round(r["three_ms"] / r[f"{k}_ms"], 4)
        return r
    if sparse_ab:
        from . import sparse_attn
        variants = {"off": None, "full": 21, **{f"w{w}": w for w in SPARSE_WINDOWS}}
        times, clocks, outs = {k: [] for k in variants}, [], {}
        with torch.no_grad():
            for _ in range(3):
                for k, w in variants.items():
                    m.enable_sparse_attention(w or 0, enabled=w is not None)
                    times[k].append(_time(fwd, iters=2, warmup=1))
                    outs[k] = fwd().float()
                clocks.append(_sclk_mhz())
        m.enable_sparse_attention(0, enabled=False)
        r = {"kernel": "dit_forward_sparse_ab", "tflop": round(fl / 1e12, 1), "sclk_mhz": clocks,
             "full_equals_off": bool(torch.equal(outs["full"], outs["off"])),
             "rounds_ms": {k: [round(v, 2) for v in times[k]] for k in variants}}
        for k, w in variants.items():
            r[f"{k}_ms"] = round(sorted(times[k])[1], 2)
            if w is not None:
                r[f"{k}_density"] = _table_stats(*sparse_attn.frame_window_table(21, 1024, 21504, 21504, w), 21504,
                                                 21504)["density"]
                r[f"rel_l2_{k}_vs_off"] = round(((outs[k] - outs["off"]).norm() / outs["off"].norm()).item(), 5)
                r[f"ratio_{k}"] = round(r["off_ms"] / r[f"{k}_ms"], 4)
        return r
    if env_variants:  # "K=V" settings of one environment switch read per call by the library, interleaved
        import os
        times = {v: [] for v in env_variants}
        with torch.no_grad():
            for _ in range(3):
                for v in env_variants:
                    k, _, val = v.partition("=")
                    os.environ[k] = val
                    times[v].append(_time(fwd, iters=2, warmup=1))
                    os.environ.pop(k, None)
        r = {"kernel": "dit_forward_env_ab", "tflop": round(fl / 1e12, 1)}
        for v in env_variants:
            r[f"{v}_ms"] = round(sorted(times[v])[1], 2)
        return r
    if attn_variants:
        times = {v: [] for v in attn_variants}
        with torch.no_grad():
            for _ in range(3):
                for v in attn_variants:
                    m.attn_kernel = v
                    times[v].append(_time(fwd, iters=2, warmup=1))
        m.attn_kernel = 0
        r = {"kernel": "dit_forward_attn_ab", "tflop": round(fl / 1e12, 1)}
        for v in attn_variants:
            r[f"attn_v{v}_ms"] = round(sorted(times[v])[1], 2)
        return r
    with torch.no_grad():
        ms = _time(fwd, iters=iters, warmup=1)
    return {"kernel": "dit_forward", "ms": round(ms, 2), "tflop": round(fl / 1e12, 1),
            "tflops": round(fl / ms / 1e9, 1)}


if __name__ == "__main__":
    main(tuple(sys.argv[1:]) or ("gemm", "attn"))
