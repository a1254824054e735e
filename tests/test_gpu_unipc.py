"""sa_unipc_step and the UniPC denoise loop on the GPU: the kernel bit for bit against tests/unipc_ref.py (pinned to
the reference scheduler by test_unipc_cpu.py) in the bf16 latents and both fp32 state buffers, its argument checks,
pipe.denoise with a FlowUniPCMultistepScheduler against tests/golden/pipeline_unipc.npz, and the Euler path's launch
sequence, which the new dispatch must leave as it was."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import dit_ref as R  # noqa: E402
import unipc_ref as U  # noqa: E402
from golden_cases import PIPE, pipe_fixed_inputs  # noqa: E402

from stableavatar_amd import ops, synthetic  # noqa: E402
from stableavatar_amd._lib import KernelError, call  # noqa: E402
from stableavatar_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowUniPCMultistepScheduler  # noqa: E402

pytestmark = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")
G = lambda n: np.load(os.path.join(HERE, "golden", n))  # noqa: E731


def _sched(steps=4):
    s = FlowUniPCMultistepScheduler(1000, shift=5.0)
    s.set_timesteps(steps, mu=1)
    return s


# the four step kinds are the four steps of a 4-step schedule: (corrector, predictor) orders
KINDS = {"first": (0, (0, 1)), "second": (1, (1, 2)), "middle": (2, (2, 2)), "last": (3, (2, 1))}


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _state(seed):
    """old state xh / m0 / m1 and the content of the buffers the step writes (what a previous window left there: the
    blend reads it, and outside the window it must survive), fp32 [1, C, T, H, W]"""
    g = torch.Generator().manual_seed(100 + seed)
    shp = (1, R.FLOW_C, R.FLOW_T) + R.FLOW_HW
    return [torch.randn(shp, generator=g) for _ in range(5)]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("R_,start,Fw,overlap,prev_end,blend", R.FLOW_CASES)
def test_unipc_step(R_, start, Fw, overlap, prev_end, blend, kind):
    """bit-equal to unipc_ref.unipc_step in pred (bf16) and in the written xhat / m buffers (fp32), over dit_ref's
    sa_flow_step cases (C T HW = 5 * 30 * 21 elements, no multiple of 256; windows that wrap past T; a wrapping blend
    partner; overlap == Fw; R = 1 and 3) at each of the four step kinds; frames outside the window keep their
    content in all three outputs, the inputs stay as they were; and with every history buffer the step's orders
    leave unused filled with NaN (all three at the first step, m1 at corrector order 1) nothing changes"""
    i, orders = KINDS[kind]
    k = _sched().step_coefficients(i)
    assert (k.corrector, k.predictor) == orders
    lat, pred, noise, wts = R.flow_inputs(R_, Fw)
    xh, m0, m1, xh_new, m_new = _state(R_ + Fw)
    args = (start, k, 5.3, 3.1, overlap, prev_end)
    ref = U.unipc_step(lat, pred, noise, *args, wts, blend, xh, m0, m1, xh_new, m_new)
    unused = [k.corrector == 0, k.corrector == 0 and k.predictor == 1, k.corrector != 2]  # xh, m0, m1
    for poison in (False, True):
        old = [torch.full_like(t, NAN) if poison and u else t for t, u in zip((xh, m0, m1), unused)]
        ld, pd, nd = lat.to(dev), pred.to(dev), noise.to(dev)
        od = [t.to(dev) for t in old]
        xn_d, mn_d = xh_new.to(dev), m_new.to(dev)
        ops.unipc_step(ld, pd, nd, *args, wts.to(dev) if blend else None, blend, *od, xn_d, mn_d)
        torch.cuda.synchronize()
        for got, want in zip((pd.cpu(), xn_d.cpu(), mn_d.cpu()), ref):
            assert torch.equal(_bits(got), _bits(want)), (poison, (got.float() - want.float()).abs().max().item())
        outside = [f for f in range(R.FLOW_T) if f not in {(start + j) % R.FLOW_T for j in range(Fw)}]
        for got, init in zip((pd.cpu(), xn_d.cpu(), mn_d.cpu()), (pred, xh_new, m_new)):
            assert torch.equal(got[:, :, outside], init[:, :, outside])
        assert torch.equal(ld.cpu(), lat) and torch.equal(nd.cpu(), noise)
        for t, o in zip(od, old):
            assert torch.equal(_bits(t.cpu()), _bits(o))
        if not any(unused):
            break


def test_unipc_step_bad_arguments():
    """every refusal of sa_unipc_step returns SA_ERR_ARG without a launch: sa_flow_step's own (sizes, start, the
    blend conditions), a null state pointer the orders require, a corrector / predictor order outside {0, 1, 2} /
    {1, 2}, a non-finite scalar; the same calls with valid values pass"""
    f = torch.zeros(4096, device=dev)
    h = torch.zeros(4096, device=dev, dtype=torch.bfloat16)
    F_, H_, st = f.data_ptr(), h.data_ptr(), ops._stream()
    S = [F_ + 4096 * j for j in range(4)]  # four disjoint 1024-float state regions of f
    inf = float("inf")

    def unipc(C=1, T=4, Fw=2, HW=4, start=0, overlap=0, prev_end=0, blend=0, R_=1, sc=(0.5,) * 8, corrector=2,
              predictor=2, a=0.0, t=0.0, xh=S[0], m0=S[1], m1=S[2], xn=S[3], mn=S[3] + 512, lat=H_, pred=H_ + 2048,
              noise=H_ + 4096, w=F_):
        return (lat, pred, noise, R_, C, T, Fw, HW, start, *sc, corrector, predictor, a, t, overlap, prev_end, w,
                blend, xh, m0, m1, xn, mn, st)

    def sc(j, v):
        return tuple(v if i == j else 0.5 for i in range(8))

    bad = [unipc(C=0), unipc(T=0, Fw=0), unipc(Fw=0), unipc(Fw=-1), unipc(HW=0), unipc(start=-1), unipc(Fw=5),
           unipc(R_=2), unipc(lat=0), unipc(pred=0), unipc(noise=0),
           unipc(overlap=2, prev_end=1, blend=1), unipc(overlap=0, blend=1), unipc(overlap=3, prev_end=3, blend=1),
           unipc(overlap=2, prev_end=2, blend=1, w=0),
           unipc(xn=0), unipc(mn=0), unipc(xh=0), unipc(m0=0), unipc(m1=0),
           unipc(corrector=1, xh=0), unipc(corrector=1, m0=0), unipc(corrector=0, predictor=2, m0=0),
           unipc(corrector=3), unipc(corrector=-1), unipc(predictor=0), unipc(predictor=3),
           unipc(a=NAN), unipc(t=inf)]
    bad += [unipc(sc=sc(j, v)) for j in range(8) for v in (NAN, inf, -inf)]
    for args in bad:
        with pytest.raises(KernelError, match="bad argument"):
            call("sa_unipc_step", *args)
    torch.cuda.synchronize()
    good = [unipc(), unipc(overlap=2, prev_end=2, blend=1), unipc(corrector=1, m1=0),
            unipc(corrector=0, predictor=1, xh=0, m0=0, m1=0), unipc(corrector=0, xh=0, m1=0), unipc(R_=3, C=1)]
    for args in good:
        call("sa_unipc_step", *args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the loop

def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm()).item()


def psnr(a, b, peak):
    mse = ((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()) ** 2).mean().item()
    return 10 * math.log10(peak * peak / max(mse, 1e-30))


def _pipe(P, sched, with_vae=False):
    from stableavatar_amd.pipeline import WanI2VTalkingInferenceLongPipeline
    from stableavatar_amd.transformer import WanTransformer3DFantasyModel, param_shapes
    dcfg = P["dit"]
    dit = WanTransformer3DFantasyModel(**{k: v for k, v in dcfg.items() if k != "seed"})
    dit.load_state_dict(synthetic.fill_state_dict(param_shapes(dcfg), dcfg["seed"]))
    vae = None
    if with_vae:
        from stableavatar_amd.vae import AutoencoderKLWan, encoder_param_shapes
        from stableavatar_amd.vae import param_shapes as vae_shapes
        vae = AutoencoderKLWan(dim=P["vae"]["dim"])
        shapes = dict(vae_shapes(dim=P["vae"]["dim"]), **encoder_param_shapes(dim=P["vae"]["dim"]))
        vae.load_state_dict(synthetic.fill_state_dict(shapes, P["vae"]["seed"]), strict=True)
        vae = vae.cuda()
    return WanI2VTalkingInferenceLongPipeline(vae=vae, transformer=dit.cuda(), scheduler=sched)


def _denoise(pipe, P, sched, noise):
    from stableavatar_amd.pipeline import audio_window, window_schedule
    fx = pipe_fixed_inputs(P)
    T = fx["latents"].shape[2]
    fpb = (P["clip_length"] - 1) // 4 + 1
    feats = {}
    for (s, e, _) in window_schedule(T, fpb, P["overlap"]):
        a = synthetic.fake_wav2vec_features(fx["audio"][audio_window(s, e, T, 640, fx["audio"].shape[0])][None]).cuda()
        feats[(s, e)] = torch.cat([torch.zeros_like(a), a, a])
    ctx = [fx["neg_embeds"].cuda(), fx["neg_embeds"].cuda(), fx["pos_embeds"].cuda()]
    seq_len = math.ceil(P["width"] // 8 * P["height"] // 8 / 4 * fpb)
    with torch.no_grad():
        return pipe.denoise(noise, torch.from_numpy(G("pipeline_small.npz")["y"]).cuda(), ctx,
                            torch.cat([fx["clip"]] * 3).cuda(), feats, sched.timesteps, sched.sigmas,
                            clip_length=P["clip_length"], seq_len=seq_len, overlap=P["overlap"],
                            text_guide_scale=P["text_guide"], audio_guide_scale=P["audio_guide"])


def test_pipeline_unipc_vs_cpu_loop():
    """pipe.denoise under FlowUniPCMultistepScheduler on golden_cases.PIPE (two windows per step, overlap 2), 4 steps
    = all four step kinds, + decode, against unipc_ref.denoise over the CPU oracle DiT and the oracle VAE
    (pipeline_unipc.npz): the project's pipeline bars, latents rel-L2 < 3e-2 and video PSNR > 30 dB on [0, 1]; the
    caller's noise tensor is left as it was"""
    g = G("pipeline_unipc.npz")
    sched = _sched(int(g["steps"]))
    pipe = _pipe(PIPE, sched, with_vae=True)
    noise = pipe_fixed_inputs(PIPE)["latents"].cuda().bfloat16()
    keep = noise.clone()
    lat = _denoise(pipe, PIPE, sched, noise)
    with torch.no_grad():
        video = pipe.vae.decode_clip(lat[0].float(), post=True)[None]
    torch.cuda.synchronize()
    assert torch.equal(noise, keep), "denoise overwrote its input latents"
    e, p = rel(lat.float(), g["latents"]), psnr(video, g["video"].astype(np.float32), 1.0)
    print(f"UniPC pipeline, 4 steps: latents rel-L2 {e:.2e}, video PSNR {p:.1f} dB")
    assert e < 3e-2, e
    assert p > 30.0, p


def test_unipc_needs_matching_step_count():
    sched = _sched(4)
    pipe = _pipe(PIPE, sched)
    noise = pipe_fixed_inputs(PIPE)["latents"].cuda().bfloat16()
    ts = sched.timesteps
    sched.set_timesteps(3)
    sched.timesteps = ts
    with pytest.raises(ValueError, match="set_timesteps"):
        _denoise(pipe, PIPE, sched, noise)


def test_euler_launch_sequence_unchanged(monkeypatch):
    """with the Euler scheduler denoise makes the sa_flow_step launches it made before the sampler dispatch -- per
    step and window (latents, pred, noise, start, sigma_{i+1} - sigma_i as a Python float of the fp32 table, the two
    scales, overlap / prev_end / weights only when blending) on buffers that swap per step -- and no sa_unipc_step;
    the values those launches compute are pinned by the pipeline tests, which stay as they are"""
    from stableavatar_amd.pipeline import window_schedule
    sched = FlowMatchEulerDiscreteScheduler(1000, shift=5.0)
    sched.set_timesteps(PIPE["steps"], device="cuda")
    pipe = _pipe(PIPE, sched)
    seen = []
    real = ops.flow_step

    def rec(lat, pred, noise, start, dsigma, a, t, overlap, prev_end, weights, blend):
        seen.append((lat.data_ptr(), pred.data_ptr(), start, dsigma, a, t, overlap, prev_end, weights is None, blend))
        real(lat, pred, noise, start, dsigma, a, t, overlap, prev_end, weights, blend)

    monkeypatch.setattr(ops, "flow_step", rec)
    monkeypatch.setattr(ops, "unipc_step", lambda *a, **k: pytest.fail("sa_unipc_step under the Euler scheduler"))
    out = _denoise(pipe, PIPE, sched, pipe_fixed_inputs(PIPE)["latents"].cuda().bfloat16())
    torch.cuda.synchronize()
    sig = [float(s) for s in sched.sigmas]
    wins = window_schedule(6, 5, PIPE["overlap"])
    assert len(seen) == PIPE["steps"] * len(wins)
    bufs = (seen[0][0], seen[0][1])
    it = iter(seen)
    for i in range(PIPE["steps"]):
        for (s, e, pe) in wins:
            blend = s != 0 and i != 0
            assert next(it) == (bufs[i % 2], bufs[1 - i % 2], s, sig[i + 1] - sig[i], PIPE["audio_guide"],
                                PIPE["text_guide"], PIPE["overlap"] if blend else 0, pe, not blend, blend)
    assert out.data_ptr() == bufs[PIPE["steps"] % 2]
