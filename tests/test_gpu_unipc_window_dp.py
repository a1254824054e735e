"""Window-parallel denoising under the UniPC sampler: the sampler step runs replicated on every rank after the noise
predictions are gathered, so 2 ranks x 3 windows per step over gloo (the first case of test_gpu_window_dp.py, whose
inputs and process pattern this reuses) must reproduce the single-GPU loop bit for bit -- latents and, with them, the
solver state every later step was computed from.  4 steps: all four step kinds."""
import math
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

from mp_util import collect  # noqa: E402
from test_gpu_window_dp import _inputs, _rendezvous_file  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, T, CLIP, OVERLAP, WORLD = 4, 9, 17, 2, 2


def _run(pipe, window_parallel):
    from stableavatar_amd import synthetic
    from stableavatar_amd.pipeline import audio_window, window_schedule
    fpb = (CLIP - 1) // 4 + 1
    lat, y, ctx, clip, audio = _inputs(T, CLIP)
    feats = {}
    for (s, e, _) in window_schedule(T, fpb, OVERLAP):
        a = synthetic.fake_wav2vec_features(audio[audio_window(s, e, T, 640, audio.shape[0])][None])
        feats[(s, e)] = torch.cat([torch.zeros_like(a), a, a]).cuda()
    sched = pipe.scheduler
    sched.set_timesteps(STEPS, device="cuda", mu=1)
    pipe.window_group = None
    if window_parallel:
        pipe.enable_window_parallel()
    with torch.no_grad():
        out = pipe.denoise(lat.cuda(), y.cuda(), [c.cuda() for c in ctx], clip.cuda(), feats, sched.timesteps,
                           sched.sigmas, clip_length=CLIP, seq_len=math.ceil(8 * 8 / 4 * fpb), overlap=OVERLAP,
                           text_guide_scale=3.0, audio_guide_scale=5.0)
    torch.cuda.synchronize()
    return out.cpu()


def _worker(rank, world, port, qret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    import torch.distributed as dist
    from golden_cases import PIPE
    from stableavatar_amd import synthetic
    from stableavatar_amd.pipeline import WanI2VTalkingInferenceLongPipeline
    from stableavatar_amd.scheduler import FlowUniPCMultistepScheduler
    from stableavatar_amd.transformer import WanTransformer3DFantasyModel, param_shapes
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        dcfg = PIPE["dit"]
        dit = WanTransformer3DFantasyModel(**{k: v for k, v in dcfg.items() if k != "seed"})
        dit.load_state_dict(synthetic.fill_state_dict(param_shapes(dcfg), dcfg["seed"]))
        pipe = WanI2VTalkingInferenceLongPipeline(transformer=dit.cuda(),
                                                  scheduler=FlowUniPCMultistepScheduler(1000, shift=5.0))
        single = _run(pipe, False)
        par = _run(pipe, True)
        qret.put((rank, bool(torch.equal(single, par)), float((single.float() - par.float()).abs().max()),
                  bool(torch.isfinite(par.float()).all())))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_unipc_window_parallel_bit_exact():
    from stableavatar_amd.pipeline import window_schedule
    assert len(window_schedule(T, (CLIP - 1) // 4 + 1, OVERLAP)) == 3
    ctx = mp.get_context("spawn")
    qret = ctx.Queue()
    port = _rendezvous_file()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, qret)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = collect(procs, qret, WORLD, timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert len(res) == WORLD
    for rank, same, mx, finite in res:
        assert same and finite, (rank, mx, finite)
