"""Expected latents and video of the UniPC denoise loop on golden_cases.PIPE (overlap 2: windows (0,5),(3,6)) at 4
steps -- the fewest that hold all four step kinds (first: no corrector, order-1 predictor; second: order-1 corrector;
middle: both order 2; last: order-1 predictor onto sigma 0) -- from tests/unipc_ref.denoise over the CPU oracle DiT
(oracle/dit.py, pinned to the reference's goldens by tests/test_oracle_golden.py) and the oracle VAE decode.  The
reference has no UniPC loop over overlapping windows to run ("UniPC sampler").  CPU only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_unipc_pipeline_golden.py

Writes tests/golden/pipeline_unipc.npz: latents (fp32 holding bf16 values) and video (fp16, [0, 1])."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from golden_cases import PIPE, pipe_fixed_inputs  # noqa: E402

import unipc_ref  # noqa: E402
from oracle import dit as odit  # noqa: E402
from oracle import vae as ovae  # noqa: E402
from stableavatar_amd import synthetic  # noqa: E402
from stableavatar_amd.scheduler import FlowUniPCMultistepScheduler  # noqa: E402

STEPS = 4


def main():
    P = PIPE
    Pd = synthetic.fill_state_dict(odit.param_shapes(P["dit"]), P["dit"]["seed"])
    Pv = synthetic.fill_state_dict(ovae.param_shapes(dim=P["vae"]["dim"]), P["vae"]["seed"])
    fx = pipe_fixed_inputs(P)
    y = torch.from_numpy(np.load(os.path.join(HERE, "pipeline_small.npz"))["y"])  # the reference's VAE-encoded y
    ctx = [fx["neg_embeds"], fx["neg_embeds"], fx["pos_embeds"]]

    def dit(x, t, context, seq_len, yy, clip_fea, vocal, n):
        return odit.forward(Pd, P["dit"], x, t, context, seq_len, clip_fea, yy.to(torch.bfloat16).float(), vocal, n)

    enc = lambda s: synthetic.fake_wav2vec_features(torch.as_tensor(s)[None])  # noqa: E731
    with torch.no_grad():
        lat = unipc_ref.denoise(dit, fx["latents"].to(torch.bfloat16).float(), y, ctx, torch.cat([fx["clip"]] * 3),
                                fx["audio"], enc, FlowUniPCMultistepScheduler(1000, shift=5.0),
                                num_inference_steps=STEPS, clip_length=P["clip_length"], num_frames=P["clip_length"],
                                height=P["height"], width=P["width"], overlap=P["overlap"],
                                text_guide_scale=P["text_guide"], audio_guide_scale=P["audio_guide"])
        video = (ovae.decode(Pv, lat, dim=P["vae"]["dim"]) / 2 + 0.5).clamp(0, 1)
    print("latents", tuple(lat.shape), float(lat.abs().max()), "video", tuple(video.shape))
    np.savez_compressed(os.path.join(HERE, "pipeline_unipc.npz"), latents=lat.numpy(),
                        video=video.numpy().astype(np.float16), steps=STEPS)


if __name__ == "__main__":
    main()
