"""`inference.py --sampler unipc` end to end on test_gpu_inference_cli.py's synthetic model tree: the command line
hands the pipeline a FlowUniPCMultistepScheduler built from the config's scheduler_kwargs, __call__ drives it
(set_timesteps with the pipeline's mu=1 and device, int64 timesteps into the DiT) over 4 steps x 2 windows through
sa_unipc_step and no sa_flow_step, and the written video is finite and in range.  Without the flag the scheduler is
the Euler one (that run is test_gpu_inference_cli.py's)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_gpu_inference_cli import _write_tree  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(600)
def test_inference_cli_sampler_unipc(tmp_path, monkeypatch):
    from stableavatar_amd import _lib, inference
    from stableavatar_amd.pipeline import WanI2VTalkingInferenceLongPipeline
    from stableavatar_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowUniPCMultistepScheduler
    assert inference.parse_args(["--pretrained_model_name_or_path", "x"]).sampler == "euler"
    root = str(tmp_path)
    _write_tree(root)
    out_dir = os.path.join(root, "output")
    calls, launches = [], []
    orig = WanI2VTalkingInferenceLongPipeline.__call__

    def spy(self, *a, **kw):
        out = orig(self, *a, **kw)
        calls.append((self, out.videos.detach().float().cpu().clone()))
        return out

    real_call = _lib.call

    def count(name, *args):
        if name in ("sa_flow_step", "sa_unipc_step"):
            launches.append(name)
        return real_call(name, *args)

    monkeypatch.setattr(WanI2VTalkingInferenceLongPipeline, "__call__", spy)
    from stableavatar_amd import ops
    monkeypatch.setattr(ops, "call", count)
    inference.main(["--config_path", os.path.join(root, "config.yaml"), "--pretrained_model_name_or_path", root,
                    "--transformer_path", os.path.join(root, "transformer3d-square.pt"),
                    "--pretrained_wav2vec_path", os.path.join(root, "wav2vec"),
                    "--validation_reference_path", os.path.join(root, "reference.png"),
                    "--validation_driven_audio_path", os.path.join(root, "audio.wav"), "--output_dir", out_dir,
                    "--validation_prompts", "a woman is singing", "--seed", "42", "--sample_steps", "4",
                    "--width", "64", "--height", "64", "--overlap_window_length", "2", "--clip_sample_n_frames", "17",
                    "--sample_text_guide_scale", "3.0", "--sample_audio_guide_scale", "5.0", "--sampler", "unipc"])
    assert len(calls) == 1
    pipe, video = calls[0]
    s = pipe.scheduler
    assert isinstance(s, FlowUniPCMultistepScheduler) and not isinstance(s, FlowMatchEulerDiscreteScheduler)
    assert s.shift == 5.0 and s.num_inference_steps == 4 and s.timesteps.dtype == torch.int64
    assert s.sigmas.device.type == "cpu"
    assert launches == ["sa_unipc_step"] * (4 * 2)
    assert video.shape == (1, 3, 21, 64, 64) and bool(torch.isfinite(video).all())
    assert float(video.min()) >= 0 and float(video.max()) <= 1 and float(video.std()) > 0
    if os.path.exists(os.path.join(out_dir, "video.npy")):
        assert np.array_equal(np.load(os.path.join(out_dir, "video.npy")), video.numpy())
