"""Drift of the opt-in fp8 modes against the reference's own __call__: the comparison of
tests/test_gpu_fullsize.py::test_pipeline_call_vs_reference (2-layer DiT, 2 windows per step) at 5 and 50 steps with
the modes off, fp8 attention on, fp8 attention + fp8 FFN on, fp8 q/k/v alone, those three on, fp8 self-O alone and all
four on, all in one run.  One JSON line per (steps, mode): latents rel-L2 and video PSNR against the golden record.
python scripts/fp8_drift.py [out.jsonl [mode ...]]  (no mode named: every mode)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main(out_path, only=()):
    from golden_cases import PIPE_STEPS, ref_image
    from test_gpu_fullsize import _drop_in_pipeline, psnr, rel
    modes = {"off": (False, False, False, False), "fp8_attn": (True, False, False, False),
             "fp8_attn_ffn": (True, True, False, False), "fp8_qkv": (False, False, True, False),
             "fp8_attn_ffn_qkv": (True, True, True, False), "fp8_o": (False, False, False, True),
             "fp8_attn_ffn_qkv_o": (True, True, True, True)}
    unknown = set(only) - set(modes)
    if unknown:
        raise SystemExit(f"unknown modes {sorted(unknown)}; known: {list(modes)}")
    if only:
        modes = {k: v for k, v in modes.items() if k in only}
    with open(out_path, "w") as f:
        for steps in (5, 50):
            P = PIPE_STEPS[steps]
            g = np.load(os.path.join(ROOT, "tests", "golden", f"pipeline_s{steps:02d}.npz"))
            pipe, fx = _drop_in_pipeline(P)
            path = ref_image()
            kw = dict(num_frames=P["clip_length"], height=P["height"], width=P["width"], guidance_scale=6.0,
                      num_inference_steps=P["steps"], latents=fx["latents"], text_guide_scale=P["text_guide"],
                      audio_guide_scale=P["audio_guide"], vocal_input_values=fx["audio"].numpy(), fps=25, sr=16000,
                      cond_file_path=path, overlap_window_length=P["overlap"], clip_length=P["clip_length"])
            gv = g["video"].astype(np.float32)
            frames = list(g["video_frames"]) if "video_frames" in g else list(range(gv.shape[2]))
            for name, (attn, ffn, qkv, o) in modes.items():
                pipe.transformer.enable_fp8_attention(attn)
                pipe.transformer.enable_fp8_ffn(ffn)
                pipe.transformer.enable_fp8_qkv(qkv)
                pipe.transformer.enable_fp8_o(o)
                with torch.no_grad():
                    lat = pipe("pos prompt", negative_prompt="", output_type="latent", **kw).videos
                    video = pipe("pos prompt", negative_prompt="", **kw).videos
                torch.cuda.synchronize()
                r = {"steps": steps, "forwards": 2 * steps, "mode": name,
                     "latents_rel": rel(lat.float().cpu(), g["latents"]),
                     "video_psnr_db": psnr(video[:, :, frames].float(), gv, 1.0)}
                print(json.dumps(r), flush=True)
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "fp8_drift.jsonl", tuple(sys.argv[2:]))
