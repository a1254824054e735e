"""Goldens of the reference's FlowUniPCMultistepScheduler (wan/utils/fm_solvers_unipc.py, imported with the diffusers
stand-ins of _refstub.py plus the few more names that module imports).  Run here only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_unipc_golden.py

Writes tests/golden/unipc_small.npz: the sigma / timestep tables of set_timesteps for (steps, shift) in TABLES, and
one 6-step and one 4-step trajectory of scheduler.step on a [1, 4, 3, 4, 4] sample with seeded model outputs, in
fp32; the driver rounds each returned sample to bf16 before it feeds it back (the pipeline's latents are bf16), and
the stored samples are the returned fp32 values before that rounding.  Only data is stored.  The tests import
TABLES, TRAJ and trajectory_inputs from here (the reference is touched only inside main()).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

TABLES = [(4, 5.0), (20, 5.0), (50, 5.0), (20, 3.0)]
TRAJ = {"traj6": (6, 5.0, 11), "traj4": (4, 5.0, 12)}  # name -> (steps, shift, seed)
SHAPE = (1, 4, 3, 4, 4)


def _install_scheduler_names():
    """the diffusers names fm_solvers_unipc.py imports beyond _refstub's"""
    su = types.ModuleType("diffusers.schedulers.scheduling_utils")

    class SchedulerOutput:
        def __init__(self, prev_sample):
            self.prev_sample = prev_sample

    su.KarrasDiffusionSchedulers = ()
    su.SchedulerMixin = type("SchedulerMixin", (), {})
    su.SchedulerOutput = SchedulerOutput
    sys.modules["diffusers.schedulers.scheduling_utils"] = su
    ut = sys.modules["diffusers.utils"]
    ut.deprecate = lambda *a, **k: None
    ut.is_scipy_available = lambda: False


def trajectory_inputs(steps, seed):
    """x0 [SHAPE] as bf16 values in fp32, and one model output per step (fp32 holding bf16 values, as the DiT's)"""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(SHAPE, generator=g).bfloat16().float()
    vs = [torch.randn(SHAPE, generator=g).bfloat16().float() for _ in range(steps)]
    return x0, vs


def main():
    import _refstub
    _refstub.install()
    _install_scheduler_names()
    from wan.utils.fm_solvers_unipc import FlowUniPCMultistepScheduler
    out = {}
    for steps, shift in TABLES:
        s = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=shift)
        s.set_timesteps(steps, mu=1)
        tag = f"n{steps}_s{shift:g}"
        assert s.sigmas.dtype == torch.float32 and s.timesteps.dtype == torch.int64
        out[f"sigmas_{tag}"] = s.sigmas.numpy().copy()
        out[f"timesteps_{tag}"] = s.timesteps.numpy().copy()
        print(tag, s.sigmas.numpy(), s.timesteps.numpy())
    for name, (steps, shift, seed) in TRAJ.items():
        s = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=shift)
        s.set_timesteps(steps, mu=1)
        s.set_begin_index(0)  # count steps from 0 (no look-up of the truncated timesteps)
        x, vs = trajectory_inputs(steps, seed)
        ret = []
        for i, t in enumerate(s.timesteps):
            r = s.step(vs[i], t, x, return_dict=False)[0]
            assert r.dtype == torch.float32
            ret.append(r.numpy().copy())
            x = r.bfloat16().float()
        out[name] = np.stack(ret)
        print(name, "max|x|", float(np.abs(out[name]).max()))
    np.savez_compressed(os.path.join(HERE, "unipc_small.npz"), **out)


if __name__ == "__main__":
    main()
