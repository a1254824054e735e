"""FlowMatchEulerDiscreteScheduler as used by the reference pipeline (diffusers 0.30.1, constructed
at inference.py:491-496 with wan_civitai.yaml shift 5.0 / 1000 train steps).  Host-side bookkeeping
only: the step arithmetic itself runs fused in the sa_flow_step kernel.  diffusers is not installed
offline, so this restates its published algorithm (parity of the sigma table: see DESIGN.md).

FlowUniPCMultistepScheduler: the reference tree's second-order multistep solver (wan/utils/fm_solvers_unipc.py) in the
one configuration Wan samples with; its arithmetic runs fused in sa_unipc_step ("UniPC sampler")."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch


class FlowMatchEulerDiscreteScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, shift=1.0, use_dynamic_shifting=False, base_shift=0.5,
                 max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, **_):
        if use_dynamic_shifting:
            raise NotImplementedError("dynamic shifting is not used by the StableAvatar configs")
        N = num_train_timesteps
        s = torch.from_numpy(np.linspace(1, N, N, dtype=np.float32)[::-1].copy() / N)
        s = shift * s / (1 + (shift - 1) * s)
        self.num_train_timesteps, self.shift = N, shift
        self.timesteps = s * N
        self.sigmas = s
        self.sigma_min, self.sigma_max = s[-1].item(), s[0].item()
        self._step_index = None
        self.config = type("cfg", (), dict(num_train_timesteps=N, shift=shift, use_dynamic_shifting=False))()

    def set_timesteps(self, num_inference_steps=None, device=None, sigmas=None, mu=None, **_):
        if sigmas is None:
            t = np.linspace(self.sigma_max * self.num_train_timesteps, self.sigma_min * self.num_train_timesteps,
                            num_inference_steps)
            sigmas = t / self.num_train_timesteps
        sigmas = self.shift * np.asarray(sigmas) / (1 + (self.shift - 1) * np.asarray(sigmas))
        s = torch.from_numpy(sigmas).to(dtype=torch.float32, device=device)
        self.timesteps = s * self.num_train_timesteps
        self.sigmas = torch.cat([s, torch.zeros(1, device=s.device)])
        self.num_inference_steps = len(s)
        self._step_index = None

    def step(self, model_output, timestep, sample, return_dict=False, **_):
        """Reference semantics (for callers that step manually); the pipeline uses sa_flow_step."""
        if self._step_index is None:
            idx = (self.timesteps == timestep).nonzero()
            self._step_index = idx[1 if len(idx) > 1 else 0].item()
        out = sample.float() + (self.sigmas[self._step_index + 1] - self.sigmas[self._step_index]) * model_output
        self._step_index += 1
        return (out.to(model_output.dtype),)


class UniPCStep(NamedTuple):
    """fp32 scalars of one FlowUniPCMultistepScheduler step as sa_unipc_step takes them:
    m = x - sigma v;  xc = c0 xhat + c1 m0 + c2 m1 + c3 m (corrector > 0, else xc = x);  x_next = p0 xc + p1 m + p2 m0.
    corrector: 0 off, else its order (1 leaves c2 / m1 unused);  predictor: its order (1 leaves p2 / m0 unused)."""
    sigma: float
    c0: float
    c1: float
    c2: float
    c3: float
    p0: float
    p1: float
    p2: float
    corrector: int
    predictor: int


def _f32(v):
    return float(np.float32(v))


class FlowUniPCMultistepScheduler:
    """The reference's second-order multistep solver for flow matching (wan/utils/fm_solvers_unipc.py, from diffusers
    0.31 scheduling_unipc_multistep.py) in the one configuration Wan samples with: solver_order 2, bh2, predict_x0,
    flow_prediction, lower_order_final, final sigma 0, corrector at every step after the first.  Host-side
    bookkeeping: the pipeline takes step_coefficients(i) and runs the arithmetic fused in sa_unipc_step.

    Its sigma table is not the Euler scheduler's: linspace(sigma_max, sigma_min, N + 1)[:-1] (not N points down to
    sigma_min), shifted, then 0; timesteps are the sigmas * num_train_timesteps truncated to int64; sigmas stay on
    the CPU."""
    order = 1

    def __init__(self, num_train_timesteps=1000, solver_order=2, prediction_type="flow_prediction", shift=1.0,
                 use_dynamic_shifting=False, thresholding=False, dynamic_thresholding_ratio=0.995,
                 sample_max_value=1.0, predict_x0=True, solver_type="bh2", lower_order_final=True,
                 disable_corrector=(), solver_p=None, timestep_spacing="linspace", steps_offset=0,
                 final_sigmas_type="zero"):
        if use_dynamic_shifting:
            raise NotImplementedError("dynamic shifting is not used by the StableAvatar configs")
        if thresholding:
            raise NotImplementedError("dynamic thresholding is for pixel-space models, not the Wan latents")
        if solver_order != 2:
            raise NotImplementedError(f"solver_order {solver_order}: only the order-2 solver Wan samples with is built")
        if solver_type != "bh2":
            raise NotImplementedError(f"solver_type {solver_type!r}: only bh2 is built")
        if prediction_type != "flow_prediction":
            raise NotImplementedError(f"prediction_type {prediction_type!r}: the Wan models predict the flow")
        if not predict_x0:
            raise NotImplementedError("predict_x0=False (the noise-prediction form) is not built")
        if not lower_order_final:
            raise NotImplementedError("lower_order_final=False: the last step ends at sigma 0, where only order 1 is "
                                      "finite")
        if final_sigmas_type != "zero":
            raise NotImplementedError(f"final_sigmas_type {final_sigmas_type!r}: only a final sigma of 0 is built")
        if len(disable_corrector):
            raise NotImplementedError("disable_corrector: the corrector runs at every step after the first")
        if solver_p is not None:
            raise NotImplementedError("solver_p: another predictor under UniC is not built")
        N = num_train_timesteps
        s = torch.from_numpy(1.0 - np.linspace(1, 1 / N, N)[::-1].copy()).to(dtype=torch.float32)
        s = shift * s / (1 + (shift - 1) * s)
        self.num_train_timesteps, self.shift = N, shift
        self.sigmas = s
        self.timesteps = s * N
        self.sigma_min, self.sigma_max = s[-1].item(), s[0].item()
        self.num_inference_steps = None
        self.config = type("cfg", (), dict(num_train_timesteps=N, shift=shift, use_dynamic_shifting=False,
                                           solver_order=2, solver_type="bh2", prediction_type="flow_prediction",
                                           predict_x0=True, lower_order_final=True, final_sigmas_type="zero"))()
        self._reset()

    def _reset(self):
        self._step_index = 0
        self._last_sample = None      # the previous step's corrected sample (fp32)
        self._m = [None, None]        # converted model outputs: [previous step's, the one before]

    def set_timesteps(self, num_inference_steps=None, device=None, sigmas=None, mu=None, shift=None):
        """mu is accepted and ignored (it belongs to dynamic shifting; the pipeline passes mu=1 to every scheduler)."""
        if sigmas is None:
            sigmas = np.linspace(self.sigma_max, self.sigma_min, num_inference_steps + 1).copy()[:-1]
        if shift is None:
            shift = self.shift
        sigmas = np.asarray(sigmas)
        sigmas = shift * sigmas / (1 + (shift - 1) * sigmas)
        timesteps = sigmas * self.num_train_timesteps
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(timesteps).to(device=device, dtype=torch.int64)
        self.num_inference_steps = len(timesteps)
        self._reset()

    def step_orders(self, i):
        """(corrector order at step i (0: off), predictor order at step i): the predictor takes min(solver_order,
        steps left, steps taken + 1), the corrector the order of the predictor that produced its sample."""
        N = self.num_inference_steps
        pred = lambda j: min(2, N - j, j + 1)  # noqa: E731
        return (pred(i - 1) if i >= 1 else 0), pred(i)

    def step_coefficients(self, i) -> UniPCStep:
        """The weights of step i's two linear forms (UniPCStep), computed in float64 from the fp32 sigma table and
        each cast to fp32.  With alpha = 1 - sigma, lambda = log alpha - log sigma, h = lambda_t - lambda_s, hh = -h,
        phi = B = expm1(hh) (bh2), r = (lambda_before_s - lambda_s) / h:
          corrector (s = i - 1, t = i):   xc = sigma_t / sigma_s xhat - alpha_t phi m0
                                               - alpha_t B (rho_1 (m1 - m0) / r + rho_last (m - m0))
          predictor (s = i, t = i + 1):   x_next = sigma_t / sigma_s xc - alpha_t phi m - alpha_t B 0.5 (m0 - m) / r
        rho = [0.5] at corrector order 1, the solution of [[1, 1], [r, 1]] rho = b at order 2.  At the last step
        sigma_t = 0, lambda_t = +inf and phi = B = expm1(-inf) = -1 with alpha_t = 1: x_next = m, returned as
        (p0, p1, p2) = (0, 1, 0) without forming an infinity."""
        N = self.num_inference_steps
        if N is None:
            raise ValueError("run set_timesteps first")
        if not 0 <= i < N:
            raise IndexError(f"step {i} of {N}")
        sg = [float(v) for v in self.sigmas]  # fp32 values, exact in float64
        lam = lambda j: math.log(1 - sg[j]) - math.log(sg[j])  # noqa: E731
        corr, pord = self.step_orders(i)
        c0 = c1 = c2 = c3 = 0.0
        if corr:
            a_t = 1 - sg[i]
            h = lam(i) - lam(i - 1)
            hh = -h
            phi = B = math.expm1(hh)
            k1 = phi / hh - 1
            b0 = k1 / B
            if corr == 2:
                r = (lam(i - 2) - lam(i - 1)) / h
                b1 = (k1 / hh - 0.5) * 2 / B
                rho1 = (b0 - b1) / (1 - r)
                rho_last = b0 - rho1
                c2 = -a_t * B * rho1 / r
            else:
                rho_last = 0.5
            c0 = sg[i] / sg[i - 1]
            c3 = -a_t * B * rho_last
            c1 = -a_t * phi - c2 - c3
        if sg[i + 1] == 0.0:
            p0, p1, p2 = 0.0, 1.0, 0.0
        else:
            a_t = 1 - sg[i + 1]
            h = lam(i + 1) - lam(i)
            phi = B = math.expm1(-h)
            p0 = sg[i + 1] / sg[i]
            p2 = -a_t * B * 0.5 / ((lam(i - 1) - lam(i)) / h) if pord == 2 else 0.0
            p1 = -a_t * phi - p2
        out = UniPCStep(*(_f32(v) for v in (sg[i], c0, c1, c2, c3, p0, p1, p2)), corr, pord)
        if not all(math.isfinite(v) for v in out[:8]):
            raise FloatingPointError(f"non-finite UniPC coefficient at step {i}: {out}")
        return out

    def step(self, model_output, timestep, sample, return_dict=False, **_):
        """Reference semantics on torch tensors (for callers that step manually; the pipeline uses sa_unipc_step):
        the two linear forms of step_coefficients in fp32, in the kernel's order; returns the sample's dtype.
        Steps are counted from set_timesteps; `timestep` is not looked up.  The reference finds its first index by
        searching the int-truncated timesteps, which repeat at high step counts, and then takes the second match
        (index_for_timestep): it would start such a schedule one sigma late.  The counter does not."""
        i = self._step_index
        k = self.step_coefficients(i)
        f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
        x = sample.float()
        m = x - f(k.sigma) * model_output.float()
        m0, m1 = self._m
        xc = x
        if k.corrector:
            xc = f(k.c0) * self._last_sample + f(k.c1) * m0
            if k.corrector == 2:
                xc = xc + f(k.c2) * m1
            xc = xc + f(k.c3) * m
        xn = f(k.p0) * xc + f(k.p1) * m
        if k.predictor == 2:
            xn = xn + f(k.p2) * m0
        self._last_sample, self._m = xc, [m, m0]
        self._step_index += 1
        return (xn.to(sample.dtype),)
