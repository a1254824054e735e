"""FlowUniPCMultistepScheduler (stableavatar_amd/scheduler.py) and tests/unipc_ref.py, the CPU statement of
sa_unipc_step, against the reference scheduler's goldens (tests/golden/unipc_small.npz, gen_unipc_golden.py), the
overlap rule, and the solver's order on an ODE with a closed-form solution.

The fp32 bound used throughout, 1e-5 max|x|, is derived, not measured: one step is at most 16 fp32 roundings (2 for m,
7 for the corrector form, 5 for the predictor form, and the coefficients' own casts) of terms bounded by about
8 max|x| (|v| up to ~4 max|x| on these inputs, the weights of each form sum to 1 in magnitude below 1.2):
16 * 2^-24 * 8 = 7.6e-6."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import unipc_ref as U  # noqa: E402
from gen_unipc_golden import TABLES, TRAJ, trajectory_inputs  # noqa: E402

from stableavatar_amd.scheduler import (FlowMatchEulerDiscreteScheduler, FlowUniPCMultistepScheduler,  # noqa: E402
                                        UniPCStep)

G = np.load(os.path.join(HERE, "golden", "unipc_small.npz"))
FP32_BOUND = 1e-5


def _sched(steps, shift=5.0):
    s = FlowUniPCMultistepScheduler(1000, shift=shift)
    s.set_timesteps(steps, device=None, mu=1)
    return s


def _bf16_ulps(a, b):
    """distance of two bf16 tensors in units in the last place (sign-magnitude bit patterns mapped to a line)"""
    def line(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


@pytest.mark.parametrize("steps,shift", TABLES)
def test_tables_equal_reference(steps, shift):
    """the fp32 sigma table (N + 1 entries, last 0, on the CPU) and the int64 timesteps, bit for bit"""
    s = _sched(steps, shift)
    tag = f"n{steps}_s{shift:g}"
    assert s.sigmas.dtype == torch.float32 and s.sigmas.device.type == "cpu" and s.timesteps.dtype == torch.int64
    assert np.array_equal(s.sigmas.numpy(), G[f"sigmas_{tag}"])
    assert np.array_equal(s.timesteps.numpy(), G[f"timesteps_{tag}"])
    assert s.order == 1 and s.num_inference_steps == steps and float(s.sigmas[-1]) == 0.0
    # not the Euler scheduler's table: that one places N points down to sigma_min
    e = FlowMatchEulerDiscreteScheduler(1000, shift=shift)
    e.set_timesteps(steps)
    assert not np.array_equal(e.sigmas.numpy(), s.sigmas.numpy())


def test_set_timesteps_shift_argument_and_reset():
    """set_timesteps' own shift replaces the constructor's on the per-call table only (sigma_max / sigma_min keep the
    constructor's), and set_timesteps starts a new trajectory"""
    s = _sched(20, 3.0)
    s.set_timesteps(20, shift=3.0)
    assert np.array_equal(s.sigmas.numpy(), G["sigmas_n20_s3"])
    s.set_timesteps(20, shift=5.0)
    assert not np.array_equal(s.sigmas.numpy(), G["sigmas_n20_s3"])
    assert not np.array_equal(s.sigmas.numpy(), G["sigmas_n20_s5"])
    s.step(torch.ones(2), s.timesteps[0], torch.ones(2))
    s.set_timesteps(4)
    assert s._step_index == 0 and s._last_sample is None


def _check_step(got32, ref32, worst):
    mx = ref32.abs().max().item()
    e = ((got32 - ref32).abs().max() / mx).item()
    ulps = _bf16_ulps(got32.bfloat16(), ref32.bfloat16())
    frac = (ulps != 0).float().mean().item()
    worst[0], worst[1], worst[2] = max(worst[0], e), max(worst[1], int(ulps.max())), max(worst[2], frac)
    assert e <= FP32_BOUND, e
    # the bf16 roundings agree unless the value sits within the fp32 error of a rounding boundary
    assert int(ulps.max()) <= 1 and frac <= 0.01, (int(ulps.max()), frac)


@pytest.mark.parametrize("name", list(TRAJ))
def test_scheduler_step_vs_reference_trajectory(name):
    """scheduler.step on the golden's inputs, fed back through bf16 as the golden's driver did: every returned
    fp32 sample within 1e-5 max|x| of the reference's, its bf16 rounding at most one ulp off on at most 1 %"""
    steps, shift, seed = TRAJ[name]
    s = _sched(steps, shift)
    x, vs = trajectory_inputs(steps, seed)
    worst = [0.0, 0, 0.0]
    for i in range(steps):
        r = s.step(vs[i], s.timesteps[i], x)[0]
        assert r.dtype == torch.float32
        _check_step(r, torch.from_numpy(G[name][i]), worst)
        x = torch.from_numpy(G[name][i]).bfloat16().float()  # the reference's own trajectory: errors do not add up
    print(f"{name}: scheduler.step max err / max|x| {worst[0]:.2e}, bf16 max ulps {worst[1]}, "
          f"off fraction {worst[2]:.4f}")


@pytest.mark.parametrize("name", list(TRAJ))
def test_unipc_ref_vs_reference_trajectory(name):
    """unipc_ref.unipc_step (one window over all frames, R = 1, state rotated as the pipeline does) with
    step_coefficients on the same trajectories, same bounds.  The fp32 sample before the bf16 store is
    unipc_ref.solve's; the stored bf16 pred is compared in ulps."""
    steps, shift, seed = TRAJ[name]
    s = _sched(steps, shift)
    x, vs = trajectory_inputs(steps, seed)
    lat = x.bfloat16()
    xh = m0 = m1 = None
    worst = [0.0, 0, 0.0]
    for i in range(steps):
        k = s.step_coefficients(i)
        ref = torch.from_numpy(G[name][i])
        sel = lambda t: None if t is None else t[0]  # noqa: E731
        xn32 = U.solve(lat[0].float(), vs[i][0], k, sel(xh), sel(m0), sel(m1))[0]
        _check_step(xn32[None], ref, worst)
        z = torch.full(lat.shape, float("nan"))
        pred, xh_new, m_new = U.unipc_step(lat, torch.zeros_like(lat), vs[i].bfloat16(), 0, k, 0.0, 0.0, xh=xh, m0=m0,
                                           m1=m1, xh_new=z, m_new=z)
        assert torch.equal(pred, xn32[None].bfloat16())
        lat, xh, m0, m1 = pred, xh_new, m_new, m0
        # continue from the reference's own sample where the rounding fell the other way
        lat = ref.bfloat16()
    print(f"{name}: unipc_ref max err / max|x| {worst[0]:.2e}, bf16 max ulps {worst[1]}, off fraction {worst[2]:.4f}")


@pytest.mark.parametrize("steps", [1, 2, 4, 20, 50])
def test_coefficients_finite_and_last_step_is_m(steps):
    """every coefficient finite at every step, the orders as the reference's counters give them, and at the last
    step (sigma_next = 0: lambda = +inf) x_next == m exactly"""
    s = _sched(steps)
    for i in range(steps):
        k = s.step_coefficients(i)
        assert isinstance(k, UniPCStep) and all(math.isfinite(v) for v in k[:8])
        assert all(float(np.float32(v)) == v for v in k[:8])  # fp32 values
        assert k.corrector == (0 if i == 0 else min(2, steps - (i - 1), i))
        assert k.predictor == min(2, steps - i, i + 1)
        # both forms reproduce a constant: with x = xhat = m0 = m1 = m the sample stays where it is
        assert abs(k.p0 + k.p1 + k.p2 - 1) < 1e-6
        if k.corrector:
            assert abs(k.c0 + k.c1 + k.c2 + k.c3 - 1) < 1e-6
    assert (k.p0, k.p1, k.p2, k.predictor) == (0.0, 1.0, 0.0, 1)
    g = torch.Generator().manual_seed(steps)
    x, v = torch.randn(64, generator=g), torch.randn(64, generator=g)
    xh, m0, m1 = (torch.randn(64, generator=g) for _ in range(3))
    xn, xc, m = U.solve(x, v, k, xh, m0, m1)
    assert torch.equal(xn, m)
    with pytest.raises(IndexError):
        s.step_coefficients(steps)


def test_overlap_rule_equals_solver_on_blended_velocity():
    """Two overlapping windows through unipc_ref.unipc_step (random old state, R = 3, a middle step: both orders 2)
    equal the single-tensor solver applied to the blended velocity: the written state (xc, m) within the fp32
    bound.  pred is stored as bf16, and so was the blend partner the first window left there: it is within the fp32
    bound plus those two roundings, each at most half a bf16 ulp = 2^-8 of its value (8 significant bits):
    2^-8 (|x_next| + (1 - w) |x_next of the first window|).  Outside the blended frames the later window overwrites
    the earlier."""
    T, C, HW, Fw, ov = 8, 3, (2, 3), 5, 2
    g = torch.Generator().manual_seed(3)
    shp = (1, C, T) + HW
    lat = torch.randn(shp, generator=g).bfloat16()
    xh, m0, m1 = (torch.randn(shp, generator=g) for _ in range(3))
    wins = [(0, 5, 5), (3, 8, 5)]
    noise = [torch.randn((3, C, Fw) + HW, generator=g).bfloat16() for _ in wins]
    wts = torch.tensor([0.25, 0.75])
    k = _sched(6).step_coefficients(3)
    assert (k.corrector, k.predictor) == (2, 2)
    pred, xh_new, m_new = torch.zeros_like(lat), torch.zeros(shp), torch.zeros(shp)
    for n, (s, e, pe) in zip(noise, wins):
        blend = s != 0
        pred, xh_new, m_new = U.unipc_step(lat, pred, n, s, k, 5.3, 3.1, ov if blend else 0, pe, wts if blend else None,
                                           blend, xh, m0, m1, xh_new, m_new)
    # the blended velocity on all T frames
    va, vb = (U.cfg_combine(n, 5.3, 3.1) for n in noise)
    v = torch.zeros((C, T) + HW)
    v[:, 0:5] = va
    v[:, 5:8] = vb[:, 2:]
    w = wts.view(1, ov, 1, 1)
    v[:, 3:5] = vb[:, :ov] * w + va[:, 3:5] * (1 - w)
    xn, xc, m = U.solve(lat[0].float(), v, k, xh[0], m0[0], m1[0])
    mx = max(t.abs().max().item() for t in (lat.float(), xh, m0, m1, v))
    e_xc = ((xh_new[0] - xc).abs().max() / mx).item()
    e_m = ((m_new[0] - m).abs().max() / mx).item()
    d = (pred[0].float() - xn).abs()
    print(f"overlap rule: xc err / max {e_xc:.2e}, m err / max {e_m:.2e}, pred err / max {(d.max() / mx).item():.2e}")
    assert e_xc <= FP32_BOUND and e_m <= FP32_BOUND, (e_xc, e_m)
    v_first = v.clone()
    v_first[:, 3:5] = va[:, 3:5]
    partner = torch.zeros_like(xn)
    partner[:, 3:5] = (1 - w) * U.solve(lat[0].float(), v_first, k, xh[0], m0[0], m1[0])[0][:, 3:5].abs()
    assert bool((d <= FP32_BOUND * mx + 2 ** -8 * (xn.abs() + partner)).all())
    # frames outside the blend are bit-equal to one window's own result
    assert torch.equal(m_new[0][:, [0, 1, 2, 5, 6, 7]], m[:, [0, 1, 2, 5, 6, 7]])


# ------------------------------------------------------------------------------------------------ order

def _ode_errors(N):
    """dx/dsigma = v(x, sigma) = a x + b sigma from sigma_0 down to 0 (a = 0.7, b = 1.3), solved over the UniPC
    scheduler's own sigma table at shift 5.0 (the shift the Wan configs sample with) by Euler and by UniPC
    (scheduler.step), fp32, no bf16 rounding; the closed form is
    x(sigma) = (x0 + b sigma0 / a + b / a^2) exp(a (sigma - sigma0)) - b sigma / a - b / a^2.  Returns the two
    max errors at sigma = 0."""
    a, b = 0.7, 1.3
    s = FlowUniPCMultistepScheduler(1000, shift=5.0)
    s.set_timesteps(N)
    sg = s.sigmas.double()
    x0 = torch.linspace(-2, 2, 16, dtype=torch.float64)
    s0 = sg[0].item()
    exact = (x0 + b * s0 / a + b / a ** 2) * math.exp(-a * s0) - b / a ** 2
    vel = lambda x, sig: (a * x.double() + b * sig).float()  # noqa: E731
    xe = x0.float()
    xu = x0.float()
    for i in range(N):
        xe = xe + (s.sigmas[i + 1] - s.sigmas[i]) * vel(xe, sg[i].item())
        xu = s.step(vel(xu, sg[i].item()), s.timesteps[i], xu)[0]
    return (xe.double() - exact).abs().max().item(), (xu.double() - exact).abs().max().item()


def test_unipc_has_the_higher_order():
    """on the analytic ODE, N in {10, 20, 40}: UniPC's error is below Euler's at every N and shrinks by a larger
    factor than Euler's each time N doubles (no absolute figure asserted).  The figures are in DESIGN.md, "UniPC
    sampler", with those of the unshifted table (shift 1.0), where UniPC's error is 26 times below Euler's at N = 10
    already but does not fall evenly from there to N = 20: this check is made on the shift the product uses."""
    err = {N: _ode_errors(N) for N in (10, 20, 40)}
    for N, (e, u) in err.items():
        print(f"ODE N={N}: Euler {e:.3e}, UniPC {u:.3e}")
        assert u < e, (N, e, u)
    for N in (10, 20):
        fe, fu = err[N][0] / err[2 * N][0], err[N][1] / err[2 * N][1]
        print(f"N {N} -> {2 * N}: Euler shrinks {fe:.2f}x, UniPC {fu:.2f}x")
        assert fu > fe, (N, fe, fu)


@pytest.mark.parametrize("kw", [dict(solver_order=3), dict(solver_order=1), dict(solver_type="bh1"),
                                dict(predict_x0=False), dict(prediction_type="epsilon"),
                                dict(lower_order_final=False), dict(final_sigmas_type="sigma_min"),
                                dict(thresholding=True), dict(use_dynamic_shifting=True),
                                dict(disable_corrector=[0]), dict(solver_p=object())])
def test_unsupported_arguments_raise(kw):
    with pytest.raises(NotImplementedError):
        FlowUniPCMultistepScheduler(1000, shift=5.0, **kw)
    FlowUniPCMultistepScheduler(1000, shift=5.0, solver_order=2, solver_type="bh2", disable_corrector=[])
