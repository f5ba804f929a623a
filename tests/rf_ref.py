"""CPU restatement (test infrastructure, not product code) of the reference's rectified-flow pieces -- ``ReFlow.denoise_fn`` in both modes
(src/models/components/diffusion.py:367-418), ``RFEDMSchedule`` (scheduler.py:105-120) and the ``ReflowEulerSampler`` loop (sampler_rf.py:24-70) --
written independently of audiodiffuser_amd's plugin classes so that the device and the plugins are held to something they do not share code
with.  tools/gen_golden_rf.py pins these functions to the reference's classes when it writes tests/golden/rf_golden.npz.

Everything runs in the dtype of the state it is given: torch.float32 is the reference's arithmetic, torch.float64 the same formulas at double
precision on the same fp32 inputs (what a device result is compared with, and what the conditioning of a run is measured against).  ``rows``
takes the dtype as an argument, like tests/precond_ref.py."""
from __future__ import annotations

from typing import Callable, Optional

import torch


# ---- schedules at the reference's signatures ---------------------------------------------------------------------------------------
def linear_schedule(start=1.0, end=0.0, num_steps=50):
    return torch.linspace(start, end, num_steps)


def rfedm_schedule(start=1.0, end=0.0, num_steps=50):
    assert start <= 1.0 and end >= 0.0
    t = torch.linspace(start, end, num_steps)
    return t / (1 - t)


# ---- rows -------------------------------------------------------------------------------------------------------------------------
def rows(for_edm: bool, sigmas: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """[n, 4] = (c_in, c_noise, c_skip, c_out) per sigma, the device's row layout: (1, s, 0, 1) for the raw velocity, and with ``for_edm``
    (1 - t, t, 1 - t, -t) at t = s / (s + 1).  ``sigmas`` are fp32 values; with float64 they are widened first and every operation runs in double."""
    s = sigmas.to(dtype)
    if not for_edm:
        return torch.stack([torch.ones_like(s), s, torch.zeros_like(s), torch.ones_like(s)], dim=1)
    t = s / (s + 1)
    return torch.stack([1 - t, t, 1 - t, -t], dim=1)


# ---- denoiser ---------------------------------------------------------------------------------------------------------------------
def denoise(for_edm: bool, net: Callable[..., torch.Tensor], x_noisy: torch.Tensor, sigma=None, sigmas: Optional[torch.Tensor] = None,
            cond_scale: float = 1.0) -> torch.Tensor:
    """``ReFlow(for_edm).denoise_fn(..., inference=True)`` around ``net(x, time[, cond_drop_prob])`` in the dtype of ``x_noisy``, as written in
    the reference (x (1 - t), then x_in - v t), with the per-sample factors shaped [B, 1, ...] -- what the reference gives sample by sample."""
    assert (sigma is None) ^ (sigmas is None)
    b, dt = x_noisy.shape[0], x_noisy.dtype
    if sigmas is None:
        sigmas = torch.full((b,), float(sigma), dtype=torch.float32)
    t = sigmas.to(torch.float32).to(dt)
    if for_edm:
        t = t / (t + 1)
        te = t.view(b, *((1,) * (x_noisy.ndim - 1)))
        x_noisy = x_noisy * (1 - te)
    if cond_scale == 1.0:
        v = net(x_noisy, t)
    else:
        v = net(x_noisy, t, cond_drop_prob=0.0)
        null = net(x_noisy, t, cond_drop_prob=1.0)
        v = null + (v - null) * cond_scale
    return x_noisy - v * te if for_edm else v


def make_fn(for_edm: bool, net: Callable[..., torch.Tensor], cond_scale: float = 1.0) -> Callable:
    """The closure the sampler restatements call: fn(x, sigma=<0-dim tensor>) or fn(x, sigmas=[B])."""
    return lambda x, sigma=None, sigmas=None: denoise(for_edm, net, x, sigma=sigma, sigmas=sigmas, cond_scale=cond_scale)


# ---- sampler ----------------------------------------------------------------------------------------------------------------------
def euler_sampler(noise: torch.Tensor, fn: Callable, sigmas: torch.Tensor, num_steps: int, use_heun: bool = True, clamp: bool = True) -> torch.Tensor:
    """ReflowEulerSampler.forward (sampler_rf.py:54-70) and .step (:24-52): ``fn`` returns the velocity.  The sigma arithmetic stays on 0-dim
    tensors, as in the reference, in the dtype of ``noise``.  ``clamp=False`` returns the state before the closing clamp(-1, 1)."""
    sig = sigmas.to(noise.dtype)
    x = sig[0] * noise
    for i in range(num_steps):
        s, s_next = sig[i], sig[i + 1]              # IndexError on a schedule of num_steps entries, as in the reference
        v = fn(x, sigma=sigmas[i])
        x_next = x + (s_next - s) * v
        if s_next != 0 and use_heun:
            v_next = fn(x_next, sigma=sigmas[i + 1])
            x_next = x + 0.5 * (s_next - s) * (v + v_next)
        x = x_next
    return x.clamp(-1.0, 1.0) if clamp else x
