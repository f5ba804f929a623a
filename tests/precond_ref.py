"""CPU restatement (test infrastructure, not product code) of the reference's VE / VP / v preconditioning and sigma schedules
(src/models/components/diffusion.py:99-170, :260-326; scheduler.py:24-103), written independently of audiodiffuser_amd's plugin classes so that
the device and the plugins are held to something they do not share code with.  tools/gen_golden_precond.py pins these functions to the
reference's classes (exactly, in fp32) when it writes tests/golden/precond_golden.npz.

``dtype`` is torch.float32 (the reference's arithmetic) or torch.float64 (the same formulas at double precision: what the conditioning of
an expression is measured against)."""
from __future__ import annotations

import math
from typing import Callable, Optional

import torch

from oracle.edm import clip, edm_scale_weights

KINDS = ("edm", "ve", "vp", "v")
VP_ARGS = dict(beta_min=0.1, beta_d=19.9, M=1000)          # diffunet_complex_sc09_eval_vp.yaml
SIGMA_DATA = 0.2                                           # diffunet_complex_sc09_eval_dpm.yaml


# ---- schedules at the reference's signatures ---------------------------------------------------------------------------------------
def linear_schedule(start=1.0, end=0.0, num_steps=50):
    return torch.linspace(start, end, num_steps)


def geometric_schedule(sigma_max=100, sigma_min=0.02, num_steps=50):
    steps = torch.arange(num_steps, dtype=torch.float32)
    return (sigma_max ** 2) * ((sigma_min ** 2 / sigma_max ** 2) ** (steps / (num_steps - 1)))


def vp_schedule(start=1.0, end=1e-3, beta_d=19.9, beta_min=0.1, num_steps=50):
    t = torch.linspace(start, end, num_steps)
    return ((0.5 * beta_d * (t ** 2) + beta_min * t).exp() - 1) ** 0.5


def ve_schedule(sigma_max=100, sigma_min=0.02, num_steps=50):
    return geometric_schedule(sigma_max, sigma_min, num_steps).sqrt()


def v_schedule(logsnr_min=-15, logsnr_max=15, shift=0.0, num_steps=50):
    t_min, t_max = math.atan(math.exp(-0.5 * logsnr_max)), math.atan(math.exp(-0.5 * logsnr_min))
    t = torch.linspace(1.0, 0.0, num_steps)
    logsnr = -2 * (torch.tan(t_min + t * (t_max - t_min)).log()) + 2 * shift
    return torch.sqrt(torch.sigmoid(-logsnr)) / torch.sqrt(torch.sigmoid(logsnr))


def shipped_schedule(kind: str, num_steps: int) -> torch.Tensor:
    """The ``noise_scheduler`` of the shipped sc09 inference file of each kind."""
    if kind == "ve":
        return ve_schedule(100, 0.02, num_steps)
    if kind == "vp":
        return vp_schedule(beta_d=19.9, beta_min=0.1, end=0.001, num_steps=num_steps)
    if kind == "v":
        return v_schedule(num_steps=num_steps)
    inv = 1.0 / 7.0                                          # KarrasSchedule(0.002, 80, 7)
    i = torch.arange(num_steps, dtype=torch.float32)
    return (80.0 ** inv + i / (num_steps - 1) * (0.002 ** inv - 80.0 ** inv)) ** 7.0


# ---- rows -------------------------------------------------------------------------------------------------------------------------
def rows(kind: str, sigmas: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """[n, 4] = (c_in, c_noise, c_skip, c_out) per sigma, the device's row layout.  ``sigmas`` are fp32 values; with float64 they are widened
    first and every operation runs in double."""
    s = sigmas.to(dtype)
    one = torch.ones_like(s)
    if kind == "edm":
        c_skip, c_out, c_in, c_noise = edm_scale_weights(s, SIGMA_DATA, 1)
    elif kind == "ve":
        c_in, c_noise, c_skip, c_out = one, (0.5 * s).log(), one, s
    elif kind == "vp":
        bm, bd, M = VP_ARGS["beta_min"], VP_ARGS["beta_d"], VP_ARGS["M"]
        t = ((bm ** 2 + 2 * bd * (1 + s ** 2).log()).sqrt() - bm) / bd
        c_in, c_noise, c_skip, c_out = 1 / (s ** 2 + 1).sqrt(), (M - 1) * t, one, -s
    elif kind == "v":
        logsnr = -2 * s.log()
        sigmat, alphat = torch.sqrt(torch.sigmoid(-logsnr)), torch.sqrt(torch.sigmoid(logsnr))
        c_in, c_noise, c_skip, c_out = alphat, logsnr, alphat * alphat, -sigmat
    else:
        raise ValueError(kind)
    return torch.stack([c_in, c_noise, c_skip, c_out], dim=1)


# ---- denoiser ---------------------------------------------------------------------------------------------------------------------
def denoise(kind: str, net: Callable[..., torch.Tensor], x_noisy: torch.Tensor, sigma=None, sigmas: Optional[torch.Tensor] = None,
            cond_scale: float = 1.0, dynamic_threshold: float = 0.0, unclipped: bool = False) -> torch.Tensor:
    """``denoise_fn(..., inference=True)`` of the reference class of ``kind`` around ``net(x, time[, cond_drop_prob])``, in the dtype of
    ``x_noisy``.  The v kind follows VDiffusion.denoise_fn(for_edm=True) as written (alpha_t (alpha_t x) - sigma_t v, no clipping), with the
    per-sample factors shaped [B, 1, ...].  ``unclipped``: the estimate before ``clip`` (what a clamped result's error has to be scaled by when
    most of it saturates)."""
    assert (sigma is None) ^ (sigmas is None)
    b, dt = x_noisy.shape[0], x_noisy.dtype
    if sigmas is None:
        sigmas = torch.full((b,), float(sigma), dtype=torch.float32)
    r = rows(kind, sigmas.to(torch.float32), dt)
    ext = lambda v: v.view(b, *((1,) * (x_noisy.ndim - 1)))
    c_in, c_noise, c_skip, c_out = ext(r[:, 0]), r[:, 1], ext(r[:, 2]), ext(r[:, 3])
    x_in = c_in * x_noisy
    if cond_scale == 1.0:
        pred = net(x_in, c_noise)
    else:
        pred = net(x_in, c_noise, cond_drop_prob=0.0)
        null = net(x_in, c_noise, cond_drop_prob=1.0)
        pred = null + (pred - null) * cond_scale
    if kind == "v":
        return c_in * x_in + c_out * pred
    den = c_skip * x_noisy + c_out * pred
    return den if unclipped else clip(den, dynamic_threshold)


def make_fn(kind: str, net: Callable[..., torch.Tensor], cond_scale: float = 1.0) -> Callable:
    """The closure oracle/samplers.py calls: fn(x, sigma=<0-dim tensor>) or fn(x, sigmas=[B])."""
    return lambda x, sigma=None, sigmas=None: denoise(kind, net, x, sigma=sigma, sigmas=sigmas, cond_scale=cond_scale)
