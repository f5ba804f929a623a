"""CPU restatement (test infrastructure, not product code) of the reference's losses -- ``Diffusion.forward`` for EluDiffusion / VEDiffusion,
``VPDiffusion.forward`` and ``ReFlow(for_edm=False).forward`` (src/models/components/diffusion.py:65-97, :185-218, :420-442) -- with the noise given
instead of drawn, written on tests/precond_ref.py and tests/rf_ref.py and independently of audiodiffuser_amd's plugin classes.
tools/gen_golden_loss.py pins these functions to the reference's classes when it writes tests/golden/loss_golden.npz.

Everything runs in the dtype of ``x``: torch.float32 is the reference's arithmetic, torch.float64 the same formulas at double precision on the same
fp32 inputs (what a device result is compared with).  ``emulate_loss`` is the arithmetic of the device's two loss kernels in NumPy."""
from __future__ import annotations

from typing import Callable

import numpy as np
import torch

import precond_ref as P
import rf_ref as RF

KINDS = ("edm", "ve", "vp", "rf")          # vp: the coefficients handed in are TIMES (VPDiffusion.forward maps them to sigma)
LOSS_KIND = {"edm": 0, "ve": 1, "vp": 1, "rf": 2}      # ADF_LOSS_* of include/audiodiffuser_amd.h

# the inputs of the GPU tests (tests/test_loss_gpu.py) and of the bar derivation (tests/test_loss_host.py)
SIGMAS = (0.05, 0.6, 7.0)
TIMES = (0.1, 0.5, 0.93)
SIGMA_DATA = P.SIGMA_DATA


def inputs(shape, seed: int = 5):
    """(x, noise): x = 0.3 randn clamped to +-1, then the noise from the same generator."""
    g = torch.Generator().manual_seed(seed)
    x = (0.3 * torch.randn(*shape, generator=g)).clamp(-1.0, 1.0)
    return x, torch.randn(*shape, generator=g)


def coefs(kind: str, b: int) -> torch.Tensor:
    """What the diffusion class of ``kind`` is called with: sigmas for edm / ve, times for vp / rf."""
    return torch.tensor((TIMES if kind in ("vp", "rf") else SIGMAS)[:b])


def _ext(v: torch.Tensor, ndim: int) -> torch.Tensor:
    return v.view(v.shape[0], *((1,) * (ndim - 1)))


def vp_t_to_sigma(t: torch.Tensor) -> torch.Tensor:
    return ((0.5 * P.VP_ARGS["beta_d"] * (t ** 2) + P.VP_ARGS["beta_min"] * t).exp() - 1).sqrt()


def sigmas_of(kind: str, coef: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """The sigmas (rf: times) behind ``coef`` in ``dtype``: the fp32 values widened, and for vp the time mapped in ``dtype``."""
    c = coef.to(torch.float32).to(dtype)
    return vp_t_to_sigma(c) if kind == "vp" else c


def mix(kind: str, x: torch.Tensor, noise: torch.Tensor, sig: torch.Tensor) -> torch.Tensor:
    s = _ext(sig.to(x.dtype), x.ndim)
    return (1 - s) * x + s * noise if kind == "rf" else x + s * noise


def weight(kind: str, sig: torch.Tensor) -> torch.Tensor:
    if kind == "edm":
        return (sig ** 2 + SIGMA_DATA ** 2) * (sig * SIGMA_DATA) ** -2
    return torch.ones_like(sig) if kind == "rf" else 1 / sig ** 2


def loss_of_pred(kind: str, x: torch.Tensor, noise: torch.Tensor, pred: torch.Tensor, sig: torch.Tensor) -> torch.Tensor:
    """[B] losses from a given denoiser output, in the dtype of ``x``."""
    dt = x.dtype
    d = (noise.to(dt) - x - pred.to(dt)) if kind == "rf" else (pred.to(dt) - x)
    return (d ** 2).reshape(x.shape[0], -1).sum(dim=1) * weight(kind, sig.to(dt)) / float(x[0].numel())


def forward(kind: str, net: Callable[..., torch.Tensor], x: torch.Tensor, noise: torch.Tensor, coef: torch.Tensor, cond_scale: float = 1.0,
            dynamic_threshold: float = 0.0) -> torch.Tensor:
    """``diffusion(x, net, sigmas=coef, inference=True, cond_scale=...)`` of the reference class of ``kind`` with ``noise`` in the place of its draw,
    in the dtype of ``x``.  Without guidance this is also the ``inference=False`` call on a net whose ``cond_drop_prob`` is 0."""
    dt = x.dtype
    noise = noise.to(dt)
    sig = sigmas_of(kind, coef, dt)
    x_noisy = mix(kind, x, noise, sig)
    if kind == "rf":
        pred = RF.denoise(False, net, x_noisy, sigmas=coef, cond_scale=cond_scale)
    else:
        pred = P.denoise(kind, net, x_noisy, sigmas=sig, cond_scale=cond_scale, dynamic_threshold=dynamic_threshold)
    return loss_of_pred(kind, x, noise, pred, sig)


def toy_net(x: torch.Tensor, t: torch.Tensor, **kwargs) -> torch.Tensor:
    """The small deterministic callable the fixture's reference losses were recorded around (any dtype, any [B, ...] shape)."""
    return 0.7 * torch.tanh(1.5 * x + 0.1 * _ext(t.to(x.dtype), x.ndim)) + 0.1 * x.roll(1, -1)


def emulate_loss(kind: str, x: torch.Tensor, noise: torch.Tensor, pred: torch.Tensor, sig32: torch.Tensor) -> np.ndarray:
    """The device's loss kernels in NumPy: the difference(s) and the square each rounded to fp32, the sum in float64, w / N in float64 from the fp32
    sigma, one rounding of the product to fp32.  (The device sums in another order; in float64 that moves the sum by ~1e-16 relative.)"""
    xs, zs, ps = (t.to(torch.float32).numpy().reshape(x.shape[0], -1) for t in (x, noise, pred))
    d = ((zs - xs).astype(np.float32) - ps).astype(np.float32) if kind == "rf" else (ps - xs).astype(np.float32)
    sq = (d * d).astype(np.float32)
    s = sig32.to(torch.float32).numpy().astype(np.float64)
    sd = np.float64(np.float32(SIGMA_DATA))
    w = {"edm": (s * s + sd * sd) / ((s * sd) * (s * sd)), "rf": np.ones_like(s)}.get(kind, 1.0 / (s * s))
    return (w / float(xs.shape[1]) * sq.astype(np.float64).sum(axis=1)).astype(np.float32)
