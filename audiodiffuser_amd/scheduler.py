"""``model.noise_scheduler`` plugins (reference: src/models/components/scheduler.py:6-120): the same torch ops in the same order,
so every schedule equals the reference's bit for bit.

The Lightning module stores ``noise_scheduler()`` once (diffunet_complex_module.py:64), i.e. the
instance call returns the fp32 sigma tensor on the CPU; it is moved to the device at the call site.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
from torch import Tensor


class KarrasSchedule(nn.Module):
    """EDM eq. 5: sigma_i = (smax^(1/rho) + i/(N-1) (smin^(1/rho) - smax^(1/rho)))^rho."""

    def __init__(self, sigma_min: float, sigma_max: float, rho: float = 7.0, num_steps: int = 50):
        super().__init__()
        self.sigma_min, self.sigma_max, self.rho, self.num_steps = sigma_min, sigma_max, rho, num_steps

    def forward(self) -> Tensor:
        inv = 1.0 / self.rho
        ramp = torch.arange(self.num_steps, dtype=torch.float32) / (self.num_steps - 1)
        lo, hi = self.sigma_min ** inv, self.sigma_max ** inv
        return (hi + ramp * (lo - hi)) ** self.rho


class LinearSchedule(nn.Module):
    """scheduler.py:24-36: ``linspace(start, end, num_steps)`` (the time grid of the reference's ``sampler_vobj`` samplers)."""

    def __init__(self, start: float = 1.0, end: float = 0.0, num_steps: int = 50):
        super().__init__()
        self.start, self.num_steps, self.end = start, num_steps, end

    def forward(self) -> Tensor:
        return torch.linspace(self.start, self.end, self.num_steps)


class GeometricSchedule(nn.Module):
    """scheduler.py:39-51: the variances ``sigma_max^2 (sigma_min^2 / sigma_max^2)^(i / (N - 1))`` (``VESchedule`` without the square root)."""

    def __init__(self, sigma_max: float = 100, sigma_min: float = 0.02, num_steps: int = 50):
        super().__init__()
        self.sigma_max, self.sigma_min, self.num_steps = sigma_max, sigma_min, num_steps

    def forward(self) -> Tensor:
        steps = torch.arange(self.num_steps, dtype=torch.float32)
        return (self.sigma_max ** 2) * ((self.sigma_min ** 2 / self.sigma_max ** 2) ** (steps / (self.num_steps - 1)))


class VPSchedule(nn.Module):
    """scheduler.py:53-71: sigma(t) = sqrt(exp(beta_d t^2 / 2 + beta_min t) - 1) on ``t = linspace(start, end, num_steps)``."""

    def __init__(self, start: float = 1.0, end: float = 1e-3, beta_d: float = 19.9, beta_min: float = 0.1, num_steps: int = 50):
        super().__init__()
        self.start, self.num_steps, self.end, self.beta_d, self.beta_min = start, num_steps, end, beta_d, beta_min

    def forward(self) -> Tensor:
        sigmas = torch.linspace(self.start, self.end, self.num_steps)
        return ((0.5 * self.beta_d * (sigmas ** 2) + self.beta_min * sigmas).exp() - 1) ** 0.5


class VESchedule(nn.Module):
    """scheduler.py:73-85: geometric in the variance, ``sigma_max`` down to ``sigma_min``."""

    def __init__(self, sigma_max: float = 100, sigma_min: float = 0.02, num_steps: int = 50):
        super().__init__()
        self.sigma_max, self.sigma_min, self.num_steps = sigma_max, sigma_min, num_steps

    def forward(self) -> Tensor:
        steps = torch.arange(self.num_steps, dtype=torch.float32)
        sigmas = (self.sigma_max ** 2) * ((self.sigma_min ** 2 / self.sigma_max ** 2) ** (steps / (self.num_steps - 1)))
        return sigmas.sqrt()


class VSchedule(nn.Module):
    """scheduler.py:87-103: the shifted-cosine log-SNR grid of v-diffusion as sigma = sigma_t / alpha_t (1808 down to 5.5e-4 at the defaults)."""

    def __init__(self, logsnr_min=-15, logsnr_max=15, shift=0.0, num_steps: int = 50):
        super().__init__()
        self.shift, self.num_steps = shift, num_steps
        self.t_min = math.atan(math.exp(-0.5 * logsnr_max))
        self.t_max = math.atan(math.exp(-0.5 * logsnr_min))

    def forward(self) -> Tensor:
        t = torch.linspace(1.0, 0.0, self.num_steps)
        logsnr_t = -2 * (torch.tan(self.t_min + t * (self.t_max - self.t_min)).log()) + 2 * self.shift
        alpha_t = torch.sqrt(torch.sigmoid(logsnr_t))
        sigma_t = torch.sqrt(torch.sigmoid(-logsnr_t))
        return sigma_t / alpha_t


class RFEDMSchedule(nn.Module):
    """scheduler.py:105-120: the rectified-flow time grid ``t = linspace(start, end, num_steps)`` as the EDM sigma ``t / (1 - t)`` that
    ``ReFlow(for_edm=True)`` maps back (``t = sigma / (sigma + 1)``).  As in the reference the defaults give ``inf`` first (start = 1) and a last
    sigma of 0, which the EDM-family samplers divide by: use ``start < 1`` and ``end > 0``."""

    def __init__(self, start: float = 1.0, end: float = 0.0, num_steps: int = 50):
        super().__init__()
        assert start <= 1.0 and end >= 0.0, "start must be less than or equal to 1.0 and end must be greater than or equal to 0.0"
        self.start, self.num_steps, self.end = start, num_steps, end

    def forward(self) -> Tensor:
        sigmas = torch.linspace(self.start, self.end, self.num_steps)
        return sigmas / (1 - sigmas)
