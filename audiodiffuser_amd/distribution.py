"""``model.noise_distribution`` plugins (reference: src/models/components/distribution.py:9-68): where ``DiffUnetComplexModule.forward`` draws the
sigmas (or times) of a training / validation batch before it calls ``model.diffusion`` (diffunet_complex_module.py:116-121).

The reference's constructor keywords, ``__call__(num_samples, device)`` and its expressions in its order, so that the same seed gives the same
draws bit for bit (tests/golden/loss_golden.npz).  These are a handful of [B]-sized tensor ops per batch: stock torch, not a device kernel.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor


class Distribution:
    def __call__(self, num_samples: int, device: torch.device):
        raise NotImplementedError()


class LogNormalDistribution(Distribution):
    """exp(mean + std * randn): EDM's training distribution of sigma (distribution.py:9-16)."""

    def __init__(self, mean: float, std: float):
        self.mean = mean
        self.std = std

    def __call__(self, num_samples: int, device: torch.device = torch.device("cpu")) -> Tensor:
        normal = self.mean + self.std * torch.randn((num_samples,), device=device)
        return normal.exp()


class UniformDistribution(Distribution):
    """(vmin - vmax) * rand + vmax, as the reference writes it (distribution.py:18-25)."""

    def __init__(self, vmin: float = 0.0, vmax: float = 1.0):
        super().__init__()
        self.vmin, self.vmax = vmin, vmax

    def __call__(self, num_samples: int, device: torch.device = torch.device("cpu")) -> Tensor:
        vmax, vmin = self.vmax, self.vmin
        return (vmin - vmax) * torch.rand(num_samples, device=device) + vmax


class LogUniformDistribution(Distribution):
    """sigma_min * (sigma_max / sigma_min) ** rand: loss against noise level (distribution.py:27-40)."""

    def __init__(self, sigma_min: float = 0.001, sigma_max: float = 100):
        super().__init__()
        self.sigma_min = sigma_min
        self.sigma_max = sigma_max

    def __call__(self, num_samples: int, device: torch.device = torch.device("cpu")) -> Tensor:
        rnd_uniform = torch.rand(num_samples, device=device)
        return self.sigma_min * ((self.sigma_max / self.sigma_min) ** rnd_uniform)


class LogitDistribution(Distribution):
    """Times in (0, 1) for rectified flow (distribution.py:42-68): uniform, or with ``ln_scale`` the logit-normal sigmoid(logit_mean + logit_std z),
    where ``stratified`` draws z through one uniform per quantile bin of the batch."""

    def __init__(self, logit_mean: float = 0.0, logit_std: float = 1.0, ln_scale=False, stratified=False):
        super().__init__()
        self.logit_std, self.logit_mean = logit_std, logit_mean
        self.ln_scale = ln_scale
        self.stratified = stratified

    def __call__(self, num_samples: int, device: torch.device = torch.device("cpu")) -> Tensor:
        if not self.ln_scale:
            return torch.rand(num_samples, device=device)
        if self.stratified:
            quantiles = torch.linspace(0, 1, num_samples + 1).to(device)
            z = quantiles[:-1] + torch.rand(num_samples, device=device) / num_samples
            z = torch.erfinv(2 * z - 1) * math.sqrt(2)
            z = z * self.logit_std + self.logit_mean
            return torch.sigmoid(z)
        nt = torch.randn(num_samples, device=device) * self.logit_std + self.logit_mean
        return torch.sigmoid(nt)
