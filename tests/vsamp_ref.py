"""CPU restatement (test infrastructure, not product code) of the reference's four table-driven sampler loops -- ``VESampler`` / ``VPSampler``
(src/models/components/sampler_edm.py:31-227) and ``VEulerSampler`` / ``VSampler`` (sampler_vobj.py:31-194) -- and of the raw v prediction
``VDiffusion(for_edm=False).denoise_fn`` they drive (diffusion.py:306-326), written independently of audiodiffuser_amd's plugin classes so that the
device and the plugins are held to something they do not share code with.  tools/gen_golden_vsamp.py pins these functions to the reference's
classes when it writes tests/golden/vsamp_golden.npz.

Every schedule scalar stays on fp32 0-dim tensors and is formed by the reference's own sequence of torch operations, whatever the dtype of the
state: with a float64 state torch promotes ``scalar * state`` to float64, so a float64 run is the reference's loop with the reference's fp32
scalars and a double-precision state (what a device result is compared with); an fp32 run is the reference's arithmetic itself.

``draws`` ([n, *state shape]) replaces the ``randn_like`` calls, in the reference's order; without it the loops draw like the reference.  ``record``
(a list) receives one dict of the step's fp32 scalars per step."""
from __future__ import annotations

import math
from math import sqrt
from typing import Callable, Optional

import torch
from torch.special import expm1


def _draw(draws: Optional[torch.Tensor], k: int, like: torch.Tensor) -> torch.Tensor:
    return torch.randn_like(like) if draws is None else draws[k].to(like.dtype)


def _gammas(sigmas, lo, hi, s_churn, num_steps):
    return torch.where((sigmas >= lo) & (sigmas <= hi), min(s_churn / num_steps, sqrt(2) - 1), 0.0)


# ---- VESampler ----------------------------------------------------------------------------------------------------------------------
def ve_sampler(noise: torch.Tensor, fn: Callable, sigmas: torch.Tensor, num_steps: int, s_tmin=0, s_tmax=float("inf"), s_churn=200, s_noise=1,
               use_heun: bool = True, draws: Optional[torch.Tensor] = None, record: Optional[list] = None, clamp: bool = True) -> torch.Tensor:
    """sampler_edm.py:55-123.  ``fn(x, sigma=<0-dim fp32 tensor>)`` returns the denoised estimate."""
    to_sigma = lambda t: t.sqrt()
    deriv = lambda t: 0.5 / t.sqrt()
    to_t = lambda s: s ** 2
    ts = to_t(sigmas)
    ts = torch.cat([ts, torch.zeros_like(ts[:1])])
    gammas = _gammas(sigmas, s_tmin, s_tmax, s_churn, num_steps)
    x = noise * sigmas[0]
    for i in range(num_steps):
        t, t_next, gamma = ts[i], ts[i + 1], gammas[i]
        t_hat = to_t(to_sigma(t) + gamma * to_sigma(t))
        nc = (to_sigma(t_hat) ** 2 - to_sigma(t) ** 2).clip(min=0).sqrt() * s_noise
        x_hat = x + nc * _draw(draws, i, x)
        d = (deriv(t_hat) / to_sigma(t_hat)) * x_hat - deriv(t_hat) / to_sigma(t_hat) * fn(x_hat, sigma=to_sigma(t_hat))
        h = t_next - t_hat
        x_next = x_hat + h * d
        rec = dict(gamma=float(gamma), t_hat=float(t_hat), a0=1.0, a1=float(nc), sigma1=float(to_sigma(t_hat)), h=float(h))
        if t_next != 0 and use_heun:
            t_prime = t_hat + h
            d_prime = deriv(t_prime) / to_sigma(t_prime) * x_next - deriv(t_prime) / to_sigma(t_prime) * fn(x_next, sigma=to_sigma(t_prime))
            x_next = x_hat + 1 / 2 * h * (d + d_prime)
            rec["sigma2"] = float(to_sigma(t_prime))
        if record is not None:
            record.append(rec)
        x = x_next
    return x.clamp(-1.0, 1.0) if clamp else x


# ---- VPSampler ----------------------------------------------------------------------------------------------------------------------
def vp_sampler(noise: torch.Tensor, fn: Callable, sigmas: torch.Tensor, num_steps: int, beta_d=19.9, beta_min=0.1, s_churn=200.0, s_noise=1.0,
               s_min=0.0, s_max=float("inf"), use_heun: bool = True, draws: Optional[torch.Tensor] = None, record: Optional[list] = None) -> torch.Tensor:
    """sampler_edm.py:152-227.  The result is NOT clamped, as in the reference."""
    to_sigma = lambda t: ((0.5 * beta_d * (t ** 2) + beta_min * t).exp() - 1) ** 0.5
    to_t = lambda s: ((beta_min ** 2 + 2 * beta_d * (s ** 2 + 1).log()).sqrt() - beta_min) / beta_d
    deriv = lambda t: 0.5 * (beta_min + beta_d * t) * (to_sigma(t) + 1 / to_sigma(t))
    scale = lambda t: 1 / (1 + to_sigma(t) ** 2).sqrt()
    scale_deriv = lambda t: -to_sigma(t) * deriv(t) * (scale(t) ** 3)
    ts = to_t(sigmas)
    ts = torch.cat([ts, torch.zeros_like(ts[:1])])
    gammas = _gammas(sigmas, s_min, s_max, s_churn, num_steps)
    x = noise * sigmas[0] * scale(ts[0])
    for i in range(num_steps):
        t, t_next, gamma = ts[i], ts[i + 1], gammas[i]
        t_hat = to_t(to_sigma(t) + gamma * to_sigma(t))
        a0 = scale(t_hat) / scale(t)
        nc = (to_sigma(t_hat) ** 2 - to_sigma(t) ** 2).clip(min=0).sqrt() * scale(t_hat) * s_noise
        x_hat = a0 * x + nc * _draw(draws, i, x)
        den = fn(x_hat / scale(t_hat), sigma=to_sigma(t_hat))
        d = (deriv(t_hat) / to_sigma(t_hat) + scale_deriv(t_hat) / scale(t_hat)) * x_hat - deriv(t_hat) * scale(t_hat) / to_sigma(t_hat) * den
        h = t_next - t_hat
        x_next = x_hat + h * d
        rec = dict(gamma=float(gamma), t_hat=float(t_hat), a0=float(a0), a1=float(nc), sigma1=float(to_sigma(t_hat)), h=float(h))
        if t_next != 0 and use_heun:
            t_prime = t_hat + h
            den_p = fn(x_next / scale(t_prime), sigma=to_sigma(t_prime))
            d_prime = ((deriv(t_prime) / to_sigma(t_prime) + scale_deriv(t_prime) / scale(t_prime)) * x_next
                       - deriv(t_prime) * scale(t_prime) / to_sigma(t_prime) * den_p)
            x_next = x_hat + 1 / 2 * h * (d + d_prime)
            rec["sigma2"] = float(to_sigma(t_prime))
        if record is not None:
            record.append(rec)
        x = x_next
    return x


# ---- the v objective ------------------------------------------------------------------------------------------------------------------
def shifted_cosine(t: torch.Tensor, logsnr_min=-15, logsnr_max=15, shift=0.0) -> torch.Tensor:
    t_min = math.atan(math.exp(-0.5 * logsnr_max))
    t_max = math.atan(math.exp(-0.5 * logsnr_min))
    return -2 * (torch.tan(t_min + t * (t_max - t_min)).log()) + 2 * shift


def v_raw(net: Callable[..., torch.Tensor], x: torch.Tensor, sigma, cond_scale: float = 1.0) -> torch.Tensor:
    """``VDiffusion(for_edm=False).denoise_fn(x, sigma=logsnr, inference=True)``: the v network at that log-SNR, guided where cond_scale != 1."""
    t = torch.full((x.shape[0],), float(sigma), dtype=torch.float32).to(x.dtype)
    if cond_scale == 1.0:
        return net(x, t)
    v, null = net(x, t, cond_drop_prob=0.0), net(x, t, cond_drop_prob=1.0)
    return null + (v - null) * cond_scale


def make_v_fn(net: Callable[..., torch.Tensor], cond_scale: float = 1.0) -> Callable:
    return lambda x, sigma: v_raw(net, x, sigma, cond_scale)


def _v_scalars(t, t_next, logsnr_min, logsnr_max, shift):
    lt, ls = shifted_cosine(t, logsnr_min, logsnr_max, shift), shifted_cosine(t_next, logsnr_min, logsnr_max, shift)
    return lt, ls, torch.sqrt(torch.sigmoid(lt)), torch.sqrt(torch.sigmoid(-lt)), torch.sqrt(torch.sigmoid(ls)), torch.sqrt(torch.sigmoid(-ls))


def v_sampler(noise: torch.Tensor, fn: Callable, ts: torch.Tensor, num_steps: int, logsnr_min=-15, logsnr_max=15, shift=0.0,
              draws: Optional[torch.Tensor] = None, record: Optional[list] = None, clamp: bool = True) -> torch.Tensor:
    """sampler_vobj.py:131-194.  ``fn(x, sigma=<0-dim fp32 log-SNR>)`` returns the raw v prediction; one draw per step with t_next != 0."""
    ts = torch.cat([ts, torch.zeros_like(ts[:1])])
    x, k = noise, 0
    for i in range(num_steps):
        t, t_next = ts[i], ts[i + 1]
        lt, ls, alpha_t, sigma_t, alpha_s, sigma_s = _v_scalars(t, t_next, logsnr_min, logsnr_max, shift)
        v_pred = fn(x, sigma=lt)
        x_pred = alpha_t * x - sigma_t * v_pred
        x_pred = x_pred.clamp(-1.0, 1.0)
        c = -expm1(lt - ls)
        mu = alpha_s * (x * (1 - c) / alpha_t + c * x_pred)
        variance = (sigma_s ** 2) * c
        if record is not None:
            record.append(dict(logsnr_t=float(lt), logsnr_s=float(ls), alpha_t=float(alpha_t), sigma_t=float(sigma_t), alpha_s=float(alpha_s),
                               sigma_s=float(sigma_s), c=float(c), std=float(torch.sqrt(variance)), share_clamped=float((x_pred.abs() >= 1).double().mean())))
        if t_next != 0:
            x = mu + _draw(draws, k, mu) * torch.sqrt(variance)
            k += 1
        else:
            x = mu
    return x.clamp(-1.0, 1.0) if clamp else x


def veuler_sampler(noise: torch.Tensor, fn: Callable, ts: torch.Tensor, num_steps: int, logsnr_min=-15, logsnr_max=15, shift=0.5,
                   use_heun: bool = False, record: Optional[list] = None, clamp: bool = True) -> torch.Tensor:
    """sampler_vobj.py:53-109: no draws."""
    ts = torch.cat([ts, torch.zeros_like(ts[:1])])
    x = noise
    for i in range(num_steps):
        t, t_next = ts[i], ts[i + 1]
        lt, ls, alpha_t, sigma_t, alpha_s, sigma_s = _v_scalars(t, t_next, logsnr_min, logsnr_max, shift)
        v_pred = fn(x, sigma=lt)
        if record is not None:
            record.append(dict(logsnr_t=float(lt), logsnr_s=float(ls), alpha_t=float(alpha_t), sigma_t=float(sigma_t), alpha_s=float(alpha_s),
                               sigma_s=float(sigma_s)))
        if t_next == 0.0:
            x_next = alpha_t * x - sigma_t * v_pred
        else:
            score_cur = - alpha_t * sigma_t * v_pred
            x_next = x + 0.5 * (ls - lt) * score_cur
            if use_heun:
                v_pred_next = fn(x_next, sigma=ls)
                score_next = - alpha_s * sigma_s * v_pred_next
                x_next = x + 0.25 * (ls - lt) * (score_next + score_cur)
        x = x_next
    return x.clamp(-1.0, 1.0) if clamp else x
