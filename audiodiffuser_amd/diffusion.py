"""``model.diffusion`` plugins: preconditioning + denoise wrapper
(reference: src/models/components/diffusion.py:15-63 ``Diffusion``, :99-133 ``VEDiffusion``, :136-218 ``VPDiffusion``,
:220-258 ``EluDiffusion``, :260-365 ``VDiffusion``, :367-442 ``ReFlow``).

``denoise_fn`` keeps the reference signature.  When ``net`` is one of this package's HIP nets and the call
is the inference case the whole thing -- c_in scaling, sigma embedding, network,
(for a class-conditional net: label embedding and classifier-free guidance), c_skip/c_out combine,
clipping -- is one ``adf_denoise`` call; which class's formulas the device uses travels as handle state
(``adf_set_preconditioning``).
For any other ``net`` (e.g. an unpickled reference module, diffunet_complex_module.py:239-242) the
same arithmetic is expressed with tensor ops around ``net(...)``; that branch exists for interface
compatibility and is not the accelerated path.

``forward`` is the loss (``DiffUnetComplexModule.forward`` / ``validation_step``, diffunet_complex_module.py:104-125, :186-195).  Under
``torch.no_grad()`` on a HIP net it is one ``adf_diffusion_loss`` call -- noising, the same ``adf_denoise`` evaluation, weighted per-sample squared
error -- for the classes whose loss has an x0 or velocity form (``_loss_kind``); ``loss_route_refusal`` says for which calls, and every other
call runs ``_tensor_loss``, the tensor ops this module has always used.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from .net import HipNet, UNet1dBase  # noqa: F401


def _extend(x: Tensor, ndim: int) -> Tensor:
    return x.view(*x.shape, *((1,) * (ndim - x.ndim)))


def _require_native() -> bool:
    return os.environ.get("ADF_REQUIRE_NATIVE", "0") not in ("", "0")


def conditioning_refusal(net: HipNet, cond_scale: float, kwargs: dict) -> Optional[str]:
    """The only conditioning keyword the device understands is ``classes`` (labels) on a class-conditional net, where ``cond_scale != 1`` is
    classifier-free guidance.  Returns None for such a call, otherwise why it leaves the device (``denoise_fn`` and every sampler ask here)."""
    extra = {k for k, v in kwargs.items() if v is not None}
    if net.cfg.class_cond:
        return None if extra == {"classes"} else "a class-conditional net takes exactly the `classes` keyword"
    return "conditioning keywords / cond_scale != 1 on an unconditional net" if extra or cond_scale != 1.0 else None


def loss_route_refusal(diff: "Diffusion", net, x_is_cuda: bool, inference: bool, cond_scale: float, kwargs: dict) -> Optional[str]:
    """None when ``diff.forward(x, net, sigmas, inference, cond_scale, **kwargs)`` is one ``adf_diffusion_loss`` call, otherwise why it stays on
    the tensor route (``_tensor_loss``).  Host logic only: no device is touched."""
    if diff._loss_kind() is None:
        return f"{type(diff).__name__}'s loss has no device form (neither x0 nor velocity)"
    if diff._precond() is None:
        return "the device has no row form for this preconditioning"
    if not isinstance(net, HipNet):
        return "`net` is not one of this package's HIP nets"
    if not x_is_cuda:
        return "`x` is not on a ROCm device"
    if not 0.0 <= diff.dynamic_threshold <= 1.0:
        return "dynamic_threshold outside [0, 1]"
    if "x_mask" in kwargs:
        return "`x_mask` weights the loss per element"
    if inference:
        return conditioning_refusal(net, cond_scale, kwargs)
    # not inferring, the reference calls net(x, c_noise, **kwargs): `cond_scale` is ignored and the label mask follows the net's cond_drop_prob
    extra = {k for k, v in kwargs.items() if v is not None}
    if not net.cfg.class_cond:
        return "conditioning keywords on an unconditional net" if extra else None
    if extra != {"classes"}:
        return "a class-conditional net takes exactly the `classes` keyword"
    if net.cond_drop_prob not in (0, 0.0, 1, 1.0):
        return "cond_drop_prob other than 0 or 1 draws a random label mask"
    return None


class Diffusion(nn.Module):
    """What the preconditioned diffusion classes share (diffusion.py:15-97): ``denoise_fn`` with the native fast path and the
    tensor-op compatibility branch, and the training ``forward``.  Subclasses give ``get_scale_weights`` / ``loss_weight`` and the
    device's name for their formulas (``_precond``)."""

    sigma_data = 1.0            # read by the samplers' descriptors; only EluDiffusion's formulas use it
    _clips = True               # False: the estimate is returned as it is (VDiffusion, diffusion.py:326)
    _mask_floor = 0.01          # weight of masked-out positions in the training loss (diffusion.py:81; VPDiffusion :209 uses 0.1)

    def __init__(self, dynamic_threshold: float = 0.0):
        super().__init__()
        self.dynamic_threshold = dynamic_threshold

    def _precond(self) -> Optional[tuple]:
        """(ADF_PRECOND_* kind, beta_min, beta_d, M) of ``adf_set_preconditioning``, or None when the device has no row form for it."""
        raise NotImplementedError

    def _loss_kind(self) -> Optional[int]:
        """The ADF_LOSS_* kind of ``adf_diffusion_loss`` this class's ``forward`` is, or None when the device has no form for it."""
        return None

    def _not_native_note(self) -> str:
        return ""

    def _native_ok(self, net, inference: bool, cond_scale: float, kwargs: dict) -> bool:
        """The HIP fast path covers inference (clamp clipping or the dynamic threshold) with the conditioning of ``conditioning_refusal``."""
        return (isinstance(net, HipNet) and inference and 0.0 <= self.dynamic_threshold <= 1.0 and self._precond() is not None
                and conditioning_refusal(net, cond_scale, kwargs) is None)

    def _configure(self, hd) -> None:
        """Preconditioning and clipping of every evaluation the handle runs from here on."""
        hd.set_preconditioning(*self._precond())
        hd.set_dynamic_threshold(self.dynamic_threshold if self._clips else 0.0)

    # diffusion.py:32-63
    def denoise_fn(self, x_noisy: Tensor, net: nn.Module = None, inference: bool = False, cond_scale: float = 1.0,
                   sigmas: Optional[Tensor] = None, sigma: Optional[float] = None, **kwargs) -> Tensor:
        assert (sigma is not None) ^ (sigmas is not None), "Either x or xs must be provided"   # components/utils.py:47
        if self._native_ok(net, inference, cond_scale, kwargs) and x_noisy.is_cuda:
            hd = net.native(x_noisy.device)
            self._configure(hd)
            x = x_noisy.detach().to(torch.float32).contiguous()
            if net.cfg.class_cond:      # labels + guidance scale for this call (diffusion.py:49-54)
                hd.set_condition(kwargs["classes"], x.device, null_labels=False, cond_scale=float(cond_scale))
            with torch.cuda.device(x.device):
                if sigmas is not None:
                    sv = sigmas.detach().to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
                    return hd.denoise(x, self.sigma_data, sigmas=sv).to(x_noisy.dtype)
                return hd.denoise(x, self.sigma_data, sigma=float(sigma)).to(x_noisy.dtype)
        # ---- interface-compatibility branch: arbitrary `net` callable -------------------------
        if isinstance(net, HipNet) and inference and _require_native():
            raise RuntimeError("denoise_fn: ADF_REQUIRE_NATIVE is set and this inference call on a HIP net would not be one adf_denoise call"
                               + self._not_native_note())
        b, device = x_noisy.shape[0], x_noisy.device
        if sigmas is None:
            sigmas = torch.full((b,), float(sigma), dtype=torch.float32, device=device)
        return self._compat_denoise(x_noisy, net, inference, cond_scale, sigmas, kwargs)

    def _compat_denoise(self, x_noisy: Tensor, net, inference: bool, cond_scale: float, sigmas: Tensor, kwargs: dict) -> Tensor:
        b = x_noisy.shape[0]
        c_skip, c_out, c_in, c_noise = self.get_scale_weights(sigmas, x_noisy.ndim)
        if inference:
            pred = net(c_in * x_noisy, c_noise, cond_drop_prob=0.0, **kwargs)
            if cond_scale != 1.0:
                null = net(c_in * x_noisy, c_noise, cond_drop_prob=1.0, **kwargs)
                pred = null + (pred - null) * cond_scale
        else:
            pred = net(c_in * x_noisy, c_noise, **kwargs)
        den = c_skip * x_noisy + c_out * pred
        if self.dynamic_threshold == 0.0:
            return den.clamp(-1.0, 1.0)
        flat = den.reshape(b, -1)                                           # components/utils.py:23-33
        scale = torch.quantile(flat.abs(), self.dynamic_threshold, dim=-1).clamp_(min=1.0)
        scale = _extend(scale, den.ndim)
        return den.clamp(-scale, scale) / scale

    def _training_guard(self, net) -> None:
        if isinstance(net, HipNet) and torch.is_grad_enabled() and any(p.requires_grad for p in net.parameters()):
            raise NotImplementedError(f"{type(self).__name__}.forward is the training loss; the HIP nets are an inference path without "
                                      "backward -- train the reference module and load its state_dict here, or call under torch.no_grad()")

    # diffusion.py:65-98
    def forward(self, x: Tensor, net: nn.Module, sigmas: Tensor, inference: bool = False, cond_scale: float = 1.0,
                **kwargs) -> Tensor:
        if loss_route_refusal(self, net, x.is_cuda, inference, cond_scale, kwargs) is None:
            self._training_guard(net)
            return self._device_loss(x, net, sigmas, inference, cond_scale, kwargs)
        return self._tensor_loss(x, net, sigmas, inference=inference, cond_scale=cond_scale, **kwargs)

    def _device_loss(self, x: Tensor, net: HipNet, sigmas: Tensor, inference: bool, cond_scale: float, kwargs: dict) -> Tensor:
        """One ``adf_diffusion_loss`` call.  The noise is drawn first, once, on ``x``'s device, as ``_tensor_loss`` draws it: with the same seed both
        routes see the same noise and leave the global generator in the same state."""
        noise = torch.randn_like(x)
        hd = net.native(x.device)
        self._configure(hd)
        if net.cfg.class_cond:
            if inference:           # labels + two-pass guidance (diffusion.py:49-54)
                hd.set_condition(kwargs["classes"], x.device, null_labels=False, cond_scale=float(cond_scale))
            else:                   # net(x, c_noise, classes=...): the net's own cond_drop_prob, no guidance (:56)
                hd.set_condition(kwargs["classes"], x.device, null_labels=bool(net.cond_drop_prob), cond_scale=1.0)
        xf = x.detach().to(torch.float32).contiguous()
        nf = noise.to(torch.float32).contiguous()
        sv = sigmas.detach().to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
        with torch.cuda.device(x.device):
            return hd.diffusion_loss(self._loss_kind(), xf, nf, sv, self.sigma_data).to(x.dtype)

    # diffusion.py:65-98 as stock tensor ops: the route of every call `loss_route_refusal` names a reason for
    def _tensor_loss(self, x: Tensor, net: nn.Module, sigmas: Tensor, inference: bool = False, cond_scale: float = 1.0,
                     **kwargs) -> Tensor:
        self._training_guard(net)
        noise = torch.randn_like(x)
        x_noisy = x + _extend(sigmas, x.ndim) * noise
        mask = torch.ones_like(x)
        if "x_mask" in kwargs:
            m = kwargs["x_mask"]
            mask = mask * m + torch.ones_like(x) * (~m) * self._mask_floor
        den = self.denoise_fn(x_noisy=x_noisy, net=net, sigmas=sigmas, inference=inference, cond_scale=cond_scale, **kwargs)
        losses = ((den - x) ** 2 * mask).reshape(x.shape[0], -1).sum(dim=1)
        per_sample = float(x[0].numel())
        return losses * self.loss_weight(sigmas) / per_sample


class EluDiffusion(Diffusion):
    """Elucidated diffusion (EDM) preconditioning, table 1 of arXiv:2206.00364."""

    def __init__(self, sigma_data: float, dynamic_threshold: float = 0.0):
        super().__init__(dynamic_threshold)
        self.sigma_data = sigma_data

    def _precond(self):
        return (_lib.PRECOND_EDM, 0.0, 1.0, 1.0)

    def _loss_kind(self):
        return _lib.LOSS_X0_EDM

    # diffusion.py:232-241
    def get_scale_weights(self, sigmas: Tensor, ex_dim: int) -> Tuple[Tensor, ...]:
        sd = self.sigma_data
        c_noise = torch.log(sigmas) * 0.25
        s = _extend(sigmas, ex_dim)
        c_skip = (sd ** 2) / (s ** 2 + sd ** 2)
        c_out = s * sd * (sd ** 2 + s ** 2) ** -0.5
        c_in = (s ** 2 + sd ** 2) ** -0.5
        return c_skip, c_out, c_in, c_noise

    # diffusion.py:243-245
    def loss_weight(self, sigmas: Tensor) -> Tensor:
        return (sigmas ** 2 + self.sigma_data ** 2) * (sigmas * self.sigma_data) ** -2


class VEDiffusion(Diffusion):
    """Variance-exploding preconditioning (diffusion.py:99-133; EDM table 1, column VE)."""

    def __init__(self, dynamic_threshold: float = 0.0):
        super().__init__(dynamic_threshold)

    def _precond(self):
        return (_lib.PRECOND_VE, 0.0, 1.0, 1.0)

    def _loss_kind(self):
        return _lib.LOSS_X0_INV_SIGMA2

    # diffusion.py:107-116
    def get_scale_weights(self, sigmas: Tensor, ex_dim: int) -> Tuple:
        c_noise = (0.5 * sigmas).log()
        sigmas = _extend(sigmas, ex_dim)
        return 1, sigmas, 1, c_noise

    # diffusion.py:118-120
    def loss_weight(self, sigmas: Tensor) -> Tensor:
        return 1 / (sigmas ** 2)


class VPDiffusion(Diffusion):
    """Variance-preserving diffusion in EDM's formulation (diffusion.py:136-218; EDM table 1, column VP)."""

    _mask_floor = 0.1           # :209

    def __init__(self, beta_min: float, beta_d: float, M: float, dynamic_threshold: float = 0.0):
        super().__init__(dynamic_threshold)
        self.beta_min, self.beta_d, self.M = beta_min, beta_d, M

    def _precond(self):
        return (_lib.PRECOND_VP, float(self.beta_min), float(self.beta_d), float(self.M))

    def _loss_kind(self):
        return _lib.LOSS_X0_INV_SIGMA2

    # diffusion.py:152-154
    def loss_weight(self, sigmas: Tensor) -> Tensor:
        return 1 / sigmas ** 2

    # diffusion.py:156-157
    def t_to_sigma(self, t):
        return ((0.5 * self.beta_d * (t ** 2) + self.beta_min * t).exp() - 1).sqrt()

    # diffusion.py:159-160
    def sigma_to_t(self, sigmas):
        return ((self.beta_min ** 2 + 2 * self.beta_d * (1 + sigmas ** 2).log()).sqrt() - self.beta_min) / self.beta_d

    # diffusion.py:162-170
    def get_scale_weights(self, sigmas: Tensor, ex_dim: int) -> Tuple:
        c_noise = (self.M - 1) * self.sigma_to_t(sigmas)
        sigmas = _extend(sigmas, ex_dim)
        c_in = 1 / (sigmas ** 2 + 1).sqrt()
        return 1, -sigmas, c_in, c_noise

    # diffusion.py:185-218: `sigmas` are times t, mapped to sigma first (in torch, on either route: `_device_loss` and `_tensor_loss` take sigmas)
    def forward(self, x: Tensor, net: nn.Module, sigmas: Tensor, inference: bool = False, cond_scale: float = 1.0, **kwargs) -> Tensor:
        return super().forward(x, net, self.t_to_sigma(sigmas), inference=inference, cond_scale=cond_scale, **kwargs)


class VDiffusion(Diffusion):
    """v-prediction (diffusion.py:260-365).  ``for_edm=True`` wraps the v network as an x0 denoiser over sigma = sigma_t / alpha_t, which
    is what the ``sampler_edm`` samplers drive: ``alpha_t x_in - sigma_t v`` with ``x_in = alpha_t x`` and ``alpha_t = sqrt(sigmoid(-2 ln sigma))``,
    returned unclipped (``dynamic_threshold`` is stored and never read, as in the reference).  ``for_edm=False`` returns the raw v prediction
    at the given log-SNR for the reference's ``sampler_vobj`` samplers.  All four are built (samplers.py: ``VSampler``, ``VEulerSampler``, ``VDPMSampler``,
    ``VUniPCSampler``) and run it on the device through rows of their own; ``denoise_fn`` called directly, and every other sampler given it, take the
    compatibility branch as before."""

    _clips = False

    def __init__(self, dynamic_threshold: float = 0.0, logsnr_min=-15, logsnr_max=15, shift=0.0, for_edm: bool = False):
        super().__init__(dynamic_threshold)
        self.logsnr_min, self.logsnr_max, self.shift, self.for_edm = logsnr_min, logsnr_max, shift, for_edm

    def _precond(self):
        return (_lib.PRECOND_V_EDM, 0.0, 1.0, 1.0) if self.for_edm else None

    def _not_native_note(self) -> str:
        return ("" if self.for_edm else ": VDiffusion(for_edm=False) returns the raw v, which only the sampler_vobj samplers take -- VSampler, VEulerSampler, "
                "VDPMSampler and VUniPCSampler run it on the device through rows of their own; for every other caller only for_edm=True has a device form")

    # diffusion.py:282-285
    def shifted_cosine_transform(self, t: Tensor) -> Tensor:
        t_min = math.atan(math.exp(-0.5 * self.logsnr_max))
        t_max = math.atan(math.exp(-0.5 * self.logsnr_min))
        return -2 * (torch.tan(t_min + t * (t_max - t_min)).log()) + 2 * self.shift

    def sigma_to_logsnr(self, sigma):
        return -2 * sigma.log()

    def v_to_x0(self, x_noisy: Tensor, v_pred: Tensor, alphat: Tensor, sigmat: Tensor) -> Tensor:
        return alphat * x_noisy - sigmat * v_pred

    def v_to_eps(self, x_noisy: Tensor, v_pred: Tensor, alphat: Tensor, sigmat: Tensor) -> Tensor:
        return sigmat * x_noisy + alphat * v_pred

    def get_scale_weights(self, sigmas: Tensor, ex_dim: int) -> Tuple[Tensor, ...]:
        """The ``for_edm`` wrapper (:310-313, :290) in the row form the device runs: (c_skip, c_out, c_in, c_noise) =
        (alpha_t^2, -sigma_t, alpha_t, logsnr)."""
        logsnr = self.sigma_to_logsnr(sigmas)
        sigmat = _extend(torch.sqrt(torch.sigmoid(-logsnr)), ex_dim)
        alphat = _extend(torch.sqrt(torch.sigmoid(logsnr)), ex_dim)
        return alphat * alphat, -sigmat, alphat, logsnr

    def loss_weight(self, sigmas: Tensor) -> Tensor:
        """1 / (1 + min(snr, 5)) at the log-SNR values ``forward`` trains at (:357-358)."""
        return 1 / (1 + torch.exp(sigmas).clamp(max=5))

    # diffusion.py:306-326.  The reference multiplies x_noisy by the [B] vector alphat as it is, which broadcasts against the LAST axis and so
    # only runs for B = 1 (or B = W); the per-sample factors are extended to [B, 1, ...] here, which gives what the reference gives sample by sample.
    def _compat_denoise(self, x_noisy: Tensor, net, inference: bool, cond_scale: float, sigmas: Tensor, kwargs: dict) -> Tensor:
        alphat = sigmat = None
        if self.for_edm:
            logsnr = self.sigma_to_logsnr(sigmas)
            sigmat = _extend(torch.sqrt(torch.sigmoid(-logsnr)), x_noisy.ndim)
            alphat = _extend(torch.sqrt(torch.sigmoid(logsnr)), x_noisy.ndim)
            x_noisy = x_noisy * alphat
            sigmas = logsnr
        if inference:
            v_pred = net(x_noisy, sigmas, cond_drop_prob=0.0, **kwargs)
            if cond_scale != 1.0:
                null = net(x_noisy, sigmas, cond_drop_prob=1.0, **kwargs)
                v_pred = null + (v_pred - null) * cond_scale
        else:
            v_pred = net(x_noisy, sigmas, **kwargs)
        return self.v_to_x0(x_noisy, v_pred, alphat, sigmat) if self.for_edm else v_pred

    # diffusion.py:328-365 (training loss on the noise prediction; `sigmas` are times in [0, 1]); no device form (`_loss_kind` is None)
    def _tensor_loss(self, x: Tensor, net: nn.Module, sigmas: Tensor, inference: bool = False, cond_scale: float = 1.0, **kwargs) -> Tensor:
        self._training_guard(net)
        logsnr_t = self.shifted_cosine_transform(sigmas)
        alpha_t = _extend(torch.sqrt(torch.sigmoid(logsnr_t)), x.ndim)
        sigma_t = _extend(torch.sqrt(torch.sigmoid(-logsnr_t)), x.ndim)
        noise = torch.randn_like(x)
        x_noisy = alpha_t * x + sigma_t * noise
        mask = torch.ones_like(x)
        if "x_mask" in kwargs:
            m = kwargs["x_mask"]
            mask = mask * m + torch.ones_like(x) * (~m) * 0.1
        v_pred = self.denoise_fn(x_noisy, net, sigmas=logsnr_t, inference=inference, cond_scale=cond_scale, **kwargs)
        eps_pred = self.v_to_eps(x_noisy, v_pred, alpha_t, sigma_t)
        weight = _extend(self.loss_weight(logsnr_t), x.ndim)
        losses = (weight * (eps_pred - noise) ** 2 * mask).reshape(x.shape[0], -1).sum(dim=1)
        return losses / float(x[0].numel())


class ReFlow(Diffusion):
    """Rectified flow (diffusion.py:367-442).  ``for_edm=False``: ``denoise_fn`` returns the network's velocity ``net(x, t)`` as it is -- the
    "sigma" it is given is already the time t in [0, 1] -- which is what ``ReflowEulerSampler`` and ``DPM2MSampler(reflow=True)`` integrate.
    ``for_edm=True`` wraps the velocity net as an x0 denoiser over sigma = t / (1 - t) (``RFEDMSchedule``) for the ``sampler_edm`` samplers:
    ``t = sigma / (sigma + 1)``, ``x_in = x (1 - t)``, ``x0 = x_in - v t``.  Neither mode clips.  The reference multiplies the [B, C, ...] input by
    the [B] vector ``1 - t`` as it is, which broadcasts against the LAST axis and so only runs for B = 1 (or B = W); the per-sample factors are
    extended to [B, 1, ...] here, which gives what the reference gives sample by sample (as ``VDiffusion`` does)."""

    _clips = False

    def __init__(self, for_edm: bool = False):
        super().__init__(0.0)
        self.for_edm = for_edm

    def _precond(self):
        return (_lib.PRECOND_RF_EDM if self.for_edm else _lib.PRECOND_RF, 0.0, 1.0, 1.0)

    def _loss_kind(self):
        return None if self.for_edm else _lib.LOSS_RF       # for_edm trains the same velocity through the x0 wrapper: tensor route

    # diffusion.py:379-386
    def sigma_to_t(self, t):
        return t / (t + 1)

    def v_to_x0(self, x_noisy: Tensor, v_pred: Tensor, sigmas: Tensor) -> Tensor:
        return x_noisy - v_pred * sigmas

    def v_to_eps(self, x_noisy: Tensor, v_pred: Tensor, sigmas: Tensor) -> Tensor:
        return x_noisy + v_pred * (1 - sigmas)

    # diffusion.py:388-418.  On the device the two modes are the rows (c_in, c_noise, c_skip, c_out) = (1, t, 0, 1) and (1 - t, t, 1 - t, -t).
    def _compat_denoise(self, x_noisy: Tensor, net, inference: bool, cond_scale: float, sigmas: Tensor, kwargs: dict) -> Tensor:
        t = None
        if self.for_edm:
            sigmas = self.sigma_to_t(sigmas)
            t = _extend(sigmas, x_noisy.ndim)
            x_noisy = x_noisy * (1 - t)
        if inference:
            v_pred = net(x_noisy, sigmas, cond_drop_prob=0.0, **kwargs)
            if cond_scale != 1.0:
                null = net(x_noisy, sigmas, cond_drop_prob=1.0, **kwargs)
                v_pred = null + (v_pred - null) * cond_scale
        else:
            v_pred = net(x_noisy, sigmas, **kwargs)
        return self.v_to_x0(x_noisy, v_pred, t) if self.for_edm else v_pred

    # diffusion.py:420-442 (training loss on the velocity; `sigmas` are times in [0, 1])
    def _tensor_loss(self, x: Tensor, net: nn.Module, sigmas: Tensor, inference: bool = False, cond_scale: float = 1.0, **kwargs) -> Tensor:
        self._training_guard(net)
        t = sigmas
        t_padded = _extend(sigmas, x.ndim)
        z1 = torch.randn_like(x)
        zt = (1 - t_padded) * x + t_padded * z1
        zt, t = zt.to(x.dtype), t.to(x.dtype)
        vtheta = self.denoise_fn(zt, net, sigmas=t, inference=inference, cond_scale=cond_scale, **kwargs)
        return ((z1 - x - vtheta) ** 2).mean(dim=list(range(1, x.ndim)))
