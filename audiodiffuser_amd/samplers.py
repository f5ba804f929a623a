"""``model.sampler`` plugins: EDM-family sampling loops and the rectified-flow Euler / Heun loop
(reference: src/models/components/sampler_edm.py:229-300 ``EDMAlphaSampler``, :302-397 ``EDMSampler``,
:495-805 ``DPMSampler``; src/models/components/sampler_rf.py:7-70 ``ReflowEulerSampler``).

Constructor kwargs and ``forward(noise, fn, net, sigmas, **kwargs)`` follow the reference.  When ``fn``
is the ``denoise_fn`` of one of this package's diffusion classes and ``net`` one of its HIP nets, the whole step
loop runs inside ``libadf_hip.so`` (one ``adf_sampler_run`` call, optionally one hipGraph replay): all
branch conditions of the reference loop (``gamma > 0``, ``sigma_next != 0``, warm-up orders) depend only
on the sigma schedule, so they are resolved on the host before anything is enqueued.  For any other
callable the same recurrences are expressed with tensor ops around ``fn`` (interface compatibility).

``VESampler`` / ``VPSampler`` (sampler_edm.py:31-227) and ``VSampler`` / ``VEulerSampler`` (sampler_vobj.py:31-194) go one step further: the host
resolves a run into a table with one record per step -- coefficients of a few whole-state linear combinations and the rows of the step's one or two
denoiser evaluations -- and one generic device loop runs it (``adf_sampler_run_table``; ``_TableSampler`` below).

``VDPMSampler`` / ``VUniPCSampler`` (sampler_vobj.py:196-732) are linear multistep methods: their runs are resolved into a straight-line program over a
few state buffers (``adf_sampler_run_program``; ``_VObjProgramSampler`` at the end of this file).
"""
from __future__ import annotations

import os
from math import atan, exp, sqrt
from typing import Callable, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib
from .diffusion import Diffusion, EluDiffusion, VDiffusion, conditioning_refusal
from .net import HipNet


# ADF_REQUIRE_NATIVE=1 (or ``samplers.REQUIRE_NATIVE = True``): a sampler call that would NOT run inside libadf_hip.so raises
# instead of taking the interface-compatibility branch.  The GPU test-suite sets it (tests/conftest.py), so a refactor that
# silently sends the package's own (fn, net) pair down the tensor-op restatement fails every sampler parity test.
REQUIRE_NATIVE = os.environ.get("ADF_REQUIRE_NATIVE", "0") not in ("", "0")


def _native_pair(fn: Callable, net, cond_scale: float, kwargs: dict, noise: Optional[Tensor] = None,
                 who: str = "sampler") -> Optional[Diffusion]:
    """The whole loop runs inside the HIP library when ``fn`` is the ``denoise_fn`` of one of this package's diffusion classes
    (``EluDiffusion``, ``VEDiffusion``, ``VPDiffusion``, ``VDiffusion(for_edm=True)``, ``ReFlow`` in both modes), ``net`` one of its HIP nets and ``noise``
    lives on a ROCm device.  The only conditioning it understands is ``classes`` (labels) on a
    class-conditional net, where ``cond_scale != 1`` is classifier-free guidance (two network passes per evaluation).
    Returns the owner of ``fn`` (-> device loop) or None (-> interface-compatibility branch)."""
    owner = getattr(fn, "__self__", None)
    why = None
    if not (isinstance(owner, Diffusion) and getattr(fn, "__func__", None) is Diffusion.denoise_fn):
        why = "fn is not the denoise_fn of one of audiodiffuser_amd's diffusion classes"
    elif owner._precond() is None:
        why = "this diffusion class has no device form" + owner._not_native_note()
    elif not isinstance(net, HipNet):
        why = "net is not one of this package's HIP networks"
    elif not 0.0 <= owner.dynamic_threshold <= 1.0:
        why = "dynamic_threshold outside [0, 1]"
    elif noise is not None and not noise.is_cuda:
        why = "noise is not on a ROCm device"
    else:
        why = conditioning_refusal(net, cond_scale, kwargs)
    if why is None:
        return owner
    if REQUIRE_NATIVE:
        raise RuntimeError(f"{who}: ADF_REQUIRE_NATIVE is set and this call would leave the device loop ({why})")
    return None


def _enter(noise: Tensor, net: HipNet, cond_scale: float, kwargs: dict, diff: Optional[Diffusion] = None) -> tuple:
    """The way into every device loop: (the noise as the library takes it, the handle of ``net``), with the handle set for this run.  ``diff``, where
    given, sets the preconditioning and clipping of the owner of ``fn`` (its get_scale_weights; clamp, dynamic threshold or -- VDiffusion -- none,
    diffusion.py:61, :326); then labels + guidance scale (the reference forwards them to every fn call, e.g. sampler_edm.py:341-345)."""
    x = _prep(noise)
    hd = net.native(x.device)
    if diff is not None:
        diff._configure(hd)
    if net.cfg.class_cond:
        hd.set_condition(kwargs["classes"], x.device, null_labels=False, cond_scale=float(cond_scale))
    return x, hd


def _draws(x: Tensor, n: int, injected: Optional[Tensor], needed: bool) -> Optional[Tensor]:
    """The per-step ``randn_like`` draws of a reference loop ([n, B, C, L]).  ``injected`` replaces them after a shape
    check (the C side copies n * B * C * L floats from the pointer).  Without it the draws are made here, one
    ``randn_like`` per step in the reference's order -- ALSO when the schedule never uses them (``needed`` False, e.g.
    s_churn = 0): the reference steps draw unconditionally (sampler_edm.py:346, :439), so the global generator is left
    in the state the reference leaves it in and the next batch's initial noise matches seed for seed."""
    if injected is not None:
        if injected.ndim != x.ndim + 1 or tuple(injected.shape[1:]) != tuple(x.shape) or injected.shape[0] < n:
            raise ValueError(f"injected_noise must be shaped [>= {n}, {', '.join(str(d) for d in x.shape)}] (one draw per step), "
                             f"got {tuple(injected.shape)}")
        return injected[:n].detach().to(device=x.device, dtype=torch.float32).contiguous()
    if not needed or n <= 0:
        scratch = torch.empty_like(x)                # the draws only advance the generator: one buffer, n times
        for _ in range(n):
            scratch.normal_()
        return None
    out = torch.empty((n,) + tuple(x.shape), dtype=x.dtype, device=x.device)     # one [n, *x.shape] tensor filled row by row: the same
    for i in range(n):                                                            # generator, the same order as n randn_like calls,
        out[i].normal_()                                                          # half the transient memory of stack()
    return out


def _prep(noise: Tensor) -> Tensor:
    if noise.ndim not in (3, 4):
        raise ValueError("the HIP sampler expects waveforms shaped [B, C, L] (or [B, C, H, W] for the 2-D UNetModel)")
    return noise.detach().to(torch.float32).contiguous()


class _Sampler(nn.Module):
    """What the eleven samplers share: the way into the device loop.  A sampler gives ``_desc`` (its fields of the descriptor), ``cond_scale``
    and, if its reference loop draws noise, ``_draw_plan``."""

    def _draw_plan(self, sigmas: Tensor) -> Optional[Tuple[int, bool]]:
        """(number of ``randn_like`` draws the reference loop makes on this schedule, whether the device loop reads them), or None."""
        return None

    def _native(self, noise: Tensor, fn: Callable, net, sigmas: Tensor, kwargs: dict, injected_noise: Optional[Tensor] = None) -> Optional[Tensor]:
        """The whole loop as one ``adf_sampler_run``, or None when the call is not native (-> the tensor-op branch).  The order is the
        reference's: the condition is set before the run, and the draws advance the global generator after everything that can refuse."""
        diff = _native_pair(fn, net, self.cond_scale, kwargs, noise, type(self).__name__)
        if diff is None:
            return None
        x, hd = _enter(noise, net, self.cond_scale, kwargs, diff)
        plan = self._draw_plan(sigmas)
        inj = _draws(x, plan[0], injected_noise, plan[1]) if plan is not None else None
        return hd.sampler_run(self._desc(diff.sigma_data), sigmas, x, inj).to(noise.dtype)


class _TableSampler(nn.Module):
    """What the four table-driven samplers share (``VESampler``, ``VPSampler``, ``VSampler``, ``VEulerSampler``): every branch and scalar of their
    reference loops depends on the schedule and the constructor arguments only, so the host resolves a run into one record per step
    (``adf_table_step``, include/audiodiffuser_amd.h) and the device runs the table (``adf_sampler_run_table``).  A sampler gives ``_scalars`` (the
    reference's per-step fp32 scalars, computed with the reference's own torch fp32 op sequence on CPU tensors, so they match it bit for bit),
    ``_table`` (those scalars combined, in double, into the records) and ``_owner`` (whose ``denoise_fn`` makes a call native)."""

    @staticmethod
    def _eval(c_in: float, c_noise: float, c_skip: float, c_out: float, clip: int) -> "_lib.AdfTableEval":
        return _lib.AdfTableEval(c_in=c_in, c_noise=c_noise, c_skip=c_skip, c_out=c_out, clip=clip)

    @staticmethod
    def _step(eval1, a=(1.0, 0.0), b=(1.0, 0.0, 0.0), eval2=None, c=(0.0, 0.0, 0.0, 0.0), draw: int = 0) -> "_lib.AdfTableStep":
        r = _lib.AdfTableStep(a0=a[0], a1=a[1], eval1=eval1, b0=b[0], b1=b[1], b2=b[2], second=int(eval2 is not None),
                              c0=c[0], c1=c[1], c2=c[2], c3=c[3], draw=int(draw))
        if eval2 is not None:
            r.eval2 = eval2
        return r

    def _refuse(self, why: str) -> None:
        if REQUIRE_NATIVE:
            raise RuntimeError(f"{type(self).__name__}: ADF_REQUIRE_NATIVE is set and this call would leave the device loop ({why})")

    def _run_table(self, noise: Tensor, net, owner: Diffusion, kwargs: dict, steps: list, x0_scale: float, final_clamp: bool,
                   n_draws: int, injected_noise: Optional[Tensor], configure: bool) -> Tensor:
        """One ``adf_sampler_run_table`` call.  The order is the other samplers': the condition is set before the run, and the draws advance the
        global generator after everything that can refuse."""
        x, hd = _enter(noise, net, self.cond_scale, kwargs, owner if configure else None)
        inj = _draws(x, n_draws, injected_noise, True) if n_draws > 0 else None
        desc = _lib.AdfTableDesc(num_steps=len(steps), x0_scale=x0_scale, final_clamp=int(final_clamp), use_graph=int(self.use_graph))
        return hd.sampler_run_table(desc, (_lib.AdfTableStep * len(steps))(*steps), x, inj).to(noise.dtype)


class _ChurnTableSampler(_TableSampler):
    """The loop ``VESampler`` and ``VPSampler`` share (sampler_edm.py:55-123, :168-227; EDM algorithm 2 in the time variable of each): churn to
    ``t_hat``, an Euler step to ``t_next`` and, wherever ``t_next != 0``, the Heun correction.  A subclass gives the reference's ``t_to_sigma`` /
    ``sigma_to_t`` / ``t_to_sigma_deriv`` (and, VP, ``scale`` / ``scale_deriv``) and the three scalar groups that differ between the two."""

    _final_clamp = True
    _window = ("s_tmin", "s_tmax")      # the constructor's names of the churn window

    def _x_hat(self, t: Tensor, t_hat: Tensor, nc: Tensor):
        """(coefficient of x, coefficient of randn) of ``x_hat``, fp32, in the reference's order of operations."""
        raise NotImplementedError

    def _slope(self, t: Tensor):
        """(coefficient of x, coefficient of the denoised estimate) of ``d`` at time ``t`` and the factor the state is divided by before ``fn``."""
        raise NotImplementedError

    def _x0(self, sig: Tensor, ts: Tensor) -> Tensor:
        raise NotImplementedError

    def _scalars(self, sigmas: Tensor) -> list:
        """The fp32 scalars of every step as Python floats (each exactly an fp32 value), computed as the reference computes them: the same torch
        ops in the same order on 0-dim / 1-D fp32 CPU tensors.  ``t_hat = sigma_to_t(t_to_sigma(t) + gamma t_to_sigma(t))`` round-trips through
        fp32 also where ``gamma = 0``, so the noise coefficient ``a1`` of such a step is rounding-sized and, in general, not zero -- the reference
        adds that much noise, and so does the table."""
        sig = sigmas.detach().to("cpu", torch.float32)
        ts = self.sigma_to_t(sig)
        ts = torch.cat([ts, torch.zeros_like(ts[:1])])
        lo, hi = (getattr(self, k) for k in self._window)
        gammas = torch.where((sig >= lo) & (sig <= hi), min(self.s_churn / self.num_steps, sqrt(2) - 1), 0.0)
        out = []
        for i in range(self.num_steps):
            t, t_next, gamma = ts[i], ts[i + 1], gammas[i]
            t_hat = self.sigma_to_t(self.t_to_sigma(t) + gamma * self.t_to_sigma(t))
            nc = (self.t_to_sigma(t_hat) ** 2 - self.t_to_sigma(t) ** 2).clip(min=0).sqrt()
            a0, a1 = self._x_hat(t, t_hat, nc)
            kx, kd, div = self._slope(t_hat)
            h = t_next - t_hat
            rec = dict(gamma=gamma, t_hat=t_hat, a0=a0, a1=a1, sigma1=self.t_to_sigma(t_hat), kx1=kx, kd1=kd, div1=div, h=h,
                       second=bool(t_next != 0) and bool(self.use_heun))
            if rec["second"]:
                t_prime = t_hat + h
                kx2, kd2, div2 = self._slope(t_prime)
                rec.update(sigma2=self.t_to_sigma(t_prime), kx2=kx2, kd2=kd2, div2=div2)
            out.append({k: (v if isinstance(v, bool) else float(v)) for k, v in rec.items()})
        out[0]["x0_scale"] = float(self._x0(sig, ts))
        return out

    def _table(self, sigmas: Tensor, owner: Diffusion):
        """(records, x0_scale, final_clamp, draws).  The rows come from ``owner.get_scale_weights`` at the fp32 sigmas the reference hands ``fn``;
        ``fn(x / scale)`` is folded into the row (``c_in / scale``, ``c_skip / scale``), so there is no extra pass."""
        sc = self._scalars(sigmas)
        ev_sig = torch.tensor([v for r in sc for v in ([r["sigma1"], r["sigma2"]] if r["second"] else [r["sigma1"]])], dtype=torch.float32)
        cols = [[float(x) for x in (v.reshape(-1) if isinstance(v, Tensor) else torch.full((len(ev_sig),), float(v)))]
                for v in owner.get_scale_weights(ev_sig, 1)]                  # (c_skip, c_out, c_in, c_noise); VE / VP give Python ints for some
        clip = _lib.CLIP_CONFIGURED if owner._clips else _lib.CLIP_NONE
        k, steps = 0, []

        def ev(div):
            nonlocal k
            c_skip, c_out, c_in, c_noise = (col[k] for col in cols)
            k += 1
            return self._eval(c_in / div, c_noise, c_skip / div, c_out, clip)

        for i, r in enumerate(sc):
            h = r["h"]
            e1 = ev(r["div1"])
            if not r["second"]:
                steps.append(self._step(e1, a=(r["a0"], r["a1"]), b=(1.0 + h * r["kx1"], -h * r["kd1"], 0.0), draw=i))
                continue
            steps.append(self._step(e1, a=(r["a0"], r["a1"]), b=(1.0 + h * r["kx1"], -h * r["kd1"], 0.0), eval2=ev(r["div2"]),
                                    c=(1.0 + 0.5 * h * r["kx1"], -0.5 * h * r["kd1"], 0.5 * h * r["kx2"], -0.5 * h * r["kd2"]), draw=i))
        return steps, sc[0]["x0_scale"], self._final_clamp, self.num_steps       # one randn_like per step, always (sampler_edm.py:63, :176)

    def _owner(self, fn: Callable, net, kwargs: dict, noise: Tensor) -> Optional[Diffusion]:
        owner = _native_pair(fn, net, self.cond_scale, kwargs, noise, type(self).__name__)
        if owner is not None and not hasattr(owner, "get_scale_weights"):
            self._refuse(f"{type(owner).__name__} has no get_scale_weights to take the rows from")
            return None
        return owner

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, injected_noise: Optional[Tensor] = None, **kwargs) -> Tensor:
        owner = self._owner(fn, net, kwargs, noise)
        if owner is not None:
            steps, x0, clamp, n_draws = self._table(sigmas, owner)
            return self._run_table(noise, net, owner, kwargs, steps, x0, clamp, n_draws, injected_noise, configure=True)
        return self._compat(noise, fn, net, sigmas, injected_noise, kwargs)


class VESampler(_ChurnTableSampler):
    """EDM's variance-exploding sampler (sampler_edm.py:31-123): time ``t = sigma^2``, one ``randn_like`` per step, Heun wherever ``t_next != 0``,
    final clamp.  ``injected_noise`` ([num_steps, B, C, L]) replaces the draws."""

    def __init__(self, s_tmin: float = 0, s_tmax: float = float("inf"), s_churn: float = 200, s_noise: float = 1, num_steps: int = 200,
                 cond_scale: float = 1.0, use_heun: bool = True, use_graph: bool = True):
        super().__init__()
        self.s_tmin, self.s_tmax, self.s_churn, self.s_noise = s_tmin, s_tmax, s_churn, s_noise
        self.num_steps, self.cond_scale, self.use_heun, self.use_graph = num_steps, cond_scale, use_heun, use_graph

    def t_to_sigma(self, t: Tensor) -> Tensor:
        return t.sqrt()

    def t_to_sigma_deriv(self, t: Tensor) -> Tensor:
        return 0.5 / t.sqrt()

    def sigma_to_t(self, sigma: Tensor) -> Tensor:
        return sigma ** 2

    def _x_hat(self, t, t_hat, nc):
        return 1.0, nc * self.s_noise                                                     # :63

    def _slope(self, t):
        r = self.t_to_sigma_deriv(t) / self.t_to_sigma(t)                                 # :72, :85: the same quotient in front of x and of the estimate
        return r, r, 1.0

    def _x0(self, sig, ts):
        return sig[0]                                                                     # :115

    def _compat(self, noise, fn, net, sigmas, injected_noise, kwargs):
        """sampler_edm.py:55-123 as written."""
        ts = self.sigma_to_t(sigmas)
        ts = torch.cat([ts, torch.zeros_like(ts[:1])])
        gammas = torch.where((sigmas >= self.s_tmin) & (sigmas <= self.s_tmax), min(self.s_churn / self.num_steps, sqrt(2) - 1), 0.0)
        call = lambda x_, t_: fn(x_, net=net, sigma=self.t_to_sigma(t_), inference=True, cond_scale=self.cond_scale, **kwargs)
        x = noise * sigmas[0]
        for i in range(self.num_steps):
            t, t_next, gamma = ts[i], ts[i + 1], gammas[i]
            eps = injected_noise[i] if injected_noise is not None else torch.randn_like(x)
            t_hat = self.sigma_to_t(self.t_to_sigma(t) + gamma * self.t_to_sigma(t))
            x_hat = x + (self.t_to_sigma(t_hat) ** 2 - self.t_to_sigma(t) ** 2).clip(min=0).sqrt() * self.s_noise * eps
            r = self.t_to_sigma_deriv(t_hat) / self.t_to_sigma(t_hat)
            d = r * x_hat - r * call(x_hat, t_hat)
            h = t_next - t_hat
            x = x_hat + h * d
            if t_next != 0 and self.use_heun:
                t_prime = t_hat + h
                r2 = self.t_to_sigma_deriv(t_prime) / self.t_to_sigma(t_prime)
                d_prime = r2 * x - r2 * call(x, t_prime)
                x = x_hat + 1 / 2 * h * (d + d_prime)
        return x.clamp(-1.0, 1.0)


class VPSampler(_ChurnTableSampler):
    """EDM's variance-preserving sampler (sampler_edm.py:125-227): the state is ``scale(t) * (x0 + sigma(t) noise)``, ``fn`` sees ``x / scale(t)``;
    one ``randn_like`` per step, Heun wherever ``t_next != 0``; the result is returned UNCLAMPED, as in the reference.  ``injected_noise``
    ([num_steps, B, C, L]) replaces the draws."""

    _final_clamp = False
    _window = ("s_min", "s_max")

    def __init__(self, beta_d: float = 19.9, beta_min: float = 0.1, s_churn: float = 200.0, s_noise: float = 1.0, s_min: float = 0.0,
                 s_max: float = float("inf"), num_steps: int = 200, cond_scale: float = 1.0, use_heun: bool = True, use_graph: bool = True):
        super().__init__()
        self.beta_d, self.beta_min, self.s_noise, self.s_churn, self.s_min, self.s_max = beta_d, beta_min, s_noise, s_churn, s_min, s_max
        self.num_steps, self.cond_scale, self.use_heun, self.use_graph = num_steps, cond_scale, use_heun, use_graph

    def t_to_sigma(self, t: Tensor) -> Tensor:
        return ((0.5 * self.beta_d * (t ** 2) + self.beta_min * t).exp() - 1) ** 0.5

    def sigma_to_t(self, sigma: Tensor) -> Tensor:
        return ((self.beta_min ** 2 + 2 * self.beta_d * (sigma ** 2 + 1).log()).sqrt() - self.beta_min) / self.beta_d

    def t_to_sigma_deriv(self, t: Tensor) -> Tensor:
        return 0.5 * (self.beta_min + self.beta_d * t) * (self.t_to_sigma(t) + 1 / self.t_to_sigma(t))

    def scale(self, t: Tensor) -> Tensor:
        return 1 / (1 + self.t_to_sigma(t) ** 2).sqrt()

    def scale_deriv(self, t: Tensor) -> Tensor:
        return -self.t_to_sigma(t) * self.t_to_sigma_deriv(t) * (self.scale(t) ** 3)

    def _x_hat(self, t, t_hat, nc):
        return self.scale(t_hat) / self.scale(t), nc * self.scale(t_hat) * self.s_noise                                  # :176

    def _slope(self, t):
        return (self.t_to_sigma_deriv(t) / self.t_to_sigma(t) + self.scale_deriv(t) / self.scale(t),                     # :184, :196
                self.t_to_sigma_deriv(t) * self.scale(t) / self.t_to_sigma(t), self.scale(t))

    def _x0(self, sig, ts):
        return sig[0].double() * self.scale(ts[0]).double()                                                               # :218

    def _compat(self, noise, fn, net, sigmas, injected_noise, kwargs):
        """sampler_edm.py:168-227 as written."""
        ts = self.sigma_to_t(sigmas)
        ts = torch.cat([ts, torch.zeros_like(ts[:1])])
        gammas = torch.where((sigmas >= self.s_min) & (sigmas <= self.s_max), min(self.s_churn / self.num_steps, sqrt(2) - 1), 0.0)
        call = lambda x_, t_: fn(x_ / self.scale(t_), net=net, sigma=self.t_to_sigma(t_), inference=True, cond_scale=self.cond_scale, **kwargs)
        slope = lambda x_, t_: ((self.t_to_sigma_deriv(t_) / self.t_to_sigma(t_) + self.scale_deriv(t_) / self.scale(t_)) * x_
                                - self.t_to_sigma_deriv(t_) * self.scale(t_) / self.t_to_sigma(t_) * call(x_, t_))
        x = noise * sigmas[0] * self.scale(ts[0])
        for i in range(self.num_steps):
            t, t_next, gamma = ts[i], ts[i + 1], gammas[i]
            eps = injected_noise[i] if injected_noise is not None else torch.randn_like(x)
            t_hat = self.sigma_to_t(self.t_to_sigma(t) + gamma * self.t_to_sigma(t))
            x_hat = (self.scale(t_hat) / self.scale(t) * x
                     + (self.t_to_sigma(t_hat) ** 2 - self.t_to_sigma(t) ** 2).clip(min=0).sqrt() * self.scale(t_hat) * self.s_noise * eps)
            d = slope(x_hat, t_hat)
            h = t_next - t_hat
            x = x_hat + h * d
            if t_next != 0 and self.use_heun:
                x = x_hat + 1 / 2 * h * (d + slope(x, t_hat + h))
        return x


class _VObjTableSampler(_TableSampler):
    """What ``VSampler`` and ``VEulerSampler`` share (sampler_vobj.py:31-194): ``sigmas`` are times in [0, 1], mapped by the SAMPLER's shifted cosine
    schedule to the log-SNR the v network is evaluated at; ``fn`` is the ``denoise_fn`` of a ``VDiffusion(for_edm=False)``, which returns the
    raw v prediction.  That class keeps ``_precond() is None`` (no other sampler may take it), so these two have their own pair check."""

    def shifted_cosine_transform(self, t: Tensor) -> Tensor:
        t_min = atan(exp(-0.5 * self.logsnr_max))
        t_max = atan(exp(-0.5 * self.logsnr_min))
        return -2 * (torch.tan(t_min + t * (t_max - t_min)).log()) + 2 * self.shift

    def _scalars(self, sigmas: Tensor) -> list:
        """Per step the reference's fp32 scalars (Python floats, each exactly an fp32 value), by its own op sequence on 0-dim CPU tensors."""
        ts = sigmas.detach().to("cpu", torch.float32)
        ts = torch.cat([ts, torch.zeros_like(ts[:1])])
        out = []
        for i in range(self.num_steps):
            t, t_next = ts[i], ts[i + 1]
            lt, ls = self.shifted_cosine_transform(t), self.shifted_cosine_transform(t_next)
            rec = dict(logsnr_t=lt, logsnr_s=ls, alpha_t=torch.sqrt(torch.sigmoid(lt)), sigma_t=torch.sqrt(torch.sigmoid(-lt)),
                       alpha_s=torch.sqrt(torch.sigmoid(ls)), sigma_s=torch.sqrt(torch.sigmoid(-ls)), last=bool(t_next == 0))
            self._more_scalars(rec)
            out.append({k: (v if isinstance(v, bool) else float(v)) for k, v in rec.items()})
        return out

    def _owner(self, fn: Callable, net, kwargs: dict, noise: Tensor) -> Optional[VDiffusion]:
        owner = getattr(fn, "__self__", None)
        if not (isinstance(owner, VDiffusion) and getattr(fn, "__func__", None) is Diffusion.denoise_fn):
            why = "fn is not the denoise_fn of an audiodiffuser_amd VDiffusion"
        elif owner.for_edm:
            why = "VDiffusion(for_edm=True) is an x0 denoiser over sigma: it goes with the sampler_edm samplers, these two take the raw v of for_edm=False"
        elif not isinstance(net, HipNet):
            why = "net is not one of this package's HIP networks"
        elif not noise.is_cuda:
            why = "noise is not on a ROCm device"
        else:
            why = conditioning_refusal(net, self.cond_scale, kwargs)
        if why is None:
            return owner
        self._refuse(why)
        return None

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, injected_noise: Optional[Tensor] = None, **kwargs) -> Tensor:
        owner = self._owner(fn, net, kwargs, noise)
        if owner is not None:
            steps, n_draws = self._table(sigmas)
            return self._run_table(noise, net, owner, kwargs, steps, 1.0, True, n_draws, injected_noise, configure=False)
        return self._compat(noise, fn, net, sigmas, injected_noise, kwargs)


class VSampler(_VObjTableSampler):
    """The stochastic v-diffusion sampler of simple diffusion (sampler_vobj.py:111-194): per step one v prediction, ``x_pred = clamp(alpha_t x -
    sigma_t v)``, the posterior mean towards the next log-SNR and, wherever ``t_next != 0``, one ``randn_like`` draw at the posterior variance;
    final clamp.  ``injected_noise`` ([that many, B, C, L]) replaces the draws."""

    def __init__(self, logsnr_min=-15, logsnr_max=15, shift=0.0, num_steps=200, cond_scale=1.0, use_graph: bool = True):
        super().__init__()
        self.logsnr_min, self.logsnr_max, self.shift = logsnr_min, logsnr_max, shift
        self.num_steps, self.cond_scale, self.use_graph = num_steps, cond_scale, use_graph

    def _more_scalars(self, rec: dict) -> None:
        rec["c"] = -torch.special.expm1(rec["logsnr_t"] - rec["logsnr_s"])                     # :154
        rec["std"] = torch.sqrt((rec["sigma_s"] ** 2) * rec["c"])                              # :156, :159

    def _table(self, sigmas: Tensor):
        """The row (1, logsnr_t, alpha_t, -sigma_t) with the unit clamp makes the evaluation's epilogue yield ``x_pred`` itself."""
        steps, k = [], 0
        for r in self._scalars(sigmas):
            e = self._eval(1.0, r["logsnr_t"], r["alpha_t"], -r["sigma_t"], _lib.CLIP_UNIT)
            b = (r["alpha_s"] * (1.0 - r["c"]) / r["alpha_t"], r["alpha_s"] * r["c"], 0.0 if r["last"] else r["std"])
            steps.append(self._step(e, b=b, draw=k))
            k += 0 if r["last"] else 1
        return steps, k

    def _compat(self, noise, fn, net, sigmas, injected_noise, kwargs):
        """sampler_vobj.py:131-194 as written."""
        ts = torch.cat([sigmas, torch.zeros_like(sigmas[:1])])
        x, k = noise, 0
        for i in range(self.num_steps):
            t, t_next = ts[i], ts[i + 1]
            lt, ls = self.shifted_cosine_transform(t), self.shifted_cosine_transform(t_next)
            v = fn(x, net=net, sigma=lt, inference=True, cond_scale=self.cond_scale, **kwargs)
            alpha_t, sigma_t = torch.sqrt(torch.sigmoid(lt)), torch.sqrt(torch.sigmoid(-lt))
            alpha_s, sigma_s = torch.sqrt(torch.sigmoid(ls)), torch.sqrt(torch.sigmoid(-ls))
            x_pred = (alpha_t * x - sigma_t * v).clamp(-1.0, 1.0)
            c = -torch.special.expm1(lt - ls)
            mu = alpha_s * (x * (1 - c) / alpha_t + c * x_pred)
            if t_next != 0:
                eps = injected_noise[k] if injected_noise is not None else torch.randn_like(mu)
                k += 1
                mu = mu + eps * torch.sqrt((sigma_s ** 2) * c)
            x = mu
        return x.clamp(-1.0, 1.0)


class VEulerSampler(_VObjTableSampler):
    """The deterministic sibling (sampler_vobj.py:31-109): an Euler step of the probability-flow ODE in log-SNR, with ``use_heun`` a second v
    prediction at the next log-SNR; the step into ``t_next = 0`` returns ``alpha_t x - sigma_t v``; final clamp.  It draws nothing;
    ``injected_noise`` is accepted for the shared signature and ignored."""

    def __init__(self, logsnr_min=-15, logsnr_max=15, shift=0.5, num_steps=200, cond_scale=1.0, use_heun=False, use_graph: bool = True):
        super().__init__()
        self.logsnr_min, self.logsnr_max, self.shift = logsnr_min, logsnr_max, shift
        self.num_steps, self.cond_scale, self.use_heun, self.use_graph = num_steps, cond_scale, use_heun, use_graph

    def _more_scalars(self, rec: dict) -> None:
        dl = rec["logsnr_s"] - rec["logsnr_t"]
        rec.update(k_cur=-rec["alpha_t"] * rec["sigma_t"], k_next=-rec["alpha_s"] * rec["sigma_s"], half_dl=0.5 * dl, quarter_dl=0.25 * dl)      # :76-83

    def _table(self, sigmas: Tensor):
        """The row (1, logsnr, 0, 1) without a clip: the evaluation is the raw v."""
        steps = []
        for r in self._scalars(sigmas):
            e = self._eval(1.0, r["logsnr_t"], 0.0, 1.0, _lib.CLIP_NONE)
            if r["last"]:
                steps.append(self._step(e, b=(r["alpha_t"], -r["sigma_t"], 0.0)))
            elif not self.use_heun:
                steps.append(self._step(e, b=(1.0, r["half_dl"] * r["k_cur"], 0.0)))
            else:
                steps.append(self._step(e, b=(1.0, r["half_dl"] * r["k_cur"], 0.0), eval2=self._eval(1.0, r["logsnr_s"], 0.0, 1.0, _lib.CLIP_NONE),
                                        c=(1.0, r["quarter_dl"] * r["k_cur"], 0.0, r["quarter_dl"] * r["k_next"])))
        return steps, 0

    def _compat(self, noise, fn, net, sigmas, injected_noise, kwargs):
        """sampler_vobj.py:53-109 as written."""
        ts = torch.cat([sigmas, torch.zeros_like(sigmas[:1])])
        x = noise
        for i in range(self.num_steps):
            t, t_next = ts[i], ts[i + 1]
            lt, ls = self.shifted_cosine_transform(t), self.shifted_cosine_transform(t_next)
            v = fn(x, net=net, sigma=lt, inference=True, cond_scale=self.cond_scale, **kwargs)
            alpha_t, sigma_t = torch.sqrt(torch.sigmoid(lt)), torch.sqrt(torch.sigmoid(-lt))
            alpha_s, sigma_s = torch.sqrt(torch.sigmoid(ls)), torch.sqrt(torch.sigmoid(-ls))
            if t_next == 0.0:
                x = alpha_t * x - sigma_t * v
                continue
            score = -alpha_t * sigma_t * v
            x_next = x + 0.5 * (ls - lt) * score
            if self.use_heun:
                v_next = fn(x_next, net=net, sigma=ls, inference=True, cond_scale=self.cond_scale, **kwargs)
                x_next = x + 0.25 * (ls - lt) * (-alpha_s * sigma_s * v_next + score)
            x = x_next
        return x.clamp(-1.0, 1.0)


class EDMSampler(_Sampler):
    """EDM stochastic sampler (Heun, optional churn); ``s_churn=0`` is the deterministic Heun ODE solver."""

    def __init__(self, s_tmin: float = 0, s_tmax: float = float("inf"), s_churn: float = 150.0, s_noise: float = 1.04,
                 num_steps: int = 200, cond_scale: float = 1.0, use_heun: bool = True, use_graph: bool = True):
        super().__init__()
        self.s_tmin, self.s_tmax, self.s_noise, self.s_churn = s_tmin, s_tmax, s_noise, s_churn
        self.num_steps, self.cond_scale, self.use_heun, self.use_graph = num_steps, cond_scale, use_heun, use_graph

    def _desc(self, sigma_data: float) -> "_lib.AdfSamplerDesc":
        return _lib.make_sampler_desc(_lib.SAMPLER_EDM, self.num_steps, sigma_data, self.use_graph, s_tmin=self.s_tmin, s_tmax=min(self.s_tmax, 3.0e38),
                                      s_churn=self.s_churn, s_noise=self.s_noise, use_heun=int(self.use_heun))

    def _draw_plan(self, sigmas):
        return self.num_steps, self.s_churn > 0           # one draw per step, read where gamma > 0 (sampler_edm.py:346)

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, injected_noise: Optional[Tensor] = None,
                **kwargs) -> Tensor:
        y = self._native(noise, fn, net, sigmas, kwargs, injected_noise)
        if y is not None:
            return y
        # ---- interface-compatibility branch (sampler_edm.py:333-397) -----------------------------
        sig = torch.cat([sigmas, torch.zeros_like(sigmas[:1])])
        x = sig[0] * noise
        gam = torch.where((sig >= self.s_tmin) & (sig <= self.s_tmax), min(self.s_churn / self.num_steps, sqrt(2) - 1), 0.0)
        for i in range(self.num_steps):
            s, s_next, g = sig[i], sig[i + 1], gam[i]
            eps = injected_noise[i] if injected_noise is not None else torch.randn_like(x)
            eps = self.s_noise * eps
            if g > 0:
                s_hat = s + g * s
                x_hat = x + (s_hat ** 2 - s ** 2) ** 0.5 * eps
            else:
                s_hat, x_hat = s, x
            d = (x_hat - fn(x_hat, net=net, sigma=s_hat, inference=True, cond_scale=self.cond_scale, **kwargs)) / s_hat
            x = x_hat + (s_next - s_hat) * d
            if s_next != 0 and self.use_heun:
                d2 = (x - fn(x, net=net, sigma=s_next, inference=True, cond_scale=self.cond_scale, **kwargs)) / s_next
                x = x_hat + 0.5 * (s_next - s_hat) * (d + d2)
        return x


class EDMAlphaSampler(_Sampler):
    """EDM algorithm 3, generalised second-order Runge-Kutta; ``alpha=1`` is Heun."""

    def __init__(self, alpha: float = 1.0, num_steps: int = 50, cond_scale: float = 1.0, use_heun: bool = True,
                 use_graph: bool = True):
        super().__init__()
        self.alpha, self.num_steps, self.cond_scale, self.use_heun, self.use_graph = alpha, num_steps, cond_scale, use_heun, use_graph

    def _desc(self, sigma_data: float) -> "_lib.AdfSamplerDesc":
        return _lib.make_sampler_desc(_lib.SAMPLER_EDM_ALPHA, self.num_steps, sigma_data, self.use_graph, use_heun=int(self.use_heun), alpha=self.alpha)

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, **kwargs) -> Tensor:
        y = self._native(noise, fn, net, sigmas, kwargs)
        if y is not None:
            return y
        x = sigmas[0] * noise                                            # sampler_edm.py:284-300
        for i in range(self.num_steps - 1):
            s, s_next = sigmas[i], sigmas[i + 1]
            h = s_next - s
            d = (x - fn(x, net=net, sigma=s, inference=True, cond_scale=self.cond_scale, **kwargs)) / s
            s_p = s + self.alpha * h
            if s_p != 0 and self.use_heun:
                x_p = x + self.alpha * h * d
                d_p = (x_p - fn(x_p, net=net, sigma=s_p, inference=True, cond_scale=self.cond_scale, **kwargs)) / s_p
                x = x + h * ((1 - 0.5 / self.alpha) * d + 0.5 / self.alpha * d_p)
            else:
                x = x + h * d
        return x


class DPMSampler(_Sampler):
    """DPM-Solver with x0 prediction (sampler_edm.py:495-805): the multistep solver (``multisteps=True``; the shipped
    configuration is configs/experiment/sc09_inference/diffunet_complex_sc09_eval_dpm.yaml:57-64 with
    ``log_time_spacing=False``) and the single-step "DPM-Solver-fast" (``multisteps=False``), each on the sigma grid
    itself or on a grid linear in log sigma.  The reference's quirks are kept: without log spacing the single-step run
    walks only ``len(orders)`` intervals of the sigma list (stops early) and its intermediate points add a
    lambda-space step to a sigma (:584, :604).  ``x0_pred=False`` is the noise-prediction form of every update (:700-706); combined with the single-step
    solver on the sigma grid the reference itself returns NaN, and so does this class."""

    def __init__(self, cond_scale, order=1, num_steps=10, multisteps=False, x0_pred: bool = True,
                 log_time_spacing: bool = True, use_graph: bool = True):
        super().__init__()
        self.order, self.cond_scale, self.multisteps = order, cond_scale, multisteps
        self.x0_pred, self.log_time_spacing, self.use_graph = x0_pred, log_time_spacing, use_graph
        self.ctor_num_steps = num_steps
        self.num_steps = num_steps if log_time_spacing else num_steps - 1      # sampler_edm.py:526

    def _check_supported(self) -> None:
        if self.order not in (1, 2, 3):
            raise ValueError("'order' must be '1' or '2' or '3'.")

    def singlestep_orders(self):
        """sampler_edm.py:770-789."""
        n, order = self.num_steps, self.order
        if order == 3:
            k = n // 3 + 1
            return ([3] * (k - 2) + [2, 1] if n % 3 == 0 else [3] * (k - 1) + [n % 3]), k
        if order == 2:
            return ([2] * (n // 2) if n % 2 == 0 else [2] * (n // 2) + [1]), (n + 1) // 2
        return [1] * n, n

    def nfe(self) -> int:
        return self.num_steps if self.multisteps else sum(self.singlestep_orders()[0])

    def _desc(self, sigma_data: float) -> "_lib.AdfSamplerDesc":
        return _lib.make_sampler_desc(_lib.SAMPLER_DPM_MULTISTEP if self.multisteps else _lib.SAMPLER_DPM_SINGLESTEP, self.ctor_num_steps, sigma_data,
                                      self.use_graph, order=int(self.order), log_time_spacing=int(bool(self.log_time_spacing)),
                                      eps_pred=int(not self.x0_pred))

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, **kwargs) -> Tensor:
        self._check_supported()
        y = self._native(noise, fn, net, sigmas, kwargs)
        if y is not None:
            return y
        # ---- interface-compatibility branch (sampler_edm.py:710-805, :568-690) --------------------
        if not self.x0_pred:
            raise NotImplementedError("DPMSampler(x0_pred=False) with a foreign net / fn: noise prediction runs on the native path only")
        call = lambda x, s: fn(x, net=net, sigma=s, inference=True, cond_scale=self.cond_scale, **kwargs)
        if self.log_time_spacing:           # grid of lambda = -log sigma (:546-552); lambd = inv_lambd = identity
            lam = inv = lambda v: v
            sig = lambda l: l.neg().exp()
            grid_of = lambda n: torch.linspace(-sigmas[0].log(), -sigmas[-1].log(), n + 1)
        else:                               # the grid is the sigma list (:556)
            lam = lambda v: -v.log()
            sig = lambda v: v
            inv = lambda l: l.neg().exp()
            grid_of = lambda n: sigmas
        x = sigmas[0] * noise
        if not self.multisteps:
            orders, k = self.singlestep_orders()
            grid = grid_of(k)
            for i, o in enumerate(orders):
                cur, nxt = grid[i], grid[i + 1]
                h = lam(nxt) - lam(cur)
                eps = call(x, sig(cur))
                base = sig(nxt) / sig(cur) * x - torch.expm1(-h) * eps
                if o == 1:
                    x = base
                elif o == 2:
                    r1 = 1 / 2
                    s1 = inv(cur + r1 * h)
                    u1 = sig(s1) / sig(cur) * x - torch.expm1(-r1 * h) * eps
                    x = base - 1 / (2 * r1) * torch.expm1(-h) * (call(u1, sig(s1)) - eps)
                else:
                    r1, r2 = 1 / 3, 2 / 3
                    s1, s2 = inv(cur + r1 * h), inv(cur + r2 * h)
                    u1 = sig(s1) / sig(cur) * x - (-r1 * h).expm1() * eps
                    eps_r1 = call(u1, sig(s1))
                    u2 = (sig(s2) / sig(cur) * x - (-r2 * h).expm1() * eps
                          + (r2 / r1) * ((-r2 * h).expm1() / (r2 * h) + 1) * (eps_r1 - eps))
                    x = base + 1 / r2 * (torch.expm1(-h) / h + 1) * (call(u2, sig(s2)) - eps)
            return x.clamp(-1.0, 1.0)
        steps, order = self.num_steps, self.order
        assert steps >= order
        grid = grid_of(steps)
        s_hist, m_hist = [grid[0]], [call(x, sig(grid[0]))]
        for step in range(1, steps + 1):
            o = step if step < order else min(order, steps + 1 - step)
            s_cur, s0 = grid[step], s_hist[-1]
            h = lam(s_cur) - lam(s0)
            phi1 = torch.expm1(-h)
            new = sig(s_cur) / sig(s0) * x - phi1 * m_hist[-1]
            if o == 2:
                r0 = (lam(s0) - lam(s_hist[-2])) / h
                new = new - 0.5 * phi1 * ((1.0 / r0) * (m_hist[-1] - m_hist[-2]))
            elif o == 3:
                r0 = (lam(s0) - lam(s_hist[-2])) / h
                r1 = (lam(s_hist[-2]) - lam(s_hist[-3])) / h
                d10 = (1.0 / r0) * (m_hist[-1] - m_hist[-2])
                d11 = (1.0 / r1) * (m_hist[-2] - m_hist[-3])
                d1 = d10 + (r0 / (r0 + r1)) * (d10 - d11)
                d2 = (1.0 / (r0 + r1)) * (d10 - d11)
                phi2 = phi1 / h + 1.0
                phi3 = phi2 / h - 0.5
                new = new + phi2 * d1 - phi3 * d2
            x = new
            s_hist = (s_hist + [s_cur])[-order:]
            if step < steps:
                m_hist = (m_hist + [call(x, sig(s_cur))])[-order:]
        return x.clamp(-1.0, 1.0)


class DPM2MSampler(_Sampler):
    """'DPM-Solver++(2M) Karras' (sampler_edm.py:1056-1131).  The loop reads ``sigmas[i + 1]`` for ``i < num_steps``: the schedule
    must hold ``num_steps + 1`` entries (a final 0 returns the last denoised estimate); with the module's own N-entry schedule the
    reference raises IndexError on its last step, and so does this class.  ``reflow`` is the constructor flag of the class of the same
    name in stochastic_sampler_edm.py:180-259 (otherwise the same recurrence): the network output is read as a velocity,
    ``denoised = x - output * sigma`` (:214-215)."""

    def __init__(self, num_steps: int = 50, cond_scale: float = 1.0, reflow: bool = False, use_graph: bool = True):
        super().__init__()
        self.num_steps, self.cond_scale, self.reflow, self.use_graph = num_steps, cond_scale, reflow, use_graph

    def _desc(self, sigma_data: float) -> "_lib.AdfSamplerDesc":
        return _lib.make_sampler_desc(_lib.SAMPLER_DPM2M, self.num_steps, sigma_data, self.use_graph, order=2, reflow=int(bool(self.reflow)))

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, **kwargs) -> Tensor:
        if len(sigmas) < self.num_steps + 1:
            raise IndexError(f"index {self.num_steps} is out of bounds for dimension 0 with size {len(sigmas)}")
        y = self._native(noise, fn, net, sigmas, kwargs)
        if y is not None:
            return y
        # ---- interface-compatibility branch --------------------------------------------------------
        x = sigmas[0] * noise
        old = None
        for i in range(self.num_steps):
            s_last, s, s_next = sigmas[i - 1], sigmas[i], sigmas[i + 1]
            den = fn(x, net=net, sigma=s, inference=True, cond_scale=self.cond_scale, **kwargs)
            if self.reflow:
                den = x - den * s
            t, t_next = s.log().neg(), s_next.log().neg()
            h = t_next - t
            t_min, t_max = min(t_next.neg().exp(), t.neg().exp()), max(t_next.neg().exp(), t.neg().exp())
            if old is None or s_next == 0:
                x = (t_min / t_max) * x - (-h).expm1() * den
            else:
                h_last = t - s_last.log().neg()
                h_min, h_max = min(h_last, h), max(h_last, h)
                r = h_max / h_min
                h_d = (h_max + h_min) / 2
                x = (t_min / t_max) * x - (-h_d).expm1() * ((1 + 1 / (2 * r)) * den - (1 / (2 * r)) * old)
            old = den
        return x.clamp(-1.0, 1.0)


class ReflowEulerSampler(_Sampler):
    """Rectified-flow Euler sampler with a fixed schedule (sampler_rf.py:7-70): ``fn`` returns the velocity (``ReFlow(for_edm=False)``), one
    evaluation per step plus a Heun correction wherever ``sigma_next != 0``; the result is clamped to [-1, 1].  The loop reads
    ``sigmas[i + 1]`` for ``i < num_steps``: the schedule must hold ``num_steps + 1`` entries (``LinearSchedule(1, 0, num_steps + 1)``); with
    ``num_steps`` entries the reference raises IndexError on its last step, and so does this class, before anything runs."""

    def __init__(self, num_steps: int = 200, cond_scale: float = 1.0, use_heun: bool = True, use_graph: bool = True):
        super().__init__()
        self.num_steps, self.cond_scale, self.use_heun, self.use_graph = num_steps, cond_scale, use_heun, use_graph

    def _desc(self, sigma_data: float) -> "_lib.AdfSamplerDesc":
        return _lib.make_sampler_desc(_lib.SAMPLER_RF_EULER, self.num_steps, sigma_data, self.use_graph, use_heun=int(bool(self.use_heun)))

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, **kwargs) -> Tensor:
        if len(sigmas) < self.num_steps + 1:
            raise IndexError(f"index {self.num_steps} is out of bounds for dimension 0 with size {len(sigmas)}")
        y = self._native(noise, fn, net, sigmas, kwargs)
        if y is not None:
            return y
        # ---- interface-compatibility branch (sampler_rf.py:24-70) ---------------------------------
        x = sigmas[0] * noise
        for i in range(self.num_steps):
            s, s_next = sigmas[i], sigmas[i + 1]
            v = fn(x, net=net, sigma=s, inference=True, cond_scale=self.cond_scale, **kwargs)
            x_next = x + (s_next - s) * v
            if s_next != 0 and self.use_heun:
                v_next = fn(x_next, net=net, sigma=s_next, inference=True, cond_scale=self.cond_scale, **kwargs)
                x_next = x + 0.5 * (s_next - s) * (v + v_next)
            x = x_next
        return x.clamp(-1.0, 1.0)


class LMSSampler(_Sampler):
    """'LMS Karras' linear multistep solver (sampler_edm.py:1134-1190): ``num_steps - 1`` evaluations, the last ``order``
    derivatives combined with the integrals of their Lagrange basis polynomials over the step (the reference integrates
    them with scipy ``quad`` on fp32 NumPy scalars, so its values carry ~1e-7 relative noise that depends on the NumPy
    version's promotion rules; they are cubics at most, so 3-point Gauss-Legendre in double is exact)."""

    def __init__(self, num_steps: int = 50, cond_scale: float = 1.0, order: int = 4, use_graph: bool = True):
        super().__init__()
        self.num_steps, self.cond_scale, self.order, self.use_graph = num_steps, cond_scale, order, use_graph

    @staticmethod
    def linear_multistep_coeff(order: int, t, i: int, j: int) -> float:
        if order - 1 > i:
            raise ValueError(f"Order {order} too high for step {i}")
        a, b = float(t[i]), float(t[i + 1])
        half, mid, acc = 0.5 * (b - a), 0.5 * (a + b), 0.0
        for gx, gw in ((-0.7745966692414834, 5 / 9), (0.0, 8 / 9), (0.7745966692414834, 5 / 9)):
            tau, prod = mid + half * gx, 1.0
            for k in range(order):
                if k != j:
                    prod *= (tau - float(t[i - k])) / (float(t[i - j]) - float(t[i - k]))
            acc += gw * prod
        return acc * half

    def _desc(self, sigma_data: float) -> "_lib.AdfSamplerDesc":
        return _lib.make_sampler_desc(_lib.SAMPLER_LMS, self.num_steps, sigma_data, self.use_graph, order=int(self.order))

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, **kwargs) -> Tensor:
        if not 1 <= self.order <= 4:
            raise ValueError("LMSSampler: order must be 1..4")
        y = self._native(noise, fn, net, sigmas, kwargs)
        if y is not None:
            return y
        # ---- interface-compatibility branch --------------------------------------------------------
        t = sigmas.detach().cpu().numpy()
        x = sigmas[0] * noise
        ds = []
        for i in range(self.num_steps - 1):
            d = (x - fn(x, net=net, sigma=sigmas[i], inference=True, cond_scale=self.cond_scale, **kwargs)) / sigmas[i]
            ds = (ds + [d])[-self.order:]
            cur = min(i + 1, self.order)
            coeffs = [self.linear_multistep_coeff(cur, t, i, j) for j in range(cur)]
            x = x + sum(c * dd for c, dd in zip(coeffs, reversed(ds)))
        return x.clamp(-1.0, 1.0)


class DPM2Sampler(_Sampler):
    """'DPM2 Karras' (reference: src/models/components/sampler_edm.py:401-493): midpoint method in log-sigma with the
    EDM churn.  ``injected_noise`` ([num_steps-1, B, C, L]) replaces the per-step ``randn_like`` draws."""

    def __init__(self, rho: float = 2.0, num_steps: int = 50, cond_scale: float = 1.0, s_tmin: float = 0,
                 s_tmax: float = float("inf"), s_churn: float = 150.0, s_noise: float = 1.04, use_graph: bool = True):
        super().__init__()
        self.rho, self.num_steps, self.cond_scale = rho, num_steps, cond_scale
        self.s_tmin, self.s_tmax, self.s_noise, self.s_churn, self.use_graph = s_tmin, s_tmax, s_noise, s_churn, use_graph

    def _desc(self, sigma_data: float) -> "_lib.AdfSamplerDesc":
        return _lib.make_sampler_desc(_lib.SAMPLER_DPM2, self.num_steps, sigma_data, self.use_graph, s_tmin=self.s_tmin, s_tmax=min(self.s_tmax, 3.0e38),
                                      s_churn=self.s_churn, s_noise=self.s_noise, rho=float(self.rho), eta=1.0)

    def _draw_plan(self, sigmas):
        return self.num_steps - 1, self.s_churn > 0       # one draw per step, read where gamma > 0 (sampler_edm.py:439)

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, injected_noise: Optional[Tensor] = None,
                **kwargs) -> Tensor:
        y = self._native(noise, fn, net, sigmas, kwargs, injected_noise)
        if y is not None:
            return y
        # ---- interface-compatibility branch (sampler_edm.py:428-493) ----------------------------------
        x = sigmas[0] * noise
        gam = torch.where((sigmas >= self.s_tmin) & (sigmas <= self.s_tmax), min(self.s_churn / self.num_steps, sqrt(2) - 1), 0.0)
        for i in range(self.num_steps - 1):
            s, s_next, g = sigmas[i], sigmas[i + 1], gam[i]
            s_hat = s + g * s
            eps = self.s_noise * (injected_noise[i] if injected_noise is not None else torch.randn_like(x))
            x_hat = x + (s_hat ** 2 - s ** 2) ** 0.5 * eps if g > 0 else x
            d = (x_hat - fn(x_hat, net=net, sigma=s_hat, inference=True, cond_scale=self.cond_scale, **kwargs)) / s_hat
            if s_next == 0.0:
                x = x + d * (s_next - s_hat)
            else:
                s_mid = s_hat.log().lerp(s_next.log(), 0.5).exp()
                x_2 = x + d * (s_mid - s_hat)
                d_2 = (x_2 - fn(x_2, net=net, sigma=s_mid, inference=True, cond_scale=self.cond_scale, **kwargs)) / s_mid
                x = x + d_2 * (s_next - s_hat)
        return x.clamp(-1.0, 1.0)


class ADPM2Sampler(_Sampler):
    """'DPM2 a Karras', the ancestral DPM-Solver-2 (reference: src/models/components/stochastic_sampler_edm.py:35-100;
    the Lightning module's default sampler).  Fresh noise of scale sigma_up is added every step:
    ``injected_noise`` ([num_steps-1, B, C, L]) replaces those ``randn_like`` draws."""

    def __init__(self, rho: float = 1.0, num_steps: int = 50, cond_scale: float = 1.0, eta: float = 1.0, use_graph: bool = True):
        super().__init__()
        self.rho, self.num_steps, self.cond_scale, self.eta, self.use_graph = rho, num_steps, cond_scale, eta, use_graph

    def _desc(self, sigma_data: float) -> "_lib.AdfSamplerDesc":
        return _lib.make_sampler_desc(_lib.SAMPLER_ADPM2, self.num_steps, sigma_data, self.use_graph, s_tmax=3.0e38, rho=float(self.rho), eta=float(self.eta))

    def _draw_plan(self, sigmas):
        return self.num_steps - 1, True                   # one draw per step (stochastic_sampler_edm.py:82)

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, injected_noise: Optional[Tensor] = None,
                **kwargs) -> Tensor:
        y = self._native(noise, fn, net, sigmas, kwargs, injected_noise)
        if y is not None:
            return y
        # ---- interface-compatibility branch (stochastic_sampler_edm.py:29-32, :53-100) -----------------
        x = sigmas[0] * noise
        for i in range(self.num_steps - 1):
            s, s_next = sigmas[i], sigmas[i + 1]
            s_up = min(s_next, self.eta * (s_next ** 2 * (s ** 2 - s_next ** 2) / s ** 2) ** 0.5)
            s_down = (s_next ** 2 - s_up ** 2) ** 0.5
            d = (x - fn(x, net=net, sigma=s, inference=True, cond_scale=self.cond_scale, **kwargs)) / s
            s_mid = ((s ** (1 / self.rho) + s_down ** (1 / self.rho)) / 2) ** self.rho
            x_mid = x + d * (s_mid - s)
            d_mid = (x_mid - fn(x_mid, net=net, sigma=s_mid, inference=True, cond_scale=self.cond_scale, **kwargs)) / s_mid
            x = x + d_mid * (s_down - s)
            x = x + (injected_noise[i] if injected_noise is not None else torch.randn_like(x)) * s_up
        return x.clamp(-1.0, 1.0)


class ADPMPP2SSampler(_Sampler):
    """'DPM++ 2S a Karras', ancestral DPM-Solver++(2S) (reference: src/models/components/stochastic_sampler_edm.py:102-178):
    ``num_steps - 1`` steps of two evaluations (one when sigma_down is 0), fresh noise of scale sigma_up after every step whose
    sigma_next is positive -- ``injected_noise`` ([that many, B, C, L]) replaces those ``randn_like`` draws.  ``rho`` is accepted and,
    as in the reference, never read."""

    def __init__(self, rho: float = 1.0, num_steps: int = 50, cond_scale: float = 1.0, eta: float = 1.0, use_graph: bool = True):
        super().__init__()
        self.rho, self.num_steps, self.cond_scale, self.eta, self.use_graph = rho, num_steps, cond_scale, eta, use_graph

    def _desc(self, sigma_data: float) -> "_lib.AdfSamplerDesc":
        return _lib.make_sampler_desc(_lib.SAMPLER_ADPMPP2S, self.num_steps, sigma_data, self.use_graph, s_tmax=3.0e38, rho=float(self.rho),
                                      eta=float(self.eta))

    def _draw_plan(self, sigmas):
        return int((sigmas[1:self.num_steps].detach().cpu() > 0).sum()), True      # one draw per step with sigma_next > 0 (:158)

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, injected_noise: Optional[Tensor] = None,
                **kwargs) -> Tensor:
        y = self._native(noise, fn, net, sigmas, kwargs, injected_noise)
        if y is not None:
            return y
        # ---- interface-compatibility branch (stochastic_sampler_edm.py:29-32, :117-178) ----------------
        x = sigmas[0] * noise
        k = 0
        for i in range(self.num_steps - 1):
            s, s_next = sigmas[i], sigmas[i + 1]
            den = fn(x, net=net, sigma=s, inference=True, cond_scale=self.cond_scale, **kwargs)
            s_up = min(s_next, self.eta * (s_next ** 2 * (s ** 2 - s_next ** 2) / s ** 2) ** 0.5)
            s_down = (s_next ** 2 - s_up ** 2) ** 0.5
            if s_down == 0:
                x = x + (x - den) / s * (s_down - s)
            else:
                t, t_next = s.log().neg(), s_down.log().neg()
                h = t_next - t
                sm = t + 0.5 * h
                x_2 = (sm.neg().exp() / t.neg().exp()) * x - (-h * 0.5).expm1() * den
                den_2 = fn(x_2, net=net, sigma=sm.neg().exp(), inference=True, cond_scale=self.cond_scale, **kwargs)
                x = (t_next.neg().exp() / t.neg().exp()) * x - (-h).expm1() * den_2
            if s_next > 0:
                x = x + (injected_noise[k] if injected_noise is not None else torch.randn_like(x)) * s_up
                k += 1
        return x.clamp(-1.0, 1.0)


class UniPCSampler(_Sampler):
    """Uni-PC (sampler_edm.py:807-1053, variant 'bh2'): multistep predictor-corrector, NFE = its step count -- ``num_steps`` on a lambda
    grid linear between the first and the last sigma (``log_time_spacing``, the default) or ``num_steps - 1`` on the sigma list itself.
    The reference only runs on 4-D states (hard-coded ``einsum('k,bkchw->bchw')``); here any state shape works."""

    def __init__(self, num_steps: int = 20, order: int = 2, cond_scale: float = 1.0, x0_pred: bool = True,
                 log_time_spacing: bool = True, use_graph: bool = True):
        super().__init__()
        self.order, self.cond_scale, self.x0_pred, self.log_time_spacing = order, cond_scale, x0_pred, log_time_spacing
        self._ctor_steps = num_steps
        self.num_steps = num_steps if log_time_spacing else num_steps - 1        # as the reference stores it (:828)
        self.use_graph = use_graph

    def _desc(self, sigma_data: float) -> "_lib.AdfSamplerDesc":
        return _lib.make_sampler_desc(_lib.SAMPLER_UNIPC, self._ctor_steps, sigma_data, self.use_graph, order=int(self.order),
                                      log_time_spacing=int(self.log_time_spacing), eps_pred=int(not self.x0_pred))

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, **kwargs) -> Tensor:
        assert self.num_steps >= self.order                                        # :1001
        y = self._native(noise, fn, net, sigmas, kwargs)
        if y is not None:
            return y
        # ---- interface-compatibility branch (same recurrences as tensor ops around a foreign fn / net) ----------------------------
        steps, order = self.num_steps, self.order
        if self.log_time_spacing:
            grid = torch.linspace(-sigmas[0].log(), -sigmas[-1].log(), steps + 1).to(noise.device)
            lam, sig = (lambda v: v), (lambda v: v.neg().exp())
        else:
            grid = sigmas.to(noise.device)
            lam, sig = (lambda v: -v.log()), (lambda v: v)

        def model(x_, g):
            den = fn(x_, net=net, sigma=sig(g), inference=True, cond_scale=self.cond_scale, **kwargs)
            return den if self.x0_pred else (x_ - den) / sig(g)

        def update(x_, ml, gl, g_cur, ord_, corr):
            g0, m0 = gl[-1], ml[-1]
            h = (lam(g_cur) - lam(g0)).view(-1)
            rks, d1s = [], []
            for i in range(1, ord_):
                rk = (lam(gl[-(i + 1)]) - lam(g0)) / h
                rks.append(rk)
                d1s.append((ml[-(i + 1)] - m0) / rk)
            rks = torch.tensor([float(r) for r in rks] + [1.0], device=noise.device)
            hh = -h if self.x0_pred else h
            h_phi_1 = torch.expm1(hh)
            h_phi_k, b_h, fact = h_phi_1 / hh - 1, torch.expm1(hh), 1
            R, b = [], []
            for i in range(1, ord_ + 1):
                R.append(torch.pow(rks, i - 1))
                b.append(h_phi_k * fact / b_h)
                fact *= i + 1
                h_phi_k = h_phi_k / hh - 1 / fact
            R, b = torch.stack(R), torch.cat(b)
            rho_p = (torch.tensor([0.5], device=noise.device) if ord_ == 2 else torch.linalg.solve(R[:-1, :-1], b[:-1])) if d1s else None
            scale = 1.0 if self.x0_pred else sig(g_cur)
            xt_ = sig(g_cur) / sig(g0) * x_ - h_phi_1 * m0 if self.x0_pred else x_ - sig(g_cur) * h_phi_1 * m0
            comb = lambda rho: sum(rho[k] * d for k, d in enumerate(d1s)) if d1s else 0
            x_t, m_t = xt_ - scale * b_h * comb(rho_p), None
            if corr:
                rho_c = torch.tensor([0.5], device=noise.device) if ord_ == 1 else torch.linalg.solve(R, b)
                m_t = model(x_t, g_cur)
                x_t = xt_ - scale * b_h * (comb(rho_c[:-1]) + rho_c[-1] * (m_t - m0))
            return x_t, m_t

        x = sigmas[0] * noise
        ml, gl = [model(x, grid[0])], [grid[0]]
        for step in range(1, order):
            x, m = update(x, ml, gl, grid[step], step, True)
            gl.append(grid[step]); ml.append(m)
        for step in range(order, steps + 1):
            x, m = update(x, ml, gl, grid[step], min(order, steps + 1 - step), step != steps)
            for i in range(order - 1):
                gl[i], ml[i] = gl[i + 1], ml[i + 1]
            gl[-1] = grid[step]
            if step < steps:
                ml[-1] = m
        return x.clamp(-1.0, 1.0)


class _VObjProgramSampler(_VObjTableSampler):
    """What ``VDPMSampler`` and ``VUniPCSampler`` share (sampler_vobj.py:196-732): linear multistep methods over the raw v of a
    ``VDiffusion(for_edm=False)``.  A step reads the state and up to three earlier model outputs, so the per-step record of ``_TableSampler`` cannot
    hold them; the host resolves a run into a straight-line program over a few state buffers instead (``adf_prog_op``,
    include/audiodiffuser_amd.h) and the device runs it (``adf_sampler_run_program``).  ``_scalars`` gives the reference's fp32 scalars (its own torch
    op sequence on CPU tensors), ``_program`` combines them in double into the ops; the history of a method is renamed from step to step, never copied.

    Both samplers read ``sigmas[0]`` and ``sigmas[-1]`` only, map them through the shifted cosine transform with the hard-wired
    ``logsnr_min = -15, logsnr_max = 15, shift = 0`` (:227-233, :540-546) and walk ``linspace`` between the two; ``sigma(l) = sqrt(sigmoid(-l))`` is the
    noise level, ``sigma(-l)`` is alpha, and every step width enters halved.  The model output ``alpha x - sigma v`` (``x0_pred``) or
    ``sigma x + alpha v`` is one evaluation with the row (1, l, alpha, -sigma) or (1, l, sigma, alpha) and no clip: the epilogue writes it."""

    logsnr_min, logsnr_max, shift = -15, 15, 0.0
    _MAX_ORDER = 3

    @staticmethod
    def _sig(l: Tensor) -> Tensor:
        return torch.sqrt(torch.sigmoid(-l))

    def _grid(self, sigmas: Tensor, n: int) -> Tensor:
        s = sigmas.detach().to("cpu", torch.float32)
        return torch.linspace(self.shifted_cosine_transform(s[0]), self.shifted_cosine_transform(s[-1]), n + 1)

    def _row(self, l: float) -> "_lib.AdfTableEval":
        """The model output at log-SNR ``l`` as one row; alpha and sigma as the reference forms them in fp32."""
        t = torch.tensor(l, dtype=torch.float32)
        sig, alp = float(self._sig(t)), float(self._sig(-t))
        return self._eval(1.0, l, alp, -sig, _lib.CLIP_NONE) if self.x0_pred else self._eval(1.0, l, sig, alp, _lib.CLIP_NONE)

    @staticmethod
    def _ev(dst: int, src: int, e: "_lib.AdfTableEval") -> "_lib.AdfProgOp":
        return _lib.AdfProgOp(kind=_lib.PROG_EVAL, dst=dst, src=src, eval=e)

    @staticmethod
    def _lin(dst: int, terms, clamp: bool = False) -> "_lib.AdfProgOp":
        """``terms``: (slot, coefficient) pairs; a slot named twice is summed here (in double), a zero coefficient is not an operand."""
        acc = {}
        for slot, k in terms:
            acc[slot] = acc.get(slot, 0.0) + float(k)
        acc = [(s, k) for s, k in acc.items() if k != 0.0] or [(terms[0][0], 0.0)]
        op = _lib.AdfProgOp(kind=_lib.PROG_LIN, dst=dst, n_terms=len(acc), clamp=int(clamp))
        for j, (s, k) in enumerate(acc):
            op.slot[j], op.coef[j] = s, k
        return op

    def _class_drop(self) -> Optional[str]:
        """Why this run cannot be native on a class-conditional net (the reference drops ``classes`` on some evaluations), or None."""
        raise NotImplementedError

    def _owner(self, fn: Callable, net, kwargs: dict, noise: Tensor) -> Optional[VDiffusion]:
        owner = super()._owner(fn, net, kwargs, noise)
        if owner is None:
            return None
        why = None
        if not 1 <= self.order <= self._MAX_ORDER:
            why = f"order = {self.order}: the device program covers orders 1 to {self._MAX_ORDER}"
        elif net.cfg.class_cond:
            why = self._class_drop()
        if why is None:
            return owner
        self._refuse(why)
        return None

    def _run_program(self, noise: Tensor, net, kwargs: dict, ops: list, x0_scale: float, result_slot: int) -> Tensor:
        x, hd = _enter(noise, net, self.cond_scale, kwargs)
        desc = _lib.AdfProgDesc(num_ops=len(ops), result_slot=result_slot, x0_scale=x0_scale, use_graph=int(self.use_graph))
        return hd.sampler_run_program(desc, (_lib.AdfProgOp * len(ops))(*ops), x).to(noise.dtype)

    @torch.no_grad()
    def forward(self, noise: Tensor, fn: Callable, net: nn.Module, sigmas: Tensor, **kwargs) -> Tensor:
        self._check()
        if self._owner(fn, net, kwargs, noise) is not None:
            ops, x0_scale, result = self._program(sigmas)
            return self._run_program(noise, net, kwargs, ops, x0_scale, result)
        return self._compat(noise, fn, net, sigmas, kwargs)


class VDPMSampler(_VObjProgramSampler):
    """``sampler_vobj.DPMSampler`` (sampler_vobj.py:196-499): DPM-Solver in the halved log-SNR, orders 1 to 3, single-step ("DPM-Solver-fast", the
    order list ``[3] * (K - 2) + [2, 1]`` etc. of :465-481) or multistep; the start state is ``noise`` itself, the result is clamped.  What the
    reference does and this class keeps: the single-step inner evaluations are called without ``**kwargs`` (``classes`` reaches only the first
    evaluation of a step, :286-314); the multistep order-1 update calls ``fn`` and discards the result whenever the model output is handed in (:323,
    one dead network pass at step 1 and one at every trailing order-1 step).  The device program skips the dead passes -- they change nothing -- and
    the tensor-op branch makes them."""

    def __init__(self, cond_scale, order=1, num_steps=10, multisteps=False, x0_pred: bool = True, use_graph: bool = True):
        super().__init__()
        self.order, self.num_steps, self.cond_scale, self.multisteps, self.x0_pred, self.use_graph = order, num_steps, cond_scale, multisteps, x0_pred, use_graph

    def _check(self) -> None:
        if self.multisteps:
            assert self.num_steps >= self.order                                           # :401
        elif self.order not in (1, 2, 3):
            raise ValueError("'order' must be '1' or '2' or '3'.")                        # :483

    def singlestep_orders(self):
        """(orders, K) of sampler_vobj.py:465-481."""
        n, order = self.num_steps, self.order
        if order == 3:
            k = n // 3 + 1
            return ([3] * (k - 2) + [2, 1] if n % 3 == 0 else [3] * (k - 1) + [n % 3]), k
        if order == 2:
            return ([2] * (n // 2), n // 2) if n % 2 == 0 else ([2] * (n // 2) + [1], n // 2 + 1)
        return [1] * n, n

    def multistep_orders(self):
        """The order of the update into grid point 1 .. num_steps (:423-452)."""
        n, order = self.num_steps, self.order
        return [step if step < order else min(order, n + 1 - step) for step in range(1, n + 1)]

    def _class_drop(self) -> Optional[str]:
        if self.multisteps or all(o == 1 for o in self.singlestep_orders()[0]):
            return None
        return ("the reference drops `classes` on the inner evaluations of a single-step update of order 2 or 3 (sampler_vobj.py:286-314): "
                "a class-conditional run is native in multistep mode or with an all-order-1 list")

    def _scalars(self, sigmas: Tensor) -> dict:
        """``grid`` (the log-SNR list) and per step the reference's fp32 scalars as Python floats, each formed by its own sequence of torch
        operations on 0-dim CPU tensors: ``l`` the log-SNRs the step evaluates at, ``A`` the coefficient of x and the products in front of the model
        outputs / differences, per intermediate state (single-step) or per update (multistep)."""
        sig, x0 = self._sig, self.x0_pred
        num = (lambda l: sig(l)) if x0 else (lambda l: sig(-l))               # the factor in front of x: sigma ratio (x0) or alpha ratio
        fac = (lambda l: sig(-l)) if x0 else (lambda l: sig(l))               # the factor in front of the model output: alpha (x0) or sigma
        em = (lambda v: torch.expm1(-v)) if x0 else (lambda v: torch.expm1(v))
        fl = lambda d: {k: ([float(u) for u in v] if isinstance(v, (list, tuple)) else v if isinstance(v, int) else float(v)) for k, v in d.items()}
        steps = []
        if not self.multisteps:
            orders, k = self.singlestep_orders()
            grid = self._grid(sigmas, k)
            for i, o in enumerate(orders):
                lc, ln = grid[i], grid[i + 1]
                h = ln - lc
                if o == 1:
                    h = h / 2
                    rec = dict(order=1, l=[lc], A3=num(ln) / num(lc), B3=fac(ln) * em(h))
                elif o == 2:
                    r1 = 1 / 2
                    s1 = lc + r1 * h
                    h = h / 2
                    rec = dict(order=2, l=[lc, s1], A1=num(s1) / num(lc), B1=fac(s1) * em(r1 * h), A3=num(ln) / num(lc), B3=fac(ln) * em(h),
                               C3=fac(ln) / (2 * r1) * em(h))
                else:
                    r1, r2 = 1 / 3, 2 / 3
                    s1 = lc + r1 * h
                    s2 = lc + r2 * h
                    h = h / 2
                    if x0:
                        c2 = sig(-s2) * (r2 / r1) * ((-r2 * h).expm1() / (r2 * h) + 1)
                        c3 = sig(-ln) * 1 / r2 * (torch.expm1(-h) / h + 1)
                    else:
                        c2 = sig(s2) * (r2 / r1) * ((r2 * h).expm1() / (r2 * h) - 1)
                        c3 = sig(ln) / r2 * (h.expm1() / h - 1)
                    rec = dict(order=3, l=[lc, s1, s2], A1=num(s1) / num(lc), B1=fac(s1) * em(r1 * h), A2=num(s2) / num(lc), B2=fac(s2) * em(r2 * h),
                               C2=c2, A3=num(ln) / num(lc), B3=fac(ln) * em(h), C3=c3)
                steps.append(fl(rec))
            return dict(grid=[float(v) for v in grid], steps=steps)
        grid = self._grid(sigmas, self.num_steps)
        for step, o in enumerate(self.multistep_orders(), start=1):
            lc, l0 = grid[step], grid[step - 1]
            h = lc - l0
            rec = dict(order=o, l=[lc] if step < self.num_steps else [])
            if o >= 2:
                rec["inv_r0"] = 1. / ((l0 - grid[step - 2]) / h)
            if o == 3:
                r0, r1 = (l0 - grid[step - 2]) / h, (grid[step - 2] - grid[step - 3]) / h
                rec.update(inv_r1=1. / r1, q=r0 / (r0 + r1), w=1. / (r0 + r1))
            h = h / 2
            phi1 = em(h)
            rec.update(A=num(lc) / num(l0), B=fac(lc) * phi1)
            if o == 2:
                rec["C"] = fac(lc) * 0.5 * phi1 if x0 else 0.5 * (fac(lc) * phi1)
            if o == 3:
                phi2 = phi1 / h + 1. if x0 else phi1 / h - 1.
                phi3 = phi2 / h - 0.5
                rec.update(P2=fac(lc) * phi2, P3=fac(lc) * phi3)
            steps.append(fl(rec))
        return dict(grid=[float(v) for v in grid], steps=steps)

    def _program(self, sigmas: Tensor):
        """(ops, x0_scale, result slot).  Single-step: x in slot 0, the step's model outputs in 1, 3, 4 and its intermediate state in 2.  Multistep: x in
        slot 0, the history in slots renamed from step to step; the discarded evaluations of the reference are not part of the program."""
        sc, x0 = self._scalars(sigmas), self.x0_pred
        ops, n = [], len(sc["steps"])
        if not self.multisteps:
            X, E0, U, E1, E2 = 0, 1, 2, 3, 4
            for i, r in enumerate(sc["steps"]):
                last = i + 1 == n
                ops.append(self._ev(E0, X, self._row(r["l"][0])))
                if r["order"] == 1:
                    ops.append(self._lin(X, [(X, r["A3"]), (E0, -r["B3"])], last))
                    continue
                ops += [self._lin(U, [(X, r["A1"]), (E0, -r["B1"])]), self._ev(E1, U, self._row(r["l"][1]))]
                if r["order"] == 2:
                    ops.append(self._lin(X, [(X, r["A3"]), (E0, -r["B3"] + r["C3"]), (E1, -r["C3"])], last))
                    continue
                s = 1.0 if x0 else -1.0                                     # the sign of the difference terms (:306-315)
                ops += [self._lin(U, [(X, r["A2"]), (E0, -r["B2"] - s * r["C2"]), (E1, s * r["C2"])]), self._ev(E2, U, self._row(r["l"][2])),
                        self._lin(X, [(X, r["A3"]), (E0, -r["B3"] - s * r["C3"]), (E2, s * r["C3"])], last)]
            return ops, 1.0, 0
        X, free, hist = 0, [1, 2, 3, 4], []
        hist.append(free.pop(0))
        ops.append(self._ev(hist[-1], X, self._row(sc["grid"][0])))
        for step, r in enumerate(sc["steps"], start=1):
            o = r["order"]
            m = hist[::-1]                                                  # m[0] the newest
            if o == 1:
                terms = [(m[0], -r["B"])]
            elif o == 2:
                terms = [(m[0], -r["B"] - r["C"] * r["inv_r0"]), (m[1], r["C"] * r["inv_r0"])]
            else:
                i0, i1, q, w = r["inv_r0"], r["inv_r1"], r["q"], r["w"]
                e = (i0, -(i0 + i1), i1)                                    # D1_0 - D1_1 over (m0, m1, m2)
                d1 = (i0 + q * e[0], -i0 + q * e[1], q * e[2])
                s = 1.0 if x0 else -1.0
                terms = [(m[j], (-r["B"] if j == 0 else 0.0) + s * r["P2"] * d1[j] - r["P3"] * w * e[j]) for j in range(3)]
            ops.append(self._lin(X, [(X, r["A"])] + terms, step == n))
            if step < n:
                if len(hist) == self.order:
                    free.append(hist.pop(0))
                hist.append(free.pop(0))
                ops.append(self._ev(hist[-1], X, self._row(r["l"][0])))
        return ops, 1.0, 0

    def _compat(self, noise, fn, net, sigmas, kwargs):
        """sampler_vobj.py:389-499 as written, dead calls and dropped keywords included."""
        sig, x0 = self._sig, self.x0_pred
        call = lambda x_, l, **kw: fn(x_, net=net, sigma=l, inference=True, cond_scale=self.cond_scale, **kw)

        def model(x_, l, **kw):
            v = call(x_, l, **kw)
            return sig(-l) * x_ - sig(l) * v if x0 else sig(l) * x_ + sig(-l) * v

        x = noise
        l_start, l_end = self.shifted_cosine_transform(sigmas[0]), self.shifted_cosine_transform(sigmas[-1])
        if not self.multisteps:
            orders, k = self.singlestep_orders()
            grid = torch.linspace(l_start, l_end, k + 1, device=x.device)
            for i, o in enumerate(orders):
                lc, ln = grid[i], grid[i + 1]
                eps = model(x, lc, **kwargs)
                h = ln - lc
                if o == 1:
                    h = h / 2
                    x = sig(ln) / sig(lc) * x - sig(-ln) * (-h).expm1() * eps if x0 else sig(-ln) / sig(-lc) * x - sig(ln) * h.expm1() * eps
                elif o == 2:
                    r1 = 1 / 2
                    s1 = lc + r1 * h
                    h = h / 2
                    if x0:
                        u1 = sig(s1) / sig(lc) * x - sig(-s1) * torch.expm1(-r1 * h) * eps
                        e1 = model(u1, s1)
                        x = sig(ln) / sig(lc) * x - sig(-ln) * torch.expm1(-h) * eps - sig(-ln) / (2 * r1) * torch.expm1(-h) * (e1 - eps)
                    else:
                        u1 = sig(-s1) / sig(-lc) * x - sig(s1) * (r1 * h).expm1() * eps
                        e1 = model(u1, s1)
                        x = sig(-ln) / sig(-lc) * x - sig(ln) * h.expm1() * eps - sig(ln) / (2 * r1) * h.expm1() * (e1 - eps)
                else:
                    r1, r2 = 1 / 3, 2 / 3
                    s1 = lc + r1 * h
                    s2 = lc + r2 * h
                    h = h / 2
                    if x0:
                        u1 = sig(s1) / sig(lc) * x - sig(-s1) * (-r1 * h).expm1() * eps
                        e1 = model(u1, s1)
                        u2 = (sig(s2) / sig(lc) * x - sig(-s2) * (-r2 * h).expm1() * eps
                              + sig(-s2) * (r2 / r1) * ((-r2 * h).expm1() / (r2 * h) + 1) * (e1 - eps))
                        e2 = model(u2, s2)
                        x = sig(ln) / sig(lc) * x - sig(-ln) * torch.expm1(-h) * eps + sig(-ln) * 1 / r2 * (torch.expm1(-h) / h + 1) * (e2 - eps)
                    else:
                        u1 = sig(-s1) / sig(-lc) * x - sig(s1) * (r1 * h).expm1() * eps
                        e1 = model(u1, s1)
                        u2 = (sig(-s2) / sig(-lc) * x - sig(s2) * (r2 * h).expm1() * eps
                              - sig(s2) * (r2 / r1) * ((r2 * h).expm1() / (r2 * h) - 1) * (e1 - eps))
                        e2 = model(u2, s2)
                        x = sig(-ln) / sig(-lc) * x - sig(ln) * h.expm1() * eps - sig(ln) / r2 * (h.expm1() / h - 1) * (e2 - eps)
            return x.clamp(-1.0, 1.0)

        def update(x_, o, ml, ll, lc):
            l0, m0 = ll[-1], ml[-1]
            h = lc - l0
            if o == 1:
                h = h / 2
                call(x_, l0, **kwargs)                                      # :323: evaluated and discarded, the model output is handed in
                phi1 = torch.expm1(-h) if x0 else torch.expm1(h)
                return sig(lc) / sig(l0) * x_ - sig(-lc) * phi1 * m0 if x0 else sig(-lc) / sig(-l0) * x_ - sig(lc) * phi1 * m0
            if o == 2:
                r0 = (l0 - ll[-2]) / h
                d10 = (1. / r0) * (m0 - ml[-2])
                h = h / 2
                if x0:
                    phi1 = torch.expm1(-h)
                    return sig(lc) / sig(l0) * x_ - sig(-lc) * phi1 * m0 - sig(-lc) * 0.5 * phi1 * d10
                phi1 = torch.expm1(h)
                return sig(-lc) / sig(-l0) * x_ - (sig(lc) * phi1) * m0 - 0.5 * (sig(lc) * phi1) * d10
            if o == 3:
                l2, l1, l0 = ll                                             # exactly three entries, as the reference unpacks them (:360)
                m2, m1, m0 = ml
                r0, r1 = (l0 - l1) / h, (l1 - l2) / h
                h = h / 2
                d10, d11 = (1. / r0) * (m0 - m1), (1. / r1) * (m1 - m2)
                d1 = d10 + (r0 / (r0 + r1)) * (d10 - d11)
                d2 = (1. / (r0 + r1)) * (d10 - d11)
                if x0:
                    phi1 = torch.expm1(-h)
                    phi2 = phi1 / h + 1.
                    phi3 = phi2 / h - 0.5
                    return sig(lc) / sig(l0) * x_ - sig(-lc) * phi1 * m0 + sig(-lc) * phi2 * d1 - sig(-lc) * phi3 * d2
                phi1 = torch.expm1(h)
                phi2 = phi1 / h - 1.
                phi3 = phi2 / h - 0.5
                return sig(-lc) / sig(-l0) * x_ - (sig(lc) * phi1) * m0 - (sig(lc) * phi2) * d1 - (sig(lc) * phi3) * d2
            return x_                                                       # no branch of :446-452 matches an order above 3

        n, order = self.num_steps, self.order
        grid = torch.linspace(l_start, l_end, n + 1, device=x.device)
        ml, ll = [model(x, grid[0], **kwargs)], [grid[0]]
        for step in range(1, order):
            x = update(x, step, ml, ll, grid[step])
            ll.append(grid[step])
            ml.append(model(x, grid[step], **kwargs))
        for step in range(order, n + 1):
            x = update(x, min(order, n + 1 - step), ml, ll, grid[step])
            for i in range(order - 1):
                ll[i], ml[i] = ll[i + 1], ml[i + 1]
            ll[-1] = grid[step]
            if step < n:
                ml[-1] = model(x, grid[step], **kwargs)
        return x.clamp(-1.0, 1.0)


class VUniPCSampler(_VObjProgramSampler):
    """``sampler_vobj.UniPCSampler`` (sampler_vobj.py:502-732, variant 'bh2'): multistep predictor-corrector in the halved log-SNR, one corrector
    evaluation per step except the last (NFE = ``num_steps``); the start state is ``sigmas[0] * noise``, the result is clamped.  What the reference
    does and this class keeps: the corrector's evaluation gets no keywords (``forward`` hands none to ``multistep_uni_pc_update``, :694, :715); with
    ``x0_pred`` the corrector line lacks the alpha factor the predictor has (:644 against :634); for order 3 ``rhos_p`` / ``rhos_c`` come from
    ``torch.linalg.solve`` in fp32.  The reference's ``einsum('k,bkchw->bchw')`` runs orders >= 2 on 4-D states only; here any rank works and on 4-D
    input the result is the reference's."""

    def __init__(self, num_steps: int = 20, order: int = 2, cond_scale: float = 1.0, x0_pred: bool = True, use_graph: bool = True):
        super().__init__()
        self.num_steps, self.order, self.cond_scale, self.x0_pred, self.use_graph = num_steps, order, cond_scale, x0_pred, use_graph

    def _check(self) -> None:
        assert self.num_steps >= self.order                                               # :677

    def update_plan(self):
        """(order, corrector?) of the update into grid point 1 .. num_steps (:692-719)."""
        n, order = self.num_steps, self.order
        return [(step, True) if step < order else (min(order, n + 1 - step), step != n) for step in range(1, n + 1)]

    def _class_drop(self) -> Optional[str]:
        if not any(corr for _, corr in self.update_plan()):
            return None
        return ("the reference drops `classes` on every corrector evaluation (sampler_vobj.py:694, :715 hand multistep_uni_pc_update no keywords): "
                "a class-conditional run is native only without one (num_steps = 1)")

    def _update_scalars(self, ll: list, lc: Tensor, o: int, corr: bool) -> dict:
        """multistep_uni_pc_update (:551-668) up to the state arithmetic: every scalar on fp32 tensors in the reference's order."""
        sig, x0 = self._sig, self.x0_pred
        lc = lc.view(-1)
        l0 = ll[-1]
        h = lc - l0
        rks = [(ll[-(i + 1)] - l0) / h for i in range(1, o)]
        rk_t = torch.tensor([float(r) for r in rks] + [1.], dtype=torch.float32)
        hh = -h / 2 if x0 else h / 2
        h_phi_1 = torch.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1
        fact, b_h = 1, torch.expm1(hh)
        R, b = [], []
        for i in range(1, o + 1):
            R.append(torch.pow(rk_t, i - 1))
            b.append(h_phi_k * fact / b_h)
            fact *= (i + 1)
            h_phi_k = h_phi_k / hh - 1 / fact
        R, b = torch.stack(R), torch.cat(b)
        rhos_p = [] if o == 1 else torch.tensor([0.5]) if o == 2 else torch.linalg.solve(R[:-1, :-1], b[:-1])
        rhos_c = [] if not corr else torch.tensor([0.5]) if o == 1 else torch.linalg.solve(R, b)
        f = sig(-lc) if x0 else sig(lc)
        A = sig(lc) / sig(l0) if x0 else sig(-lc) / sig(-l0)
        return dict(order=o, corr=int(corr), l=float(lc), A=float(A), M0=float(f * h_phi_1), PB=float(f * b_h), CB=float(b_h if x0 else f * b_h),
                    rks=[float(r) for r in rks], rhos_p=[float(r) for r in rhos_p], rhos_c=[float(r) for r in rhos_c])

    def _scalars(self, sigmas: Tensor) -> dict:
        """``grid``, ``x0_scale`` (= sigmas[0]) and per update the reference's fp32 scalars as Python floats: the coefficient ``A`` of x, the products
        ``M0`` (in front of the newest model output), ``PB`` / ``CB`` (in front of the predictor's / corrector's history sum), ``rks`` and the
        ``rhos_p`` / ``rhos_c`` it solves for."""
        grid = self._grid(sigmas, self.num_steps)
        steps = [self._update_scalars([grid[j] for j in range(max(0, step - self.order), step)], grid[step], o, corr)
                 for step, (o, corr) in enumerate(self.update_plan(), start=1)]
        return dict(grid=[float(v) for v in grid], x0_scale=float(sigmas.detach().to("cpu", torch.float32)[0]), steps=steps)

    def _program(self, sigmas: Tensor):
        """(ops, x0_scale, result slot): x in slot 0, the predictor's state in slot 1, the history and the corrector's model output in slots 2 .. 5,
        renamed from step to step.  The corrected state is one update over x, the history and the new output: five operands at order 3."""
        sc = self._scalars(sigmas)
        X, P, free, hist = 0, 1, [2, 3, 4, 5], []
        hist.append(free.pop(0))
        ops, n = [self._ev(hist[-1], X, self._row(sc["grid"][0]))], len(sc["steps"])
        for step, r in enumerate(sc["steps"], start=1):
            m = hist[::-1]                                                  # m[0] the newest, m[k + 1] goes with rks[k]
            kk = range(r["order"] - 1)
            pred = [(X, r["A"]), (m[0], -r["M0"] + r["PB"] * sum(r["rhos_p"][k] / r["rks"][k] for k in kk))]
            pred += [(m[k + 1], -r["PB"] * r["rhos_p"][k] / r["rks"][k]) for k in kk]
            if not r["corr"]:
                ops.append(self._lin(X, pred, step == n))
            else:
                rc, cb = r["rhos_c"], r["CB"]
                mt = free.pop(0)
                corr = [(X, r["A"]), (m[0], -r["M0"] + cb * (sum(rc[k] / r["rks"][k] for k in kk) + rc[-1]))]
                corr += [(m[k + 1], -cb * rc[k] / r["rks"][k]) for k in kk] + [(mt, -cb * rc[-1])]
                ops += [self._lin(P, pred), self._ev(mt, P, self._row(r["l"])), self._lin(X, corr, step == n)]
                if step >= self.order and len(hist) == self.order:
                    free.append(hist.pop(0))
                hist.append(mt)
        return ops, sc["x0_scale"], X

    def _compat(self, noise, fn, net, sigmas, kwargs):
        """sampler_vobj.py:670-732 and :551-668 as written; the history sums are plain sums, so any rank of state works."""
        sig, x0 = self._sig, self.x0_pred

        def model(x_, l, **kw):
            v = fn(x_, net=net, sigma=l, inference=True, cond_scale=self.cond_scale, **kw)
            return sig(-l) * x_ - sig(l) * v if x0 else sig(l) * x_ + sig(-l) * v

        def update(x_, ml, ll, lc, o, corr):
            lc = lc.view(-1)
            l0, m0 = ll[-1], ml[-1]
            h = lc - l0
            rks, d1s = [], []
            for i in range(1, o):
                rk = (ll[-(i + 1)] - l0) / h
                rks.append(rk)
                d1s.append((ml[-(i + 1)] - m0) / rk)
            rks = torch.tensor([float(r) for r in rks] + [1.], device=x_.device)
            hh = -h / 2 if x0 else h / 2
            h_phi_1 = torch.expm1(hh)
            h_phi_k, b_h, fact = h_phi_1 / hh - 1, torch.expm1(hh), 1
            R, b = [], []
            for i in range(1, o + 1):
                R.append(torch.pow(rks, i - 1))
                b.append(h_phi_k * fact / b_h)
                fact *= (i + 1)
                h_phi_k = h_phi_k / hh - 1 / fact
            R, b = torch.stack(R), torch.cat(b)
            comb = lambda rho: sum(rho[k] * d for k, d in enumerate(d1s)) if d1s else 0
            rho_p = (torch.tensor([0.5], device=b.device) if o == 2 else torch.linalg.solve(R[:-1, :-1], b[:-1])) if d1s else None
            if corr:
                rho_c = torch.tensor([0.5], device=b.device) if o == 1 else torch.linalg.solve(R, b)
            if x0:
                xt_ = sig(lc) / sig(l0) * x_ - sig(-lc) * h_phi_1 * m0
                x_t, m_t = xt_ - sig(-lc) * b_h * comb(rho_p), None
                if corr:
                    m_t = model(x_t, lc[0])                                 # no keywords (:637)
                    x_t = xt_ - b_h * (comb(rho_c[:-1]) + rho_c[-1] * (m_t - m0))          # no alpha factor (:644)
            else:
                xt_ = sig(-lc) / sig(-l0) * x_ - sig(lc) * h_phi_1 * m0
                x_t, m_t = xt_ - sig(lc) * b_h * comb(rho_p), None
                if corr:
                    m_t = model(x_t, lc[0])
                    x_t = xt_ - sig(lc) * b_h * (comb(rho_c[:-1]) + rho_c[-1] * (m_t - m0))
            return x_t, m_t

        n, order = self.num_steps, self.order
        x = sigmas[0] * noise
        grid = torch.linspace(self.shifted_cosine_transform(sigmas[0]), self.shifted_cosine_transform(sigmas[-1]), n + 1, device=x.device)
        ml, ll = [model(x, grid[0], **kwargs)], [grid[0]]
        for step in range(1, order):
            x, m = update(x, ml, ll, grid[step], step, True)
            ll.append(grid[step])
            ml.append(m)
        for step in range(order, n + 1):
            x, m = update(x, ml, ll, grid[step], min(order, n + 1 - step), step != n)
            for i in range(order - 1):
                ll[i], ml[i] = ll[i + 1], ml[i + 1]
            ll[-1] = grid[step]
            if step < n:
                ml[-1] = m
        return x.clamp(-1.0, 1.0)
