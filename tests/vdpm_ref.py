"""CPU restatement (test infrastructure, not product code) of the reference's two multistep v-objective samplers -- ``sampler_vobj.DPMSampler``
(src/models/components/sampler_vobj.py:196-499) and ``sampler_vobj.UniPCSampler`` (:502-732) -- written independently of audiodiffuser_amd's plugin
classes, so that the device and the plugins are held to something they do not share code with.  tools/gen_golden_vdpm.py pins these functions to the
reference's classes when it writes tests/golden/vdpm_golden.npz.

Every schedule scalar stays an fp32 tensor formed by the reference's own sequence of torch operations, whatever the dtype of the state: with a
float64 state torch promotes ``scalar * state`` to float64, so a float64 run is the reference's loop with the reference's fp32 scalars and a
double-precision state (what a device result is compared with); an fp32 run is the reference's arithmetic itself.  The reference's UniPC cannot run a
float64 state at order >= 2 at all (its fp32 ``rhos`` meet the float64 history in an ``einsum``); here the history sums are plain sums, which also
take any rank of state.

``fn(x, sigma=<0-dim fp32 log-SNR>)`` returns the raw v prediction (tests/vsamp_ref.py ``make_v_fn``).  ``record`` (a list) receives one dict per
``fn`` call: ``logsnr`` and ``used`` (False for the calls whose result the reference discards, :323); with ``dead_calls=False`` those calls are not
made -- they change nothing.  ``rhos`` (a list) receives per UniPC update ``(rhos_p, rhos_c)`` as lists of floats (empty where the reference forms
none)."""
from __future__ import annotations

import math
from typing import Callable, Optional

import torch


def logsnr_of(t: torch.Tensor) -> torch.Tensor:
    """The hard-wired shifted cosine transform of both samplers (:227-233, :540-546): logsnr_min = -15, logsnr_max = 15, shift = 0."""
    t_min = math.atan(math.exp(-0.5 * 15))
    t_max = math.atan(math.exp(-0.5 * -15))
    return -2 * (torch.tan(t_min + t * (t_max - t_min)).log()) + 2 * 0.0


def sigma_of(l: torch.Tensor) -> torch.Tensor:
    return torch.sqrt(torch.sigmoid(-l))


def alpha_of(l: torch.Tensor) -> torch.Tensor:
    return sigma_of(-l)


def singlestep_orders(num_steps: int, order: int):
    """:465-483 -> (orders, K)."""
    if order == 3:
        k = num_steps // 3 + 1
        return ([3] * (k - 2) + [2, 1], k) if num_steps % 3 == 0 else ([3] * (k - 1) + [num_steps % 3], k)
    if order == 2:
        return ([2] * (num_steps // 2), num_steps // 2) if num_steps % 2 == 0 else ([2] * (num_steps // 2) + [1], num_steps // 2 + 1)
    if order == 1:
        return [1] * num_steps, num_steps
    raise ValueError("'order' must be '1' or '2' or '3'.")


class _Model:
    """``model_fn`` of both samplers: the v prediction at log-SNR l turned into the x0 estimate or the noise estimate."""

    def __init__(self, fn: Callable, x0_pred: bool, record: Optional[list]):
        self.fn, self.x0_pred, self.record = fn, x0_pred, record

    def raw(self, x, l, used=True):
        if self.record is not None:
            self.record.append(dict(logsnr=float(l), used=used))
        return self.fn(x, sigma=l)

    def __call__(self, x, l):
        v = self.raw(x, l)
        if self.x0_pred:
            return alpha_of(l) * x - sigma_of(l) * v
        return sigma_of(l) * x + alpha_of(l) * v


# ---- DPMSampler --------------------------------------------------------------------------------------------------------------------------
def _single_1(x, eps, lc, ln, x0_pred):
    h = (ln - lc) / 2
    if x0_pred:
        return sigma_of(ln) / sigma_of(lc) * x - alpha_of(ln) * (-h).expm1() * eps
    return alpha_of(ln) / alpha_of(lc) * x - sigma_of(ln) * h.expm1() * eps


def _single_2(x, eps, lc, ln, model, x0_pred, r1=1 / 2):
    h = ln - lc
    s1 = lc + r1 * h
    h = h / 2
    if x0_pred:
        u1 = sigma_of(s1) / sigma_of(lc) * x - alpha_of(s1) * torch.expm1(-r1 * h) * eps
        eps_r1 = model(u1, s1)
        return (sigma_of(ln) / sigma_of(lc) * x - alpha_of(ln) * torch.expm1(-h) * eps
                - alpha_of(ln) / (2 * r1) * torch.expm1(-h) * (eps_r1 - eps))
    u1 = alpha_of(s1) / alpha_of(lc) * x - sigma_of(s1) * (r1 * h).expm1() * eps
    eps_r1 = model(u1, s1)
    return alpha_of(ln) / alpha_of(lc) * x - sigma_of(ln) * h.expm1() * eps - sigma_of(ln) / (2 * r1) * h.expm1() * (eps_r1 - eps)


def _single_3(x, eps, lc, ln, model, x0_pred, r1=1 / 3, r2=2 / 3):
    h = ln - lc
    s1 = lc + r1 * h
    s2 = lc + r2 * h
    h = h / 2
    if x0_pred:
        u1 = sigma_of(s1) / sigma_of(lc) * x - alpha_of(s1) * (-r1 * h).expm1() * eps
        eps_r1 = model(u1, s1)
        u2 = (sigma_of(s2) / sigma_of(lc) * x - alpha_of(s2) * (-r2 * h).expm1() * eps
              + alpha_of(s2) * (r2 / r1) * ((-r2 * h).expm1() / (r2 * h) + 1) * (eps_r1 - eps))
        eps_r2 = model(u2, s2)
        return (sigma_of(ln) / sigma_of(lc) * x - alpha_of(ln) * torch.expm1(-h) * eps
                + alpha_of(ln) * 1 / r2 * (torch.expm1(-h) / h + 1) * (eps_r2 - eps))
    u1 = alpha_of(s1) / alpha_of(lc) * x - sigma_of(s1) * (r1 * h).expm1() * eps
    eps_r1 = model(u1, s1)
    u2 = (alpha_of(s2) / alpha_of(lc) * x - sigma_of(s2) * (r2 * h).expm1() * eps
          - sigma_of(s2) * (r2 / r1) * ((r2 * h).expm1() / (r2 * h) - 1) * (eps_r1 - eps))
    eps_r2 = model(u2, s2)
    return alpha_of(ln) / alpha_of(lc) * x - sigma_of(ln) * h.expm1() * eps - sigma_of(ln) / r2 * (h.expm1() / h - 1) * (eps_r2 - eps)


def _multi_1(x, m0, lp, lc, x0_pred):
    h = (lc - lp) / 2
    if x0_pred:
        return sigma_of(lc) / sigma_of(lp) * x - alpha_of(lc) * torch.expm1(-h) * m0
    return alpha_of(lc) / alpha_of(lp) * x - sigma_of(lc) * torch.expm1(h) * m0


def _multi_2(x, ms, ls, lc, x0_pred):
    (l1, l0), (m1, m0) = ls[-2:], ms[-2:]
    h = lc - l0
    r0 = (l0 - l1) / h
    d1_0 = (1. / r0) * (m0 - m1)
    h = h / 2
    if x0_pred:
        phi_1 = torch.expm1(-h)
        return sigma_of(lc) / sigma_of(l0) * x - alpha_of(lc) * phi_1 * m0 - alpha_of(lc) * 0.5 * phi_1 * d1_0
    phi_1 = torch.expm1(h)
    return alpha_of(lc) / alpha_of(l0) * x - (sigma_of(lc) * phi_1) * m0 - 0.5 * (sigma_of(lc) * phi_1) * d1_0


def _multi_3(x, ms, ls, lc, x0_pred):
    (l2, l1, l0), (m2, m1, m0) = ls, ms
    h = lc - l0
    r0, r1 = (l0 - l1) / h, (l1 - l2) / h
    h = h / 2
    d1_0 = (1. / r0) * (m0 - m1)
    d1_1 = (1. / r1) * (m1 - m2)
    d1 = d1_0 + (r0 / (r0 + r1)) * (d1_0 - d1_1)
    d2 = (1. / (r0 + r1)) * (d1_0 - d1_1)
    if x0_pred:
        phi_1 = torch.expm1(-h)
        phi_2 = phi_1 / h + 1.
        phi_3 = phi_2 / h - 0.5
        return sigma_of(lc) / sigma_of(l0) * x - alpha_of(lc) * phi_1 * m0 + alpha_of(lc) * phi_2 * d1 - alpha_of(lc) * phi_3 * d2
    phi_1 = torch.expm1(h)
    phi_2 = phi_1 / h - 1.
    phi_3 = phi_2 / h - 0.5
    return alpha_of(lc) / alpha_of(l0) * x - (sigma_of(lc) * phi_1) * m0 - (sigma_of(lc) * phi_2) * d1 - (sigma_of(lc) * phi_3) * d2


def dpm_sampler(noise: torch.Tensor, fn: Callable, sigmas: torch.Tensor, num_steps: int, order: int = 1, multisteps: bool = False,
                x0_pred: bool = True, record: Optional[list] = None, clamp: bool = True, dead_calls: bool = True) -> torch.Tensor:
    """sampler_vobj.py:389-499.  The start state is ``noise`` itself."""
    model = _Model(fn, x0_pred, record)
    x = noise
    l_start, l_end = logsnr_of(sigmas[0]), logsnr_of(sigmas[-1])
    if not multisteps:
        orders, k = singlestep_orders(num_steps, order)
        grid = torch.linspace(l_start, l_end, k + 1)
        for i, o in enumerate(orders):
            lc, ln = grid[i], grid[i + 1]
            eps = model(x, lc)
            x = _single_1(x, eps, lc, ln, x0_pred) if o == 1 else _single_2(x, eps, lc, ln, model, x0_pred) if o == 2 else \
                _single_3(x, eps, lc, ln, model, x0_pred)
        return x.clamp(-1.0, 1.0) if clamp else x
    assert num_steps >= order
    grid = torch.linspace(l_start, l_end, num_steps + 1)
    ms, ls = [model(x, grid[0])], [grid[0]]

    def advance(x, o, lc):
        if o == 1:
            if dead_calls:
                model.raw(x, ls[-1], used=False)             # :323: fn runs, its result is dropped because the model output is handed in
            return _multi_1(x, ms[-1], ls[-1], lc, x0_pred)
        return _multi_2(x, ms, ls, lc, x0_pred) if o == 2 else _multi_3(x, ms, ls, lc, x0_pred)

    for step in range(1, order):
        x = advance(x, step, grid[step])
        ls.append(grid[step])
        ms.append(model(x, grid[step]))
    for step in range(order, num_steps + 1):
        x = advance(x, min(order, num_steps + 1 - step), grid[step])
        ls = ls[1:] + [grid[step]]
        if step < num_steps:
            ms = ms[1:] + [model(x, grid[step])]
    return x.clamp(-1.0, 1.0) if clamp else x


# ---- UniPCSampler ------------------------------------------------------------------------------------------------------------------------
def _unipc_update(x, ms, ls, lc, order, model, x0_pred, corrector, rhos):
    """multistep_uni_pc_update (:551-668), variant bh2, with ``x_t=None`` as ``forward`` always calls it."""
    lc = lc.view(-1)
    l0, m0 = ls[-1], ms[-1]
    h = lc - l0
    rks, d1s = [], []
    for i in range(1, order):
        rk = (ls[-(i + 1)] - l0) / h
        rks.append(rk)
        d1s.append((ms[-(i + 1)] - m0) / rk)
    rks = torch.tensor([float(r) for r in rks] + [1.])
    hh = -h / 2 if x0_pred else h / 2
    h_phi_1 = torch.expm1(hh)
    h_phi_k = h_phi_1 / hh - 1
    factorial_i = 1
    b_h = torch.expm1(hh)
    R, b = [], []
    for i in range(1, order + 1):
        R.append(torch.pow(rks, i - 1))
        b.append(h_phi_k * factorial_i / b_h)
        factorial_i *= (i + 1)
        h_phi_k = h_phi_k / hh - 1 / factorial_i
    R, b = torch.stack(R), torch.cat(b)
    rhos_p = rhos_c = None
    if d1s:
        rhos_p = torch.tensor([0.5]) if order == 2 else torch.linalg.solve(R[:-1, :-1], b[:-1])
    if corrector:
        rhos_c = torch.tensor([0.5]) if order == 1 else torch.linalg.solve(R, b)
    if rhos is not None:
        rhos.append(([float(v) for v in rhos_p] if rhos_p is not None else [], [float(v) for v in rhos_c] if rhos_c is not None else []))
    weighted = lambda rho: sum(rho[k] * d for k, d in enumerate(d1s)) if d1s else 0
    m_t = None
    if x0_pred:
        x_t_ = sigma_of(lc) / sigma_of(l0) * x - alpha_of(lc) * h_phi_1 * m0
        x_t = x_t_ - alpha_of(lc) * b_h * weighted(rhos_p)
        if corrector:
            m_t = model(x_t, lc[0])
            x_t = x_t_ - b_h * (weighted(rhos_c[:-1]) + rhos_c[-1] * (m_t - m0))          # :644: no alpha factor, as the reference has it
    else:
        x_t_ = alpha_of(lc) / alpha_of(l0) * x - sigma_of(lc) * h_phi_1 * m0
        x_t = x_t_ - sigma_of(lc) * b_h * weighted(rhos_p)
        if corrector:
            m_t = model(x_t, lc[0])
            x_t = x_t_ - sigma_of(lc) * b_h * (weighted(rhos_c[:-1]) + rhos_c[-1] * (m_t - m0))
    return x_t, m_t


def unipc_sampler(noise: torch.Tensor, fn: Callable, sigmas: torch.Tensor, num_steps: int, order: int = 2, x0_pred: bool = True,
                  record: Optional[list] = None, rhos: Optional[list] = None, clamp: bool = True) -> torch.Tensor:
    """sampler_vobj.py:670-732.  The start state is ``sigmas[0] * noise``."""
    assert num_steps >= order
    model = _Model(fn, x0_pred, record)
    x = sigmas[0] * noise
    grid = torch.linspace(logsnr_of(sigmas[0]), logsnr_of(sigmas[-1]), num_steps + 1)
    ms, ls = [model(x, grid[0])], [grid[0]]
    for step in range(1, order):
        x, m = _unipc_update(x, ms, ls, grid[step], step, model, x0_pred, True, rhos)
        ls.append(grid[step])
        ms.append(m)
    for step in range(order, num_steps + 1):
        x, m = _unipc_update(x, ms, ls, grid[step], min(order, num_steps + 1 - step), model, x0_pred, step != num_steps, rhos)
        ls = ls[1:] + [grid[step]]
        if step < num_steps:
            ms = ms[1:] + [m]
    return x.clamp(-1.0, 1.0) if clamp else x
