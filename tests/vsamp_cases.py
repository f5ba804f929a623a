"""The runs of the four table-driven samplers (VESampler, VPSampler, VSampler, VEulerSampler) that tools/gen_golden_vsamp.py measures on the CPU
and tests/test_vsamp_gpu.py runs on the device (test infrastructure, not product code): one table, so the recorded ``dist_fp32_fp64`` of a run belongs
to exactly the inputs the GPU test uses.

A run is the CPU restatement tests/vsamp_ref.py (the denoiser of the VE / VP runs: tests/precond_ref.py) around one of the oracle nets of
tests/rf_cases.py with deterministic random weights, at the smallest shape the net takes: the 1-D U-Net at its total down-sampling factor (L = 64),
the ``small`` UNet2dBase structure at [2, 2, 32, 16], the ADM net at [3, 1, 32, 32], the WaveNet at an odd T (3 x 501 elements: the scalar tail of
the update kernel).  ``out_scale`` multiplies the net's output layer, ``noise_scale`` the unit noise and the injected draws: chosen (and checked by
the generator) so that the float64 result has max |y| > 0.05, at most 1 % of its entries at the final clamp, at most 50 % of any clamped
per-evaluation estimate at +-1, and fp32 and float64 end less than 2.5e-4 apart -- a clamp hides every difference in a saturated entry.  The VP
runs end unclamped and are scaled so that the result leaves [-1, 1].

Every VE / VP schedule has steps inside the churn window (gamma > 0) and outside it (gamma = 0), and every run ends with a step into t_next = 0."""
from __future__ import annotations

from collections import OrderedDict

import torch

import precond_ref as PR
import rf_cases as RC
import vsamp_ref as VR

SHAPES = {"tiny": (3, 1, 64), "tiny1": (1, 1, 64), "tiny_cc": (3, 1, 64), "u2d": (2, 2, 32, 16), "adm": (3, 1, 32, 32), "wn": (3, 1, 501)}
NET_OF = {"tiny1": "tiny"}                                   # shape name -> net of tests/rf_cases.py where they differ

DEFAULTS = dict(heun=True, cond_scale=1.0, out_scale=0.2, noise_scale=0.1, noise_seed=70, steps=5, shift=None)
RUNS = OrderedDict([
    # VESampler over VEDiffusion: sigmas 3 .. 0.05 geometric, churn window [0.2, 2]
    ("ve_tiny1_heun", dict(shape="tiny1", sampler="ve", out_scale=0.05)),
    ("ve_tiny_euler", dict(shape="tiny", sampler="ve", heun=False, out_scale=0.05)),
    ("ve_u2d_heun", dict(shape="u2d", sampler="ve", out_scale=0.05, steps=4)),
    ("ve_wn_heun", dict(shape="wn", sampler="ve", out_scale=0.5)),
    # VPSampler over VPDiffusion(0.1, 19.9, 1000): the same sigma list, window [0.04, 2]
    ("vp_tiny_heun", dict(shape="tiny", sampler="vp", out_scale=0.002, noise_scale=0.3)),
    ("vp_tiny1_euler", dict(shape="tiny1", sampler="vp", heun=False, out_scale=0.002, noise_scale=0.3)),
    ("vp_adm_heun", dict(shape="adm", sampler="vp", out_scale=0.02, noise_scale=0.3, steps=4)),
    # VSampler over VDiffusion(): times 0.9 .. 0.15, then 0
    ("v_tiny_shift0", dict(shape="tiny", sampler="v", shift=0.0, noise_scale=0.3)),
    ("v_u2d_shift", dict(shape="u2d", sampler="v", shift=0.25, noise_scale=0.3, steps=4)),
    ("v_tiny_cc_guided", dict(shape="tiny_cc", sampler="v", shift=0.0, cond_scale=3.0, noise_scale=0.25, out_scale=0.1)),
    # VEulerSampler
    ("veuler_tiny1_euler", dict(shape="tiny1", sampler="veuler", heun=False, shift=0.5, noise_scale=0.2)),
    ("veuler_tiny_heun", dict(shape="tiny", sampler="veuler", shift=0.5, noise_scale=0.2)),
    ("veuler_u2d_heun", dict(shape="u2d", sampler="veuler", shift=0.25, noise_scale=0.2, steps=4)),
    ("veuler_wn_heun", dict(shape="wn", sampler="veuler", shift=0.5, noise_scale=0.2, out_scale=2.0)),
])
# gamma = min(s_churn / steps, sqrt(2) - 1) inside [lo, hi].  VE: the first step (sigma 3) and the last (0.05) have gamma = 0.  VP: only the first has;
# the churn of the last steps, at s_noise 3, is what carries the unclamped result beyond +-1 (without it the state has contracted onto the clamped estimate)
CHURN = {"ve": dict(lo=0.2, hi=2.0, s_churn=1.0, s_noise=1.0), "vp": dict(lo=0.04, hi=2.0, s_churn=10.0, s_noise=3.0)}
VP_ARGS = PR.VP_ARGS


# ---- host cases: tables and toy runs (tests/test_vsamp_host.py; recorded from the reference's classes by tools/gen_golden_vsamp.py) -----------
_geo = lambda hi, lo, n: hi * (lo / hi) ** (torch.arange(n, dtype=torch.float32) / (n - 1))
# name -> (sampler, constructor keywords, schedule).  The *_window cases have gamma > 0 inside [0.2, 2] and gamma = 0 outside; *_nochurn has
# gamma = 0 on every step (the noise coefficient of such a step is the rounding of sigma_to_t(t_to_sigma(t)), recorded from the reference).
TABLES = OrderedDict([
    ("ve_window", ("ve", dict(s_tmin=0.2, s_tmax=2.0, s_churn=2.0, s_noise=1.003, num_steps=7), _geo(10.0, 0.02, 7))),
    ("ve_nochurn_euler", ("ve", dict(s_churn=0.0, num_steps=9, use_heun=False), _geo(80.0, 0.002, 9))),
    ("ve_shipped", ("ve", dict(s_churn=200, s_noise=1, num_steps=8), PR.ve_schedule(100, 0.02, 8))),
    ("vp_window", ("vp", dict(s_min=0.2, s_max=2.0, s_churn=2.0, s_noise=1.003, num_steps=7), _geo(10.0, 0.02, 7))),
    ("vp_nochurn_euler", ("vp", dict(s_churn=0.0, num_steps=9, use_heun=False), PR.vp_schedule(num_steps=9))),
    # 50 steps of the shipped VP schedule without churn: step 39 is one whose round trip does not close (a1 = 1.96e-4 at sigma 0.74)
    ("vp_nochurn_50", ("vp", dict(s_churn=0.0, num_steps=50, use_heun=False), PR.vp_schedule(num_steps=50))),
    ("vp_shipped", ("vp", dict(beta_d=19.9, beta_min=0.1, s_churn=200.0, num_steps=8), PR.vp_schedule(num_steps=8))),
    ("v_shift0", ("v", dict(shift=0.0, num_steps=8), torch.linspace(1.0, 0.05, 8))),
    ("v_shift", ("v", dict(logsnr_min=-12, logsnr_max=14, shift=0.3, num_steps=6), torch.linspace(0.97, 0.1, 6))),
    ("veuler_default", ("veuler", dict(num_steps=8), torch.linspace(1.0, 0.05, 8))),
    ("veuler_heun", ("veuler", dict(shift=0.25, use_heun=True, num_steps=6), torch.linspace(0.97, 0.1, 6))),
])
TOY_SHAPE, TOY_SEED = (2, 1, 16), 11


def toy_fn(x, sigma, **_):
    """A smooth stand-in denoiser for the host runs: an estimate inside (-1, 1) for the x0 samplers, a v of moderate size for the other two."""
    return torch.tanh(0.8 * x / (1 + sigma.abs()).sqrt())


def toy_noise() -> torch.Tensor:
    return torch.randn(*TOY_SHAPE, generator=torch.Generator().manual_seed(TOY_SEED)) * 0.7


def spec(name: str) -> dict:
    sp = {**DEFAULTS, **RUNS[name], "name": name}
    sp["net"] = NET_OF.get(sp["shape"], sp["shape"])
    return sp


def ref_dtype(sp: dict):
    return RC.ref_dtype(sp["net"])


def noise_of(sp: dict) -> torch.Tensor:
    shape = SHAPES[sp["shape"]]
    n = int(torch.tensor(shape[2:]).prod())
    return RC.generate_noise(sp["noise_seed"], shape[0], n, channels=shape[1]).reshape(shape) * sp["noise_scale"]


def draws_of(sp: dict) -> torch.Tensor:
    """[steps, *shape] draws at ``noise_scale`` (the samplers apply their own coefficients on top): one per step; VSampler reads the first
    steps - 1, VEulerSampler none."""
    shape = SHAPES[sp["shape"]]
    n = int(torch.tensor(shape[2:]).prod())
    return torch.stack([RC.generate_noise(sp["noise_seed"] + 100 * (i + 1), shape[0], n, channels=shape[1]).reshape(shape) for i in range(sp["steps"])]) * sp["noise_scale"]


def sigmas_of(sp: dict) -> torch.Tensor:
    n = sp["steps"]
    if sp["sampler"] in ("ve", "vp"):
        return 3.0 * (0.05 / 3.0) ** (torch.arange(n, dtype=torch.float32) / (n - 1))
    return torch.linspace(0.9, 0.15, n)


def sampler_kwargs(sp: dict) -> dict:
    """The constructor keywords of the plugin class (and of the reference class) of this run, without ``use_graph``."""
    kw = dict(num_steps=sp["steps"], cond_scale=sp["cond_scale"])
    ch = CHURN.get(sp["sampler"])
    if sp["sampler"] == "ve":
        kw.update(s_tmin=ch["lo"], s_tmax=ch["hi"], s_churn=ch["s_churn"], s_noise=ch["s_noise"], use_heun=sp["heun"])
    elif sp["sampler"] == "vp":
        kw.update(s_min=ch["lo"], s_max=ch["hi"], s_churn=ch["s_churn"], s_noise=ch["s_noise"], use_heun=sp["heun"],
                  beta_d=VP_ARGS["beta_d"], beta_min=VP_ARGS["beta_min"])
    elif sp["sampler"] == "v":
        kw.update(shift=sp["shift"])
    else:
        kw.update(shift=sp["shift"], use_heun=sp["heun"])
    return kw


def reference(name: str, dtype=torch.float64, clamp: bool = True, info: dict = None) -> torch.Tensor:
    """The CPU result of run ``name`` with the state in ``dtype``.  ``info`` (a dict) receives ``clamped_share``: the largest share of entries at
    +-1 over the run's clamped per-evaluation estimates (0 for VEulerSampler, whose evaluations are the raw v)."""
    sp = spec(name)
    cfg, w = RC.weights(sp["net"], sp["out_scale"])
    net = RC.oracle_net(sp["net"], cfg, w, dtype)
    noise, draws, sig, n = noise_of(sp).to(dtype), draws_of(sp), sigmas_of(sp), sp["steps"]
    shares, rec, ch = [0.0], [], CHURN.get(sp["sampler"])
    with torch.no_grad():
        if sp["sampler"] in ("ve", "vp"):
            inner = PR.make_fn(sp["sampler"], net, sp["cond_scale"])

            def fn(x, sigma):
                d = inner(x, sigma=sigma)
                shares.append(float((d.abs() >= 1).double().mean()))
                return d
            if sp["sampler"] == "ve":
                y = VR.ve_sampler(noise, fn, sig, n, ch["lo"], ch["hi"], ch["s_churn"], ch["s_noise"], sp["heun"], draws, clamp=clamp)
            else:
                y = VR.vp_sampler(noise, fn, sig, n, VP_ARGS["beta_d"], VP_ARGS["beta_min"], ch["s_churn"], ch["s_noise"], ch["lo"], ch["hi"],
                                  sp["heun"], draws)
        elif sp["sampler"] == "v":
            y = VR.v_sampler(noise, VR.make_v_fn(net, sp["cond_scale"]), sig, n, shift=sp["shift"], draws=draws, record=rec, clamp=clamp)
            shares += [r["share_clamped"] for r in rec]
        else:
            y = VR.veuler_sampler(noise, VR.make_v_fn(net, sp["cond_scale"]), sig, n, shift=sp["shift"], use_heun=sp["heun"], clamp=clamp)
    if info is not None:
        info["clamped_share"] = max(shares)
    return y
