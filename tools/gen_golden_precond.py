"""Fixture generator (build container only: it imports the reference project on the CPU, as oracle/gen_golden_unet2d.py does) for the VE / VP /
v preconditioning: writes ``tests/golden/precond_golden.npz`` + ``precond_golden.json`` from the REFERENCE's classes and pins the CPU
restatement ``tests/precond_ref.py`` to them.  Only its output is committed; nothing that runs on the GPU machine imports the reference.

Usage:  python tools/gen_golden_precond.py [--check-only]

What the fixture holds
  * ``sched_<name>_<n>``: LinearSchedule / GeometricSchedule / VPSchedule / VESchedule / VSchedule at the shipped arguments, n = 30 and 50;
  * ``rows_<kind>_<sched>`` [30, 4] = (c_in, c_noise, c_skip, c_out): ``get_scale_weights`` of EluDiffusion(0.2) on the Karras schedule, of
    VEDiffusion / VPDiffusion and the v row (VDiffusion.denoise_fn(for_edm=True) :310-313 with the reference's own ``sigma_to_logsnr``) on each of
    the ve / vp / v schedules; ``rows64_*`` the same classes fed the same sigmas widened to float64; ``bar_*`` = max(1e-6, 4 |fp32 - fp64| / |fp64|)
    per entry -- where the reference's fp32 expression is itself ill-conditioned (ln(1 + sigma^2) at small sigma) a second correct fp32
    evaluation may differ by that much and no more;
  * ``den_<kind>_{x, sigmas, y_scalar, y_batch}``: one inference ``denoise_fn`` call per kind with a scalar sigma and with [B] sigmas around the
    reference ``UNet2dBase`` of the ``small`` fixture variant.  VDiffusion multiplies the [B, C, H, W] input by the [B] vector as it is (it broadcasts
    against the last axis, so the reference only runs at B = 1 or B = W): both of its cases are the reference called sample by sample.
  * json: constructor parameter names and defaults of every class (``inspect.signature``).
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference, GOLD          # noqa: E402
from oracle.gen_golden_next import load_into                  # noqa: E402

# Sigmas at which at most half of the reference's result is clipped and the network's time input stays moderate: oracle/unet2d.py is pinned to the
# reference's UNet2dBase at times in [-0.9, 0.4]; at VPDiffusion's c_noise = 218 (sigma 0.8) the two nets already differ by 6.6e-5 with this fixture's
# random weights (measured with this script's inputs), which says nothing about the preconditioning.
SIGMA_SCALAR = {"edm": 0.7, "ve": 0.3, "vp": 0.05, "v": 0.9}
SIGMA_BATCH = {"edm": [0.3, 2.0], "ve": [0.1, 0.5], "vp": [0.03, 0.1], "v": [0.5, 3.0]}


def signature_of(cls):
    out = []
    for name, p in inspect.signature(cls.__init__).parameters.items():
        if name == "self":
            continue
        out.append([name, None if p.default is inspect.Parameter.empty else p.default])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import_reference()
    from src.models.backbones.unet2d import UNet2dBase
    from src.models.components import diffusion as RD, scheduler as RS
    from oracle import unet2d as U
    import precond_ref as PR

    out, meta = {}, {"signatures": {}, "max_bar": {}}
    for cls in (RD.VEDiffusion, RD.VPDiffusion, RD.VDiffusion, RD.EluDiffusion, RS.KarrasSchedule, RS.LinearSchedule, RS.GeometricSchedule,
                RS.VPSchedule, RS.VESchedule, RS.VSchedule):
        meta["signatures"][cls.__name__] = signature_of(cls)

    # ---- schedules -------------------------------------------------------------------------------------------------------------
    for n in (30, 50):
        sch = {"linear": RS.LinearSchedule(start=1.0, end=0.0, num_steps=n), "geometric": RS.GeometricSchedule(num_steps=n),
               "vp": RS.VPSchedule(beta_d=19.9, beta_min=0.1, end=0.001, num_steps=n), "ve": RS.VESchedule(sigma_max=100, sigma_min=0.02, num_steps=n),
               "v": RS.VSchedule(num_steps=n), "karras": RS.KarrasSchedule(0.002, 80.0, 7.0, n)}
        for k, m in sch.items():
            out[f"sched_{k}_{n}"] = m().numpy()
        for k, mine in (("linear", PR.linear_schedule(num_steps=n)), ("geometric", PR.geometric_schedule(num_steps=n)), ("vp", PR.shipped_schedule("vp", n)),
                        ("ve", PR.shipped_schedule("ve", n)), ("v", PR.shipped_schedule("v", n)), ("karras", PR.shipped_schedule("edm", n))):
            assert np.array_equal(mine.numpy(), out[f"sched_{k}_{n}"]), ("precond_ref schedule differs from the reference", k, n)

    # ---- rows ------------------------------------------------------------------------------------------------------------------
    diffs = {"edm": RD.EluDiffusion(sigma_data=0.2), "ve": RD.VEDiffusion(), "vp": RD.VPDiffusion(beta_min=0.1, beta_d=19.9, M=1000),
             "v": RD.VDiffusion(for_edm=True)}

    def ref_rows(kind, sig):
        d = diffs[kind]
        if kind == "v":                                                 # :310-313 as written, v_to_x0 :290 folded into the row
            sigmat = torch.sqrt(torch.sigmoid(-d.sigma_to_logsnr(sig)))
            alphat = torch.sqrt(torch.sigmoid(d.sigma_to_logsnr(sig)))
            return torch.stack([alphat, d.sigma_to_logsnr(sig), alphat * alphat, -sigmat], dim=1)
        c_skip, c_out, c_in, c_noise = d.get_scale_weights(sig, 1)
        full = lambda v: v if torch.is_tensor(v) else torch.full_like(sig, float(v))
        return torch.stack([full(c_in), c_noise, full(c_skip), full(c_out)], dim=1)

    for kind in PR.KINDS:
        for sname in (("karras",) if kind == "edm" else ("ve", "vp", "v")):
            sig = torch.from_numpy(out[f"sched_{sname}_30"])
            r32, r64 = ref_rows(kind, sig), ref_rows(kind, sig.double())
            assert r32.dtype == torch.float32 and r64.dtype == torch.float64
            bar = torch.clamp(4 * (r32.double() - r64).abs() / r64.abs().clamp_min(1e-300), min=1e-6)
            bar[r64 == 0] = 1e-6
            out[f"rows_{kind}_{sname}"], out[f"rows64_{kind}_{sname}"], out[f"bar_{kind}_{sname}"] = r32.numpy(), r64.numpy(), bar.numpy()
            meta["max_bar"][f"{kind}_{sname}"] = float(bar.max())
            assert torch.equal(PR.rows(kind, sig), r32), ("precond_ref rows differ from the reference", kind, sname)
            assert torch.equal(PR.rows(kind, sig, torch.float64), r64), (kind, sname)

    # ---- one denoise_fn call per kind around the reference net ----------------------------------------------------------------------
    cfg, (b, hh, ww) = U.fixture_variants()["small"]
    w = U.generate_weights(cfg, seed=5)
    net = load_into(UNet2dBase(**cfg.to_kwargs()), w)
    classes = (torch.arange(b) * 3 + 1) % cfg.num_classes
    out["den_classes"] = classes.numpy()
    net_o = lambda xi, ti, cond_drop_prob=0.0: U.unet2d_forward(w, cfg, xi, ti, classes=classes, cond_drop_prob=cond_drop_prob)
    meta["denoise"] = {}
    for i, kind in enumerate(PR.KINDS):
        g = torch.Generator().manual_seed(900 + i)
        sg = torch.tensor(SIGMA_BATCH[kind])
        x = torch.randn(b, cfg.channels, hh, ww, generator=g) * (1.0 + sg.view(b, 1, 1, 1) ** 2).sqrt() * 0.4
        d = diffs[kind]
        with torch.no_grad():
            if kind == "v":
                ys = torch.cat([d.denoise_fn(x[j:j + 1], net=net, inference=True, sigma=SIGMA_SCALAR[kind], classes=classes[j:j + 1]) for j in range(b)])
                yb = torch.cat([d.denoise_fn(x[j:j + 1], net=net, inference=True, sigmas=sg[j:j + 1], classes=classes[j:j + 1]) for j in range(b)])
            else:
                ys = d.denoise_fn(x, net=net, inference=True, sigma=SIGMA_SCALAR[kind], classes=classes)
                yb = d.denoise_fn(x, net=net, inference=True, sigmas=sg, classes=classes)
            es = float((PR.denoise(kind, net_o, x, sigma=SIGMA_SCALAR[kind]) - ys).abs().max() / ys.abs().max())
            eb = float((PR.denoise(kind, net_o, x, sigmas=sg) - yb).abs().max() / yb.abs().max())
        clipped = float((ys.abs() >= 1).float().mean())
        print(kind, es, eb, clipped)
        assert clipped <= 0.5
        assert es <= 2.1e-6 and eb <= 2.1e-6, (kind, es, eb)
        assert float(ys.abs().max()) > 0.05
        meta["denoise"][kind] = {"precond_ref_rel_err_scalar": es, "precond_ref_rel_err_batch": eb, "share_clipped_scalar": clipped,
                                 "max_abs_scalar": float(ys.abs().max()), "max_abs_batch": float(yb.abs().max())}
        out[f"den_{kind}_x"], out[f"den_{kind}_sigmas"] = x.numpy(), sg.numpy()
        out[f"den_{kind}_sigma"] = np.float32(SIGMA_SCALAR[kind])
        out[f"den_{kind}_y_scalar"], out[f"den_{kind}_y_batch"] = ys.numpy(), yb.numpy()
    print(json.dumps(meta, indent=1))
    if args.check_only:
        return
    np.savez_compressed(os.path.join(GOLD, "precond_golden.npz"), **out)
    with open(os.path.join(GOLD, "precond_golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote precond_golden.npz", sum(v.nbytes for v in out.values()) // 1024, "KiB")


if __name__ == "__main__":
    main()
