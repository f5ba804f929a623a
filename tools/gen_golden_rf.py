"""Fixture generator (build container only: it imports the reference project on the CPU, as tools/gen_golden_precond.py does) for the
rectified-flow pieces: writes ``tests/golden/rf_golden.npz`` + ``rf_golden.json`` from the REFERENCE's classes (``diffusion.ReFlow``,
``scheduler.RFEDMSchedule`` / ``LinearSchedule``, ``sampler_rf.ReflowEulerSampler``) and pins the CPU restatement ``tests/rf_ref.py`` to them.
Only its output is committed; nothing that runs on the GPU machine imports the reference.

Usage:  python tools/gen_golden_rf.py [--check-only]        (--check-only recomputes everything and compares it with the committed fixture)

What the fixture holds
  * ``sched_linear_<n>`` (LinearSchedule(1, 0, n): the N + 1 entries a run of N steps needs) and ``sched_rfedm_<n>`` (RFEDMSchedule(0.98, 0.02, n): at the
    defaults start = 1 gives inf and end = 0 a division by zero in the EDM samplers, in the reference's own arithmetic);
  * ``rows_rfedm`` / ``rows64_rfedm`` / ``bar_rfedm`` [30, 4] = (c_in, c_noise, c_skip, c_out) = (1 - t, t, 1 - t, -t) with the reference's own
    ``sigma_to_t`` on sched_rfedm_30, in fp32 and on the same sigmas widened to float64, and the per-entry bar max(1e-6, 4 |fp32 - fp64| / |fp64|);
    ``rows_rf`` [30, 4] = (1, s, 0, 1) on the first 30 entries of sched_linear_31;
  * ``den_<mode>_{x, sigma, sigmas, y_scalar, y_batch}`` (mode ``raw`` = ReFlow(), ``edm`` = ReFlow(for_edm=True)): one inference ``denoise_fn`` call
    with a scalar sigma and with [B] sigmas around the reference ``UNet2dBase`` of the ``small`` fixture variant.  With for_edm the reference multiplies
    the [B, C, H, W] input by the [B] vector as it is (it only runs at B = 1 or B = W): those cases are the reference called sample by sample;
  * ``run_noise``, ``run_classes``, ``run_<euler|heun|heun_cfg>_final``: 6 steps of the reference's ReflowEulerSampler over ReFlow() around the reference
    ``UNet2dBase`` of the ``u2d`` net of tests/rf_cases.py -- the ``small`` structure at dim 128, the smallest width the device runs, so the GPU suite can
    repeat the run (final_conv x 0.3, noise x 0.2; ``heun_cfg`` with cond_scale 2);
  * json: constructor signatures, that the reference raises IndexError on a schedule of num_steps entries, how far tests/rf_ref.py around oracle/unet2d.py
    is from each reference result, and for every run of tests/rf_cases.py (the runs tests/test_rf_gpu.py makes on the device) its scales, max |y|, share
    of entries at |y| >= 1 and ``dist_fp32_fp64`` = max |y32 - y64| / max |y64| of the CPU restatement in fp32 and in float64 (the bar of a run is
    max(1e-3, 4 * dist_fp32_fp64)).  The ADM oracle only runs in fp32, so its run has no distance.
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

SIGMA_SCALAR = {"raw": 0.6, "edm": 0.9}                      # raw: the time t itself; edm: sigma, t = sigma / (sigma + 1) = 0.47
SIGMA_BATCH = {"raw": [0.3, 0.8], "edm": [0.5, 3.0]}
ORACLE_PIN = 2.1e-6          # one call: the bar at which oracle/unet2d.py is pinned to the reference's UNet2dBase (tests/test_oracle_unet2d.py)
RUN_PIN = 2e-5               # a 6-step run (11 evaluations with Heun) around the two nets


def signature_of(cls):
    return [[name, None if p.default is inspect.Parameter.empty else p.default]
            for name, p in inspect.signature(cls.__init__).parameters.items() if name != "self"]


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import_reference()
    from src.models.backbones.unet2d import UNet2dBase
    from src.models.components import diffusion as RD, scheduler as RS, sampler_rf as RSM
    from oracle import unet2d as U
    import rf_cases as RC
    import rf_ref as RF

    out, meta = {}, {"signatures": {}}
    for cls in (RD.ReFlow, RS.RFEDMSchedule, RS.LinearSchedule, RSM.ReflowEulerSampler):
        meta["signatures"][cls.__name__] = signature_of(cls)

    # ---- schedules -------------------------------------------------------------------------------------------------------------
    for n in (7, 8, 9, 31, 51):
        out[f"sched_linear_{n}"] = RS.LinearSchedule(start=1.0, end=0.0, num_steps=n)().numpy()
        assert np.array_equal(RF.linear_schedule(1.0, 0.0, n).numpy(), out[f"sched_linear_{n}"])
    for n in (8, 30):
        out[f"sched_rfedm_{n}"] = RS.RFEDMSchedule(start=0.98, end=0.02, num_steps=n)().numpy()
        assert np.array_equal(RF.rfedm_schedule(0.98, 0.02, n).numpy(), out[f"sched_rfedm_{n}"])
    dflt = RS.RFEDMSchedule()()
    meta["rfedm_defaults"] = {"first": float(dflt[0]), "last": float(dflt[-1])}
    assert torch.isinf(dflt[0]) and float(dflt[-1]) == 0.0

    # ---- rows ------------------------------------------------------------------------------------------------------------------
    d_edm, d_raw = RD.ReFlow(for_edm=True), RD.ReFlow()

    def ref_rows(sig):                                                  # :401-402, :383 as written
        t = d_edm.sigma_to_t(sig)
        return torch.stack([1 - t, t, 1 - t, -t], dim=1)

    sig = torch.from_numpy(out["sched_rfedm_30"])
    r32, r64 = ref_rows(sig), ref_rows(sig.double())
    assert r32.dtype == torch.float32 and r64.dtype == torch.float64
    bar = torch.clamp(4 * (r32.double() - r64).abs() / r64.abs().clamp_min(1e-300), min=1e-6)
    out["rows_rfedm"], out["rows64_rfedm"], out["bar_rfedm"] = r32.numpy(), r64.numpy(), bar.numpy()
    meta["max_bar_rfedm"] = float(bar.max())
    assert torch.equal(RF.rows(True, sig), r32) and torch.equal(RF.rows(True, sig, torch.float64), r64)
    lin = torch.from_numpy(out["sched_linear_31"])[:30]
    out["rows_rf"] = torch.stack([torch.ones_like(lin), lin, torch.zeros_like(lin), torch.ones_like(lin)], dim=1).numpy()
    assert np.array_equal(RF.rows(False, lin).numpy(), out["rows_rf"])

    # ---- one denoise_fn call per mode around the reference net ----------------------------------------------------------------------
    cfg, (b, hh, ww) = U.fixture_variants()["small"]
    w = U.generate_weights(cfg, seed=5)
    net = load_into(UNet2dBase(**cfg.to_kwargs()), w)
    classes = (torch.arange(b) * 3 + 1) % cfg.num_classes
    out["den_classes"] = classes.numpy()
    net_o = lambda xi, ti, cond_drop_prob=0.0: U.unet2d_forward(w, cfg, xi, ti, classes=classes, cond_drop_prob=cond_drop_prob)
    meta["denoise"] = {}
    for i, mode in enumerate(("raw", "edm")):
        g = torch.Generator().manual_seed(950 + i)
        sg = torch.tensor(SIGMA_BATCH[mode])
        x = torch.randn(b, cfg.channels, hh, ww, generator=g) * ((1.0 + sg.view(b, 1, 1, 1) ** 2).sqrt() if mode == "edm" else 1.0) * 0.6
        d = d_edm if mode == "edm" else d_raw
        with torch.no_grad():
            if mode == "edm":
                ys = torch.cat([d.denoise_fn(x[j:j + 1], net=net, inference=True, sigma=SIGMA_SCALAR[mode], classes=classes[j:j + 1]) for j in range(b)])
                yb = torch.cat([d.denoise_fn(x[j:j + 1], net=net, inference=True, sigmas=sg[j:j + 1], classes=classes[j:j + 1]) for j in range(b)])
            else:
                ys = d.denoise_fn(x, net=net, inference=True, sigma=SIGMA_SCALAR[mode], classes=classes)
                yb = d.denoise_fn(x, net=net, inference=True, sigmas=sg, classes=classes)
            es = rel(RF.denoise(mode == "edm", net_o, x, sigma=SIGMA_SCALAR[mode]), ys)
            eb = rel(RF.denoise(mode == "edm", net_o, x, sigmas=sg), yb)
        print(mode, es, eb, float(ys.abs().max()), float(yb.abs().max()))
        assert es <= ORACLE_PIN and eb <= ORACLE_PIN, (mode, es, eb)
        assert float(ys.abs().max()) > 1.0 and float(yb.abs().max()) > 1.0          # neither mode clips: the cases must show it
        meta["denoise"][mode] = {"rf_ref_rel_err_scalar": es, "rf_ref_rel_err_batch": eb, "max_abs_scalar": float(ys.abs().max()),
                                 "max_abs_batch": float(yb.abs().max())}
        out[f"den_{mode}_x"], out[f"den_{mode}_sigmas"], out[f"den_{mode}_sigma"] = x.numpy(), sg.numpy(), np.float32(SIGMA_SCALAR[mode])
        out[f"den_{mode}_y_scalar"], out[f"den_{mode}_y_batch"] = ys.numpy(), yb.numpy()

    # ---- short runs of the reference's sampler ------------------------------------------------------------------------------------------
    cfg_r, w_r = RC.weights("u2d", 0.3)
    net_r = load_into(UNet2dBase(**cfg_r.to_kwargs()), w_r)
    cl_r = RC.labels("u2d")
    net_ro = RC.oracle_net("u2d", cfg_r, w_r)
    noise = torch.randn(2, 2, 32, 16, generator=torch.Generator().manual_seed(41)) * 0.2
    sig7 = torch.from_numpy(out["sched_linear_7"])
    out["run_noise"], out["run_classes"] = noise.numpy(), cl_r.numpy()
    meta["reference_runs"] = {"final_conv_scale": 0.3, "noise_scale": 0.2, "steps": 6}
    for tag, heun, cs in (("euler", False, 1.0), ("heun", True, 1.0), ("heun_cfg", True, 2.0)):
        smp = RSM.ReflowEulerSampler(num_steps=6, cond_scale=cs, use_heun=heun)
        with torch.no_grad():
            y = smp(noise, fn=d_raw.denoise_fn, net=net_r, sigmas=sig7, classes=cl_r)
            mine = RF.euler_sampler(noise, RF.make_fn(False, net_ro, cs), sig7, 6, use_heun=heun)
        e, share, top = rel(mine, y), float((y.abs() >= 1).float().mean()), float(y.abs().max())
        print("reference run", tag, e, share, top)
        assert e <= RUN_PIN and share <= 0.01 and top > 0.05, (tag, e, share, top)
        out[f"run_{tag}_final"] = y.numpy()
        meta["reference_runs"][tag] = {"rf_ref_rel_err": e, "share_abs_ge_1": share, "max_abs": top}
    try:
        RSM.ReflowEulerSampler(num_steps=6, use_heun=False)(noise, fn=d_raw.denoise_fn, net=net_r, sigmas=sig7[:6], classes=cl_r)
        raised = False
    except IndexError:
        raised = True
    assert raised
    meta["reference_raises_index_error_on_num_steps_sigmas"] = raised

    # ---- the runs of tests/rf_cases.py: conditioning and saturation of each, on the CPU ------------------------------------------------------
    meta["runs"] = {}
    for name in RC.RUNS:
        sp = RC.spec(name)
        dt = RC.ref_dtype(sp["net"])
        y = RC.reference(name, dt).double()
        rec = {"net": sp["net"], "loop": sp["loop"], "steps": sp["steps"], "out_scale": sp["out_scale"], "noise_scale": sp["noise_scale"],
               "max_abs": round(float(y.abs().max()), 6), "share_abs_ge_1": float((y.abs() >= 1).double().mean()),
               "dist_fp32_fp64": None if dt == torch.float32 else float(f"{rel(RC.reference(name, torch.float32), y):.4e}")}
        print(name, rec)
        assert bool(torch.isfinite(y).all()) and rec["max_abs"] > 0.05, name
        if name == "tiny_clamp":
            assert 0.25 <= rec["share_abs_ge_1"] <= 0.75, rec              # many entries saturate, many do not
        else:
            assert rec["share_abs_ge_1"] <= 0.01, (name, rec)
        assert rec["dist_fp32_fp64"] is None or rec["dist_fp32_fp64"] < 2.5e-4, (name, rec)      # well conditioned: the bar of every run is the project's 1e-3
        meta["runs"][name] = rec

    if args.check_only:
        have = np.load(os.path.join(GOLD, "rf_golden.npz"))
        assert sorted(have.files) == sorted(out), (sorted(have.files), sorted(out))
        for k, v in out.items():
            assert np.array_equal(have[k], v), ("the committed fixture differs", k)
        with open(os.path.join(GOLD, "rf_golden.json")) as f:
            have_meta = json.load(f)
        assert have_meta["signatures"] == json.loads(json.dumps(meta["signatures"]))
        assert {k: (r["out_scale"], r["noise_scale"], r["steps"]) for k, r in have_meta["runs"].items()} == \
               {k: (r["out_scale"], r["noise_scale"], r["steps"]) for k, r in meta["runs"].items()}
        print("rf_golden.npz reproduced:", len(out), "arrays equal")
        return
    np.savez_compressed(os.path.join(GOLD, "rf_golden.npz"), **out)
    with open(os.path.join(GOLD, "rf_golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote rf_golden.npz", sum(v.nbytes for v in out.values()) // 1024, "KiB")


if __name__ == "__main__":
    main()
