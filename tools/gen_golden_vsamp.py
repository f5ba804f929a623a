"""Fixture generator (build container only: it imports the reference project on the CPU, as tools/gen_golden_rf.py does) for the four table-driven
samplers: writes ``tests/golden/vsamp_golden.npz`` + ``vsamp_golden.json`` from the REFERENCE's classes (``sampler_edm.VESampler`` / ``VPSampler``,
``sampler_vobj.VSampler`` / ``VEulerSampler``) and pins the CPU restatement ``tests/vsamp_ref.py`` to them.  Only its output is committed; nothing that
runs on the GPU machine imports the reference.

Usage:  python tools/gen_golden_vsamp.py [--check-only]        (--check-only recomputes everything and compares it with the committed fixture)

What the fixture holds
  * per table case of tests/vsamp_cases.py (``TABLES``): ``<case>_sigmas`` and the fp32 scalars the reference itself formed, one row per step, read
    off its own execution -- ``step`` is called with a probe ``fn`` that records the ``sigma`` it is handed (VE / VP: sigma(t_hat) and, under Heun,
    sigma(t_prime); V / VEuler: logsnr_t and logsnr_s) and with ``randn_like`` replaced so that the state it hands ``fn`` (or returns) IS a
    coefficient: x = 0, eps = 1 gives the noise coefficient ``a1`` (V: the posterior standard deviation ``std``), x = 1, eps = 0 gives ``a0``:
        ``<case>_sigma`` [n, 2] (NaN where the step has no second evaluation), ``<case>_a`` [n, 2] = (a0, a1) (VE / VP), ``<case>_std`` [n] (V);
  * per toy run (every table case on ``toy_fn``): ``toy_<case>_draws`` (the ``randn_like`` draws of the reference run, re-drawn from the same seed),
    ``toy_<case>_out`` (what the reference returned) and ``toy_<case>_next`` (four normals drawn after the run: the state it leaves the global generator in);
  * json: constructor signatures, how far tests/vsamp_ref.py is from each toy run, and for every run of tests/vsamp_cases.py (``RUNS``, what
    tests/test_vsamp_gpu.py runs on the device) its scales, max |y|, share of entries at the final clamp, the largest share of a clamped
    per-evaluation estimate at +-1 and ``dist_fp32_fp64`` = max |y32 - y64| / max |y64| of the CPU restatement (the bar of a run is
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

TOY_PIN = 1e-6            # tests/vsamp_ref.py against a reference toy run: the same fp32 operations in the same order (measured: equal)


def signature_of(cls):
    return [[name, None if p.default is inspect.Parameter.empty else p.default]
            for name, p in inspect.signature(cls.__init__).parameters.items() if name != "self"]


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


class FixedNormal:
    """``torch.randn_like`` replaced by a constant for the duration of a probe."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.real = torch.randn_like
        torch.randn_like = lambda x: torch.full_like(x, self.value)

    def __exit__(self, *exc):
        torch.randn_like = self.real


def probe_churn(smp, sigmas, vp: bool):
    """The reference's own forward-loop preamble (sampler_edm.py:105-112, :207-215), then ``step`` per step with probes."""
    ts = smp.sigma_to_t(sigmas)
    ts = torch.cat([ts, torch.zeros_like(ts[:1])])
    lo, hi = (smp.s_min, smp.s_max) if vp else (smp.s_tmin, smp.s_tmax)
    gammas = torch.where((sigmas >= lo) & (sigmas <= hi), min(smp.s_churn / smp.num_steps, 2 ** 0.5 - 1), 0.0)
    sig, a = [], []
    for i in range(smp.num_steps):
        seen_sigma, seen_x = [], []

        def fn(x, net=None, sigma=None, **kw):
            seen_sigma.append(float(sigma)); seen_x.append(x.clone())
            return torch.zeros_like(x)
        with FixedNormal(1.0):
            smp.step(torch.zeros(1), fn=fn, net=None, t=ts[i], t_next=ts[i + 1], gamma=gammas[i])
        # x = 0, eps = 1: the state of the first evaluation is 0 + a1 * 1.  VE hands it to fn as it is: the recorded a1 IS what the reference formed.
        # VP hands fn x_hat / scale(t_hat), which cannot be undone exactly: a1 is formed by the reference's own methods in its own order (:176) and the
        # division repeated, which must reproduce what fn saw bit for bit.  The same with x = 1, eps = 0 for a0.
        t_hat = smp.sigma_to_t(smp.t_to_sigma(ts[i]) + gammas[i] * smp.t_to_sigma(ts[i]))
        nc = (smp.t_to_sigma(t_hat) ** 2 - smp.t_to_sigma(ts[i]) ** 2).clip(min=0).sqrt()
        if not vp:
            a0, a1 = 1.0, float(seen_x[0])
            assert a1 == float(nc * smp.s_noise), (i, a1, float(nc * smp.s_noise))
        else:
            a0_t, a1_t = smp.scale(t_hat) / smp.scale(ts[i]), nc * smp.scale(t_hat) * smp.s_noise
            assert float(seen_x[0]) == float((a0_t * torch.zeros(1) + a1_t * torch.ones(1)) / smp.scale(t_hat)), (i, float(seen_x[0]), float(a1_t))
            first = []
            with FixedNormal(0.0):
                smp.step(torch.ones(1), fn=lambda x, net=None, sigma=None, **kw: first.append(x.clone()) or torch.zeros_like(x), net=None,
                         t=ts[i], t_next=ts[i + 1], gamma=gammas[i])
            assert float(first[0]) == float((a0_t * torch.ones(1) + a1_t * torch.zeros(1)) / smp.scale(t_hat)), (i, float(first[0]), float(a0_t))
            a0, a1 = float(a0_t), float(a1_t)
        sig.append([seen_sigma[0], seen_sigma[1] if len(seen_sigma) > 1 else float("nan")])
        a.append([a0, a1])
    return np.array(sig, np.float32), np.array(a, np.float32)


def probe_vobj(smp, ts_in, stochastic: bool):
    ts = torch.cat([ts_in, torch.zeros_like(ts_in[:1])])
    sig, std = [], []
    for i in range(smp.num_steps):
        seen = []

        def fn(x, net=None, sigma=None, **kw):
            seen.append(float(sigma))
            return torch.zeros_like(x)
        with FixedNormal(1.0):
            y = smp.step(torch.zeros(1), fn=fn, net=None, t=ts[i], t_next=ts[i + 1])
        second = len(seen) > 1
        sig.append([seen[0], seen[1] if second else float("nan")])
        std.append(float(y) if stochastic else 0.0)         # x = 0, v = 0: mu = 0 and the step returns 1 * sqrt(variance) (0 into t_next = 0)
    return np.array(sig, np.float32), np.array(std, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import_reference()
    from src.models.components import sampler_edm as RSE, sampler_vobj as RSV
    import vsamp_cases as VC
    import vsamp_ref as VR

    ref_cls = {"ve": RSE.VESampler, "vp": RSE.VPSampler, "v": RSV.VSampler, "veuler": RSV.VEulerSampler}
    out, meta = {}, {"signatures": {c.__name__: signature_of(c) for c in ref_cls.values()}, "toy": {}, "runs": {}}

    # ---- tables: the reference's own fp32 scalars, and its runs on the toy fn ---------------------------------------------------------
    for case, (kind, kw, sigmas) in VC.TABLES.items():
        smp = ref_cls[kind](**kw)
        out[f"{case}_sigmas"] = sigmas.numpy()
        if kind in ("ve", "vp"):
            out[f"{case}_sigma"], out[f"{case}_a"] = probe_churn(smp, sigmas, kind == "vp")
        else:
            out[f"{case}_sigma"], std = probe_vobj(smp, sigmas, kind == "v")
            if kind == "v":
                out[f"{case}_std"] = std
        noise = VC.toy_noise()
        torch.manual_seed(VC.TOY_SEED + 1)
        with torch.no_grad():
            y = smp(noise, fn=VC.toy_fn, net=None, sigmas=sigmas)
        nxt = torch.randn(4)
        n_draws = {"ve": smp.num_steps, "vp": smp.num_steps, "v": int((torch.cat([sigmas, torch.zeros(1)])[1:smp.num_steps + 1] != 0).sum()), "veuler": 0}[kind]
        torch.manual_seed(VC.TOY_SEED + 1)
        draws = torch.stack([torch.randn_like(noise) for _ in range(n_draws)]) if n_draws else torch.zeros((0,) + tuple(noise.shape))
        assert torch.equal(torch.randn(4), nxt), (case, "the reference makes another number of draws than this generator assumes")
        args_ = dict(kw)
        n = args_.pop("num_steps")
        with torch.no_grad():
            if kind == "ve":
                mine = VR.ve_sampler(noise, VC.toy_fn, sigmas, n, draws=draws, **args_)
            elif kind == "vp":
                mine = VR.vp_sampler(noise, VC.toy_fn, sigmas, n, draws=draws, **args_)
            elif kind == "v":
                mine = VR.v_sampler(noise, VC.toy_fn, sigmas, n, draws=draws, **args_)
            else:
                mine = VR.veuler_sampler(noise, VC.toy_fn, sigmas, n, **args_)
        e = rel(mine, y)
        print("toy", case, "vsamp_ref vs reference", e, "equal" if torch.equal(mine, y) else "", "max |y|", float(y.abs().max()))
        assert e <= TOY_PIN and bool(torch.isfinite(y).all()), (case, e)
        out[f"toy_{case}_draws"], out[f"toy_{case}_out"], out[f"toy_{case}_next"] = draws.numpy(), y.numpy(), nxt.numpy()
        meta["toy"][case] = {"vsamp_ref_rel_err": e, "draws": n_draws, "max_abs": float(y.abs().max())}

    # ---- the runs of tests/vsamp_cases.py: conditioning and saturation of each, on the CPU -------------------------------------------------
    for name in VC.RUNS:
        sp = VC.spec(name)
        dt = VC.ref_dtype(sp)
        info = {}
        y = VC.reference(name, dt, info=info).double()
        rec = {"net": sp["net"], "sampler": sp["sampler"], "steps": sp["steps"], "out_scale": sp["out_scale"], "noise_scale": sp["noise_scale"],
               "max_abs": round(float(y.abs().max()), 6), "share_abs_ge_1": float((y.abs() >= 1).double().mean()),
               "clamped_share": info["clamped_share"],
               "dist_fp32_fp64": None if dt == torch.float32 else float(f"{rel(VC.reference(name, torch.float32), y):.4e}")}
        print(name, rec)
        assert bool(torch.isfinite(y).all()) and rec["max_abs"] > 0.05, name
        if sp["sampler"] == "vp":
            assert rec["max_abs"] > 1.0, (name, rec)                          # unclamped: the run must show it
        else:
            assert rec["share_abs_ge_1"] <= 0.01, (name, rec)
        assert rec["clamped_share"] <= 0.5, (name, rec)
        assert rec["dist_fp32_fp64"] is None or rec["dist_fp32_fp64"] < 2.5e-4, (name, rec)      # well conditioned: the bar of every run is the project's 1e-3
        meta["runs"][name] = rec

    if args.check_only:
        have = np.load(os.path.join(GOLD, "vsamp_golden.npz"))
        assert sorted(have.files) == sorted(out), (sorted(have.files), sorted(out))
        for k, v in out.items():
            assert np.array_equal(have[k], v, equal_nan=True), ("the committed fixture differs", k)
        with open(os.path.join(GOLD, "vsamp_golden.json")) as f:
            have_meta = json.load(f)
        assert have_meta["signatures"] == json.loads(json.dumps(meta["signatures"]))
        key = lambda runs: {k: (r["out_scale"], r["noise_scale"], r["steps"]) for k, r in runs.items()}
        assert key(have_meta["runs"]) == key(meta["runs"])
        print("vsamp_golden.npz reproduced:", len(out), "arrays equal")
        return
    np.savez_compressed(os.path.join(GOLD, "vsamp_golden.npz"), **out)
    with open(os.path.join(GOLD, "vsamp_golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote vsamp_golden.npz", sum(v.nbytes for v in out.values()) // 1024, "KiB")


if __name__ == "__main__":
    main()
