"""Fixture generator (build container only: it imports the reference project on the CPU, as tools/gen_golden_vsamp.py does) for the two program-driven
samplers: writes ``tests/golden/vdpm_golden.npz`` + ``vdpm_golden.json`` from the REFERENCE's classes (``sampler_vobj.DPMSampler`` /
``sampler_vobj.UniPCSampler``) and pins the CPU restatement ``tests/vdpm_ref.py`` to them.  Only its output is committed; nothing that runs on the GPU
machine imports the reference.

Usage:  python tools/gen_golden_vdpm.py [--check-only]        (--check-only recomputes everything and compares it with the committed fixture)

What the fixture holds
  * per host case of tests/vdpm_cases.py (``CASES``), read off the reference's own execution on the toy ``fn`` (4-D state, fp32):
        ``<case>_sigmas``   the schedule;
        ``<case>_logsnr``   the fp32 log-SNR of every ``fn`` call, in call order;
        ``<case>_used``     0 for the calls whose result the reference discards -- those made inside ``multistep_dpm_solver_1_step`` while the model
                            output is handed in (sampler_vobj.py:323) --, 1 for every other;
        ``<case>_solves``   [n, 3] what every ``torch.linalg.solve`` of the run returned (the reference's own ``rhos_p`` / ``rhos_c`` of the UniPC
                            updates that solve for them, in call order, NaN-padded; [0, 3] for a run that solves nothing);
        ``toy_<case>_out``  what the reference returned.
  * json: constructor signatures, per case the call counts with and without the discarded calls and how far tests/vdpm_ref.py is from the toy run
    (its own call record and ``rhos`` must equal the reference's exactly), and for every run of tests/vdpm_cases.py (``RUNS``, what
    tests/test_vdpm_gpu.py runs on the device) its inputs, max |y|, share of entries at the final clamp and ``dist_fp32_fp64`` = max |y32 - y64| /
    max |y64| of the CPU restatement (the bar of a run is max(1e-3, 4 * dist_fp32_fp64)).  The ADM oracle only runs in fp32, so its run has no distance.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle.gen_golden import import_reference, GOLD          # noqa: E402
from gen_golden_vsamp import TOY_PIN, signature_of, rel        # noqa: E402


def reference_toy_run(cls, kind, kw, sigmas, noise, toy_fn):
    """(result, log-SNRs handed to fn, used flags, solve outputs) of one run of the reference's class."""
    smp = cls(**kw)
    calls, used, solves, inside = [], [], [], [False]

    def fn(x, net=None, sigma=None, **_):
        calls.append(float(sigma)); used.append(0 if inside[0] else 1)
        return toy_fn(x, sigma)
    if kind == "dpm":
        inner = smp.multistep_dpm_solver_1_step

        def flagged(*a, model_s=None, **k):
            inside[0] = model_s is not None
            try:
                return inner(*a, model_s=model_s, **k)
            finally:
                inside[0] = False
        smp.multistep_dpm_solver_1_step = flagged
    real = torch.linalg.solve

    def solve(A, B):
        r = real(A, B)
        solves.append([float(v) for v in r] + [float("nan")] * (3 - r.numel()))
        return r
    torch.linalg.solve = solve
    try:
        with torch.no_grad():
            y = smp(noise, fn=fn, net=None, sigmas=sigmas)
    finally:
        torch.linalg.solve = real
    return y, np.array(calls, np.float32), np.array(used, np.int32), np.array(solves, np.float32).reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import_reference()
    from src.models.components import sampler_vobj as RSV
    import vdpm_cases as DC
    import vdpm_ref as DR

    ref_cls = {"dpm": RSV.DPMSampler, "unipc": RSV.UniPCSampler}
    out, meta = {}, {"signatures": {c.__name__: signature_of(c) for c in ref_cls.values()}, "toy": {}, "runs": {}}

    # ---- host cases: what the reference hands fn, what it solves for, what it returns ----------------------------------------------------
    for case, (kind, kw, sigmas) in DC.CASES.items():
        noise = DC.toy_noise(DC.toy_scale(kw))
        y, calls, used, solves = reference_toy_run(ref_cls[kind], kind, kw, sigmas, noise, DC.toy_fn)
        rec, rhos = [], []
        with torch.no_grad():
            if kind == "dpm":
                mine = DR.dpm_sampler(noise, DC.toy_fn, sigmas, kw["num_steps"], kw["order"], kw.get("multisteps", False), kw.get("x0_pred", True), record=rec)
            else:
                mine = DR.unipc_sampler(noise, DC.toy_fn, sigmas, kw["num_steps"], kw["order"], kw.get("x0_pred", True), record=rec, rhos=rhos)
        e = rel(mine, y)
        print("toy", case, "vdpm_ref vs reference", e, "equal" if torch.equal(mine, y) else "", "max |y|", float(y.abs().max()),
              "calls", len(calls), "used", int(used.sum()), "solves", len(solves))
        assert e <= TOY_PIN and bool(torch.isfinite(y).all()) and 0.02 < float(y.abs().max()), (case, e)
        assert float((y.abs() >= 1).float().mean()) <= 0.25, (case, "the toy run is mostly clamped")
        assert [np.float32(r["logsnr"]) for r in rec] == list(calls) and [int(r["used"]) for r in rec] == list(used), (case, "vdpm_ref calls fn differently")
        mine_solves = [v for p, c in rhos for v in ([p] if len(p) > 1 else []) + ([c] if len(c) > 1 else [])]
        assert len(mine_solves) == len(solves) and all(np.array_equal(np.array(a, np.float32), s[:len(a)]) for a, s in zip(mine_solves, solves)), case
        out[f"{case}_sigmas"], out[f"{case}_logsnr"], out[f"{case}_used"], out[f"{case}_solves"] = sigmas.numpy(), calls, used, solves
        out[f"toy_{case}_out"] = y.numpy()
        meta["toy"][case] = {"vdpm_ref_rel_err": e, "calls": int(len(calls)), "calls_used": int(used.sum()), "max_abs": float(y.abs().max())}

    # ---- the runs of tests/vdpm_cases.py: conditioning and saturation of each, on the CPU ---------------------------------------------------
    for name in DC.RUNS:
        sp = DC.spec(name)
        dt = DC.ref_dtype(sp)
        calls = []
        y = DC.reference(name, dt, record=calls).double()
        rec = {k: sp[k] for k in ("net", "shape", "sampler", "order", "steps", "multisteps", "x0_pred", "cond_scale", "out_scale", "noise_scale", "noise_seed",
                                  "t0", "t1")}
        rec.update(evaluations=len(calls), max_abs=round(float(y.abs().max()), 6), share_abs_ge_1=float((y.abs() >= 1).double().mean()),
                   dist_fp32_fp64=None if dt == torch.float32 else float(f"{rel(DC.reference(name, torch.float32), y):.4e}"))
        print(name, rec)
        assert bool(torch.isfinite(y).all()) and rec["max_abs"] > 0.05, name
        assert rec["share_abs_ge_1"] <= 0.01, (name, rec)
        assert rec["dist_fp32_fp64"] is None or rec["dist_fp32_fp64"] < 2.5e-4, (name, rec)
        meta["runs"][name] = rec

    if args.check_only:
        have = np.load(os.path.join(GOLD, "vdpm_golden.npz"))
        assert sorted(have.files) == sorted(out), (sorted(have.files), sorted(out))
        for k, v in out.items():
            assert np.array_equal(have[k], v, equal_nan=True), ("the committed fixture differs", k)
        with open(os.path.join(GOLD, "vdpm_golden.json")) as f:
            have_meta = json.load(f)
        assert have_meta["signatures"] == json.loads(json.dumps(meta["signatures"]))
        key = lambda runs: {k: (r["out_scale"], r["noise_scale"], r["steps"]) for k, r in runs.items()}
        assert key(have_meta["runs"]) == key(meta["runs"])
        print("vdpm_golden.npz reproduced:", len(out), "arrays equal")
        return
    np.savez_compressed(os.path.join(GOLD, "vdpm_golden.npz"), **out)
    with open(os.path.join(GOLD, "vdpm_golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote vdpm_golden.npz", sum(v.nbytes for v in out.values()) // 1024, "KiB")


if __name__ == "__main__":
    main()
