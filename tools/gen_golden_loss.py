"""Fixture generator (build container only: it imports the reference project on the CPU, as tools/gen_golden_rf.py does) for the validation loss:
writes ``tests/golden/loss_golden.npz`` + ``loss_golden.json`` from the REFERENCE's classes (``distribution.LogNormalDistribution`` /
``UniformDistribution`` / ``LogUniformDistribution`` / ``LogitDistribution``; ``diffusion.EluDiffusion`` / ``VEDiffusion`` / ``VPDiffusion`` / ``ReFlow``)
and pins the CPU restatement ``tests/loss_ref.py`` and the package's classes to them.  Only its output is committed; nothing that runs on the GPU
machine imports the reference.

Usage:  python tools/gen_golden_loss.py [--check-only]        (--check-only recomputes everything and compares it with the committed fixture)

What the fixture holds
  * ``dist_<name>``: 16 draws of each distribution of DISTRIBUTIONS below after ``torch.manual_seed(seed)`` (json: class, keywords, seed);
  * ``loss_x`` [3, 2, 8, 4] (tests/loss_ref.py ``inputs``), ``loss_noise`` (what ``randn_like`` gives after ``torch.manual_seed(LOSS_SEED)``: the draw
    of every ``forward`` below), ``coef_<kind>`` (sigmas for edm / ve, times for vp / rf) and ``loss_<case>``: the [3] losses of the reference's
    ``forward`` around ``loss_ref.toy_net`` -- EluDiffusion(0.2), EluDiffusion(0.2, dynamic_threshold=0.9), VEDiffusion(), VPDiffusion(0.1, 19.9, 1000),
    ReFlow() -- plus EluDiffusion(0.2) with ``inference=True``;
  * json: how far tests/loss_ref.py (fp32 and float64) and the package's classes are from each recorded loss.
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
from oracle.gen_golden import import_reference, GOLD          # noqa: E402

N_DRAWS = 16
LOSS_SEED = 11
LOSS_SHAPE = (3, 2, 8, 4)
PIN = 1e-6                   # per-sample relative: the package's classes and the fp32 restatement against the reference's losses
# name -> (class, keywords, seed)
DISTRIBUTIONS = {
    "lognormal": ("LogNormalDistribution", {"mean": -3.0, "std": 1.0}, 101),
    "uniform": ("UniformDistribution", {}, 102),
    "uniform_range": ("UniformDistribution", {"vmin": 0.2, "vmax": 0.9}, 103),
    "loguniform": ("LogUniformDistribution", {}, 104),
    "loguniform_range": ("LogUniformDistribution", {"sigma_min": 0.01, "sigma_max": 50.0}, 105),
    "logit_uniform": ("LogitDistribution", {}, 106),
    "logit_ln": ("LogitDistribution", {"ln_scale": True}, 107),
    "logit_ln_shift": ("LogitDistribution", {"logit_mean": 0.3, "logit_std": 1.2, "ln_scale": True}, 108),
    "logit_stratified": ("LogitDistribution", {"logit_mean": -0.2, "logit_std": 0.8, "ln_scale": True, "stratified": True}, 109),
    "logit_stratified_flag_only": ("LogitDistribution", {"stratified": True}, 110),       # without ln_scale the flag is not read
}
# case -> (kind of tests/loss_ref.py, class, keywords, forward keywords, loss_ref.forward keywords)
LOSSES = {
    "edm": ("edm", "EluDiffusion", {"sigma_data": 0.2}, {}, {}),
    "edm_dyn": ("edm", "EluDiffusion", {"sigma_data": 0.2, "dynamic_threshold": 0.9}, {}, {"dynamic_threshold": 0.9}),
    "edm_inference": ("edm", "EluDiffusion", {"sigma_data": 0.2}, {"inference": True}, {}),
    "ve": ("ve", "VEDiffusion", {}, {}, {}),
    "vp": ("vp", "VPDiffusion", {"beta_min": 0.1, "beta_d": 19.9, "M": 1000}, {}, {}),
    "rf": ("rf", "ReFlow", {}, {}, {}),
}


def rel_b(a, b):
    """Largest per-sample relative distance of two [B] loss vectors."""
    return float(((a.double() - b.double()).abs() / b.double().abs()).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(8)
    import_reference()
    from src.models.components import diffusion as RD, distribution as RDist
    import audiodiffuser_amd as A
    import loss_ref as LR

    out, meta = {}, {"distributions": {}, "losses": {}, "n_draws": N_DRAWS, "loss_seed": LOSS_SEED}
    # ---- distributions ---------------------------------------------------------------------------------------------------------------
    for name, (cls, kw, seed) in DISTRIBUTIONS.items():
        torch.manual_seed(seed)
        want = getattr(RDist, cls)(**kw)(num_samples=N_DRAWS, device=torch.device("cpu"))
        torch.manual_seed(seed)
        got = getattr(A, cls)(**kw)(num_samples=N_DRAWS, device=torch.device("cpu"))
        assert torch.equal(got, want), name
        out[f"dist_{name}"] = want.numpy()
        meta["distributions"][name] = {"class": cls, "kwargs": kw, "seed": seed}

    # ---- losses ----------------------------------------------------------------------------------------------------------------------
    x, _ = LR.inputs(LOSS_SHAPE)
    torch.manual_seed(LOSS_SEED)
    noise = torch.randn_like(x)
    out["loss_x"], out["loss_noise"] = x.numpy(), noise.numpy()
    for case, (kind, cls, kw, fkw, rkw) in LOSSES.items():
        coef = LR.coefs(kind, LOSS_SHAPE[0])
        out[f"coef_{kind}"] = coef.numpy()
        with torch.no_grad():
            torch.manual_seed(LOSS_SEED)
            want = getattr(RD, cls)(**kw)(x, LR.toy_net, sigmas=coef, **fkw)
            torch.manual_seed(LOSS_SEED)
            mine = getattr(A, cls)(**kw)(x, LR.toy_net, sigmas=coef, **fkw)
            r32 = LR.forward(kind, LR.toy_net, x, noise, coef, **rkw)
            r64 = LR.forward(kind, LR.toy_net, x.double(), noise, coef, **rkw)
        rec = {"kind": kind, "class": cls, "kwargs": kw, "forward_kwargs": fkw, "package_rel": rel_b(mine, want), "loss_ref_fp32_rel": rel_b(r32, want),
               "loss_ref_fp64_rel": rel_b(r64, want), "losses": [float(v) for v in want]}
        print(case, rec)
        assert want.shape == (LOSS_SHAPE[0],) and bool(torch.isfinite(want).all())
        assert rec["package_rel"] <= PIN and rec["loss_ref_fp32_rel"] <= PIN and rec["loss_ref_fp64_rel"] <= PIN, (case, rec)
        out[f"loss_{case}"] = want.numpy()
        meta["losses"][case] = rec

    if args.check_only:
        have = np.load(os.path.join(GOLD, "loss_golden.npz"))
        assert sorted(have.files) == sorted(out), (sorted(have.files), sorted(out))
        for k, v in out.items():
            assert np.array_equal(have[k], v), ("the committed fixture differs", k)
        print("loss_golden.npz reproduced:", len(out), "arrays equal")
        return
    np.savez_compressed(os.path.join(GOLD, "loss_golden.npz"), **out)
    with open(os.path.join(GOLD, "loss_golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote loss_golden.npz", sum(v.nbytes for v in out.values()), "bytes")


if __name__ == "__main__":
    main()
