"""Fixture generator (build container only: it imports the reference project on the CPU, as tools/gen_golden_dit.py does) for the DAC decoder stack:
runs the REFERENCE's ``src/models/backbones/dac/dac.py::Decoder`` on the cases ``odd`` and ``w96`` of tests/dac_ref.py and
``src/models/backbones/dac_vae.py::FineTuneAutoencoder.decode`` on ``ae``, and pins the CPU restatement tests/dac_ref.py to them.  Only its output
is committed; nothing that runs on the GPU machine imports the reference.

Usage:  python tools/gen_golden_dac.py [--check-only]        (--check-only recomputes everything and compares it with the committed fixture)

tests/golden/dac_golden.npz, per case ``<case>``:
    ``<case>_x``                 the input (tests/dac_ref.py ``inputs``);
    ``<case>_out``               what the reference module returned (fp32);
    ``<case>_<tap>``             forward hooks: ``model.<i>`` of every DecoderBlock and the conv in front of tanh (``odd`` also ``model.0``);
                                 ``decoder_layers.0`` / ``.2`` of the autoencoder.  (Every tap is compared in the report; these fit the file under 1 MB.)
tests/golden/dac_golden_report.json: the reference's state-dict names and shapes per case, the two constructor signatures, and per hooked tensor the
distance max |restatement - reference| / max |reference| of tests/dac_ref.py in fp32 and in float64 (bar 5e-6).
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
from oracle.gen_golden import import_reference          # noqa: E402

NPZ = os.path.join(ROOT, "tests", "golden", "dac_golden.npz")
REPORT = os.path.join(ROOT, "tests", "golden", "dac_golden_report.json")
BAR = 5e-6
STORED = {"odd": None, "w96": ("model.1", "model.3"), "ae": ("decoder_layers.0", "decoder_layers.2")}      # None: every hooked tensor


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def reference_run(RD, RV, case, DR):
    """(hooked tensors, output, state-dict layout) of one case on the reference module."""
    kw = DR.ctor_kwargs(case)
    torch.manual_seed(0)
    got, hooks = {}, []
    hook = lambda name: (lambda m, i, o: got.__setitem__(name, o.detach().clone()))
    if DR.kind(case) == "ae":
        net = RV.FineTuneAutoencoder(**kw).eval()
        for j, m in enumerate(net.decoder_layers):
            if j % 2 == 0:
                hooks.append(m.register_forward_hook(hook(f"decoder_layers.{j}")))
    else:
        net = RD.Decoder(kw["input_channel"], kw["channels"], kw["rates"]).eval()
        n = len(kw["rates"])
        hooks.append(net.model[0].register_forward_hook(hook("model.0")))
        hooks.append(net.model[n + 2].register_forward_hook(hook(f"model.{n + 2}")))
        for i in range(1, n + 1):
            hooks.append(net.model[i].register_forward_hook(hook(f"model.{i}")))
            for j in range(1, 5):
                hooks.append(net.model[i].block[j].register_forward_hook(hook(f"model.{i}.block.{j}")))
    layout = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    net.load_state_dict(DR.weights(case), strict=True)
    with torch.no_grad():
        out = net.decode(DR.inputs(case)) if DR.kind(case) == "ae" else net(DR.inputs(case))
    for h in hooks:
        h.remove()
    return got, out, layout, net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(8)
    import_reference()
    from src.models.backbones.dac import dac as RD
    from src.models.backbones import dac_vae as RV
    import dac_ref as DR

    out = {}
    report = {"signature": {"Decoder": str(inspect.signature(RD.Decoder.__init__)), "FineTuneAutoencoder": str(inspect.signature(RV.FineTuneAutoencoder.__init__))},
              "bar": BAR, "cases": {}}
    for case in DR.GOLDEN_CASES:
        got, ref_out, layout, net = reference_run(RD, RV, case, DR)
        dist = {}
        for dname, dt in (("fp32", torch.float32), ("fp64", torch.float64)):
            taps = {}
            with torch.no_grad():
                y = DR.forward(case, dtype=dt, taps=taps)
                if dt == torch.float64:          # the reference module itself in float64 is what the float64 restatement must reproduce
                    net64 = net.double()
                    x64 = DR.inputs(case).double()
                    ref64 = net64.decode(x64) if DR.kind(case) == "ae" else net64(x64)
                    d = {"out": rel(y, ref64)}
                    net.float()
                else:
                    d = {"out": rel(y, ref_out)}
            assert sorted(taps) == sorted(got), (sorted(taps), sorted(got))
            if dt == torch.float32:
                for k in got:
                    d[k] = rel(taps[k], got[k])
            dist[dname] = d
            worst = max(d.values())
            print(f"{case:6s} {dname}: worst restatement-vs-reference distance {worst:.3e} over {len(d)} tensors")
            assert worst < BAR, (case, dname, d)
        y64, _ = DR.reference(case)
        report["cases"][case] = {"ctor": DR.ctor_kwargs(case), "state_dict": layout, "dist": dist, "out_shape": list(ref_out.shape),
                                 "fp32_reference_vs_fp64_restatement": rel(ref_out, y64), "max_abs_out": float(ref_out.abs().max())}
        out[f"{case}_x"], out[f"{case}_out"] = DR.inputs(case).numpy(), ref_out.numpy()
        for k, v in got.items():
            if STORED[case] is None and k.count(".") == 1 or STORED[case] is not None and k in STORED[case]:
                out[f"{case}_{k}"] = v.numpy()
    if args.check_only:
        old = np.load(NPZ)
        assert sorted(old.files) == sorted(out), "the committed fixture holds other tensors"
        for k in out:
            assert np.array_equal(old[k], out[k]), k
        print("fixture reproduced bit for bit")
        return
    np.savez_compressed(NPZ, **out)
    with open(REPORT, "w") as f:
        json.dump(report, f, indent=1)
    print(f"wrote {NPZ} ({os.path.getsize(NPZ)} bytes) and {REPORT}")
    assert os.path.getsize(NPZ) < 1000000


if __name__ == "__main__":
    main()
