"""Fixture generator (build container only: it imports the reference project on the CPU, as tools/gen_golden_dac.py does) for the DAC encoder stack:
runs the REFERENCE's ``src/models/backbones/dac/dac.py::Encoder`` on the cases ``odd`` and ``w96`` of tests/dac_enc_ref.py and
``src/models/backbones/dac_vae.py::FineTuneAutoencoder.encode(x, is_train=False)`` on ``ae`` and ``ae_clamp``, and pins the CPU restatement
tests/dac_enc_ref.py to them.  Only its output is committed; nothing that runs on the GPU machine imports the reference.

Usage:  python tools/gen_golden_dac_enc.py [--check-only]        (--check-only recomputes everything and compares it with the committed fixture)

tests/golden/dac_enc_golden.npz, per case ``<case>``:
    ``<case>_x``                 the input (tests/dac_enc_ref.py ``inputs``);
    ``<case>_out``               what the reference module returned (fp32): the encoder's result, or the autoencoder's mean;
    ``<case>_kl``                the autoencoder's KL term (fp32);
    ``<case>_<tap>``             forward hooks: ``block.<i>`` of every EncoderBlock and the last conv (``odd`` also ``block.0``); the autoencoder's
                                 last ``encoder_layers`` conv and ``btnk_layer``.  (Every tap is compared in the report; these fit the file under 1 MB.)
tests/golden/dac_enc_golden_report.json: the reference's state-dict names and shapes per case, the constructor and ``encode`` signatures, and per
hooked tensor the distance max |restatement - reference| / max |reference| of tests/dac_enc_ref.py in fp32 and in float64 (bar 5e-6; the KL term
relative to itself).
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

NPZ = os.path.join(ROOT, "tests", "golden", "dac_enc_golden.npz")
REPORT = os.path.join(ROOT, "tests", "golden", "dac_enc_golden_report.json")
BAR = 5e-6
STORED = {"odd": None, "w96": ("block.1", "block.3"), "ae": ("encoder_layers.5", "btnk_layer"), "ae_clamp": ("encoder_layers.1", "btnk_layer")}


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def relf(a, b):
    return abs(float(a) - float(b)) / (abs(float(b)) + 1e-300)


def hooked(net, ER, case, got):
    """Forward hooks on every module the library keeps a tap of."""
    hook = lambda name: (lambda m, i, o: got.__setitem__(name, o.detach().clone()))
    hooks = []
    if ER.kind(case) == "ae":
        for j, m in enumerate(net.encoder_layers):
            if j % 2 == 1:
                hooks.append(m.register_forward_hook(hook(f"encoder_layers.{j}")))
        hooks.append(net.btnk_layer.register_forward_hook(hook("btnk_layer")))
    else:
        n = len(ER.ctor_kwargs(case)["strides"])
        hooks.append(net.block[0].register_forward_hook(hook("block.0")))
        hooks.append(net.block[n + 2].register_forward_hook(hook(f"block.{n + 2}")))
        for i in range(1, n + 1):
            hooks.append(net.block[i].register_forward_hook(hook(f"block.{i}")))
            for j in range(3):
                hooks.append(net.block[i].block[j].register_forward_hook(hook(f"block.{i}.block.{j}")))
    return hooks


def reference_run(RD, RV, case, ER, dtype):
    """(hooked tensors, output, state-dict layout) of one case on the reference module in ``dtype``."""
    kw = ER.ctor_kwargs(case)
    torch.manual_seed(0)
    net = (RV.FineTuneAutoencoder(**kw) if ER.kind(case) == "ae" else RD.Encoder(kw["d_model"], kw["strides"], kw["d_latent"])).eval()
    layout = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    net.load_state_dict(ER.weights(case), strict=True)
    net = net.to(dtype)
    got = {}
    hooks = hooked(net, ER, case, got)
    x = ER.inputs(case).to(dtype)
    with torch.no_grad():
        out = net.encode(x, is_train=False) if ER.kind(case) == "ae" else net(x)
    for h in hooks:
        h.remove()
    return got, out, layout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(8)
    import_reference()
    from src.models.backbones.dac import dac as RD
    from src.models.backbones import dac_vae as RV
    import dac_enc_ref as ER

    out = {}
    report = {"signature": {"Encoder": str(inspect.signature(RD.Encoder.__init__)),
                            "FineTuneAutoencoder": str(inspect.signature(RV.FineTuneAutoencoder.__init__)),
                            "FineTuneAutoencoder.encode": str(inspect.signature(RV.FineTuneAutoencoder.encode)),
                            "FineTuneAutoencoder.forward": str(inspect.signature(RV.FineTuneAutoencoder.forward))},
              "bar": BAR, "cases": {}}
    for case in ER.GOLDEN_CASES:
        ae = ER.kind(case) == "ae"
        dist, ref32 = {}, None
        for dname, dt in (("fp32", torch.float32), ("fp64", torch.float64)):
            got, ref_out, layout = reference_run(RD, RV, case, ER, dt)
            taps = {}
            with torch.no_grad():
                y = ER.forward(case, dtype=dt, taps=taps)
            assert sorted(taps) == sorted(got), (sorted(taps), sorted(got))
            d = {"mean": rel(y[0], ref_out[0]), "kl": relf(y[1], ref_out[1])} if ae else {"out": rel(y, ref_out)}
            for k in got:
                d[k] = rel(taps[k], got[k])
            dist[dname] = d
            worst = max(d.values())
            print(f"{case:8s} {dname}: worst restatement-vs-reference distance {worst:.3e} over {len(d)} tensors")
            assert worst < BAR, (case, dname, d)
            if dt == torch.float32:
                ref32 = (got, ref_out, layout)
        got, ref_out, layout = ref32
        y64, _ = ER.reference(case)
        main_out = ref_out[0] if ae else ref_out
        rec = {"ctor": ER.ctor_kwargs(case), "state_dict": layout, "dist": dist, "out_shape": list(main_out.shape),
               "fp32_reference_vs_fp64_restatement": rel(main_out, y64[0] if ae else y64), "max_abs_out": float(main_out.abs().max())}
        if ae:
            rec["kl"] = float(ref_out[1])
            rec["kl_fp32_reference_vs_fp64_restatement"] = relf(ref_out[1], y64[1])
            out[f"{case}_kl"] = ref_out[1].numpy()
        report["cases"][case] = rec
        out[f"{case}_x"], out[f"{case}_out"] = ER.inputs(case).numpy(), main_out.numpy()
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
