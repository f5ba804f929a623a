"""Fixture generator (build container only: it imports the reference project on the CPU, as tools/gen_golden_vdpm.py does) for the DiT backbone:
runs the REFERENCE's ``src/models/backbones/dit.py::DiT`` on the three variants ``GOLDEN_CASES`` of tests/dit_ref.py and pins the CPU restatement
``tests/dit_ref.py`` to it.  Only its output is committed; nothing that runs on the GPU machine imports the reference.

Usage:  python tools/gen_golden_dit.py [--check-only]        (--check-only recomputes everything and compares it with the committed fixture)

tests/golden/dit_golden.npz, per variant ``<case>``:
    ``<case>_x`` / ``_t`` / ``_classes``   the inputs (tests/dit_ref.py ``inputs``);
    ``<case>_out``                          what the reference module returned (fp32; labels: cond_drop_prob = 0);
    ``<case>_null``                         labels only: the same call with cond_drop_prob = 1 (every sample takes the null embedding);
    ``<case>_blocks.<i>``                   the output of every DiTBlock (forward hooks), ``<case>_x_embedder`` that of PatchEmbed, ``<case>_c`` the
                                            conditioning vector the blocks received, ``<case>_final_layer`` the FinalLayer output before unpatchify;
    ``<case>_pos_embed``                    the reference's own ``pos_embed`` buffer as its constructor filled it.
tests/golden/dit_golden_report.json: the reference's state-dict names and shapes per variant, the constructor signature, and per tensor the distance
max |restatement - reference| / max |reference| of tests/dit_ref.py in fp32 and in float64 (the bar of tests/test_dit_ref.py is 5e-6), plus the mean
row variance entering blocks.0.norm1 (what makes ``lowvar`` see eps).
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

NPZ = os.path.join(ROOT, "tests", "golden", "dit_golden.npz")
REPORT = os.path.join(ROOT, "tests", "golden", "dit_golden_report.json")
BAR = 5e-6


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def reference_run(RD, case, DR):
    """(tensors of the fixture, state-dict layout) of one variant on the reference module."""
    kw = DR.ctor_kwargs(case)
    torch.manual_seed(0)
    net = RD.DiT(depth=kw.pop("depth"), cond_drop_prob=0.0, **kw).eval()
    layout = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    own_pos = net.pos_embed.detach().clone()
    w = DR.weights(case)
    net.load_state_dict(w, strict=True)
    x, t, classes = DR.inputs(case)
    got = {}
    hooks = [net.x_embedder.register_forward_hook(lambda m, i, o: got.__setitem__("x_embedder", o.detach().clone())),
             net.final_layer.register_forward_hook(lambda m, i, o: got.__setitem__("final_layer", o.detach().clone())),
             net.blocks[0].register_forward_hook(lambda m, i, o: got.__setitem__("c", i[1].detach().clone()))]
    for j, blk in enumerate(net.blocks):
        hooks.append(blk.register_forward_hook(lambda m, i, o, j=j: got.__setitem__(f"blocks.{j}", o.detach().clone())))
    with torch.no_grad():
        out = net(x, t, classes=classes, cond_drop_prob=0.0)
        for h in hooks:
            h.remove()
        null = net(x, t, classes=classes, cond_drop_prob=1.0) if classes is not None else None
    # (the module adds pos_embed after the PatchEmbed hook fires: the restatement's tap is the sum)
    got["x_embedder"] = got["x_embedder"] + w["pos_embed"]
    tensors = {"x": x, "t": t, "out": out, "pos_embed": own_pos, **got}
    if classes is not None:
        tensors["classes"], tensors["null"] = classes, null
    return tensors, layout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(8)
    import_reference()
    from src.models.backbones import dit as RD
    import dit_ref as DR

    out, report = {}, {"signature": str(inspect.signature(RD.DiT.__init__)), "bar": BAR, "variants": {}}
    for case in DR.GOLDEN_CASES:
        tensors, layout = reference_run(RD, case, DR)
        cfg, w = DR.config(case), DR.weights(case)
        x, t, classes = DR.inputs(case)
        dist = {}
        for dname, dt in (("fp32", torch.float32), ("fp64", torch.float64)):
            taps = {}
            y = DR.forward(w, cfg, x, t, classes, dtype=dt, taps=taps)
            d = {"out": rel(y, tensors["out"])}
            for k in tensors:
                if k in taps:
                    d[k] = rel(taps[k], tensors[k])
            if classes is not None:
                d["null"] = rel(DR.forward(w, cfg, x, t, classes, cond_drop_prob=1.0, dtype=dt), tensors["null"])
            dist[dname] = d
            worst = max(d.values())
            print(f"{case:8s} {dname}: worst restatement-vs-reference distance {worst:.3e} over {len(d)} tensors")
            assert worst < BAR, (case, dname, d)
        from audiodiffuser_amd.dit import sincos_pos_embed
        assert torch.equal(sincos_pos_embed(cfg.hidden_size, cfg.grid), tensors["pos_embed"][0]), "pos_embed is not bit-equal to the reference's"
        taps = {}
        DR.forward(w, cfg, x, t, classes, taps=taps)
        report["variants"][case] = {"ctor": DR.ctor_kwargs(case), "state_dict": layout, "dist": dist,
                                    "norm1_row_variance": float(taps["x_embedder"].var(dim=-1, unbiased=False).mean()),
                                    "max_abs_out": float(tensors["out"].abs().max())}
        for k, v in tensors.items():
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


if __name__ == "__main__":
    main()
