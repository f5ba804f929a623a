"""Golden vectors for the constructor and shape sweep of the 1-D U-Net (oracle/unet1d_sweep.py): the REFERENCE ``UNet1dBase`` imported on CPU and
built for every sweep configuration with this repo's generated weights; checks the oracle restatement against it on the output and on every module
boundary a forward hook reaches (bound 2e-5, as oracle/gen_golden.py), and writes ``tests/golden/unet1d_sweep_golden.npz`` +
``unet1d_sweep_golden_report.json``: per case the inputs, ``y`` and the hooked block outputs, strided (``sub(v, stride)``, stride 7 or the next
prime that keeps a case near 12000 values, so the whole fixture stays under 1 MB).  A form the reference refuses to build or run is recorded in the
report under "refused" and left out of the fixture.

Usage:  python oracle/gen_golden_unet1d_sweep.py [--check-only]
Test infrastructure only (see oracle/__init__.py)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference, build_ref_net, rel_err, sub, GOLD   # noqa: E402

PRIMES = (7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131)
PER_CASE = 12000            # values of strided block outputs per case


def hooked_forward(net, x, t, classes=None, cond_drop_prob=0.0):
    taps, hs = {}, []
    u = net.unet

    def add(mod, name):
        hs.append(mod.register_forward_hook(lambda m, i, o, name=name: taps.__setitem__(name, o.detach())))
    add(u.to_in, "to_in"); add(u.to_time, "temb")
    for i, d in enumerate(u.downsamples):
        add(d.downsample, f"down{i}.conv")
        for j, b in enumerate(d.blocks):
            add(b, f"down{i}.block{j}")
        if d.use_attention:
            add(d.transformer, f"down{i}.attn")
    add(u.bottleneck.pre_block, "mid.pre")
    if u.bottleneck.use_attention:
        add(u.bottleneck.transformer, "mid.attn")
    add(u.bottleneck.post_block, "mid.post")
    for k, up in enumerate(u.upsamples):
        for j, b in enumerate(up.blocks):
            add(b, f"up{k}.block{j}")
        if up.use_attention:
            add(up.transformer, f"up{k}.attn")
        add(up.upsample, f"up{k}.conv")
    if classes is not None:
        add(net.label_conditioner, "class_emb")
    y = net(x, t, classes=classes, cond_drop_prob=cond_drop_prob)
    for h in hs:
        h.remove()
    return y, taps


def main():
    check_only = "--check-only" in sys.argv
    torch.manual_seed(0)
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    ref = import_reference()
    from audiodiffuser_amd.weights import generate_weights
    from oracle import unet1d as O
    from oracle.unet1d_sweep import CASES, inputs

    out, report = {}, {"bound": 2e-5, "cases": {}, "refused": {}}
    for cid, (cfg, shape, seed, _) in CASES.items():
        w = generate_weights(cfg, seed=seed)
        x, t = inputs(cfg, shape, seed)
        try:
            net = build_ref_net(ref, cfg, w)
            y_ref, taps_ref = hooked_forward(net, x, t)
        except Exception as e:                      # the reference itself refuses the form
            report["refused"][cid] = f"{type(e).__name__}: {e}"
            continue
        taps_o = {}
        y_o = O.unet1d_forward(w, cfg, x, t, taps=taps_o)
        # (.h1 = conv1 output inside a resblock, .attn.<x> = stored tensors inside a transformer block: no module boundary to hook)
        assert {k for k in taps_o if not k.endswith(".h1") and ".attn." not in k} == set(taps_ref), cid
        errs = {k: rel_err(taps_o[k], v) for k, v in taps_ref.items()}
        errs["out"] = rel_err(y_o, y_ref)
        worst = max(errs, key=errs.get)
        assert errs[worst] < 2e-5, (cid, worst, errs[worst])
        total = sum(v.numel() for v in taps_ref.values())
        stride = next(p for p in PRIMES if total / p <= PER_CASE)
        report["cases"][cid] = {"shape": list(shape), "seed": seed, "hooked": len(taps_ref), "worst": worst, "max_rel_err_over_taps": errs[worst],
                                "out_rel_err": errs["out"], "stride": stride}
        out[f"{cid}_x"] = x.numpy(); out[f"{cid}_t"] = t.numpy(); out[f"{cid}_y"] = y_ref.numpy()
        out[f"{cid}_stride"] = np.array([stride], dtype=np.int32)
        for k, v in taps_ref.items():
            out[f"{cid}_tap_{k}"] = sub(v, stride)
    print(json.dumps(report))
    if check_only:
        return
    path = os.path.join(GOLD, "unet1d_sweep_golden.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(GOLD, "unet1d_sweep_golden_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
