"""Golden vectors for the width and shape sweep of WaveNetNoise (oracle/wavenet_sweep.py): the REFERENCE ``WaveNetNoise`` imported on CPU and built for
every sweep configuration but ``deep`` with this repo's generated weights; checks the fp32 oracle restatement (the reference's arithmetic, not
``exact_norm``) against it on the output and on what a forward hook reaches -- every layer input ``y<n>``, every gated activation ``g<n>``, the skip sum
and the activated skip projection ``sp``, as oracle/gen_golden_next.py does at the presets -- at 2e-5, and writes
``tests/golden/wavenet_sweep_golden.npz`` + ``wavenet_sweep_golden_report.json``: per case the inputs, ``y`` and the hooked tensors, strided
(``sub(v, stride)``, the smallest prime that keeps a case near 5000 values, so the whole fixture stays under 1 MB).  A form the reference refuses to
build or run is recorded in the report under "refused" and left out of the fixture.

``deep`` (1024 layers) is pinned by construction only: the same restatement loop as ``cyc24`` / ``d4096``, which are pinned here, run over more layers.
The report also carries, per case and unbounded, how far the fp32 oracle lies from its own float64 run in the reference's arithmetic and with
``exact_norm`` (tests/test_oracle_wavenet_sweep.py bounds the second).

Usage:  python oracle/gen_golden_wavenet_sweep.py [--check-only]      (--check-only: recompute, compare with the committed report, write nothing)
Test infrastructure only (see oracle/__init__.py)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import rel_err, sub, GOLD                      # noqa: E402
from oracle.gen_golden_next import import_next, load_into             # noqa: E402

BOUND = 2e-5
PER_CASE = 5000             # values of strided hooked tensors per case
NOT_BUILT = {"deep": "pinned by construction: the restatement loop of cyc24 / d4096 (pinned against the reference here) over 1024 layers"}
REPORT = os.path.join(GOLD, "wavenet_sweep_golden_report.json")


def primes():
    n = 2
    while True:
        if all(n % d for d in range(2, int(n ** 0.5) + 1)):
            yield n
        n += 1


def hooked_forward(net, audio, step):
    taps, hs = {}, []
    for n, blk in enumerate(net.residual_layer.residual_blocks):
        hs.append(blk.dilated_conv.register_forward_hook(lambda _m, i, _o, k=f"y{n}": taps.__setitem__(k, i[0].detach())))
        hs.append(blk.output_projection.register_forward_hook(lambda _m, i, _o, k=f"g{n}": taps.__setitem__(k, i[0].detach())))
    hs.append(net.residual_layer.register_forward_hook(lambda _m, _i, o: taps.__setitem__("skip", o.detach())))
    hs.append(net.output_projection.register_forward_hook(lambda _m, i, _o: taps.__setitem__("sp", i[0].detach())))
    y = net(audio, step)
    for h in hs:
        h.remove()
    return y, taps


def main():
    check_only = "--check-only" in sys.argv
    torch.manual_seed(0)
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    ref = import_next()
    from oracle import wavenet as W
    from oracle import wavenet_sweep as SW

    out, report = {}, {"bound": BOUND, "cases": {}, "refused": {}, "not_built": NOT_BUILT, "fp32_oracle_vs_float64": {}}
    for cid, (cfg, shape, seed, _, _) in SW.CASES.items():
        _, _, dist = SW.float64_case(cid)
        worst = [max(dist, key=lambda k: dist[k][j]) for j in (0, 1)]
        report["fp32_oracle_vs_float64"][cid] = {"reference_arithmetic": dist[worst[0]][0], "reference_arithmetic_worst": worst[0],
                                                 "exact_norm": dist[worst[1]][1], "exact_norm_worst": worst[1]}
        if cid in NOT_BUILT:
            continue
        w, _ = SW.weights(cid)
        audio, step = SW.case_inputs(cid)
        try:
            net = load_into(ref["WaveNetNoise"](**cfg.to_kwargs()), w)
            y_ref, taps_ref = hooked_forward(net, audio, step)
        except Exception as e:                      # the reference itself refuses the form
            report["refused"][cid] = f"{type(e).__name__}: {e}"
            continue
        taps_o = {}
        y_o = W.wavenet_forward(w, cfg, audio, step, taps=taps_o)
        assert set(taps_o) == set(taps_ref) and len(taps_ref) == 2 * cfg.residual_layers + 2, cid
        errs = {k: rel_err(taps_o[k], v) for k, v in taps_ref.items()}
        errs["out"] = rel_err(y_o, y_ref)
        worst = max(errs, key=errs.get)
        assert errs[worst] < BOUND, (cid, worst, errs[worst])
        assert float(y_ref.abs().max()) > 1e-2, "vacuous output"
        total = sum(v.numel() for v in taps_ref.values())
        stride = next(p for p in primes() if p >= 3 and total / p <= PER_CASE)
        report["cases"][cid] = {"config": [cfg.residual_channels, cfg.residual_layers, cfg.dilation_cycle], "shape": list(shape), "seed": seed,
                                "hooked": len(taps_ref), "worst": worst, "max_rel_err_over_taps": errs[worst], "out_rel_err": errs["out"], "stride": stride}
        out[f"{cid}_audio"] = audio.numpy(); out[f"{cid}_step"] = step.numpy(); out[f"{cid}_y"] = y_ref.numpy()
        out[f"{cid}_stride"] = np.array([stride], dtype=np.int32)
        for k, v in taps_ref.items():
            out[f"{cid}_tap_{k}"] = sub(v, stride)
        del net
    print(json.dumps(report))
    if check_only:
        with open(REPORT) as f:
            old = json.load(f)
        plain = lambda r: {c: {k: v for k, v in d.items() if not isinstance(v, float)} for c, d in r["cases"].items()}
        assert plain(old) == plain(report) and old["refused"] == report["refused"] and old["not_built"] == report["not_built"], "the committed report differs"
        moved = {c: (old["cases"][c]["max_rel_err_over_taps"], d["max_rel_err_over_taps"]) for c, d in report["cases"].items()
                 if old["cases"][c]["max_rel_err_over_taps"] != d["max_rel_err_over_taps"]}
        print("agrees with the committed report" + (f"; figures that moved (both under the bound): {moved}" if moved else ", figure for figure"))
        return
    path = os.path.join(GOLD, "wavenet_sweep_golden.npz")
    np.savez_compressed(path, **out)
    with open(REPORT, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
