"""The device side of tests/test_up_rows_gpu.py (its child process): the configs[1] network in bf16 at the given batches and waveform lengths, and
for every transposed conv of the up path the tensor the walk fed it, the tensor it stored and the GroupNorm statistics it reduced.

    ADF_GEMM_TRACE=1 [ADF_GEMM_UP=2] python tests/diag/gpu_up_rows_report.py OUT.pt B:LENGTH[:U,U,...] [...]        (U: only these convs are kept)

OUT.pt: {"B:LENGTH": {"upU.conv": {"fed": name of the tensor fed to it, "x": fp32 [B][Cin][L], "y": fp32 [B][Cout][f L],
"stats": float64 [B][8][2] or None}}} (the recorded bf16 tensors converted exactly); stderr: the [adf gemm] lines; last stdout line: a JSON summary."""
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import audiodiffuser_amd as A                      # noqa: E402
from audiodiffuser_amd.weights import generate_noise   # noqa: E402
import gpu_helpers as H                             # noqa: E402


def main():
    out_path, shapes = sys.argv[1], [s.split(":") for s in sys.argv[2:]]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = A.PRESETS["c2"]()
    net, _ = H.make_net(cfg, "bf16")
    dev = torch.device("cuda", torch.cuda.current_device())
    n_up = cfg.num_layers
    rep = {}
    for spec in shapes:
        B, length = int(spec[0]), int(spec[1])
        keep = [int(v) for v in spec[2].split(",")] if len(spec) > 2 else list(range(n_up))
        x = generate_noise(11, B, length) * 0.7
        t = torch.linspace(-0.9, 0.6, B)
        with torch.no_grad():
            net(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        hd = net.native(dev)
        names = hd.tap_names()
        case = {}
        for u in keep:
            name = f"up{u}.conv"
            # the walk feeds the conv the level's transformer result where the level has one, else its last block's
            blocks = sorted((n for n in names if re.fullmatch(rf"up{u}\.block\d+", n)), key=lambda n: int(n.rsplit("block", 1)[1]))
            fed = f"up{u}.attn" if f"up{u}.attn" in names else blocks[-1]
            assert names.index(fed) < names.index(name)
            case[name] = {"fed": fed, "x": hd.tap(fed, B, dev).cpu(), "y": hd.tap(name, B, dev).cpu(),
                          "stats": hd.tap_stats(name, B, dev) if u + 1 < n_up else None}
        rep[":".join(spec)] = case
    torch.save(rep, out_path)
    print(json.dumps({"cases": sorted(rep), "convs": n_up}))


if __name__ == "__main__":
    main()
