"""One case of the 1-D U-Net sweep on the device, as a report (the child process of tests/test_unet1d_sweep_gpu.py's route cases; the
comparison itself is tests/gpu_helpers.py ``sweep_fp32_report`` / ``sweep_bf16_report``, which the module's in-process cases call too).

    ADF_GEMM_TRACE=1 python tests/diag/gpu_unet1d_routes_report.py <route case>        # last stdout line: the report as JSON; stderr: [adf gemm] lines

fp32: the output and every recorded tensor, unsubsampled, against oracle/unet1d.py run in float64 (max |a - b| / max |b|).
f32x3: the same ("free"), and every recorded tensor teacher-forced against the split-bf16 oracle (relative L2; ``sweep_x3_report``).
bf16: every stored tensor teacher-forced against the bf16-storage oracle (relative L2), the output against the oracle's forced output."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import audiodiffuser_amd as A                      # noqa: E402
from audiodiffuser_amd.config import UNet1dConfig   # noqa: E402
from audiodiffuser_amd.weights import generate_weights   # noqa: E402
from oracle import unet1d_sweep as SW               # noqa: E402
import gpu_helpers as H                             # noqa: E402


def _cfg(**kw):
    cfg = UNet1dConfig(attentions=[False] * (len(kw["multipliers"]) - 1), use_attention_bottleneck=False, **kw)
    cfg.out_channels = cfg.in_channels
    return cfg


# route case -> (configuration, (B, L), weight seed, compute mode); the gates that place them are spelled out in tests/test_unet1d_sweep_gpu.py
ROUTE_CASES = {}
for _dt in ("fp32", "bf16"):
    ROUTE_CASES["ws192_" + _dt] = (_cfg(channels=32, num_filters=32, multipliers=[1, 6, 6, 6], factors=[2, 8, 2], num_blocks=[1, 1, 1]), (16, 8192), 51, _dt)
ROUTE_CASES["ws192_f32x3"] = ROUTE_CASES["ws192_fp32"][:3] + ("f32x3",)
for _b in (17, 9):
    ROUTE_CASES["rbx3_small_b%d_f32x3" % _b] = (_cfg(channels=64, num_filters=64, multipliers=[1, 2, 4], factors=[2, 2], num_blocks=[1, 1]), (_b, 2048), 54, "f32x3")
ROUTE_CASES["pp384_bf16"] = (_cfg(channels=64, num_filters=64, multipliers=[1, 6], factors=[2], num_blocks=[1]), (44, 512), 52, "bf16")
ROUTE_CASES["pp128g1_bf16"] = (_cfg(channels=64, num_filters=64, multipliers=[1, 2], factors=[2], num_blocks=[1], resnet_groups=1), (32, 2048), 53, "bf16")


def main():
    case = sys.argv[1]
    cfg, shape, seed, dtype = ROUTE_CASES[case]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    w = generate_weights(cfg, seed=seed)
    x, t = SW.inputs(cfg, shape, seed)
    net = H.sweep_make(cfg, w, dtype)
    if dtype == "bf16":
        rep = H.sweep_bf16_report(cfg, w, x, t, net)
    elif dtype == "f32x3":
        rep = H.sweep_x3_report(cfg, w, {k: v.double() for k, v in w.items()}, x, t, net)
    else:
        rep = H.sweep_fp32_report(cfg, w, {k: v.double() for k, v in w.items()}, x, t, net)
    rep.pop("y"); rep.pop("got")
    rep.update(case=case, dtype=dtype, shape=list(shape))
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
