"""GPU diagnostic, run as a child process by tests/test_wavenet_sweep_gpu.py (ADF_WN_PREFETCH is read once per process): one bf16 WaveNetNoise forward
at a grid large enough for the next-tile L2 prefetch of the 128-position layer kernel to run -- the kernel prefetches only when workgroup
``lin + pf_stride`` exists, and pf_stride is the CU count rounded down to a multiple of 8 -- teacher-forced per layer against the bf16-storage oracle,
with a SHA-256 of the output and of the skip sum: a prefetch moves no value, so the two settings of the switch must hash alike.
Prints one JSON object as its last line.
usage: python tests/diag/gpu_wn_sweep_report.py CHANNELS LAYERS CYCLE BATCH T SEED"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_helpers as R                                    # noqa: E402
from oracle import wavenet_sweep as SW                     # noqa: E402
from audiodiffuser_amd.config import WaveNetConfig         # noqa: E402


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def main():
    ch, nl, cyc, b, tlen, seed = map(int, sys.argv[1:7])
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    cfg = WaveNetConfig(residual_channels=ch, residual_layers=nl, dilation_cycle=cyc)
    w, _ = SW.weights_of(cfg, seed)
    audio, step = SW.inputs(cfg, (b, tlen), seed)
    net = R.wn_make(cfg, w, "bf16")
    rep = R.wn_bf16_report(cfg, w, audio, step, net, free_running=False)
    worst = max(rep["taps"], key=rep["taps"].get)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = -(-tlen // 128)
    out = {"config": [ch, nl, cyc], "shape": [b, tlen], "prefetch": os.environ.get("ADF_WN_PREFETCH", "0"), "cus": cus, "workgroups": tiles * b,
           "names": rep["names"], "missing": rep["missing"], "forced_taps": len(rep["taps"]), "forced_max_rel_l2": rep["taps"][worst], "forced_worst_tap": worst,
           "out_vs_forced_oracle_rel_l2": rep["out"], "sha256_out": sha(rep["y"]), "sha256_skip": sha(rep["got"]["skip"]),
           "device_seconds": rep["device_seconds"], "oracle_seconds": rep["oracle_seconds"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
