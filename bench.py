#!/usr/bin/env python
"""Headline benchmark: audio samples / second for full EDM sampler runs on MI355X.

A "step" is ONE complete sampler run over one batch of synthetic noise that is already resident in HBM.  Default
workload = BASELINE.json configs[1]: UNet1d 64 ch, 16384-sample waveforms, KarrasSchedule N=50 Heun (99 denoiser
evaluations), batch 64 per GPU, bf16 storage / fp32 accumulate.  `--config c3 --sampler dpm` is configs[2]
(attention from the 16x level, DPM-Solver++ multistep order 3, 50 sigmas = 49 evaluations, 64 waveforms per GPU).
With N > 1 GPUs the batch is sharded (weak scaling: --batch waveforms per rank) and the only exchange is one
all-gather of the finished waveforms (audiodiffuser_amd/distributed.py).

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts the N ranks itself
(torch.distributed.run, one process per GPU, before this process touches a GPU); under torchrun it is one rank.

Prints ONE JSON line on rank 0 (metric, value, unit, higher_is_better, dtype, ms_per_step, ...).  A plain run sets up, warms up, times the
--steps sampler runs, writes the last one's waveforms if --dump-outputs DIR is given, and prints the line.  `--full` adds
the measurements below, each of which takes runs of its own (the --no-* options drop single ones of them):
  roofline     -- the dominant kernel (fused resblock implicit GEMM): algorithmic bytes / flops per launch
                  over its HIP-event-timed launch duration, replayed exactly as the network pass issues it on rotating
                  operand copies (adf_bench_resblock); `traffic` = HBM bytes per launch from two rocprofv3 --pmc passes
                  (FETCH_SIZE, WRITE_SIZE) of `bench.py --roofline-only` run as child processes, or null
  cpu_baseline -- the CPU oracle (a port of the reference PyTorch path) timed on the host cores: the same workload on a
                  bounded sample (`value`), and SURVEY.md 8(d)'s protocol on BASELINE configs[0] (`config1`)
  bf16_vs_fp32 -- deviation of the timed (bf16) run's first waveforms from the fp32 (parity-grade) mode on the same noise
  other_workloads -- the configs[2] / [3] / [4] lines as child runs (default workload only)
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = {"c1": "BASELINE configs[0] network", "c2": "BASELINE configs[1]", "c3": "BASELINE configs[2]", "tiny": "unit-test network",
             "c5": "BASELINE configs[4]", "c4": "BASELINE configs[3]"}
# per-config defaults of --batch (per GPU), --length, --num-steps: c5 = 1024 waveforms over 8 GPUs, 22050 samples, 6-step sampler
# c4 = one 80 x 256 mel block per sample (length = 80 * 256 bins), 35-step stochastic EDM sampler; BASELINE gives no batch: 64 as configs[1]
DEFAULTS = {"c5": (128, 22050, 6), "c4": (64, 80 * 256, 35)}
C4_SHAPE = (80, 256)
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3, "f32x3": 2500.0 / 3}      # f32x3: three bf16 MFMAs per product
SURVEY_REFERENCE_CONFIG1_S = 3.81    # the reference itself, config 1, in the build container (8 threads)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="c2", choices=["c1", "c2", "c3", "tiny", "c5", "c4"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "f32x3"])
    ap.add_argument("--batch", type=int, default=None, help="waveforms per GPU (default 64; c5: 128)")
    ap.add_argument("--length", type=int, default=None, help="samples per waveform (default 16384; c5: 22050)")
    ap.add_argument("--num-steps", type=int, default=None, help="sigma schedule length N (Heun => 2N-1 NFE; default 50; c5: 6)")
    ap.add_argument("--sampler", default=None, choices=["heun", "dpm", "churn"], help="default: heun; dpm for --config c3; churn (the stochastic EDM sampler of configs[3]) for c4")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the line's own steps, also measure the roofline, PMC traffic, other precisions and workloads and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's waveforms as DIR/samples.npy (float32; a seeded sample of rows beyond 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="skip the rocprofv3 --pmc child passes (roofline.traffic = null)")
    ap.add_argument("--no-precision-check", action="store_true", help="skip the fp32 run behind bf16_vs_fp32")
    ap.add_argument("--no-other-workloads", action="store_true", help="skip the child runs of configs[2] / [3] / [4] appended as other_workloads")
    ap.add_argument("--mock-device", action="store_true",
                    help="CPU rehearsal of the rank / reporting path (gloo, a stand-in step instead of the HIP sampler): tests only, value is null")
    ap.add_argument("--roofline-iters", type=int, default=60)
    ap.add_argument("--roofline-only", action="store_true", help="only replay the resblock kernels (for rocprofv3)")
    ap.add_argument("--roofline-level", type=int, default=-1, help="with --roofline-only: replay this resblock only")
    ap.add_argument("--roofline-conv", type=int, default=0, choices=[0, 1, 2], help="with --roofline-level: only conv1 / conv2 of the block")
    a = ap.parse_args(argv)
    db, dl, dn = DEFAULTS.get(a.config, (64, 16384, 50))
    a.batch = db if a.batch is None else a.batch
    a.length = dl if a.length is None else a.length
    a.num_steps = dn if a.num_steps is None else a.num_steps
    if a.sampler is None:
        a.sampler = "dpm" if a.config == "c3" else ("churn" if a.config == "c4" else "heun")
    return a


# ---------------------------------------------------------------------------------------------------- launcher
def launch_ranks(n: int, argv) -> int:
    """Start n ranks of this script (one per GPU) with torch.distributed.run and return its exit code.  Called BEFORE
    anything in this process touches a GPU (torch.cuda.device_count() does not initialise it)."""
    from audiodiffuser_amd.distributed import launch_ranks as _launch
    return _launch(os.path.abspath(__file__), n, argv)


# ---------------------------------------------------------------------------------------------------- roofline
def replay_rows(hd, batch, length, iters, device, only_level=-1, only_conv=0):
    """HIP-event replay of the resblock GEMM launches of the last forward (adf_bench_resblock / adf_bench_layer)."""
    import torch
    lib = hd.lib
    stream = torch.cuda.current_stream(device).cuda_stream
    if only_level >= 0 and only_conv in (1, 2):
        ms, by, fl, cp = C.c_float(), C.c_double(), C.c_double(), C.c_int()
        rc = lib.adf_bench_layer(hd.h, batch, length, only_level, only_conv, iters, C.byref(ms), C.byref(by), C.byref(fl), C.byref(cp),
                                 C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError("adf_bench_layer: " + lib.adf_last_error(hd.h).decode())
        return [{"resblock": only_level, "kernel": only_conv, "ms": ms.value, "bytes": by.value, "flops": fl.value, "copies": cp.value}]
    rows, idx = [], 0 if only_level < 0 else only_level
    while True:
        ms1, ms2 = C.c_float(), C.c_float()
        b1, b2, f1, f2 = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        rc = lib.adf_bench_resblock(hd.h, batch, length, idx, iters, C.byref(ms1), C.byref(ms2), C.byref(b1), C.byref(b2),
                                    C.byref(f1), C.byref(f2), C.c_void_p(stream))
        if rc != 0:
            msg = lib.adf_last_error(hd.h).decode()
            if "out of range" in msg and only_level < 0:
                break
            raise RuntimeError("adf_bench_resblock: " + msg)
        for k, (ms, by, fl) in enumerate(((ms1.value, b1.value, f1.value), (ms2.value, b2.value, f2.value))):
            if ms > 0:
                rows.append({"resblock": idx, "kernel": k + 1, "ms": ms, "bytes": by, "flops": fl})
        if only_level >= 0:
            break
        idx += 1
    return rows


def roofline(hd, batch, length, dtype, iters, device):
    """Replay every resblock's two GEMM launches (as the network pass issues them, rotating operand copies) with HIP events
    on the launch stream and report the launch that dominates the pass (largest time)."""
    # three batches of `iters` launches per layer, per launch the fastest batch mean: single batches of one layer in a loop sometimes run in a slower
    # power state (the same launch 80 and 94 us in back-to-back bench runs on one box, with the step time unchanged); the in-pass durations of the
    # rocprofv3 traces under profiles/ agree with the fast figure
    rows = replay_rows(hd, batch, length, iters, device)
    if not rows:
        return None
    for r in rows:
        r["batch_ms"] = [r["ms"]]
    for _ in range(2):
        again = {(r["resblock"], r["kernel"]): r["ms"] for r in replay_rows(hd, batch, length, iters, device)}
        for r in rows:
            r["batch_ms"].append(again.get((r["resblock"], r["kernel"]), r["ms"]))
    # round 4 (ADVICE r3 / VERDICT r3 item 1): the figure is quoted on the MEDIAN of the three batch means; best and worst are carried beside it
    # (`ms_per_launch_batches`), so that lines of different rounds can be compared whatever statistic they quoted (r01 / r02: one batch, r03: the best)
    for r in rows:
        b = sorted(r["batch_ms"])
        r["ms_best"], r["ms"], r["ms_worst"] = b[0], b[len(b) // 2], b[-1]
    # The launches of the two biggest blocks (conv1: K = 768 over the concat, 201.5 MB; conv2: K = 640 with the 1x1 residual segment, 268.6 MB) sit
    # within 2-3 % of each other in time and trade places from run to run: among the launches within 5 % of the longest one the figure is quoted on the
    # one with the LOWEST bytes / time (the conservative one, and the launch rounds 1-2 reported); the near ties are listed beside it.
    t_max = max(r["ms"] for r in rows)
    ties = [r for r in rows if r["ms"] >= 0.95 * t_max]
    dom = min(ties, key=lambda r: r["bytes"] / r["ms"])
    ai = dom["flops"] / dom["bytes"]
    ridge = MFMA_PEAK_TFLOPS[dtype] * 1e12 / (HBM_PEAK_GBS * 1e9)
    gbs = dom["bytes"] / (dom["ms"] * 1e-3) / 1e9
    tfs = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
    total_ms = sum(r["ms"] for r in rows)
    all_bytes = sum(r["bytes"] for r in rows)
    all_flops = sum(r["flops"] for r in rows)
    # SURVEY.md 8(d) defines the figure per RESBLOCK (conv1 + conv2 launches of one block): report the dominant launch's block too
    pair = [r for r in rows if r["resblock"] == dom["resblock"]]
    pair_ms, pair_bytes = sum(r["ms"] for r in pair), sum(r["bytes"] for r in pair)
    out = {
        "bound": "hbm" if ai < ridge else "mfma",
        "kernel": f"fused resblock implicit-GEMM (resblock {dom['resblock']} conv{dom['kernel']})",
        "definition": "dominant single launch (of the launches within 5 % of the longest: the one with the lowest bytes / time): SURVEY.md 8(d) "
                      "algorithmic bytes of that conv / its mean duration (MEDIAN of three batches of launches; best and worst in ms_per_launch_batches), HIP events, "
                      "in-pass launch form (GroupNorm table + statistics epilogue on), operands rotated over >= 320 MiB",
        "level": dom["resblock"], "conv": dom["kernel"],
        "ms_per_launch": dom["ms"],
        "ms_per_launch_batches": {"best": dom["ms_best"], "median": dom["ms"], "worst": dom["ms_worst"]},
        "frac_best": dom["bytes"] / (dom["ms_best"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
        "algorithmic_bytes": dom["bytes"], "algorithmic_flops": dom["flops"], "flop_per_byte": ai, "ridge_flop_per_byte": ridge,
        "hbm_GBps": gbs, "hbm_frac": gbs / HBM_PEAK_GBS,
        "mfma_TFLOPs": tfs, "mfma_frac": tfs / MFMA_PEAK_TFLOPS[dtype],
        "resblock_pair": {"ms": pair_ms, "algorithmic_bytes": pair_bytes, "hbm_GBps": pair_bytes / (pair_ms * 1e-3) / 1e9,
                          "hbm_frac": pair_bytes / (pair_ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
        "all_resblocks": {"ms": total_ms, "hbm_GBps": all_bytes / (total_ms * 1e-3) / 1e9,
                          "hbm_frac": all_bytes / (total_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          "mfma_TFLOPs": all_flops / (total_ms * 1e-3) / 1e12},
        "traffic": None,
        "near_ties": [{"resblock": r["resblock"], "conv": r["kernel"], "ms": r["ms"], "algorithmic_bytes": r["bytes"],
                       "hbm_frac": r["bytes"] / (r["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS} for r in sorted(ties, key=lambda r: -r["ms"])],
    }
    if os.environ.get("ADF_BENCH_VERBOSE"):
        out["rows"] = rows
    if out["bound"] == "hbm":
        out.update({"achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS})
    else:
        out.update({"achieved": tfs, "peak": MFMA_PEAK_TFLOPS[dtype], "unit": "TFLOP/s", "frac": tfs / MFMA_PEAK_TFLOPS[dtype]})
    return out


def wavenet_rows(hd, batch, length, iters, device, layers):
    """HIP-event replay of residual-layer launches of the last WaveNetNoise pass (adf_bench_wavenet_layer)."""
    import torch
    stream = torch.cuda.current_stream(device).cuda_stream
    rows = []
    for n in layers:
        ms, by, fl = C.c_float(), C.c_double(), C.c_double()
        rc = hd.lib.adf_bench_wavenet_layer(hd.h, batch, length, n, iters, C.byref(ms), C.byref(by), C.byref(fl), C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError("adf_bench_wavenet_layer: " + hd.lib.adf_last_error(hd.h).decode())
        rows.append({"layer": n, "ms": ms.value, "bytes": by.value, "flops": fl.value})
    return rows


def wavenet_roofline(hd, cfg, batch, length, dtype, iters, device):
    """The residual-layer kernel (36 of the 40 launches of a pass, > 99 % of its flops): dilations 1 / 32 / 2048 and the last
    layer replayed with HIP events; the slowest is reported against the roofline that bounds it."""
    layers = sorted({0, min(5, cfg.residual_layers - 1), min(cfg.dilation_cycle - 1, cfg.residual_layers - 1), cfg.residual_layers - 1})
    rows = wavenet_rows(hd, batch, length, iters, device, layers)
    mid = [r for r in rows if 0 < r["layer"] < cfg.residual_layers - 1] or rows
    dom = max(mid, key=lambda r: r["ms"])
    ai = dom["flops"] / dom["bytes"]
    ridge = MFMA_PEAK_TFLOPS[dtype] * 1e12 / (HBM_PEAK_GBS * 1e9)
    gbs = dom["bytes"] / (dom["ms"] * 1e-3) / 1e9
    tfs = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
    out = {"bound": "hbm" if ai < ridge else "mfma", "kernel": f"fused WaveNet residual layer (layer {dom['layer']}, dilation {cfg.dilation(dom['layer'])})",
           "definition": "slowest of the replayed residual-layer launches: algorithmic bytes (y read + y_next write in the storage type, fp32 skip "
                         "read-modify-write, both weight matrices once) and flops (K = 3C and K = C GEMMs onto 2C columns) / mean duration, HIP events",
           "level": dom["layer"], "conv": 0, "ms_per_launch": dom["ms"], "algorithmic_bytes": dom["bytes"], "algorithmic_flops": dom["flops"],
           "flop_per_byte": ai, "ridge_flop_per_byte": ridge, "hbm_GBps": gbs, "hbm_frac": gbs / HBM_PEAK_GBS, "mfma_TFLOPs": tfs,
           "mfma_frac": tfs / MFMA_PEAK_TFLOPS[dtype], "rows": rows, "traffic": None}
    if out["bound"] == "hbm":
        out.update({"achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS})
    else:
        out.update({"achieved": tfs, "peak": MFMA_PEAK_TFLOPS[dtype], "unit": "TFLOP/s", "frac": tfs / MFMA_PEAK_TFLOPS[dtype]})
    return out


def adm_conv_flops(cfg, batch, H, W):
    """Multiply-add flops x 2 of every convolution / 1x1 projection / attention contraction of one UNetModel pass (from the structure)."""
    from audiodiffuser_amd.adm_config import structure
    s = structure(cfg)
    fl = 0.0
    hw = {0: (H, W)}
    def run(layers, h, w):
        nonlocal fl
        for l in layers:
            if l.kind == "conv":
                fl += 2.0 * h * w * 9 * l.cin * l.cout
            elif l.kind == "res":
                fl += 2.0 * h * w * (9 * l.cin * l.cout + 9 * l.cout * l.cout + (l.cin * l.cout if l.cin != l.cout else 0))
            elif l.kind == "attn":
                fl += 2.0 * h * w * (3 * l.cin * l.cin + l.cin * l.cin) + 4.0 * (h * w) ** 2 * l.cin
            elif l.kind == "down":
                h, w = h // 2, w // 2
                fl += 2.0 * h * w * 9 * l.cin * l.cout
            elif l.kind == "up":
                h, w = h * 2, w * 2
                fl += 2.0 * h * w * 9 * l.cin * l.cout
        return h, w
    h, w = H, W
    for blk in s.input_blocks:
        h, w = run(blk, h, w)
    h, w = run(s.middle, h, w)
    for blk in s.output_blocks:
        h, w = run(blk, h, w)
    fl += 2.0 * h * w * 9 * s.input_ch * cfg.out_channels
    return fl * batch


def adm_pass_bytes(cfg, batch, H, W, esize=2):
    """Algorithmic HBM bytes of one UNetModel pass: every conv / projection launch reads its input tensor(s) once, writes its output once (a
    residual operand is one more read) and reads its weights once; GroupNorm tables and statistics are negligible.  Same walk as adm_conv_flops."""
    from audiodiffuser_amd.adm_config import structure
    s = structure(cfg)
    by = 0.0
    def conv(h_in, w_in, cin, h, w, cout, taps, res=False):
        return (h_in * w_in * cin + h * w * cout * (2 if res else 1)) * esize * batch + taps * cin * cout * esize
    def run(layers, h, w):
        nonlocal by
        for l in layers:
            if l.kind == "conv":
                by += conv(h, w, l.cin, h, w, l.cout, 9)
            elif l.kind == "res":
                by += conv(h, w, l.cin, h, w, l.cout, 9) + conv(h, w, l.cout, h, w, l.cout, 9, res=True)
                if l.cin != l.cout:
                    by += conv(h, w, l.cin, h, w, l.cout, 1)
            elif l.kind == "attn":
                c = l.cin
                by += 2 * h * w * c * esize * batch                          # GroupNorm applied (xn)
                by += conv(h, w, c, h, w, 3 * c, 1) + 4 * h * w * c * esize * batch + conv(h, w, c, h, w, c, 1, res=True)
            elif l.kind == "down":
                by += conv(h, w, l.cin, h // 2, w // 2, l.cout, 9)
                h, w = h // 2, w // 2
            elif l.kind == "up":
                by += conv(h, w, l.cin, h * 2, w * 2, l.cout, 9)
                h, w = h * 2, w * 2
        return h, w
    h, w = H, W
    by += (H * W * cfg.in_channels * 4 + H * W * s.input_ch * esize) * batch      # first conv: fp32 planes in, channels-last out
    for blk in s.input_blocks:
        h, w = run([l for l in blk if not (l.kind == "conv" and l.cin == cfg.in_channels)], h, w)
    h, w = run(s.middle, h, w)
    for blk in s.output_blocks:
        h, w = run(blk, h, w)
    by += (h * w * s.input_ch * esize + 2 * h * w * cfg.out_channels * 4) * batch   # last conv: reads h, reads x_noisy, writes fp32 planes
    return by


def adm_pass_row(net, cfg, x, device, iters):
    """One eager network pass timed with events on the launch stream (the pass launches on torch's current stream)."""
    import torch
    t = torch.zeros(x.shape[0], device=device)
    net(x, t)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = max(2, min(iters, 5))
    e0.record()
    for _ in range(n):
        net(x, t)
    e1.record()
    torch.cuda.synchronize()
    return {"pass_ms": e0.elapsed_time(e1) / n, "flops": adm_conv_flops(cfg, x.shape[0], x.shape[2], x.shape[3]),
            "bytes": adm_pass_bytes(cfg, x.shape[0], x.shape[2], x.shape[3], 2 if str(getattr(net, "compute_dtype", "bf16")) == "bf16" else 4)}


def adm_roofline(net, cfg, x, device, dtype):
    """The GEMM flops of one network pass (3x3 / 1x1 convs, attention) over the pass time (per-layer figures: tools/adm_layer_table.py)."""
    row = adm_pass_row(net, cfg, x, device, 5)
    tfs = row["flops"] / (row["pass_ms"] * 1e-3) / 1e12
    return {"bound": "mfma", "kernel": "conv2d_tile_kernel / conv2d_gemm_kernel (implicit GEMM over channels-last pixels), whole network pass",
            "definition": "multiply-add flops x 2 of every conv / projection / attention contraction of one UNetModel pass / the eager pass time (events on the launch "
                          "stream): a per-pass figure, not a single launch (per-layer table: profiles/r02_adm_layer_table.txt)",
            "level": -1, "conv": 0, "pass_ms": row["pass_ms"], "algorithmic_flops": row["flops"], "algorithmic_bytes": row["bytes"],
            "hbm_GBps": row["bytes"] / (row["pass_ms"] * 1e-3) / 1e9, "mfma_TFLOPs": tfs, "achieved": tfs,
            "peak": MFMA_PEAK_TFLOPS[dtype], "unit": "TFLOP/s", "frac": tfs / MFMA_PEAK_TFLOPS[dtype], "traffic": None}


def pmc_traffic(a, level: int, conv: int):
    """HBM bytes per launch of the dominant kernel from the PMC counters, measured now: two child runs of
    `rocprofv3 --kernel-trace --pmc <counter> -- python3 bench.py --roofline-only --roofline-level K` (FETCH_SIZE and WRITE_SIZE
    need separate passes), read from the counter CSV.  gfx950: FETCH_SIZE counts a 16-B/lane streaming read at half its bytes
    (MI355X_MICROARCH.md, HBM) -> read bytes = 2 * FETCH_SIZE KB; WRITE_SIZE is exact.  Returns (bytes, detail) or (None, why)."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 not found"
    vals = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        tmp = tempfile.mkdtemp(prefix="adf_pmc_", dir=os.environ.get("TMPDIR", "/tmp"))
        cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--roofline-only", "--roofline-level", str(level), "--roofline-conv", str(conv), "--roofline-iters", "4", "--config", a.config, "--dtype", a.dtype,
               "--batch", str(a.batch), "--length", str(a.length), "--no-cpu-baseline", "--no-pmc"]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=tmp, env=dict(os.environ, TMPDIR=tmp))
        except subprocess.TimeoutExpired:
            shutil.rmtree(tmp, ignore_errors=True)
            return None, f"rocprofv3 --pmc {counter} timed out"
        files = glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True)
        if r.returncode != 0 or not files:
            shutil.rmtree(tmp, ignore_errors=True)
            return None, f"rocprofv3 --pmc {counter} failed (rc {r.returncode})"
        per = {}
        if a.config == "c4":
            # per network pass: every dispatch from the last conv2d_in_kernel (the first launch of a pass) to the end of the trace
            allk = {}
            for row in csv.DictReader(open(files[0])):
                if row.get("Counter_Name") == counter:
                    allk.setdefault(int(row["Dispatch_Id"]), [row["Kernel_Name"], 0.0])[1] += float(row["Counter_Value"])
            shutil.rmtree(tmp, ignore_errors=True)
            ids = sorted(allk)
            starts = [i for i in ids if "conv2d_in_kernel" in allk[i][0]]
            if not starts:
                return None, f"no conv2d_in_kernel dispatch in the {counter} pass"
            vals[counter] = (sum(allk[i][1] for i in ids if i >= starts[-1]), f"all {sum(1 for i in ids if i >= starts[-1])} dispatches of the last network pass")
            continue
        for row in csv.DictReader(open(files[0])):
            if row.get("Counter_Name") != counter or ("wn_layer" if a.config == "c5" else "conv_gemm") not in row.get("Kernel_Name", ""):
                continue
            per.setdefault(row["Dispatch_Id"], [row["Kernel_Name"], 0.0])[1] += float(row["Counter_Value"])
        shutil.rmtree(tmp, ignore_errors=True)
        # the child's last launches are the 4 timed replays of (level, conv): the last 4 conv_gemm dispatches of the trace
        seq = [v for _, v in sorted(per.items(), key=lambda kv: int(kv[0]))]
        if len(seq) < 4:
            return None, f"no matching dispatch in the {counter} pass"
        if a.config == "c5":
            # round 4: the MEAN over the residual layers of one network pass (the child's eager pass: its first `residual_layers` dispatches), not the one
            # replayed layer: a layer's traffic depends on its dilation and position (profiles/r04_c5_traffic_per_layer.txt: 9.0 GB at dilation 1-64 to
            # 10.6 GB at dilation 2048 -- three disjoint windows, y is read twice from memory -- against 8.67 GB algorithmic), and the layers the replay
            # picks as "slowest" trade places from run to run: that was the 9.6-11.1 GB spread of the round-3 lines
            import audiodiffuser_amd as A_
            nl = A_.config_c5().residual_layers
            if len(seq) < nl:
                return None, f"fewer than {nl} layer dispatches in the {counter} pass"
            first = [v for _, v in seq[:nl]]
            vals[counter] = (sum(first) / nl, f"mean over the {nl} residual layers of one pass (min {min(first):.0f} KB, max {max(first):.0f} KB)")
            continue
        tail = seq[-4:]
        if len({nm for nm, _ in tail}) != 1:
            return None, f"the {counter} pass ended on mixed kernels"
        vals[counter] = (statistics.median(v for _, v in tail), tail[-1][0])
    fetch_kb, write_kb = vals["FETCH_SIZE"][0], vals["WRITE_SIZE"][0]
    return (2.0 * fetch_kb + write_kb) * 1024.0, {"FETCH_SIZE_KB": fetch_kb, "WRITE_SIZE_KB": write_kb, "kernel": vals["FETCH_SIZE"][1].split("(")[0],
                                                   "formula": "(2 * FETCH_SIZE + WRITE_SIZE) * 1024 (gfx950 FETCH_SIZE half-count correction)"}


# ---------------------------------------------------------------------------------------------------- CPU baseline
def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def physical_cores():
    try:
        seen = set()
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    seen.add((phys, core))
                phys = core = None
        avail = len(os.sched_getaffinity(0))
        return max(1, min(len(seen), avail)) if seen else avail
    except OSError:
        return os.cpu_count() or 1


def cpu_baseline(cfg, length, nfe_per_waveform, gpu_value):
    """The CPU oracle (port of the reference PyTorch path, pinned against the reference) on the host cores.
    (1) the SAME workload as the GPU line on a bounded sample: the denoiser of this network at batch 2, 1 warm-up + 3 x 3
        evaluations, median per-evaluation time, scaled to the sampler's evaluation count;
    (2) SURVEY.md 8(d) / BASELINE.md section 3: BASELINE configs[0] exactly (16 ch, B = 4, N = 18 Heun = 35 NFE, fp32, full
        sampler via oracle.samplers.edm_sampler), k = all physical cores and k = 8 threads, 1 warm-up + 3 runs, median."""
    import torch
    import audiodiffuser_amd as A
    from audiodiffuser_amd.weights import generate_weights, generate_noise
    from oracle import edm as E, samplers as S
    cores = physical_cores()
    prev = torch.get_num_threads()
    out = {"unit": "mel-bins/s" if isinstance(cfg, A.ADMConfig) else "audio-samples/s", "kind": "port", "cpu_model": cpu_model(), "physical_cores": cores}
    try:
        if isinstance(cfg, A.ADMConfig):
            from audiodiffuser_amd.adm_config import generate_weights as generate_adm_weights
            from oracle import unet2d_oai as OA
            w = generate_adm_weights(cfg, seed=0)
            fn = lambda xx, sigma=None, sigmas=None: E.denoise(lambda xi, ti, **kw: OA.unet2d_forward(w, cfg, xi, ti), xx, 0.2, sigma=sigma, sigmas=sigmas)
        elif isinstance(cfg, A.WaveNetConfig):
            from audiodiffuser_amd.weights import generate_wavenet_weights
            from oracle import wavenet as OW
            w = generate_wavenet_weights(cfg, seed=0)
            wnet = OW.wavenet_net(w, cfg)
            fn = lambda xx, sigma=None, sigmas=None: E.denoise(wnet, xx, 0.2, sigma=sigma, sigmas=sigmas)
        else:
            w = generate_weights(cfg, seed=0)
            fn = E.make_denoiser(w, cfg, 0.2)
        heavy = isinstance(cfg, (A.WaveNetConfig, A.ADMConfig))       # 0.83 / 0.2 TFLOP per sample and evaluation: a smaller sample keeps the leg bounded
        b = 1 if heavy else 2
        x = generate_noise(0, b, length) * 3.0
        if isinstance(cfg, A.ADMConfig):
            x = x.reshape(b, 1, *C4_SHAPE)
        reps = []
        with torch.no_grad():
            # torch's CPU convolutions do not scale to every core of a large host (oversubscription): give the CPU its best
            # thread count -- one evaluation at each candidate after a warm-up, keep the fastest
            scan = {}
            for k in sorted({min(c, cores) for c in ((16, 64) if heavy else (8, 16, 32, 64, cores))}):
                torch.set_num_threads(k)
                fn(x, sigma=torch.tensor(3.0))
                t0 = time.perf_counter()
                fn(x, sigma=torch.tensor(2.0))
                scan[k] = time.perf_counter() - t0
            best_k = min(scan, key=scan.get)
            torch.set_num_threads(best_k)
            out["thread_scan_s_per_evaluation"] = scan
            fn(x, sigma=torch.tensor(3.0))           # warm-up
            per = 1 if heavy else 3
            for rep in range(3):
                t0 = time.perf_counter()
                for i in range(per):
                    fn(x, sigma=torch.tensor(3.0 / (3 * rep + i + 1)))
                reps.append((time.perf_counter() - t0) / per)
        dt = statistics.median(reps)
        wps = b / (dt * nfe_per_waveform)
        out.update({"value": wps * length, "waveforms_per_s": wps, "cores": best_k,
                    "sample": f"same network and sampler as the GPU line: oracle denoiser at batch {b}, 1 warm-up + 3 x {per} evaluations, median "
                              f"{dt:.3f} s per evaluation (repeats {', '.join('%.3f' % r for r in reps)}), scaled to {nfe_per_waveform} evaluations per waveform"})
        del w, fn
        if isinstance(cfg, (A.WaveNetConfig, A.ADMConfig)):
            out["gpu_over_cpu_same_workload"] = gpu_value / out["value"] if out.get("value") else None
            return out
        # ---- SURVEY.md 8(d) protocol on configs[0] ------------------------------------------------------------------
        c1 = A.config_c1()
        w1 = generate_weights(c1, seed=0)
        fn1 = E.make_denoiser(w1, c1, 0.2)
        sig = A.KarrasSchedule(0.002, 80.0, 7.0, 18)()
        noise = generate_noise(1234, 4, 16384)
        proto = {"workload": "BASELINE configs[0]: UNet1d 16 ch, B=4, L=16384, KarrasSchedule N=18 Heun (35 NFE), fp32, oracle.samplers.edm_sampler",
                 "reference_in_build_container_s_per_batch_8_threads": SURVEY_REFERENCE_CONFIG1_S}
        # k = 8: 1 warm-up + 3 timed runs, median.  k = all physical cores: ONE timed run after the k = 8 leg has warmed everything
        # (on a 128-core host torch's CPU convolutions run ~18x slower there than at 8-32 threads: 15.6 s per run, which at
        # 1 + 3 runs was 60 % of the whole bench wall time) -- and one run at the thread count the scan above found fastest
        proto["protocol"] = "k = 8: 1 warm-up + 3 timed runs, median; k = all cores and k = the scan's best: 1 timed run each (warm)"
        for k, nrun in [(min(8, cores), 3)] + [(kk, 1) for kk in sorted({cores, best_k} - {min(8, cores)})]:
            torch.set_num_threads(k)
            runs = []
            with torch.no_grad():
                for i in range(nrun + (1 if nrun > 1 else 0)):
                    t0 = time.perf_counter()
                    S.edm_sampler(noise, fn1, sig, 18, s_churn=0.0, s_noise=1.0)
                    if i or nrun == 1:
                        runs.append(time.perf_counter() - t0)
            med = statistics.median(runs)
            proto[f"threads_{k}"] = {"s_per_batch_median": med, "runs_s": runs, "waveforms_per_s": 4.0 / med, "audio_samples_per_s": 4.0 * 16384 / med}
        out["config1"] = proto
    finally:
        torch.set_num_threads(prev)
    out["gpu_over_cpu_same_workload"] = gpu_value / out["value"] if out.get("value") else None
    return out


def gpu_config1(device):
    """The HIP path on BASELINE configs[0] exactly (fp32 parity mode, B = 4, N = 18 Heun): waveforms / s, for the ratio against
    cpu_baseline.config1 on the identical workload."""
    import torch
    import audiodiffuser_amd as A
    from audiodiffuser_amd.weights import generate_weights, generate_noise
    cfg = A.config_c1()
    net = A.UNet1dBase.from_config(cfg, compute_dtype="fp32")
    net.load_state_dict(generate_weights(cfg, seed=0))
    net = net.to(device)
    diff = A.EluDiffusion(sigma_data=0.2)
    sig = A.KarrasSchedule(0.002, 80.0, 7.0, 18)()
    smp = A.EDMSampler(s_churn=0.0, s_noise=1.0, num_steps=18, use_heun=True)
    noise = generate_noise(1234, 4, 16384).to(device)
    smp(noise, fn=diff.denoise_fn, net=net, sigmas=sig)
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        smp(noise, fn=diff.denoise_fn, net=net, sigmas=sig)
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    med = statistics.median(runs)
    return {"s_per_batch_median": med, "waveforms_per_s": 4.0 / med, "audio_samples_per_s": 4.0 * 16384 / med, "dtype": "fp32"}


def other_workloads(a):
    """The other BASELINE configs as child runs of this script, appended to the default line so that the driver's record
    carries them: configs[2] (`--config c3 --sampler dpm`), configs[3] (`--config c4`), configs[4] (`--config c5`), each 1 warm-up
    + 2 timed sampler runs at its per-GPU batch, with its own roofline object.  Child processes: each network's workspace is
    released with its process, and a failure of one cannot take the headline line with it."""
    out = {}
    for name, argv in (("c3", ["--config", "c3", "--sampler", "dpm"]), ("c4", ["--config", "c4"]), ("c5", ["--config", "c5"])):
        # (configs[3] / [4] also collect their PMC traffic -- two rocprofv3 passes each, ~30 s -- so that the figure rides in the driver's line)
        cmd = [sys.executable, os.path.abspath(__file__)] + argv + ["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"] + (["--no-pmc"] if name == "c3" else []) + [
               "--no-precision-check", "--no-other-workloads", "--roofline-iters", "10"]
        t0 = time.perf_counter()
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                out[name] = {"error": f"rc {r.returncode}: {r.stderr.strip().splitlines()[-1] if r.stderr.strip() else 'no output'}"}
                continue
            j = json.loads(line[-1])
            rf = j.get("roofline") or {}
            out[name] = {"workload": j["config"]["workload"], "metric": j["metric"], "value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"],
                         "steps": j["steps"], "warmup": j["warmup"], "dtype": j["dtype"], "finite": j["finite"], "clamped": j["clamped"],
                         "waveforms_per_s": j["waveforms_per_s"], "nfe_per_waveform": j["nfe_per_waveform"],
                         "roofline": {k: rf.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "ms_per_launch", "pass_ms", "traffic", "algorithmic_bytes")},
                         "wall_s_incl_setup": time.perf_counter() - t0}
        except subprocess.TimeoutExpired:
            out[name] = {"error": "timed out after 300 s"}
    return out


# ---------------------------------------------------------------------------------------------------- main
def make_sampler(A, a):
    if A is None:        # evaluation count only
        return None, (a.num_steps - 1 if a.sampler == "dpm" else 2 * a.num_steps - 1)
    if a.sampler == "churn":     # configs[3]: EDMSampler(s_churn=40, s_noise=1.003, s_tmin=0.05, s_tmax=50) -- 2N - 1 evaluations, one draw per step
        return A.EDMSampler(s_tmin=0.05, s_tmax=50.0, s_churn=40.0, s_noise=1.003, num_steps=a.num_steps, use_heun=True,
                            use_graph=not a.no_graph), 2 * a.num_steps - 1
    if a.sampler == "heun":
        return A.EDMSampler(s_churn=0.0, s_noise=1.0, num_steps=a.num_steps, use_heun=True, use_graph=not a.no_graph), 2 * a.num_steps - 1
    return A.DPMSampler(1.0, order=3, num_steps=a.num_steps, multisteps=True, x0_pred=True, log_time_spacing=False,
                        use_graph=not a.no_graph), a.num_steps - 1


def timed_steps(a, step, fence, world, device, dist):
    """The driver contract's timed region: W untimed warm-up steps, then EXACTLY K steps between two fences (barrier +
    device synchronise), the MAX over ranks of the elapsed time."""
    import torch
    out = None
    for _ in range(a.warmup):
        out = step()
    fence()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step()
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    return out, dt


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, out):
    """`--dump-outputs DIR`: the waveforms (mel blocks for c4) the last timed step returned, as DIR/samples.npy in float32,
    so that two builds can be compared output for output on the same seeded inputs.  Beyond DUMP_LIMIT_BYTES only a fixed,
    seeded sample of rows (whole waveforms, ascending order) is written."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    x = out.detach().float().cpu().numpy()
    if x.nbytes > DUMP_LIMIT_BYTES:
        keep = max(1, DUMP_LIMIT_BYTES // x[0].nbytes)
        x = x[np.sort(np.random.default_rng(0).choice(x.shape[0], keep, replace=False))]
    np.save(os.path.join(path, "samples.npy"), x)


def base_line(a, world, dist, dt, value, metric, unit, workload, nfe, finite, clamped):
    """The fields of the one JSON line that do not depend on the device layer."""
    global_batch = a.batch * world
    return {
        "metric": metric, "value": value, "unit": unit,
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
        "waveforms_per_s": global_batch * a.steps / dt, "nfe_per_waveform": nfe, "finite": finite, "clamped": clamped,
        "rccl_ranks": dist.get_world_size() if world > 1 else 1,
        "config": {"workload": workload, "global_batch": global_batch, "sampler": a.sampler, "num_steps": a.num_steps, "nfe": nfe,
                   "hipgraph": not a.no_graph, "parallelism": f"batch-sharded x{world}, one all-gather"},
    }


def mock_ranks(a, world, rank, dist):
    """`--mock-device`: the rank path of this script (rendezvous, index-keyed noise slices, fences, MAX over ranks, the single
    all-gather, rank 0 printing ONE line) rehearsed on CPU over gloo with a stand-in step -- NOT the HIP sampler, so `value`
    is null and the line says so.  tests/test_dist_gloo.py runs it at world_size 2."""
    import torch
    from audiodiffuser_amd.distributed import rank_noise, gather_samples
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    device = torch.device("cpu")
    global_batch = a.batch * world
    noise = rank_noise(global_batch, a.length, rank, world)

    def step():
        return gather_samples(torch.tanh(noise * 0.5), global_batch)

    def fence():
        if world > 1:
            dist.barrier()

    out, dt = timed_steps(a, step, fence, world, device, dist)
    _, nfe = make_sampler(None, a)
    res = base_line(a, world, dist, dt, None, "mock", "audio-samples/s", "mock device (CPU, gloo): rank / reporting path only", nfe,
                    bool(torch.isfinite(out).all()), float(out.abs().max()) <= 1.0)
    res["mock_device"] = True
    res["gathered_shape"] = list(out.shape)
    res["gathered_checksum"] = float(out.double().sum())
    if rank == 0:
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, out)
        print(json.dumps(res))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    a = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if a.gpus > 1 and env_world is None:
        # not under a launcher: start the ranks (this parent never touches a GPU)
        import torch
        have = a.gpus if a.mock_device else torch.cuda.device_count()
        if have < a.gpus:
            print(f"bench.py: --gpus {a.gpus} but only {have} device(s) visible", file=sys.stderr)
            raise SystemExit(2)
        raise SystemExit(launch_ranks(a.gpus, sys.argv[1:]))
    import torch
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        if rank == 0:
            print(f"bench.py: --gpus {a.gpus} does not match WORLD_SIZE {world}", file=sys.stderr)
        raise SystemExit(2)
    import torch.distributed as dist
    if a.mock_device:
        return mock_ranks(a, world, rank, dist)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the HIP path)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)

    import audiodiffuser_amd as A
    from audiodiffuser_amd.weights import generate_weights
    from audiodiffuser_amd.distributed import rank_noise, gather_samples

    wavenet = a.config == "c5"
    adm = a.config == "c4"
    if adm:
        from audiodiffuser_amd.adm_config import generate_weights as generate_adm_weights
        cfg = A.config_c4()
        make_net = lambda dt: A.UNetModel.from_config(cfg, compute_dtype=dt)
        make_weights = lambda: generate_adm_weights(cfg, seed=0)
    elif wavenet:
        from audiodiffuser_amd.weights import generate_wavenet_weights
        cfg = A.config_c5()
        make_net = lambda dt: A.WaveNetNoise.from_config(cfg, compute_dtype=dt)
        make_weights = lambda: generate_wavenet_weights(cfg, seed=0)
    else:
        cfg = A.PRESETS[a.config]()
        make_net = lambda dt: A.UNet1dBase.from_config(cfg, compute_dtype=dt)
        make_weights = lambda: generate_weights(cfg, seed=0)
    net = make_net(a.dtype)
    net.load_state_dict(make_weights())     # every rank regenerates the same weights
    net = net.to(device)
    diff = A.EluDiffusion(sigma_data=0.2)
    sigmas = A.KarrasSchedule(0.002, 80.0, 7.0, a.num_steps)()
    sampler, nfe = make_sampler(A, a)
    global_batch = a.batch * world
    noise = rank_noise(global_batch, a.length, rank, world).to(device)
    extra = {}
    if adm:
        if a.length != C4_SHAPE[0] * C4_SHAPE[1]:
            raise SystemExit("--config c4 runs on 80 x 256 mel blocks")
        noise = noise.reshape(noise.shape[0], 1, *C4_SHAPE).contiguous()
    if a.sampler == "churn":     # synthetic per-step draws (the plugin would draw them itself; fixed here so every step times the same work)
        g = torch.Generator(device=device).manual_seed(4321 + rank)
        extra["injected_noise"] = torch.randn((a.num_steps,) + tuple(noise.shape), generator=g, device=device)

    def step():
        y = sampler(noise, fn=diff.denoise_fn, net=net, sigmas=sigmas, **extra)
        return gather_samples(y, global_batch)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    hd = net.native(device)
    if a.roofline_only:
        net(noise[:a.batch], torch.zeros(a.batch, device=device))
        torch.cuda.synchronize()
        if adm:
            rows = [adm_pass_row(net, cfg, noise[:a.batch], device, a.roofline_iters)]
        elif wavenet:
            rows = wavenet_rows(hd, a.batch, a.length, a.roofline_iters, device, [max(a.roofline_level, 0)])
        else:
            rows = replay_rows(hd, a.batch, a.length, a.roofline_iters, device, a.roofline_level, a.roofline_conv)
        print(json.dumps({"rows": rows}))
        return

    out, dt = timed_steps(a, step, fence, world, device, dist)
    finite = bool(torch.isfinite(out).all().item())
    clamped = float(out.abs().max()) <= 1.0 + 1e-6
    value = global_batch * a.steps * a.length / dt
    sname = {"heun": "Heun", "dpm": "DPM-Solver multistep", "churn": "stochastic EDM (Heun + churn)"}[a.sampler]
    netname = (f"WaveNetNoise {cfg.residual_layers} x {cfg.residual_channels} ch (unconditional, as the reference class is)" if wavenet else
               (f"ADM UNetModel {cfg.model_channels} ch x {cfg.channel_mult}, 1 x 80 x 256 mel blocks" if adm else f"UNet1d {cfg.channels} ch"))
    res = base_line(a, world, dist, dt, value,
                    (f"mel bins/sec (80 x 256 mel block, {a.num_steps}-step {sname})" if adm else
                     f"audio samples/sec ({a.length}-sample waveform, {a.num_steps}-step {sname})"),
                    "mel-bins/s" if adm else "audio-samples/s",
                    f"{WORKLOADS.get(a.config, a.config)}: {netname} ({a.config}), {a.length}-sample waveforms, KarrasSchedule N={a.num_steps} "
                    f"{a.sampler}, batch {a.batch}/GPU, random-init weights", nfe, finite, clamped)
    res["device_loop"] = hd.counters()            # adf_get_counters: the timed steps were hipGraph replays of adf_sampler_run
    if rank == 0:
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, out)
        if a.full:
            net(noise[:a.batch], torch.zeros(a.batch, device=device))       # one eager pass: the replay reads its operands
            torch.cuda.synchronize()
            if adm:
                rf = adm_roofline(net, cfg, noise[:a.batch], device, a.dtype)
            elif wavenet:
                rf = wavenet_roofline(hd, cfg, a.batch, a.length, a.dtype, min(a.roofline_iters, 10), device)
            else:
                rf = roofline(hd, a.batch, a.length, a.dtype, a.roofline_iters, device)
            res["roofline"] = rf
            if rf and world == 1 and not a.no_pmc:
                traffic, detail = pmc_traffic(a, rf["level"], rf["conv"])
                rf["traffic"] = traffic
                rf["traffic_source"] = detail
            if a.dtype == "bf16" and not a.no_precision_check:
                # the parity-grade (fp32) mode on the same noise: what the storage precision costs the audio.  On the headline
                # workload the fp32 mode runs the WHOLE batch and its second (graph-replayed) run is timed: the throughput of the
                # mode that meets the north star's <= 1e-3 bar (`fp32_mode_ms_per_step`)
                full = a.config == "c2" and world == 1
                nb = a.batch if full else min(2, a.batch)
                net32 = make_net("fp32")
                net32.load_state_dict(make_weights())
                net32 = net32.to(device)
                t1 = time.perf_counter()
                extra32 = {k: v[:, :nb].contiguous() for k, v in extra.items()}       # the same per-step draws as the timed run
                n32 = noise[:nb].contiguous()
                y32 = sampler(n32, fn=diff.denoise_fn, net=net32, sigmas=sigmas, **extra32)
                torch.cuda.synchronize()
                t32 = time.perf_counter() - t1
                if full:
                    t1 = time.perf_counter()
                    y32 = sampler(n32, fn=diff.denoise_fn, net=net32, sigmas=sigmas, **extra32)
                    torch.cuda.synchronize()
                    t32b = time.perf_counter() - t1
                    res["fp32_mode_ms_per_step"] = t32b * 1e3
                    res["fp32_mode"] = {"ms_per_step": t32b * 1e3, "value": nb * a.length / t32b, "unit": res["unit"], "waveforms_per_s": nb / t32b, "batch": nb,
                                        "note": "same workload in the fp32 (parity-grade, exact-fp32 MFMA) mode: one graph-replayed sampler run after the capturing one"}
                    # the split-bf16 mode (ADF_DTYPE_F32X3: fp32 storage, bf16 hi + lo operands, three bf16 MFMAs per product) on the same workload: the
                    # in-tolerance mode meant to be USED (tests/test_gpu_parity.py::test_config2_full_sampler_fp32_vs_oracle holds it to the oracle at 1e-3)
                    netx = make_net("f32x3")
                    netx.load_state_dict(make_weights())
                    netx = netx.to(device)
                    yx = sampler(n32, fn=diff.denoise_fn, net=netx, sigmas=sigmas, **extra32)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    yx = sampler(n32, fn=diff.denoise_fn, net=netx, sigmas=sigmas, **extra32)
                    torch.cuda.synchronize()
                    tx = time.perf_counter() - t1
                    dx = yx.to(torch.float64) - y32.to(torch.float64)
                    res["f32x3_mode_ms_per_step"] = tx * 1e3
                    res["f32x3_mode"] = {"ms_per_step": tx * 1e3, "value": nb * a.length / tx, "unit": res["unit"], "waveforms_per_s": nb / tx, "batch": nb,
                                         "vs_fp32_rel_l2": float(dx.norm() / y32.to(torch.float64).norm()),
                                         "vs_fp32_max_abs_over_max": float(dx.abs().max() / y32.abs().max()),
                                         "note": "same workload in the split-bf16 mode (fp32 storage; every GEMM operand as bf16 hi + lo, 3 bf16 MFMAs per product, fp32 "
                                                 "accumulation); deviation from the exact-fp32 mode over the whole 99-evaluation sampler on all waveforms"}
                    del netx, yx
                y16 = out[:nb].to(torch.float64)
                d = y16 - y32.to(torch.float64)
                res["bf16_vs_fp32"] = {"waveforms": nb, "rel_l2": float(d.norm() / y32.to(torch.float64).norm()),
                                       "max_abs_over_max": float(d.abs().max() / y32.abs().max()),
                                       "note": "bf16 run (the timed one) against the fp32 mode (held to the CPU oracle at <= 1e-3 by tests/test_gpu_parity.py) on the same noise",
                                       "fp32_first_run_s_incl_setup": t32}
                res["bf16_vs_fp32_rel_err"] = res["bf16_vs_fp32"]["rel_l2"]
                del net32, y32
                torch.cuda.empty_cache()
            if world == 1 and a.config == "c2" and not a.no_other_workloads:
                res["other_workloads"] = other_workloads(a)
            if world == 1 and not a.no_cpu_baseline:
                res["cpu_baseline"] = cpu_baseline(cfg, a.length, nfe, value)
                res["gpu_over_cpu"] = res["cpu_baseline"]["gpu_over_cpu_same_workload"]
                if "config1" in res["cpu_baseline"]:
                    g1 = gpu_config1(device)
                    res["cpu_baseline"]["config1"]["gpu_hip_fp32"] = g1
                    best = max(v["waveforms_per_s"] for key, v in res["cpu_baseline"]["config1"].items() if key.startswith("threads_"))
                    res["cpu_baseline"]["config1"]["gpu_over_cpu"] = g1["waveforms_per_s"] / best      # against the FASTER of the two thread counts
        print(json.dumps(res))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
