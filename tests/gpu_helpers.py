"""Shared helpers of the GPU parity tests: build the HIP net with the deterministic weights, run it,
and compare every recorded activation ("tap") with the CPU oracle on the same inputs."""
from __future__ import annotations

import json
import os
import re
import time

import torch

import audiodiffuser_amd as A
from audiodiffuser_amd.weights import generate_weights, generate_noise
from oracle import unet1d as O
from oracle import unet1d_sweep as SW


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def make_net(cfg, dtype="fp32", flags=0, seed=0):
    w = generate_weights(cfg, seed=seed)
    net = A.UNet1dBase.from_config(cfg, compute_dtype=dtype, native_flags=flags)
    net.load_state_dict(w, strict=True)
    return net.cuda(), w


def golden_inputs(tag: str):
    B, L = (2, 256) if tag == "tiny" else (2, 2048)
    x = generate_noise(0, B, L) * 0.7
    t = torch.tensor([-0.9, 0.35][:B], dtype=torch.float32)
    return x, t


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    return O.rel_l2(a, b)


def tap_errors_bf16(cfg, x, t, flags=0, chained=True, classes=None):
    """The HIP bf16 (throughput) path against the bf16-STORAGE oracle (oracle/unet1d.py, storage="bf16": the fp32
    restatement with a bf16 rounding wherever the device stores bf16), relative L2 per recorded layer.

    forced[name]  -- teacher-forced: the oracle computes each layer from the DEVICE's own output of the previous layer,
                     so the figure is that one layer's deviation (summation order + the roundings it flips);
    chain[name]   -- the oracle runs free from the same input: deviations compound through the net (only if ``chained``).
    Returns (forced, chain, y_device, y_oracle_forced, y_oracle_chain)."""
    net, w = make_net(cfg, "bf16", flags)
    kw = {} if classes is None else {"classes": classes.cuda()}
    y = net(x.cuda(), t.cuda(), **kw)
    torch.cuda.synchronize()
    hd = net.native(torch.device("cuda", torch.cuda.current_device()))
    dev = {name: hd.tap(name, x.shape[0], y.device).cpu() for name in hd.tap_names()}
    y = y.cpu()
    forced, chain = {}, {}
    with torch.no_grad():
        y_f = O.unet1d_forward(w, cfg, x, t, storage="bf16", force=dev, errs=forced, classes=classes)
        forced["out"] = rel_l2(y, y_f)
        y_c = None
        if chained:
            taps_c = {}
            y_c = O.unet1d_forward(w, cfg, x, t, storage="bf16", taps=taps_c, classes=classes)
            chain = {k: rel_l2(v, taps_c[k]) for k, v in dev.items()}
            chain["out"] = rel_l2(y, y_c)
    missing = set(dev) - set(forced)
    assert not missing, f"device taps the oracle does not record: {missing}"
    return forced, chain, y, y_f, y_c


def tap_errors(cfg, x, t, dtype="fp32", flags=0):
    net, w = make_net(cfg, dtype, flags)
    y = net(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    hd = net.native(torch.device("cuda", torch.cuda.current_device()))
    taps_o = {}
    with torch.no_grad():
        y_o = O.unet1d_forward(w, cfg, x, t, taps=taps_o)
    errs = {}
    for name in hd.tap_names():
        got = hd.tap(name, x.shape[0], y.device).cpu()
        errs[name] = rel_err(got, taps_o[name])
    errs["out"] = rel_err(y.cpu(), y_o)
    return errs, y.cpu(), y_o


def tap_errors_x3(cfg, x, t, flags=0):
    """``tap_errors`` in the split-bf16 mode plus, from the SAME device run, every recorded tensor teacher-forced against the split-bf16 oracle
    (storage="f32x3", relative L2; "out" from the device's last tensor).  -> (free-running errors, forced errors)."""
    net, w = make_net(cfg, "f32x3", flags)
    y = net(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    hd = net.native(torch.device("cuda", torch.cuda.current_device()))
    dev = {name: hd.tap(name, x.shape[0], y.device).cpu() for name in hd.tap_names()}
    y = y.cpu()
    taps_o, forced = {}, {}
    with torch.no_grad():
        y_o = O.unet1d_forward(w, cfg, x, t, taps=taps_o)
        y_f = O.unet1d_forward({k: v.double() for k, v in w.items()}, cfg, x.double(), t.double(), storage="f32x3", force=dev, errs=forced)
    errs = {name: rel_err(dev[name], taps_o[name]) for name in dev}
    errs["out"] = rel_err(y, y_o)
    missing = set(dev) - set(forced)
    assert not missing, f"device taps the oracle does not record: {missing}"
    forced["out"] = rel_l2(y, y_f)
    return errs, forced


_C2_LINE = re.compile(r"^\[adf conv2d\] (\S+)\s+B=(\d+) H=(\d+) W=(\d+) cin=(\d+) c0=(\d+) cout=(\d+) taps=(\d+) mode=(\d+) ab=(\d+) act=(\d+) res=(\d+) stats=(\d+)$")
_C2_KEYS = ("B", "H", "W", "cin", "c0", "cout", "taps", "mode", "ab", "act", "res", "stats")


def conv2d_trace_lines(stderr: str):
    """The ``[adf conv2d]`` lines a process started with ADF_C2_TRACE=1 wrote (one per launch_conv2d call), as dicts: "route" plus the integers of
    the line.  A line of that prefix that does not parse is an error, so a change of the trace format cannot silently empty a route census."""
    lines = []
    for l in stderr.splitlines():
        if l.startswith("[adf conv2d]"):
            m = _C2_LINE.match(l.strip())
            assert m, f"unparsed route line: {l!r}"
            lines.append(dict(zip(_C2_KEYS, map(int, m.groups()[1:])), route=m.group(1)))
    return lines


_GEMM_LINE = re.compile(r"^\[adf gemm\] (\S+)\s+B=(\d+) lin=(\d+) mrows=(\d+) n=(\d+)/(\d+) nseg=(\d+) seg0\(c=(\d+)\+(\d+) taps=(\d+) stride=(\d+) off0=(-?\d+) step=(-?\d+) ab=(\d+) act=(\d+)\)"
                        r"(?: seg1\(c=(\d+)\+(\d+) taps=(\d+) ab=(\d+)\))? res=(\d+) gelu=(\d+) scatter=(\d+) out=(\d+)x(\d+) stats=(\d+) flat=(\d+) tile=(\d+)x(\d+)$")
_GEMM_KEYS = ("B", "lin", "mrows", "n", "n_pad", "nseg", "c0", "c1", "taps", "stride", "off0", "step", "ab", "act", "s1c0", "s1c1", "s1taps", "s1ab",
              "res", "gelu", "scatter", "out_rows", "out_c", "stats", "flat", "tm", "tn")


def gemm_trace_lines(stderr: str):
    """The ``[adf gemm]`` lines a process started with ADF_GEMM_TRACE=1 wrote (one per launch_conv_gemm call), as dicts: "route" plus the integers of
    the line (the second segment's are 0 where there is none).  A line of that prefix that does not parse is an error, so a change of the trace format
    cannot silently empty a route census."""
    lines = []
    for l in stderr.splitlines():
        if l.startswith("[adf gemm]"):
            m = _GEMM_LINE.match(l.strip())
            assert m, f"unparsed route line: {l!r}"
            lines.append(dict(zip(_GEMM_KEYS, (int(v) if v is not None else 0 for v in m.groups()[1:])), route=m.group(1)))
    return lines


def assert_gemm_route_trace(case: str, stderr: str):
    """The ``[adf gemm]`` lines of a child process, verbatim and in order, equal those recorded for the same command in tests/golden/gemm_route_traces.json
    (its ``_recorded`` entry names the commit and the command lines): the whole route sequence -- kernel, tile, flat, fused statistics of every launch --
    not a census of subsets.  Routes do not depend on the CU count (only grid sizes do, and the lines do not print them)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_route_traces.json")) as f:
        want = json.load(f)[case]
    got = [l for l in stderr.splitlines() if l.startswith("[adf gemm]")]
    i = next((k for k, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, f"{case}: {len(got)} route lines against {len(want)} recorded; first difference at line {i}: {got[i:i + 1]} against {want[i:i + 1]}"


# ---------------------------------------------------------------- the 1-D constructor and shape sweep (tests/test_unet1d_sweep_gpu.py and its child script)
def sweep_make(cfg, w, dtype, flags=0):
    net = A.UNet1dBase.from_config(cfg, compute_dtype=dtype, native_flags=flags)
    net.load_state_dict(w, strict=True)
    return net.cuda()


SWEEP_TROUBLE = []        # a device run that raised (a refusal of the library, or a fault that surfaces as an ordinary error): the caller starts nothing after it


def sweep_device_run(net, x, t, only=None, classes=None, cond_drop_prob=None):
    """-> (output, {name: recorded tensor}, names in walk order), all on the host.  ``only``: the recorded names to copy back (default: all of them).
    ``classes`` / ``cond_drop_prob``: the labels of a class-conditional net and whether they are dropped (1) or kept (0 or None)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    kw = {} if classes is None else {"classes": classes.cuda(), "cond_drop_prob": cond_drop_prob}
    try:
        with torch.no_grad():
            y = net(x.cuda(), t.cuda(), **kw)
        torch.cuda.synchronize()
    except Exception as e:
        # a refusal of the library ("<launcher>: <reason>") leaves the device as it was; anything else, or a HIP call that failed, may not
        if type(e).__name__ != "AdfError" or any(s in str(e).lower() for s in ("hip", "failed", "illegal", "fault")):
            SWEEP_TROUBLE.append(f"{type(e).__name__}: {e}")
        raise
    hd = net.native(dev)
    names = hd.tap_names()
    assert len(names) == len(set(names))
    got = {k: hd.tap(k, x.shape[0], dev).cpu() for k in names if only is None or k in only}
    if classes is not None:     # the label embedding is handle state, not a tensor of the walk: read under the oracle's name, [B, 4 * channels], first in order
        names = ["class_emb"] + names
        if only is None or "class_emb" in only:
            got["class_emb"] = hd.tap("class_emb", x.shape[0], dev).cpu().squeeze(-1)
    return y.cpu(), got, names


def sweep_fp32_report(cfg, w, w64, x, t, net, oracle=None, classes=None, cond_drop_prob=None):
    """fp32 / f32x3 device run against the float64 oracle.  ``oracle``: a (y64, taps64, dist) triple already computed for these inputs (and labels)."""
    t0 = time.time()
    y, got, names = sweep_device_run(net, x, t, classes=classes, cond_drop_prob=cond_drop_prob)
    t1 = time.time()
    y64, t64, dist = oracle if oracle is not None else SW.float64_run(cfg, w, w64, x, t, classes=classes, cond_drop_prob=cond_drop_prob or 0.0)
    missing = [k for k in names if k not in t64]
    errs = {}
    for k in names:
        if k in t64:
            assert got[k].shape == t64[k].shape, (k, got[k].shape, t64[k].shape)
            errs[k] = SW.rel(got[k], t64[k]) if bool(torch.isfinite(got[k]).all()) else float("inf")
    assert y.shape == y64.shape
    return {"taps": errs, "names": names, "missing": missing, "out": SW.rel(y, y64) if bool(torch.isfinite(y).all()) else float("inf"),
            "oracle_dist": max(dist.values()), "ref_absmax": min(float(v.abs().max()) for v in t64.values()),
            "device_seconds": t1 - t0, "oracle_seconds": time.time() - t1, "y": y, "got": got}


def sweep_x3_report(cfg, w, w64, x, t, net, oracle=None, classes=None, cond_drop_prob=None):
    """f32x3 device run, ONE run held two ways.  ``taps`` / ``out``: every recorded tensor teacher-forced against the split-bf16 oracle (oracle/unet1d.py
    storage="f32x3": relative L2 of one launch on the device's own inputs; the output from the device's last tensor), bar SW.X3_LAUNCH_TOL.  ``free`` /
    ``free_out``: the same tensors free-running against the float64 oracle (max-norm relative), bar F32X3_TOL.  ``oracle``: as in sweep_fp32_report."""
    t0 = time.time()
    y, got, names = sweep_device_run(net, x, t, classes=classes, cond_drop_prob=cond_drop_prob)
    t1 = time.time()
    y64, t64, dist = oracle if oracle is not None else SW.float64_run(cfg, w, w64, x, t, classes=classes, cond_drop_prob=cond_drop_prob or 0.0)
    finite = bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(v).all()) for v in got.values())
    missing = [k for k in names if k not in t64]
    free = {}
    for k in names:
        if k in t64:
            assert got[k].shape == t64[k].shape, (k, got[k].shape, t64[k].shape)
            free[k] = SW.rel(got[k], t64[k]) if finite else float("inf")
    assert y.shape == y64.shape
    forced = {}
    with torch.no_grad():
        y_f = O.unet1d_forward(w64, cfg, x.double(), t.double(), storage="f32x3", force=got, errs=forced, classes=classes,
                               cond_drop_prob=cond_drop_prob or 0.0)
    missing += sorted(set(got) - set(forced))
    if not finite:
        forced = {k: float("inf") for k in forced}
    return {"taps": forced, "names": names, "missing": missing, "out": O.rel_l2(y, y_f) if finite else float("inf"),
            "free": free, "free_out": SW.rel(y, y64) if finite else float("inf"),
            "oracle_dist": max(dist.values()), "ref_absmax": min(float(v.abs().max()) for v in t64.values()),
            "shapes": {k: list(v.shape) for k, v in got.items()},
            "device_seconds": t1 - t0, "oracle_seconds": time.time() - t1, "y": y, "got": got}


def sweep_bf16_report(cfg, w, x, t, net, classes=None, cond_drop_prob=None):
    """bf16 device run, every stored tensor teacher-forced against the bf16-storage oracle."""
    t0 = time.time()
    y, got, names = sweep_device_run(net, x, t, classes=classes, cond_drop_prob=cond_drop_prob)
    t1 = time.time()
    forced = {}
    with torch.no_grad():
        y_f = O.unet1d_forward(w, cfg, x, t, storage="bf16", force=got, errs=forced, classes=classes, cond_drop_prob=cond_drop_prob or 0.0)
    missing = sorted(set(got) - set(forced))
    finite = bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(v).all()) for v in got.values())
    return {"taps": forced, "names": names, "missing": missing, "out": O.rel_l2(y, y_f) if finite else float("inf"),
            "ref_absmax": min(float(v.abs().max()) for v in got.values()), "device_seconds": t1 - t0, "oracle_seconds": time.time() - t1,
            "y": y, "got": got}


# ---------------------------------------------------------------- the WaveNetNoise width and shape sweep (tests/test_wavenet_sweep_gpu.py and its child script)
def wn_make(cfg, w, dtype):
    net = A.WaveNetNoise.from_config(cfg, compute_dtype=dtype)
    net.load_state_dict(w, strict=True)
    return net.cuda()


def wn_fp32_report(cfg, w, w64, audio, step, net, oracle=None):
    """fp32 device run against the float64 oracle: the output and every recorded tensor.  ``oracle``: a (y64, taps64, dist) triple already computed for
    these inputs."""
    from oracle import wavenet_sweep as WS
    t0 = time.time()
    y, got, names = sweep_device_run(net, audio, step)
    t1 = time.time()
    y64, t64, _ = oracle if oracle is not None else WS.float64_run(cfg, w, w64, audio, step, fp32_runs=False)
    missing = [k for k in names if k not in t64]
    errs = {}
    for k in names:
        if k in t64:
            assert got[k].shape == t64[k].shape, (k, got[k].shape, t64[k].shape)
            errs[k] = WS.rel(got[k], t64[k]) if bool(torch.isfinite(got[k]).all()) else float("inf")
    assert y.shape == y64.shape, (y.shape, y64.shape)
    return {"taps": errs, "names": names, "missing": missing, "out": WS.rel(y, y64) if bool(torch.isfinite(y).all()) else float("inf"),
            "ref_absmax": min([float(t64[k].abs().max()) for k in names if k in t64] + [float(y64.abs().max())]),
            "device_seconds": t1 - t0, "oracle_seconds": time.time() - t1, "y": y, "got": got}


def wn_bf16_report(cfg, w, audio, step, net, free_running=True):
    """bf16 device run: every recorded tensor teacher-forced against the bf16-storage oracle (relative L2: one fused layer kernel's own deviation), the
    output from the device's skip sum, and (``free_running``) the output against the fp32 oracle."""
    from oracle import wavenet as W
    t0 = time.time()
    y, got, names = sweep_device_run(net, audio, step)
    t1 = time.time()
    forced = {}
    with torch.no_grad():
        y_f = W.wavenet_forward(w, cfg, audio, step, storage="bf16", force=got, errs=forced)
        y_32 = W.wavenet_forward(w, cfg, audio, step) if free_running else None
    finite = bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(v).all()) for v in got.values())
    return {"taps": forced, "names": names, "missing": sorted(set(got) - set(forced)), "out": W.rel_l2(y, y_f) if finite else float("inf"),
            "net": (W.rel_l2(y, y_32) if finite else float("inf")) if free_running else None,
            "device_seconds": t1 - t0, "oracle_seconds": time.time() - t1, "y": y, "got": got}
