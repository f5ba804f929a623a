"""GPU: the transposed-conv kernel of the up path (csrc/adf_gemm_up.h) indexed by output block j = 0 .. L - 1 -- exactly L rows per phase, the lower
phases shifted by one input row, the tile height chosen from the live rows, a tile staged once per workgroup -- on the configs[1] network in bf16.

Cases (device side: tests/diag/gpu_up_rows_report.py, one child process per environment, because the route switches are read once per process):
  3:4096    the x4 convs see L = 4, 16, 64: a tile with more dead than live rows, the 32- and 64-row heights
  3:16384   L = 16, 64, 256: two full 128-row tiles
  3:20480   L = 20, 80, 320: a partial last tile (the heights are 32, 32 and 64 rows: a batch of 3 is one round at any height)
  33:20480  the x4 convs only: at L = 320 the 128-row tile saves a round over the shorter ones, and its third tile is partial
  5:5120    with ADF_GEMM_UP=2, so that the three x2 shapes (256 -> 128, 128 -> 128, 128 -> 64 at L = 320, 640, 1280) run the same indexing
            (at this batch the three-tap form of the resblock conv kernel does not take them)

Stored tensors.  For every ``up*.conv`` launch that took the ``up`` route: conv_transpose1d in float64 on the CPU from the bf16 tensor the walk fed
the conv and the bf16-rounded weights; every stored element within one bf16 ulp of the float64 value, 2^-8 |ref|, plus the fp32 accumulation bound
K 2^-24 sum|x w| with K = 2 Cin products per element.  Both are derived, not tuned; an indexing error is O(1).  The first and last f output rows of
every sample -- the rows the shift touches -- are held again on their own.

Statistics.  The (sum, sum of squares) per sample and GroupNorm group that the launch reduced in its epilogue against float64 sums of the stored
tensor: the project has no other check of fused statistics to take a bound from, so n 2^-24 sum|v| (n 2^-24 sum v^2) with n the elements of a group.
"""
import functools
import os
import subprocess
import sys
import time

import pytest
import torch
import torch.nn.functional as F

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
from audiodiffuser_amd.weights import generate_weights
from gpu_helpers import gemm_trace_lines

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "tests", "diag", "gpu_up_rows_report.py")
# child -> (extra environment, its cases as batch:waveform length, its time limit in seconds: imports, 24 M weights, three passes -- some ten seconds)
CHILD = {"default": ({}, ["3:4096", "3:16384", "3:20480", "33:20480:0,1,2"], 120), "up2": ({"ADF_GEMM_UP": "2"}, ["5:5120"], 120)}
CASES = [("default", "3:4096"), ("default", "3:16384"), ("default", "3:20480"), ("default", "33:20480:0,1,2"), ("up2", "5:5120")]
_DEVICE_TROUBLE = []          # a child that failed in any way or ran into its time limit: nothing of this module goes to the device after it


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    _lib.load_library()


@functools.lru_cache(maxsize=None)
def child(which, tmp):
    assert not _DEVICE_TROUBLE, f"not started: an earlier child of this module faulted or hung ({_DEVICE_TROUBLE[0]})"
    env, cases, limit = CHILD[which]
    out = os.path.join(tmp, which + ".pt")
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, REPORT, out] + cases, capture_output=True, text=True, env=dict(os.environ, ADF_GEMM_TRACE="1", **env), timeout=limit)
    except subprocess.TimeoutExpired:
        _DEVICE_TROUBLE.append(f"{which}: no result within {limit} s")
        raise
    if r.returncode != 0:
        _DEVICE_TROUBLE.append(f"{which}: exit status {r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    print(which, "child wall s", round(time.time() - t0, 1))
    return torch.load(out), gemm_trace_lines(r.stderr)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("up_rows"))


@functools.lru_cache(maxsize=None)
def weights():
    cfg = A.PRESETS["c2"]()
    return cfg, {k: v for k, v in generate_weights(cfg, seed=0).items() if ".upsample." in k}


@functools.lru_cache(maxsize=None)
def reference(which, case, tmp):
    """-> {conv name: (route, f, x, y, stats, float64 value, bound)} of one case, computed once for the tests that share it."""
    rep, lines = child(which, tmp)
    cfg, w = weights()
    B = int(case.split(":")[0])
    n = cfg.num_layers
    out = {}
    for u, i in enumerate(reversed(range(n))):
        if f"up{u}.conv" not in rep[case]:
            continue
        rec = rep[case][f"up{u}.conv"]
        f = cfg.factors[i]
        wt, bias = w[f"unet.upsamples.{u}.upsample.weight"], w[f"unet.upsamples.{u}.upsample.bias"]
        x, y = rec["x"], rec["y"]
        cin, cout, L = wt.shape[0], wt.shape[1], x.shape[2]
        assert tuple(wt.shape) == (cin, cout, 2 * f) and tuple(x.shape) == (B, cin, L) and tuple(y.shape) == (B, cout, f * L), (u, wt.shape, x.shape, y.shape)
        assert torch.equal(x, x.bfloat16().float()) and torch.equal(y, y.bfloat16().float())           # bf16 storage, converted exactly
        routes = {l["route"] for l in lines if l["B"] == B and l["lin"] == L and l["c0"] == cin and l["out_c"] == cout and l["scatter"] == f}
        assert len(routes) <= 1, (u, routes)
        w64 = wt.bfloat16().double()
        x64 = x.double()
        ref = F.conv_transpose1d(x64, w64, bias.double(), stride=f, padding=f // 2)
        mag = F.conv_transpose1d(x64.abs(), w64.abs(), None, stride=f, padding=f // 2)
        bound = 2.0 ** -8 * ref.abs() + 2 * cin * 2.0 ** -24 * mag
        out[f"up{u}.conv"] = (routes.pop() if routes else None, f, x, y, rec["stats"], ref, bound)
    return out


def up_route(which, case, tmp):
    got = {k: v for k, v in reference(which, case, tmp).items() if v[0] == "up"}
    # the three x4 convs of the network always take the route; with ADF_GEMM_UP=2 at batch 5 all six transposed convs do
    want = {"up0.conv", "up1.conv", "up2.conv"} | ({"up3.conv", "up4.conv", "up5.conv"} if which == "up2" else set())
    assert want <= set(got), (case, {k: v[0] for k, v in reference(which, case, tmp).items()})
    return got


@pytest.mark.parametrize("which,case", CASES, ids=[c[1].replace(":", "x").replace(",", "") for c in CASES])
def test_stored_tensors_within_one_bf16_ulp_of_float64(which, case, tmp):
    for name, (_, f, x, y, _, ref, bound) in up_route(which, case, tmp).items():
        err = (y.double() - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{case} {name}: L = {x.shape[2]} f = {f}: max |y - ref| / bound = {worst:.3f}, max |y - ref| = {float(err.max()):.3e}, max |ref| = {float(ref.abs().max()):.3e}")
        assert float(ref.abs().max()) > 1e-2 and bool(torch.isfinite(y).all())
        assert bool((err <= bound).all()), f"{case} {name}: {int((err > bound).sum())} stored elements off, the first at {tuple((err > bound).nonzero()[0].tolist())}"
        # the rows the shift touches: the first and the last f output rows of every sample
        for sl, what in ((slice(0, f), "first"), (slice(f * x.shape[2] - f, f * x.shape[2]), "last")):
            assert bool((err[:, :, sl] <= bound[:, :, sl]).all()), f"{case} {name}: the {what} {f} output rows"
            assert float(y[:, :, sl].abs().max()) > 0


@pytest.mark.parametrize("which,case", CASES, ids=[c[1].replace(":", "x").replace(",", "") for c in CASES])
def test_fused_statistics_are_the_sums_of_the_stored_tensor(which, case, tmp):
    seen = 0
    for name, (_, f, x, y, stats, _, _) in up_route(which, case, tmp).items():
        if stats is None:          # the last conv of the up path feeds no GroupNorm
            assert name == "up5.conv"
            continue
        B, cout, lout = y.shape
        assert tuple(stats.shape) == (B, 8, 2)
        v = y.double().reshape(B, 8, cout // 8, lout)
        n = (cout // 8) * lout
        s1, s2, sa = v.sum(dim=(2, 3)), (v * v).sum(dim=(2, 3)), v.abs().sum(dim=(2, 3))
        e1, e2 = (stats[:, :, 0] - s1).abs(), (stats[:, :, 1] - s2).abs()
        b1, b2 = n * 2.0 ** -24 * sa, n * 2.0 ** -24 * s2
        print(f"{case} {name}: n = {n}: sum off by {float((e1 / b1).max()):.2e} of its bound, sum of squares by {float((e2 / b2).max()):.2e}")
        assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), (case, name, float((e1 / b1).max()), float((e2 / b2).max()))
        assert float(s2.min()) > 0
        seen += 1
    assert seen >= 3
