"""The ADM UNetModel in the split-bf16 mode (compute_dtype="f32x3"): fp32 tensors, every 3x3 / 1x1 conv on conv2d_tile_kernel<f32x3_t> /
conv2d_gemm_kernel<f32x3_t> (adf_conv2d.hip: each operand as bf16 hi + lo, three bf16 MFMAs per product) and the head-dim-32 attention on
attention_x3_kernel; everything else is the fp32 mode's.

The comparison is tests/diag/gpu_conv2d_routes_report.py::fp32_report: free-running, the output and EVERY tensor the device records
(``hd.tap_names()``, unsubsampled) against oracle/unet2d_oai.py, max |a - b| / max |b|, at F32X3_TOL = 2e-4 (tests/test_gpu_parity.py: the project's
split-bf16 bar; the arithmetic emulated on the CPU sits at 1.2e-5 to 4.6e-5 per case, so the bar leaves 4x or more).  Weights: generate_weights with
the case's seed; every sample has its own time.

The cases that need an environment switch or a route census are child processes (tests/diag/gpu_adm_f32x3_report.py, ADF_C2_TRACE=1), each with its
own time limit; after a child that failed or timed out the module starts nothing more on the device.  The (route, taps, mode, ab, res, stats,
c0 < cin) tuples a case must show are spelled out below: a missing one fails the test, and so does any route label without the ``.x3`` suffix --
that is what proves the split kernels ran rather than the exact ones.  With config_c4_small (32 / 64 channels, two levels):
  small          2 x 16 x 32    level 0 (W = 32, 8 tiles) on t2; level 1 (W = 16), the stride-2 conv and every 1x1 conv on g64; two-source concats;
                                attention at head dim 32 (attention_x3).  input_blocks.1.0.h1 must differ in its bits from the fp32 mode's
  t4             8 x 32 x 64    level 0: 128 tiles of 128 pixels -> t4; level 1 (16 x 32, 32 tiles) on t2
  t5             32 x 10 x 128  level 0: 5 x 32 tiles (256 of them); level 1 (5 x 64) on g64
  g128           512 x 16 x 32  level 1: one g128 tile per image, 512 tiles exactly; level 0 on t4
  gather         2 x 16 x 32    ADF_CONV2D_TILE=0: every conv on g64, modes 0, 1 and 2
  updown         2 x 16 x 32    resblock_updown, additive conditioning: ResBlock(up=True)'s conv1 (mode 1 with a prologue) on t2, ResBlock(down=True)'s
                                conv1 over the pooled activation (raw input, per-sample bias rows)
  updown_gather  as updown with ADF_CONV2D_TILE=0: that mode-1 conv on the gather kernel
In process: add (per-sample bias rows), pool (pooled resampling, three levels, attention at 2048 tokens: the exact kernel), heads16 (head dim 16: the
exact-attention fallback), w96 (partial N tile, 192 channels without epilogue statistics, fine group 2), c4 (config_c4() at 1 x 80 x 256: 1024-channel
two-source K; the output also against the reference's own adm_c4_y).  Sampler: config 4's churn EDMSampler (35 steps, 69 evaluations) on the reference's
fixture, eager once and graph-replayed twice, at the 2e-4 of the fp32 mode's test; one guided denoise_fn call (10 classes, cond_scale 3, per-sample sigmas).

Measured on one MI355X, worst recorded tensor per case (bar 2e-4) and the output:
  small          output_blocks.1.1.att 2.5e-5, output 1.3e-5 (49 tensors); input_blocks.1.0.h1 5.2e-6 from the fp32 mode's, not bit-equal
  t4             output_blocks.1.1.att 2.9e-5, output 1.3e-5          t5             middle_block.1.att 4.3e-5, output 1.7e-5
  g128           output_blocks.0.1.att 3.0e-5, output 1.7e-5          gather         output_blocks.0.1.att 2.1e-5, output 1.6e-5
  updown         output_blocks.1.1.att 2.8e-5, output 2.0e-5 (51)     updown_gather  output_blocks.1.1.att 3.3e-5, output 2.1e-5 (51)
  add            output_blocks.1.1.att 2.4e-5, output 1.4e-5          pool           output_blocks.3.1.att 4.3e-5, output 2.1e-5 (75)
  heads16        output_blocks.1.1.att 2.4e-5, output 1.2e-5          w96            output_blocks.1.1.att 1.8e-5, output 1.5e-5
  c4             output_blocks.3.0.skip 1.6e-5, output 1.2e-5 (94 tensors), 1.2e-5 from the reference's adm_c4_y
  sampler        1.7e-5 eager, 1.5e-5 / 1.5e-5 graph-replayed (bar 2e-4)          guided denoise_fn 5.6e-5
On the parent commit every GPU test of this module fails at construction of the device handle ("adf_adm_create: bad dtype").
"""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd.adm_config import generate_weights
from gpu_helpers import conv2d_trace_lines
from oracle import unet2d_oai as O
from test_gpu_parity import F32X3_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "diag", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("gpu_conv2d_routes_report")       # fp32_report, make_case, rel
X = _load("gpu_adm_f32x3_report")           # the case table and the child
REPORT = os.path.join(ROOT, "tests", "diag", "gpu_adm_f32x3_report.py")

# case -> (extra environment of the child, its time limit in seconds)
CHILD = {"small": ({}, 120), "t4": ({}, 120), "t5": ({}, 180), "g128": ({}, 240), "gather": ({"ADF_CONV2D_TILE": "0"}, 120),
         "updown": ({}, 120), "updown_gather": ({"ADF_CONV2D_TILE": "0"}, 120)}

_DEVICE_TROUBLE = []          # a child that failed in any way or ran into its time limit: nothing of this module goes to the device after it


def device_still_trusted():
    assert not _DEVICE_TROUBLE, f"not started: an earlier child of this module faulted or hung ({_DEVICE_TROUBLE[0]})"


@functools.lru_cache(maxsize=None)
def child(case):
    device_still_trusted()
    env, limit = CHILD[case]
    try:
        r = subprocess.run([sys.executable, REPORT, case], capture_output=True, text=True, env=dict(os.environ, ADF_C2_TRACE="1", **env), timeout=limit)
    except subprocess.TimeoutExpired:
        _DEVICE_TROUBLE.append(f"{case}: no result within {limit} s")
        raise
    if r.returncode != 0:
        _DEVICE_TROUBLE.append(f"{case}: exit status {r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    lines = conv2d_trace_lines(r.stderr)
    assert rep["case"] == case and rep["route_tile"] == env.get("ADF_CONV2D_TILE", "1") and lines, (rep["case"], rep["route_tile"], len(lines))
    assert all(l["B"] == rep["shape"][0] for l in lines)
    return rep, lines


def census(lines):
    """{(route, taps, mode, ab, res, stats, c0 < cin)}; every label must carry the suffix of the split-bf16 instantiations."""
    plain = sorted({l["route"] for l in lines if not l["route"].endswith(".x3")})
    assert not plain, f"convs of an f32x3 net ran on the fp32 / bf16 instantiations: {plain}"
    assert all(l["ab"] == l["act"] for l in lines)
    return {(l["route"], l["taps"], l["mode"], l["ab"], l["res"], l["stats"], int(l["c0"] < l["cin"])) for l in lines}


def need(cen, required):
    missing = sorted(set(required) - cen)
    assert not missing, f"no conv of this case ran as {missing}; the census was {sorted(cen)}"


def check_values(rep):
    taps = rep["taps"]
    worst = max(taps, key=taps.get)
    print(rep["case"], "f32x3: taps", len(taps), "worst", worst, taps[worst], "out", rep["out"], "oracle s", round(rep["oracle_seconds"], 1))
    assert not rep["missing"], f"the device records tensors the oracle has no name for: {rep['missing']}"
    assert len(taps) > 30 and rep["ref_absmax"] > 1e-3
    over = {k: e for k, e in taps.items() if not e < F32X3_TOL}
    assert not over and rep["out"] < F32X3_TOL, (rep["case"], rep["out"], sorted(over.items(), key=lambda kv: -kv[1])[:8])


# what a conv of the walk looks like to the launcher: (taps, mode, ab, res, stats, split source)
CONV1, CONV1_CAT, CONV2 = (9, 0, 1, 0, 1, 0), (9, 0, 1, 0, 1, 1), (9, 0, 1, 1, 1, 0)
ONE, ONE_CAT, PROJ = (1, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 1), (1, 0, 0, 1, 1, 0)      # qkv and skip; skip over a concat; proj_out
UP, DOWN = (9, 1, 0, 0, 1, 0), (9, 2, 0, 0, 1, 0)                                     # Upsample's / Downsample's conv
UP_RES, POOLED = (9, 1, 1, 0, 1, 0), (9, 0, 0, 0, 1, 0)                               # conv1 of ResBlock(up=True) / of ResBlock(down=True), over the pooled activation


def routes(route, kinds):
    return {(route + ".x3",) + k for k in kinds}


@pytest.mark.gpu
def test_small_t2_and_g64_two_sources_and_the_split_attention():
    rep, lines = child("small")
    need(census(lines), routes("t2", (CONV1, CONV1_CAT, CONV2, UP)) | routes("g64", (CONV1, CONV1_CAT, CONV2, ONE, ONE_CAT, PROJ, DOWN)))
    assert {l["route"] for l in lines} == {"t2.x3", "g64.x3"}
    check_values(rep)
    # the split kernels ran: the first ResBlock's conv1 output is not the exact-fp32 one, bit for bit
    device_still_trusted()
    dev = torch.device("cuda", torch.cuda.current_device())
    changes, shape, seed = X.CASES["small"]
    got = {}
    for dtype in ("f32x3", "fp32"):
        cfg, w, x, t, net = R.make_case(dtype, changes, shape, seed)
        net = net.to(dev)
        net(x.to(dev), t.to(dev))
        got[dtype] = net.native(dev).tap("input_blocks.1.0.h1", shape[0], dev).cpu()
    d = R.rel(got["f32x3"], got["fp32"])
    print("small: input_blocks.1.0.h1, f32x3 against fp32 on the device:", d)
    assert not torch.equal(got["f32x3"], got["fp32"]) and d < F32X3_TOL


@pytest.mark.gpu
def test_t4_128_pixel_tiles_at_level_0():
    rep, lines = child("t4")
    need(census(lines), routes("t4", (CONV1, CONV1_CAT, CONV2, UP)) | routes("t2", (CONV1, CONV1_CAT, CONV2)) | routes("g64", (ONE, ONE_CAT, PROJ, DOWN)))
    assert all(l["route"] == "t4.x3" and l["B"] * 32 * 64 // 128 == 128 for l in lines if l["taps"] == 9 and l["mode"] != 2 and l["H"] == 32)
    check_values(rep)


@pytest.mark.gpu
def test_t5_160_pixel_tiles_on_ten_row_images():
    rep, lines = child("t5")
    need(census(lines), routes("t5", (CONV1, CONV1_CAT, CONV2, UP)) | routes("g64", (CONV1, CONV1_CAT, CONV2, ONE, ONE_CAT, PROJ, DOWN)))
    assert {l["route"] for l in lines} == {"t5.x3", "g64.x3"}
    assert sum(1 for l in lines if l["route"] == "t5.x3") >= 6
    check_values(rep)


@pytest.mark.gpu
def test_g128_one_128_pixel_tile_per_image():
    rep, lines = child("g128")
    need(census(lines), routes("g128", (CONV1, CONV1_CAT, CONV2, ONE, ONE_CAT, PROJ, DOWN)) | routes("t4", (CONV1, CONV1_CAT, CONV2, UP)))
    assert {l["route"] for l in lines} == {"g128.x3", "t4.x3"}
    lv1 = [l for l in lines if l["H"] * l["W"] == 128]
    assert len(lv1) >= 20 and min(l["B"] * -(-l["cout"] // 128) for l in lv1) == 512          # exactly at the threshold
    check_values(rep)


@pytest.mark.gpu
def test_gather_every_conv_on_the_per_tap_kernel():
    rep, lines = child("gather")
    need(census(lines), routes("g64", (CONV1, CONV1_CAT, CONV2, ONE, ONE_CAT, PROJ, UP, DOWN)))
    assert {l["route"] for l in lines} == {"g64.x3"}
    check_values(rep)


@pytest.mark.gpu
def test_updown_mode_1_with_a_prologue_on_the_tile_kernel_and_pooled_inputs():
    rep, lines = child("updown")
    need(census(lines), routes("t2", (CONV1, CONV1_CAT, CONV2, UP_RES)) | routes("g64", (CONV1, CONV1_CAT, CONV2, ONE, ONE_CAT, PROJ, POOLED)))
    assert {l["route"] for l in lines} == {"t2.x3", "g64.x3"}
    check_values(rep)


@pytest.mark.gpu
def test_updown_gather_mode_1_on_the_gather_kernel():
    rep, lines = child("updown_gather")
    need(census(lines), routes("g64", (CONV1, CONV1_CAT, CONV2, ONE, ONE_CAT, PROJ, UP_RES, POOLED)))
    assert {l["route"] for l in lines} == {"g64.x3"}
    assert {l["mode"] for l in lines} == {0, 1}          # (the only mode-1 convs of this net are ResBlock(up=True)'s conv1; it has no stride-2 conv)
    check_values(rep)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["add", "pool", "heads16", "w96"])
def test_in_process_variants(case):
    device_still_trusted()
    check_values(X.run_case(case, torch.device("cuda", torch.cuda.current_device())))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_c4_full_size_1024_channel_two_source_k():
    device_still_trusted()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "next_golden.npz"))
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = A.config_c4()
    w = generate_weights(cfg, seed=4)
    net = A.UNetModel.from_config(cfg, compute_dtype="f32x3")
    net.load_state_dict(w, strict=True)
    x, t = T(gold["adm_c4_x"]), T(gold["adm_c4_t"])
    rep = R.fp32_report(cfg, w, x, t, net, dev)
    rep.update(case="c4", dtype="f32x3")
    y = net(x.to(dev), t.to(dev)).cpu()
    e = R.rel(y, T(gold["adm_c4_y"]))
    print("c4: output against the reference's adm_c4_y", e)
    check_values(rep)
    assert len(rep["taps"]) > 90 and e < F32X3_TOL, (len(rep["taps"]), e)


@pytest.mark.gpu
def test_config4_churn_sampler_eager_and_graph_replayed_vs_reference_golden():
    """EDMSampler(s_churn=40, s_noise=1.003, s_tmin=0.05, s_tmax=50, num_steps=35): 69 evaluations on the reference's 2 x 1 x 16 x 32 fixture with
    its randn_like draws injected (tests/test_adm.py runs the same in fp32 at the same bar)."""
    device_still_trusted()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "next_golden.npz"))
    cfg = A.config_c4_small()
    net = A.UNetModel.from_config(cfg, compute_dtype="f32x3")
    net.load_state_dict(generate_weights(cfg, seed=3), strict=True)
    net = net.cuda()
    diff = A.EluDiffusion(sigma_data=0.5)
    noise, draws, sig = T(gold["adm_samp_noise"]), T(gold["adm_samp_draws"]), T(gold["adm_samp_sigmas"])
    errs = []
    for use_graph in (False, True, True):
        smp = A.EDMSampler(s_tmin=0.05, s_tmax=50.0, s_churn=40.0, s_noise=1.003, num_steps=35, use_graph=use_graph)
        y = smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig, injected_noise=draws.cuda()).cpu()
        assert y.shape == noise.shape
        errs.append(R.rel(y, T(gold["adm_samp_y"])))
    print("sampler (eager, graph, graph):", errs)
    assert all(e < 2e-4 for e in errs), errs


@pytest.mark.gpu
def test_guided_denoise_call_with_per_sample_sigmas_vs_oracle():
    from oracle import edm as E
    device_still_trusted()
    cfg = A.ADMConfig(**{**A.config_c4_small().to_kwargs(), "num_classes": 10})
    w = generate_weights(cfg, seed=71)
    net = A.UNetModel.from_config(cfg, compute_dtype="f32x3")
    net.load_state_dict(w, strict=True)
    net = net.cuda()
    diff = A.EluDiffusion(sigma_data=0.5)
    x, cl, sig = torch.randn(2, 1, 16, 32, generator=torch.Generator().manual_seed(72)) * 1.5, torch.tensor([3, 7]), torch.tensor([0.7, 2.5])

    def net_o(xi, ti, cond_drop_prob=0.0):
        return O.unet2d_forward(w, cfg, xi, ti, classes=cl, cond_drop_prob=cond_drop_prob)

    with torch.no_grad():
        d = diff.denoise_fn(x.cuda(), net=net, inference=True, cond_scale=3.0, sigmas=sig.cuda(), classes=cl.cuda()).cpu()
        ref = E.denoise(net_o, x, 0.5, sigmas=sig, cond_scale=3.0)
    e = R.rel(d, ref)
    print("guided denoise_fn:", e)
    assert float(ref.abs().max()) > 1e-3 and e < F32X3_TOL, e
