"""The conv2d routes only large batches reach, and the ADM widths whose GroupNorm group is no power of two.

launch_conv2d (adf_conv2d.hip) picks its kernel from the launch geometry: with px = B*H*W and ny = ceil(cout / 128), the same-size 3x3 convs take the
spatial tiles t4 from px/128*ny >= 128 on (t2 below), and every stride-2 conv, every 1x1 conv and every 3x3 conv whose width is no multiple of 32 takes the
per-tap gather kernel as conv2d_gemm_kernel<T, 128> (route g128, 512 threads) where H*W % 128 == 0 and px/128*ny >= 512, as <T, 64> (g64) otherwise.  Both
benchmarked 2-D workloads run g128; the rest of the suite stays below 512 tiles (its largest gather conv has 320).  The bf16 attention launcher has a gate of
the same kind: two query tiles per wave (qrep = 2) from B*heads*(qtiles/8) >= 1024 on, which no other test reaches either (at most 64).

Each route case is a child process (tests/diag/gpu_conv2d_routes_report.py, ADF_C2_TRACE=1) whose ``[adf conv2d]`` lines are parsed into a census: the
tuples (route, dtype, taps, mode, ab, res, stats, c0 < cin) a case must show are spelled out below and a missing one fails the test, so a later change of
the routing cannot silently empty these cases.  fp32: output and every recorded tensor against oracle/unet2d_oai.py at FP32_TIGHT; bf16: every stored tensor
teacher-forced against the bf16-storage oracle at BF16_CONV_TOL / BF16_ATT_TOL (the bars of tests/test_adm.py).  Every sample has its own time.

  R1  B = 512 at 16 x 32, config_c4_small (bf16: model_channels 64): level 1 is 8 x 16 = 128 pixels, ONE g128 tile per image, 512 tiles exactly (qkv: ny = 2
      / 3); level 0 takes t4.  No conv of the case runs g64.
  R2  ADF_CONV2D_TILE=0, B = 64 at 32 x 128, additive conditioning (per-sample bias rows): every conv of the net on g128, modes 0, 1 and 2; level 1 at 512 tiles.
  R3  model_channels 128, channel_mult (1, 2), 8 heads, B = 32 at 32 x 128: the 1x1 convs of level 1 (16 x 64) on g128 with cout 256 (ny = 2, 512 tiles;
      proj_out with epilogue statistics) and 768 (qkv, ny = 6); bf16: head dim 32, 1024 tokens, B*heads*(qtiles/8) = 32*8*4 = 1024: qrep = 2.
  R4  B = 63 against R2's 64 (level 1: 504 tiles -> g64, 512 -> g128) and B = 31 against 32 at 16 x 32 (level 0: 124 tiles -> t2, 128 -> t4).

CPU oracle time per case, measured on 8 threads: r1 2.2 s (bf16 5.1 s), r2 2.4 s (5.9 s), r3 6.5 s (9.3 s), r4 at most 2.4 s, a width case 0.1 s.

Width cases: AdmNet::build_weights chose the fine statistics group as min(g, 4) stepped down to a divisor of 128 (g = gcd of all widths / 32), which need not
divide g: 96 -> 2, 160 / 192 / 224 -> 4 against GroupNorm groups of 3, 5, 6 and 7 channels, and the first forward was refused ("gn_finalize_fine: group size
and source widths must be multiples of the fine group").  It is now the largest power of two dividing g, at most 4 (1, 1, 2, 1; 32 / 64 / 128 / 256 keep 1, 2,
4, 4).  channel_mult (1, 3) at width 64 gives 192 output channels: a partial second N tile and no epilogue statistics (the separate statistics pass).

Measured on one MI355X, worst of the 49 recorded tensors per case (fp32: bar 5e-5; bf16: convs bar 5e-4, attention bar 1e-3) and the output:
  r1_fp32     output_blocks.0.1.att 2.0e-6, output 1.5e-6          r1_bf16   conv output_blocks.1.0.h1 8.1e-5, attention input_blocks.3.1.att 4.8e-5, output 2.1e-7
  r2_fp32     output_blocks.1.1.att 2.9e-6, output 1.1e-6          r2_bf16   conv middle_block.2.h1 8.3e-5, attention output_blocks.0.1.att 5.6e-5, output 2.8e-7
  r3_fp32     input_blocks.3.1.att 4.0e-6, output 1.8e-6           r3_bf16   within both bars (worst values not recorded)
  r4_g_below  output_blocks.1.1.att 2.7e-6, output 1.0e-6          r4_t_below  middle_block.1.att 2.3e-6, output 1.3e-6      r4_t_at  output_blocks.0.1.att 2.0e-6, output 1.2e-6
  w96   output_blocks.0.0.h1 3.7e-6 (output 2.2e-6)    w160  input_blocks.3.1.att 3.0e-6 (1.5e-6)    w192  output_blocks.0.0.h1 4.5e-6 (3.0e-6)
  w224  output_blocks.1.0.h1 3.5e-6 (1.8e-6)           w64x3 output_blocks.1.2 2.2e-6 (1.5e-6)
With the library before the fix 96, 160, 192 and 224 were refused at the first forward with the message above (64 and 64 x (1, 3) ran).  R2's first run
also showed that the fp32 branch of the oracle recorded ``.h1`` as conv1 alone where the device (and the oracle's bf16 branch) stores conv1 + emb_out under
additive conditioning (0.11 to 0.17 apart); the oracle now records the stored tensor in both branches.

That the cases have teeth was checked once on three value-only edits of conv2d_gemm_kernel (not committed), each against r1_fp32, r2_fp32, r2_bf16, r3_fp32:
  table / bias_b / statistics row of image 0 instead of m0 / HW   caught by all four: first tensor over input_blocks.3.0.h1 2.3e4 (r1) and 1.3e3 (r3), input_blocks.1.0.h1
                                                                  0.080 (r2_fp32) and 0.098 (r2_bf16); 32 to 47 of 49 tensors over, outputs NaN or 0.42
  no prologue in the second activation sweep (k = 1)              caught by r1_fp32 (input_blocks.3.0.h1 1.3, 41 tensors over), r2_fp32 (input_blocks.1.0.h1 1.04, 47
                                                                  over) and r2_bf16 (0.50, 16 over); not by r3_fp32, whose g128 convs are the 1x1 ones, without a prologue
  no zeroing of weight rows past n_pad (``wok``)                  NOT caught, and cannot be: such rows feed only output columns >= n_pad = round_up(cout, 32) >= cout,
                                                                  which c2_store_tile neither stores nor reduces (col < cout) and which no MFMA mixes with others; the
                                                                  clamp of their address to row 0 is what keeps the load in bounds, the zeroing changes no value
"""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import pytest
import torch

import audiodiffuser_amd as A
from gpu_helpers import conv2d_trace_lines
from test_adm import FP32_TIGHT, BF16_CONV_TOL, BF16_ATT_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "tests", "diag", "gpu_conv2d_routes_report.py")
_spec = importlib.util.spec_from_file_location("gpu_conv2d_routes_report", REPORT)
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

# case -> (extra environment of the child, its time limit in seconds)
CHILD = {"r1_fp32": ({}, 240), "r1_bf16": ({}, 240), "r2_fp32": ({"ADF_CONV2D_TILE": "0"}, 240), "r2_bf16": ({"ADF_CONV2D_TILE": "0"}, 240),
         "r3_fp32": ({}, 300), "r3_bf16": ({}, 300), "r4_g_below": ({"ADF_CONV2D_TILE": "0"}, 240), "r4_t_below": ({}, 120), "r4_t_at": ({}, 120)}


_DEVICE_TROUBLE = []          # a child that failed in any way (a device fault may surface as an ordinary Python error, exit status 1) or ran into its time
                              # limit: nothing of this module goes to the device after it


def device_still_trusted():
    assert not _DEVICE_TROUBLE, f"not started: an earlier child of this module faulted or hung ({_DEVICE_TROUBLE[0]})"


@functools.lru_cache(maxsize=None)
def child(case):
    """One child per case and session (R4 reads R2's fp32 run again): -> (report, trace lines as dicts with "route")."""
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


def census(lines, dtype):
    """{(route, dtype, taps, mode, ab, res, stats, c0 < cin)}; a GroupNorm prologue always comes with SiLU in this net (ab == act)."""
    assert all(l["ab"] == l["act"] for l in lines)
    return {(l["route"], dtype, l["taps"], l["mode"], l["ab"], l["res"], l["stats"], int(l["c0"] < l["cin"])) for l in lines}


def check_values(rep):
    """The bars of tests/test_adm.py on everything the child compared; prints the worst figures before it asserts."""
    taps = rep["taps"]
    if rep["dtype"] == "fp32":
        worst = max(taps, key=taps.get)
        print(rep["case"], "fp32: taps", len(taps), "worst", worst, taps[worst], "out", rep["out"], "oracle s", round(rep["oracle_seconds"], 1))
        assert not rep["missing"], f"the device records tensors the oracle has no name for: {rep['missing']}"
        assert len(taps) > 30 and rep["ref_absmax"] > 1e-3
        over = {k: e for k, e in taps.items() if not e < FP32_TIGHT}
        assert not over and rep["out"] < FP32_TIGHT, (rep["case"], rep["out"], sorted(over.items(), key=lambda kv: -kv[1])[:8])
        return
    conv = {k: e for k, e in taps.items() if not k.endswith(".att")}
    att = {k: e for k, e in taps.items() if k.endswith(".att")}
    wc, wa = max(conv, key=conv.get), max(att, key=att.get)
    print(rep["case"], "bf16: taps", len(taps), "worst conv", wc, conv[wc], "worst att", wa, att[wa], "out vs forced", rep["out"],
          "oracle s", round(rep["oracle_seconds"], 1))
    assert not rep["missing"], rep["missing"]            # set(errs) == set(taps)
    assert len(taps) > 30 and rep["ref_absmax"] > 1e-3
    over = {k: e for k, e in taps.items() if not e < (BF16_ATT_TOL if k.endswith(".att") else BF16_CONV_TOL)}
    assert not over and rep["out"] < BF16_CONV_TOL, (rep["case"], rep["out"], sorted(over.items(), key=lambda kv: -kv[1])[:8])


def need(cen, required):
    missing = sorted(set(required) - cen)
    assert not missing, f"no conv of this case ran as {missing}; the census was {sorted(cen)}"


# what a ResBlock / AttentionBlock / resampling conv of the walk looks like to the launcher: (taps, mode, ab, res, stats, split source)
CONV1, CONV1_CAT, CONV2 = (9, 0, 1, 0, 1, 0), (9, 0, 1, 0, 1, 1), (9, 0, 1, 1, 1, 0)
ONE, ONE_CAT, PROJ = (1, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 1), (1, 0, 0, 1, 1, 0)      # qkv and skip; skip over a concat; proj_out
UP, DOWN = (9, 1, 0, 0, 1, 0), (9, 2, 0, 0, 1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_r1_one_128_pixel_tile_per_image(dtype):
    rep, lines = child("r1_" + dtype)
    cen = census(lines, dtype)
    need(cen, {("g128", dtype) + k for k in (CONV1, CONV1_CAT, CONV2, ONE, ONE_CAT, PROJ, DOWN)}
         | {("t4", dtype) + k for k in (CONV1, CONV1_CAT, CONV2, UP)})
    assert {l["route"] for l in lines} == {"g128", "t4"}
    lv1 = [l for l in lines if l["H"] * l["W"] == 128]
    assert len(lv1) >= 20 and all(l["route"] == "g128" and l["B"] * 128 // 128 * -(-l["cout"] // 128) >= 512 for l in lv1)
    assert min(l["B"] * -(-l["cout"] // 128) for l in lv1) == 512                          # exactly at the threshold
    check_values(rep)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_r2_every_conv_on_the_128_pixel_gather_kernel_additive_conditioning(dtype):
    rep, lines = child("r2_" + dtype)
    need(census(lines, dtype), {("g128", dtype) + k for k in (CONV1, CONV1_CAT, CONV2, ONE, ONE_CAT, PROJ, UP, DOWN)})
    assert {l["route"] for l in lines} == {"g128"}
    assert {(l["H"], l["W"]) for l in lines} == {(32, 128), (16, 64)}
    check_values(rep)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_r3_two_and_six_n_tiles_and_two_query_tiles_per_wave(dtype):
    rep, lines = child("r3_" + dtype)
    need(census(lines, dtype), {("g128", dtype) + k for k in (ONE, ONE_CAT, PROJ)} | {("t4", dtype) + k for k in (CONV1, CONV1_CAT, CONV2, UP)}
         | {("g64", dtype) + DOWN})
    g128 = [l for l in lines if l["route"] == "g128"]
    assert any(l["cout"] == 256 and l["stats"] and l["res"] and l["B"] * l["H"] * l["W"] // 128 * 2 == 512 for l in g128)      # proj_out: two full N tiles
    assert any(l["cout"] == 256 and l["c0"] < l["cin"] for l in g128) and any(l["cout"] == 768 for l in g128)
    assert all(l["mode"] == 2 for l in lines if l["route"] == "g64")
    if dtype == "bf16":
        # the attention gate of adf_kernels.hip (bf16, head dim 32, at most 1024 tokens): qtiles = ceil(tokens / 32), two query tiles per wave from
        # qtiles >= 8 and B * heads * (qtiles / 8) >= 1024 on.  The launcher prints no line; the launch geometry is read off the qkv conv that feeds it
        # (1x1, cout = 3 C, one row per token) and the head count off the case's configuration
        heads = R.CASES["r3_bf16"][1]["num_heads"]
        qkv = [l for l in lines if l["taps"] == 1 and l["cout"] == 3 * l["cin"]]
        assert len(qkv) >= 4                          # four attention blocks (the plan's warm-up pass traces them once more)
        for l in qkv:
            tokens, qtiles = l["H"] * l["W"], -(-l["H"] * l["W"] // 32)
            assert l["cin"] // heads == 32 and tokens <= 1024 and qtiles >= 8 and l["B"] * heads * (qtiles // 8) >= 1024, l
    check_values(rep)


@pytest.mark.gpu
def test_r4_one_batch_below_and_one_at_each_threshold():
    below, lb = child("r4_g_below")
    at, la = child("r2_fp32")
    assert below["shape"][1:] == at["shape"][1:] and below["shape"][0] + 1 == at["shape"][0]
    # level 1 (16 x 64): 63 * 1024 / 128 = 504 tiles at ny = 1; qkv (cout 192, ny = 2) has 1008 and stays on g128
    assert all(l["route"] == ("g64" if l["H"] == 16 and l["cout"] <= 128 else "g128") for l in lb) and all(l["route"] == "g128" for l in la)
    assert {l["B"] * 16 * 64 // 128 * -(-l["cout"] // 128) for l in lb if l["route"] == "g64"} == {504}
    need(census(lb, "fp32"), {("g64", "fp32") + k for k in (CONV1, CONV1_CAT, CONV2, ONE, ONE_CAT, PROJ, DOWN)} | {("g128", "fp32") + k for k in (CONV1, CONV2, UP)})
    check_values(below)
    check_values(at)
    below, lb = child("r4_t_below")
    at, la = child("r4_t_at")
    assert below["shape"][1:] == at["shape"][1:] and below["shape"][0] + 1 == at["shape"][0]
    same3 = lambda ls: [l for l in ls if l["taps"] == 9 and l["mode"] != 2 and l["W"] == 32]
    assert len(same3(lb)) == len(same3(la)) >= 7
    assert all(l["route"] == "t2" and l["B"] * 512 // 128 == 124 for l in same3(lb)) and all(l["route"] == "t4" and l["B"] * 512 // 128 == 128 for l in same3(la))
    need(census(lb, "fp32"), {("t2", "fp32") + k for k in (CONV1, CONV1_CAT, CONV2, UP)})
    need(census(la, "fp32"), {("t4", "fp32") + k for k in (CONV1, CONV1_CAT, CONV2, UP)})
    check_values(below)
    check_values(at)


# ------------------------------------------------------------------ widths
WIDTHS = {"w96": {"model_channels": 96}, "w160": {"model_channels": 160}, "w192": {"model_channels": 192}, "w224": {"model_channels": 224},
          "w64x3": {"model_channels": 64, "channel_mult": (1, 3)}}


@pytest.mark.gpu
@pytest.mark.parametrize("wid", list(WIDTHS))
def test_widths_whose_group_size_is_no_power_of_two(wid):
    """B = 2 at 16 x 32, two levels, 32-channel heads: the forward succeeds (the fine statistics group divides every GroupNorm group) and every recorded
    tensor matches the oracle."""
    device_still_trusted()
    cfg, w, x, t, net = R.make_case("fp32", {**WIDTHS[wid], "num_head_channels": 32}, (2, 16, 32), 50 + len(wid))
    rep = R.fp32_report(cfg, w, x, t, net, torch.device("cuda", torch.cuda.current_device()))
    rep.update(case=wid, dtype="fp32")
    check_values(rep)


def test_widths_the_device_cannot_serve_are_refused_at_construction():
    """Not by the library at the first forward: a width above 256, a skip concat of more than 1024 channels, a head dim the attention kernels are not
    built for.  The widths of the cases above construct."""
    for mc in (288, 512):
        with pytest.raises(ValueError, match="model_channels up to 256"):
            A.UNetModel(model_channels=mc, channel_mult=(1, 2), compute_dtype="fp32")
    with pytest.raises(ValueError, match="at most 1024 input channels: output_blocks.0.0 reads 2048"):
        A.UNetModel(model_channels=256, channel_mult=(1, 4), num_res_blocks=1, num_head_channels=64, compute_dtype="fp32")
    with pytest.raises(ValueError, match="head dim of 8, 16, 32 or 64: middle_block.1 has 192 channels in 2 heads"):
        A.UNetModel(model_channels=96, channel_mult=(1, 2), num_heads=2, compute_dtype="fp32")
    with pytest.raises(ValueError, match="head dim of 8, 16, 32 or 64"):
        A.UNetModel(model_channels=128, channel_mult=(1, 2), num_res_blocks=1, num_head_channels=128, compute_dtype="fp32")
    for kw in WIDTHS.values():
        A.UNetModel(image_size=32, in_channels=1, out_channels=1, num_res_blocks=1, **{"channel_mult": (1, 2), **kw}, num_head_channels=32)
    A.UNetModel(model_channels=256, channel_mult=(1, 2), num_res_blocks=1, compute_dtype="bf16")              # 512 + 512 channels: the widest concat served
