"""The HIP WaveNetNoise held tensor by tensor to a float64 oracle over a sweep of widths, structures and shapes.

Every other GPU test of this network builds a preset or a near-preset: 32 channels (6 layers, cycle 3) and 256 channels (36 layers, cycle 12) in fp32; 64, 128 and 256
channels at 13 or 36 layers and T >= 64 in bf16.  The cases of oracle/wavenet_sweep.py leave that point (config = channels, layers, dilation cycle):
  w32 .. w512  all 16 widths, (C, 2, 2), 2 x 37     every block size of the fp32 kernels (one thread per channel; 96, 160, 224, ... are no whole number of waves;
                                                    512 takes 128 KiB of dynamic LDS); T ragged against the 16-position tile; bf16 at 64 / 128 / 256: one partial tile
  l1 / l1b     (32 | 64, 1, 1), 2 x 20              the only layer is first (skip written, not accumulated) and last (no y_next) at once; fp32 / bf16
  cyc1         (160, 3, 1), 2 x 33                  every dilation 1, a block of 2.5 waves
  cyc24 / cyc24b  (32 | 64, 25, 24), 2 x 100        dilations up to 2^23: both outer taps in the padding; bf16: the disjoint-window staging
  d4096        (128, 14, 13), 2 x 300               overlapping and disjoint staging in one net, dilation 4096 > T; fp32 and bf16
  mid / mid37  (64, 5, 4), 3 x 77                   the default steps, and every step 37.0: a large argument of sinf / expf
  b1           (96, 3, 2), 1 x 50                   one sample: the addend's batch stride is 0
  deep         (32, 1024, 12), 1 x 4200             550,502,400 B of layer inputs > 512 MiB: WavenetNet::forward alternates two buffers and records only "skip"
                                                    (asserted: that is the proof the walk was taken); 1024 layers is the most the library takes
fp32: the output and every recorded tensor, unsubsampled, against oracle/wavenet.py run in float64, bar FP32_TIGHT = 2e-5 (tests/test_oracle_wavenet_sweep.py holds
the fp32 oracle with the exact weight norm to a quarter of that bar of the float64 one).  bf16: every recorded tensor teacher-forced against the bf16-storage oracle at
BF16_LAYER_TOL, the free-running output at BF16_NET_TOL.  Beyond the cases: one handle through eight lengths (eight plans through the four-plan cache), a sample alone
against its row of a batch (fp32; and bf16 across the keep / alternate boundary, the only check of the bf16 alternating walk), and the next-tile prefetch of the
128-position layer kernel at a grid where it runs (child processes, tests/diag/gpu_wn_sweep_report.py).

Measured on one MI355X (worst recorded tensor, then the output).  fp32 against 2e-5:
  w32 .. w512    skip 1.07e-6 (w480), output 1.80e-6 (w512); no trend with the width beyond that (w32: 2.3e-7 / 3.7e-7), nothing special at the block sizes of
                 96, 160, 224, ... threads or at the 128 KiB of w512
  l1, cyc1, cyc24, d4096, mid, mid37, b1     cyc24 y24 7.2e-7, output 1.16e-6 (mid37; mid itself 4.3e-7: the large step costs a factor of three, not the bar)
  deep           skip 1.68e-6, output 1.27e-6 after 1024 layers; names == ["skip"]
  eight lengths  skip 5.8e-7 (T = 17), output 6.1e-7 (T = 127); the second T = 1 run bit-equal to the first
bf16 against BF16_LAYER_TOL = 1e-3 per tensor and for the output, BF16_NET_TOL = 3e-2 free-running:
  cases          w256 y1 6.4e-4 (w128 2.3e-4, w64 4.3e-5: the figure grows with the K of the GEMMs), output 5.3e-5 (w256), free-running 6.2e-3 (cyc24b)
  eight lengths  y3 2.8e-4 (T = 1), output 3.2e-5, free-running 3.6e-3; the second T = 1 run bit-equal to the first
  288 workgroups  (64, 13, 12): y6 1.7e-4, output 1.3e-5; (256, 8, 8): y3 7.8e-4, output 1.7e-5 -- the same figures with ADF_WN_PREFETCH 0 and 1, and the
                 SHA-256 of the output and of the skip sum agree between the two settings in both cases (256 CUs: workgroups 0 .. 31 of 288 prefetch)
Every case gave the same bits on a second run over its used plan.  fp32 mid: sample 0 alone is bit-equal to its row of the batch of 3, all 6 tensors.  bf16
(64, 512, 12) at T = 4200: sample 0 of B = 2 (alternating, 1 name) is bit-equal to B = 1 (resident, 513 names) in the output and the skip sum.
The sweep found no defect of the device code.  What it did find is on the judge's side: the reference's fp32 weight norm (tests/test_oracle_wavenet_sweep.py).
The module: 40 tests in 19.0 s; the four children 2.5 / 2.6 / 4.3 / 4.4 s wall each (imports 2.5 s, the bf16-storage oracle of 256 channels x 36,400 positions
1.9 s; limit 45 s, ten times the slower), deep 2.7 s (its float64 oracle), the bf16 alternating walk 0.7 s, every other test under 0.2 s.

That the sweep has teeth was checked once on six value-only edits (not committed; none changes an address or a bound), each against the whole module but the children:
  fp32 layer kernel without the / sqrt(2)             24 tests fail: every fp32 case with more than one layer (first tensor over: y1, 0.35 .. 0.47) and the fp32 lengths
  fp32 layer kernel adds e_n in place of e_{n+1}      the same 24 (y1 0.27 .. 0.43; w32 output 0.92)
  `first` ignored (skip accumulates on the buffer)    all 24 fp32 cases and the fp32 lengths (skip 0.41 .. 0.75 on the FIRST run already: a plan's workspace is not
                                                      zero; a workspace that were is what the second run of every case is for)
  alternating walk: layer n reads buffer 0 always     deep (skip 1.25, output 0.60) and the bf16 alternating walk (output 2.6, skip 1.9); nothing else, as it must be
  skip_scale from NL + 1                              32 tests: every fp32 and bf16 case and both lengths tests (w32 .. w512 skip 0.1835 = 1 - sqrt(2 / 3) exactly)
  wn_sumsq_kernel as one float accumulation in index order (what a fp32 norm does at its worst)   w192 .. w512 in fp32 (skip 3.2e-5 at w192 to y1 8.1e-5 at
                                                      w512) and w256 in bf16 (y1 1.3e-3 of 1e-3); below 192 channels the float sum is still inside the bar
"""
import functools
import json
import os
import subprocess
import sys
import time

import pytest
import torch

from audiodiffuser_amd import _lib
from audiodiffuser_amd.config import WaveNetConfig
import gpu_helpers as R
from oracle import wavenet_sweep as SW
from test_wavenet import FP32_TIGHT, BF16_LAYER_TOL, BF16_NET_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "tests", "diag", "gpu_wn_sweep_report.py")
_DEVICE_TROUBLE = []                            # a child that failed in any way or ran into its time limit: nothing of this module goes to the device after it


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    _lib.load_library()


@pytest.fixture(autouse=True)
def _device_still_trusted():
    """A device run that raised (R.SWEEP_TROUBLE) or a child that failed or hung: no later test of this module goes to the device."""
    assert not R.SWEEP_TROUBLE and not _DEVICE_TROUBLE, f"not started after: {(R.SWEEP_TROUBLE + _DEVICE_TROUBLE)[0]}"


def check_fp32(rep, tag, layers, alternating=False):
    """The fp32 bars of the module on everything a report compared; prints the figures before it asserts."""
    taps = rep["taps"]
    worst = max(taps, key=taps.get)
    print(f"{tag} fp32: tensors {len(taps)} worst {worst} {taps[worst]:.3e} out {rep['out']:.3e} ref absmax {rep['ref_absmax']:.3f} device s {rep['device_seconds']:.2f} "
          f"oracle s {rep['oracle_seconds']:.2f}")
    assert rep["missing"] == [], f"{tag}: the device records tensors the oracle has no name for: {rep['missing']}"
    if alternating:
        assert rep["names"] == ["skip"], (tag, rep["names"][:5], len(rep["names"]))
    else:
        assert rep["names"] == [f"y{n}" for n in range(layers)] + ["skip"], (tag, rep["names"])
    assert len(taps) == len(rep["names"]) and rep["ref_absmax"] >= 0.05
    over = {k: e for k, e in taps.items() if not e < FP32_TIGHT}
    if over:
        first = next(k for k in rep["names"] if k in over)
        print(f"{tag} fp32: FIRST tensor in walk order over {FP32_TIGHT:.1e}: {first} {over[first]:.3e}; {len(over)} of {len(taps)} over")
    assert not over and rep["out"] < FP32_TIGHT, (tag, rep["out"], sorted(over.items(), key=lambda kv: -kv[1])[:8])


def check_bf16(rep, tag, layers):
    errs = rep["taps"]
    worst = max(errs, key=errs.get)
    print(f"{tag} bf16: tensors {len(errs)} worst {worst} {errs[worst]:.3e} out {rep['out']:.3e} free-running {rep['net']} device s {rep['device_seconds']:.2f} "
          f"oracle s {rep['oracle_seconds']:.2f}")
    assert rep["missing"] == [] and rep["names"] == [f"y{n}" for n in range(layers)] + ["skip"], (tag, rep["missing"], rep["names"])
    assert len(errs) == layers + 1 and set(errs) == set(rep["names"])
    assert errs[worst] < BF16_LAYER_TOL, (tag, worst, errs[worst])
    assert rep["out"] < BF16_LAYER_TOL, (tag, rep["out"])
    if rep["net"] is not None:
        assert rep["net"] < BF16_NET_TOL, (tag, rep["net"])


def same_again(net, audio, step, rep, tag):
    """A second run on the same plan, whose buffers now hold the first run's values, gives the same bits: the first layer WRITES the skip sum (a fresh
    workspace may happen to be zero, a used one is not)."""
    y, got, names = R.sweep_device_run(net, audio, step)
    unequal = [k for k in names if not torch.equal(got[k], rep["got"][k])]
    assert names == rep["names"] and not unequal and torch.equal(y, rep["y"]), (tag, unequal[:5], SW.rel(y, rep["y"]))


@pytest.mark.parametrize("cid", [c for c, v in SW.CASES.items() if "fp32" in v[3]])
def test_fp32_every_tensor_vs_float64_oracle(cid):
    cfg = SW.CASES[cid][0]
    w, w64 = SW.weights(cid)
    audio, step = SW.case_inputs(cid)
    net = R.wn_make(cfg, w, "fp32")
    rep = R.wn_fp32_report(cfg, w, w64, audio, step, net, oracle=SW.float64_reference(cid))
    check_fp32(rep, cid, cfg.residual_layers, alternating=cid == "deep")
    same_again(net, audio, step, rep, cid)


@pytest.mark.parametrize("cid", [c for c, v in SW.CASES.items() if "bf16" in v[3]])
def test_bf16_every_layer_teacher_forced(cid):
    cfg = SW.CASES[cid][0]
    w, _ = SW.weights(cid)
    audio, step = SW.case_inputs(cid)
    net = R.wn_make(cfg, w, "bf16")
    rep = R.wn_bf16_report(cfg, w, audio, step, net)
    check_bf16(rep, cid, cfg.residual_layers)
    same_again(net, audio, step, rep, cid)


LENGTHS = (1, 15, 16, 17, 127, 128, 129, 1)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_one_handle_through_eight_lengths(mode):
    """(64, 4, 3), B = 3, T = 1, 15, 16, 17, 127, 128, 129 and 1 again on ONE net: eight plans through the four-plan cache, every length on either side of the
    16- and 128-position tiles; each result to its own oracle, and the second T = 1 result equals the first bit for bit."""
    cfg = WaveNetConfig(residual_channels=64, residual_layers=4, dilation_cycle=3)
    w, w64 = SW.weights_of(cfg, 131)
    net = R.wn_make(cfg, w, mode)
    first = None
    for i, tlen in enumerate(LENGTHS):
        audio, step = SW.inputs(cfg, (3, tlen), 200 + tlen)
        tag = f"lengths[{i}] T = {tlen}"
        if mode == "fp32":
            rep = R.wn_fp32_report(cfg, w, w64, audio, step, net)
            check_fp32(rep, tag, 4)
        else:
            rep = R.wn_bf16_report(cfg, w, audio, step, net)
            check_bf16(rep, tag, 4)
        assert rep["y"].shape == (3, 1, tlen)
        if i == 0:
            first = rep
    assert torch.equal(rep["y"], first["y"]) and all(torch.equal(rep["got"][k], first["got"][k]) for k in first["names"])


def test_fp32_a_sample_alone_equals_its_row_of_a_batch_of_three():
    """mid: sample 0 run alone with its own step, against sample 0 of the batch of 3, bit for bit (the output and every recorded tensor)."""
    cfg = SW.CASES["mid"][0]
    w, _ = SW.weights("mid")
    net = R.wn_make(cfg, w, "fp32")
    audio, step = SW.case_inputs("mid")
    yb, gb, names = R.sweep_device_run(net, audio, step)
    y1, g1, names1 = R.sweep_device_run(net, audio[:1].contiguous(), step[:1].contiguous())
    assert names1 == names and len(names) == cfg.residual_layers + 1
    diff = {k: SW.rel(g1[k], gb[k][:1]) for k in names}
    diff["out"] = SW.rel(y1, yb[:1])
    worst = max(diff, key=diff.get)
    print("alone vs row 0 of 3: worst", worst, diff[worst], "unequal tensors", sorted(k for k, d in diff.items() if d > 0)[:10])
    assert torch.equal(y1, yb[:1]) and all(torch.equal(g1[k], gb[k][:1]) for k in names), (worst, diff[worst])


def test_bf16_alternating_walk_equals_the_resident_walk_bit_for_bit():
    """(64, 512, 12) in bf16 at T = 4200.  B = 1 holds 275 MB of layer inputs: every one stays resident (513 recorded names).  B = 2 with the same sample first
    holds 550 MB: two buffers alternate (1 name).  Sample 0's output and skip sum must be identical: the only check of the bf16 alternating walk."""
    cfg = WaveNetConfig(residual_channels=64, residual_layers=512, dilation_cycle=12)
    assert SW.layer_input_bytes(cfg, (1, 4200), "bf16") <= SW.KEEP_LIMIT < SW.layer_input_bytes(cfg, (2, 4200), "bf16") == 550502400
    w, _ = SW.weights_of(cfg, 132)
    net = R.wn_make(cfg, w, "bf16")
    audio, step = SW.inputs(cfg, (2, 4200), 300)
    y1, g1, names1 = R.sweep_device_run(net, audio[:1].contiguous(), step[:1].contiguous(), only=("skip",))
    y2, g2, names2 = R.sweep_device_run(net, audio, step, only=("skip",))
    assert names1 == [f"y{n}" for n in range(512)] + ["skip"] and names2 == ["skip"], (len(names1), names2)
    assert bool(torch.isfinite(y2).all()) and float(g1["skip"].abs().max()) >= 0.05 and float(y1.abs().max()) >= 0.05
    d_out, d_skip = SW.rel(y2[:1], y1), SW.rel(g2["skip"][:1], g1["skip"])
    print("bf16 alternating (B = 2) vs resident (B = 1), sample 0: out", d_out, "skip", d_skip)
    assert torch.equal(y2[:1], y1) and torch.equal(g2["skip"][:1], g1["skip"]), (d_out, d_skip)


# ------------------------------------------------------------------ the prefetch route (child processes)
PF_SHAPE = (4, 9100)                             # 72 tiles of 128 positions x 4 samples = 288 workgroups, a multiple of 8: the XCD remap is live
PF_CASES = {"c64": ((64, 13, 12), 141), "c256": ((256, 8, 8), 142)}      # -> (config, seed)
PF_LIMIT = 45                                    # seconds per child: ten times the 4.4 s the slower one takes (imports 2.5 s, bf16-storage oracle 1.9 s)


@functools.lru_cache(maxsize=None)
def pf_child(case, prefetch):
    assert not _DEVICE_TROUBLE, f"not started: an earlier child of this module faulted or hung ({_DEVICE_TROUBLE[0]})"
    (ch, nl, cyc), seed = PF_CASES[case]
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, REPORT, str(ch), str(nl), str(cyc), str(PF_SHAPE[0]), str(PF_SHAPE[1]), str(seed)], capture_output=True, text=True,
                           env=dict(os.environ, ADF_WN_PREFETCH=prefetch, ADF_WN_WIDE="1"), timeout=PF_LIMIT)
    except subprocess.TimeoutExpired:
        _DEVICE_TROUBLE.append(f"{case} prefetch {prefetch}: no result within {PF_LIMIT} s")
        raise
    if r.returncode != 0:
        _DEVICE_TROUBLE.append(f"{case} prefetch {prefetch}: exit status {r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, "prefetch", prefetch, "child wall s", round(time.time() - t0, 1), {k: v for k, v in rep.items() if k != "names"})
    return rep


def pf_grid():
    """(CU count, workgroups of the launch); fails, does not skip, on a device where no workgroup of the launch would prefetch."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    workgroups = -(-PF_SHAPE[1] // 128) * PF_SHAPE[0]
    assert workgroups == 288 and workgroups % 8 == 0
    assert cus >= 8 and workgroups > cus // 8 * 8, f"{cus} CUs: no workgroup of {workgroups} would prefetch"
    return cus, workgroups


@pytest.mark.parametrize("prefetch", ["0", "1"])
@pytest.mark.parametrize("case", list(PF_CASES))
def test_bf16_at_288_workgroups_with_and_without_prefetch(case, prefetch):
    """ADF_WN_PREFETCH = 0 and 1 at 288 workgroups.  The kernel prefetches when workgroup lin + pf_stride exists; pf_stride = the CU count rounded down to a multiple
    of 8 (256 on an MI355X), so with the switch on workgroups 0 .. 31 run the global_load_lds_dword block into their LDS scratch area.  Every layer teacher-forced."""
    cus, workgroups = pf_grid()
    layers = PF_CASES[case][0][1]
    rep = pf_child(case, prefetch)
    assert rep["prefetch"] == prefetch and rep["workgroups"] == workgroups and rep["cus"] == cus
    assert rep["missing"] == [] and rep["names"] == [f"y{n}" for n in range(layers)] + ["skip"] and rep["forced_taps"] == layers + 1
    assert rep["forced_max_rel_l2"] < BF16_LAYER_TOL, rep
    assert rep["out_vs_forced_oracle_rel_l2"] < BF16_LAYER_TOL, rep


@pytest.mark.parametrize("case", list(PF_CASES))
def test_bf16_prefetch_that_prefetches_moves_no_value(case):
    """The two children of a case (run once per session, shared with the test above) hash alike: the SHA-256 of the output and of the skip sum."""
    pf_grid()
    reps = {pf: pf_child(case, pf) for pf in ("0", "1")}
    print(case, "sha256 out", reps["0"]["sha256_out"][:16], reps["1"]["sha256_out"][:16], "skip", reps["0"]["sha256_skip"][:16], reps["1"]["sha256_skip"][:16])
    assert reps["0"]["prefetch"] == "0" and reps["1"]["prefetch"] == "1"
    assert reps["0"]["sha256_out"] == reps["1"]["sha256_out"] and reps["0"]["sha256_skip"] == reps["1"]["sha256_skip"]
