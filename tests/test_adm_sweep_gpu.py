"""The HIP ADM UNetModel held tensor by tensor to a float64 oracle over a sweep of constructor arguments and image shapes (oracle/adm_sweep.py).

Every other ADM test builds config_c4_small, a one-argument change of it, or config_c4 at 1 x 80 x 256.  The cases here reach what those never do: the
first conv with 4 input channels (conv2d_in_kernel<T, 0>, weights from LDS), the last conv with 3 output channels (4 x 32 tiles), ResBlock(up / down) with
scale-shift conditioning, pooled resampling right after an attention block, attention at level 0 (1024 tokens), three levels with two res blocks, a
narrowing channel_mult and a single-entry one, head dims 8 and 64 and 3 heads, images of one, two (at level 1), three and four rows, a coarse level two
pixels wide, batches of 1, 3, 5 and 7 with per-sample times and labels.  The case table, its inputs and the float64 run live in oracle/adm_sweep.py; the CPU
side (the fp32 oracle against the float64 run) is tests/test_oracle_adm_sweep.py.

  fp32    every run: the output and EVERY tensor the device records (``hd.tap_names()``, unsubsampled) against the float64 run, max |a - b| / max |b|.  Bar
          per tensor: FP32_TIGHT = 5e-5, or 4 x the tensor's own fp32-oracle distance where that exceeds a quarter of it (never here: worst 3.5e-6).  A
          device tap without an oracle name fails the test.  io43 also with its labels dropped, lv3 also at 2 x 16 x 64, on the same handle.
  f32x3   every run, free-running against the float64 run at F32X3_TOL = 2e-4; the worst tensor must be > 1e-7 (not silently the exact route).
  bf16    the cases whose widths are multiples of 64, teacher-forced per stored tensor against the bf16-storage oracle (relative L2) at BF16_CONV_TOL /
          BF16_ATT_TOL of tests/test_adm.py.
  one handle through four shapes, returning to the first; sample 3 of io43 alone against its row of the batch of 7 at FP32_TIGHT (the statistics are
  reduced with atomics whose order varies, so the claim is the fp32 bar, not bit equality).

Measured on one MI355X, worst recorded tensor and the output per run:
  run           fp32 (bar 5e-5)                         f32x3 (bar 2e-4)                        tensors
  lv3           output_blocks.0.1.att 3.8e-6, 1.0e-6    output_blocks.5.1.att 3.2e-5, 1.4e-5    114
  lv3_16x64     output_blocks.3.1.att 4.7e-6, 1.9e-6    input_blocks.5.1.att 3.9e-5, 1.7e-5     114
  updown_ss     output_blocks.0.1.att 2.4e-6, 1.7e-6    output_blocks.0.1.att 2.1e-5, 2.1e-5    52
  pool_hd8      output_blocks.5.1.att 2.6e-6, 1.9e-6    output_blocks.4.1.att 3.7e-5, 2.4e-5    88
  one_level     output_blocks.1.0.h1 1.4e-6, 1.8e-6     middle_block.1.att 1.4e-5, 9.8e-6       23
  io43          output_blocks.1.2 2.1e-6, 1.4e-6        output_blocks.0.1.att 2.3e-5, 1.1e-5    50
  io43_dropped  output_blocks.1.2 2.2e-6, 1.4e-6        output_blocks.1.1.att 1.7e-5, 1.2e-5    50
  flat          output_blocks.1.1.att 1.8e-6, 1.8e-6    output_blocks.0.1.att 2.3e-5, 1.8e-5    50
  tall          middle_block.1.att 2.4e-6, 1.0e-6       output_blocks.1.1.att 3.8e-5, 1.6e-5    50
  mult21        output_blocks.1.1.att 5.3e-6, 1.9e-6    output_blocks.0.1.att 7.1e-5, 1.5e-5    94
  odd_h         middle_block.1.att 2.2e-6, 9.6e-7       middle_block.1.qkv 1.4e-5, 1.6e-5       23
  one_row       output_blocks.1.0.skip 9.8e-7, 9.6e-7   output_blocks.0.0.skip 2.0e-5, 1.3e-5   23
  bf16 (convs bar 5e-4, attention bar 1e-3, output against the forced run bar 5e-4):
  updown_ss     conv output_blocks.0.0.h1 1.4e-4, attention input_blocks.3.1.att 6.9e-5, output 2.4e-7 (51 tensors)
  one_level     conv middle_block.2 1.1e-4, attention middle_block.1.att 1.3e-4, output 2.3e-7 (22)
  flat_w64      conv output_blocks.2.0 1.9e-4, attention input_blocks.3.1.att 1.0e-4, output 2.2e-7 (49)
  lv3_w64       conv input_blocks.1.0 1.5e-4, attention input_blocks.7.1.att 7.1e-5, output 2.7e-7 (113)
  four shapes on one handle: at most 5.1e-6 (output_blocks.5.1.att at 2 x 16 x 64), outputs at most 1.8e-6.  io43 sample 3 alone against its row of the
  batch of 7: output_blocks.3.0 1.7e-6 at worst, output 1.3e-6.  The whole module takes about 4 s on the device.

No case exposed a kernel defect, and none is refused: every gate the new shapes pass (launch_conv2d, conv2d_in, conv2d_out, avgpool2, nearest_up2,
launch_attention, the bounds tests of the gather kernel) was read before the first run.  The bf16 runs did expose a defect of the ORACLE: at head dim 32
the device rounds the probabilities of each 32-key tile relative to the running maximum of its online softmax, while oracle/unet2d_oai.py rounded
exp(w - global maximum).  flat_w64 (middle_block.1.att, 64 tokens) and lv3_w64 (input_blocks.7.1.att, 128 tokens) found it: 9.6e-4 and 9.5e-4 against the
bar of 1e-3, where the suite's other head-dim-32 bf16 run (1024 tokens, tests/test_conv2d_routes_gpu.py r3_bf16) sits at 6e-5.  The oracle now rounds tile by
tile as the kernel does (figures above; r3_bf16 stays at 6.1e-5).

That the sweep has teeth was checked once on three value-only edits (not committed), each run against the whole module:
  conv2d_in_kernel<T, 0> reads its LDS weights without the        caught by io43 and io43_dropped, fp32 and f32x3: first tensor over input_blocks.0.0 1.18, 50 of
  ``ci * 9`` stride (every input channel takes channel 0's taps)  50 over.  No other case has more than 2 input channels.  NOT caught by the sample-alone test: both runs
                                                                  are wrong alike
  ResBlock(down=True) adds the pooled ACTIVATION (p1) instead     caught by updown_ss in all three modes: input_blocks.2.0 0.77 (fp32, f32x3; 46 of 52 over) and 0.61
  of the pooled input (p2) as its residual                        (bf16, teacher-forced: that one tensor alone).  No other case has resblock_updown
  attention_kernel<T, D> writes head h's output to the columns    caught in fp32 by every case with more than one head (lv3, updown_ss, pool_hd8, io43, flat, tall,
  of head heads - 1 - h                                           mult21: the level's first .att 1.05 to 1.28) and by the four-shapes test; in f32x3 by the cases off head
                                                                  dim 32 (updown_ss, pool_hd8, flat, tall, mult21).  NOT caught by one_level, odd_h, one_row (one head: the
                                                                  edit changes nothing), by lv3 / io43 in f32x3 (head dim 32: attention_x3_kernel) or in bf16 (head dims 32
                                                                  and 64 run attention_mfma32_kernel), and cannot be there: the edited kernel does not run
"""
import pytest
import torch

import audiodiffuser_amd as A
from oracle import adm_sweep as S
from oracle import unet2d_oai as O
from test_adm import FP32_TIGHT, BF16_CONV_TOL, BF16_ATT_TOL
from test_gpu_parity import F32X3_TOL

assert S.FP32_TIGHT == FP32_TIGHT


def make(cid, dtype="fp32"):
    net = A.UNetModel.from_config(S.config(cid), compute_dtype=dtype)
    net.load_state_dict(S.weights(cid)[0], strict=True)
    return net.cuda()


def device_run(net, x, t, cl, cdp=0.0):
    """One device forward -> (output, {name: recorded tensor [B, C, H*W]}) on the host."""
    dev = torch.device("cuda", torch.cuda.current_device())
    kw = {} if cl is None else dict(classes=cl.cuda(), cond_drop_prob=cdp)
    with torch.no_grad():
        y = net(x.cuda(), t.cuda(), **kw).cpu()
    hd = net.native(dev)
    names = hd.tap_names()
    assert len(names) == len(set(names))
    return y, {k: hd.tap(k, x.shape[0], dev).cpu() for k in names}


def compare(tag, y, got, ref, bar):
    """The output and every device tap against the float64 run ``ref`` = (y64, taps, dist); ``bar(name)`` gives the tensor's bar.  -> {name: error}."""
    y64, t64, _ = ref
    errs, over = {}, []
    for k in list(got) + ["out"]:
        assert k == "out" or k in t64, f"{tag}: the device records {k!r} and the oracle has no tensor under that name"
        a, r = (y, y64) if k == "out" else (got[k], t64[k].reshape(got[k].shape))
        assert a.shape == r.shape, (tag, k, tuple(a.shape), tuple(r.shape))
        assert bool(torch.isfinite(a).all()), (tag, k, "not finite")
        errs[k] = S.rel(a, r)
        if not errs[k] <= bar(k):
            over.append((k, errs[k], bar(k)))
    worst = max(got, key=errs.get)
    print(f"{tag}: compared {len(errs)} tensors; worst {worst} {errs[worst]:.2e}, out {errs['out']:.2e}")
    assert len(errs) == len(got) + 1 >= 21
    if over:
        print(f"{tag}: FIRST tensor in walk order over its bar: {over[0][0]}: {over[0][1]:.3e} > {over[0][2]:.3e}; {len(over)} of {len(errs)} over")
        for k, e, b in over[:12]:
            print(f"    {k}: {e:.3e} (bar {b:.3e})")
    assert not over, (tag, over[0], len(over))
    return errs


def run_case(cid, dtype, bar):
    net = make(cid, dtype)
    worst = 0.0
    for rid in S.runs_of(cid):
        _, shape, seed, cdp = S.RUNS[rid]
        x, t, cl = S.inputs(S.config(cid), shape, seed)
        ref = S.float64_case(rid)
        y, got = device_run(net, x, t, cl, cdp)
        errs = compare(f"{rid} {dtype}", y, got, ref, (lambda k: bar(ref[2][k])))
        worst = max(worst, max(errs.values()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(S.FP32_CASES))
def test_fp32_every_tensor_vs_float64_oracle(cid):
    run_case(cid, "fp32", S.bar_of)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(S.FP32_CASES))
def test_f32x3_every_tensor_free_running_vs_float64_oracle(cid):
    worst = run_case(cid, "f32x3", lambda d: F32X3_TOL)
    assert worst > 1e-7, f"{cid}: worst tensor {worst:.2e}: the split-bf16 net computed what the exact route computes"


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(S.BF16_CASES))
def test_bf16_every_stored_tensor_teacher_forced(cid):
    cfg = S.config(cid)
    _, shape, seed = S.CASES[cid]
    net = make(cid, "bf16")
    x, t, cl = S.inputs(cfg, shape, seed)
    y, taps = device_run(net, x, t, cl)
    errs = {}
    with torch.no_grad():
        y_f = O.unet2d_forward(S.weights(cid)[0], cfg, x, t, storage="bf16", force=taps, errs=errs)
    conv = {k: e for k, e in errs.items() if not k.endswith(".att")}
    att = {k: e for k, e in errs.items() if k.endswith(".att")}
    wc, wa, eo = max(conv, key=conv.get), max(att, key=att.get), O.rel_l2(y, y_f)
    print(f"{cid} bf16: {len(errs)} tensors; worst conv {wc} {conv[wc]:.2e}, worst attention {wa} {att[wa]:.2e}, out vs forced {eo:.2e}")
    assert set(errs) == set(taps) and len(errs) >= 20 and float(y_f.abs().max()) > 1e-3
    over = {k: e for k, e in errs.items() if not e < (BF16_ATT_TOL if k.endswith(".att") else BF16_CONV_TOL)}
    assert not over and eo < BF16_CONV_TOL, (cid, eo, sorted(over.items(), key=lambda kv: -kv[1])[:8])


@pytest.mark.gpu
def test_one_handle_through_four_shapes_and_back():
    """Every change of shape re-plans the arena and the statistics slab; each result to its own float64 run, the last shape being the first again."""
    net = make(S.FOUR_SHAPES[0][0])
    for i, (cid, shape) in enumerate(S.FOUR_SHAPES):
        x, t, cl = S.inputs(S.config(cid), shape, 80 + i)
        ref = S.float64_shape(cid, shape, 80 + i)
        y, got = device_run(net, x, t, cl)
        compare(f"shape {i} {shape}", y, got, ref, lambda k: S.bar_of(ref[2][k]))


@pytest.mark.gpu
def test_a_sample_alone_equals_its_row_in_the_batch():
    """io43: sample 3 of the batch of 7, alone with its own time and label (per-sample bias rows, per-sample statistics)."""
    cfg = S.config("io43")
    _, shape, seed = S.CASES["io43"]
    net = make("io43")
    x, t, cl = S.inputs(cfg, shape, seed)
    yb, tb = device_run(net, x, t, cl)
    y1, t1 = device_run(net, x[3:4], t[3:4], cl[3:4])
    assert list(t1) == list(tb) and len(t1) >= 20
    errs = {k: S.rel(t1[k], tb[k][3:4]) for k in t1}
    errs["out"] = S.rel(y1, yb[3:4])
    worst = max(errs, key=errs.get)
    print(f"alone vs batch row: worst {worst} {errs[worst]:.2e}, out {errs['out']:.2e}")
    assert float(yb[3:4].abs().max()) > 1e-3 and errs[worst] <= FP32_TIGHT, (worst, errs[worst])
