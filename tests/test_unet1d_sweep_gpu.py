"""The HIP UNet1dBase held tensor by tensor to a float64 oracle over a sweep of constructor arguments and lengths.

Every other GPU test of the 1-D net builds a preset: channels 16 or 64 (widths 16 .. 256, all powers of two), 8 heads at head dim 32, 8 groups (32 once),
kernel multiplier 2, factors 2 and 4, window 8 / stride 2 / one waveform channel, the scaled skip and the bottleneck transformer.  The cases of
oracle/unet1d_sweep.py leave that point (T = config_tiny's structure):
  w24    channels 24, 3 heads, 2 x 448        widths 24 / 48 / 96: 6 / 12 / 24 chunks per row in gn_stats_kernel, groups of 6 / 12 channels (never fused statistics),
                                              n_pad > n, head dim 32 with 3 heads, levels 224 / 112 / 28 / 7, the non-MFMA to_out in bf16
  w48    channels 48, 6 heads, 3 x 512        widths 48 / 96 / 192, bf16 MFMA attention with 6 heads, attention_x3_kernel (f32x3 too)
  w32    channels 32, 3 x 512                 head dim 16, groups of 8 / 16 channels
  h64    channels 64, 4 heads, 3 x 1024       head dim 64 (attention_mfma32_kernel<64> on a 1-D handle); in bf16 the one-launch resblocks take the 64- and 16-token
                                              levels (no stored h1) and the one-launch transformer declines 4 heads (its nine tensors are recorded): asserted
  h2     channels 16, 2 heads, 2 x 320        head dim 32 at C = 64
  g1, g16  groups 1 (channels 16) / 16 (channels 32), 2 x 320   one group per sample: the group of a skip concat lies across both sources; groups of 4 / 8 channels
  g1s, g3s  groups 1 (channels 16) / 3 (channels 24, 3 heads), 2 x 512   levels 256 / 128 / 32 / 8: the straddling group (the only one; the middle one of three, 32 / 64
                                              channels over stored groups of 16 / 32) on the short levels too, where gn_norm_apply_kernel normalises (<= 32 rows, a power of two)
  km4    kernel_multiplier_downsample 4, 2 x 576       down convs of 4 f + 1 taps: 5 folded taps against kTapGroup = 3
  f83    factors [8, 3], blocks [3, 1], attentions [T, F], unscaled skip, no bottleneck transformer, attention_multiplier 4, 4 heads, 3 x 432
                                              odd factor (output_padding), factor 8 folded over 8 C channels, head dim 8, 27 / 9 rows.  (With the default 8 heads
                                              the 32-channel level has head dim 4, which no attention kernel serves and the constructor now refuses: the case runs 4 heads.)
  win16  num_filters 32, window 16, stride 4, 2 waveform channels, attention_multiplier 1, 2 x 176     the general to_in_kernel, to_out at its window limit
fp32: output and every recorded tensor, unsubsampled, against oracle/unet1d.py run in float64, bar FP32_TIGHT = 5e-5 (tests/test_oracle_unet1d_sweep.py holds
the fp32 oracle to a quarter of that bar of the float64 one: worst 1.4e-6).  bf16: every stored tensor teacher-forced against the bf16-storage oracle at the bars
of _bf16_tol.  f32x3 (all twelve cases): see "The split-bf16 mode" below.  Weights: generate_weights with the case's seed; every sample has its own t.

Defects the sweep found, both fixed here:
  * gn_stats_kernel / launch_gn_stats served only a power-of-two number of 16-byte chunks per row (the launcher's refusal, read in its code, not observed: "gn_stats:
    C/chunk must be a power of two <= 256"), which refuses the first forward of widths 24 / 48 / 96 / 192.  Any count up to 256 is served
    now; the 256 % chunks threads that would walk lane 0's rows again sit out.
  * resnet_groups = 1 (any odd count): "adf_net_forward: gn_finalize: a group straddles the two concatenated sources" at the first forward of g1 (observed on the
    device); launch_gn_norm_apply had the same refusal in its code (read, not observed: g1 has no short level).  gn_finalize_kernel and gn_norm_apply_kernel now sum
    such a group over both sources (the second scaled): g1 / g1s / g3s run the first, g1s / g3s the second.  The GEMM kernels that derive their GroupNorm table
    themselves decline the shape and get the table from gn_finalize: conv_gemm_rb_kernel did already, the pp route does now (route case pp128g1).
No bf16 case came near its bar by a defect of either side: the worst are one-launch resblocks (h64 mid.pre 5.3e-4 of 1e-3) and w24 up1.block1.h1 (4.1e-4 of 5e-4).

Measured on one MI355X, worst tensor (and the output); fp32 against 5e-5, bf16 against _bf16_tol (convs 5e-4, one-launch resblocks 1e-3, .att 1.5e-3), f32x3 against 2e-4:
  w24    fp32 up1.attn.att 1.5e-6 (6.4e-7)    bf16 up1.block1.h1 4.1e-4 (1.6e-7)        g1     fp32 up1.attn.att 1.2e-6 (1.1e-6)    bf16 up2.block0 1.3e-4 (6.2e-8)
  w48    fp32 up2.conv 1.1e-6 (7.6e-7)        bf16 up2.block0 1.0e-4 (1.0e-7)           g16    fp32 up1.attn.att 2.1e-6 (8.4e-7)    bf16 up1.block2.h1 1.1e-4 (7.9e-8)
         f32x3 up2.conv 1.7e-5 (1.3e-5)                                                  km4    fp32 up0.attn.att 2.0e-6 (8.3e-7)    bf16 up0.conv 1.5e-4 (5.8e-8)
  w32    fp32 up1.attn.n2 9.9e-7 (6.4e-7)     bf16 down2.attn 1.3e-4 (7.8e-8)           f83    fp32 up1.attn.n2 9.1e-7 (6.1e-7)     bf16 down0.block0.h1 2.4e-4 (4.3e-8)
  h64    fp32 up1.attn.f1 1.1e-6 (8.9e-7)     bf16 mid.pre 5.3e-4 (1.1e-7)              win16  fp32 up0.attn.att 1.0e-6 (6.1e-7)    bf16 up0.block1 1.3e-4 (7.3e-8)
  h2     fp32 up0.attn.n2 1.5e-6 (7.0e-7)     bf16 up2.block0 9.0e-5 (5.9e-8)            g1s    fp32 up0.attn.att 1.0e-6 (5.3e-7)    bf16 down1.block1 1.6e-4 (5.9e-8)
                                                                                         g3s    fp32 up0.attn.f1 1.1e-6 (8.2e-7)     bf16 down2.attn.f1 4.4e-4 (1.9e-7)
  one handle through 448 / 512 / 64 / 1088 / 448: at most 1.9e-6 (output 1.4e-6).  w24 bf16, sample 1 alone against its row of a batch of 3: bit-equal, all 71 tensors.
  ADF_FLAG_SEPARATE_GN_STATS: w48 1.1e-6 (7.4e-7), w32 9.8e-7 (6.1e-7).
The module before the split-bf16 tests: 33 tests in 13.0 s; no test over 3.2 s (the four children: 3.1 / 2.8 / 2.4 / 2.2 s wall each, most of it imports; limit 30 s, ten times that), every
in-process test under 0.3 s.

Route cases (child processes, tests/diag/gpu_unet1d_routes_report.py with ADF_GEMM_TRACE=1; census = (route, dtype, n, taps of segment 0, segments)):
  ws192 (fp32 and bf16): channels 32, multipliers [1, 6, 6, 6], factors [2, 8, 2], one block per level, no attention, 16 x 8192.  Level 0 is 192 wide at 2048 rows:
        16 * 16 = 256 tiles of 128 rows, the ws_min_m threshold.  The folded down conv (64 channels in, 3 taps: 3 (bf16) / 6 (fp32) weight slabs fit the 160 KB) takes ws
        with a partial second 128-column tile; the 192 -> 192 resblock convs do not fit (9 / 18 slabs) and take plain on 64-column tiles.  Level 1 (256 rows, B * rows =
        4096 = ADF_GEMM_KSPLIT_ROWS, 16 * 4 * 3 = 192 >= 128 tiles) takes the 64-row split-K tiles, level 2 (128 rows: 96 tiles) the 32-row ones.
        census, either dtype: ws (192, 3, 1); plain (192, 3, 1) (192, 3, 2) (64, 2, 1) (384, 2, 1) (1536, 2, 1) [the last three: transposed convs]; ksplit64 and ksplit32
        (192, 3, 1) (192, 3, 2).  fp32 worst up2.block0.h1 1.5e-6 (output 1.0e-6); bf16 worst up0.block0.h1 8.6e-5 (4.4e-8).
  pp384 (bf16, ADF_GEMM_PP=2): channels 64, multipliers [1, 6], factors [2], 44 x 512: 384 channels at 128 rows; 44 * 12 = 528 >= 512 blocks keeps 128-row tiles and
        44 * 3 = 132 >= 128 tiles meets pp_eligible's count.  census: pp (384, 3, 1) (384, 3, 2) [conv2 with its identity residual as a second segment]; plain (384, 3, 1)
        [conv1 over the 768-channel concat: more than the 512 channels of pp's GroupNorm table] (128, 2, 1).  Worst down0.block0 9.6e-5 (output 6.0e-8).
  pp128g1 (bf16, ADF_GEMM_PP=2): channels 64, multipliers [1, 2], factors [2], resnet_groups 1, 32 x 2048: 128 channels at 512 rows, 32 * 4 = 128 tiles of 128 rows.  The
        concat conv1 (128 + 128 channels, its one group across both sources) is declined by conv_gemm_rb_kernel's host check and takes pp with the table from gn_finalize.
        census: pp (128, 3, 1) (128, 3, 2), plain (128, 2, 1).  Worst mid.pre 7.0e-5 (output 1.1e-7).
  Not reachable off the presets, by the gates: rb / rbx3 (rb_shape_ok: n of 128 or 256 only, an even number of 64-channel blocks), up (cin 256 / 128 and cout 256 / 128 / 64
  only), pp in fp32 (bf16 only), ws for a 3-tap conv wider than 6 weight slabs of 128 columns (so no off-preset resblock conv: 192 channels need 9).

The split-bf16 mode (compute_dtype="f32x3"), launch by launch.  ONE device run per case is held two ways (gpu_helpers.sweep_x3_report):
  forced   every recorded tensor teacher-forced against oracle/unet1d.py storage="f32x3" (the same hi / lo split of every operand of every split product, three
           products, float64 accumulation) in relative L2, the output from the device's last tensor: bar X3_LAUNCH_TOL = 2.8e-6, half the smallest figure a truncating
           split leaves on any GEMM-fed tensor, derived on the CPU by tests/test_oracle_unet1d_x3.py and never fitted to a device figure;
  free     the same tensors free-running against the float64 oracle, max norm: bar F32X3_TOL = 2e-4 as before, and max > 1e-7 (not silently the exact-fp32 route).
The oracle restates launch_attention_x3's and launch_to_out's gates: h64 / w32 / f83 (head dim 64 / 16 / 8) record their .att from the fp32 vector kernel, asserted by
name (X3_ATT), and hold it to the same launch bar, so a split on the wrong side of a gate is 1e-5 against 2.8e-6; h64 alone runs to_out_x3_kernel (64 filters).
Measured on one MI355X, worst forced tensor (forced output) | worst free-running tensor (free-running output):
  w24    mid.post.h1 1.6e-6 (9.0e-8) | up1.attn.att 3.0e-5 (1.1e-5)        g16    up1.block2.h1 8.7e-7 (1.2e-7) | up0.block1.h1 2.1e-5 (1.5e-5)
  w48    down2.block0.h1 8.9e-7 (1.3e-7) | up0.conv 1.9e-5 (1.5e-5)        g1s    up1.block2.h1 7.8e-7 (8.5e-8) | up0.attn.att 2.6e-5 (1.1e-5)
  w32    mid.pre.h1 1.0e-6 (1.0e-7) | up1.attn.n2 2.0e-5 (1.2e-5)          g3s    up0.block0.h1 1.1e-6 (1.1e-7) | up0.attn.ln 2.3e-5 (1.5e-5)
  h64    up0.block0.h1 8.4e-7 (8.0e-8) | up0.attn.n2 1.7e-5 (1.5e-5)       km4    down1.block0.h1 1.2e-6 (9.6e-8) | up0.attn.att 3.2e-5 (1.7e-5)
  h2     mid.post.h1 1.2e-6 (9.5e-8) | mid.post.h1 2.5e-5 (1.8e-5)         f83    up1.block2.h1 8.0e-7 (7.8e-8) | up1.attn.n2 2.2e-5 (1.8e-5)
  g1     up2.block0.h1 8.8e-7 (8.6e-8) | up0.attn.att 2.4e-5 (2.2e-5)      win16  mid.pre.h1 1.2e-6 (1.1e-7) | up0.attn.ln 1.5e-5 (1.2e-5)
  every in-process f32x3 case 0.04 .. 0.33 s.  The attention edge sweep (16 token counts on one handle, 2.4 s): worst forced tensor 1.3e-6 (output 9.6e-8), worst
  forced .att 1.6e-7 .. 4.0e-7 on attention_x3_kernel and 6.7e-7 at 1025 tokens (fp32 vector kernel); free-running at most 2.4e-5.  No token count was refused.
Outcome against the aim "the device's worst forced figure is at most half the bar (1.4e-6)": missed by one tensor, w24 mid.post.h1 1.57e-6 (every other case <= 1.2e-6,
the presets of tests/test_gpu_parity.py <= 1.1e-6).  The worst tensor of EVERY case is a conv1 output (".h1"), so that launch was read: its A operand is silu(a x + b)
with GroupNorm folded to a per-channel affine in fp32 (adf_common.h gn_affine_finish: A = rstd * gamma, Bc = beta - mean * A; adf_gemm.h store_lds: packed fp32 FMA,
hardware exp2 and rcp), where the oracle keeps GroupNorm and SiLU in float64.  Restating that prologue in fp32 on the CPU (fp32 A and Bc, one FMA, fp32 SiLU) moves the
forced .h1 tensors of w24 / h2 by 5e-7 .. 9e-7 from the float64 prologue (measured, not committed): the whole device figure is fp32 arithmetic in front of the split,
amplified by the cancellation inside the conv, not an arithmetic difference of the split products (those tensors whose operand is a stored tensor -- down / up convs,
qkv, x1, f1 -- sit at 1e-7 .. 4e-7).  The statistics themselves are fp32 too: gn_stats_kernel sums each channel in fp32 and joins the row lanes with fp32 LDS atomics
(adf_kernels.hip:40-45), whose order changes from run to run, so the .h1 figures do: a second run of the whole suite gave w24 7.9e-7 (down0.block0), g1 1.2e-6, h2 9.8e-7,
attention at 7 / 33 tokens 1.56e-6 / 1.36e-6 where the table above and the attention line are the first run; the largest figure of either run is 1.57e-6, 56 % of the bar.
It was NOT added to the oracle: the hardware exp2 / rcp and the order of the fold's roundings cannot be restated bit for bit, so
a second fp32 prologue would only trade one few-ulp difference for another.  No defect of the kernels was found; the bar stays 2.8e-6.

Route cases of the mode (child processes; `one_pass`: the report's net runs twice and both passes print the same lines):
  ws192_f32x3   the ws192 configuration, 16 x 8192.  decide_conv_gemm closes the weight-stationary kernel to the mode (ws_ok ... !x3) and rbx3 needs n = 128 / 256, so the
        five level-0 convs (2048 rows: the folded down conv, conv1 / conv2 of the down and the up resblock, conv2 once with an identity residual and once with the 1x1
        K segment over 192 + 192 channels) are conv_gemm_kernel<f32x3_t> on 128 x 64 tiles (n_pad = 192 is no multiple of 128, so tn = 64: 16 * 16 * 3 = 768 >= 512
        blocks keep 128 rows); the factor-8 transposed conv (n = 1536 at 257 rows: 3 * 16 * 12 = 576 blocks) is the one 128 x 128 tile; level 1 (16 * 256 = 4096 rows =
        ADF_GEMM_KSPLIT_ROWS, 6 K chunks of 32 channels >= 4, 16 * 4 * 3 = 192 >= 128 tiles) is launch_ksplit<f32x3_t, 2, 2>, level 2 (96 tiles) <1, 1>, both with n = 192
        = three 64-column / six 32-column tiles.  census: plain (192, 3, 1) (192, 3, 2) (64, 2, 1) (384, 2, 1) (1536, 2, 1); ksplit64 and ksplit32 (192, 3, 1) (192, 3, 2);
        nothing on ws or rbx3.  Measured: worst forced up2.block0.h1 7.3e-7 (output 1.1e-7); free-running up0.conv 1.4e-5 (1.1e-5).
  rbx3_small (ADF_GEMM_RBX3=2: from 32 tiles on): channels 64, multipliers [1, 2, 4], factors [2, 2], one block per level, no attention, L = 2048: 128 channels at 512
        rows, 256 at 256 rows.  The shape the issue proposed (batch 16 and 8) does not reach the kernel where it was meant to: the split-K route is asked BEFORE rbx3
        (decide_conv_gemm step 3) and takes every conv of a level with B * rows <= ADF_GEMM_KSPLIT_ROWS = 4096, i.e. the 256-row level at batch 16 and both levels at
        batch 8.  The nearest batches that pass, switches untouched:
        batch 17  rb_tiles: 17 * (512 / 256) * (128 / 128) = 34 and 17 * (256 / 256) * (256 / 128) = 34 tiles of 256 rows, >= 32: conv_gemm_rbx3_kernel<2> on both
                  levels, all 16 conv launches of a pass (17 * 256 = 4352 rows > 4096).  Raw segment 0 four times: the two folded down convs and both transposed convs
                  in the x3 three-tap form (256 -> 2 x 128 columns, n = 256 / 256, and 128 -> 2 x 64); nseg = 2 with a two-source 1x1 segment (256 + 256, 128 + 128);
                  res = 1; two-source conv1.
        batch 9   level 0: 9 * 2 = 18 tiles of 256 rows < 32 <= 9 * 4 = 36 of 128 rows: conv_gemm_rbx3_kernel<1> (9 * 512 = 4608 rows > 4096), six launches with the
                  same forms at n = 128.  Level 1 (2304 rows) goes to split-K -- <1> at n = 256 needs 2048 <= B * rows < 4096, which split-K always takes -- except the
                  three-tap transposed conv, which only the resblock kernel serves (phase-major columns, asked first): the one <1> launch at n = 256 (18 / 36 tiles).
        (The trace does not print the template argument: the arithmetic above is asserted on the traced B, rows and n.  The existing 16384-long c2 / c3 test of
        tests/test_gpu_parity.py runs <2> only -- 8 * 4 * 2 = 64 tiles at its shortest rbx3 level -- so batch 9 is the suite's one run of <1>.)
        Measured: batch 17 worst forced up0.block0.h1 8.3e-7 (output 9.5e-8), free-running up0.conv 1.8e-5 (1.4e-5); batch 9 up1.block0.h1 7.6e-7 (9.4e-8), up0.block0 1.5e-5 (1.8e-5).
  The three children: 4.7 / 2.7 / 2.5 s wall each (limits 60 / 30 / 30 s).  The module with them: 48 tests in 28.3 s; its f32x3 part (12 + 3 + 1 tests) 15.6 s.

Teeth of the mode's tests, checked once on three value-only edits (no address or control-flow change; not committed), each against every f32x3 test of this module and
of tests/test_gpu_parity.py.  "old" = the free-running 2e-4 comparison alone, which was all the suite had:
  split_bf16x4 truncating instead of rounding          caught by all twelve sweep cases (first over: down0.conv 1.2e-5, 30 .. 55 tensors of 43 .. 71), ws192 (22 of 23),
                                                       rbx3_small batch 9 (down1.conv on split-K 1.2e-5) and batch 17 (the output alone, 2.6e-5: conv_gemm_rbx3_kernel
                                                       splits in its own prologue, not through split_bf16x4; to_out_x3_kernel does), the attention sweep at its first
                                                       count, and all five f32x3 parity tests (worst 1.4e-5 .. 2.7e-5).  old: blind everywhere -- the worst free-running
                                                       figure of any case was 8.0e-5.
  conv_gemm_kernel<f32x3_t> without a_lo b_hi on segment 1   caught by w24, h2, g1, g16, g1s, km4, f83, win16, ws192 and the attention sweep (first over: up0.block0 1.4e-3 ..
                                                       1.7e-3, 1 .. 6 tensors); not by w48, w32, h64, g3s and rbx3_small, whose 1x1 residual segments run on the split-K or
                                                       the resblock kernel.  old: caught too where the kernel runs (free-running 2.5e-3 .. 4.5e-3), but of the sweep only
                                                       w48 ran the mode before, which does not.
  attention_x3_kernel feeding P as hi only             caught by w24, w48, h2, g3s (first over: down1.attn.att 4.6e-4 .. 7.0e-4, 5 tensors), the attention sweep (9.4e-4)
                                                       and the three config-3 parity tests; the other cases have no split attention.  old: caught too (w48 1.4e-3).

That the sweep has teeth was checked once on four value-only edits (not committed), each against every case of test_every_tensor_vs_oracle and the separate-statistics test:
  gn_stats_kernel summing gs - 1 channels per group        caught by all 23 (first tensor over: w24 down0.block0.h1 0.12, w48 0.059, g1 down1.block0.h1 0.014, ...)
  store guard n < a.n -> n < a.n_pad (conv_gemm_kernel)    caught by w24 fp32 (down0.conv 0.85, 70 of 71 over) and w24 bf16 (up2.block0.h1 0.48); no other case has n_pad > n on that kernel
  head offset hh * (C / 8) in attention_kernel              caught by w24, w48, h64, h2, f83 in fp32 (first .att 0.85 .. 0.93), f83 bf16 (0.62 / 0.65 of 1.5e-3) and w48 separate statistics
  odd-factor transposed conv without its output_padding row caught by f83 fp32 (up0.conv 0.43, 18 of 43 over) and f83 bf16 (up0.conv 0.15 of 5e-4)
  gn_straddle_sums without the skip scale on the second source's sum   caught by g1, g1s, g3s in fp32 (up0.block0.h1 0.032 / 0.012 / 0.010, 31 of 71 over) and bf16
                                                            (up0.block1.h1 0.042, 0.025; g3s up2.block0.h1 0.011 of 5e-4); pp128g1 was not run against an edit: without the
                                                            decline in decide_conv_gemm the pp kernel would read a statistics group past the sample's own, so that edit stayed off the device
Not attempted: a factor of 1 (the reference's plain Conv1d(k = 3) is not built; the constructor refuses it).
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
import gpu_helpers as R
from gpu_helpers import assert_gemm_route_trace, gemm_trace_lines
from oracle import unet1d as O
from oracle import unet1d_sweep as SW
from test_gpu_parity import FP32_TIGHT, F32X3_TOL, _bf16_tol

X3_LAUNCH_TOL = SW.X3_LAUNCH_TOL                # per launch, teacher-forced, relative L2 (derived in tests/test_oracle_unet1d_x3.py)
# the recorded attention outputs of the three cases whose head dim (64 / 16 / 8) keeps attention_x3_kernel out: fp32 vector kernel, still within the launch bar
X3_ATT = {"h64": ["down1.attn.att", "down2.attn.att", "mid.attn.att", "up0.attn.att", "up1.attn.att"],
          "w32": ["down1.attn.att", "down2.attn.att", "mid.attn.att", "up0.attn.att", "up1.attn.att"],
          "f83": ["down0.attn.att", "up1.attn.att"]}

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "tests", "diag", "gpu_unet1d_routes_report.py")

PRESET_WIDTHS = {16, 32, 64, 128, 256}          # every channel count of c1 / c2 / c3
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


def check(rep, mode, tag, expect_names=None):
    """The bars of the module on everything a report compared; prints the figures before it asserts."""
    taps = rep["taps"]
    worst = max(taps, key=taps.get)
    print(f"{tag} {mode}: tensors {len(taps)} worst {worst} {taps[worst]:.3e} out {rep['out']:.3e} device s {rep['device_seconds']:.2f} "
          f"oracle s {rep['oracle_seconds']:.2f}")
    assert not rep["missing"], f"{tag}: the device records tensors the oracle has no name for: {rep['missing']}"
    assert len(taps) == len(rep["names"]) > 10 and rep["ref_absmax"] > 1e-3
    if expect_names is not None:
        assert rep["names"] == expect_names, (tag, rep["names"], expect_names)
    if mode == "f32x3":
        # one device run held two ways: every launch teacher-forced against the split-bf16 oracle (relative L2), and free-running against float64 (max norm)
        free = rep["free"]
        wf = max(free, key=free.get)
        print(f"{tag} f32x3: free-running worst {wf} {free[wf]:.3e} out {rep['free_out']:.3e}")
        over = {k: e for k, e in taps.items() if not e < X3_LAUNCH_TOL}
        if over:
            first = next(k for k in rep["names"] if k in over)
            print(f"{tag} f32x3: FIRST tensor in walk order over {X3_LAUNCH_TOL:.1e} (forced): {first} {over[first]:.3e}; {len(over)} of {len(taps)} over")
        assert not over and rep["out"] < X3_LAUNCH_TOL, (tag, rep["out"], sorted(over.items(), key=lambda kv: -kv[1])[:8])
        over = {k: e for k, e in free.items() if not e < F32X3_TOL}
        assert len(free) == len(taps) and not over and rep["free_out"] < F32X3_TOL, (tag, rep["free_out"], sorted(over.items(), key=lambda kv: -kv[1])[:8])
        assert max(free.values()) > 1e-7          # (not silently the exact-fp32 route)
        return
    if mode == "bf16":
        over = {k: (e, _bf16_tol(k, taps)) for k, e in taps.items() if not e < _bf16_tol(k, taps)}
        assert not over and rep["out"] < _bf16_tol("out", taps), (tag, rep["out"], sorted(over.items(), key=lambda kv: -kv[1][0])[:8])
        return
    assert mode == "fp32"
    bar = FP32_TIGHT
    over = {k: e for k, e in taps.items() if not e < bar}
    if over:
        first = next(k for k in rep["names"] if k in over)
        print(f"{tag} {mode}: FIRST tensor in walk order over {bar:.1e}: {first} {over[first]:.3e}; {len(over)} of {len(taps)} over")
    assert not over and rep["out"] < bar, (tag, rep["out"], sorted(over.items(), key=lambda kv: -kv[1])[:8])


def run_case(cid, mode, flags=0, tag=None):
    cfg, shape, seed, _ = SW.CASES[cid]
    w, w64 = SW.weights(cid)
    x, t = SW.inputs(cfg, shape, seed)
    net = R.sweep_make(cfg, w, mode, flags)
    if mode == "bf16":
        rep = R.sweep_bf16_report(cfg, w, x, t, net)
    elif mode == "f32x3":
        rep = R.sweep_x3_report(cfg, w, w64, x, t, net, oracle=SW.float64_case(cid))
    else:
        rep = R.sweep_fp32_report(cfg, w, w64, x, t, net, oracle=SW.float64_case(cid))
    check(rep, mode, tag or cid)
    return rep


@pytest.mark.parametrize("cid,mode", [(c, m) for c, v in SW.CASES.items() for m in v[3]])
def test_every_tensor_vs_oracle(cid, mode):
    rep = run_case(cid, mode)
    names = set(rep["names"])
    if mode == "bf16" and cid == "h64":
        # 256 channels at 64 and 16 tokens with 4 heads: the one-launch resblocks take them (no stored h1), the one-launch transformer must not
        assert "down1.block0.h1" not in names and "down2.block0.h1" not in names and "mid.pre.h1" not in names
        assert {"down1.attn.qkv", "down2.attn.ln", "mid.attn.n2", "up0.attn.att", "up1.attn.f1"} <= names
    else:
        assert {k for k in names if k.endswith(".h1")} and (not any(SW.CASES[cid][0].attentions) or {k for k in names if k.endswith(".attn.att")})
    if mode == "f32x3":
        # where attention_x3_kernel must and must not run (head dim 64 / 16 / 8 fall back to the fp32 vector kernel): the oracle restates launch_attention_x3's
        # gate, so a split applied on the wrong side of it is 1e-5 on that .att against the launch bar check() has just held it to
        cfg = SW.CASES[cid][0]
        att = {k: rep["shapes"][k] for k in rep["names"] if k.endswith(".attn.att")}
        split = {k for k, (_, c, n) in att.items() if O.x3_attention(c // cfg.attention_heads, n, c)}
        assert att and set(att) <= set(rep["taps"])
        assert split == (set(att) if cid in ("w24", "w48", "h2", "g3s") else set()), (cid, sorted(split), att)
        if cid in X3_ATT:
            assert list(att) == X3_ATT[cid], (cid, list(att))


def test_one_handle_through_five_lengths():
    """448, 512, 64, 1088, 448 on ONE w48 fp32 net: every change of length evicts or rebuilds a plan at widths 48 / 96 / 192; each result to its own oracle."""
    cfg = SW.CASES["w48"][0]
    w, w64 = SW.weights("w48")
    net = R.sweep_make(cfg, w, "fp32")
    names = None
    for i, l in enumerate((448, 512, 64, 1088, 448)):
        x, t = SW.inputs(cfg, (3, l), 60 + i)
        rep = R.sweep_fp32_report(cfg, w, w64, x, t, net)
        check(rep, "fp32", f"w48 length {i} = {l}", names)
        names = rep["names"]


def test_a_sample_alone_equals_its_row_of_a_batch_of_three():
    """w24 in bf16 at 448: sample 1 of a batch of 3, run alone with its own time, bit for bit (output and every stored tensor)."""
    cfg, _, seed, _ = SW.CASES["w24"]
    w, _ = SW.weights("w24")
    net = R.sweep_make(cfg, w, "bf16")
    x, t = SW.inputs(cfg, (3, 448), seed)
    yb, gb, names = R.sweep_device_run(net, x, t)
    y1, g1, names1 = R.sweep_device_run(net, x[1:2].contiguous(), t[1:2].contiguous())
    assert names1 == names
    diff = {k: SW.rel(g1[k], gb[k][1:2]) for k in names}
    diff["out"] = SW.rel(y1, yb[1:2])
    worst = max(diff, key=diff.get)
    print("alone vs row 1 of 3: worst", worst, diff[worst], "unequal tensors", sorted(k for k, d in diff.items() if d > 0)[:10])
    assert torch.equal(y1, yb[1:2]) and all(torch.equal(g1[k], gb[k][1:2]) for k in names), (worst, diff[worst])


@pytest.mark.parametrize("cid", ["w48", "w32"])
def test_separate_statistics_pass_for_every_tensor(cid):
    """ADF_FLAG_SEPARATE_GN_STATS: no conv epilogue reduces statistics, every statistics tensor comes from gn_stats_kernel (6 to 48 chunks per row at w48)."""
    run_case(cid, "fp32", _lib.FLAG_SEPARATE_GN_STATS, cid + " separate statistics")


# ------------------------------------------------------------------ route cases (child processes)
# case -> (extra environment of the child, its time limit in seconds)
# (measured 3.1 / 2.6 / 2.2 s wall per child, most of it the imports: 30 s is ten times that; ws192_f32x3 5.9 s with its two float64 oracle runs: 60 s)
CHILD = {"ws192_f32x3": ({}, 60), "rbx3_small_b17_f32x3": ({"ADF_GEMM_RBX3": "2"}, 30), "rbx3_small_b9_f32x3": ({"ADF_GEMM_RBX3": "2"}, 30),
         "ws192_fp32": ({}, 30), "ws192_bf16": ({}, 30), "pp384_bf16": ({"ADF_GEMM_PP": "2"}, 30), "pp128g1_bf16": ({"ADF_GEMM_PP": "2"}, 30)}


@functools.lru_cache(maxsize=None)
def child(case):
    assert not _DEVICE_TROUBLE, f"not started: an earlier child of this module faulted or hung ({_DEVICE_TROUBLE[0]})"
    env, limit = CHILD[case]
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, REPORT, case], capture_output=True, text=True, env=dict(os.environ, ADF_GEMM_TRACE="1", **env), timeout=limit)
    except subprocess.TimeoutExpired:
        _DEVICE_TROUBLE.append(f"{case}: no result within {limit} s")
        raise
    if r.returncode != 0:
        _DEVICE_TROUBLE.append(f"{case}: exit status {r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    lines = gemm_trace_lines(r.stderr)
    assert rep["case"] == case and lines
    print(case, "child wall s", round(time.time() - t0, 1))
    return rep, lines, r.stderr


def one_pass(lines):
    """The report runs the net twice (the plan is built on the first call): both passes take the same routes; -> the lines of one."""
    h = len(lines) // 2
    assert len(lines) == 2 * h and lines[:h] == lines[h:]
    return lines[:h]


def route_of(l):
    return "ksplit%d" % l["tm"] if l["route"] == "ksplit" else l["route"]


def census(lines, dtype):
    """{(route, dtype, n, taps of segment 0, segments)}"""
    return {(route_of(l), dtype, l["n"], l["taps"], l["nseg"]) for l in lines}


def need(cen, required):
    missing = sorted(set(required) - cen)
    print("census:", sorted(cen))
    assert not missing, f"no launch of this case ran as {missing}; the census was {sorted(cen)}"


def off_preset(lines, route):
    return [l for l in lines if route_of(l) == route and (l["n"] not in PRESET_WIDTHS or l["c0"] not in PRESET_WIDTHS)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_route_ws_plain_and_both_split_k_tiles_at_width_192(dtype):
    """ws192 of the module docstring: the weight-stationary kernel at its tile threshold with a partial second N tile, the plain kernel on 64-column tiles and both
    split-K tile sizes, all at 192 channels; values at the module's bars."""
    rep, lines, stderr = child("ws192_" + dtype)
    assert_gemm_route_trace("ws192_" + dtype, stderr)
    req = {("ws", dtype, 192, 3, 1), ("plain", dtype, 192, 3, 1), ("plain", dtype, 192, 3, 2), ("ksplit64", dtype, 192, 3, 2), ("ksplit32", dtype, 192, 3, 2)}
    need(census(lines, dtype), req)
    for route in ("ws", "plain", "ksplit64", "ksplit32"):
        assert off_preset(lines, route), route
    ws = [l for l in lines if l["route"] == "ws"]
    assert all(l["n_pad"] == 192 and l["tn"] == 128 and l["B"] * -(-l["mrows"] // 128) == 256 for l in ws), ws      # at the threshold, second N tile partial
    check(rep, dtype, "ws192")


def test_route_pp_at_width_384():
    """pp384 of the module docstring: the persistent LDS-DMA kernel at 384 channels on 128-row tiles, 132 tiles against the threshold of 128 (ADF_GEMM_PP=2)."""
    rep, lines, stderr = child("pp384_bf16")
    assert_gemm_route_trace("pp384_bf16", stderr)
    need(census(lines, "bf16"), {("pp", "bf16", 384, 3, 1), ("pp", "bf16", 384, 3, 2)})
    pp = off_preset(lines, "pp")
    assert pp and all(l["tm"] == 128 and l["B"] * (l["mrows"] // 128) * (l["n_pad"] // 128) == 132 for l in pp), pp
    check(rep, "bf16", "pp384")


def test_route_pp_with_one_group_per_sample_takes_its_table_from_gn_finalize():
    """pp128g1 of the module docstring: a concat conv1 whose single GroupNorm group lies across both sources on the persistent LDS-DMA kernel, which cannot derive
    that table itself (decide_conv_gemm's plan sends it to gn_finalize); values at the module's bars."""
    rep, lines, stderr = child("pp128g1_bf16")
    assert_gemm_route_trace("pp128g1_bf16", stderr)
    need(census(lines, "bf16"), {("pp", "bf16", 128, 3, 1), ("pp", "bf16", 128, 3, 2)})
    cat = [l for l in lines if l["route"] == "pp" and l["c1"] == 128 and l["ab"] == 1]
    assert cat and all(l["tm"] == 128 and l["B"] * (l["mrows"] // 128) == 128 for l in cat), cat
    check(rep, "bf16", "pp128g1")


# ------------------------------------------------------------------ the split-bf16 mode's own routes
def test_route_f32x3_plain_128_row_tiles_and_both_split_k_tiles_at_width_192():
    """ws192_f32x3 of the module docstring: with the weight-stationary kernel closed to the mode every level-0 conv is conv_gemm_kernel<f32x3_t> on 128-row
    tiles (64 columns at n = 192, 128 columns at the factor-8 transposed conv), levels 1 and 2 launch_ksplit<f32x3_t> on 64 x 64 and 32 x 32 tiles."""
    rep, lines, stderr = child("ws192_f32x3")
    assert_gemm_route_trace("ws192_f32x3", stderr)
    lines = one_pass(lines)
    cen = census(lines, "f32x3")
    need(cen, {("plain", "f32x3", 192, 3, 1), ("plain", "f32x3", 192, 3, 2), ("plain", "f32x3", 1536, 2, 1), ("plain", "f32x3", 384, 2, 1), ("plain", "f32x3", 64, 2, 1),
               ("ksplit64", "f32x3", 192, 3, 1), ("ksplit64", "f32x3", 192, 3, 2), ("ksplit32", "f32x3", 192, 3, 1), ("ksplit32", "f32x3", 192, 3, 2)})
    assert {route_of(l) for l in lines} == {"plain", "ksplit64", "ksplit32"}, sorted({route_of(l) for l in lines})        # no ws, no rbx3
    lvl0 = [l for l in lines if l["route"] == "plain" and l["mrows"] == 2048]
    assert len(lvl0) == 5 and all(l["n"] == 192 and (l["tm"], l["tn"]) == (128, 64) and l["flat"] == 0 for l in lvl0), lvl0
    assert any(l["c0"] == 64 and l["ab"] == 0 for l in lvl0) and any(l["c1"] == 192 and l["ab"] == 1 for l in lvl0) and any(l["res"] == 1 for l in lvl0)
    assert [(l["tm"], l["tn"]) for l in lines if l["route"] == "plain" and l["n"] == 1536] == [(128, 128)]
    for route in ("plain", "ksplit64", "ksplit32"):
        assert off_preset(lines, route), route
    assert all(l["mrows"] == 256 and l["n_pad"] == 192 for l in lines if route_of(l) == "ksplit64")
    assert all(l["mrows"] == 128 and l["n_pad"] == 192 for l in lines if route_of(l) == "ksplit32")
    check(rep, "f32x3", "ws192")


@pytest.mark.parametrize("batch", [17, 9])
def test_route_rbx3_both_tile_heights_on_a_small_net(batch):
    """rbx3_small of the module docstring (ADF_GEMM_RBX3=2: from 32 tiles on): conv_gemm_rbx3_kernel<2> on both levels at batch 17, <1> on the 128-wide level at
    batch 9; every form of the kernel's K-block table among the launches."""
    case = "rbx3_small_b%d_f32x3" % batch
    rep, lines, stderr = child(case)
    assert_gemm_route_trace(case, stderr)
    lines = one_pass(lines)
    rb = [l for l in lines if l["route"] == "rbx3"]
    raw = [l for l in rb if l["ab"] == 0 and l["act"] == 0]
    print(case, "rbx3 launches", len(rb), "of", len(lines), "raw", len(raw))
    if batch == 17:
        assert len(rb) == len(lines) == 16 and {(l["mrows"], l["n"]) for l in rb} == {(512, 128), (256, 256)}, sorted({(route_of(l), l["mrows"], l["n"]) for l in lines})
        assert all(l["B"] * (l["mrows"] // 256) * (l["n"] // 128) == 34 for l in rb)                 # >= 32 tiles of 256 rows: <2>
        # raw segment 0: the two folded down convs and the two three-tap transposed convs (256 -> 2 x 128 and 128 -> 2 x 64 columns)
        assert [(l["c0"], l["n"], l["mrows"]) for l in raw] == [(128, 128, 512), (256, 256, 256), (256, 256, 256), (128, 128, 512)], raw
    else:
        assert len(rb) == 7 and {(l["mrows"], l["n"]) for l in rb} == {(512, 128), (256, 256)}, sorted({(route_of(l), l["mrows"], l["n"]) for l in lines})
        assert all(l["B"] * (l["mrows"] // 256) * (l["n"] // 128) == 18 and l["B"] * (l["mrows"] // 128) * (l["n"] // 128) == 36 for l in rb)      # 18 < 32 <= 36: <1>
        # 9 * 256 rows <= ADF_GEMM_KSPLIT_ROWS: the split-K kernel is asked first and takes the 256-wide level, but for the three-tap transposed conv (phase-major
        # columns: the resblock kernel alone serves it) -- the one <1> launch at n = 256
        assert {route_of(l) for l in lines if l["mrows"] == 256 and l not in rb} == {"ksplit64"} and len(lines) == 16
        assert [(l["c0"], l["n"], l["mrows"]) for l in raw] == [(128, 128, 512), (256, 256, 256), (128, 128, 512)], raw
    assert all(l["nseg"] == 1 and l["res"] == 0 and l["taps"] == 3 for l in raw)
    assert any(l["nseg"] == 2 and l["s1c0"] > 0 and l["s1c1"] > 0 for l in rb), "no 1x1 residual K segment over two sources"
    assert any(l["res"] == 1 for l in rb) and any(l["c1"] > 0 and l["ab"] == 1 for l in rb)
    check(rep, "f32x3", case)


ATT_TOKENS = (7, 31, 32, 33, 63, 65, 96, 129, 255, 256, 257, 288, 513, 1000, 1024, 1025)
ATT_REFUSED = ()                # token counts the net refuses with an AdfError (none)


def test_split_attention_through_every_workgroup_shape_on_one_handle():
    """attention_x3_kernel at its edges: 64 channels in 2 heads, batch 3 (6 pairs), one level, tokens = L / 4.  Up to 256 tokens <4, false>: 1 / 2 / 4 waves per
    pair and 4 / 2 / 1 pairs per workgroup (6 pairs leave the last workgroup of 4 half filled), partial key and query tiles; 257 .. 1024 <8, true>: K from global,
    2 to 4 query tiles per wave with a last group that is not full; 1025: the fp32 vector kernel.  Each count held launch by launch to the split-bf16 oracle,
    whose gate restates the launcher's."""
    cfg = SW._t(64, multipliers=[1, 1], factors=[2], num_blocks=[1], attentions=[True], attention_heads=2, use_attention_bottleneck=False)
    w = SW.generate_weights(cfg, seed=61)
    w64 = {k: v.double() for k, v in w.items()}
    net = R.sweep_make(cfg, w, "f32x3")
    refused, worst = [], {}
    t0 = time.time()
    for i, n in enumerate(ATT_TOKENS):
        x, t = SW.inputs(cfg, (3, 4 * n), 70 + i)
        try:
            rep = R.sweep_x3_report(cfg, w, w64, x, t, net)
        except Exception as e:
            if type(e).__name__ != "AdfError" or R.SWEEP_TROUBLE:
                raise
            print(f"{n} tokens refused: {e}")
            refused.append(n)
            continue
        att = [k for k in rep["names"] if k.endswith(".attn.att")]
        assert att == ["down0.attn.att", "up0.attn.att"] and all(rep["shapes"][k] == [3, 64, n] for k in att), (n, att)
        assert O.x3_attention(32, n, 64) == (n <= 1024)
        worst[n] = max(rep["taps"][k] for k in att)
        check(rep, "f32x3", f"attention at {n} tokens")
    print("worst forced .att per token count:", {n: f"{e:.2e}" for n, e in worst.items()}, "wall s", round(time.time() - t0, 1))
    assert tuple(refused) == ATT_REFUSED, refused
