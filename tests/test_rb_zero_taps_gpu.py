"""GPU: the raw launches of the resblock conv kernel (csrc/adf_gemm_rb.h) with their structurally zero sub-steps left out (ADF_RB_ZSKIP=1, the default) against
the same launches with every block three-tap (ADF_RB_ZSKIP=0).  A folded strided conv has a zero third tap from folded channel C on (two-tap K blocks), the
3-tap form of a x2 transposed conv a zero (tap 2, phase 0) and (tap 0, phase 1) (four sub-steps per block on 256-column tiles; 128-column tiles stay as
they were).  A product left out is x * 0 and adding +-0 changes no finite sum, so the stored tensors are
EQUAL, not close.  The fused GroupNorm statistics are fp64 atomic adds of the same fp32 partial sums in a free order, so they agree to fp64 rounding: 1e-12
relative -- the sum of squares to itself, the sum to sqrt(count * sum of squares), which bounds it and is the scale of its addends (a sum that cancels to
near zero has no digits of its own to compare).  Each case is the smallest UNet1dConfig that holds the
layer at the smallest shape that reaches the kernel form (ADF_GEMM_RB=2: from 32 tiles on, but for the 128-row form); the switch is read once per process, so each side is a child
process (tests/diag/gpu_rb_zero_taps.py), one pair per configuration shared by the cases that read it."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from gpu_helpers import gemm_trace_lines

pytestmark = pytest.mark.gpu

BF16_CONV_TOL = 5e-4         # tests/test_gpu_parity.py: one stage behind the forced input
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case -> (multipliers, factors, B, input samples, tap, plan arguments (K, f, C, phase_c, n, B, rows), expected (tile rows, N halves, nb3, nb2, phase2))
CASES = {
    # <1,true,2> two-tap: 32 tiles of 256 x 128, four per sample -- first, interior and last tile of a sample
    "down_128_128_f2": ((2, 2), (2,), 8, 4096, "down0.conv", (5, 2, 128, 0, 128, 8, 1024), (256, 1, 2, 2, 0)),
    # <2,true,2> two-tap: 256 x 256 tiles
    "down_128_256_f2": ((2, 4), (2,), 8, 4096, "down0.conv", (5, 2, 128, 0, 256, 8, 1024), (256, 2, 2, 2, 0)),
    # <1,true,1> two-tap: 128-row tiles, 4 three-tap + 12 two-tap blocks.  The 128-row form takes B * rows in [16384, 32768) with the route's default switch only:
    # from 32 tiles on (ADF_GEMM_RB=2) it would need B * rows < 4096, and those rows go to the split-K kernel
    "down_256_256_f4": ((4, 4), (4,), 16, 8192, "down0.conv", (9, 4, 256, 0, 256, 16, 1024), (128, 1, 4, 12, 0)),
    # <2,true,2> phase form (with fused statistics over the phase-major columns: up0 is not the last up conv)
    "up_256_128_f2": ((2, 2, 4), (2, 2), 8, 8192, "up0.conv", (0, 2, 256, 128, 256, 8, 1024), (256, 2, 4, 0, 1)),
    "up_128_128_f2": ((2, 2, 2), (2, 2), 8, 8192, "up0.conv", (0, 2, 128, 128, 256, 8, 1024), (256, 2, 2, 0, 1)),
    # <1,true,2>, n = 128: the wave columns are the phases; skipping their zero tap's MFMAs measured no faster, the launch is left as it was
    "up_128_64_f2": ((1, 1, 2), (2, 2), 8, 8192, "up0.conv", (0, 2, 128, 64, 128, 8, 1024), (256, 1, 2, 0, 0)),
    # several tiles per workgroup: 320 tiles over 256 workgroups, uneven ranges
    "down_128_128_f2_tiles": ((2, 2), (2,), 5, 65536, "down0.conv", (5, 2, 128, 0, 128, 5, 16384), (256, 1, 2, 2, 0)),
    # left alone: one three-tap block would be left (an odd count): the table stays all three-tap
    "down_64_128_f2": ((1, 1, 2), (2, 2), 8, 8192, "down1.conv", (5, 2, 64, 0, 128, 8, 1024), (256, 1, 2, 0, 0)),
}
RB_SWITCH = {"down_256_256_f4": "1"}          # ADF_GEMM_RB of a case's runs (default 2)
MIN_TILES = {"1": 256, "2": 32}
# the taps one configuration's pair of runs stores
TAPS_OF_RUN = {}
for _m, _f, _b, _l, _tap, _p, _e in CASES.values():
    TAPS_OF_RUN.setdefault((_m, _f, _b, _l), []).append(_tap)


@functools.lru_cache(maxsize=None)
def run_pair(multipliers, factors, B, L, rb):
    """-> {"0" / "1": (stored tensors of the child, its [adf gemm] lines verbatim, parsed)}"""
    taps = sorted(set(TAPS_OF_RUN[(multipliers, factors, B, L)]))
    out = {}
    tmp = tempfile.TemporaryDirectory(prefix="rb_zero_taps_")
    for z in ("0", "1"):
        path = os.path.join(tmp.name, f"z{z}.pt")
        env = dict(os.environ, ADF_RB_ZSKIP=z, ADF_GEMM_RB=rb, ADF_GEMM_TRACE="1")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "diag", "gpu_rb_zero_taps.py"), path, ",".join(map(str, multipliers)),
                            ",".join(map(str, factors)), str(B), str(L), ",".join(taps)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out[z] = (torch.load(path), [l for l in r.stderr.splitlines() if l.startswith("[adf gemm]")], gemm_trace_lines(r.stderr))
    tmp.cleanup()
    return out


def block_plan(args, min_tiles, zskip):
    from audiodiffuser_amd import _lib
    lib = _lib.load_library()
    K, f, c, phase_c, n, B, rows = args
    v = [C.c_int() for _ in range(5)]
    assert lib.adf_debug_rb_block_plan(K, f, c, phase_c, n, B, rows, min_tiles, zskip, *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


@pytest.mark.parametrize("case", sorted(CASES))
def test_zero_taps_left_out_change_nothing(case):
    multipliers, factors, B, L, tap, plan_args, plan_want = CASES[case]
    # the launch takes the form the case is about (host arithmetic of launch_rb), and with the switch off every block is three-tap
    rb = RB_SWITCH.get(case, "2")
    assert block_plan(plan_args, MIN_TILES[rb], 1) == plan_want
    off = block_plan(plan_args, MIN_TILES[rb], 0)
    assert off[:2] == plan_want[:2] and off[2] == plan_want[2] + plan_want[3] and off[3:] == (0, 0)
    runs = run_pair(multipliers, factors, B, L, rb)
    (a, lines_a, parsed_a), (b, lines_b, _) = runs["1"], runs["0"]
    # the same launches on both sides, the layer's on the resblock conv kernel in its raw form
    assert lines_a == lines_b and lines_a
    K, f, c, phase_c, n, _, rows = plan_args
    mine = [l for l in parsed_a if l["taps"] == 3 and l["ab"] == 0 and l["c0"] == (c if phase_c else f * c) and l["c1"] == 0 and l["n"] == n
            and l["mrows"] == rows and l["B"] == B and l["nseg"] == 1]
    assert mine and all(l["route"] == "rb" for l in mine), mine
    ta, tb = a[tap], b[tap]
    print(f"{case}: {tap} {tuple(ta.shape)} differing elements {int((ta != tb).sum())}, oracle rel L2 {a[tap + '/oracle_rel_l2']:.3e} / {b[tap + '/oracle_rel_l2']:.3e}")
    assert a["out_finite"] and b["out_finite"]
    assert bool(torch.isfinite(ta).all()) and bool(torch.isfinite(tb).all())
    assert torch.equal(ta, tb)
    sa, sb = a[tap + "/stats"], b[tap + "/stats"]
    assert (sa is None) == (sb is None)
    if sa is not None:
        assert bool(torch.isfinite(sa).all())
        count = ta.shape[1] * ta.shape[2] // sa.shape[1]
        scale = torch.stack(((count * sb[..., 1]).sqrt(), sb[..., 1]), dim=-1)
        assert bool((sb[..., 0].abs() <= scale[..., 0] * (1 + 1e-6)).all())
        rel = float(((sa - sb).abs() / scale.clamp_min(1e-300)).max())
        print(f"{case}: statistics {tuple(sa.shape)} worst relative difference {rel:.3e}")
        assert rel <= 1e-12, rel
    assert a[tap + "/oracle_rel_l2"] < BF16_CONV_TOL, a[tap + "/oracle_rel_l2"]
