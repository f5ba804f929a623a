"""CPU: the K-block table launch_rb builds for the raw launches of the resblock conv kernel (csrc/adf_gemm.hip ``rb_fill_args``, through
adf_debug_rb_block_plan; no device is touched).  The rule, restated here by enumeration: slot j of folded tap t' of a Conv1d(K, stride f) folded to stride 1
carries kernel tap t' f + j and is real iff that is < K; the 64-channel K blocks whose tap 2 is all zero become two-tap blocks when taps 0 and 1 are real
everywhere and an even number >= 2 of three-tap blocks stays ahead of them (the two-stage weight ring keeps its parity; a tile starts three-tap)."""
import ctypes as C

import pytest

from audiodiffuser_amd import _lib


def plan(K, f, c, phase_c, n, B, rows, min_tiles, zskip):
    lib = _lib.load_library()
    v = [C.c_int() for _ in range(5)]
    rc = lib.adf_debug_rb_block_plan(K, f, c, phase_c, n, B, rows, min_tiles, zskip, *[C.byref(x) for x in v])
    return None if rc else tuple(x.value for x in v)


# the seven raw launches of an evaluation of the benchmark (batch 64, from 256 tiles on): (K, f, C, phase_c, n, rows) -> (tile rows, N halves, nb3, nb2, phase2)
BENCH = [
    ((5, 2, 128, 0, 128, 2048), (256, 1, 2, 2, 0)),
    ((5, 2, 128, 0, 256, 1024), (256, 2, 2, 2, 0)),
    ((9, 4, 256, 0, 256, 256), (128, 1, 4, 12, 0)),
    ((0, 2, 256, 128, 256, 1024), (256, 2, 4, 0, 1)),
    ((0, 2, 128, 128, 256, 2048), (256, 2, 2, 0, 1)),
    ((0, 2, 128, 64, 128, 4096), (256, 1, 2, 0, 0)),         # 128 columns: the phases are the wave columns, every sub-step has work -- stays as it was
    ((5, 2, 64, 0, 128, 4096), (256, 1, 2, 0, 0)),           # one three-tap block would be left: stays as it was
]


@pytest.mark.parametrize("shape,want", BENCH)
def test_block_plan_of_the_benchmark_launches(shape, want):
    K, f, c, phase_c, n, rows = shape
    assert plan(K, f, c, phase_c, n, 64, rows, 256, 1) == want
    # switch off: the same tiles, every block three-tap
    assert plan(K, f, c, phase_c, n, 64, rows, 256, 0) == (want[0], want[1], want[2] + want[3], 0, 0)


def expected_blocks(K, f, c):
    """(nb3, nb2) by enumeration of the folded weights' structure"""
    nb = f * c // 64
    real = lambda t, ci: t * f + ci // c < K
    if not all(real(t, ci) for t in (0, 1) for ci in range(f * c)):
        return nb, 0
    zero_blocks = [all(not real(2, ci) for ci in range(64 * k, 64 * k + 64)) for k in range(nb)]
    # the zero blocks must be the table's tail, and whole blocks: no block may mix real and zero channels of tap 2 behind the first zero one
    first = zero_blocks.index(True) if True in zero_blocks else nb
    whole = all(real(2, ci) for ci in range(64 * first)) and all(zero_blocks[first:])
    if not whole or first < 2 or first % 2 or first == nb:
        return nb, 0
    return first, nb - first


def test_two_tap_blocks_follow_the_folded_structure():
    seen_two_tap = 0
    for f in (2, 4):
        for K in range(2 * f + 1, 3 * f + 1):            # three folded taps
            for c in (64, 128, 192, 256):
                for n in (128, 256):
                    for B, rows, min_tiles in ((8, 1024, 32), (64, 256, 256), (64, 2048, 256), (3, 512, 1)):
                        got = plan(K, f, c, 0, n, B, rows, min_tiles, 1)
                        nb = f * c // 64
                        if nb > 24 or nb % 2:
                            assert got is None, (K, f, c, n, B, rows)
                            continue
                        if got is None:                   # too few tiles for the route
                            assert B * (rows // 128) * (n // 128) < min_tiles, (K, f, c, n, B, rows)
                            continue
                        assert got[2:4] == expected_blocks(K, f, c) and got[4] == 0, (K, f, c, n, B, rows, got)
                        if got[3]:
                            seen_two_tap += 1
                            assert got[2] >= 2 and got[2] % 2 == 0
                        assert plan(K, f, c, 0, n, B, rows, min_tiles, 0)[2:] == (nb, 0, 0)
    assert seen_two_tap


def test_phase_form_needs_two_phases():
    # x2 on 256-column tiles: the N halves are the phases; four phases of 64 channels are not, nor are two on 128 columns or on two 128-column tiles
    assert plan(0, 2, 128, 128, 256, 8, 1024, 32, 1)[4] == 1
    assert plan(0, 2, 128, 64, 256, 8, 1024, 32, 1)[4] == 0
    assert plan(0, 2, 128, 64, 128, 8, 1024, 32, 1)[4] == 0
    assert plan(0, 2, 128, 128, 256, 8, 512, 32, 1)[1:] == (1, 2, 0, 0)
