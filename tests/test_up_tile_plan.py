"""CPU: the tile height launch_up takes for the transposed-conv kernel (csrc/adf_gemm_up.h ``up_tile_plan``, through adf_debug_up_tile_plan; no device
is touched).  The rule, restated here by enumeration: tiles of 32 mt wrows output blocks (mt = 1, 2, 4), one work item per (sample, tile, column
pass) on 256 persistent workgroups; fewest rounds of 256 workgroups, then fewest rows of a sample's last tile past L, then the taller tile."""
import ctypes as C

import pytest

from audiodiffuser_amd import _lib

# (cin, cout, f) -> (rows of a wave-row 32 mt tile stack = 32 * wrows, column passes): N = f cout columns in passes of 256 (128 -> 64 x2: one pass of 128 columns
# on four wave columns, two wave rows)
SHAPES = {(256, 256, 4): (32, 4), (256, 128, 2): (32, 1), (128, 128, 2): (32, 1), (128, 64, 2): (64, 1)}
LENGTHS = [4, 16, 20, 64, 80, 256, 320, 1024]
BATCHES = [3, 5, 64]


def plan(shape, B, L):
    lib = _lib.load_library()
    tr, it, ro, de = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.adf_debug_up_tile_plan(*shape, B, L, C.byref(tr), C.byref(it), C.byref(ro), C.byref(de)) == 0
    return tr.value, it.value, ro.value, de.value


def candidates(shape, B, L):
    base, npass = SHAPES[shape]
    out = []
    for mt in (1, 2, 4):
        tm = base * mt
        tiles = -(-L // tm)
        items = B * tiles * npass
        out.append((tm, items, -(-items // 256), tiles * tm - L))
    return out


@pytest.mark.parametrize("shape", sorted(SHAPES), ids=lambda s: "%dto%dx%d" % s)
@pytest.mark.parametrize("B", BATCHES)
def test_fewest_rounds_then_fewest_dead_rows_then_the_taller_tile(shape, B):
    for L in LENGTHS:
        tm, items, rounds, dead = plan(shape, B, L)
        cand = candidates(shape, B, L)
        assert (tm, items, rounds, dead) in cand, (L, (tm, items, rounds, dead), cand)
        for ctm, _, crounds, cdead in cand:
            assert (rounds, dead, -tm) <= (crounds, cdead, -ctm), (L, (tm, rounds, dead), (ctm, crounds, cdead))
        # what the numbers mean: the tiles cover every row of every sample exactly once, and no tile is all dead
        assert items % (B * SHAPES[shape][1]) == 0 and 0 <= dead < tm and (items // (B * SHAPES[shape][1])) * tm == L + dead


def test_the_flagship_launches_at_batch_64():
    """256 -> 256 x4 at L = 16 / 64 / 256: 32, 64 and 128 rows; the L = 256 launch is 512 items = two rounds (three 128-row tiles of m = 0 .. 256 were 768)."""
    s = (256, 256, 4)
    assert plan(s, 64, 16) == (32, 256, 1, 16)
    assert plan(s, 64, 64) == (64, 256, 1, 0)
    assert plan(s, 64, 256) == (128, 512, 2, 0)
    assert plan(s, 64, 1024) == (128, 2048, 8, 0)
    # a tile with more dead than live rows only where the shortest tile has them
    assert plan(s, 3, 4) == (32, 12, 1, 28)
    # a partial last 128-row tile needs a batch at which the shorter tiles cost a round more
    assert plan(s, 33, 320) == (128, 396, 2, 64) and plan(s, 22, 320) == (64, 440, 2, 0)
    assert plan(s, 3, 20) == (32, 12, 1, 12) and plan(s, 3, 80) == (32, 36, 1, 16) and plan(s, 3, 320) == (64, 60, 1, 0)


def test_other_shapes_and_bad_arguments_are_refused():
    lib = _lib.load_library()
    z = C.c_int()
    for args in ((256, 256, 2, 3, 16), (64, 64, 4, 3, 16), (256, 256, 4, 0, 16), (256, 256, 4, 3, 0)):
        assert lib.adf_debug_up_tile_plan(*args, C.byref(z), C.byref(z), C.byref(z), C.byref(z)) != 0, args
