"""CPU: the split-bf16 (f32x3) mode of ``audiodiffuser_amd.DiT`` without a device -- the emulating restatement tests/dit_x3_ref.py against
tests/dit_ref.py in float64 (exact products: equal; split products: inside a quarter of the bar the device is held to; one dropped lo term per
site: outside the bar), and the constructor, config and build-list additions.

F32X3_TOL = 2e-4 is the project's split-bf16 bar (tests/test_gpu_parity.py).  The emulation's own distance from float64 over the eleven cases is
6.5e-6 .. 1.4e-5 of max |reference| per tap (worst: ``x3_deep`` blocks.4.attn 1.4e-5, ``lowvar`` blocks.0 1.2e-5), so the bar leaves 12x over the arithmetic.  The device itself measures 6.1e-6 .. 1.2e-5 on the same cases
(tests/golden/dit_x3_report.json).
"""
import functools
import os

import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib, build
import dit_ref as DR
import dit_x3_ref as X3

F32X3_TOL = 2e-4             # tests/test_gpu_parity.py
SMALL = dict(input_size=[16, 8], hidden_size=128, depth=1, num_heads=2)


@functools.lru_cache(maxsize=None)
def float64_taps(case):
    """(out, taps) of dit_ref.forward in float64, computed once per case and only read afterwards."""
    x, t, classes = X3.inputs(case)
    taps = {}
    with torch.no_grad():
        out = DR.forward(X3.weights(case), X3.config(case), x, t, classes, taps=taps)
    return out, taps


def emulated_worst(case, drop=None):
    """Worst distance of the emulated f32x3 forward from float64 over the output and every tap, per tensor."""
    x, t, classes = X3.inputs(case)
    ref, ref_taps = float64_taps(case)
    taps = {}
    with torch.no_grad():
        out = X3.forward(X3.weights(case), X3.config(case), x, t, classes, dtype=torch.float32, taps=taps, mm=X3.emulation(drop))
    worst = {"out": X3.rel(out, ref)}
    for n in X3.tap_names(X3.config(case).depth):
        worst[n] = X3.rel(taps[n], ref_taps[n])
    return worst


def test_the_cases_are_dit_refs_plus_four_and_reach_what_they_name():
    assert list(X3.CASES)[:len(DR.CASES)] == list(DR.CASES) and list(X3.CASES)[len(DR.CASES):] == ["x3_edge", "x3_long32", "x3_long64", "x3_deep"]
    e = X3.config("x3_edge")
    assert (e.tokens, e.tokens * X3.CASES["x3_edge"]["B"], e.hidden_size, e.mlp_hidden, e.hidden_size // e.num_heads) == (72, 144, 192, 480, 64)
    for case, hd in (("x3_long32", 32), ("x3_long64", 64)):
        c = X3.config(case)
        assert c.tokens == 1056 and c.hidden_size // c.num_heads == hd
    assert X3.config("x3_deep").depth == 8
    for case in X3.CASES:
        X3.config(case).validate_device()
    for case in DR.CASES:                       # the same weights and inputs as dit_ref's
        assert all(torch.equal(a, b) for a, b in zip(X3.weights(case).values(), DR.weights(case).values()))
        assert torch.equal(X3.inputs(case)[0], DR.inputs(case)[0]) and torch.equal(X3.inputs(case)[1], DR.inputs(case)[1])


@pytest.mark.parametrize("case", list(X3.CASES))
def test_exact_products_give_dit_ref_in_float64(case):
    x, t, classes = X3.inputs(case)
    ref, ref_taps = float64_taps(case)
    taps = {}
    with torch.no_grad():
        out = X3.forward(X3.weights(case), X3.config(case), x, t, classes, taps=taps)
    worst = {"out": X3.rel(out, ref), **{n: X3.rel(taps[n], ref_taps[n]) for n in X3.tap_names(X3.config(case).depth)}}
    assert sorted(taps) == sorted(ref_taps) and max(worst.values()) < 1e-14, worst


@pytest.mark.parametrize("case", list(X3.CASES))
def test_emulated_f32x3_is_inside_a_quarter_of_the_bar(case):
    worst = emulated_worst(case)
    print(case, max(worst, key=worst.get), max(worst.values()))
    assert max(worst.values()) < F32X3_TOL / 4, worst
    assert max(worst.values()) > 1e-7, "the emulation split nothing"


@pytest.mark.parametrize("drop", X3.DROPS)
def test_one_dropped_lo_term_moves_tiny_beyond_the_bar(drop):
    """Measured on ``tiny``: 3.3e-3, 2.9e-3, 1.1e-3, 1.2e-3, 1.0e-3, 1.5e-3 (the long cases are less sensitive at the P and V sites: 2.6e-4, 2.0e-4)."""
    worst = emulated_worst("tiny", drop)
    print(drop, max(worst, key=worst.get), max(worst.values()))
    assert max(worst.values()) > F32X3_TOL, (drop, worst)


def test_split_is_hi_plus_lo_to_two_to_the_minus_17():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4096, generator=g) * 3.0
    hi, lo = X3.split(x)
    assert torch.equal(hi, x.to(torch.bfloat16).float()) and float(((hi + lo) - x).abs().max() / x.abs().max()) < 2.0 ** -16


def test_f32x3_constructs_and_other_dtypes_are_refused_by_name():
    net = A.DiT(compute_dtype="f32x3", **SMALL)
    assert net.compute_dtype == "f32x3" and A.DiT(**SMALL).compute_dtype == "fp32"
    for bad in ("bf16", "bfloat16", "fp16", "f32x2"):
        with pytest.raises(ValueError, match="compute_dtype"):
            A.DiT(compute_dtype=bad, **SMALL)
    for kw in (dict(hidden_size=1152, num_heads=16), dict(hidden_size=96, num_heads=3), dict(mlp_ratio=4.1)):       # the width rules are the fp32 mode's
        with pytest.raises(ValueError):
            A.DiT(compute_dtype="f32x3", **{**SMALL, **kw})


def test_make_dit_config_carries_f32x3():
    assert _lib.DTYPE_F32X3 == 2 and _lib.make_dit_config(X3.config("x3_edge"), _lib.DTYPE_F32X3).dtype == 2
    from audiodiffuser_amd.net import _DTYPES
    assert _DTYPES["f32x3"] == _lib.DTYPE_F32X3


def test_new_sources_are_listed_and_the_abi_stays_7():
    assert "adf_dit_x3.hip" in build.SOURCES and "adf_dit.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "adf_dit_x3.hip"))
    assert _lib.load_library().adf_abi_version() == 7 and _lib.ABI_VERSION == 7
