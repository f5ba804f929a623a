"""CPU: the float64 restatement tests/dac_ref.py against the reference modules' own results (tests/golden/dac_golden.npz, written by
tools/gen_golden_dac.py), the conditions its weight generator has to keep for the comparisons to mean something, and five mis-statements that each
move the output far beyond the device bar."""
import json
import os

import numpy as np
import pytest
import torch

import dac_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 5e-6                  # restatement vs reference (tools/gen_golden_dac.py)
DEVICE_BAR = 5e-5           # what the device is held to (tests/test_dac_gpu.py)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "dac_golden.npz"))


@pytest.fixture(scope="module")
def report():
    with open(os.path.join(ROOT, "tests", "golden", "dac_golden_report.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", DR.GOLDEN_CASES)
def test_restatement_reproduces_the_reference_fixture(gold, case):
    x = torch.from_numpy(gold[f"{case}_x"])
    assert torch.equal(x, DR.inputs(case))
    out, taps = DR.reference(case)
    worst = {"out": rel(out, torch.from_numpy(gold[f"{case}_out"]))}
    names = [k[len(case) + 1:] for k in gold.files if k.startswith(case + "_") and k not in (f"{case}_x", f"{case}_out")]
    assert names
    for n in names:
        assert tuple(taps[n].shape) == gold[f"{case}_{n}"].shape
        worst[n] = rel(taps[n], torch.from_numpy(gold[f"{case}_{n}"]))
    assert max(worst.values()) < BAR, worst          # (the fixture is the reference in fp32: its own rounding is ~1e-6)


def test_report_holds_the_recorded_distances_under_the_bar(report):
    assert report["bar"] == BAR and sorted(report["cases"]) == sorted(DR.GOLDEN_CASES)
    for case, r in report["cases"].items():
        assert max(r["dist"]["fp32"].values()) < BAR and max(r["dist"]["fp64"].values()) < BAR, case
        assert r["fp32_reference_vs_fp64_restatement"] < BAR


def test_fixture_is_small(gold):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "dac_golden.npz")) < 1 << 20


@pytest.mark.parametrize("case", list(DR.CASES))
def test_generator_keeps_the_activations_order_one(case):
    """Unit-normal weight_g saturates tanh (mean |out| 0.97) and every comparison would be vacuous: the generator's conditions on the real cases."""
    out, taps = DR.reference(case)
    for n, t in taps.items():
        assert 0.5 <= float(t.abs().max()) <= 10.0, (n, float(t.abs().max()))
    if DR.kind(case) == "dec":
        a = out.abs()
        assert float((a > 0.99).double().mean()) <= 0.01
        assert 0.1 <= float(a.mean()) <= 0.7, float(a.mean())
        assert out.shape[-1] == DR.output_length(case)


def test_output_lengths_of_the_cases():
    assert [DR.output_length(c) for c in ("odd", "r8", "w96", "long", "short")] == [518, 887, 140, 800, 38]
    assert [DR.up_length(13, 4), DR.up_length(52, 5), DR.up_length(37, 8), DR.up_length(296, 3)] == [52, 259, 296, 887]


def test_alpha_edge_case_holds_a_zero_and_a_tiny_alpha_in_every_snake():
    w = DR.weights("alpha0")
    alphas = [v for k, v in w.items() if k.endswith(".alpha")]
    assert alphas and all(float(a[0, 1, 0]) == 0.0 and float(a[0, 2, 0]) == pytest.approx(1e-4) for a in alphas)
    x = torch.linspace(-3, 3, 7, dtype=torch.float64).view(1, 1, 7).repeat(1, 3, 1)
    y = DR.snake(x, torch.tensor([1.0, 0.0, 1e-4], dtype=torch.float64).view(1, 3, 1))
    assert torch.equal(y[0, 1], x[0, 1]) and torch.isfinite(y).all()          # alpha = 0 returns x


def _cases_for(bug):
    return [c for c in DR.DECODER_CASES if bug != "floor_pad" or any(s % 2 for s in DR.config(c).rates)]


@pytest.mark.parametrize("bug", ["convT_axis", "no_dilation", "floor_pad", "no_residual", "scalar_alpha"])
def test_each_misstatement_moves_the_output_far_beyond_the_device_bar(bug):
    cases = _cases_for(bug)
    assert cases
    for case in cases:
        good, _ = DR.reference(case)
        with torch.no_grad():
            bad = DR.forward(case, bug=bug)
        if bad.shape != good.shape:                   # floor instead of ceil changes the length at an odd rate
            assert bug == "floor_pad"
            continue
        d = rel(bad, good)
        assert d > 100 * DEVICE_BAR, (bug, case, d)
