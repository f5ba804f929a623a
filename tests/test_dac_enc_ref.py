"""CPU: the float64 restatement tests/dac_enc_ref.py against the reference modules' own results (tests/golden/dac_enc_golden.npz, written by
tools/gen_golden_dac_enc.py), the conditions its weight generator has to keep for the comparisons to mean something (the KL bar's among them), seven
mis-statements that each move an output far beyond the device bar, and the down conv's length formula against ``F.conv1d`` for every stride."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dac_enc_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 5e-6                  # restatement vs reference (tools/gen_golden_dac_enc.py); fp32 arithmetic vs float64 on the autoencoder cases
DEVICE_BAR = 5e-5           # what the device is held to (tests/test_dac_enc_gpu.py)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def relf(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "dac_enc_golden.npz"))


@pytest.fixture(scope="module")
def report():
    with open(os.path.join(ROOT, "tests", "golden", "dac_enc_golden_report.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", ER.GOLDEN_CASES)
def test_restatement_reproduces_the_reference_fixture(gold, case):
    x = torch.from_numpy(gold[f"{case}_x"])
    assert torch.equal(x, ER.inputs(case))
    out, taps = ER.reference(case)
    if ER.kind(case) == "ae":
        worst = {"mean": rel(out[0], torch.from_numpy(gold[f"{case}_out"])), "kl": relf(out[1], gold[f"{case}_kl"])}
    else:
        worst = {"out": rel(out, torch.from_numpy(gold[f"{case}_out"]))}
    names = ER.golden_taps(gold.files, case)
    assert names
    for n in names:
        assert tuple(taps[n].shape) == gold[f"{case}_{n}"].shape
        worst[n] = rel(taps[n], torch.from_numpy(gold[f"{case}_{n}"]))
    assert max(worst.values()) < BAR, worst          # (the fixture is the reference in fp32: its own rounding is ~1e-6)


def test_report_holds_the_recorded_distances_under_the_bar(report):
    assert report["bar"] == BAR and sorted(report["cases"]) == sorted(ER.GOLDEN_CASES)
    for case, r in report["cases"].items():
        assert max(r["dist"]["fp32"].values()) < BAR and max(r["dist"]["fp64"].values()) < BAR, case
        assert r["fp32_reference_vs_fp64_restatement"] < BAR
        if ER.kind(case) == "ae":
            assert r["kl_fp32_reference_vs_fp64_restatement"] < BAR
    assert "is_train" in report["signature"]["FineTuneAutoencoder.encode"] and "is_train" in report["signature"]["FineTuneAutoencoder.forward"]


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "dac_enc_golden.npz")) < 1 << 20


@pytest.mark.parametrize("case", list(ER.CASES))
def test_generator_keeps_every_tap_order_one(case):
    """No comparison is vacuous: every tap (and the result) reaches 0.25, and nothing blows up (the raw bottleneck of ae_clamp holds the +25 / -35 biases)."""
    out, taps = ER.reference(case)
    top = 40.0 if case == "ae_clamp" else 10.0
    for n, t in taps.items():
        assert 0.25 <= float(t.abs().max()) <= top, (n, float(t.abs().max()))
    main = out[0] if ER.kind(case) == "ae" else out
    assert float(main.abs().max()) >= 0.25
    if ER.kind(case) == "enc":
        assert out.shape[-1] == ER.output_length(case)


@pytest.mark.parametrize("case", ER.AE_CASES)
def test_fp32_reference_arithmetic_is_within_5e_6_of_float64_on_the_autoencoder_cases(case):
    """What the device's 5e-5 bar on the KL term rests on: the reference's own arithmetic in fp32 (mean, and the KL summed in fp32) is within 5e-6 of
    float64 -- ae_clamp included, whose sum is dominated by exp(20)."""
    (mean, kl), _ = ER.reference(case)
    with torch.no_grad():
        m32, k32 = ER.forward(case, dtype=torch.float32)
    assert m32.dtype == torch.float32 and k32.dtype == torch.float32
    assert rel(m32, mean) < BAR and relf(k32, kl) < BAR, (rel(m32, mean), relf(k32, kl))


def test_clamp_case_binds_both_clamps_and_tanh_case_bounds_the_mean():
    (_, _), taps = ER.reference("ae_clamp")
    logvar = taps["btnk_layer"][:, 8:]
    assert float(logvar[:, 2].min()) > 20.0 and float(logvar[:, 5].max()) < -30.0
    others = [c for c in range(8) if c not in (2, 5)]
    assert float(logvar[:, others].abs().max()) < 20.0
    (mean, _), taps = ER.reference("ae_tanh")
    assert float(mean.abs().max()) < 1.0 < float(taps["btnk_layer"][:, :32].abs().max())


def test_output_lengths_of_the_cases():
    for case in ER.ENCODER_CASES:
        cfg, L, got = ER.config(case), ER.CASES[case][3], []
        for s in cfg.rates:
            L = ER.down_length(L, s)
            got.append(L)
        assert got == ER.LENGTHS[case] and ER.output_length(case) == got[-1], case
    assert ER.down_min_length(2) == 2 and ER.LENGTHS["short"][-2] == 2          # `short` meets its last stage at the minimum


@pytest.mark.parametrize("s", range(2, 17))
def test_length_formula_is_conv1d_s_for_every_stride(s):
    """floor((L + 2 p - 2 s) / s) + 1 = L // s (even s) or (L + 1) // s (odd s), from the shortest valid length on; one below it F.conv1d refuses."""
    p, w = math.ceil(s / 2), torch.zeros(1, 1, 2 * s)
    lo = ER.down_min_length(s)
    assert lo == 2 * s - 2 * p == (s if s % 2 == 0 else s - 1)
    for L in list(range(lo, 60)) + [523, 805, 887]:
        want = F.conv1d(torch.zeros(1, 1, L), w, stride=s, padding=p).shape[-1]
        assert ER.down_length(L, s) == want == (L // s if s % 2 == 0 else (L + 1) // s), (s, L)
    with pytest.raises(RuntimeError):
        F.conv1d(torch.zeros(1, 1, lo - 1), w, stride=s, padding=p)


def test_alpha_edge_case_holds_a_zero_and_a_tiny_alpha_in_every_snake():
    w = ER.weights("alpha0")
    alphas = [v for k, v in w.items() if k.endswith(".alpha")]
    assert len(alphas) == 8 and all(float(a[0, 1, 0]) == 0.0 and float(a[0, 2, 0]) == pytest.approx(1e-4) for a in alphas)


ENC_BUGS = ["floor_pad", "no_dilation", "no_residual", "down_axis"]
AE_BUGS = ["swap_halves", "no_clamp", "kl_batch_sum"]


def _cases_for(bug):
    if bug == "floor_pad":
        return [c for c in ER.ENCODER_CASES if any(s % 2 for s in ER.config(c).rates)]
    if bug in ENC_BUGS:
        return list(ER.ENCODER_CASES)
    if bug == "no_clamp":
        return ["ae_clamp"]
    if bug == "kl_batch_sum":
        return [c for c in ER.AE_CASES if ER.CASES[c][2] > 1]
    return list(ER.AE_CASES)


@pytest.mark.parametrize("bug", ENC_BUGS + AE_BUGS)
def test_each_misstatement_moves_an_output_far_beyond_the_device_bar(bug):
    cases = _cases_for(bug)
    assert cases
    for case in cases:
        good, _ = ER.reference(case)
        with torch.no_grad():
            bad = ER.forward(case, bug=bug)
        if ER.kind(case) == "ae":
            d = max(rel(bad[0], good[0]), relf(bad[1], good[1]))
        elif bug == "floor_pad" and bad.shape != good.shape:      # floor instead of ceil changes the length where (L + 1) // s != (L - 1) // s:
            assert bad.shape[:2] == good.shape[:2] and bad.shape[-1] < good.shape[-1], (case, bad.shape, good.shape)      # that is the move
            continue
        else:
            d = rel(bad, good)
        assert d > 100 * DEVICE_BAR, (bug, case, d)
