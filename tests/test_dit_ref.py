"""CPU: the float64 restatement tests/dit_ref.py against the reference module's own tensors (tests/golden/dit_golden.npz, written by
tools/gen_golden_dit.py), and what the DiT cases can see.

Bar of the restatement: 5e-6 of max |reference| per tensor, the bar tests/test_oracle_unet2d.py holds its oracle to.  Measured (recorded in
tests/golden/dit_golden_report.json): 3.8e-7 .. 6.8e-7 in fp32 and in float64 -- the reference itself runs in fp32, so float64 does not come closer.

Sensitivity, measured here (max |wrong - right| / max |right| of the network output, float64):
                 tiny        lowvar
  erf-GELU       6.8e-5      1.2e-4
  eps = 1e-5     6.3e-6      2.3e-3     (tiny's rows enter norm1 with variance 1.2: eps is 1e-5 of it, invisible by construction; lowvar's 7.7e-4)
  gate per tile  1.4e-1      3.1e-1
  sin first      6.4e-1      1.0
Every one is asserted above FP32_TIGHT = 5e-5 on lowvar, and all but eps on tiny.
"""
import json
import os

import numpy as np
import pytest
import torch

import dit_ref as DR
from audiodiffuser_amd.dit import sincos_pos_embed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 5e-6
FP32_TIGHT = 5e-5


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "dit_golden.npz"))


@pytest.fixture(scope="module")
def report():
    with open(os.path.join(ROOT, "tests", "golden", "dit_golden_report.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", DR.GOLDEN_CASES)
def test_restatement_vs_every_golden_tensor(gold, case, dtype):
    cfg, w = DR.config(case), DR.weights(case)
    x, t, classes = DR.inputs(case)
    assert np.array_equal(gold[f"{case}_x"], x.numpy()) and np.array_equal(gold[f"{case}_t"], t.numpy()), "the fixture belongs to other inputs"
    taps = {}
    y = DR.forward(w, cfg, x, t, classes, dtype=dtype, taps=taps)
    names = ["x_embedder", "c", "final_layer"] + [f"blocks.{i}" for i in range(cfg.depth)]
    worst = {"out": rel(y, torch.from_numpy(gold[f"{case}_out"]))}
    for n in names:
        worst[n] = rel(taps[n], torch.from_numpy(gold[f"{case}_{n}"]))
    if classes is not None:
        assert np.array_equal(gold[f"{case}_classes"], classes.numpy())
        worst["null"] = rel(DR.forward(w, cfg, x, t, classes, cond_drop_prob=1.0, dtype=dtype), torch.from_numpy(gold[f"{case}_null"]))
    print(case, dtype, worst)
    assert max(worst.values()) < BAR, worst


@pytest.mark.parametrize("case", DR.GOLDEN_CASES)
def test_pos_embed_is_bit_equal_to_the_reference(gold, case):
    cfg = DR.config(case)
    mine = sincos_pos_embed(cfg.hidden_size, cfg.grid).unsqueeze(0)
    assert mine.dtype == torch.float32 and np.array_equal(mine.numpy(), gold[f"{case}_pos_embed"])


def test_report_records_the_measured_distances(report):
    for case in DR.GOLDEN_CASES:
        for dt in ("fp32", "fp64"):
            d = report["variants"][case]["dist"][dt]
            assert "out" in d and max(d.values()) < BAR
    assert report["variants"]["lowvar"]["norm1_row_variance"] < 2e-3 < 0.5 < report["variants"]["tiny"]["norm1_row_variance"]


MISSTATEMENTS = {"erf": dict(gelu="erf"), "eps": dict(eps=1e-5), "gate_tile": dict(gate_tile=128), "sin_first": dict(sin_first=True)}


@pytest.mark.parametrize("case,what", [("lowvar", k) for k in MISSTATEMENTS] + [("tiny", k) for k in MISSTATEMENTS if k != "eps"])
def test_the_cases_see_each_misstatement(case, what):
    cfg, w = DR.config(case), DR.weights(case)
    x, t, classes = DR.inputs(case)
    right = DR.forward(w, cfg, x, t, classes)
    wrong = DR.forward(w, cfg, x, t, classes, **MISSTATEMENTS[what])
    d = rel(wrong, right)
    print(case, what, d)
    assert d > FP32_TIGHT, (case, what, d)


def test_three_dim_input_is_the_h1_call():
    cfg, w = DR.config("row"), DR.weights("row")
    x, t, _ = DR.inputs("row")
    assert x.ndim == 3
    assert torch.equal(DR.forward(w, cfg, x, t), DR.forward(w, cfg, x.unsqueeze(2), t).squeeze(2))
