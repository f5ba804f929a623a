"""CPU: the rectified-flow plugin classes (ReFlow, RFEDMSchedule, ReflowEulerSampler) and the restatement tests/rf_ref.py against the reference's
own values (tests/golden/rf_golden.npz, written by tools/gen_golden_rf.py from the reference's classes); the host step logic of the new sampler kind
through adf_sampler_nfe; what the constructor and the ABI promise.

adf_set_preconditioning needs a handle and a handle needs a device, so that the library takes kinds 4 and 5 and refuses 6 is asserted on the device
(tests/test_rf_gpu.py); here the constants are held to the header."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
from oracle import unet2d as U
import rf_cases as RC
import rf_ref as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
ORACLE_PIN = 2.1e-6          # one call: the bar at which oracle/unet2d.py is pinned to the reference's UNet2dBase (tests/test_oracle_unet2d.py)
RUN_PIN = 2e-5               # a 6-step run around the two nets (tools/gen_golden_rf.py; measured 3e-7 .. 9e-7)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "rf_golden.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(ROOT, "tests", "golden", "rf_golden.json")) as f:
        return json.load(f)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_schedules_equal_the_reference_exactly(gold):
    for n in (7, 8, 9, 31, 51):
        assert np.array_equal(A.LinearSchedule(1.0, 0.0, n)().numpy(), gold[f"sched_linear_{n}"])
        assert np.array_equal(RF.linear_schedule(1.0, 0.0, n).numpy(), gold[f"sched_linear_{n}"])
    for n in (8, 30):
        sig = A.RFEDMSchedule(start=0.98, end=0.02, num_steps=n)()
        assert sig.dtype == torch.float32 and sig.shape == (n,)
        assert np.array_equal(sig.numpy(), gold[f"sched_rfedm_{n}"])
        assert np.array_equal(RF.rfedm_schedule(0.98, 0.02, n).numpy(), gold[f"sched_rfedm_{n}"])
    dflt = A.RFEDMSchedule()()                                  # the reference's own arithmetic at its defaults: inf first, 0 last
    assert torch.isinf(dflt[0]) and float(dflt[-1]) == 0.0
    for bad in (dict(start=1.5), dict(end=-0.1)):
        with pytest.raises(AssertionError):
            A.RFEDMSchedule(**bad)


def test_constructor_signatures_equal_the_reference(meta):
    want = dict(meta["signatures"])
    assert set(want) == {"ReFlow", "RFEDMSchedule", "LinearSchedule", "ReflowEulerSampler"}
    want["ReflowEulerSampler"] = want["ReflowEulerSampler"] + [["use_graph", True]]         # this package's one extra keyword, as on every sampler
    for name, sig in want.items():
        got = [[k, None if p.default is inspect.Parameter.empty else p.default]
               for k, p in inspect.signature(getattr(A, name).__init__).parameters.items() if k != "self"]
        assert got == sig, (name, got, sig)


def test_rows_of_the_restatement_equal_the_reference_exactly(gold):
    sig = T(gold["sched_rfedm_30"])
    assert np.array_equal(RF.rows(True, sig).numpy(), gold["rows_rfedm"])
    assert np.array_equal(RF.rows(True, sig, torch.float64).numpy(), gold["rows64_rfedm"])
    assert np.array_equal(RF.rows(False, T(gold["sched_linear_31"])[:30]).numpy(), gold["rows_rf"])
    bar, r64 = gold["bar_rfedm"], gold["rows64_rfedm"]
    assert np.all(bar >= 1e-6) and np.all(np.abs(gold["rows_rfedm"].astype(np.float64) - r64) <= 0.25 * bar * np.abs(r64) * (1 + 1e-9) + 1e-300)
    t = A.ReFlow(for_edm=True).sigma_to_t(sig)                 # the plugin's own map is the reference's
    assert np.array_equal(t.numpy(), gold["rows_rfedm"][:, 1]) and np.array_equal((1 - t).numpy(), gold["rows_rfedm"][:, 0])


@pytest.mark.parametrize("mode", ["raw", "edm"])
def test_denoise_fn_restatement_and_compatibility_branch_vs_reference(gold, mode):
    """One inference call per mode (scalar sigma and [B] sigmas) of tests/rf_ref.py and of the plugin's tensor-op branch around oracle/unet2d.py,
    against what the reference's ReFlow returned around the reference's UNet2dBase with the same weights (for_edm: sample by sample)."""
    cfg, _ = U.fixture_variants()["small"]
    w = U.generate_weights(cfg, seed=5)
    classes = T(gold["den_classes"])
    net = lambda xi, ti, cond_drop_prob=0.0, classes=None: U.unet2d_forward(w, cfg, xi, ti, classes=classes, cond_drop_prob=cond_drop_prob)
    net_o = lambda xi, ti, cond_drop_prob=0.0: net(xi, ti, cond_drop_prob, classes)
    d = A.ReFlow(for_edm=mode == "edm")
    x, s0, sb = T(gold[f"den_{mode}_x"]), float(gold[f"den_{mode}_sigma"]), T(gold[f"den_{mode}_sigmas"])
    ws, wb = T(gold[f"den_{mode}_y_scalar"]), T(gold[f"den_{mode}_y_batch"])
    with torch.no_grad():
        got = {"plugin scalar": (d.denoise_fn(x, net=net, inference=True, sigma=s0, classes=classes), ws),
               "plugin batch": (d.denoise_fn(x, net=net, inference=True, sigmas=sb, classes=classes), wb),
               "rf_ref scalar": (RF.denoise(mode == "edm", net_o, x, sigma=s0), ws), "rf_ref batch": (RF.denoise(mode == "edm", net_o, x, sigmas=sb), wb)}
        y64 = RF.denoise(mode == "edm", lambda xi, ti, cond_drop_prob=0.0: U.unet2d_forward({k: v.double() for k, v in w.items()}, cfg, xi, ti,
                                                                                         classes=classes, cond_drop_prob=cond_drop_prob), x.double(), sigmas=sb)
    for name, (y, want) in got.items():
        print(mode, name, rel(y, want))
        assert y.dtype == torch.float32 and rel(y, want) <= ORACLE_PIN, (mode, name, rel(y, want))
    assert y64.dtype == torch.float64 and rel(y64, wb) <= 2 * ORACLE_PIN
    assert float(ws.abs().max()) > 1.0 and float(got["plugin scalar"][0].abs().max()) > 1.0        # ReFlow does not clip in either mode


def test_reflow_never_clips_and_guides_and_trains():
    net = lambda xi, ti, cond_drop_prob=0.0: 3.0 * xi + ti.view(-1, 1, 1) + cond_drop_prob
    x = torch.randn(2, 1, 8, generator=torch.Generator().manual_seed(0))
    tb = torch.tensor([0.3, 0.9])
    raw = A.ReFlow().denoise_fn(x, net=net, inference=True, sigmas=tb)
    assert torch.equal(raw, 3.0 * x + tb.view(2, 1, 1)) and float(raw.abs().max()) > 1.0
    guided = A.ReFlow().denoise_fn(x, net=net, inference=True, cond_scale=2.0, sigmas=tb)         # null + (cond - null) * 2 = cond - 1 with this net
    assert torch.allclose(guided, raw - 1.0, atol=1e-6)
    t = tb / (tb + 1)
    xin = x * (1 - t).view(2, 1, 1)
    assert torch.allclose(A.ReFlow(for_edm=True).denoise_fn(x, net=net, inference=True, sigmas=tb), xin - (3.0 * xin + t.view(2, 1, 1)) * t.view(2, 1, 1), atol=1e-6)
    assert A.ReFlow()._clips is False and A.ReFlow().dynamic_threshold == 0.0
    assert A.ReFlow()._precond()[0] == _lib.PRECOND_RF == 4 and A.ReFlow(for_edm=True)._precond()[0] == _lib.PRECOND_RF_EDM == 5
    # the training loss (:420-442): with a net that returns z1 - x exactly the loss is 0; here only shape, finiteness and the draw order are held
    torch.manual_seed(3)
    loss = A.ReFlow()(x, lambda xi, ti: torch.zeros_like(xi), tb)
    torch.manual_seed(3)
    z1 = torch.randn_like(x)
    assert loss.shape == (2,) and torch.allclose(loss, ((z1 - x) ** 2).mean(dim=[1, 2]))


@pytest.mark.parametrize("tag,heun,cs", [("euler", False, 1.0), ("heun", True, 1.0), ("heun_cfg", True, 2.0)])
def test_sampler_restatement_and_compatibility_branch_vs_reference_runs(gold, meta, tag, heun, cs):
    """6 steps of the reference's ReflowEulerSampler over ReFlow() around its UNet2dBase (fixture) against tests/rf_ref.py and the plugin's
    tensor-op branch, both around oracle/unet2d.py."""
    cfg, w = RC.weights("u2d", meta["reference_runs"]["final_conv_scale"])
    cl = T(gold["run_classes"])
    net = lambda xi, ti, cond_drop_prob=0.0, classes=None: U.unet2d_forward(w, cfg, xi, ti, classes=classes, cond_drop_prob=cond_drop_prob)
    noise, sig, want = T(gold["run_noise"]), T(gold["sched_linear_7"]), T(gold[f"run_{tag}_final"])
    with torch.no_grad():
        mine = RF.euler_sampler(noise, RF.make_fn(False, lambda xi, ti, cond_drop_prob=0.0: net(xi, ti, cond_drop_prob, cl), cs), sig, 6, use_heun=heun)
        plug = A.ReflowEulerSampler(num_steps=6, cond_scale=cs, use_heun=heun)(noise, fn=A.ReFlow().denoise_fn, net=net, sigmas=sig, classes=cl)
    print(tag, rel(mine, want), rel(plug, want))
    assert rel(mine, want) <= RUN_PIN and rel(plug, want) <= RUN_PIN
    assert float(want.abs().max()) > 0.05 and float((want.abs() >= 1).float().mean()) <= 0.01
    assert float(plug.abs().max()) <= 1.0


def test_index_error_on_a_schedule_of_num_steps_entries(meta):
    """The reference indexes sigmas[i + 1] for i < num_steps (recorded in the fixture): this class raises the same way, on both branches, before
    anything runs -- the net is never called."""
    assert meta["reference_raises_index_error_on_num_steps_sigmas"] is True
    calls = []
    fn = lambda x, **kw: calls.append(1) or x
    noise = torch.zeros(1, 1, 64)
    with pytest.raises(IndexError):
        A.ReflowEulerSampler(num_steps=6)(noise, fn=fn, net=None, sigmas=torch.linspace(1, 0, 6))
    net = A.UNet1dBase.from_config(A.config_tiny())
    with pytest.raises(IndexError):                                       # the package's own (fn, net) pair: refused before the device is looked for
        A.ReflowEulerSampler(num_steps=6)(noise, fn=A.ReFlow().denoise_fn, net=net, sigmas=torch.linspace(1, 0, 6))
    assert calls == []
    with pytest.raises(IndexError):
        RF.euler_sampler(noise, fn, torch.linspace(1, 0, 6), 6, use_heun=False)
    assert calls == [1] * 5                                               # (the restatement, like the reference, fails on its last step)
    A.ReflowEulerSampler(num_steps=6)(noise, fn=fn, net=None, sigmas=torch.linspace(1, 0, 7))
    assert len(calls) == 5 + 11                                           # 6 Euler evaluations + 5 Heun corrections (none into sigma_next = 0)


def test_sampler_nfe_of_the_new_kind_via_abi():
    lib = _lib.load_library()

    def nfe(smp, sg):
        arr = (C.c_float * len(sg))(*sg.tolist())
        return lib.adf_sampler_nfe(C.byref(smp._desc(1.0)), arr, len(sg))
    for n in (1, 6, 50):
        to0, above = torch.linspace(1.0, 0.0, n + 1), torch.linspace(1.0, 0.02, n + 1)
        assert nfe(A.ReflowEulerSampler(num_steps=n, use_heun=False), to0) == n
        assert nfe(A.ReflowEulerSampler(num_steps=n, use_heun=False), above) == n
        assert nfe(A.ReflowEulerSampler(num_steps=n), to0) == 2 * n - 1          # no Heun correction into sigma_next = 0
        assert nfe(A.ReflowEulerSampler(num_steps=n), above) == 2 * n
        assert nfe(A.ReflowEulerSampler(num_steps=n), to0[:n]) == -1             # num_steps sigmas: rejected
        assert nfe(A.ReflowEulerSampler(num_steps=n), torch.cat([to0, to0[-1:]])) == 2 * n - 1      # a longer schedule: only num_steps + 1 entries are read
    assert nfe(A.ReflowEulerSampler(num_steps=0), torch.linspace(1.0, 0.0, 3)) == -1
    d = A.ReflowEulerSampler(num_steps=6)._desc(1.0)
    d.kind = 11
    assert lib.adf_sampler_nfe(C.byref(d), (C.c_float * 7)(*torch.linspace(1, 0, 7).tolist()), 7) == -1


def test_native_pair_accepts_reflow_in_both_modes():
    import audiodiffuser_amd.samplers as SM
    net = A.UNet1dBase.from_config(A.config_tiny())
    for d in (A.ReFlow(), A.ReFlow(for_edm=True)):
        assert getattr(d.denoise_fn, "__func__") is A.diffusion.Diffusion.denoise_fn          # not overridden: what _native_pair recognises
        assert SM._native_pair(d.denoise_fn, net, 1.0, {}) is d
    cc = A.UNet1dBase.from_config(A.config_tiny_cc())
    assert SM._native_pair(A.ReFlow().denoise_fn, cc, 2.0, {"classes": torch.tensor([1])}) is not None


def test_constants_descriptor_and_header_agree():
    hdr = open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")).read()
    kinds = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ADF_PRECOND_([A-Z_]+) (\d+)\b", hdr)}
    assert kinds == {"EDM": 0, "VE": 1, "VP": 2, "V_EDM": 3, "RF": 4, "RF_EDM": 5}              # 6 is no kind: the library refuses it (tests/test_rf_gpu.py)
    assert all(getattr(_lib, f"PRECOND_{k}") == v for k, v in kinds.items())
    assert _lib.SAMPLER_RF_EULER == int(re.search(r"#define ADF_SAMPLER_RF_EULER (\d+)", hdr).group(1)) == 10
    assert C.sizeof(_lib.AdfSamplerDesc) == 64                                                # the new kind reads existing fields only
    d = A.ReflowEulerSampler(num_steps=9, use_heun=False, use_graph=False)._desc(1.0)
    assert (d.kind, d.num_steps, d.use_heun, d.use_graph, d.reflow, d.order) == (10, 9, 0, 0, 0, 0)
    assert _lib.load_library().adf_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define ADF_ABI_VERSION (\d+)", hdr).group(1))
