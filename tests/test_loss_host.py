"""CPU: the validation loss off the device -- the ``model.noise_distribution`` plugins and the loss classes against the reference's recorded
results (tests/golden/loss_golden.npz, written by tools/gen_golden_loss.py), the C ABI of ``adf_diffusion_loss``, the routing predicate of
``Diffusion.forward``, and the derivation of the 1e-6 bar tests/test_loss_gpu.py holds the device's loss kernels to.

The bar.  The device forms d = fl(pred - x) and fl(d d) in fp32 and sums in double.  d carries one rounding (2^-24 relative) and d^2 three (two
through d, one of the product): Sum fl(d^2) is within 3 * 2^-24 = 1.8e-7 of Sum d^2, relative, and the double sum and the one final rounding add
2^-24 = 6e-8 more: 2.4e-7 for the x0 kinds.  For the velocity loss d = fl(fl(noise - x) - pred), and the rounded noise - x adds an ABSOLUTE error of
2^-24 |noise - x| to d, so d^2 moves by 2 |d| 2^-24 |noise - x| and the sum, by Cauchy-Schwarz, by at most 2^-23 sqrt(Sum d^2 Sum (noise - x)^2); with
Sum d^2 >= 0.1 Sum (noise - x)^2 that is 2^-23 / sqrt(0.1) = 3.8e-7 relative, in all 1.8e-7 + 3.8e-7 = 5.6e-7 <= 1e-6.  The 0.1 condition is asserted
on the inputs below (the losses of an untrained net are of the order of the target's energy); the NumPy emulation of that arithmetic stays at or
below half the bar."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
from audiodiffuser_amd.diffusion import loss_route_refusal
import loss_ref as LR
import precond_ref as P
import rf_cases as RC
import rf_ref as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
PIN = 1e-6                   # the package's classes and tests/loss_ref.py against the reference's recorded losses, per sample, relative
LOSS_BAR = 1e-6              # the bar of tests/test_loss_gpu.py for the device's loss of its own prediction (derivation above)


def rel_b(a, b):
    return float(((a.double() - b.double()).abs() / b.double().abs()).max())


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "loss_golden.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(ROOT, "tests", "golden", "loss_golden.json")) as f:
        return json.load(f)


# ---- the reference's recorded results ------------------------------------------------------------------------------------------------------
def test_distributions_reproduce_the_reference_draws_bit_for_bit(gold, meta):
    assert len(meta["distributions"]) >= 9
    classes = set()
    for name, rec in meta["distributions"].items():
        torch.manual_seed(rec["seed"])
        got = getattr(A, rec["class"])(**rec["kwargs"])(num_samples=meta["n_draws"], device=torch.device("cpu"))
        assert got.dtype == torch.float32 and got.shape == (meta["n_draws"],)
        assert np.array_equal(got.numpy(), gold[f"dist_{name}"]), name
        classes.add(rec["class"])
    assert classes == {"LogNormalDistribution", "UniformDistribution", "LogUniformDistribution", "LogitDistribution"}
    kws = [rec["kwargs"] for rec in meta["distributions"].values()]
    assert any(k.get("ln_scale") and k.get("stratified") for k in kws) and any(k.get("ln_scale") and not k.get("stratified") for k in kws)


def test_distributions_are_exported_and_documented_as_noise_distribution():
    from audiodiffuser_amd import distribution as D
    for name in ("LogNormalDistribution", "UniformDistribution", "LogUniformDistribution", "LogitDistribution"):
        assert getattr(A, name) is getattr(D, name) and name in A.__doc__
    assert "model.noise_distribution" in A.__doc__


def test_loss_classes_and_restatement_reproduce_the_reference_losses(gold, meta):
    x, noise = T(gold["loss_x"]), T(gold["loss_noise"])
    assert len(meta["losses"]) >= 5
    for case, rec in meta["losses"].items():
        kind, coef, want = rec["kind"], T(gold[f"coef_{rec['kind']}"]), T(gold[f"loss_{case}"])
        diff = getattr(A, rec["class"])(**rec["kwargs"])
        with torch.no_grad():
            torch.manual_seed(meta["loss_seed"])
            got = diff(x, LR.toy_net, sigmas=coef, **rec["forward_kwargs"])
            after = torch.rand(1)
            torch.manual_seed(meta["loss_seed"])
            assert torch.equal(torch.randn_like(x), noise)            # the one draw of forward is randn_like(x), first
            assert torch.equal(torch.rand(1), after)                  # ... and the only one
            rkw = {"dynamic_threshold": rec["kwargs"]["dynamic_threshold"]} if "dynamic_threshold" in rec["kwargs"] else {}
            r32 = LR.forward(kind, LR.toy_net, x, noise, coef, **rkw)
            r64 = LR.forward(kind, LR.toy_net, x.double(), noise, coef, **rkw)
        assert got.shape == want.shape == (x.shape[0],) and got.dtype == torch.float32
        assert rel_b(got, want) <= PIN and rel_b(r32, want) <= PIN and rel_b(r64, want) <= PIN, (case, rel_b(got, want), rel_b(r32, want), rel_b(r64, want))
        assert diff._loss_kind() == LR.LOSS_KIND[kind]


def test_forward_of_a_foreign_net_is_the_tensor_route(gold):
    """Every class: ``forward`` around a plain callable equals ``_tensor_loss`` with the same seed (VPDiffusion's takes the mapped sigmas)."""
    x = T(gold["loss_x"])
    t = torch.tensor(LR.TIMES)
    for diff in (A.EluDiffusion(0.2), A.VEDiffusion(), A.VPDiffusion(0.1, 19.9, 1000), A.VDiffusion(), A.VDiffusion(for_edm=True), A.ReFlow(), A.ReFlow(True)):
        torch.manual_seed(3)
        a = diff(x, LR.toy_net, t)
        torch.manual_seed(3)
        b = diff._tensor_loss(x, LR.toy_net, diff.t_to_sigma(t) if isinstance(diff, A.VPDiffusion) else t)
        assert a.shape == (x.shape[0],) and torch.allclose(a, b, rtol=0.0, atol=0.0, equal_nan=True), type(diff).__name__


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_constants_and_version():
    hdr = open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")).read()
    lib = _lib.load_library()
    for sym in ("adf_diffusion_loss", "adf_loss_calls"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTS
        assert re.search(rf"\b{sym}\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for macro, val in (("ADF_LOSS_X0_EDM", _lib.LOSS_X0_EDM), ("ADF_LOSS_X0_INV_SIGMA2", _lib.LOSS_X0_INV_SIGMA2), ("ADF_LOSS_RF", _lib.LOSS_RF)):
        assert int(re.search(rf"#define {macro}\s+(\d+)", hdr).group(1)) == val
    assert (_lib.LOSS_X0_EDM, _lib.LOSS_X0_INV_SIGMA2, _lib.LOSS_RF) == (0, 1, 2)
    assert _lib.ABI_VERSION == 7 and lib.adf_abi_version() == 7 and "#define ADF_ABI_VERSION 7" in hdr
    assert "adf_diffusion_loss" in re.search(r"^ \* 7: .*?\*/", hdr, flags=re.S | re.M).group(0)          # the changelog entry under 7
    assert set(re.findall(r"#define (ADF_PRECOND_\w+)", hdr)) == {"ADF_PRECOND_EDM", "ADF_PRECOND_VE", "ADF_PRECOND_VP", "ADF_PRECOND_V_EDM", "ADF_PRECOND_RF",
                                                                 "ADF_PRECOND_RF_EDM"}
    assert C.sizeof(_lib.AdfRunCounters) == 6 * 8 and C.sizeof(_lib.AdfSamplerDesc) == 64
    # the chunk length the tests build their row sweep around is the kernels'
    src = open(os.path.join(ROOT, "audiodiffuser_amd", "csrc", "adf_loss.h")).read()
    assert int(re.search(r"constexpr int kLossChunk = (\d+);", src).group(1)) == _lib.LOSS_CHUNK


def test_null_handle_is_refused_without_a_device():
    lib = _lib.load_library()
    z = C.c_void_p(0)
    assert lib.adf_diffusion_loss(z, 0, z, z, z, 0.2, z, z, z, 1, 256, z) != 0
    assert lib.adf_loss_calls(z) == 0


def test_sources_are_in_the_build_lists():
    from audiodiffuser_amd import build
    assert "adf_loss.hip" in build.SOURCES and "adf_loss.h" in build.HEADERS


# ---- routing predicate ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nets():
    plain = A.UNet1dBase.from_config(A.config_tiny())
    cc = A.UNet1dBase.from_config(A.config_tiny_cc())
    return plain, cc


def test_loss_kind_table():
    assert A.EluDiffusion(0.2)._loss_kind() == _lib.LOSS_X0_EDM
    assert A.VEDiffusion()._loss_kind() == A.VPDiffusion(0.1, 19.9, 1000)._loss_kind() == _lib.LOSS_X0_INV_SIGMA2
    assert A.ReFlow()._loss_kind() == _lib.LOSS_RF
    assert A.VDiffusion()._loss_kind() is None and A.VDiffusion(for_edm=True)._loss_kind() is None and A.ReFlow(for_edm=True)._loss_kind() is None
    assert A.VDiffusion()._precond() is None


def test_routing_accepts_exactly_the_listed_calls():
    plain, cc = _nets()
    cl = torch.tensor([1, 2, 3])
    ok = lambda *a: loss_route_refusal(*a) is None
    for diff in (A.EluDiffusion(0.2), A.EluDiffusion(0.2, dynamic_threshold=0.9), A.EluDiffusion(0.2, dynamic_threshold=1.0), A.VEDiffusion(),
                 A.VPDiffusion(0.1, 19.9, 1000), A.ReFlow()):
        # unconditional net, either mode; cond_scale is ignored when not inferring, as in the reference
        assert ok(diff, plain, True, False, 1.0, {})
        assert ok(diff, plain, True, True, 1.0, {})
        assert ok(diff, plain, True, False, 2.0, {})
        assert ok(diff, plain, True, False, 1.0, {"classes": None})
        # class-conditional: guidance in two passes when inferring, the net's own cond_drop_prob (0 or 1) otherwise
        assert ok(diff, cc, True, True, 1.0, {"classes": cl})
        assert ok(diff, cc, True, True, 2.0, {"classes": cl})
        for cdp in (0, 0.0, 1, 1.0):
            cc.cond_drop_prob = cdp
            assert ok(diff, cc, True, False, 1.0, {"classes": cl})
            assert ok(diff, cc, True, False, 3.0, {"classes": cl})
        cc.cond_drop_prob = 0.0


def test_routing_refuses_with_a_reason():
    plain, cc = _nets()
    cl = torch.tensor([1, 2, 3])
    edm = A.EluDiffusion(0.2)
    why = lambda *a: loss_route_refusal(*a) or ""
    # classes without a device form of the loss
    for diff in (A.VDiffusion(), A.VDiffusion(for_edm=True), A.ReFlow(for_edm=True)):
        assert "no device form" in why(diff, plain, True, False, 1.0, {})
    # foreign net, host tensor, threshold outside [0, 1], x_mask
    assert "HIP nets" in why(edm, LR.toy_net, True, False, 1.0, {})
    assert "ROCm device" in why(edm, plain, False, False, 1.0, {})
    assert "dynamic_threshold" in why(A.EluDiffusion(0.2, dynamic_threshold=1.5), plain, True, False, 1.0, {})
    assert "dynamic_threshold" in why(A.EluDiffusion(0.2, dynamic_threshold=-0.1), plain, True, True, 1.0, {})
    for inference in (False, True):
        assert "x_mask" in why(edm, plain, True, inference, 1.0, {"x_mask": torch.ones(1, dtype=torch.bool)})
    # conditioning the device does not understand: inferring, conditioning_refusal decides
    assert why(edm, plain, True, True, 2.0, {}) and why(edm, plain, True, True, 1.0, {"classes": cl})
    assert why(edm, cc, True, True, 1.0, {}) and why(edm, cc, True, True, 1.0, {"classes": cl, "text_embeds": cl})
    # ... and not inferring
    assert "unconditional" in why(edm, plain, True, False, 1.0, {"classes": cl})
    assert "`classes`" in why(edm, cc, True, False, 1.0, {})
    assert "`classes`" in why(edm, cc, True, False, 1.0, {"classes": cl, "cond_drop_prob": 0.0})
    cc.cond_drop_prob = 0.3
    try:
        assert "random label mask" in why(edm, cc, True, False, 1.0, {"classes": cl})
        assert loss_route_refusal(edm, cc, True, True, 1.0, {"classes": cl}) is None       # inferring, the net's cond_drop_prob is not read
    finally:
        cc.cond_drop_prob = 0.0


def test_forward_keeps_the_training_guard_and_does_not_read_require_native(monkeypatch):
    plain, _ = _nets()
    x = torch.zeros(3, 1, 256)
    with pytest.raises(NotImplementedError, match="training loss"):
        A.EluDiffusion(0.2)(x, plain, torch.tensor(LR.SIGMAS))
    monkeypatch.setenv("ADF_REQUIRE_NATIVE", "1")
    with torch.no_grad():             # a host tensor stays on the tensor route, which reaches the net's own "no CPU fallback" error, not the env check
        with pytest.raises(RuntimeError, match="ROCm device"):
            A.EluDiffusion(0.2)(x, plain, torch.tensor(LR.SIGMAS))


# ---- the 1e-6 bar of the device's loss kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net_name", ["tiny", "tiny_cc", "u2d", "wn"])
def test_bar_derivation_on_the_gpu_tests_inputs(net_name):
    """On the inputs of tests/test_loss_gpu.py, around the fp32 oracle net: the kernels' arithmetic in NumPy against the float64 loss of the SAME
    prediction stays at or below half the bar; the conditions the derivation and the issue state hold on these inputs."""
    cfg, w = RC.weights(net_name, 1.0)
    net = RC.oracle_net(net_name, cfg, w, torch.float32)
    shape = RC.NETS[net_name][3]
    x, noise = LR.inputs(shape)
    assert float(x.abs().max()) <= 1.0
    for kind in LR.KINDS:
        coef = LR.coefs(kind, shape[0])
        sig = LR.sigmas_of(kind, coef)
        with torch.no_grad():
            x_noisy = LR.mix(kind, x, noise, sig)
            pred = RF.denoise(False, net, x_noisy, sigmas=coef) if kind == "rf" else P.denoise(kind, net, x_noisy, sigmas=sig)
        want = LR.loss_of_pred(kind, x.double(), noise, pred, sig)
        got = T(LR.emulate_loss(kind, x, noise, pred, sig))
        err = rel_b(got, want)
        print(net_name, kind, "losses", [round(float(v), 4) for v in want], "emulation vs float64", err)
        assert err <= 0.5 * LOSS_BAR, (net_name, kind, err)
        assert bool((want > 0).all())
        if kind == "rf":
            energy = ((noise.double() - x.double()) ** 2).reshape(shape[0], -1).mean(dim=1)
            assert bool((want >= 0.1 * energy).all()), (want, energy)             # the condition of the derivation
            assert bool((want >= 0.9 * energy).all())                            # what these inputs give
        elif kind == "edm":
            assert 1.0 <= float(want.min()) and float(want.max()) <= 4.8
            assert float((pred.abs() >= 1.0).double().mean()) <= 0.003           # the clamped estimate hardly saturates (VE's c_out = sigma = 7 does)
