"""CPU: the four table-driven samplers (VESampler, VPSampler, VSampler, VEulerSampler) -- their host tables against the fp32 scalars the reference's
classes formed (tests/golden/vsamp_golden.npz, written by tools/gen_golden_vsamp.py), their tensor-op branches against the reference's runs on a toy
``fn``, draw counts and generator state, the host logic of adf_sampler_table_nfe, and what the ABI still promises (no new sampler or preconditioning
kind, VDiffusion() refused everywhere else).  The device loop itself is tests/test_vsamp_gpu.py."""
import ctypes as C
import inspect
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
import audiodiffuser_amd.samplers as SM
from audiodiffuser_amd import _lib
import precond_ref as PR
import vsamp_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
CLS = {"ve": A.VESampler, "vp": A.VPSampler, "v": A.VSampler, "veuler": A.VEulerSampler}
# A tensor-op branch against a reference toy run: the same fp32 operations in the same order, so the results are expected equal; the bar leaves room
# for one rounding per step where an expression is associated differently (8 steps x 2^-24 ~ 5e-7).
TOY_PIN = 1e-6


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "vsamp_golden.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(ROOT, "tests", "golden", "vsamp_golden.json")) as f:
        return json.load(f)


def f32(v):
    return float(np.float32(v))


def make(case):
    kind, kw, sigmas = VC.TABLES[case]
    return kind, CLS[kind](**kw, use_graph=False), sigmas


def test_constructor_signatures_equal_the_reference(meta):
    for name, sig in meta["signatures"].items():
        got = [[k, None if p.default is inspect.Parameter.empty else p.default]
               for k, p in inspect.signature(getattr(A, name).__init__).parameters.items() if k != "self"]
        assert got == sig + [["use_graph", True]], (name, got, sig)         # this package's one extra keyword, as on every sampler


@pytest.mark.parametrize("case", [c for c, v in VC.TABLES.items() if v[0] in ("ve", "vp")])
def test_churn_tables_hold_the_reference_scalars_bit_for_bit(gold, case):
    """sigma(t_hat), sigma(t_prime) and the coefficients (a0, a1) of x_hat of every step, as the reference formed them -- including the steps with
    gamma = 0, whose noise coefficient is the fp32 round trip sigma_to_t(t_to_sigma(t)) and is asserted EQUAL to the reference's, whatever it is."""
    kind, smp, sigmas = make(case)
    assert np.array_equal(sigmas.numpy(), gold[f"{case}_sigmas"])
    sc = smp._scalars(sigmas)
    want_sig, want_a = gold[f"{case}_sigma"], gold[f"{case}_a"]
    assert len(sc) == len(want_sig) == smp.num_steps
    owner = A.VEDiffusion() if kind == "ve" else A.VPDiffusion(**PR.VP_ARGS)
    steps, x0, final_clamp, n_draws = smp._table(sigmas, owner)
    assert n_draws == smp.num_steps and final_clamp == (kind == "ve")
    zero_gamma = []
    for i, (r, st) in enumerate(zip(sc, steps)):
        assert r["sigma1"] == float(want_sig[i, 0]), (case, i)
        assert r["second"] == (not math.isnan(want_sig[i, 1])) == bool(st.second), (case, i)
        if r["second"]:
            assert r["sigma2"] == float(want_sig[i, 1]), (case, i)
        assert (r["a0"], r["a1"]) == (float(want_a[i, 0]), float(want_a[i, 1])), (case, i, r["a0"], r["a1"], want_a[i])
        assert (st.a0, st.a1, st.draw) == (f32(want_a[i, 0]), f32(want_a[i, 1]), i)                # ... and the records carry exactly these
        if r["gamma"] == 0.0:
            zero_gamma.append(float(want_a[i, 1]))
    print(case, "noise coefficients of the gamma = 0 steps:", zero_gamma)
    if "window" in case or "nochurn" in case:
        assert zero_gamma, "the case is meant to hold steps with gamma = 0"
    if "window" in case:
        assert any(r["gamma"] > 0 for r in sc)
    # the rows: the owner's get_scale_weights at exactly those sigmas, with 1 / scale folded into c_in and c_skip for VP
    ev_sig = torch.tensor([v for r in sc for v in ([r["sigma1"], r["sigma2"]] if r["second"] else [r["sigma1"]])])
    rows = PR.rows(kind, ev_sig).double()
    divs = [v for r in sc for v in ([r["div1"], r["div2"]] if r["second"] else [r["div1"]])]
    evs = [e for st in steps for e in ([st.eval1, st.eval2] if st.second else [st.eval1])]
    assert len(evs) == len(divs) == rows.shape[0]
    for k, (e, dv) in enumerate(zip(evs, divs)):
        want = (f32(rows[k, 0] / dv), f32(rows[k, 1]), f32(rows[k, 2] / dv), f32(rows[k, 3]))
        assert (e.c_in, e.c_noise, e.c_skip, e.c_out) == want and e.clip == _lib.CLIP_CONFIGURED, (case, k)
    assert steps[-1].second == 0                                                                  # the last step goes into t_next = 0


def test_a_zero_gamma_noise_coefficient_is_rounding_sized_and_not_zero(gold):
    """With gamma = 0 the reference still adds sqrt(clip(sigma(t_hat)^2 - sigma(t)^2, 0)) s_noise randn, t_hat = sigma_to_t(t_to_sigma(t)) in fp32.  On
    the recorded schedules VE's round trip (a square root squared) closes on every step -- the reference's coefficient is exactly 0 there, and so is
    the table's (asserted equal above) -- while VP's (exp / log) does not always: step 39 of the 50-step run carries a coefficient of rounding size
    that is not zero, in the reference and, bit for bit, in the table.  A restatement that sets x_hat = x where gamma = 0 would drop it."""
    for case in ("ve_nochurn_euler", "ve_window"):
        sc = make(case)[1]._scalars(make(case)[2])
        assert [r["a1"] for r in sc if r["gamma"] == 0.0] == [float(v) for v, r in zip(gold[f"{case}_a"][:, 1], sc) if r["gamma"] == 0.0]
    kind, smp, sigmas = make("vp_nochurn_50")
    sc, want = smp._scalars(sigmas), gold["vp_nochurn_50_a"][:, 1]
    assert all(r["gamma"] == 0.0 for r in sc)
    live = [i for i in range(50) if want[i] != 0.0]
    print("vp_nochurn_50: steps with a non-zero coefficient", [(i, float(want[i]), sc[i]["sigma1"]) for i in live])
    assert live, "the reference's run has no such step: pick another schedule"
    for i in live:      # sigma_hat^2 - sigma^2 is a few ulps (2^-23 each) of 1 + sigma^2: a1 ~ sqrt(k * 1.2e-7 (1 + sigma^2)) scale, far below 1e-2
        assert sc[i]["a1"] == float(want[i]) and 0.0 < sc[i]["a1"] < 1e-2, (i, sc[i]["a1"], float(want[i]))


@pytest.mark.parametrize("case", [c for c, v in VC.TABLES.items() if v[0] in ("v", "veuler")])
def test_vobj_tables_hold_the_reference_scalars_bit_for_bit(gold, case):
    kind, smp, ts = make(case)
    sc = smp._scalars(ts)
    want = gold[f"{case}_sigma"]
    steps, n_draws = smp._table(ts)
    assert len(sc) == len(steps) == smp.num_steps
    for i, (r, st) in enumerate(zip(sc, steps)):
        assert r["logsnr_t"] == float(want[i, 0]) and st.eval1.c_noise == f32(want[i, 0]), (case, i)
        assert bool(st.second) == (not math.isnan(want[i, 1])), (case, i)
        if st.second:
            assert r["logsnr_s"] == float(want[i, 1]) and st.eval2.c_noise == f32(want[i, 1])
        assert r["last"] == (i == smp.num_steps - 1)
        if kind == "v":
            std = float(gold[f"{case}_std"][i])
            assert (0.0 if r["last"] else r["std"]) == std and st.b2 == f32(std), (case, i)
            assert (st.eval1.c_in, st.eval1.c_skip, st.eval1.c_out, st.eval1.clip) == (1.0, f32(r["alpha_t"]), f32(-r["sigma_t"]), _lib.CLIP_UNIT)
        else:
            assert (st.eval1.c_in, st.eval1.c_skip, st.eval1.c_out, st.eval1.clip) == (1.0, 0.0, 1.0, _lib.CLIP_NONE)
            assert st.a1 == 0.0 and st.b2 == 0.0
    assert n_draws == (smp.num_steps - 1 if kind == "v" else 0)
    last = steps[-1]
    if kind == "veuler":                                                                          # the alpha x - sigma v branch
        assert (last.second, last.b0, last.b1) == (0, f32(sc[-1]["alpha_t"]), f32(-sc[-1]["sigma_t"]))


@pytest.mark.parametrize("case", list(VC.TABLES))
def test_tensor_op_branch_equals_the_reference_run_with_injected_and_with_drawn_noise(gold, meta, case):
    """The compatibility branch on the toy fn: with the recorded draws injected, and with its own draws from the reference's seed -- then the global
    generator is left where the reference leaves it (draw count and order)."""
    kind, smp, sigmas = make(case)
    noise, want, draws = VC.toy_noise(), T(gold[f"toy_{case}_out"]), T(gold[f"toy_{case}_draws"])
    assert draws.shape[0] == meta["toy"][case]["draws"] == {"ve": smp.num_steps, "vp": smp.num_steps, "v": smp.num_steps - 1, "veuler": 0}[kind]
    y = smp(noise, fn=VC.toy_fn, net=None, sigmas=sigmas, injected_noise=draws if draws.shape[0] else None)
    torch.manual_seed(VC.TOY_SEED + 1)
    y2 = smp(noise, fn=VC.toy_fn, net=None, sigmas=sigmas)
    nxt = torch.randn(4)
    e = float((y.double() - want.double()).abs().max() / want.double().abs().max())
    print(case, "rel err", e, "equal" if torch.equal(y, want) else "")
    assert e <= TOY_PIN and torch.equal(y2, y)
    assert torch.equal(nxt, T(gold[f"toy_{case}_next"])), "the run leaves the global generator in another state than the reference"
    if kind == "vp":
        assert "vp_shipped" != case or float(want.abs().max()) > 1.0            # VPSampler returns x unclamped
    else:
        assert float(y.abs().max()) <= 1.0


def _nfe(smp, steps):
    lib = _lib.load_library()
    d = _lib.AdfTableDesc(num_steps=len(steps), x0_scale=1.0, final_clamp=1, use_graph=0)
    return lib.adf_sampler_table_nfe(C.byref(d), (_lib.AdfTableStep * max(len(steps), 1))(*steps))


def test_table_nfe_via_abi():
    lib = _lib.load_library()
    sig = VC.sigmas_of(VC.spec("ve_tiny1_heun"))
    n = len(sig)
    for cls, owner in ((A.VESampler, A.VEDiffusion()), (A.VPSampler, A.VPDiffusion(**PR.VP_ARGS))):
        assert _nfe(None, cls(num_steps=n, use_heun=True)._table(sig, owner)[0]) == 2 * n - 1          # no correction into t_next = 0
        assert _nfe(None, cls(num_steps=n, use_heun=False)._table(sig, owner)[0]) == n
        assert _nfe(None, cls(num_steps=n - 1, use_heun=True)._table(sig, owner)[0]) == 2 * (n - 1)     # the run stops above 0: every step corrects
    ts = torch.linspace(0.9, 0.1, 6)
    assert _nfe(None, A.VSampler(num_steps=6)._table(ts)[0]) == 6
    assert _nfe(None, A.VEulerSampler(num_steps=6)._table(ts)[0]) == 6
    assert _nfe(None, A.VEulerSampler(num_steps=6, use_heun=True)._table(ts)[0]) == 11
    assert _nfe(None, A.VEulerSampler(num_steps=5, use_heun=True)._table(ts)[0]) == 10
    # malformed tables
    good = A.VEulerSampler(num_steps=3, use_heun=True)._table(torch.linspace(0.9, 0.3, 3))[0]
    assert _nfe(None, good) == 5
    d0 = _lib.AdfTableDesc(num_steps=0, x0_scale=1.0, final_clamp=1, use_graph=0)
    arr = (_lib.AdfTableStep * 3)(*good)
    assert lib.adf_sampler_table_nfe(C.byref(d0), arr) == -1
    assert lib.adf_sampler_table_nfe(None, arr) == -1 and lib.adf_sampler_table_nfe(C.byref(_lib.AdfTableDesc(num_steps=3, x0_scale=1.0)), None) == -1

    def broken(**fields):
        steps = A.VEulerSampler(num_steps=3, use_heun=True)._table(torch.linspace(0.9, 0.3, 3))[0]
        for k, v in fields.items():
            obj, name = (steps[0], k) if "." not in k else (getattr(steps[0], k.split(".")[0]), k.split(".")[1])
            setattr(obj, name, v)
        return _nfe(None, steps)
    assert broken(b0=0.0, b1=0.0, b2=0.0) == -1                      # D2 without x_e
    assert broken(c1=float("nan")) == -1 and broken(a0=float("inf")) == -1
    assert broken(**{"eval1.c_noise": float("nan")}) == -1 and broken(**{"eval2.clip": 3}) == -1
    assert broken(a0=0.0) == -1 and broken(c0=0.0, c1=0.0, c2=0.0, c3=0.0) == -1
    d_bad = _lib.AdfTableDesc(num_steps=3, x0_scale=float("nan"), final_clamp=1, use_graph=0)
    assert lib.adf_sampler_table_nfe(C.byref(d_bad), arr) == -1


def test_header_bindings_and_struct_layouts():
    hdr = open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("adf_sampler_run_table", "adf_sampler_table_nfe"):
        assert re.search(rf"\b{name}\s*\(", code) and name in _lib.EXPORTS
        assert hasattr(_lib.load_library(), name)
    assert (C.sizeof(_lib.AdfTableEval), C.sizeof(_lib.AdfTableStep), C.sizeof(_lib.AdfTableDesc)) == (20, 84, 16)
    for cname, pyc in (("adf_table_eval", _lib.AdfTableEval), ("adf_table_step", _lib.AdfTableStep), ("adf_table_desc", _lib.AdfTableDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), code, flags=re.S).group(1)
        names = [n.strip() for decl in re.findall(r"(?:float|int32_t|adf_table_eval)\s+([^;]+);", body) for n in decl.split(",")]
        assert names == [n for n, _ in pyc._fields_], (cname, names)
    for k in ("NONE", "CONFIGURED", "UNIT"):
        assert getattr(_lib, f"CLIP_{k}") == int(re.search(rf"#define ADF_CLIP_{k} (\d+)", hdr).group(1))


def test_the_pins_still_hold():
    hdr = open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")).read()
    lib = _lib.load_library()
    assert lib.adf_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define ADF_ABI_VERSION (\d+)", hdr).group(1)) == 7
    assert C.sizeof(_lib.AdfSamplerDesc) == 64 and C.sizeof(_lib.AdfRunCounters) == 48
    kinds = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ADF_PRECOND_([A-Z_]+) (\d+)\b", hdr)}
    assert kinds == {"EDM": 0, "VE": 1, "VP": 2, "V_EDM": 3, "RF": 4, "RF_EDM": 5}
    assert sorted(int(m.group(1)) for m in re.finditer(r"#define ADF_SAMPLER_[A-Z0-9_]+ (\d+)", hdr)) == list(range(11))
    d = A.ReflowEulerSampler(num_steps=6)._desc(1.0)
    d.kind = 11
    assert lib.adf_sampler_nfe(C.byref(d), (C.c_float * 7)(*torch.linspace(1, 0, 7).tolist()), 7) == -1
    v = A.VDiffusion()
    assert v._precond() is None and v._loss_kind() is None and "sampler_vobj" in v._not_native_note()
    net = A.UNet1dBase.from_config(A.config_tiny())
    assert "no device form" in A.diffusion.loss_route_refusal(v, net, True, True, 1.0, {})
    assert SM._native_pair(v.denoise_fn, net, 1.0, {}) is None                  # every other sampler still leaves the device with VDiffusion()


def test_native_pair_checks_and_require_native(monkeypatch):
    """Host logic of the two pair checks (no device): which (fn, net) pairs are native, and that ADF_REQUIRE_NATIVE turns the others into errors
    that say why."""
    net = A.UNet1dBase.from_config(A.config_tiny())
    on_host = torch.zeros(1, 1, 64)

    class Dev:                                                                  # stands in for a device tensor: only .is_cuda is read
        is_cuda = True
    vs, ve = A.VSampler(num_steps=3), A.VESampler(num_steps=3)
    v, v_edm = A.VDiffusion(), A.VDiffusion(for_edm=True)
    assert vs._owner(v.denoise_fn, net, {}, Dev()) is v and A.VEulerSampler(num_steps=3)._owner(v.denoise_fn, net, {}, Dev()) is v
    assert vs._owner(v_edm.denoise_fn, net, {}, Dev()) is None and vs._owner(A.VEDiffusion().denoise_fn, net, {}, Dev()) is None
    assert vs._owner(v.denoise_fn, net, {}, on_host) is None and vs._owner(v.denoise_fn, torch.nn.Identity(), {}, Dev()) is None
    assert vs._owner(v.denoise_fn, net, {"classes": torch.tensor([1])}, Dev()) is None
    for d in (A.EluDiffusion(sigma_data=0.2), A.VEDiffusion(), A.VPDiffusion(**PR.VP_ARGS), v_edm):
        assert ve._owner(d.denoise_fn, net, {}, Dev()) is d
    assert ve._owner(v.denoise_fn, net, {}, Dev()) is None and ve._owner(A.ReFlow().denoise_fn, net, {}, Dev()) is None
    monkeypatch.setattr(SM, "REQUIRE_NATIVE", True)
    with pytest.raises(RuntimeError, match="VSampler.*for_edm=True"):
        vs._owner(v_edm.denoise_fn, net, {}, Dev())
    with pytest.raises(RuntimeError, match="VESampler.*no device form"):
        ve._owner(v.denoise_fn, net, {}, Dev())
    with pytest.raises(RuntimeError, match="get_scale_weights"):
        ve._owner(A.ReFlow().denoise_fn, net, {}, Dev())
    with pytest.raises(RuntimeError, match="VEulerSampler.*not the denoise_fn"):
        A.VEulerSampler(num_steps=3)(torch.zeros(1, 1, 64), fn=VC.toy_fn, net=None, sigmas=torch.linspace(0.9, 0.1, 3))


def test_vp_int_c_skip_and_elu_rows_reach_the_table():
    """VPDiffusion / VEDiffusion return Python ints for some row entries; EluDiffusion's rows carry sigma_data."""
    sig = VC.sigmas_of(VC.spec("vp_tiny_heun"))
    steps = A.VPSampler(num_steps=len(sig), use_heun=False)._table(sig, A.VPDiffusion(**PR.VP_ARGS))[0]
    sc = A.VPSampler(num_steps=len(sig), use_heun=False)._scalars(sig)
    for st, r in zip(steps, sc):
        assert st.eval1.c_skip == f32(1.0 / r["div1"]) and st.eval1.c_out == f32(-r["sigma1"])
    steps = A.VESampler(num_steps=len(sig), use_heun=False)._table(sig, A.EluDiffusion(sigma_data=0.2))[0]
    sc = A.VESampler(num_steps=len(sig), use_heun=False)._scalars(sig)
    want = PR.rows("edm", torch.tensor([r["sigma1"] for r in sc]))
    for k, st in enumerate(steps):
        assert (st.eval1.c_in, st.eval1.c_noise, st.eval1.c_skip, st.eval1.c_out) == tuple(float(v) for v in want[k])
    assert A.VESampler(num_steps=len(sig))._table(sig, A.VDiffusion(for_edm=True))[0][0].eval1.clip == _lib.CLIP_NONE
