"""CPU: the two program-driven samplers (VDPMSampler, VUniPCSampler) -- their host scalars against what the reference's classes formed
(tests/golden/vdpm_golden.npz, written by tools/gen_golden_vdpm.py), the structure of their programs in every mode, their tensor-op branches
against the reference's runs on a toy ``fn``, the host logic of adf_sampler_program_nfe, and what the ABI still promises.  The device loop itself is
tests/test_vdpm_gpu.py."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
import audiodiffuser_amd.samplers as SM
from audiodiffuser_amd import _lib
import vdpm_cases as DC
import vdpm_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
CLS = {"dpm": A.VDPMSampler, "unipc": A.VUniPCSampler}
# A tensor-op branch against a reference toy run: the same fp32 operations in the same order, so the results are expected equal (tests/test_vsamp_host.py).
TOY_PIN = 1e-6
EVAL, LIN = _lib.PROG_EVAL, _lib.PROG_LIN


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "vdpm_golden.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(ROOT, "tests", "golden", "vdpm_golden.json")) as f:
        return json.load(f)


def f32(v):
    return float(np.float32(v))


def make(case):
    kind, kw, sigmas = DC.CASES[case]
    return kind, CLS[kind](**kw, use_graph=False), sigmas


def nfe_of(ops, result=0, x0=1.0, num_ops=None):
    d = _lib.AdfProgDesc(num_ops=len(ops) if num_ops is None else num_ops, result_slot=result, x0_scale=x0, use_graph=0)
    return _lib.load_library().adf_sampler_program_nfe(C.byref(d), (_lib.AdfProgOp * max(len(ops), 1))(*ops))


def emulate(ops, x0_scale, result, noise, fn):
    """The program as the header defines it, on the CPU with a float64 state and the fp32 rows and coefficients of the ops."""
    slots = {0: float(np.float32(x0_scale)) * noise.double()}
    for o in ops:
        if o.kind == EVAL:
            e, x = o.eval, slots[o.src]
            assert e.clip == _lib.CLIP_NONE and o.dst != o.src
            slots[o.dst] = e.c_skip * x + e.c_out * fn(e.c_in * x, torch.tensor(e.c_noise))
        else:
            v = sum(o.coef[j] * slots[o.slot[j]] for j in range(o.n_terms))
            slots[o.dst] = v.clamp(-1.0, 1.0) if o.clamp else v
    return slots[result]


def test_constructor_signatures_equal_the_reference(meta):
    for name, sig in meta["signatures"].items():
        got = [[k, None if p.default is inspect.Parameter.empty else p.default]
               for k, p in inspect.signature(getattr(A, "V" + name).__init__).parameters.items() if k != "self"]
        assert got == sig + [["use_graph", True]], (name, got, sig)         # this package's one extra keyword, as on every sampler


@pytest.mark.parametrize("case", list(DC.CASES))
def test_scalars_and_rows_are_the_reference_values_bit_for_bit(gold, meta, case):
    """The log-SNR of every evaluation the device makes is, in order, what the reference handed ``fn`` on its used calls; the rows carry alpha and sigma
    as the reference forms them; the ``rhos`` of a UniPC run are what the reference's own ``torch.linalg.solve`` calls returned."""
    kind, smp, sigmas = make(case)
    assert np.array_equal(sigmas.numpy(), gold[f"{case}_sigmas"])
    logsnr, used = gold[f"{case}_logsnr"], gold[f"{case}_used"]
    want = [float(v) for v, u in zip(logsnr, used) if u]
    sc = smp._scalars(sigmas)
    ops, x0_scale, result = smp._program(sigmas)
    evs = [o for o in ops if o.kind == EVAL]
    assert [o.eval.c_noise for o in evs] == want, case
    if kind == "unipc":                                                        # ... and they are the `l` entries of _scalars
        assert [sc["grid"][0]] + [r["l"] for r in sc["steps"] if r["corr"]] == want
    else:
        assert ([sc["grid"][0]] if smp.multisteps else []) + [l for r in sc["steps"] for l in r["l"]] == want
    for o in evs:
        l = torch.tensor(o.eval.c_noise)
        sig, alp = float(torch.sqrt(torch.sigmoid(-l))), float(torch.sqrt(torch.sigmoid(l)))
        assert (o.eval.c_in, o.eval.c_skip, o.eval.c_out, o.eval.clip) == ((1.0, alp, -sig, 0) if smp.x0_pred else (1.0, sig, alp, 0)), case
    assert x0_scale == (float(sigmas[0]) if kind == "unipc" else 1.0) and result == 0
    assert len(want) == meta["toy"][case]["calls_used"] and len(logsnr) == meta["toy"][case]["calls"]
    if kind == "unipc":
        mine = [r[k] for r in sc["steps"] for k in ("rhos_p", "rhos_c") if len(r[k]) > 1]
        solves = gold[f"{case}_solves"]
        assert len(mine) == len(solves), case
        for a, s in zip(mine, solves):
            assert a == [float(v) for v in s[:len(a)]] and bool(np.isnan(s[len(a):]).all()), (case, a, s)
        for r in sc["steps"]:                                                  # the hard-wired simplifications (:611-621)
            assert r["rhos_p"] == ([] if r["order"] == 1 else [0.5] if r["order"] == 2 else r["rhos_p"])
            assert r["rhos_c"] == ([] if not r["corr"] else [0.5] if r["order"] == 1 else r["rhos_c"])
    else:
        assert gold[f"{case}_solves"].shape == (0, 3)


@pytest.mark.parametrize("case", list(DC.CASES))
def test_compat_branch_equals_the_reference_run_and_makes_its_calls(gold, case):
    """The tensor-op branch on the toy fn: the reference's result, and the reference's ``fn`` calls one for one -- the discarded ones included."""
    kind, smp, sigmas = make(case)
    noise, want, seen = DC.toy_noise(DC.toy_scale(DC.CASES[case][1])), T(gold[f"toy_{case}_out"]), []

    def fn(x, net=None, sigma=None, inference=None, cond_scale=None, **kw):
        assert inference is True and cond_scale == 1.0 and not kw
        seen.append(float(sigma))
        return DC.toy_fn(x, sigma)
    y = smp(noise, fn=fn, net=None, sigmas=sigmas)
    e = float((y.double() - want.double()).abs().max() / want.double().abs().max())
    print(case, "rel err", e, "equal" if torch.equal(y, want) else "")
    assert e <= TOY_PIN and float(y.abs().max()) <= 1.0
    assert seen == [float(v) for v in gold[f"{case}_logsnr"]]


@pytest.mark.parametrize("case", list(DC.CASES))
def test_program_is_the_reference_loop(gold, meta, case):
    """The program, run as the header defines it on a float64 state, against the restatement in float64 (equal to the reference's toy run in fp32, bit
    for bit, by the generator).  Both use the reference's fp32 scalars; the program rounds each combined coefficient to fp32 once more, so the two
    differ by a few 2^-24 per update times the growth of the run: the bar is the project's max(TOY_PIN, 4 * the restatement's own fp32-vs-float64
    distance)."""
    kind, smp, sigmas = make(case)
    kw = DC.CASES[case][1]
    noise = DC.toy_noise(DC.toy_scale(kw))
    with torch.no_grad():
        if kind == "dpm":
            y64 = DR.dpm_sampler(noise.double(), DC.toy_fn, sigmas, kw["num_steps"], kw["order"], kw.get("multisteps", False), kw.get("x0_pred", True))
        else:
            y64 = DR.unipc_sampler(noise.double(), DC.toy_fn, sigmas, kw["num_steps"], kw["order"], kw.get("x0_pred", True))
    top = float(y64.abs().max())
    dist = float((T(gold[f"toy_{case}_out"]).double() - y64).abs().max() / top)
    ops, x0_scale, result = smp._program(sigmas)
    y = emulate(ops, x0_scale, result, noise, DC.toy_fn)
    e = float((y - y64).abs().max() / top)
    print(case, "program vs float64 restatement", e, "reference fp32 vs float64", dist)
    assert dist < 2.5e-4 and e <= max(TOY_PIN, 4 * dist), (case, e, dist)
    assert nfe_of(ops, result, x0_scale) == meta["toy"][case]["calls_used"]


def kinds(ops):
    return "".join("E" if o.kind == EVAL else str(o.n_terms) for o in ops)


def test_singlestep_program_structure():
    """Order lists at num_steps % 3 in {0, 1, 2} and % 2 in {0, 1}; per step E (the first evaluation), then per inner point one update and one
    evaluation, then the update of x.  An order-2 step's closing update has two operands: with r1 = 1/2 the coefficient of eps, -B + C, is exactly 0."""
    D = lambda **kw: A.VDPMSampler(1.0, multisteps=False, **kw)
    assert D(order=3, num_steps=6).singlestep_orders() == ([3, 2, 1], 3) and D(order=3, num_steps=7).singlestep_orders() == ([3, 3, 1], 3)
    assert D(order=3, num_steps=8).singlestep_orders() == ([3, 3, 2], 3) and D(order=3, num_steps=2).singlestep_orders() == ([2], 1)
    assert D(order=3, num_steps=1).singlestep_orders() == ([1], 1)
    assert D(order=2, num_steps=6).singlestep_orders() == ([2, 2, 2], 3) and D(order=2, num_steps=5).singlestep_orders() == ([2, 2, 1], 3)
    assert D(order=1, num_steps=4).singlestep_orders() == ([1] * 4, 4)
    step = {1: "E2", 2: "E2E2", 3: "E2E3E3"}
    for case in ("dpm_s3_n6", "dpm_s3_n7_eps", "dpm_s3_n8", "dpm_s3_n2_eps", "dpm_s2_n6_eps", "dpm_s2_n5", "dpm_s1_n4"):
        _, smp, sigmas = make(case)
        orders, k = smp.singlestep_orders()
        ops, x0_scale, result = smp._program(sigmas)
        assert kinds(ops) == "".join(step[o] for o in orders), (case, kinds(ops))
        assert len(smp._scalars(sigmas)["grid"]) == k + 1 and nfe_of(ops) == sum(orders) == smp.num_steps
        lins = [o for o in ops if o.kind == LIN]
        assert [o.clamp for o in lins] == [0] * (len(lins) - 1) + [1] and lins[-1].dst == 0 == result
        assert all(0 <= s < 5 for o in ops for s in ([o.dst, o.src] if o.kind == EVAL else [o.dst] + list(o.slot[:o.n_terms])))
    with pytest.raises(ValueError, match="'order' must be"):
        D(order=4, num_steps=8)(torch.zeros(1, 1, 4, 4), fn=DC.toy_fn, net=None, sigmas=torch.linspace(1, 0, 8))


def test_multistep_program_structure():
    """Warm-up at orders 1 .. order - 1, trailing lower orders, num_steps == order as the edge; the discarded evaluations are not in the program; the
    history is renamed, never copied: every update reads the newest ``order`` evaluation slots, and no evaluation overwrites one still to be read."""
    D = lambda **kw: A.VDPMSampler(1.0, multisteps=True, **kw)
    assert D(order=3, num_steps=6).multistep_orders() == [1, 2, 3, 3, 2, 1] and D(order=3, num_steps=3).multistep_orders() == [1, 2, 1]
    assert D(order=2, num_steps=5).multistep_orders() == [1, 2, 2, 2, 1] and D(order=2, num_steps=2).multistep_orders() == [1, 1]
    assert D(order=1, num_steps=3).multistep_orders() == [1, 1, 1]
    for case in ("dpm_m3_n6", "dpm_m3_n6_eps", "dpm_m3_n3", "dpm_m2_n5_eps", "dpm_m2_n2", "dpm_m1_n3"):
        _, smp, sigmas = make(case)
        orders = smp.multistep_orders()
        ops, _, result = smp._program(sigmas)
        assert kinds(ops) == "E" + "E".join(str(o + 1) for o in orders), (case, kinds(ops))
        assert nfe_of(ops) == smp.num_steps and ops[-1].clamp == 1 and sum(o.clamp for o in ops if o.kind == LIN) == 1
        hist = []
        for o in ops:
            if o.kind == EVAL:
                assert o.src == 0 and o.dst != 0
                assert smp.order == 1 or o.dst not in hist[-(smp.order - 1):], (case, o.dst, hist)
                hist.append(o.dst)
            else:
                n = o.n_terms - 1
                assert o.dst == 0 and o.slot[0] == 0 and list(o.slot[1:o.n_terms]) == hist[::-1][:n], (case, list(o.slot), hist)
    with pytest.raises(AssertionError):
        D(order=3, num_steps=2)(torch.zeros(1, 1, 4, 4), fn=DC.toy_fn, net=None, sigmas=torch.linspace(1, 0, 2))


def test_unipc_program_structure():
    """Per corrected update: the predictor into slot 1, its evaluation, the corrected x over x, the history and the new output -- 3, 4 and 5 operands at
    orders 1, 2 and 3; the last update is the predictor alone, into x, clamped."""
    P = lambda **kw: A.VUniPCSampler(**kw)
    assert P(num_steps=6, order=3).update_plan() == [(1, True), (2, True), (3, True), (3, True), (2, True), (1, False)]
    assert P(num_steps=3, order=3).update_plan() == [(1, True), (2, True), (1, False)] and P(num_steps=4, order=1).update_plan() == [(1, True)] * 3 + [(1, False)]
    assert P(num_steps=6, order=2).update_plan() == [(1, True)] + [(2, True)] * 4 + [(1, False)]
    for case in ("unipc_o1_n4", "unipc_o2_n6", "unipc_o2_n5_eps", "unipc_o3_n6", "unipc_o3_n6_eps", "unipc_o3_n3", "unipc_o1_n1"):
        _, smp, sigmas = make(case)
        plan = smp.update_plan()
        ops, _, result = smp._program(sigmas)
        assert kinds(ops) == "E" + "".join(f"{o + 1}E{o + 2}" if corr else f"{o + 1}" for o, corr in plan), (case, kinds(ops))
        assert plan[-1][1] is False and all(corr for _, corr in plan[:-1])
        assert nfe_of(ops) == smp.num_steps and ops[-1].clamp == 1 and sum(o.clamp for o in ops if o.kind == LIN) == 1 and result == 0
        assert max(s for o in ops for s in ([o.dst, o.src] if o.kind == EVAL else [o.dst] + list(o.slot[:o.n_terms]))) <= 5
        for i, o in enumerate(ops):
            if o.kind == EVAL and i:                                       # a corrector evaluation: of the predictor's state, read by the next update
                assert o.src == 1 and ops[i - 1].dst == 1 and ops[i + 1].dst == 0 and o.dst in list(ops[i + 1].slot[:ops[i + 1].n_terms])
    assert "5" in kinds(A.VUniPCSampler(num_steps=6, order=3)._program(torch.linspace(1, 0, 6))[0])
    with pytest.raises(AssertionError):
        P(num_steps=2, order=3)(torch.zeros(1, 1, 4, 4), fn=DC.toy_fn, net=None, sigmas=torch.linspace(1, 0, 2))


def test_unipc_compat_takes_any_rank():
    """The one deliberate widening: the reference's einsum takes 4-D states only; the same numbers as a 3-D state give the same result."""
    _, smp, sigmas = make("unipc_o3_n6")
    noise = DC.toy_noise()
    y4 = smp(noise, fn=DC.toy_fn, net=None, sigmas=sigmas)
    y3 = smp(noise.reshape(2, 1, 16), fn=DC.toy_fn, net=None, sigmas=sigmas)
    assert torch.equal(y3.reshape(y4.shape), y4)


def _good():
    return A.VUniPCSampler(num_steps=5, order=3)._program(torch.linspace(1, 0, 5))[0]


def test_program_nfe_refuses_every_malformed_program():
    lib = _lib.load_library()
    ops = _good()
    assert kinds(ops) == "E2E33E44E53E42" and nfe_of(ops) == 5
    arr = (_lib.AdfProgOp * len(ops))(*ops)
    d = lambda **kw: _lib.AdfProgDesc(**{**dict(num_ops=len(ops), result_slot=0, x0_scale=1.0, use_graph=0), **kw})
    assert lib.adf_sampler_program_nfe(None, arr) == -1 and lib.adf_sampler_program_nfe(C.byref(d()), None) == -1
    assert lib.adf_sampler_program_nfe(C.byref(d(num_ops=0)), arr) == -1 and lib.adf_sampler_program_nfe(C.byref(d(num_ops=-3)), arr) == -1
    assert lib.adf_sampler_program_nfe(C.byref(d(x0_scale=float("nan"))), arr) == -1
    assert lib.adf_sampler_program_nfe(C.byref(d(result_slot=8)), arr) == -1
    assert lib.adf_sampler_program_nfe(C.byref(d(result_slot=-1)), arr) == -1
    assert lib.adf_sampler_program_nfe(C.byref(d(result_slot=7)), arr) == -1                          # a slot nothing has written
    assert lib.adf_sampler_program_nfe(C.byref(d(result_slot=2)), arr) == 5                           # any written slot may be the result

    def broken(i, **fields):
        ops = _good()
        for k, v in fields.items():
            if k in ("slot", "coef"):
                getattr(ops[i], k)[v[0]] = v[1]
            elif "." in k:
                setattr(ops[i].eval, k.split(".")[1], v)
            else:
                setattr(ops[i], k, v)
        return nfe_of(ops)
    nan, inf = float("nan"), float("inf")
    assert broken(0, kind=2) == -1 and broken(1, kind=-1) == -1                                       # an unknown kind
    assert broken(0, dst=8) == -1 and broken(0, dst=-1) == -1 and broken(0, src=9) == -1              # slots outside [0, 8)
    assert broken(1, slot=(1, 8)) == -1 and broken(1, slot=(0, -2)) == -1
    assert broken(0, src=3) == -1 and broken(1, slot=(1, 6)) == -1                                    # reads of unwritten slots
    assert broken(0, dst=0) == -1                                                                     # an evaluation onto its input
    assert broken(1, n_terms=0) == -1 and broken(1, n_terms=6) == -1
    assert broken(1, slot=(1, 0)) == -1                                                               # the same slot twice
    assert broken(1, coef=(0, nan)) == -1 and broken(3, coef=(2, inf)) == -1
    assert broken(0, **{"eval.c_noise": nan}) == -1 and broken(2, **{"eval.c_out": inf}) == -1
    assert broken(0, **{"eval.clip": 3}) == -1 and broken(0, **{"eval.clip": _lib.CLIP_UNIT}) == 5
    lin = SM._VObjProgramSampler._lin
    assert nfe_of([lin(0, [(0, 0.5)])]) == -1                                                         # a program without an evaluation
    assert nfe_of(ops, num_ops=1) == 1                                                                # ... one evaluation is a program
    assert nfe_of([lin(1, [(0, 1.0)]), lin(0, [(0, 1.0), (1, 2.0)], True)] + ops) == 5                # dst may be an operand; a LIN writes its slot


def test_header_bindings_and_struct_layouts():
    hdr = open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("adf_sampler_run_program", "adf_sampler_program_nfe"):
        assert re.search(rf"\b{name}\s*\(", code) and name in _lib.EXPORTS
        assert hasattr(_lib.load_library(), name)
    assert (C.sizeof(_lib.AdfProgOp), C.sizeof(_lib.AdfProgDesc)) == (12 + 20 + 4 + 20 + 20 + 4, 16)
    for cname, pyc in (("adf_prog_op", _lib.AdfProgOp), ("adf_prog_desc", _lib.AdfProgDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), code, flags=re.S).group(1)
        names = [re.sub(r"\[.*\]", "", n).strip() for decl in re.findall(r"(?:float|int32_t|adf_table_eval)\s+([^;]+);", body) for n in decl.split(",")]
        assert names == [n for n, _ in pyc._fields_], (cname, names)
        assert not re.search(r"\b(double|int64_t|char)\b|\*", body), "4-byte scalars and adf_table_eval only"
    for k in ("EVAL", "LIN", "SLOTS", "TERMS"):
        assert getattr(_lib, f"PROG_{k}") == int(re.search(rf"#define ADF_PROG_{k} (\d+)", hdr).group(1))
    assert (_lib.PROG_SLOTS, _lib.PROG_TERMS) == (8, 5)


def test_the_pins_still_hold():
    hdr = open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")).read()
    lib = _lib.load_library()
    assert lib.adf_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define ADF_ABI_VERSION (\d+)", hdr).group(1)) == 7
    assert C.sizeof(_lib.AdfSamplerDesc) == 64 and C.sizeof(_lib.AdfRunCounters) == 48
    assert (C.sizeof(_lib.AdfTableEval), C.sizeof(_lib.AdfTableStep), C.sizeof(_lib.AdfTableDesc)) == (20, 84, 16)
    kinds_ = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ADF_PRECOND_([A-Z_]+) (\d+)\b", hdr)}
    assert kinds_ == {"EDM": 0, "VE": 1, "VP": 2, "V_EDM": 3, "RF": 4, "RF_EDM": 5}
    assert sorted(int(m.group(1)) for m in re.finditer(r"#define ADF_SAMPLER_[A-Z0-9_]+ (\d+)", hdr)) == list(range(11))
    v = A.VDiffusion()
    note = v._not_native_note()
    assert v._precond() is None and v._loss_kind() is None and "sampler_vobj" in note and "not built" not in note
    assert all(k in note for k in ("VSampler", "VEulerSampler", "VDPMSampler", "VUniPCSampler"))
    net = A.UNet1dBase.from_config(A.config_tiny())
    assert SM._native_pair(v.denoise_fn, net, 1.0, {}) is None                  # every sampler_edm sampler still leaves the device with VDiffusion()
    SM_REQ = SM.REQUIRE_NATIVE
    try:
        SM.REQUIRE_NATIVE = True
        with pytest.raises(RuntimeError, match="sampler_vobj"):
            SM._native_pair(v.denoise_fn, net, 1.0, {})
    finally:
        SM.REQUIRE_NATIVE = SM_REQ
    for doc in ("README.md", "INTEGRATION.md"):
        assert "ten of ten" in open(os.path.join(ROOT, doc)).read().lower(), doc


def test_native_pair_checks_and_refusal_texts(monkeypatch):
    """Host logic of the pair check (no device): which calls are native, and that ADF_REQUIRE_NATIVE turns the others into errors that start with
    the class name and say why."""
    net, net_cc = A.UNet1dBase.from_config(A.config_tiny()), A.UNet1dBase.from_config(A.config_tiny_cc())
    on_host = torch.zeros(1, 1, 64)

    class Dev:                                                                  # stands in for a device tensor: only .is_cuda is read
        is_cuda = True
    v, v_edm, cl = A.VDiffusion(), A.VDiffusion(for_edm=True), {"classes": torch.tensor([1])}
    D, P = A.VDPMSampler, A.VUniPCSampler
    for smp in (D(1.0, order=3, num_steps=7, x0_pred=False), D(1.0, order=3, num_steps=6, multisteps=True), P(num_steps=6, order=2), P(num_steps=5, order=3)):
        assert smp._owner(v.denoise_fn, net, {}, Dev()) is v                                        # unconditional nets: native throughout
        assert smp._owner(v_edm.denoise_fn, net, {}, Dev()) is None and smp._owner(A.VEDiffusion().denoise_fn, net, {}, Dev()) is None
        assert smp._owner(v.denoise_fn, net, {}, on_host) is None and smp._owner(v.denoise_fn, torch.nn.Identity(), {}, Dev()) is None
        assert smp._owner(v.denoise_fn, net, cl, Dev()) is None and smp._owner(DC.toy_fn, net, {}, Dev()) is None
    assert D(1.0, order=4, num_steps=8, multisteps=True)._owner(v.denoise_fn, net, {}, Dev()) is None
    assert P(num_steps=8, order=4)._owner(v.denoise_fn, net, {}, Dev()) is None
    # class-conditional: native where the reference hands `classes` to every evaluation
    for smp in (D(3.0, order=3, num_steps=6, multisteps=True), D(1.0, order=1, num_steps=4, multisteps=True), D(1.0, order=1, num_steps=4),
                D(2.0, order=3, num_steps=1), D(2.0, order=2, num_steps=1), P(num_steps=1, order=1, cond_scale=2.0)):
        assert smp._owner(v.denoise_fn, net_cc, cl, Dev()) is v, smp
    for smp in (D(1.0, order=3, num_steps=6), D(1.0, order=2, num_steps=3), D(1.0, order=3, num_steps=2), P(num_steps=4, order=1), P(num_steps=6, order=2)):
        assert smp._owner(v.denoise_fn, net_cc, cl, Dev()) is None, smp
    assert D(3.0, order=3, num_steps=6, multisteps=True)._owner(v.denoise_fn, net_cc, {}, Dev()) is None
    monkeypatch.setattr(SM, "REQUIRE_NATIVE", True)
    with pytest.raises(RuntimeError, match=r"^VDPMSampler: ADF_REQUIRE_NATIVE.*reference drops `classes`.*single-step"):
        D(1.0, order=3, num_steps=6)._owner(v.denoise_fn, net_cc, cl, Dev())
    with pytest.raises(RuntimeError, match=r"^VUniPCSampler: ADF_REQUIRE_NATIVE.*reference drops `classes`.*corrector"):
        P(num_steps=6, order=2)._owner(v.denoise_fn, net_cc, cl, Dev())
    with pytest.raises(RuntimeError, match=r"^VUniPCSampler.*order = 4"):
        P(num_steps=8, order=4)._owner(v.denoise_fn, net, {}, Dev())
    with pytest.raises(RuntimeError, match=r"^VDPMSampler.*order = 5"):
        D(1.0, order=5, num_steps=8, multisteps=True)._owner(v.denoise_fn, net, {}, Dev())
    with pytest.raises(RuntimeError, match=r"^VDPMSampler.*for_edm=True"):
        D(1.0, order=3, num_steps=6)._owner(v_edm.denoise_fn, net, {}, Dev())
    with pytest.raises(RuntimeError, match=r"^VUniPCSampler.*not on a ROCm device"):
        P(num_steps=6, order=2)._owner(v.denoise_fn, net, {}, on_host)
    with pytest.raises(RuntimeError, match=r"^VUniPCSampler.*not one of this package's HIP networks"):
        P(num_steps=6, order=2)._owner(v.denoise_fn, torch.nn.Identity(), {}, Dev())
    with pytest.raises(RuntimeError, match=r"^VDPMSampler.*unconditional net"):
        D(2.0, order=3, num_steps=6)._owner(v.denoise_fn, net, {}, Dev())
    with pytest.raises(RuntimeError, match=r"^VDPMSampler.*not the denoise_fn"):
        D(1.0, order=3, num_steps=6)(torch.zeros(1, 1, 4, 4), fn=DC.toy_fn, net=None, sigmas=torch.linspace(1, 0, 6))
