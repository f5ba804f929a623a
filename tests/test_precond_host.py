"""CPU: the VE / VP / v plugin classes and the five extra schedules against the reference's own values (tests/golden/precond_golden.npz, written
by tools/gen_golden_precond.py from the reference's classes), the compatibility-branch ``denoise_fn`` around oracle/unet2d.py, the finding that
two shipped sampler settings are not finite in the reference's own arithmetic, and ABI 7."""
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
from oracle import samplers as S, unet2d as U
import precond_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
ORACLE_PIN = 2.1e-6          # the bar at which oracle/unet2d.py is pinned to the reference's UNet2dBase (tests/test_oracle_unet2d.py)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "precond_golden.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(ROOT, "tests", "golden", "precond_golden.json")) as f:
        return json.load(f)


def diffusion_of(kind, **kw):
    return {"edm": lambda: A.EluDiffusion(sigma_data=0.2, **kw), "ve": lambda: A.VEDiffusion(**kw),
            "vp": lambda: A.VPDiffusion(beta_min=0.1, beta_d=19.9, M=1000, **kw), "v": lambda: A.VDiffusion(for_edm=True, **kw)}[kind]()


def schedule_of(name, n):
    return {"linear": lambda: A.LinearSchedule(start=1.0, end=0.0, num_steps=n), "geometric": lambda: A.GeometricSchedule(num_steps=n),
            "vp": lambda: A.VPSchedule(beta_d=19.9, beta_min=0.1, end=0.001, num_steps=n), "ve": lambda: A.VESchedule(sigma_max=100, sigma_min=0.02, num_steps=n),
            "v": lambda: A.VSchedule(num_steps=n), "karras": lambda: A.KarrasSchedule(0.002, 80.0, 7.0, n)}[name]()


@pytest.mark.parametrize("n", [30, 50])
@pytest.mark.parametrize("name", ["linear", "geometric", "vp", "ve", "v", "karras"])
def test_schedules_equal_the_reference_exactly(gold, name, n):
    sig = schedule_of(name, n)()
    assert sig.dtype == torch.float32 and sig.shape == (n,)
    assert np.array_equal(sig.numpy(), gold[f"sched_{name}_{n}"])


def plugin_rows(kind, sig):
    c_skip, c_out, c_in, c_noise = diffusion_of(kind).get_scale_weights(sig, 1)
    full = lambda v: v if torch.is_tensor(v) else torch.full_like(sig, float(v))
    return torch.stack([full(c_in), c_noise, full(c_skip), full(c_out)], dim=1)


@pytest.mark.parametrize("kind,sname", [("edm", "karras")] + [(k, s) for k in ("ve", "vp", "v") for s in ("ve", "vp", "v")])
def test_scale_weights_equal_the_reference_exactly(gold, kind, sname):
    sig = T(gold[f"sched_{sname}_30"])
    want = gold[f"rows_{kind}_{sname}"]
    assert np.array_equal(plugin_rows(kind, sig).numpy(), want)
    assert np.array_equal(PR.rows(kind, sig).numpy(), want)                      # the restatement the GPU tests lean on
    assert np.array_equal(PR.rows(kind, sig, torch.float64).numpy(), gold[f"rows64_{kind}_{sname}"])
    bar = gold[f"bar_{kind}_{sname}"]
    r64 = gold[f"rows64_{kind}_{sname}"]
    assert np.all(bar >= 1e-6) and np.all(np.abs(want.astype(np.float64) - r64) <= 0.25 * bar * np.abs(r64) * (1 + 1e-9) + 1e-300)     # bar = max(1e-6, 4 |fp32 - fp64| / |fp64|)


def test_vp_time_maps_and_loss_weights(gold):
    vp = A.VPDiffusion(beta_min=0.1, beta_d=19.9, M=1000)
    t = torch.linspace(1.0, 0.001, 30)
    assert np.array_equal(vp.t_to_sigma(t).numpy(), gold["sched_vp_30"])        # VPSchedule is t_to_sigma on its own grid
    sig = T(gold["sched_vp_30"])
    assert np.array_equal((999 * vp.sigma_to_t(sig)).numpy(), gold["rows_vp_vp"][:, 1])
    assert torch.equal(vp.loss_weight(sig), 1 / sig ** 2) and torch.equal(A.VEDiffusion().loss_weight(sig), 1 / (sig ** 2))
    assert torch.equal(A.EluDiffusion(0.2).loss_weight(sig), (sig ** 2 + 0.2 ** 2) * (sig * 0.2) ** -2)


def test_constructor_signatures_equal_the_reference(meta):
    for name, want in meta["signatures"].items():
        cls = getattr(A, name)
        got = [[k, None if p.default is inspect.Parameter.empty else p.default]
               for k, p in inspect.signature(cls.__init__).parameters.items() if k != "self"]
        assert got == want, (name, got, want)
    assert set(meta["signatures"]) >= {"VEDiffusion", "VPDiffusion", "VDiffusion", "EluDiffusion", "LinearSchedule", "GeometricSchedule", "VPSchedule",
                                       "VESchedule", "VSchedule"}


@pytest.mark.parametrize("kind", ["edm", "ve", "vp", "v"])
def test_compatibility_branch_denoise_fn_around_the_oracle_net_vs_reference(gold, meta, kind):
    """One inference call per kind (scalar sigma and [B] sigmas) on the plugin's tensor-op branch around oracle/unet2d.py, against what the
    reference's class returned around the reference's UNet2dBase with the same weights."""
    cfg, _ = U.fixture_variants()["small"]
    w = U.generate_weights(cfg, seed=5)
    classes = T(gold["den_classes"])
    net = lambda xi, ti, cond_drop_prob=0.0, classes=None: U.unet2d_forward(w, cfg, xi, ti, classes=classes, cond_drop_prob=cond_drop_prob)
    d = diffusion_of(kind)
    x = T(gold[f"den_{kind}_x"])
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    with torch.no_grad():
        ys = d.denoise_fn(x, net=net, inference=True, sigma=float(gold[f"den_{kind}_sigma"]), classes=classes)
        yb = d.denoise_fn(x, net=net, inference=True, sigmas=T(gold[f"den_{kind}_sigmas"]), classes=classes)
    ws, wb = T(gold[f"den_{kind}_y_scalar"]), T(gold[f"den_{kind}_y_batch"])
    es, eb = rel(ys, ws), rel(yb, wb)
    print(kind, "scalar", es, "batch", eb)
    assert es <= ORACLE_PIN and eb <= ORACLE_PIN, (kind, es, eb)
    assert float((ws.abs() >= 1).float().mean()) <= 0.5 and float(ws.abs().max()) > 0.05          # not hidden by the clamp, not dead
    if kind == "v":
        assert float(wb.abs().max()) > 1.0 and float(yb.abs().max()) > 1.0                        # VDiffusion does not clip
    else:
        assert float(yb.abs().max()) <= 1.0


def test_v_diffusion_ignores_dynamic_threshold_and_raw_v_needs_the_vobj_samplers():
    net = lambda xi, ti, cond_drop_prob=0.0: 3.0 * xi + ti.view(-1, 1, 1)
    x = torch.randn(2, 1, 8, generator=torch.Generator().manual_seed(0))
    a = A.VDiffusion(for_edm=True).denoise_fn(x, net=net, inference=True, sigma=0.7)
    b = A.VDiffusion(for_edm=True, dynamic_threshold=0.9).denoise_fn(x, net=net, inference=True, sigma=0.7)
    assert torch.equal(a, b) and float(a.abs().max()) > 1.0
    raw = A.VDiffusion().denoise_fn(x, net=net, inference=True, sigmas=torch.tensor([0.3, -0.2]))
    assert torch.equal(raw, 3.0 * x + torch.tensor([0.3, -0.2]).view(2, 1, 1))                  # for_edm=False: the v prediction at the given log-SNR
    assert A.VDiffusion()._precond() is None and "sampler_vobj" in A.VDiffusion()._not_native_note()


def small_case():
    cfg, _ = U.fixture_variants()["small"]
    w = U.generate_weights(cfg, seed=5)
    classes = torch.tensor([1, 4])
    net_o = lambda xi, ti, cond_drop_prob=0.0: U.unet2d_forward(w, cfg, xi, ti, classes=classes, cond_drop_prob=cond_drop_prob)
    noise = torch.randn(2, 2, 32, 16, generator=torch.Generator().manual_seed(11)) * 0.003
    return net_o, noise


@pytest.mark.parametrize("row", [5, 6])
def test_shipped_single_step_dpm_rows_are_not_finite_in_the_reference_arithmetic(row):
    """diffunet_complex_sc09_eval_ve_dpm.yaml (row 5) and ..._vobj_edm_dpm.yaml (row 6): DPMSampler(multisteps False, log_time_spacing False)
    forms its intermediate point as exp(-(sigma + r1 h)) (sampler_edm.py:584, :604); at VESchedule's 100 that is a denormal and (x - D) / sigma
    overflows, at VSchedule's 1808 it is 0 and ln 0 enters the net.  With log_time_spacing=True the same pair is finite."""
    net_o, noise = small_case()
    kind, order, x0 = ("ve", 3, False) if row == 5 else ("v", 2, True)
    fn = PR.make_fn(kind, net_o)
    sig = PR.shipped_schedule(kind, 30)
    with torch.no_grad():
        shipped = S.dpm_singlestep_sampler(noise, fn, sig, 30, order=order, log_time_spacing=False, x0_pred=x0)
        logsp = S.dpm_singlestep_sampler(noise, fn, sig, 30, order=order, log_time_spacing=True, x0_pred=x0)
    assert not bool(torch.isfinite(shipped).all())
    assert bool(torch.isfinite(logsp).all()) and float(logsp.abs().max()) > 0.05


def test_abi_7_symbols_constants_and_struct_layouts_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")).read()
    lib = _lib.load_library()
    assert lib.adf_abi_version() == 7 == _lib.ABI_VERSION
    for sym in ("adf_set_preconditioning", "adf_debug_coef_rows"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTS and re.search(rf"\b{sym}\s*\(", hdr)
    for name in ("EDM", "VE", "VP", "V_EDM"):
        assert getattr(_lib, f"PRECOND_{name}") == int(re.search(rf"#define ADF_PRECOND_{name} (\d+)", hdr).group(1))
    assert re.search(r"int adf_set_preconditioning\(adf_handle\* h, int kind, double beta_min, double beta_d, double M\);", hdr)
    assert _lib.EXPORTS["adf_set_preconditioning"][1] == [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]
    # every struct the binding mirrors: field names, order and offsets as a C compiler lays the header's declaration out (all members are
    # 4- or 8-byte scalars or arrays of them, so natural alignment is the whole rule)
    ctype_of = {"int32_t": (C.c_int32, 4), "float": (C.c_float, 4), "int64_t": (C.c_int64, 8), "double": (C.c_double, 8)}
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (ADF_[A-Z0-9_]+) (\d+)\b", hdr)}
    for cname, pyc in (("adf_sampler_desc", _lib.AdfSamplerDesc), ("adf_run_counters", _lib.AdfRunCounters), ("adf_wavenet_config", _lib.AdfWaveNetConfig),
                       ("adf_adm_config", _lib.AdfAdmConfig), ("adf_unet2d_config", _lib.AdfUNet2dConfig), ("adf_net_config", _lib.AdfNetConfig)):
        body = re.search(rf"typedef struct {cname} \{{(.*?)\}} {cname};", hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        want, off = [], 0
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            ty, rest = decl.split(None, 1)
            ct, size = ctype_of[ty]
            for item in rest.split(","):
                m = re.match(r"\s*(\w+)\s*(?:\[(.+)\])?\s*$", item)
                count = 1
                if m.group(2):
                    count = eval(m.group(2), {"__builtins__": {}}, consts)
                off = (off + size - 1) // size * size
                want.append((m.group(1), off, size * count))
                off += size * count
        got = [(n, getattr(pyc, n).offset, getattr(pyc, n).size) for n, _ in pyc._fields_]
        assert got == want, (cname, got, want)
        align = max(size for _, _, size in [(n, o, ctype_of[d.strip().split(None, 1)[0]][1]) for d in body.split(';') if d.strip() for n, o in [(0, 0)]])
        assert C.sizeof(pyc) == (off + align - 1) // align * align, cname
    assert C.sizeof(_lib.AdfSamplerDesc) == 64          # unchanged since version 6: a caller that fills only those fields still gets EluDiffusion


def test_native_pair_accepts_the_new_owners_and_names_what_is_not_built(monkeypatch):
    import audiodiffuser_amd.samplers as SM
    net = A.UNet1dBase.from_config(A.config_tiny())
    for d in (A.EluDiffusion(0.2), A.VEDiffusion(), A.VPDiffusion(0.1, 19.9, 1000), A.VDiffusion(for_edm=True)):
        assert SM._native_pair(d.denoise_fn, net, 1.0, {}) is d
    monkeypatch.setattr(SM, "REQUIRE_NATIVE", False)
    assert SM._native_pair(A.VDiffusion().denoise_fn, net, 1.0, {}) is None
    monkeypatch.setattr(SM, "REQUIRE_NATIVE", True)
    with pytest.raises(RuntimeError, match="sampler_vobj"):
        SM._native_pair(A.VDiffusion().denoise_fn, net, 1.0, {})
    monkeypatch.setenv("ADF_REQUIRE_NATIVE", "1")
    with pytest.raises(RuntimeError, match="sampler_vobj"):
        A.VDiffusion().denoise_fn(torch.zeros(1, 1, 256), net=net, inference=True, sigma=0.5)
