"""GPU: rectified flow on the device -- the two preconditioning kinds ADF_PRECOND_RF / ADF_PRECOND_RF_EDM (ReFlow in both modes) and the sampler
kind ADF_SAMPLER_RF_EULER (ReflowEulerSampler: Euler, or Heun wherever sigma_next != 0), eager and graph-replayed, on all four networks.

What a result is compared with: the CPU restatement tests/rf_ref.py (pinned to the reference's classes by tools/gen_golden_rf.py) in FLOAT64 around
the oracle nets, on the runs of tests/rf_cases.py.  The ADM oracle only runs in fp32, so its cases are compared with the fp32 restatement.  The bar of
a single call is the project's 1e-3 (max-norm, relative to max |ref|); the bar of a run is max(1e-3, 4 * dist_fp32_fp64) with the fp32-vs-float64
distance of the CPU restatement recorded in tests/golden/rf_golden.json (1e-7 .. 3e-6 for every run: 1e-3 throughout).  Every run that ends in
clamp(-1, 1) has at most 1 % of its reference at |y| >= 1 (asserted by the generator and again here), except the clamp test, which wants the opposite.

Only the WaveNet cases have an element count that is no multiple of 4 (3 x 501: the scalar tail of the two update kernels): L of the 1-D U-Net is a
multiple of its down-sampling factor and H * W of both 2-D nets a multiple of 256.

Measured on one MI355X: tests/golden/rf_report.json."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
import rf_cases as RC
import rf_ref as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
TOL = 1e-3                   # the project's bar for a whole run and for one call (tests/test_unet2d_gpu.py, tests/test_precond_gpu.py)
BF16_TOL = 6e-2              # tests/test_gpu_parity.py: bf16 storage against the fp32 mode


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "rf_golden.npz"))


@pytest.fixture(scope="module")
def runs():
    with open(os.path.join(ROOT, "tests", "golden", "rf_golden.json")) as f:
        return json.load(f)["runs"]


@functools.lru_cache(maxsize=None)
def reference(name, clamp=True):
    """The CPU result of a run of tests/rf_cases.py, computed once per session and never modified."""
    return RC.reference(name, RC.ref_dtype(RC.spec(name)["net"]), clamp=clamp)


def device_net(net_name, out_scale=1.0, dtype="fp32"):
    cfg, w = RC.weights(net_name, out_scale)
    if net_name in ("tiny", "tiny_cc"):
        net = A.UNet1dBase.from_config(cfg, compute_dtype=dtype)
    elif net_name == "u2d":
        net = A.UNet2dBase(**cfg.to_kwargs())
    elif net_name == "adm":
        net = A.UNetModel.from_config(cfg)
    else:
        net = A.WaveNetNoise.from_config(cfg)
    net.load_state_dict(w, strict=True)
    return net.cuda()


def handle(net):
    return net.native(torch.device("cuda", torch.cuda.current_device()))


def device_run(name, use_graph, net=None, dtype="fp32"):
    """Run ``name`` of tests/rf_cases.py through the plugin classes on the device."""
    sp = RC.spec(name)
    net = net if net is not None else device_net(sp["net"], sp["out_scale"], dtype)
    n, cs, cl = sp["steps"], sp["cond_scale"], RC.labels(sp["net"])
    kw = {} if cl is None else {"classes": cl.cuda()}
    if sp["loop"] == "rf":
        smp, diff = A.ReflowEulerSampler(num_steps=n, cond_scale=cs, use_heun=sp["heun"], use_graph=use_graph), A.ReFlow()
    elif sp["loop"] == "dpm2m_reflow":
        smp, diff = A.DPM2MSampler(num_steps=n, cond_scale=cs, reflow=True, use_graph=use_graph), A.ReFlow()
    elif sp["loop"] == "edm_rfedm":
        smp, diff = A.EDMSampler(s_churn=0, num_steps=n, cond_scale=cs, use_heun=True, use_graph=use_graph), A.ReFlow(for_edm=True)
    else:
        smp = A.UniPCSampler(num_steps=n, order=2, cond_scale=cs, x0_pred=True, log_time_spacing=True, use_graph=use_graph)
        diff = A.ReFlow(for_edm=True)
    return smp(RC.noise_of(sp).cuda(), fn=diff.denoise_fn, net=net, sigmas=RC.sigmas_of(sp), **kw).cpu()


def run_bar(runs, name):
    rec = runs[name]
    sp = RC.spec(name)
    assert (rec["out_scale"], rec["noise_scale"], rec["steps"]) == (sp["out_scale"], sp["noise_scale"], sp["steps"]), "the fixture belongs to other inputs"
    return max(TOL, 4.0 * (rec["dist_fp32_fp64"] or 0.0))


# ---- the library takes the two kinds and no third -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_preconditioning_takes_kinds_4_and_5_and_refuses_6():
    hd = handle(device_net("tiny"))
    hd.set_preconditioning(_lib.PRECOND_RF)
    hd.set_preconditioning(_lib.PRECOND_RF_EDM)
    with pytest.raises(_lib.AdfError, match="_RF_EDM"):
        hd.set_preconditioning(6)
    hd.set_preconditioning(_lib.PRECOND_EDM)


# ---- coefficient rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rf", "rf_edm"])
def test_device_coefficient_rows_vs_reference_rows(gold, kind):
    """The per-run table (c_in, c_noise, c_skip, c_out) of a 30-evaluation run.  rf: (1, s, 0, 1) on LinearSchedule(1, 0, 31), which holds no
    arithmetic at all -- 1e-6 is only the form of the bar, the rows are expected exact.  rf_edm: (1 - t, t, 1 - t, -t) against the reference's own fp32
    values on RFEDMSchedule(0.98, 0.02, 30), within the fixture's per-entry bar max(1e-6, 4 |fp32 - fp64| / |fp64|)."""
    net = device_net("tiny", 0.2)
    noise = RC.noise_of(RC.spec("tiny_euler")).cuda() * 1e-2
    if kind == "rf":
        sig, want = T(gold["sched_linear_31"]), gold["rows_rf"].astype(np.float64)
        bar = np.full_like(want, 1e-6)
        A.ReflowEulerSampler(num_steps=30, use_heun=False, use_graph=False)(noise, fn=A.ReFlow().denoise_fn, net=net, sigmas=sig)
    else:
        sig, want, bar = T(gold["sched_rfedm_30"]), gold["rows_rfedm"].astype(np.float64), gold["bar_rfedm"]
        assert rel(A.RFEDMSchedule(0.98, 0.02, 30)(), sig) < 1e-6     # (the exact comparison is the CPU suite's)
        A.EDMSampler(s_churn=0.0, num_steps=30, use_heun=False, use_graph=False)(noise, fn=A.ReFlow(for_edm=True).denoise_fn, net=net, sigmas=sig)
    got = handle(net).coef_rows(torch.device("cuda")).cpu().double().numpy()
    assert got.shape == want.shape == (30, 4)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    worst = np.unravel_index(np.argmax(err / bar), err.shape)
    print(kind, "rows exact:", bool(np.array_equal(got, want)), "max rel err", err.max(), "worst entry", worst, err[worst], "bar", bar[worst])
    assert np.all(err <= bar), (kind, worst, err[worst], bar[worst])


# ---- single denoise calls ----------------------------------------------------------------------------------------------------------------------
DEN_SIGMA = {"raw": (0.6, [0.3, 0.8, 0.55]), "edm": (0.9, [0.5, 3.0, 1.2])}
DEN_OUT_SCALE = {"wn": 4.0}          # the random-weight WaveNet's velocity stays below 0.4 at scale 1: it could not show that nothing clips


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["raw", "edm"])
@pytest.mark.parametrize("net_name,cond_scale", [("tiny", 1.0), ("tiny_cc", 2.0), ("u2d", 1.0), ("adm", 1.0), ("wn", 1.0)])
def test_one_denoise_call_vs_cpu_restatement(net_name, cond_scale, mode):
    """ReFlow(for_edm = mode == "edm").denoise_fn with a scalar sigma and with distinct [B] sigmas at the shapes of tests/rf_cases.py (the WaveNet at an
    odd T), output layer at scale 1 (WaveNet: 4).  Neither mode clips: the reference has entries beyond +-1 and they come back as they are."""
    scale = DEN_OUT_SCALE.get(net_name, 1.0)
    cfg, w = RC.weights(net_name, scale)
    shape, cl = RC.NETS[net_name][3], RC.labels(net_name)
    dt = RC.ref_dtype(net_name)
    net_o = RC.oracle_net(net_name, cfg, w, dt)
    net = device_net(net_name, scale)
    s0, sb = DEN_SIGMA[mode]
    sb = torch.tensor(sb[:shape[0]])
    g = torch.Generator().manual_seed(77)
    x = torch.randn(*shape, generator=g) * ((1.0 + sb.view(-1, *([1] * (len(shape) - 1))) ** 2).sqrt() if mode == "edm" else 1.0) * 1.2
    kw = {} if cl is None else {"classes": cl.cuda()}
    diff = A.ReFlow(for_edm=mode == "edm")
    beyond = 0.0
    with torch.no_grad():
        for name, kw_o, kw_d in (("scalar", dict(sigma=s0), dict(sigma=s0)), ("batch", dict(sigmas=sb), dict(sigmas=sb.cuda()))):
            ref = RF.denoise(mode == "edm", net_o, x.to(dt), cond_scale=cond_scale, **kw_o)
            d = diff.denoise_fn(x.cuda(), net=net, inference=True, cond_scale=cond_scale, **kw_d, **kw).cpu()
            e = rel(d, ref)
            print(net_name, mode, name, "rel err", e, "max |ref|", float(ref.abs().max()))
            assert d.shape == x.shape and bool(torch.isfinite(d).all())
            assert float(ref.abs().max()) > 0.05 and e <= TOL, (net_name, mode, name, e)
            over = ref.abs() > 1.0
            if bool(over.any()):
                beyond = max(beyond, float(d[over].abs().max()))
                assert float((d[over].double() - ref[over].double()).abs().max()) <= TOL * float(ref.abs().max())
    assert beyond > 1.0, "no case of this net shows that the estimate is unclipped"


# ---- ReflowEulerSampler runs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_euler", "tiny_heun", "tiny_cc_euler", "tiny_cc_heun", "u2d_euler", "u2d_heun", "adm_heun", "wn_heun"])
def test_reflow_euler_sampler_eager_and_graph_vs_cpu_restatement(runs, name):
    ref = reference(name)
    share, top = float((ref.abs() >= 1).double().mean()), float(ref.abs().max())
    bar = run_bar(runs, name)
    assert share <= 0.01 and top > 0.05, (name, share, top)
    sp = RC.spec(name)
    net = device_net(sp["net"], sp["out_scale"])
    for use_graph in (False, True):
        y = device_run(name, use_graph, net)
        e = rel(y, ref)
        print(name, "graph" if use_graph else "eager", "rel err", e, "bar", bar, "share |y| >= 1:", share, "max |y|", top)
        assert y.shape == ref.shape and float(y.abs().max()) <= 1.0
        assert e <= bar, (name, use_graph, e, bar)
    if name == "wn_heun":
        assert ref.numel() % 4 == 3                                   # the update kernels' scalar tail ran


@pytest.mark.gpu
def test_reflow_euler_sampler_agrees_with_the_reference_sampler_run(gold):
    """The fixture's run of the REFERENCE's ReflowEulerSampler + ReFlow around its own UNet2dBase (6 Heun steps, guidance 2), on the device."""
    net = device_net("u2d", 0.3)
    want = T(gold["run_heun_cfg_final"])
    y = A.ReflowEulerSampler(num_steps=6, cond_scale=2.0, use_heun=True, use_graph=True)(
        T(gold["run_noise"]).cuda(), fn=A.ReFlow().denoise_fn, net=net, sigmas=T(gold["sched_linear_7"]), classes=T(gold["run_classes"]).cuda()).cpu()
    print("reference run heun_cfg rel err", rel(y, want))
    assert rel(y, want) <= TOL


# ---- pairings the feature newly enables --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_dpm2m_reflow", "u2d_edm_rfedm", "tiny_unipc_rfedm"])
def test_existing_samplers_over_reflow_vs_cpu_restatement(runs, name):
    """DPM2MSampler(reflow=True) over the raw velocity of ReFlow(); EDMSampler(s_churn=0) and UniPCSampler over ReFlow(for_edm=True) on
    RFEDMSchedule(0.98, 0.02, N)."""
    ref = reference(name)
    bar = run_bar(runs, name)
    assert float((ref.abs() >= 1).double().mean()) <= 0.01 and float(ref.abs().max()) > 0.05
    sp = RC.spec(name)
    net = device_net(sp["net"], sp["out_scale"])
    for use_graph in (False, True):
        e = rel(device_run(name, use_graph, net), ref)
        print(name, "graph" if use_graph else "eager", "rel err", e, "bar", bar)
        assert e <= bar, (name, use_graph, e, bar)


# ---- clamp -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_final_clamp_on_a_run_that_leaves_the_unit_range(runs):
    name = "tiny_clamp"
    raw = reference(name, clamp=False)
    bar = run_bar(runs, name)
    inside = raw.abs() < 1.0
    assert 0.25 <= float((~inside).double().mean()) <= 0.75 and float(raw.abs().max()) > 2.0
    y = device_run(name, True)
    assert float(y.abs().max()) <= 1.0 and bool(torch.isfinite(y).all())
    e_in = float((y[inside].double() - raw[inside]).abs().max())              # the clamped reference has max |y| = 1: absolute = relative
    e_all = float((y.double() - raw.clamp(-1.0, 1.0)).abs().max())
    print("clamp run: inside", e_in, "all", e_all, "bar", bar, "share outside", float((~inside).double().mean()))
    assert e_in <= bar and e_all <= bar


# ---- graph key ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_graphs_are_keyed_by_the_new_kinds():
    """One handle, one shape: EluDiffusion + EDMSampler, then ReFlow(for_edm=True) + the SAME sampler on the SAME sigma list (only the preconditioning
    kind tells the two graphs apart), then ReFlow() + ReflowEulerSampler, then the first pair again: bit for bit the first result, from the first graph.
    On the WaveNet handle, whose passes are bit-reproducible.  The three U-Nets accumulate their GroupNorm statistics with atomics, so two identical
    runs in a row already differ in their last bits there (measured 5e-7 on the 1-D and Imagen nets, 2e-5 on the ADM net, eager or replayed, with
    nothing in between): a bitwise comparison on them would say nothing about the key."""
    net = device_net("wn", 2.0)
    hd = handle(net)
    noise = RC.noise_of(RC.spec("wn_heun")).cuda()
    sig = A.KarrasSchedule(0.002, 80.0, 7.0, 8)()
    edm = A.EDMSampler(s_churn=0, num_steps=8, use_graph=True)
    caps = hd.counters()["graph_captures"]
    first = edm(noise, fn=A.EluDiffusion(sigma_data=0.2).denoise_fn, net=net, sigmas=sig)
    wrapped = edm(noise, fn=A.ReFlow(for_edm=True).denoise_fn, net=net, sigmas=sig)
    flow = A.ReflowEulerSampler(num_steps=7, use_graph=True)(noise, fn=A.ReFlow().denoise_fn, net=net, sigmas=sig)
    again = edm(noise, fn=A.EluDiffusion(sigma_data=0.2).denoise_fn, net=net, sigmas=sig)
    assert torch.equal(first, again)
    assert hd.counters()["graph_captures"] - caps == 3
    print("keying: wrapped vs first", rel(wrapped, first), "flow vs first", rel(flow, first), "max |first|", float(first.abs().max()))
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0.01
    assert rel(wrapped, first) > 1e-2 and rel(flow, first) > 1e-2


# ---- bf16 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bf16_storage_through_the_new_loop_stays_near_the_fp32_mode():
    """A storage-precision figure, as in tests/test_gpu_parity.py: the 1-D tiny net in bf16 through 8 Heun steps against the fp32-mode run."""
    y32, y16 = device_run("tiny_heun", True), device_run("tiny_heun", True, dtype="bf16")
    print("bf16 vs fp32 mode", rel(y16, y32))
    assert bool(torch.isfinite(y16).all()) and float(y16.abs().max()) <= 1.0
    assert rel(y16, y32) < BF16_TOL
