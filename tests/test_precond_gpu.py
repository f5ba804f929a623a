"""GPU: the VE / VP / v (for_edm) preconditioning on the device denoiser -- the coefficient table against the reference's own values
(tests/golden/precond_golden.npz), one ``denoise_fn`` call per kind, and the six shipped sc09 inference settings that need no new sampler
recurrence (rows 1-6 below) on the device loop, eager and graph-replayed, against oracle/samplers.py driven by tests/precond_ref.py.

row  shipped file (diffunet_complex_sc09_eval_*.yaml)   diffusion                  sampler (30 steps, cond_scale 1)                         schedule
 1   ve              VEDiffusion()              UniPCSampler(order 2, x0_pred False, log_time_spacing False)   VESchedule(100, 0.02)
 2   vp              VPDiffusion(0.1, 19.9, 1000)   same UniPC                                                 VPSchedule(19.9, 0.1, end 0.001)
 3   vobj            VDiffusion(for_edm True)   EDMSampler(s_churn 0, use_heun False)                          VSchedule()
 4   vobj_edm_unipc  VDiffusion(for_edm True)   same UniPC                                                     VSchedule()
 5   ve_dpm          VEDiffusion()              DPMSampler(order 3, single-step, x0_pred False)                VESchedule(100, 0.02)
 6   vobj_edm_dpm    VDiffusion(for_edm True)   DPMSampler(order 2, single-step, x0_pred True)                 VSchedule()
Rows 5 and 6 ship ``log_time_spacing False``, which is not finite in the reference's own arithmetic (tests/test_precond_host.py): parity is
claimed with ``log_time_spacing=True`` and the shipped flag only has to run.

A sampler that ends in clamp(-1, 1) hides every difference in a saturated entry, so each such row asserts on the CPU result that at most a quarter
of the final entries sit at |y| >= 1, and every row that max|y| > 0.05.  The inputs (unit noise x 0.003, row 4 with final_conv x 0.05) and the
shares they give with the full-width net are recorded in tests/golden/precond_report.json, with the fp32-vs-float64 distance of the CPU restatement
that sets each row's bar (rows 1, 2, 5 also carry final_conv x 0.05: at scale 1 the random-weight VE / VP denoisers are chaotic over 30 steps).

Measured on one MI355X (relative to max|ref|): row 1 4.3e-5, row 3 3.7e-6, row 4 1.1e-5, row 5 7.6e-5, row 6 2.0e-5; row 2 (VP) 1.1 to 1.5 -- its CPU restatement in
fp32 and float64 is 1.39 apart, so by the rule above its bar is 5.6 and the run only shows that it completes and stays finite."""
import json
import os

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd.weights import generate_noise, generate_weights, generate_wavenet_weights
from audiodiffuser_amd.adm_config import generate_weights as adm_weights
from oracle import samplers as S, unet1d as O1, unet2d as U, unet2d_oai as OA, wavenet as W
import precond_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
FP32_TIGHT = 5e-5            # tests/test_unet2d_gpu.py
RUN_TOL = 1e-3               # whole runs: tests/test_unet2d_gpu.py, BASELINE's north_star
SHIPPED_SCHEDULE = {"edm": "karras", "ve": "ve", "vp": "vp", "v": "v"}


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "precond_golden.npz"))


def diffusion_of(kind):
    return {"edm": lambda: A.EluDiffusion(sigma_data=PR.SIGMA_DATA), "ve": A.VEDiffusion, "vp": lambda: A.VPDiffusion(**PR.VP_ARGS),
            "v": lambda: A.VDiffusion(for_edm=True)}[kind]()


def schedule_of(kind, n):
    return {"edm": lambda: A.KarrasSchedule(0.002, 80.0, 7.0, n), "ve": lambda: A.VESchedule(sigma_max=100, sigma_min=0.02, num_steps=n),
            "vp": lambda: A.VPSchedule(beta_d=19.9, beta_min=0.1, end=0.001, num_steps=n), "v": lambda: A.VSchedule(num_steps=n)}[kind]()()


def make2d(cfg, seed, final_scale=1.0):
    w = U.generate_weights(cfg, seed)
    if final_scale != 1.0:
        w["final_conv.weight"] = w["final_conv.weight"] * final_scale
        w["final_conv.bias"] = w["final_conv.bias"] * final_scale
    net = A.UNet2dBase(**cfg.to_kwargs())
    net.load_state_dict(w, strict=True)
    return net.cuda(), w


def make1d(seed=0, out_scale=1.0):
    """out_scale < 1 for VE runs: c_out = sigma (up to 100) multiplies the random-weight net's Lipschitz constant and a whole run is ill-conditioned at scale 1
    (as for the 2-D net, tests/golden/precond_report.json); the reference zero-initialises this layer (unet1d.py:619)."""
    cfg = A.config_tiny()
    w = generate_weights(cfg, seed=seed)
    w["unet.to_out.to_out.weight"] = w["unet.to_out.to_out.weight"] * out_scale
    net = A.UNet1dBase.from_config(cfg)
    net.load_state_dict(w, strict=True)
    return net.cuda(), w, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["edm", "ve", "vp", "v"])
def test_device_coefficient_table_vs_reference_rows(gold, kind):
    """The per-run table (c_in, c_noise, c_skip, c_out) the device builds for a 30-evaluation run on the kind's shipped schedule, against the
    reference's get_scale_weights: 1e-6 relative, or where the reference's fp32 expression is itself ill-conditioned the fixture's per-entry bar
    max(1e-6, 4 |fp32 - fp64| / |fp64|) of the reference's own values."""
    net, _, _ = make1d()
    sname = SHIPPED_SCHEDULE[kind]
    sig = T(gold[f"sched_{sname}_30"])              # the reference's own schedule values: the rows of the fixture belong to exactly these sigmas
    assert rel(schedule_of(kind, 30), sig) < 1e-6   # (this host's pow may round an entry the other way: the exact comparison is the CPU suite's)
    smp = A.EDMSampler(s_churn=0.0, s_noise=1.0, num_steps=30, use_heun=False, use_graph=False)       # evaluates sigmas[0..29] in order
    smp(generate_noise(0, 2, 256).cuda() * 1e-3, fn=diffusion_of(kind).denoise_fn, net=net, sigmas=sig)
    got = net.native(torch.device("cuda", torch.cuda.current_device())).coef_rows(torch.device("cuda")).cpu().double().numpy()
    want, bar = gold[f"rows_{kind}_{sname}"].astype(np.float64), gold[f"bar_{kind}_{sname}"]
    assert got.shape == want.shape == (30, 4)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    worst = np.unravel_index(np.argmax(err / bar), err.shape)
    print(kind, "max rel err", err.max(), "worst entry", worst, err[worst], "bar", bar[worst], "entries above 1e-6:", int((err > 1e-6).sum()))
    assert np.all(err <= bar), (kind, worst, err[worst], bar[worst])


DENOISE_SIGMAS = {"edm": (0.7, [0.3, 2.0], None), "ve": (0.3, [0.1, 0.5], 100.0), "vp": (0.05, [0.03, 0.1], None), "v": (0.9, [0.5, 3.0], 100.0)}


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["edm", "ve", "vp", "v"])
def test_one_denoise_call_per_kind_vs_cpu_restatement(kind):
    """config_sc09(0) at [2, 2, 64, 32], scalar and per-sample sigmas at which at most half of the reference result is clipped (at sigma = 100
    a random-weight VE denoiser clips 99 %); VE and v also at sigma = 100.  The v result is not clipped: entries beyond +-1 come back as they are."""
    cfg = U.config_sc09(0)
    net, w = make2d(cfg, seed=11)
    fn_o = PR.make_fn(kind, lambda xi, ti, **kw: U.unet2d_forward(w, cfg, xi, ti))
    diff = diffusion_of(kind)
    s0, sb, big = DENOISE_SIGMAS[kind]
    sb = torch.tensor(sb)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 2, 64, 32, generator=g) * (1.0 + sb.view(2, 1, 1, 1) ** 2).sqrt() * (1.2 if kind == "v" else 0.4)
    with torch.no_grad():
        cases = [("scalar", dict(sigma=s0), dict(sigma=s0)), ("batch", dict(sigmas=sb), dict(sigmas=sb.cuda()))]
        if big is not None:
            cases.append(("large", dict(sigma=big), dict(sigma=big)))
        for name, kw_o, kw_d in cases:
            ref = fn_o(x * (big if name == "large" else 1.0), **kw_o)
            d = diff.denoise_fn(x.cuda() * (big if name == "large" else 1.0), net=net, inference=True, **kw_d).cpu()
            share = float((ref.abs() >= 1).float().mean())
            e = rel(d, ref)
            print(kind, name, "rel err", e, "share |ref| >= 1:", share, "max |ref|", float(ref.abs().max()))
            if name != "large" and kind != "v":
                assert share <= 0.5, (kind, name, share)
            assert float(ref.abs().max()) > 0.05
            if name == "large" and kind != "v":
                # 99.9 % of this result sits on the clamp and the rest is x - 100 F with |100 F| in the hundreds: the clamp is 1-Lipschitz, so the
                # error after it is bounded by the error before it, which is FP32_TIGHT of the magnitude BEFORE the clamp
                raw = PR.denoise(kind, lambda xi, ti, **kw: U.unet2d_forward(w, cfg, xi, ti), x * big, sigma=big, unclipped=True)
                assert share > 0.9 and float((d - ref).abs().max()) <= FP32_TIGHT * float(raw.abs().max()), (kind, name, e, float(raw.abs().max()))
                continue
            assert e <= FP32_TIGHT, (kind, name, e)
            if kind == "v":
                over = ref.abs() > 1.0
                if name != "large":
                    assert int(over.sum()) > 100, "the v case must have reference entries beyond +-1"
                    assert float((d[over] - ref[over]).abs().max()) <= FP32_TIGHT * float(ref.abs().max()) and float(d.abs().max()) > 1.0
            else:
                assert float(d.abs().max()) <= 1.0


ROWS = {
    1: ("ve", 0.05, lambda g: A.UniPCSampler(num_steps=30, order=2, cond_scale=1.0, x0_pred=False, log_time_spacing=False, use_graph=g),
        lambda n, fn, sig: S.unipc_sampler(n, fn, sig, 30, order=2, log_time_spacing=False, x0_pred=False)),
    2: ("vp", 0.05, lambda g: A.UniPCSampler(num_steps=30, order=2, cond_scale=1.0, x0_pred=False, log_time_spacing=False, use_graph=g),
        lambda n, fn, sig: S.unipc_sampler(n, fn, sig, 30, order=2, log_time_spacing=False, x0_pred=False)),
    3: ("v", 1.0, lambda g: A.EDMSampler(s_churn=0, num_steps=30, cond_scale=1.0, use_heun=False, use_graph=g),
        lambda n, fn, sig: S.edm_sampler(n, fn, sig, 30, s_churn=0.0, use_heun=False)),
    4: ("v", 0.05, lambda g: A.UniPCSampler(num_steps=30, order=2, cond_scale=1.0, x0_pred=False, log_time_spacing=False, use_graph=g),
        lambda n, fn, sig: S.unipc_sampler(n, fn, sig, 30, order=2, log_time_spacing=False, x0_pred=False)),
    5: ("ve", 0.05, lambda g: A.DPMSampler(cond_scale=1.0, order=3, num_steps=30, multisteps=False, x0_pred=False, log_time_spacing=True, use_graph=g),
        lambda n, fn, sig: S.dpm_singlestep_sampler(n, fn, sig, 30, order=3, log_time_spacing=True, x0_pred=False)),
    6: ("v", 1.0, lambda g: A.DPMSampler(cond_scale=1.0, order=2, num_steps=30, multisteps=False, x0_pred=True, log_time_spacing=True, use_graph=g),
        lambda n, fn, sig: S.dpm_singlestep_sampler(n, fn, sig, 30, order=2, log_time_spacing=True, x0_pred=True)),
}


def row_noise():
    return torch.randn(2, 2, 64, 32, generator=torch.Generator().manual_seed(21)) * 0.003


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("row", [1, 2, 3, 4, 5, 6])
def test_shipped_rows_on_the_device_loop_vs_oracle(row):
    """Rows 1-4 with the shipped arguments, rows 5-6 with log_time_spacing=True, 30 steps on config_sc09(0) at [2, 2, 64, 32], eager and
    graph-replayed."""
    kind, final_scale, make_sampler, oracle_run = ROWS[row]
    cfg = U.config_sc09(0)
    net, w = make2d(cfg, seed=11, final_scale=final_scale)
    noise, sig = row_noise(), schedule_of(kind, 30)
    assert torch.equal(sig, PR.shipped_schedule(kind, 30))
    with torch.no_grad():
        ref = oracle_run(noise, PR.make_fn(kind, lambda xi, ti, **kw: U.unet2d_forward(w, cfg, xi, ti)), sig)
    share, top = float((ref.abs() >= 1).float().mean()), float(ref.abs().max())
    with open(os.path.join(ROOT, "tests", "golden", "precond_report.json")) as f:
        recorded = json.load(f)["rows"][str(row)]
    assert recorded["final_conv_scale"] == final_scale
    # the issue's rule for a row whose reference arithmetic is itself ill-conditioned: the CPU restatement in fp32 and in float64 on the same input
    # (distances measured once, recorded in precond_report.json), bar = max(1e-3, 4 x their distance).  Rows 1, 3, 4, 5, 6: 1e-3.  Row 2 (VP): the two CPU
    # runs end 1.39 apart (time inputs c_noise = 999 t(sigma) up to 999 enter the random-weight time MLP raw), so its bar is no parity claim; what holds
    # row 2 is the coefficient table (exact rows) and the per-call test.
    bar = max(RUN_TOL, 4.0 * recorded["dist_fp32_fp64"])
    print("row", row, "share |y| >= 1:", share, "max |y|", top, "recorded", recorded, "bar", bar)
    if row != 3:                                          # EDMSampler does not clamp
        assert share <= 0.25, (row, share)
    assert top > 0.05 and bool(torch.isfinite(ref).all())
    diff = diffusion_of(kind)
    for use_graph in (False, True):
        y = make_sampler(use_graph)(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig).cpu()
        e = rel(y, ref)
        print("row", row, "graph" if use_graph else "eager", "rel err", e)
        assert e <= bar, (row, use_graph, e, bar)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("row", [5, 6])
def test_rows_5_and_6_with_the_shipped_flag_run_to_the_end(row):
    """log_time_spacing=False as shipped: the reference's own arithmetic is not finite here (a sigma added to a lambda step), so there is nothing
    to equal.  The run must return without error and perform every evaluation (the suite's autouse check holds adf_get_counters to
    adf_sampler_nfe).  No kernel on this path loops or indexes on data values -- the grids and loop bounds come from shapes, the radix select
    of the dynamic threshold is off at threshold 0, VDiffusion never thresholds -- so a NaN only propagates."""
    kind, _, _, _ = ROWS[row]
    cfg = U.config_sc09(0)
    net, _ = make2d(cfg, seed=11)
    order, x0 = (3, False) if row == 5 else (2, True)
    smp = A.DPMSampler(cond_scale=1.0, order=order, num_steps=30, multisteps=False, x0_pred=x0, log_time_spacing=False, use_graph=False)
    hd = net.native(torch.device("cuda", torch.cuda.current_device()))
    before = hd.counters()
    y = smp(row_noise().cuda(), fn=diffusion_of(kind).denoise_fn, net=net, sigmas=schedule_of(kind, 30))
    torch.cuda.synchronize()
    after = hd.counters()
    assert y.shape == (2, 2, 64, 32)
    assert after["sampler_runs"] == before["sampler_runs"] + 1 and after["sampler_evals"] - before["sampler_evals"] == smp.nfe() == 29


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["ve", "v"])
def test_guidance_denoise_and_short_run_vs_oracle(kind):
    """config_sc09(10) with cond_scale 3: one guided denoise_fn call (per-sample sigmas) and a 6-step guided run, eager and graph-replayed, modelled on
    tests/test_unet2d_gpu.py::test_class_conditional_guidance_denoise_and_sampler_vs_oracle.  VE: the shipped UniPC with final_conv x 0.01 (guidance triples the
    denoiser's Lipschitz constant on top of c_out = sigma: at scale 1 the result is 71 % saturated and ill-conditioned; at 0.01 the CPU restatement in fp32 and
    float64 ends 2.6e-5 apart, 0.2 % saturated).  v: the shipped EDMSampler(use_heun False), which does not clamp (fp32 vs float64: 5.6e-6, max |y| 5.6)."""
    cfg = U.config_sc09(10)
    net, w = make2d(cfg, seed=13, final_scale=0.01 if kind == "ve" else 1.0)
    g = torch.Generator().manual_seed(14)
    x, cl = torch.randn(2, 2, 64, 32, generator=g) * 0.4, torch.tensor([9, 2])
    diff = diffusion_of(kind)
    net_o = lambda xi, ti, cond_drop_prob=0.0: U.unet2d_forward(w, cfg, xi, ti, classes=cl, cond_drop_prob=cond_drop_prob)
    fn_o = PR.make_fn(kind, net_o, cond_scale=3.0)
    with torch.no_grad():
        sg = torch.tensor([0.1, 0.5])
        ref = fn_o(x, sigmas=sg)
        d = diff.denoise_fn(x.cuda(), net=net, inference=True, cond_scale=3.0, sigmas=sg.cuda(), classes=cl.cuda()).cpu()
        e = rel(d, ref)
        print(kind, "guided denoise rel err", e, "share clipped", float((ref.abs() >= 1).float().mean()))
        assert e <= 1e-4, e
        assert float((ref.abs() >= 1).float().mean()) <= 0.5
        sig = schedule_of(kind, 6)
        noise = x * 0.0075
        if kind == "ve":
            ref = S.unipc_sampler(noise, fn_o, sig, 6, order=2, log_time_spacing=False, x0_pred=False)
            assert float((ref.abs() >= 1).float().mean()) <= 0.25
        else:
            ref = S.edm_sampler(noise, fn_o, sig, 6, s_churn=0.0, use_heun=False)
        print(kind, "guided run: share |y| >= 1", float((ref.abs() >= 1).float().mean()), "max", float(ref.abs().max()))
        assert float(ref.abs().max()) > 0.05
        for use_graph in (False, True):
            if kind == "ve":
                smp = A.UniPCSampler(num_steps=6, order=2, cond_scale=3.0, x0_pred=False, log_time_spacing=False, use_graph=use_graph)
            else:
                smp = A.EDMSampler(s_churn=0, num_steps=6, cond_scale=3.0, use_heun=False, use_graph=use_graph)
            y = smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig, classes=cl.cuda()).cpu()
            print(kind, "guided run", "graph" if use_graph else "eager", "rel err", rel(y, ref))
            assert rel(y, ref) <= 1e-4, (use_graph, rel(y, ref))


@pytest.mark.gpu
def test_captured_graphs_are_keyed_by_the_preconditioning():
    """One handle, one shape, one sigma list: EluDiffusion -> VEDiffusion -> EluDiffusion with use_graph=True.  Each run matches its own oracle
    and the handle captures twice (the third run replays the first graph)."""
    net, w, cfg = make1d(seed=2, out_scale=0.02)
    hd = net.native(torch.device("cuda", torch.cuda.current_device()))
    noise = generate_noise(3, 2, 256) * 0.05
    sig = A.KarrasSchedule(0.002, 80.0, 7.0, 8)()
    net_o = lambda xi, ti, **kw: O1.unet1d_forward(w, cfg, xi, ti)
    smp = A.UniPCSampler(num_steps=8, order=2, x0_pred=True, log_time_spacing=True, use_graph=True)
    caps = hd.counters()["graph_captures"]
    for kind in ("edm", "ve", "edm"):
        with torch.no_grad():
            ref = S.unipc_sampler(noise, PR.make_fn(kind, net_o), sig, 8, order=2, log_time_spacing=True, x0_pred=True)
        y = smp(noise.cuda(), fn=diffusion_of(kind).denoise_fn, net=net, sigmas=sig).cpu()
        print("keying", kind, "rel err", rel(y, ref))
        assert rel(y, ref) <= 1e-4, (kind, rel(y, ref))
    assert rel(S.unipc_sampler(noise, PR.make_fn("ve", net_o), sig, 8, order=2), S.unipc_sampler(noise, PR.make_fn("edm", net_o), sig, 8, order=2)) > 1e-2
    assert hd.counters()["graph_captures"] - caps == 2


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ve", "v"])
def test_one_dimensional_unet_8_step_unipc_vs_cpu_restatement(kind):
    """Not UNet2dBase only: the 1-D U-Net takes the unclipped v estimate through its raw pass + the combine kernel without the clamp.  (The v run's
    final state is saturated by UniPC's closing clamp with these weights -- measured max |y| 1.0, device equal to the CPU result -- so for v the weight of this
    test lies on the denoise_fn call, whose entries beyond +-1 come back unclipped.)"""
    net, w, cfg = make1d(seed=4, out_scale=0.02 if kind == "ve" else 1.0)
    noise = generate_noise(5, 2, 256) * 0.003
    sig = schedule_of(kind, 8)
    fn_o = PR.make_fn(kind, lambda xi, ti, **kw: O1.unet1d_forward(w, cfg, xi, ti))
    diff = diffusion_of(kind)
    with torch.no_grad():
        ref = S.unipc_sampler(noise, fn_o, sig, 8, order=2, log_time_spacing=False, x0_pred=False)
        x = generate_noise(6, 2, 256)
        dref = fn_o(x, sigmas=torch.tensor([0.4, 2.5]))
        d = diff.denoise_fn(x.cuda(), net=net, inference=True, sigmas=torch.tensor([0.4, 2.5]).cuda()).cpu()
    assert rel(d, dref) <= 1e-4, rel(d, dref)
    if kind == "v":
        assert float(dref.abs().max()) > 1.0 and float(d.abs().max()) > 1.0
    assert float(ref.abs().max()) > 0.05
    for use_graph in (False, True):
        smp = A.UniPCSampler(num_steps=8, order=2, x0_pred=False, log_time_spacing=False, use_graph=use_graph)
        y = smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig).cpu()
        print("1-D", kind, "graph" if use_graph else "eager", "rel err", rel(y, ref), "max |ref|", float(ref.abs().max()))
        assert rel(y, ref) <= 1e-4, (kind, use_graph, rel(y, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["wavenet", "adm"])
def test_unclipped_v_estimate_on_the_other_two_handle_types(which):
    """WaveNetNoise and the ADM UNetModel: one VDiffusion(for_edm=True) call with entries beyond +-1, and VEDiffusion clamped."""
    g = torch.Generator().manual_seed(9)
    if which == "wavenet":
        cfg = A.config_c5_small()
        w = generate_wavenet_weights(cfg, seed=5)
        net = A.WaveNetNoise.from_config(cfg)
        net_o = W.wavenet_net(w, cfg)
        x = torch.randn(3, 1, 500, generator=g) * 1.5
    else:
        cfg = A.config_c4_small()
        w = adm_weights(cfg, seed=3)
        net = A.UNetModel.from_config(cfg)
        net_o = lambda xi, ti, **kw: OA.unet2d_forward(w, cfg, xi, ti)
        x = torch.randn(3, 1, 32, 32, generator=g) * 1.5
    net.load_state_dict(w, strict=True)
    net = net.cuda()
    sv = torch.tensor([0.3, 0.9, 4.0])
    with torch.no_grad():
        for kind in ("v", "ve"):
            ref = PR.denoise(kind, net_o, x, sigmas=sv)
            d = diffusion_of(kind).denoise_fn(x.cuda(), net=net, inference=True, sigmas=sv.cuda()).cpu()
            assert rel(d, ref) <= FP32_TIGHT, (which, kind, rel(d, ref))
            assert (float(d.abs().max()) > 1.0) == (kind == "v") and (float(ref.abs().max()) > 1.0) == (kind == "v")
