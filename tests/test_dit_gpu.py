"""GPU: ``audiodiffuser_amd.DiT`` on the device -- forward and every debug tap against the reference module's goldens and against the float64
restatement tests/dit_ref.py on all of its ``CASES``, the denoiser, four sampler loops (eager and graph-replayed), guidance, the device loss and
plan reuse.

Bars: FP32_TIGHT = 5e-5 of max |reference| per tensor (the project's exact-fp32 bar) for the forward and the taps; 1e-4 for one denoiser call and
1e-3 for a sampler run (tests/test_unet2d_gpu.py).  With ADF_DIT_REPORT=<path> the worst measured value per case is written there as JSON
(the committed copy: tests/golden/dit_report.json).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from oracle import edm as E, samplers as S
import dit_ref as DR
import loss_ref as LR
import precond_ref as P
import rf_ref as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TIGHT = 5e-5
DEN_TOL = 1e-4
RUN_TOL = 1e-3
SIGMA_DATA = 0.2
MEASURED = {}


def rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("ADF_DIT_REPORT")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump({"bar_forward": FP32_TIGHT, "bar_denoise": DEN_TOL, "bar_run": RUN_TOL, "measured": MEASURED}, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "dit_golden.npz"))


@functools.lru_cache(maxsize=None)
def device_net(case):
    net = A.DiT(cond_drop_prob=0.0, **DR.ctor_kwargs(case))
    net.load_state_dict(DR.weights(case), strict=True)
    return net.cuda()


def handle(net):
    return net.native(torch.device("cuda", torch.cuda.current_device()))


def device_taps(net, B):
    """Every tap of the last pass as the restatement lays it out: [B, T, D], "c" as [B, D]."""
    hd, dev = handle(net), torch.device("cuda")
    out = {}
    for name in hd.tap_names():
        t = hd.tap(name, B, dev).cpu()
        out[name] = t[:, :, 0] if name == "c" else t.transpose(1, 2)
    return out


def tap_names(depth):
    return ["x_embedder", "c", "final_layer"] + [f"blocks.{i}{s}" for i in range(depth) for s in ("", ".attn", ".mlp")]


# ---- forward and taps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(DR.CASES))
def test_forward_and_every_tap_vs_float64(case):
    cfg, net = DR.config(case), device_net(case)
    x, t, classes = DR.inputs(case)
    ref_taps = {}
    with torch.no_grad():
        ref = DR.forward(DR.weights(case), cfg, x, t, classes, taps=ref_taps)
        y = net(x.cuda(), t.cuda(), classes=None if classes is None else classes.cuda())
    assert y.shape == x.shape and y.dtype == torch.float32
    got = device_taps(net, x.shape[0])
    assert sorted(got) == sorted(tap_names(cfg.depth))
    worst = {"out": rel(y, ref)}
    for n in tap_names(cfg.depth):
        assert tuple(got[n].shape) == tuple(ref_taps[n].shape), n
        worst[n] = rel(got[n], ref_taps[n])
    print(case, worst)
    MEASURED[f"forward_fp64/{case}"] = max(worst.values())
    assert max(worst.values()) < FP32_TIGHT, worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", DR.GOLDEN_CASES)
def test_forward_and_taps_vs_reference_goldens(gold, case):
    cfg, net = DR.config(case), device_net(case)
    x, t = torch.from_numpy(gold[f"{case}_x"]), torch.from_numpy(gold[f"{case}_t"])
    classes = torch.from_numpy(gold[f"{case}_classes"]) if f"{case}_classes" in gold.files else None
    with torch.no_grad():
        y = net(x.cuda(), t.cuda(), classes=None if classes is None else classes.cuda())
    got = device_taps(net, x.shape[0])
    worst = {"out": rel(y, torch.from_numpy(gold[f"{case}_out"]))}
    for n in ["x_embedder", "c", "final_layer"] + [f"blocks.{i}" for i in range(cfg.depth)]:
        worst[n] = rel(got[n], torch.from_numpy(gold[f"{case}_{n}"]))
    if classes is not None:          # cond_drop_prob = 1: every sample takes the null embedding
        with torch.no_grad():
            worst["null"] = rel(net(x.cuda(), t.cuda(), classes=classes.cuda(), cond_drop_prob=1.0), torch.from_numpy(gold[f"{case}_null"]))
    print(case, worst)
    MEASURED[f"forward_golden/{case}"] = max(worst.values())
    assert max(worst.values()) < FP32_TIGHT, worst


@pytest.mark.gpu
def test_second_forward_on_the_same_handle_other_inputs_other_batch():
    """Plan reuse (the same (B, H, W) again with other inputs) and the gate indexing at another B on one handle."""
    cfg, net, w = DR.config("tiny"), device_net("tiny"), DR.weights("tiny")
    for B, seed in ((3, 11), (2, 12), (3, 13), (5, 14)):
        x, t, _ = DR.inputs("tiny", B=B, seed=seed)
        with torch.no_grad():
            d = rel(net(x.cuda(), t.cuda()), DR.forward(w, cfg, x, t))
        MEASURED[f"second_forward/B{B}_seed{seed}"] = d
        assert d < FP32_TIGHT, (B, seed, d)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tiny", "odd"])
def test_in_place_residual_stream_without_block_taps(monkeypatch, case):
    """ADF_DIT_TAPS=0 (read when the handle is created): the route a net takes on its own once the per-block taps pass 512 MiB -- the residual
    stream updated in place by the gated epilogue, no second store of the branches."""
    monkeypatch.setenv("ADF_DIT_TAPS", "0")
    cfg = DR.config(case)
    net = A.DiT(cond_drop_prob=0.0, **DR.ctor_kwargs(case))
    net.load_state_dict(DR.weights(case), strict=True)
    net = net.cuda()
    x, t, _ = DR.inputs(case)
    ref_taps = {}
    with torch.no_grad():
        ref = DR.forward(DR.weights(case), cfg, x, t, taps=ref_taps)
        y = net(x.cuda(), t.cuda())
    got = device_taps(net, x.shape[0])
    assert sorted(got) == ["c", "final_layer", "x_embedder"]
    worst = {"out": rel(y, ref), **{n: rel(got[n], ref_taps[n]) for n in got}}
    MEASURED[f"in_place/{case}"] = max(worst.values())
    assert max(worst.values()) < FP32_TIGHT, worst


# ---- denoiser and samplers ---------------------------------------------------------------------------------------------------------------------
def edm_fn(case, classes=None, cond_scale=1.0):
    net = DR.net_fn(case, classes=classes)
    return lambda x, sigma=None, sigmas=None: E.denoise(net, x, SIGMA_DATA, sigma=sigma, sigmas=sigmas, cond_scale=cond_scale)


def noise_of(case, seed=21, scale=1.0):
    x, _, _ = DR.inputs(case, seed=seed)
    return x * scale


@pytest.mark.gpu
def test_elu_denoise_fn_scalar_and_per_sample_sigmas():
    net, diff, fn = device_net("odd"), A.EluDiffusion(sigma_data=SIGMA_DATA), edm_fn("odd")
    x = noise_of("odd", scale=0.5)
    sg = torch.tensor([0.4, 2.5])
    with torch.no_grad():
        a = rel(diff.denoise_fn(x.cuda(), net=net, inference=True, sigma=0.7), fn(x.double(), sigma=0.7))
        b = rel(diff.denoise_fn(x.cuda(), net=net, inference=True, sigmas=sg.cuda()), fn(x.double(), sigmas=sg))
    MEASURED["denoise/odd_scalar"], MEASURED["denoise/odd_rows"] = a, b
    assert a < DEN_TOL and b < DEN_TOL, (a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["edm_heun", "dpm3"])
def test_edm_and_dpm_samplers_on_odd_eager_and_graph(kind):
    net, diff, fn = device_net("odd"), A.EluDiffusion(sigma_data=SIGMA_DATA), edm_fn("odd")
    sig = A.KarrasSchedule(0.002, 80.0, 7.0, 6)()
    noise = noise_of("odd")
    with torch.no_grad():
        if kind == "edm_heun":
            ref = S.edm_sampler(noise.double(), fn, sig, 6, s_churn=0.0, s_noise=1.0, use_heun=True)
        else:
            ref = S.dpm_multistep_sampler(noise.double(), fn, sig, 6, order=3, log_time_spacing=False, x0_pred=True)
    for use_graph in (False, True):
        if kind == "edm_heun":
            smp = A.EDMSampler(s_churn=0.0, s_noise=1.0, num_steps=6, use_heun=True, use_graph=use_graph)
        else:
            smp = A.DPMSampler(cond_scale=1.0, order=3, num_steps=6, multisteps=True, x0_pred=True, log_time_spacing=False, use_graph=use_graph)
        d = rel(smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig), ref)
        MEASURED[f"run/odd_{kind}_{'graph' if use_graph else 'eager'}"] = d
        assert d < RUN_TOL, (kind, use_graph, d)


@pytest.mark.gpu
def test_reflow_euler_sampler_on_tiny_eager_and_graph():
    """ReFlow(): the estimate IS the network output (FwdIO mode 0 written straight into the sampler state)."""
    net, fn = device_net("tiny"), RF.make_fn(False, DR.net_fn("tiny"))
    sig, noise = A.LinearSchedule(1.0, 0.0, 5)(), noise_of("tiny")
    with torch.no_grad():
        ref = RF.euler_sampler(noise.double(), fn, sig, 4, use_heun=True)
    for use_graph in (False, True):
        smp = A.ReflowEulerSampler(num_steps=4, use_heun=True, use_graph=use_graph)
        d = rel(smp(noise.cuda(), fn=A.ReFlow().denoise_fn, net=net, sigmas=sig), ref)
        MEASURED[f"run/tiny_reflow_{'graph' if use_graph else 'eager'}"] = d
        assert d < RUN_TOL, (use_graph, d)


@pytest.mark.gpu
def test_vdiffusion_for_edm_with_edm_sampler_on_tiny_is_the_unclipped_epilogue():
    """VDiffusion(for_edm=True) returns its estimate unclipped: one pass per evaluation through the mode 2 epilogue of the unpatchify kernel."""
    net, fn = device_net("tiny"), P.make_fn("v", DR.net_fn("tiny"))
    sig, noise = A.KarrasSchedule(0.002, 80.0, 7.0, 6)(), noise_of("tiny")
    with torch.no_grad():
        ref = S.edm_sampler(noise.double(), fn, sig, 6, s_churn=0.0, use_heun=True)
        one = fn((noise * 3.0).double(), sigma=1.5)
    diff = A.VDiffusion(for_edm=True)
    hd = handle(net)
    with torch.no_grad():
        before = hd.counters()["net_passes"]
        d1 = rel(diff.denoise_fn((noise * 3.0).cuda(), net=net, inference=True, sigma=1.5), one)
        assert hd.counters()["net_passes"] == before + 1, "the unclipped estimate took more than one network pass"
    assert float(one.abs().max()) > 1.0, "this call cannot show that nothing clips"
    assert d1 < DEN_TOL, d1
    for use_graph in (False, True):
        smp = A.EDMSampler(s_churn=0.0, num_steps=6, use_heun=True, use_graph=use_graph)
        d = rel(smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig), ref)
        MEASURED[f"run/tiny_v_edm_{'graph' if use_graph else 'eager'}"] = d
        assert d < RUN_TOL, (use_graph, d)


# ---- conditioning, loss ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_labels_guided_denoise_and_guided_dpm_run():
    net, diff = device_net("labels"), A.EluDiffusion(sigma_data=SIGMA_DATA)
    _, _, cl = DR.inputs("labels")
    fn = edm_fn("labels", classes=cl, cond_scale=3.0)
    x, sg = noise_of("labels", scale=0.5), torch.tensor([0.4, 2.5, 0.9])
    with torch.no_grad():
        d = rel(diff.denoise_fn(x.cuda(), net=net, inference=True, cond_scale=3.0, sigmas=sg.cuda(), classes=cl.cuda()), fn(x.double(), sigmas=sg))
    MEASURED["denoise/labels_guided"] = d
    assert d < DEN_TOL, d
    sig, noise = A.KarrasSchedule(0.002, 80.0, 7.0, 4)(), noise_of("labels")
    with torch.no_grad():
        ref = S.dpm_multistep_sampler(noise.double(), fn, sig, 4, order=3, log_time_spacing=False, x0_pred=True)
    for use_graph in (False, True):
        smp = A.DPMSampler(cond_scale=3.0, order=3, num_steps=4, multisteps=True, x0_pred=True, log_time_spacing=False, use_graph=use_graph)
        d = rel(smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig, classes=cl.cuda()), ref)
        MEASURED[f"run/labels_guided_dpm3_{'graph' if use_graph else 'eager'}"] = d
        assert d < RUN_TOL, (use_graph, d)


@pytest.mark.gpu
def test_classes_on_an_unconditional_net_and_a_wrong_shape_are_refused():
    net = device_net("tiny")
    x, t, _ = DR.inputs("tiny")
    with pytest.raises(ValueError, match="label_cond"):
        net(x.cuda(), t.cuda(), classes=torch.zeros(3, dtype=torch.int64).cuda())
    with pytest.raises(ValueError, match="input_size"):
        net(torch.zeros(3, 4, 8, 16).cuda(), t.cuda())


@pytest.mark.gpu
def test_validation_loss_is_one_device_call_on_a_dit_handle():
    net, diff, hd = device_net("tiny"), A.EluDiffusion(sigma_data=SIGMA_DATA), handle(device_net("tiny"))
    assert SIGMA_DATA == LR.SIGMA_DATA
    x = noise_of("tiny", seed=31, scale=0.3).clamp(-1.0, 1.0)
    sg = torch.tensor([0.5, 3.0, 1.2])
    calls, ctr = hd.loss_calls(), hd.counters()
    with torch.no_grad():
        torch.manual_seed(5)
        got = diff(x.cuda(), net, sg.cuda())
        torch.manual_seed(5)
        noise = torch.randn_like(x.cuda()).cpu()
    assert hd.loss_calls() == calls + 1 and hd.counters() == ctr
    with torch.no_grad():
        ref = LR.forward("edm", DR.net_fn("tiny"), x.double(), noise.double(), sg)
    d = float(((got.double().cpu() - ref).abs() / ref.abs()).max())
    MEASURED["loss/tiny_edm"] = d
    assert got.shape == (3,) and d < DEN_TOL, (got, ref, d)
