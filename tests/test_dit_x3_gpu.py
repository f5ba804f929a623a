"""GPU: the split-bf16 (f32x3) mode of ``audiodiffuser_amd.DiT`` -- forward and every debug tap against the float64 restatement on the eleven cases
of tests/dit_x3_ref.py, each new kernel on its own through the route switches ADF_DIT_X3_LINEAR / ADF_DIT_X3_ATT (read when the handle is created),
the in-place gated epilogue, plan reuse, the guided denoiser and two sampler loops (eager and graph-replayed).

Bars: F32X3_TOL = 2e-4 of max |reference| per tensor (the project's split-bf16 bar, tests/test_gpu_parity.py) for the forward, the taps and one
denoiser call; RUN_TOL = 1e-3 for a sampler run (tests/test_dit_gpu.py).  The CPU emulation of the mode sits at 6.5e-6 .. 1.4e-5
(tests/test_dit_x3_host.py).  With ADF_DIT_X3_REPORT=<path> the worst measured value per test is written there as JSON (the committed copy:
tests/golden/dit_x3_report.json).
"""
import functools
import json
import os

import pytest
import torch

import audiodiffuser_amd as A
from oracle import edm as E, samplers as S
import dit_ref as DR
import dit_x3_ref as X3
from test_gpu_parity import F32X3_TOL

RUN_TOL = 1e-3
SIGMA_DATA = 0.2
MEASURED = {}
rel = X3.rel


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("ADF_DIT_X3_REPORT")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump({"bar_forward": F32X3_TOL, "bar_denoise": F32X3_TOL, "bar_run": RUN_TOL, "measured": MEASURED}, f, indent=1, sort_keys=True)


def make_net(case, dtype):
    net = A.DiT(cond_drop_prob=0.0, compute_dtype=dtype, **X3.ctor_kwargs(case))
    net.load_state_dict(X3.weights(case), strict=True)
    return net.cuda()


@functools.lru_cache(maxsize=None)
def device_net(case, dtype="f32x3"):
    """The handle is created at the first forward: under the default routes for every net of this cache."""
    return make_net(case, dtype)


@functools.lru_cache(maxsize=None)
def float64_ref(case):
    """(out, taps) in float64, computed once per case and only read afterwards."""
    x, t, classes = X3.inputs(case)
    taps = {}
    with torch.no_grad():
        out = DR.forward(X3.weights(case), X3.config(case), x, t, classes, taps=taps)
    return out, taps


def handle(net):
    return net.native(torch.device("cuda", torch.cuda.current_device()))


def device_taps(net, B):
    hd, dev = handle(net), torch.device("cuda")
    out = {}
    for name in hd.tap_names():
        t = hd.tap(name, B, dev).cpu()
        out[name] = t[:, :, 0] if name == "c" else t.transpose(1, 2)
    return out


def run(net, case):
    x, t, classes = X3.inputs(case)
    with torch.no_grad():
        return net(x.cuda(), t.cuda(), classes=None if classes is None else classes.cuda())


def forward_worst(net, case, names=None):
    """Worst distance from float64 over the output and the taps ``names`` (default: all of them) of one forward."""
    ref, ref_taps = float64_ref(case)
    y = run(net, case)
    assert y.shape == ref.shape and y.dtype == torch.float32
    got = device_taps(net, ref.shape[0])
    names = X3.tap_names(X3.config(case).depth) if names is None else names
    assert sorted(got) == sorted(names)
    worst = {"out": rel(y, ref)}
    for n in names:
        assert tuple(got[n].shape) == tuple(ref_taps[n].shape), n
        worst[n] = rel(got[n], ref_taps[n])
    return y, worst


# ---- forward and taps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(X3.CASES))
def test_forward_and_every_tap_vs_float64(case):
    _, worst = forward_worst(device_net(case), case)
    print(case, worst)
    MEASURED[f"forward_fp64/{case}"] = max(worst.values())
    assert max(worst.values()) < F32X3_TOL, worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tiny", "odd", "x3_edge"])
def test_f32x3_differs_from_the_fp32_handle_and_stays_within_the_bar_of_it(case):
    y3, y32 = run(device_net(case), case), run(device_net(case, "fp32"), case)
    d = rel(y3, y32.cpu())
    MEASURED[f"vs_fp32/{case}"] = d
    assert not torch.equal(y3, y32), "the f32x3 handle returned the fp32 handle's bits: nothing was split"
    assert d < F32X3_TOL, d


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tiny", "hd32"])
def test_both_route_switches_off_is_the_fp32_handle_bit_for_bit(monkeypatch, case):
    monkeypatch.setenv("ADF_DIT_X3_LINEAR", "0")
    monkeypatch.setenv("ADF_DIT_X3_ATT", "0")
    assert torch.equal(run(make_net(case, "f32x3"), case), run(device_net(case, "fp32"), case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tiny", "odd", "x3_edge", "x3_long32", "x3_long64"])
def test_attention_kernel_alone(monkeypatch, case):
    """ADF_DIT_X3_LINEAR=0: only the attention is split -- its own error, with nothing else to hide behind."""
    monkeypatch.setenv("ADF_DIT_X3_LINEAR", "0")
    y, worst = forward_worst(make_net(case, "f32x3"), case)
    print(case, worst)
    MEASURED[f"attention_only/{case}"] = max(worst.values())
    assert not torch.equal(y, run(device_net(case, "fp32"), case))
    assert max(worst.values()) < F32X3_TOL, worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["odd", "wide", "x3_edge"])
def test_linear_kernel_alone(monkeypatch, case):
    """ADF_DIT_X3_ATT=0: only the four token linears of a block are split."""
    monkeypatch.setenv("ADF_DIT_X3_ATT", "0")
    y, worst = forward_worst(make_net(case, "f32x3"), case)
    print(case, worst)
    MEASURED[f"linear_only/{case}"] = max(worst.values())
    assert not torch.equal(y, run(device_net(case, "fp32"), case))
    assert max(worst.values()) < F32X3_TOL, worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tiny", "x3_edge"])
def test_in_place_gated_epilogue_without_block_taps(monkeypatch, case):
    """ADF_DIT_TAPS=0: the residual stream updated in place by the gated epilogue (res == y)."""
    monkeypatch.setenv("ADF_DIT_TAPS", "0")
    _, worst = forward_worst(make_net(case, "f32x3"), case, names=["x_embedder", "c", "final_layer"])
    MEASURED[f"in_place/{case}"] = max(worst.values())
    assert max(worst.values()) < F32X3_TOL, worst


@pytest.mark.gpu
def test_second_forward_on_the_same_handle_other_inputs_other_batch():
    cfg, net, w = X3.config("tiny"), device_net("tiny"), X3.weights("tiny")
    for B, seed in ((3, 11), (2, 12), (3, 13), (5, 14)):
        x, t, _ = X3.inputs("tiny", B=B, seed=seed)
        with torch.no_grad():
            d = rel(net(x.cuda(), t.cuda()), DR.forward(w, cfg, x, t))
        MEASURED[f"second_forward/B{B}_seed{seed}"] = d
        assert d < F32X3_TOL, (B, seed, d)


@pytest.mark.gpu
def test_reloaded_weights_are_split_again():
    """The fp32 buffers stay the load target; the hi / lo planes follow a reload."""
    net = make_net("tiny", "f32x3")
    run(net, "tiny")
    w2 = X3.weights("tiny", seed=4)
    net.load_state_dict({k: v.cuda() for k, v in w2.items()}, strict=True)
    net.invalidate_native()
    x, t, _ = X3.inputs("tiny")
    with torch.no_grad():
        d = rel(net(x.cuda(), t.cuda()), DR.forward(w2, X3.config("tiny"), x, t))
    MEASURED["reload/tiny"] = d
    assert d < F32X3_TOL, d


# ---- denoiser and samplers ---------------------------------------------------------------------------------------------------------------------
def edm_fn(case, classes=None, cond_scale=1.0):
    net = DR.net_fn(case, classes=classes)
    return lambda x, sigma=None, sigmas=None: E.denoise(net, x, SIGMA_DATA, sigma=sigma, sigmas=sigmas, cond_scale=cond_scale)


def noise_of(case, seed=21, scale=1.0):
    return X3.inputs(case, seed=seed)[0] * scale


@pytest.mark.gpu
def test_labels_guided_denoise_and_guided_dpm_run():
    net, diff = device_net("labels"), A.EluDiffusion(sigma_data=SIGMA_DATA)
    _, _, cl = X3.inputs("labels")
    fn = edm_fn("labels", classes=cl, cond_scale=3.0)
    x, sg = noise_of("labels", scale=0.5), torch.tensor([0.4, 2.5, 0.9])
    with torch.no_grad():
        d = rel(diff.denoise_fn(x.cuda(), net=net, inference=True, cond_scale=3.0, sigmas=sg.cuda(), classes=cl.cuda()), fn(x.double(), sigmas=sg))
    MEASURED["denoise/labels_guided"] = d
    assert d < F32X3_TOL, d
    sig, noise = A.KarrasSchedule(0.002, 80.0, 7.0, 4)(), noise_of("labels")
    with torch.no_grad():
        ref = S.dpm_multistep_sampler(noise.double(), fn, sig, 4, order=3, log_time_spacing=False, x0_pred=True)
    for use_graph in (False, True):
        smp = A.DPMSampler(cond_scale=3.0, order=3, num_steps=4, multisteps=True, x0_pred=True, log_time_spacing=False, use_graph=use_graph)
        d = rel(smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig, classes=cl.cuda()), ref)
        MEASURED[f"run/labels_guided_dpm3_{'graph' if use_graph else 'eager'}"] = d
        assert d < RUN_TOL, (use_graph, d)


@pytest.mark.gpu
def test_edm_heun_sampler_on_odd_eager_and_graph():
    net, diff, fn = device_net("odd"), A.EluDiffusion(sigma_data=SIGMA_DATA), edm_fn("odd")
    sig, noise = A.KarrasSchedule(0.002, 80.0, 7.0, 6)(), noise_of("odd")
    with torch.no_grad():
        ref = S.edm_sampler(noise.double(), fn, sig, 6, s_churn=0.0, s_noise=1.0, use_heun=True)
    for use_graph in (False, True):
        smp = A.EDMSampler(s_churn=0.0, s_noise=1.0, num_steps=6, use_heun=True, use_graph=use_graph)
        d = rel(smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig), ref)
        MEASURED[f"run/odd_edm_heun_{'graph' if use_graph else 'eager'}"] = d
        assert d < RUN_TOL, (use_graph, d)
