"""GPU: the HIP UNet2dBase (exact fp32) -- the network of the shipped sc09 experiment files -- against the reference's own fixtures
(tests/golden/unet2d_golden.npz, 'sc09': the shipped structure at full width) and against oracle/unet2d.py: the full-size unconditional net,
the two shipped samplers on the device loop (eager and graph-replayed), classifier-free guidance, and graph keying by image shape."""
import os

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from oracle import edm as E, samplers as S, unet2d as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
FP32_TIGHT = 5e-5


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "unet2d_golden.npz"))


def make(cfg, seed=5):
    w = U.generate_weights(cfg, seed)
    net = A.UNet2dBase(**cfg.to_kwargs())
    net.load_state_dict(w, strict=True)
    return net.cuda(), w


@pytest.mark.gpu
def test_sc09_forward_labels_dropped_and_block_outputs_vs_reference_golden(gold):
    cfg, _ = U.fixture_variants()["sc09"]
    net, _ = make(cfg)
    x, t, cl = T(gold["u2d_sc09_x"]), T(gold["u2d_sc09_t"]), T(gold["u2d_sc09_classes"])
    with torch.no_grad():
        y = net(x.cuda(), t.cuda(), classes=cl.cuda()).cpu()
        assert y.shape == x.shape
        e = rel(y, T(gold["u2d_sc09_y"]))
        assert e < FP32_TIGHT, e
        hd = net.native(torch.device("cuda", torch.cuda.current_device()))
        taps = [k[len("u2d_sc09_tap_"):] for k in gold.files if k.startswith("u2d_sc09_tap_")]
        assert len(taps) == 12
        for k in taps:
            tap = hd.tap(k, x.shape[0], torch.device("cuda")).cpu()
            et = rel(tap.reshape(x.shape[0], -1)[:, ::64], T(gold[f"u2d_sc09_tap_{k}"]))
            assert et < FP32_TIGHT, (k, et)
        y0 = net(x.cuda(), t.cuda(), classes=cl.cuda(), cond_drop_prob=1.0).cpu()
        e0 = rel(y0, T(gold["u2d_sc09_y_null"]))
        assert e0 < FP32_TIGHT, e0
        with pytest.raises(AssertionError):
            net(x.cuda(), t.cuda())


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_shipped_unconditional_net_at_full_size_vs_oracle():
    """config_sc09(0) at [2, 2, 256, 128]: 512- and 128-token attention at head dim 128, the 64-pixel tiles of every level."""
    cfg = U.config_sc09(0)
    net, w = make(cfg, seed=7)
    g = torch.Generator().manual_seed(3)
    x, t = torch.randn(2, 2, 256, 128, generator=g) * 0.5, torch.tensor([0.7, -1.3])
    with torch.no_grad():
        y = net(x.cuda(), t.cuda()).cpu()
        ref = U.unet2d_forward(w, cfg, x, t)
    e = rel(y, ref)
    assert e < FP32_TIGHT, e


@pytest.fixture(scope="module")
def sampler_case():
    cfg = U.config_sc09(0)
    net, w = make(cfg, seed=11)
    g = torch.Generator().manual_seed(21)
    noise = torch.randn(2, 2, 64, 32, generator=g)
    sig = A.KarrasSchedule(0.002, 80.0, 7.0, 50)()
    fn_o = lambda xx, sigma=None, sigmas=None: E.denoise(lambda xi, ti, **kw: U.unet2d_forward(w, cfg, xi, ti), xx, 0.2, sigma=sigma, sigmas=sigmas)
    return net, noise, sig, fn_o


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["dpm3", "unipc2"])
def test_shipped_samplers_on_the_device_loop_vs_oracle(sampler_case, kind):
    """The two shipped eval files: DPMSampler(order 3, multistep, x0 prediction, sigma spacing) and UniPCSampler(order 2, noise prediction),
    50 Karras steps on EluDiffusion(sigma_data 0.2), eager and graph-replayed."""
    net, noise, sig, fn_o = sampler_case
    diff = A.EluDiffusion(sigma_data=0.2)
    with torch.no_grad():
        if kind == "dpm3":
            ref = S.dpm_multistep_sampler(noise, fn_o, sig, 50, order=3, log_time_spacing=False, x0_pred=True)
        else:
            ref = S.unipc_sampler(noise, fn_o, sig, 50, order=2, log_time_spacing=True, x0_pred=False)
    for use_graph in (False, True):
        if kind == "dpm3":
            smp = A.DPMSampler(cond_scale=1.0, order=3, num_steps=50, multisteps=True, x0_pred=True, log_time_spacing=False, use_graph=use_graph)
        else:
            smp = A.UniPCSampler(num_steps=50, order=2, x0_pred=False, use_graph=use_graph)
        y = smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig).cpu()
        e = rel(y, ref)
        assert e < 1e-3, (kind, use_graph, e)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_class_conditional_guidance_denoise_and_sampler_vs_oracle():
    """num_classes=10 with cond_scale 3: one guided denoise_fn call (per-sample sigmas) and a short guided DPM run, eager and graph-replayed."""
    cfg = U.config_sc09(10)
    net, w = make(cfg, seed=13)
    g = torch.Generator().manual_seed(14)
    x, cl = torch.randn(2, 2, 64, 32, generator=g), torch.tensor([9, 2])
    diff = A.EluDiffusion(sigma_data=0.2)
    net_o = lambda xi, ti, cond_drop_prob=0.0: U.unet2d_forward(w, cfg, xi, ti, classes=cl, cond_drop_prob=cond_drop_prob)
    fn_o = lambda xx, sigma=None, sigmas=None: E.denoise(net_o, xx, 0.2, sigma=sigma, sigmas=sigmas, cond_scale=3.0)
    with torch.no_grad():
        sg = torch.tensor([0.5, 20.0])
        d = diff.denoise_fn(x.cuda(), net=net, inference=True, cond_scale=3.0, sigmas=sg.cuda(), classes=cl.cuda()).cpu()
        assert rel(d, fn_o(x, sigmas=sg)) < 1e-4
        sig = A.KarrasSchedule(0.002, 80.0, 7.0, 6)()
        ref = S.dpm_multistep_sampler(x, fn_o, sig, 6, order=3, log_time_spacing=False, x0_pred=True)
        for use_graph in (False, True):
            smp = A.DPMSampler(cond_scale=3.0, order=3, num_steps=6, multisteps=True, x0_pred=True, log_time_spacing=False, use_graph=use_graph)
            y = smp(x.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig, classes=cl.cuda()).cpu()
            assert rel(y, ref) < 1e-4, (use_graph, rel(y, ref))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_two_image_shapes_with_equal_area_do_not_share_a_captured_graph():
    """[1, 2, 64, 32] and [1, 2, 32, 64] have the same H * W: a graph captured for one must not be replayed for the other."""
    cfg = U.config_sc09(0)
    net, w = make(cfg, seed=17)
    diff = A.EluDiffusion(sigma_data=0.2)
    sig = A.KarrasSchedule(0.002, 80.0, 7.0, 4)()
    g = torch.Generator().manual_seed(8)
    fn_o = lambda xx, sigma=None, sigmas=None: E.denoise(lambda xi, ti, **kw: U.unet2d_forward(w, cfg, xi, ti), xx, 0.2, sigma=sigma, sigmas=sigmas)
    smp = A.DPMSampler(cond_scale=1.0, order=3, num_steps=4, multisteps=True, x0_pred=True, log_time_spacing=False, use_graph=True)
    for shape in ((1, 2, 64, 32), (1, 2, 32, 64), (1, 2, 64, 32)):
        noise = torch.randn(*shape, generator=g)
        with torch.no_grad():
            ref = S.dpm_multistep_sampler(noise, fn_o, sig, 4, order=3, log_time_spacing=False, x0_pred=True)
        y = smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig).cpu()
        assert rel(y, ref) < FP32_TIGHT, (shape, rel(y, ref))
        with torch.no_grad():
            y1 = net(noise.cuda(), torch.tensor([0.1]).cuda()).cpu()
            assert rel(y1, U.unet2d_forward(w, cfg, noise, torch.tensor([0.1]))) < FP32_TIGHT
