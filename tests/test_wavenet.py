"""WaveNetNoise (BASELINE configs[4]): the plugin's host-side contract on CPU, and on the GPU the HIP
path through the C ABI against (a) the reference's own outputs (fixtures of oracle/gen_golden_next.py) in fp32 mode,
(b) the bf16-storage oracle, layer by layer with teacher forcing, in bf16 (MFMA) mode, (c) the oracle's EDM wrapper and
sampler loop around the adapter this build defines."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
from audiodiffuser_amd.weights import wavenet_param_specs, generate_wavenet_weights
from oracle import edm as E, samplers as S, wavenet as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy

FP32_TOL = 1e-3        # the north-star bar (relative to the reference)
FP32_TIGHT = 2e-5      # what exact-fp32 FMA chains in another summation order give (measured ~1e-6): regressions show here
BF16_LAYER_TOL = 1e-3  # one layer from the device's own input against the bf16-storage oracle (relative L2): summation order +
                       # the bf16 roundings it flips (a flipped rounding of a value v moves it by 2^-8 |v|; ~1 % of them flip)
BF16_NET_TOL = 3e-2    # free-running bf16 net against the fp32 reference: a storage-precision figure, not a parity claim


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "next_golden.npz"))


def make(cfg, dtype="fp32", seed=5):
    w = generate_wavenet_weights(cfg, seed=seed)
    net = A.WaveNetNoise.from_config(cfg, compute_dtype=dtype)
    net.load_state_dict(w, strict=True)
    return net, w


# ------------------------------------------------------------------------------------------------ CPU: host logic
def test_plugin_state_dict_contract_and_refusals():
    net = A.WaveNetNoise()                                      # the reference's defaults
    specs = wavenet_param_specs(A.config_c5())
    sd = net.state_dict()
    assert list(sd) == list(specs)
    assert all(tuple(sd[k].shape) == specs[k][0] for k in specs)
    assert sum(p.numel() for p in net.parameters()) == 24034379
    pre = "residual_layer.residual_blocks.7.dilated_conv.conv.module."
    assert sd[pre + "weight_g"].ndim == 0 and abs(float(torch.norm(sd[pre + "weight_v"])) - 1.0) < 1e-4   # WeightNorm._reset
    assert float(sd["output_projection.conv.weight"].abs().max()) == 0.0                                  # ZeroConv1d
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 64), torch.zeros(1))
    with pytest.raises(ValueError):
        A.WaveNetNoise(residual_channels=96, compute_dtype="bf16")            # the MFMA kernels: 64, 128 or 256 channels
    A.WaveNetNoise(residual_channels=64, residual_layers=4, dilation_cycle=2, compute_dtype="bf16")
    with pytest.raises(ValueError):
        A.WaveNetNoise(residual_channels=48)
    small = A.WaveNetNoise.from_config(A.config_c5_small())
    with pytest.raises(RuntimeError):                                                                      # strict load, as Lightning does
        small.load_state_dict({k: v for k, v in generate_wavenet_weights(A.config_c5_small()).items() if "weight_g" not in k})


def test_wavenet_config_struct_matches_header():
    assert C.sizeof(_lib.AdfWaveNetConfig) == 4 * 7
    c = _lib.make_wavenet_config(A.config_c5(), _lib.DTYPE_BF16)
    assert (c.residual_channels, c.residual_layers, c.dilation_cycle, c.dim_in, c.dim_mid, c.dim_out, c.dtype) == (256, 36, 12, 128, 512, 512, 1)


# ------------------------------------------------------------------------------------------------ GPU
def _taps(net, batch):
    hd = net.native(torch.device("cuda", torch.cuda.current_device()))
    return {n: hd.tap(n, batch, torch.device("cuda")).cpu() for n in hd.tap_names()}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["small", "c5"])
def test_fp32_forward_and_layer_taps_vs_reference_golden(gold, tag):
    """fp32 mode against the REFERENCE's outputs: the network output and the recorded layer inputs / skip sum.  small: 6 layers,
    32 channels, T = 300 (ragged against the 16-position tiles); c5: the default 36 x 256 net, T = 1024 < the largest dilation."""
    cfg = {"small": A.config_c5_small, "c5": A.config_c5}[tag]()
    stride = 4 if tag == "small" else 16
    net, _ = make(cfg)
    net = net.cuda()
    audio, step = T(gold[f"wn_{tag}_audio"]), T(gold[f"wn_{tag}_step"])
    y = net(audio.cuda(), step.cuda())                     # the reference's call form: audio [B, T]
    torch.cuda.synchronize()
    assert y.shape == (audio.shape[0], 1, audio.shape[1])
    e = rel(y.cpu(), T(gold[f"wn_{tag}_y"]))
    assert e < FP32_TIGHT < FP32_TOL, e
    taps = _taps(net, audio.shape[0])
    assert len([k for k in taps if k.startswith("y")]) == cfg.residual_layers and "skip" in taps
    names = [k[len(f"wn_{tag}_tap_"):] for k in gold.files if k.startswith(f"wn_{tag}_tap_")]
    checked = 0
    for k in names:
        if k in taps:                                      # g<n> / sp live in LDS only on the device
            et = rel(taps[k].reshape(taps[k].shape[0], -1)[:, ::stride], T(gold[f"wn_{tag}_tap_{k}"]))
            assert et < FP32_TIGHT, (k, et)
            checked += 1
    assert checked >= 4
    y2 = net(audio.unsqueeze(1).cuda(), step.cuda(), cond_drop_prob=0.0)      # the adapter's call form
    assert torch.equal(y2, y)


@pytest.mark.gpu
@pytest.mark.parametrize("tlen", [1000, 64, 4200])
def test_bf16_every_layer_vs_bf16_storage_oracle(tlen):
    """bf16 (MFMA) mode, default 36 x 256 net.  Teacher-forced: the oracle computes layer n from the DEVICE's y<n>, so each figure
    is one fused layer kernel's own deviation.  T = 1000: ragged against the 64-position tile and below the 2048 dilation;
    T = 64: one tile; T = 4200: every dilation reaches inside the sample."""
    cfg = A.config_c5()
    net, w = make(cfg, "bf16")
    net = net.cuda()
    g = torch.Generator().manual_seed(77 + tlen)
    audio, step = torch.randn(2, tlen, generator=g) * 0.6, torch.tensor([0.45, -1.2])
    y = net(audio.cuda(), step.cuda()).cpu()
    taps = _taps(net, 2)
    errs = {}
    with torch.no_grad():
        y_f = W.wavenet_forward(w, cfg, audio, step, storage="bf16", force=taps, errs=errs)
        y_32 = W.wavenet_forward(w, cfg, audio, step)
    assert set(errs) == set(taps) and len(errs) == cfg.residual_layers + 1
    worst = max(errs, key=errs.get)
    assert errs[worst] < BF16_LAYER_TOL, (worst, errs[worst])
    assert W.rel_l2(y, y_f) < BF16_LAYER_TOL, W.rel_l2(y, y_f)          # final kernel from the device's skip sum
    assert W.rel_l2(y, y_32) < BF16_NET_TOL, W.rel_l2(y, y_32)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [128, 64])
def test_bf16_other_widths_every_layer_vs_bf16_storage_oracle(width):
    """bf16 (MFMA) mode at residual_channels = 128 / 64 (VERDICT r2 "missing" 3: the kernels were built for 256 only): the 128-position layer kernel
    and the final kernel with C / 32 waves.  13 layers with dilations up to 2048 (cycle 12) at T = 4200 (ragged against the tile, every dilation inside
    the sample, both the overlapping-window and the three-window staging paths), teacher-forced per layer against the bf16-storage oracle, and
    fp32 mode of the same net as the storage-precision figure."""
    from audiodiffuser_amd.config import WaveNetConfig
    cfg = WaveNetConfig(residual_channels=width, residual_layers=13, dilation_cycle=12)
    net, w = make(cfg, "bf16")
    net = net.cuda()
    g = torch.Generator().manual_seed(500 + width)
    audio, step = torch.randn(2, 4200, generator=g) * 0.6, torch.tensor([0.45, -1.2])
    y = net(audio.cuda(), step.cuda()).cpu()
    taps = _taps(net, 2)
    errs = {}
    with torch.no_grad():
        y_f = W.wavenet_forward(w, cfg, audio, step, storage="bf16", force=taps, errs=errs)
        y_32 = W.wavenet_forward(w, cfg, audio, step)
    assert set(errs) == set(taps) and len(errs) == cfg.residual_layers + 1
    worst = max(errs, key=errs.get)
    assert errs[worst] < BF16_LAYER_TOL, (worst, errs[worst])
    assert W.rel_l2(y, y_f) < BF16_LAYER_TOL, W.rel_l2(y, y_f)
    assert W.rel_l2(y, y_32) < BF16_NET_TOL, W.rel_l2(y, y_32)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", ["0", "1", "2", "1+prefetch"])
def test_bf16_both_layer_kernel_routes_in_a_child_process(wide):
    """The layer kernel has three routes (128-position tiles, default; 64-position tiles, ADF_WN_WIDE=0; 64-position tiles on four waves, two
    workgroups per CU, ADF_WN_WIDE=2); the switch is read once
    per process, so each runs in its own child: per-layer teacher-forced deviation, the fp32 path, the free-running bf16 net.

    "1+prefetch" sets ADF_WN_PREFETCH=1 but never reaches the prefetch block: the kernel prefetches only when workgroup lin + pf_stride exists, pf_stride is
    the CU count rounded down to a multiple of 8 (256 on an MI355X), and this case launches ceil(1500 / 128) x 2 = 24 workgroups.  It holds the switch's
    plumbing (a non-zero pf_stride changes no value); the global_load_lds_dword block itself runs in
    tests/test_wavenet_sweep_gpu.py::test_bf16_prefetch_that_prefetches_moves_no_value, at 288 workgroups."""
    import json, subprocess, sys
    prefetch = wide.endswith("+prefetch")        # the next-tile L2 prefetch of the 128-position kernel (ADF_WN_PREFETCH=1; off by default: no wall-clock gain)
    wide = wide.split("+")[0]
    env = dict(os.environ, ADF_WN_WIDE=wide, ADF_WN_PREFETCH="1" if prefetch else "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "diag", "gpu_wn_report.py"), "1500", "2"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["route_wide"] == wide and rep["forced_taps"] == 37
    assert rep["forced_max_rel_l2"] < BF16_LAYER_TOL, rep
    assert rep["out_vs_forced_oracle_rel_l2"] < BF16_LAYER_TOL, rep
    assert rep["bf16_vs_fp32_oracle_rel_l2"] < BF16_NET_TOL, rep
    assert rep["fp32_device_vs_oracle_max_rel"] < FP32_TIGHT, rep


@pytest.mark.gpu
def test_denoise_and_heun_sampler_fp32_vs_oracle():
    """The EDM wrapper and a 6-step Heun run (config 5's sampler length: 11 evaluations) around the adapter, eager and
    graph-replayed, against the oracle's wrapper + loop around the pinned network restatement."""
    cfg = A.config_c5_small()
    net, w = make(cfg)
    net = net.cuda()
    diff = A.EluDiffusion(sigma_data=0.5)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 1, 500, generator=g)
    fn_o = lambda xx, sigma=None, sigmas=None: E.denoise(W.wavenet_net(w, cfg), xx, 0.5, sigma=sigma, sigmas=sigmas)
    with torch.no_grad():
        d = diff.denoise_fn(x.cuda(), net=net, inference=True, sigma=2.5).cpu()
        assert rel(d, fn_o(x, sigma=2.5)) < FP32_TIGHT
        sv = torch.tensor([0.3, 4.0, 40.0])
        d = diff.denoise_fn(x.cuda(), net=net, inference=True, sigmas=sv.cuda()).cpu()
        assert rel(d, fn_o(x, sigmas=sv)) < FP32_TIGHT
        sig = A.KarrasSchedule(0.002, 80.0, 7.0, 6)()
        ref = S.edm_sampler(x, fn_o, sig, 6, s_churn=0.0, s_noise=1.0)
        for use_graph in (False, True, True):
            smp = A.EDMSampler(s_churn=0.0, s_noise=1.0, num_steps=6, use_graph=use_graph)
            y = smp(x.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig).cpu()
            assert rel(y, ref) < 5e-5, (use_graph, rel(y, ref))
        # churn (injected draws) and the multistep DPM solver ride on the same handle
        draws = torch.randn(6, 3, 1, 500, generator=g)
        ref = S.edm_sampler(x, fn_o, sig, 6, s_tmin=0.05, s_tmax=50.0, s_churn=3.0, s_noise=1.003, injected_noise=draws)
        y = A.EDMSampler(s_tmin=0.05, s_tmax=50.0, s_churn=3.0, s_noise=1.003, num_steps=6)(
            x.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig, injected_noise=draws.cuda()).cpu()
        assert rel(y, ref) < 5e-5


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_config5_exactly_full_net_22050_samples_6_step_heun_vs_oracle():
    """BASELINE configs[4] at full size: the 36 x 256 `config_c5()` net, T = 22050 (not a multiple of the
    128-position tile), B = 2, 6-step Heun = 11 evaluations, fp32 mode eager and graph-replayed against the oracle's loop around the
    pinned restatement (wavenet.py:169-180 inside sampler_edm.py:333-397); then ONE bf16 forward at T = 22050, teacher-forced
    layer by layer against the bf16-storage oracle."""
    cfg = A.config_c5()
    net, w = make(cfg)
    net = net.cuda()
    diff = A.EluDiffusion(sigma_data=0.5)
    g = torch.Generator().manual_seed(55)
    x = torch.randn(2, 1, 22050, generator=g)
    sig = A.KarrasSchedule(0.002, 80.0, 7.0, 6)()
    fn_o = lambda xx, sigma=None, sigmas=None: E.denoise(W.wavenet_net(w, cfg), xx, 0.5, sigma=sigma, sigmas=sigmas)
    with torch.no_grad():
        ref = S.edm_sampler(x, fn_o, sig, 6, s_churn=0.0, s_noise=1.0)
    for use_graph in (False, True):
        y = A.EDMSampler(s_churn=0.0, s_noise=1.0, num_steps=6, use_graph=use_graph)(x.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig).cpu()
        assert rel(y, ref) < 1e-4, (use_graph, rel(y, ref))              # 11 chained evaluations; north-star bar 1e-3
    n16, _ = make(cfg, "bf16")
    n16 = n16.cuda()
    a, st = torch.randn(1, 22050, generator=g) * 0.8, torch.tensor([0.3])
    y16 = n16(a.cuda(), st.cuda()).cpu()
    hd = n16.native(torch.device("cuda", torch.cuda.current_device()))
    taps = {k: hd.tap(k, 1, torch.device("cuda")).cpu() for k in hd.tap_names()}
    errs = {}
    with torch.no_grad():
        y_f = W.wavenet_forward(w, cfg, a, st, storage="bf16", force=taps, errs=errs)
    assert len(errs) == 37 and set(errs) == set(taps)
    worst = max(errs, key=errs.get)
    assert errs[worst] < BF16_LAYER_TOL, (worst, errs[worst])
    assert W.rel_l2(y16, y_f) < BF16_LAYER_TOL, W.rel_l2(y16, y_f)


@pytest.mark.gpu
def test_bf16_sampler_against_fp32_device_run_and_weight_reload():
    """6-step Heun on the default net: bf16 against the fp32 device path (a storage-precision figure), and a reloaded state_dict
    rebuilds the effective (weight-normed) weights."""
    cfg = A.config_c5()
    n32, w = make(cfg)
    n16, _ = make(cfg, "bf16")
    n32, n16 = n32.cuda(), n16.cuda()
    diff = A.EluDiffusion(sigma_data=0.5)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 1, 700, generator=g)
    sig = A.KarrasSchedule(0.002, 80.0, 7.0, 6)()
    smp = A.EDMSampler(s_churn=0.0, s_noise=1.0, num_steps=6)
    y32 = smp(x.cuda(), fn=diff.denoise_fn, net=n32, sigmas=sig).cpu()
    y16 = smp(x.cuda(), fn=diff.denoise_fn, net=n16, sigmas=sig).cpu()
    assert W.rel_l2(y16, y32) < 6e-2, W.rel_l2(y16, y32)
    w2 = generate_wavenet_weights(cfg, seed=6)
    n32.load_state_dict(w2)
    a, st = torch.randn(1, 256, generator=g), torch.tensor([0.1])
    with torch.no_grad():
        ref = W.wavenet_forward(w2, cfg, a, st)
    assert rel(n32(a.cuda(), st.cuda()).cpu(), ref) < FP32_TIGHT


@pytest.mark.gpu
def test_plan_cache_bounds_and_weight_update_on_the_second_network_kind():
    """The workspace cap (4 (B, L) plans per handle) and the rebuilt weight-normed weights also hold for a WaveNetNoise handle: six shapes in a
    row, the first one again, then an in-place parameter update."""
    cfg = A.config_c5_small()
    net, w = make(cfg)
    net = net.cuda()
    g = torch.Generator().manual_seed(21)
    first = None
    for i, (b, t) in enumerate([(2, 100), (1, 300), (3, 64), (2, 257), (1, 1000), (4, 33), (2, 100)]):
        a, st = torch.randn(b, t, generator=g), torch.linspace(-0.5, 0.5, b)
        if i in (0, 6):
            gg = torch.Generator().manual_seed(99)
            a = torch.randn(b, t, generator=gg)
        y = net(a.cuda(), st.cuda()).cpu()
        with torch.no_grad():
            ref = W.wavenet_forward(w, cfg, a, st)
        assert rel(y, ref) < FP32_TIGHT, (i, rel(y, ref))
        if i == 0:
            first = y
    assert torch.equal(first, y)                      # the evicted and rebuilt workspace computes the same
    with torch.no_grad():                             # an in-place update of g bumps the tensor version: the effective weights are rebuilt
        net.get_parameter("skip_projection.conv.module.weight_g").mul_(1.5)
    w2 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    a, st = torch.randn(2, 100, generator=g), torch.tensor([0.1, -0.2])
    with torch.no_grad():
        ref = W.wavenet_forward(w2, cfg, a, st)
    assert rel(net(a.cuda(), st.cuda()).cpu(), ref) < FP32_TIGHT
