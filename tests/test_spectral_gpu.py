"""GPU: SpecToWave (csrc/adf_istft.hip) against torch.istft in FLOAT64 ON THE CPU applied to spec_back in float64 of the same fp32 input -- the four
reference lines it replaces (src/models/diffunet_complex_module.py:90-99, src/models/utils.py:22-28), written out below.  The oracle is float64,
so the device's arithmetic is never its own yardstick.  Error = max|a - b| / max|b|; bar FP32_TIGHT (5e-5), the project's guard for exact-fp32 paths.
For orientation (no bar): torch.istft in fp32 on the CPU sits at 1.8e-7 .. 4.4e-7 from the same oracle.

Worst measured value per case on an MI355X (WORST_MEASURED below is what a run prints beside its own figure):
    shipped_small 1.7e-6   shipped_frames 1.0e-6   two_frames 8.4e-7   tile_edge 1.5e-6   plain 1.4e-6   general_pow 1.4e-6
    d8 9.0e-7   ragged 4.3e-7   small_f 4.6e-7   wide 1.6e-6   custom_window 1.7e-6   zeros_and_ignored_rows 1.1e-6   call_site 5.1e-7
The K = 2048 products of a shipped-geometry sample are one k-ordered fp32 fmaf chain on the MFMA (no pairwise tree as in an FFT), hence a few 1e-6
where torch's fp32 istft has a few 1e-7; every case is below the 5e-6 at which a case wants a look.
"""
import pytest
import torch

import audiodiffuser_amd as A
from oracle import unet2d as U
from test_gpu_parity import FP32_TIGHT

WORST_MEASURED = {"shipped_small": 1.7e-6, "shipped_frames": 1.0e-6, "two_frames": 8.4e-7, "tile_edge": 1.5e-6, "plain": 1.4e-6, "general_pow": 1.4e-6,
                  "d8": 9.0e-7, "ragged": 4.3e-7, "small_f": 4.6e-7, "wide": 1.6e-6, "custom_window": 1.7e-6}


def spec_back(z, e, f):
    """src/models/utils.py:22-28."""
    z = z / f
    if e != 1:
        z = z.abs() ** (1 / e) * torch.exp(1j * z.angle())
    return z


def oracle(x, n_fft, hop, e, f, window=None, normalized=True):
    """The reference's four lines in float64 on the CPU."""
    x = x.detach().cpu().double()
    z = torch.view_as_complex(x.permute(0, 2, 3, 1).contiguous())
    z = spec_back(z, e, f)
    w = window.detach().cpu().double() if window is not None else torch.hann_window(n_fft, dtype=torch.float64)
    return torch.istft(z, window=w, normalized=normalized, n_fft=n_fft, hop_length=hop, center=True)


def rel(a, b):
    return float((a.detach().cpu().double() - b).abs().max() / b.abs().max())


def make_input(B, n_fft, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 2, n_fft // 2 + 1, T, generator=g) * 0.5


#        name             B  n_fft hop  T    e    factor
CASES = [("shipped_small", 2, 510, 128, 8, 0.2, 0.6),
         ("shipped_frames", 3, 510, 128, 128, 0.2, 0.6),
         ("two_frames", 2, 510, 128, 2, 0.2, 0.6),
         ("tile_edge", 2, 510, 128, 37, 0.5, 0.3),
         ("plain", 2, 510, 128, 5, 1.0, 0.6),
         ("general_pow", 2, 510, 128, 5, 0.3, 0.45),
         ("d8", 2, 256, 32, 9, 0.2, 0.6),
         ("ragged", 2, 128, 96, 6, 0.2, 0.6),
         ("small_f", 2, 126, 32, 7, 0.5, 0.3),
         ("wide", 1, 1022, 256, 4, 0.2, 0.6),
         ("custom_window", 2, 510, 128, 6, 0.2, 0.6)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,n_fft,hop,T,e,f", CASES, ids=[c[0] for c in CASES])
def test_parity_with_the_float64_oracle(name, B, n_fft, hop, T, e, f):
    x = make_input(B, n_fft, T, seed=len(name) + T)
    win = torch.hamming_window(510) if name == "custom_window" else None
    ref = oracle(x, n_fft, hop, e, f, window=win)
    out = A.SpecToWave(n_fft=n_fft, hop_length=hop, spec_abs_exponent=e, spec_factor=f, window=win)(x.cuda())
    assert out.shape == (B, hop * (T - 1)) == tuple(ref.shape) and out.dtype == torch.float32 and out.is_cuda
    assert bool(torch.isfinite(out).all())
    err = rel(out, ref)
    print(f"spec_to_wave {name}: rel err {err:.3e} (worst measured {WORST_MEASURED[name]:.1e}, bar {FP32_TIGHT:.0e})")
    assert err < FP32_TIGHT, (name, err)


@pytest.mark.gpu
def test_zero_frames_zero_bins_and_the_ignored_imaginary_rows():
    """Exact zeros take the r == 0 branch of spec_back; the imaginary parts of the DC and Nyquist rows enter |z| (the reference's abs()) but not the
    transform (the c2r FFT ignores them)."""
    n_fft, hop, T, e, f = 510, 128, 6, 0.2, 0.6
    x = make_input(2, n_fft, T, seed=11)
    x[:, :, :, 2] = 0.0                                     # a whole frame
    x[1, :, :, 5] = 0.0
    g = torch.Generator().manual_seed(12)
    x = x * (torch.rand(1, 1, x.shape[2], T, generator=g) > 0.2)          # scattered bins, both components
    x[:, 1, 0, :] = 1.5
    x[:, 1, -1, :] = -1.25
    x[:, :, :, 2] = 0.0
    assert int((x[:, 0] == 0).logical_and(x[:, 1] == 0).sum()) > 2 * 256
    ref = oracle(x, n_fft, hop, e, f)
    x0 = x.clone()
    x0[:, 1, 0, :] = 0.0
    x0[:, 1, -1, :] = 0.0
    moved = float((oracle(x0, n_fft, hop, e, f) - ref).abs().max() / ref.abs().max())
    assert moved > 1e-3, moved                                  # they do enter r: a kernel that dropped them on the way in would be caught
    out = A.SpecToWave(n_fft=n_fft, hop_length=hop, spec_abs_exponent=e, spec_factor=f)(x.cuda())
    assert bool(torch.isfinite(out).all())
    err = rel(out, ref)
    print(f"spec_to_wave zeros_and_ignored_rows: rel err {err:.3e}, oracle moves by {moved:.2e} without the two imaginary rows")
    assert err < FP32_TIGHT, err


@pytest.mark.gpu
def test_bit_for_bit_repeat_batch_independence_and_stream():
    m = A.SpecToWave()
    x = make_input(3, 510, 40, seed=21).cuda()
    a = m(x)
    b = m(x)
    assert torch.equal(a, b)
    assert torch.equal(m(x[1:2].contiguous())[0], a[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = m(x)
    side.synchronize()
    assert torch.equal(c, a)


def three_level():
    """The constructor of tests/test_unet2d_host.py::three_level."""
    return U.UNet2dConfig(dim=128, num_classes=0, dim_mults=(1, 2, 2), channels=2, num_resnet_blocks=1, resnet_groups=8,
                          layer_attns=(False, True, True), layer_cross_attns=(False, True, False), attn_heads=4, ff_mult=1.5,
                          layer_attns_depth=2, memory_efficient=True, scale_skip_connection=False, init_cross_embed_kernel_sizes=(5, 3))


@pytest.mark.gpu
def test_call_site_takes_the_samplers_tensor_as_it_is(request):
    """synthesize_from_noise: the native sampler's [B, 2, F, T] output goes into SpecToWave without a copy or a permute."""
    cfg = three_level()
    net = A.UNet2dBase(**cfg.to_kwargs())
    net.load_state_dict(U.generate_weights(cfg, 5), strict=True)
    net = net.cuda()
    noise = torch.randn(2, 2, 32, 32, generator=torch.Generator().manual_seed(4))
    sig = A.KarrasSchedule(0.002, 80.0, 7.0, 4)()
    smp = A.DPMSampler(cond_scale=1.0, order=3, num_steps=4, multisteps=True, x0_pred=True, log_time_spacing=False, use_graph=False)
    spec = smp(noise.cuda(), fn=A.EluDiffusion(sigma_data=0.2).denoise_fn, net=net, sigmas=sig)
    assert request.node._adf_seen["runs"] == 1                 # conftest: adf_sampler_run served it
    assert spec.shape == (2, 2, 32, 32) and spec.is_cuda and spec.is_contiguous()
    audio = A.SpecToWave(n_fft=62, hop_length=32)(spec)
    ref = oracle(spec, 62, 32, 0.2, 0.6)
    assert audio.shape == (2, 32 * 31) == tuple(ref.shape) and bool(torch.isfinite(audio).all())
    assert float(ref.abs().max()) > 1e-3
    err = rel(audio, ref)
    print(f"spec_to_wave call_site: rel err {err:.3e}")
    assert err < FP32_TIGHT, err
