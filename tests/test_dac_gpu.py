"""GPU: ``audiodiffuser_amd.DACDecoder`` and ``FineTuneAutoencoder.decode`` against the float64 restatement tests/dac_ref.py (every tap of every
case) and against the reference modules' own results (tests/golden/dac_golden.npz, tools/gen_golden_dac.py).

Bars: FP32_TIGHT = 5e-5 of max |reference| per tensor (the project's exact-fp32 bar, tests/test_dit_gpu.py) for every forward and tap; DEN_TOL = 1e-4
for the autoencoder -> decoder chain.  With ADF_DAC_REPORT=<path> the worst measured value per case is written there as JSON (the committed copy:
tests/golden/dac_report.json).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
import dac_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TIGHT = 5e-5
DEN_TOL = 1e-4
MEASURED = {}


def rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("ADF_DAC_REPORT")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump({"bar_forward": FP32_TIGHT, "bar_chain": DEN_TOL, "measured": MEASURED}, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "dac_golden.npz"))


def build(case, w=None):
    net = A.FineTuneAutoencoder(**DR.ctor_kwargs(case)) if DR.kind(case) == "ae" else A.DACDecoder(**DR.ctor_kwargs(case))
    net.load_state_dict(DR.weights(case) if w is None else w, strict=True)
    return net.cuda()


device_net = functools.lru_cache(maxsize=None)(build)


def run(net, x):
    with torch.no_grad():
        return net.decode(x.cuda()) if isinstance(net, A.FineTuneAutoencoder) else net(x.cuda())


def device_taps(net, B):
    hd, dev = net.native(torch.device("cuda", torch.cuda.current_device())), torch.device("cuda")
    return {name: hd.tap(name, B, dev).cpu() for name in hd.tap_names()}


# ---- forward and taps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(DR.CASES))
def test_forward_and_every_tap_vs_float64(case):
    net, x = device_net(case), DR.inputs(case)
    ref, ref_taps = DR.reference(case)
    y = run(net, x)
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(ref.shape)
    if DR.kind(case) == "dec":
        assert y.shape[-1] == net.output_length(x.shape[-1]) == DR.output_length(case)
    got = device_taps(net, x.shape[0])
    assert sorted(got) == sorted(ref_taps)
    worst = {"out": rel(y, ref)}
    for n, r in ref_taps.items():
        assert tuple(got[n].shape) == tuple(r.shape), n
        worst[n] = rel(got[n], r)
    print(case, worst)
    MEASURED[f"forward_fp64/{case}"] = max(worst.values())
    assert max(worst.values()) < FP32_TIGHT, worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", DR.GOLDEN_CASES)
def test_forward_and_taps_vs_reference_goldens(gold, case):
    net, x = device_net(case), torch.from_numpy(gold[f"{case}_x"])
    y = run(net, x)
    got = device_taps(net, x.shape[0])
    worst = {"out": rel(y, torch.from_numpy(gold[f"{case}_out"]))}
    names = [k[len(case) + 1:] for k in gold.files if k.startswith(case + "_") and k not in (f"{case}_x", f"{case}_out")]
    assert names
    for n in names:
        worst[n] = rel(got[n], torch.from_numpy(gold[f"{case}_{n}"]))
    print(case, worst)
    MEASURED[f"forward_golden/{case}"] = max(worst.values())
    assert max(worst.values()) < FP32_TIGHT, worst


@pytest.mark.gpu
def test_second_and_third_forward_on_one_handle_other_length_other_batch():
    """Plan reuse and new plans on one handle: the same net at another T and another B, then the first shape again."""
    net, w, cfg = device_net("r8"), DR.weights("r8"), DR.config("r8")
    for B, T, seed in ((1, 37, 1), (2, 9, 2), (3, 130, 3), (1, 37, 4)):
        x = torch.randn((B, cfg.input_channel, T), generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            ref = DR.decoder_forward(w, cfg, x)
        y = run(net, x)
        assert y.shape == ref.shape
        d = rel(y, ref)
        MEASURED[f"reuse/B{B}_T{T}"] = d
        assert d < FP32_TIGHT, (B, T, d)


@pytest.mark.gpu
def test_in_place_units_without_unit_taps(monkeypatch):
    """ADF_DAC_TAPS=0 (read when the handle is created): the route a net takes on its own once the taps pass 512 MiB -- every unit adds into its input."""
    monkeypatch.setenv("ADF_DAC_TAPS", "0")
    net, x = build("odd"), DR.inputs("odd")
    ref, ref_taps = DR.reference("odd")
    y = run(net, x)
    got = device_taps(net, x.shape[0])
    assert sorted(got) == ["model.0", "model.1", "model.2", "model.3"]
    worst = {"out": rel(y, ref), **{n: rel(got[n], ref_taps[n]) for n in got}}
    MEASURED["in_place/odd"] = max(worst.values())
    assert max(worst.values()) < FP32_TIGHT, worst


@pytest.mark.gpu
def test_reloading_weight_g_alone_refolds_the_weight():
    w, cfg, x = DR.weights("long"), DR.config("long"), DR.inputs("long")
    net = build("long", w)
    y0 = run(net, x)
    key = "model.1.block.3.block.1.weight_g"
    w2 = dict(w)
    w2[key] = w[key] * torch.linspace(0.5, 1.5, w[key].numel()).view_as(w[key])
    with torch.no_grad():
        dict(net.named_parameters())[key].copy_(w2[key].cuda())
        ref0, ref2 = DR.decoder_forward(w, cfg, x), DR.decoder_forward(w2, cfg, x)
    y2 = run(net, x)
    moved = rel(ref2, ref0)
    d0, d2 = rel(y0, ref0), rel(y2, ref2)
    MEASURED["reload/weight_g"] = max(d0, d2)
    assert moved > 100 * FP32_TIGHT, moved            # (the new weights are another function ...)
    assert d0 < FP32_TIGHT and d2 < FP32_TIGHT, (d0, d2, moved)      # ... and the device follows them


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["w96", "ae_small"])
def test_graph_capture_replays_bit_equal(case):
    net, x = device_net(case), DR.inputs(case).cuda()
    eager = run(net, x).clone()
    xs = x.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(net, xs)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        out = run(net, xs)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    xs.copy_(x.flip(0).contiguous() * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, run(net, xs))


@pytest.mark.gpu
def test_chain_latent_to_waveform():
    """``dec(ae.decode(latents))``: ae_small's decode feeding a decoder with input_channel = 1024 at T = 5."""
    ae, wa, ca = device_net("ae_small"), DR.weights("ae_small"), DR.config("ae_small")
    cd = DR.DACConfig(kind=0, input_channel=1024, channels=128, rates=[4, 3])
    wd = DR.generate(cd, seed=77)
    dec = A.DACDecoder(1024, 128, [4, 3])
    dec.load_state_dict(wd, strict=True)
    dec = dec.cuda()
    z = DR.inputs("ae_small")
    with torch.no_grad():
        ref = DR.decoder_forward(wd, cd, DR.autoencoder_decode(wa, ca, z))
        y = dec(ae.decode(z.cuda()))
    assert tuple(y.shape) == (1, 1, dec.output_length(5)) == tuple(ref.shape)
    d = rel(y, ref)
    MEASURED["chain/ae_small"] = d
    assert d < DEN_TOL, d


@pytest.mark.gpu
def test_denoiser_and_sampler_calls_refuse_a_dac_handle():
    net = device_net("w96")
    hd = net.native(torch.device("cuda", torch.cuda.current_device()))
    x = torch.zeros(1, 8, 16, device="cuda")
    with pytest.raises(A._lib.AdfError, match="DAC"):
        hd.net_forward(x, torch.zeros(1, device="cuda"))
    with pytest.raises(A._lib.AdfError, match="DAC"):
        hd.denoise(x, 0.2, sigma=1.0)
