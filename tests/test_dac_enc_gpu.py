"""GPU: ``audiodiffuser_amd.DACEncoder`` and ``FineTuneAutoencoder.encode`` / ``.forward`` (``is_train=False``) against the float64 restatement
tests/dac_enc_ref.py (every tap of every case) and against the reference modules' own results (tests/golden/dac_enc_golden.npz,
tools/gen_golden_dac_enc.py).

Bars: FP32_TIGHT = 5e-5 of max |reference| per tensor (the project's exact-fp32 bar, tests/test_dac_gpu.py) for every forward and tap, and the same
5e-5 relative for the KL term (tests/test_dac_enc_ref.py asserts what that rests on: the reference arithmetic in fp32 is within 5e-6 of float64 on
every autoencoder case); DEN_TOL = 1e-4 for the encoder -> autoencoder chain.  With ADF_DAC_ENC_REPORT=<path> the worst measured value per case is
written there as JSON (the committed copy: tests/golden/dac_enc_report.json).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
import dac_enc_ref as ER
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
    path = os.environ.get("ADF_DAC_ENC_REPORT")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump({"bar_forward": FP32_TIGHT, "bar_kl": FP32_TIGHT, "bar_chain": DEN_TOL, "measured": MEASURED}, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "dac_enc_golden.npz"))


def build(case, w=None):
    net = A.FineTuneAutoencoder(**ER.ctor_kwargs(case)) if ER.kind(case) == "ae" else A.DACEncoder(**ER.ctor_kwargs(case))
    net.load_state_dict(ER.weights(case) if w is None else w, strict=True)
    return net.cuda()


device_net = functools.lru_cache(maxsize=None)(build)


def run(net, x):
    """The encoder's result, or the autoencoder's (mean, kl)."""
    with torch.no_grad():
        return net.encode(x.cuda(), is_train=False) if isinstance(net, A.FineTuneAutoencoder) else net(x.cuda())


def device_taps(net, B):
    hd, dev = net.native(torch.device("cuda", torch.cuda.current_device())), torch.device("cuda")
    return {name: hd.tap(name, B, dev).cpu() for name in hd.tap_names()}


def distances(case, y, ref, got, ref_taps):
    """Every distance of one case: the result (the autoencoder's mean and kl), then every tap."""
    if ER.kind(case) == "ae":
        (mean, kl), (rmean, rkl) = y, ref
        assert mean.dtype == torch.float32 and tuple(mean.shape) == tuple(rmean.shape) and kl.ndim == 0 and kl.dtype == torch.float32
        worst = {"mean": rel(mean, rmean), "kl": abs(float(kl) - float(rkl)) / abs(float(rkl))}
    else:
        assert y.dtype == torch.float32 and tuple(y.shape) == tuple(ref.shape)
        worst = {"out": rel(y, ref)}
    assert sorted(got) == sorted(ref_taps)
    for n, r in ref_taps.items():
        assert tuple(got[n].shape) == tuple(r.shape), n
        worst[n] = rel(got[n], r)
    return worst


# ---- forward and taps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ER.CASES))
def test_forward_and_every_tap_vs_float64(case):
    net, x = device_net(case), ER.inputs(case)
    ref, ref_taps = ER.reference(case)
    y = run(net, x)
    if ER.kind(case) == "enc":
        assert y.shape[-1] == net.output_length(x.shape[-1]) == ER.output_length(case) == ER.LENGTHS[case][-1]
    worst = distances(case, y, ref, device_taps(net, x.shape[0]), ref_taps)
    print(case, worst)
    MEASURED[f"forward_fp64/{case}"] = max(worst.values())
    assert max(worst.values()) < FP32_TIGHT, worst


@pytest.mark.gpu
def test_both_clamps_bind_on_the_device():
    """ae_clamp: the raw bottleneck tap holds a logvar above 20 and one below -30, and the KL term is the clamped one (the unclamped one is e^5 away)."""
    net, x = device_net("ae_clamp"), ER.inputs("ae_clamp")
    _, kl = run(net, x)
    raw = device_taps(net, 1)["btnk_layer"][:, 8:]
    assert float(raw.max()) > 20.0 and float(raw.min()) < -30.0
    with torch.no_grad():
        _, unclamped = ER.forward("ae_clamp", bug="no_clamp")
    _, rkl = ER.reference("ae_clamp")[0]
    assert abs(float(kl) - float(rkl)) / float(rkl) < FP32_TIGHT and float(unclamped) > 50 * float(rkl)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ER.GOLDEN_CASES)
def test_forward_and_taps_vs_reference_goldens(gold, case):
    net, x = device_net(case), torch.from_numpy(gold[f"{case}_x"])
    y = run(net, x)
    got = device_taps(net, x.shape[0])
    if ER.kind(case) == "ae":
        gkl = float(gold[f"{case}_kl"])
        worst = {"mean": rel(y[0], torch.from_numpy(gold[f"{case}_out"])), "kl": abs(float(y[1]) - gkl) / abs(gkl)}
    else:
        worst = {"out": rel(y, torch.from_numpy(gold[f"{case}_out"]))}
    names = ER.golden_taps(gold.files, case)
    assert names
    for n in names:
        worst[n] = rel(got[n], torch.from_numpy(gold[f"{case}_{n}"]))
    print(case, worst)
    MEASURED[f"forward_golden/{case}"] = max(worst.values())
    assert max(worst.values()) < FP32_TIGHT, worst


@pytest.mark.gpu
def test_other_shapes_on_one_handle_and_back():
    """Plan reuse and new plans on one handle: the same encoder at another L and another B, then the first shape again; the same for encode."""
    net, w, cfg = device_net("r8"), ER.weights("r8"), ER.config("r8")
    for B, L, seed in ((1, 887, 1), (2, 26, 2), (3, 1000, 3), (1, 887, 4)):          # 26 -> 9 -> 1: both stages near their minimum
        x = 0.5 * torch.randn((B, 1, L), generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            ref = ER.encoder_forward(w, cfg, x)
        y = run(net, x)
        assert y.shape == ref.shape
        d = rel(y, ref)
        MEASURED[f"reuse/B{B}_L{L}"] = d
        assert d < FP32_TIGHT, (B, L, d)
    net, w, cfg = device_net("ae_small"), ER.weights("ae_small"), ER.config("ae_small")
    for B, T, seed in ((1, 5, 1), (3, 130, 2), (1, 5, 3)):
        x = torch.randn((B, 1024, T), generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            rmean, rkl = ER.autoencoder_encode(w, cfg, x)
        mean, kl = run(net, x)
        d = max(rel(mean, rmean), abs(float(kl) - float(rkl)) / abs(float(rkl)))
        MEASURED[f"reuse_ae/B{B}_T{T}"] = d
        assert d < FP32_TIGHT, (B, T, d)


@pytest.mark.gpu
def test_kl_over_several_chunks_per_sample():
    """latent_dim * T = 32 * 300 = 9600 elements per sample: three 4096-element blocks each, so the per-sample chunk sums and their fixed-order
    reduction over chunks and batch run (every other case fits one block per sample)."""
    net, w, cfg = device_net("ae"), ER.weights("ae"), ER.config("ae")
    B, T = 2, 300
    assert cfg.input_channel * T > 2 * 4096
    x = torch.randn((B, 1024, T), generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        rmean, rkl = ER.autoencoder_encode(w, cfg, x)
    mean, kl = run(net, x)
    mean2, kl2 = run(net, x)
    assert torch.equal(kl, kl2) and torch.equal(mean, mean2)
    d = {"mean": rel(mean, rmean), "kl": abs(float(kl) - float(rkl)) / abs(float(rkl))}
    MEASURED["chunks/ae_B2_T300"] = max(d.values())
    assert max(d.values()) < FP32_TIGHT, d


@pytest.mark.gpu
def test_latent_dim_above_1024_encodes_and_decodes_on_one_handle():
    """latent_dim = 2048: encode's [B][2048][T] mean is wider than decode's [B][1024][T] result, and the handle's workspaces hold the larger of the two
    (the first encode of a shape runs a warm-up pass into them)."""
    cfg = ER.DACConfig(kind=1, input_channel=2048, widths=[1024, 64])
    w = ER.generate_enc(cfg, seed=5)
    net = A.FineTuneAutoencoder(intermediate_embedding_size=[1024, 64], latent_dim=2048)
    net.load_state_dict(w, strict=True)
    net = net.cuda()
    x = torch.randn((2, 1024, 5), generator=torch.Generator().manual_seed(12))
    z = torch.randn((2, 2048, 5), generator=torch.Generator().manual_seed(13))
    with torch.no_grad():
        rmean, rkl = ER.autoencoder_encode(w, cfg, x)
        rdec = DR.autoencoder_decode(w, cfg, z)
        mean, kl = net.encode(x.cuda(), is_train=False)
        dec = net.decode(z.cuda())
        mean2, kl2 = net.encode(x.cuda(), is_train=False)
    assert tuple(mean.shape) == (2, 2048, 5) and torch.equal(mean, mean2) and torch.equal(kl, kl2)
    d = {"mean": rel(mean, rmean), "kl": abs(float(kl) - float(rkl)) / abs(float(rkl)), "decode": rel(dec, rdec)}
    MEASURED["latent_2048"] = max(d.values())
    assert max(d.values()) < FP32_TIGHT, d


@pytest.mark.gpu
def test_a_too_short_length_is_refused_by_name():
    net = device_net("short")
    assert net.output_length(47) == 1
    with pytest.raises(ValueError, match="L is too short"):
        net(torch.zeros(1, 1, 35).cuda())                # 35 -> 8 -> 1, and the stride-2 stage needs 2
    hd = net.native(torch.device("cuda", torch.cuda.current_device()))
    out = torch.empty(1, 32, 1, device="cuda")
    x = torch.zeros(1, 1, 3, device="cuda")
    rc = hd.lib.adf_dac_forward(hd.h, x.data_ptr(), 1, 3, out.data_ptr(), None)
    assert rc != 0 and "L = 3" in hd.lib.adf_last_error(hd.h).decode()
    assert hd.lib.adf_dac_output_length(hd.h, 3) == -1 and hd.lib.adf_dac_output_length(hd.h, 47) == 1


@pytest.mark.gpu
def test_in_place_units_without_unit_taps(monkeypatch):
    """ADF_DAC_TAPS=0 (read when the handle is created): the route a net takes on its own once the taps pass 512 MiB."""
    monkeypatch.setenv("ADF_DAC_TAPS", "0")
    net, x = build("odd"), ER.inputs("odd")
    ref, ref_taps = ER.reference("odd")
    y = run(net, x)
    got = device_taps(net, x.shape[0])
    assert sorted(got) == ["block.0", "block.1", "block.2", "block.3", "block.5"]
    worst = {"out": rel(y, ref), **{n: rel(got[n], ref_taps[n]) for n in got}}
    MEASURED["in_place/odd"] = max(worst.values())
    assert max(worst.values()) < FP32_TIGHT, worst


@pytest.mark.gpu
def test_reloading_weight_g_alone_refolds_the_weight():
    """The down conv's weight_g: the fold kind this feature adds."""
    w, cfg, x = ER.weights("long"), ER.config("long"), ER.inputs("long")
    net = build("long", w)
    y0 = run(net, x)
    key = "block.1.block.4.weight_g"
    w2 = dict(w)
    w2[key] = w[key] * torch.linspace(0.5, 1.5, w[key].numel()).view_as(w[key])
    with torch.no_grad():
        dict(net.named_parameters())[key].copy_(w2[key].cuda())
        ref0, ref2 = ER.encoder_forward(w, cfg, x), ER.encoder_forward(w2, cfg, x)
    y2 = run(net, x)
    moved = rel(ref2, ref0)
    d0, d2 = rel(y0, ref0), rel(y2, ref2)
    MEASURED["reload/weight_g"] = max(d0, d2)
    assert moved > 100 * FP32_TIGHT, moved
    assert d0 < FP32_TIGHT and d2 < FP32_TIGHT, (d0, d2, moved)


def _captured(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


@pytest.mark.gpu
def test_graph_captured_forward_replays_bit_equal():
    net, x = device_net("w96"), ER.inputs("w96").cuda()
    eager = run(net, x).clone()
    xs = x.clone()
    g, out = _captured(lambda: run(net, xs))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    xs.copy_(x.flip(0).contiguous() * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, run(net, xs))


@pytest.mark.gpu
def test_graph_captured_encode_replays_bit_equal_and_two_eager_encodes_agree():
    net, x = device_net("ae_small"), ER.inputs("ae_small").cuda()
    m0, k0 = run(net, x)
    m1, k1 = run(net, x)
    assert torch.equal(m0, m1) and torch.equal(k0, k1)           # (no float atomics: the KL term is the same bits every time)
    xs = x.clone()
    g, (mean, kl) = _captured(lambda: run(net, xs))
    mean.zero_()
    kl.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(mean, m0) and torch.equal(kl, k0)
    xs.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    m2, k2 = run(net, xs)
    assert torch.equal(mean, m2) and torch.equal(kl, k2) and not torch.equal(k2, k0)


@pytest.mark.gpu
def test_decode_after_encode_is_bit_equal_to_decode_on_a_fresh_handle():
    w = ER.weights("ae")
    z = DR.inputs("ae").cuda()
    fresh, used = build("ae", w), build("ae", w)
    with torch.no_grad():
        want = fresh.decode(z)
        used.encode(ER.inputs("ae").cuda(), is_train=False)
        got = used.decode(z)
        used.encode(ER.inputs("ae").cuda(), is_train=False)
        again = used.decode(z)
    assert torch.equal(got, want) and torch.equal(again, want)
    hd = used.native(torch.device("cuda", torch.cuda.current_device()))
    assert sorted(hd.tap_names()) == sorted(f"decoder_layers.{2 * i}" for i in range(4))      # the taps are the last call's


@pytest.mark.gpu
def test_forward_is_decode_of_the_encoded_mean():
    net, x = device_net("ae_tanh"), ER.inputs("ae_tanh").cuda()
    with torch.no_grad():
        y, kl = net(x, is_train=False)
        mean, kl2 = net.encode(x, is_train=False)
        assert torch.equal(y, net.decode(mean)) and torch.equal(kl, kl2)
    assert float(mean.abs().max()) <= 1.0 and tuple(y.shape) == tuple(x.shape)


@pytest.mark.gpu
def test_chain_audio_to_latent():
    """``ae.encode(enc(audio))``: an encoder with d_latent = 1024 feeding ae_small's encode."""
    ae, wa, ca = device_net("ae_small"), ER.weights("ae_small"), ER.config("ae_small")
    ce = ER.DACConfig(kind=2, input_channel=1, channels=32, rates=[3, 4], d_out=1024)
    we = ER.generate_enc(ce, seed=77)
    enc = A.DACEncoder(32, [3, 4], 1024)
    enc.load_state_dict(we, strict=True)
    enc = enc.cuda()
    audio = 0.5 * torch.randn((2, 1, 200), generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        rmean, rkl = ER.autoencoder_encode(wa, ca, ER.encoder_forward(we, ce, audio))
        mean, kl = ae.encode(enc(audio.cuda()), is_train=False)
    assert tuple(mean.shape) == (2, 8, enc.output_length(200)) == tuple(rmean.shape)
    d = max(rel(mean, rmean), abs(float(kl) - float(rkl)) / abs(float(rkl)))
    MEASURED["chain/ae_small"] = d
    assert d < DEN_TOL, d


@pytest.mark.gpu
def test_encode_refuses_other_handles():
    enc = device_net("w96")
    hd = enc.native(torch.device("cuda", torch.cuda.current_device()))
    x = torch.zeros(1, 1024, 4, device="cuda")
    m, k = torch.zeros(1, 8, 4, device="cuda"), torch.zeros((), device="cuda")
    assert hd.lib.adf_dac_encode(hd.h, x.data_ptr(), 1, 4, m.data_ptr(), k.data_ptr(), None) != 0
    assert "autoencoder" in hd.lib.adf_last_error(hd.h).decode()
    with pytest.raises(A._lib.AdfError, match="DAC"):
        hd.denoise(torch.zeros(1, 1, 16, device="cuda"), 0.2, sigma=1.0)
