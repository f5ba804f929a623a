"""CPU side of the I/O cases of the 1-D U-Net (oracle/unet1d_sweep.py IO_CASES; the device side is tests/test_unet1d_io_gpu.py): the oracle is pinned to the
reference at every case, its float64 run is the reference of the GPU module, the cases reach the kernels they were chosen for (derived from the launchers'
gates as config.py restates them), and the constructor refuses the windows and strides the reference itself cannot run.

Truncating split on ``out`` (the cases where to_out_x3_kernel runs), relative L2 of the truncating variant from the rounding one on the same forced inputs,
against 2 * X3_LAUNCH_TOL = 5.6e-6: measured k12s4 2.5e-5, k16s4n128 2.7e-5, k8s2n128 2.8e-5, k8s2st 2.7e-5 (the same products summed in fp32: 8.7e-8 .. 1.7e-7) -- every case holds, the bar
stays.  Clamped share of the epilogue inputs per sample, float64 oracle: k3s1 30 / 63 %, k9s3 31 / 36 / 41 %, k12s4 31 / 27 %, k16s4n128 33 / 34 %,
k8s2n160 28 / 49 %, k8s8 31 / 12 %, k8s2n128 33 / 50 %."""
import os

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd.config import UNet1dConfig
from audiodiffuser_amd.weights import generate_weights
from oracle import edm as E
from oracle import unet1d as O
from oracle import unet1d_sweep as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TIGHT = 5e-5            # tests/test_gpu_parity.py
GOLDEN_BOUND = 2e-5          # oracle/gen_golden_unet1d_io.py
IO = SW.IO_CASES
EPILOGUE_CASES = ("k3s1", "k9s3", "k12s4", "k16s4n128", "k8s2n160")      # tests/test_unet1d_io_gpu.py, c and d
LABEL_CASES = ("c24", "c40", "c320")


@pytest.fixture(scope="module")
def io_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "unet1d_io_golden.npz"))


@pytest.mark.parametrize("cid", list(IO))
def test_oracle_matches_the_reference_fixture_at_every_io_case(io_golden, cid):
    """tests/golden/unet1d_io_golden.npz holds what the reference ``UNet1dBase`` itself computed: the output whole, every hooked block output strided, and for
    a class-conditional case the output with every label dropped."""
    g = io_golden
    cfg, shape, seed, _ = IO[cid]
    x, t = SW.inputs(cfg, shape, seed)
    cl = SW.labels(cfg, shape[0])
    assert np.array_equal(g[f"{cid}_x"], x.numpy()) and np.array_equal(g[f"{cid}_t"], t.numpy())       # the fixture's inputs are the case's
    taps = {}
    w = SW.weights(cid, IO)[0]
    with torch.no_grad():
        y = O.unet1d_forward(w, cfg, x, t, taps=taps, classes=cl)
    stride = int(g[f"{cid}_stride"][0])
    names = [k[len(cid) + 5:] for k in g.files if k.startswith(f"{cid}_tap_")]
    assert sorted(names) == sorted(k for k in taps if not k.endswith(".h1")) and "to_in" in names
    assert g[f"{cid}_y"].shape == (shape[0], cfg.in_channels, shape[1])
    errs = {"out": SW.rel(y, torch.from_numpy(g[f"{cid}_y"]))}
    if cl is not None:
        assert np.array_equal(g[f"{cid}_classes"], cl.numpy()) and int(cl.min()) == 0 and int(cl.max()) == cfg.num_classes - 1 and "class_emb" in names
        with torch.no_grad():
            errs["out_null"] = SW.rel(O.unet1d_forward(w, cfg, x, t, classes=cl, cond_drop_prob=1.0), torch.from_numpy(g[f"{cid}_y_null"]))
        assert SW.rel(torch.from_numpy(g[f"{cid}_y_null"]), torch.from_numpy(g[f"{cid}_y"])) > 1e-2          # the labels matter
    for k in names:
        ref = torch.from_numpy(g[f"{cid}_tap_{k}"])
        got = taps[k].reshape(taps[k].shape[0], -1)[:, ::stride]
        assert got.shape == ref.shape and float(ref.abs().max()) > 1e-3, k
        errs[k] = SW.rel(got, ref)
    worst = max(errs, key=errs.get)
    print(cid, "worst", worst, errs[worst], "out", errs["out"])
    assert errs[worst] < GOLDEN_BOUND, (worst, errs[worst])


def test_the_fixture_is_no_larger_than_the_sweep_fixture():
    gold = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(gold, "unet1d_io_golden.npz")) <= os.path.getsize(os.path.join(gold, "unet1d_sweep_golden.npz"))


@pytest.mark.parametrize("cid", list(IO))
def test_fp32_oracle_within_a_quarter_of_the_bar_of_the_float64_oracle(cid):
    cfg, shape, seed, _ = IO[cid]
    y64, t64, dist = SW.float64_case(cid, IO)
    assert y64.shape == (shape[0], cfg.out_channels, shape[1]) and "to_in" in t64 and ("class_emb" in t64) == cfg.class_cond
    worst = max(dist, key=dist.get)
    print(cid, "tensors", len(dist), "worst fp32-vs-float64", worst, dist[worst], "out", dist["out"])
    over = [(k, d) for k, d in dist.items() if not d <= FP32_TIGHT / 4]
    assert not over, over[:5]
    assert all(float(v.abs().max()) > 1e-3 for v in t64.values())              # nothing compared is (near) zero


def test_every_io_case_passes_validate_device_and_constructs_in_its_modes():
    for cid, (cfg, shape, _, modes) in IO.items():
        assert shape[1] % cfg.total_downsample == 0 and cfg.num_layers == 1 and not any(cfg.attentions) and not cfg.use_attention_bottleneck, cid
        assert cfg.num_filters == cfg.channels * cfg.multipliers[0] and cfg.out_channels == cfg.in_channels, cid
        for dtype in modes:
            cfg.validate_device(dtype)
            net = A.UNet1dBase.from_config(cfg, compute_dtype=dtype)
            assert net.cfg.out_channels == cfg.in_channels and set(net.state_dict()) == set(generate_weights(cfg, 0)), cid
    assert set(EPILOGUE_CASES) | set(LABEL_CASES) <= set(IO)


# ------------------------------------------------------------------ which kernel a case reaches
def to_in_kernel(cfg: UNet1dConfig, mode: str, length: int) -> str:
    """launch_to_in's gate (csrc/adf_kernels.hip) in the terms of validate_device's ``fast_in``: the row form serves one waveform channel at window 8 /
    stride 2 with a power-of-two number of 16-byte chunks per row and L % 4 == 0; everything else is the general kernel."""
    epc = 8 if mode == "bf16" else 4
    cpr = cfg.num_filters // epc
    pad = cfg.window_length // 2 - cfg.stride // 2
    rows = cfg.in_channels == 1 and cfg.window_length == 8 and cfg.stride == 2 and 0 <= pad <= 4 and length % 4 == 0 and cpr <= 256 and cpr & (cpr - 1) == 0
    return "rows" if rows else "general"


def to_out_kernel(cfg: UNet1dConfig, mode: str):
    """launch_to_out's gates in the terms of validate_device's ``mfma_out``: bf16 with a multiple of 16 filters up to 128 is the MFMA kernel (staged through
    LDS at exactly 64 filters, else direct from global memory, num_filters / 16 K steps); f32x3 with 64 or 128 filters the split kernel; else the general one."""
    nf = cfg.num_filters
    if mode == "bf16" and nf % 16 == 0 and nf <= 128:
        return ("mfma_staged" if nf == 64 else "mfma_direct", nf // 16)
    if mode == "f32x3" and nf % 64 == 0 and nf <= 128:
        assert O.x3_to_out(nf)
        return ("x3", nf)
    assert not (mode == "f32x3" and O.x3_to_out(nf))
    return ("general", mode)


def reach_table():
    return {(cid, m): (to_in_kernel(cfg, m, shape[1]), to_out_kernel(cfg, m)) for cid, (cfg, shape, _, modes) in IO.items() for m in modes}


def test_the_cases_reach_every_transform_kernel_and_form():
    tab = reach_table()
    for (cid, m), v in tab.items():
        print(f"{cid:10s} {m:6s} to_in {v[0]:8s} to_out {v[1]}")
    ins = {v[0] for v in tab.values()}
    outs = {v[1] for v in tab.values()}
    assert ins == {"rows", "general"}
    assert {("general", "bf16"), ("general", "f32x3"), ("general", "fp32"), ("mfma_staged", 4), ("mfma_direct", 6), ("mfma_direct", 8), ("x3", 64), ("x3", 128)} <= outs
    # the cases the table of the issue names for a form really take it
    assert tab[("k12s4", "bf16")][1] == ("mfma_staged", 4) and tab[("k8s2st", "bf16")] == ("general", ("mfma_staged", 4))
    assert tab[("k16s4n128", "bf16")][1] == tab[("k8s2n128", "bf16")][1] == ("mfma_direct", 8) and tab[("k8s2n96", "bf16")][1] == ("mfma_direct", 6)
    assert tab[("k8s2n96", "f32x3")][1] == ("general", "f32x3") and all(tab[("k8s2n160", m)][1] == ("general", m) for m in SW.ALL3)
    assert tab[("k16s4n128", "f32x3")][1] == tab[("k8s2n128", "f32x3")][1] == ("x3", 128) and tab[("k12s4", "f32x3")][1] == tab[("k8s2st", "f32x3")][1] == ("x3", 64)
    assert all(tab[("k8s2n128", m)][0] == "rows" for m in SW.ALL3) and all(tab[("k8s2n96", m)][0] == "general" for m in SW.ALL3)
    assert all(tab[("k8s2st", m)][0] == "general" for m in SW.ALL3)                  # two waveform channels at the shipped width
    # to_out's block geometry: feature rows, blocks of 256 and the rows of the last block against the halo
    geo = {cid: (shape[1] // cfg.stride, -(-cfg.window_length // cfg.stride)) for cid, (cfg, shape, _, _) in IO.items()}
    assert geo["k3s1"] == (556, 3) and geo["k4s2"] == (522, 2) and geo["k16s2"] == (258, 8) and geo["k8s8"] == (262, 1) and geo["k9s3"] == (516, 3)
    assert geo["k12s4"] == (296, 3) and geo["k16s4n128"] == (520, 4) and geo["k16s2"][0] - 256 < geo["k16s2"][1]       # a last block shorter than the halo
    assert IO["k8s8"][0].window_length // 2 - IO["k8s8"][0].stride // 2 == 0                                            # pad 0


X3_OUT = ("k12s4", "k16s4n128", "k8s2n128", "k8s2st")


@pytest.mark.parametrize("cid", X3_OUT)
def test_a_truncating_split_leaves_twice_the_launch_bar_on_the_output(cid):
    """What tests/test_oracle_unet1d_x3.py derives over CASES, on ``out`` of the I/O cases whose to_out is the split kernel: the emulation's own tensors forced
    into the emulation and into its truncating variant."""
    cfg, shape, seed, _ = IO[cid]
    assert O.x3_to_out(cfg.num_filters) and {c for c, v in IO.items() if O.x3_to_out(v[0].num_filters) and "f32x3" in v[3]} == set(X3_OUT)
    w64 = SW.weights(cid, IO)[1]
    x, t = SW.inputs(cfg, shape, seed)
    _, taps = SW.x3_case(cid, IO)
    force = {k: v.float() for k, v in taps.items()}
    assert "out" in SW.x3_gemm_fed(cfg, taps)
    with torch.no_grad():
        base, trunc, sum32 = (O.unet1d_forward(w64, cfg, x.double(), t.double(), force=force, storage="f32x3" + v) for v in ("", ":trunc", ":sum_fp32"))
    fig, fig32 = O.rel_l2(trunc, base), O.rel_l2(sum32, base)
    print(cid, "truncating split on out", f"{fig:.2e}", "fp32-summed", f"{fig32:.2e}", "bar", SW.X3_LAUNCH_TOL)
    assert fig > 2 * SW.X3_LAUNCH_TOL and fig32 < SW.X3_LAUNCH_TOL / 2


@pytest.mark.parametrize("cid", EPILOGUE_CASES + ("k8s8", "k8s2n128"))
def test_the_denoise_inputs_clamp_a_good_part_of_every_sample(cid):
    """The condition of the epilogue tests of the GPU module, on the float64 oracle: between 10 % and 80 % of every sample lies on the clamp."""
    cfg, shape, seed, _ = IO[cid]
    x, sig = SW.denoise_inputs(cfg, shape, seed)
    with torch.no_grad():
        d = E.make_denoiser(SW.weights(cid, IO)[1], cfg, 1.0)(x.double(), sigmas=sig)
    assert d.dtype == torch.float64
    share = (d.abs() >= 1).double().mean(dim=(1, 2))
    print(cid, "clamped share per sample", [round(float(s), 3) for s in share])
    assert bool(((share > 0.1) & (share < 0.8)).all()), share


def test_the_float64_denoiser_follows_the_dtype_of_its_input():
    cfg, shape, seed, _ = IO["k4s2"]
    x, sig = SW.denoise_inputs(cfg, shape, seed)
    w, w64 = SW.weights("k4s2", IO)
    with torch.no_grad():
        d32 = E.make_denoiser(w, cfg, 1.0)(x, sigmas=sig)
        d64 = E.make_denoiser(w64, cfg, 1.0)(x.double(), sigmas=sig)
        s64 = E.make_denoiser(w64, cfg, 1.0)(x.double(), sigma=3.0)
    assert d32.dtype == torch.float32 and d64.dtype == s64.dtype == torch.float64 and SW.rel(d32, d64) < FP32_TIGHT / 4
    assert SW.rel(s64[1], d64[1]) < 1e-12 and SW.rel(s64[0], d64[0]) > 1e-2


# ------------------------------------------------------------------ what the reference cannot run is refused at construction
def _mk(dtype="fp32", **kw):
    base = dict(channels=16, num_filters=16, multipliers=[1, 2], factors=[2], num_blocks=[1], attentions=[False], use_attention_bottleneck=False)
    base.update(kw)
    return A.UNet1dBase(compute_dtype=dtype, **base)


def test_windows_and_strides_the_reference_cannot_run_are_refused_with_the_transforms_named():
    for wl, st in ((6, 3), (7, 2), (8, 3)):                                     # 2 * pad != window - stride: the reference returns L - 1 or L + 1 samples
        with pytest.raises(ValueError, match=rf"unet\.to_in / unet\.to_out: window_length = {wl} and stride = {st} of different parity"):
            _mk(window_length=wl, stride=st)
    _mk(window_length=6, stride=2), _mk(window_length=7, stride=3), _mk(window_length=9, stride=3)
    with pytest.raises(ValueError, match=r"unet\.to_in / unet\.to_out: stride = 6 above window_length = 4"):
        _mk(window_length=4, stride=6)
    _mk(window_length=4, stride=4)                                              # stride == window: pad 0
    with pytest.raises(ValueError, match=r"unet\.to_in / unet\.to_out: stride must be at least 1, got 0"):
        _mk(window_length=4, stride=0)
    with pytest.raises(ValueError, match=r"unet\.to_in / unet\.to_out: stride must be at least 1, got -2"):
        _mk(window_length=4, stride=-2)
    _mk(window_length=3, stride=1)
    for dtype in ("fp32", "bf16", "f32x3"):
        with pytest.raises(ValueError, match=r"unet\.to_in / unet\.to_out"):
            UNet1dConfig(window_length=8, stride=3).validate_device(dtype)


def test_the_reference_itself_loses_or_gains_a_sample_at_mixed_parity():
    """Why the rule: the oracle (as the reference's ConvTranspose1d) gives 119 samples for 120 at 6 / 3 and 81 for 80 at 7 / 2, where to_in gives 39 rows."""
    import torch.nn.functional as F
    for wl, st, l, rows, want in ((6, 3, 120, 40, 119), (7, 2, 80, 39, 81), (8, 2, 80, 40, 80), (9, 3, 120, 40, 120)):
        pad = wl // 2 - st // 2                                                  # oracle/unet1d.py, as unet1d.py:584-591 and :611-622
        assert F.conv1d(torch.zeros(1, 1, l), torch.zeros(4, 1, wl), stride=st, padding=pad).shape[-1] == rows
        assert F.conv_transpose1d(torch.zeros(1, 4, l // st), torch.zeros(4, 1, wl), stride=st, padding=pad).shape[-1] == want
    with pytest.raises(RuntimeError, match="negative padding"):
        F.conv1d(torch.zeros(1, 1, 24), torch.zeros(4, 1, 4), stride=6, padding=4 // 2 - 6 // 2)


def test_a_class_conditional_net_wider_than_the_label_kernel_is_refused_at_construction():
    kw = dict(multipliers=[1, 1], resnet_groups=8, class_cond=True, num_classes=3)
    with pytest.raises(ValueError, match=r"label_conditioner: a class-conditional net of up to 512 channels is served \(launch_class_embed\), got 516"):
        _mk(channels=516, num_filters=516, **kw)
    _mk(channels=512, num_filters=512, **kw)
    _mk(channels=516, num_filters=516, multipliers=[1, 1], resnet_groups=4)      # unconditional: no label kernel
