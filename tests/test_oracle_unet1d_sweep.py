"""CPU side of the 1-D U-Net sweep (oracle/unet1d_sweep.py): the oracle is pinned to the reference at every sweep configuration, not only at the
presets; its float64 run is the reference of tests/test_unet1d_sweep_gpu.py, so the fp32 run must sit well inside that module's bar of it; and the
constructor refuses, with the layer named, what the HIP library cannot serve (it used to be refused at the first forward)."""
import os

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd.config import PRESETS, UNet1dConfig
from audiodiffuser_amd.weights import generate_weights
from oracle import unet1d as O
from oracle import unet1d_sweep as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TIGHT = 5e-5            # tests/test_gpu_parity.py
GOLDEN_BOUND = 2e-5          # oracle/gen_golden_unet1d_sweep.py


@pytest.fixture(scope="module")
def sweep_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "unet1d_sweep_golden.npz"))


@pytest.mark.parametrize("cid", list(SW.CASES))
def test_oracle_matches_the_reference_fixture_at_every_sweep_configuration(sweep_golden, cid):
    """tests/golden/unet1d_sweep_golden.npz holds what the reference ``UNet1dBase`` itself computed: the output and every hooked block output (strided)."""
    g = sweep_golden
    cfg, shape, seed, _ = SW.CASES[cid]
    x, t = SW.inputs(cfg, shape, seed)
    assert np.array_equal(g[f"{cid}_x"], x.numpy()) and np.array_equal(g[f"{cid}_t"], t.numpy())       # the fixture's inputs are the sweep's
    taps = {}
    with torch.no_grad():
        y = O.unet1d_forward(generate_weights(cfg, seed=seed), cfg, x, t, taps=taps)
    stride = int(g[f"{cid}_stride"][0])
    names = [k[len(cid) + 5:] for k in g.files if k.startswith(f"{cid}_tap_")]
    # every module boundary of the net: to_in, temb, each conv / block / transformer (.h1 and .attn.<x> are inside a module)
    assert sorted(names) == sorted(k for k in taps if not k.endswith(".h1") and ".attn." not in k)
    errs = {"out": SW.rel(y, torch.from_numpy(g[f"{cid}_y"]))}
    for k in names:
        ref = torch.from_numpy(g[f"{cid}_tap_{k}"])
        got = taps[k].reshape(taps[k].shape[0], -1)[:, ::stride]
        assert got.shape == ref.shape and float(ref.abs().max()) > 1e-3, k
        errs[k] = SW.rel(got, ref)
    worst = max(errs, key=errs.get)
    print(cid, "worst", worst, errs[worst], "out", errs["out"])
    assert errs[worst] < GOLDEN_BOUND, (worst, errs[worst])


@pytest.mark.parametrize("cid", list(SW.CASES))
def test_fp32_oracle_within_a_quarter_of_the_bar_of_the_float64_oracle(cid):
    """Output and every recorded tensor.  Behaviour on float32 inputs is unchanged by the float64 option: the float32 run returns float32."""
    cfg, shape, seed, _ = SW.CASES[cid]
    y64, t64, dist = SW.float64_case(cid)
    assert y64.shape == (shape[0], cfg.out_channels, shape[1])
    x, t = SW.inputs(cfg, shape, seed)
    with torch.no_grad():
        assert O.unet1d_forward(SW.weights(cid)[0], cfg, x, t).dtype == torch.float32
    worst = max(dist, key=dist.get)
    print(cid, "tensors", len(dist), "worst fp32-vs-float64", worst, dist[worst], "out", dist["out"])
    over = [(k, d) for k, d in dist.items() if not d <= FP32_TIGHT / 4]
    assert not over, over[:5]
    assert all(float(v.abs().max()) > 1e-3 for v in t64.values())              # nothing compared is (near) zero
    with pytest.raises(ValueError, match="bf16-storage oracle runs on float32"):
        O.unet1d_forward(SW.weights(cid)[1], cfg, x.double(), t.double(), storage="bf16")


def _mk(dtype="fp32", **kw):
    base = dict(channels=16, num_filters=16, multipliers=[1, 2, 4, 4], factors=[2, 4, 4], num_blocks=[1, 2, 1], attentions=[False, True, True])
    base.update(kw)
    return A.UNet1dBase(compute_dtype=dtype, **base)


def test_what_the_library_cannot_serve_is_refused_at_construction_with_the_layer_named():
    with pytest.raises(ValueError, match=r"unet\.downsamples\.1\.transformer: the attention kernels serve a head dim of 8, 16, 32 or 64; 192 channels in 8 heads"):
        _mk(channels=48, num_filters=48)                                        # head dim 24
    with pytest.raises(ValueError, match=r"unet\.bottleneck\.transformer: the attention kernels serve a head dim of 8, 16, 32 or 64; 64 channels in 3 heads"):
        _mk(attention_heads=3, attentions=[False, False, False])                # heads that do not divide the width
    with pytest.raises(ValueError, match=r"unet\.downsamples\.1\.transformer: .* 512 channels in 4 heads"):
        _mk(channels=128, num_filters=128, attention_heads=4)                   # head dim 128
    with pytest.raises(ValueError, match=r"unet\.to_out: window_length up to 16 is served, got 32"):
        _mk(window_length=32, stride=8)
    with pytest.raises(ValueError, match=r"unet\.to_in: 12 channels; bf16 rows are stored in chunks of 8 channels"):
        _mk("bf16", channels=12, num_filters=12, attention_heads=3)
    _mk("fp32", channels=12, num_filters=12, attention_heads=3, resnet_groups=4)                  # 12 / 24 / 48 / 48: multiples of 4
    with pytest.raises(ValueError, match=r"unet\.to_in: 10 channels; f32x3 rows are stored in chunks of 4 channels"):
        _mk("f32x3", channels=10, num_filters=10)
    with pytest.raises(ValueError, match=r"unet\.downsamples\.0: resnet_groups = 5 does not divide its 32 channels \(GroupNorm\)"):
        _mk(resnet_groups=5)
    with pytest.raises(ValueError, match=r"unet\.downsamples\.0: resnet_groups up to 256 are served \(GroupNorm statistics\), got 512"):
        _mk(channels=512, num_filters=512, resnet_groups=512, attention_heads=16, multipliers=[1, 1, 1, 1])
    with pytest.raises(ValueError, match=r"unet\.downsamples\.0: resnet_groups = 8 does not divide its 36 channels"):
        _mk(channels=12, num_filters=12, multipliers=[1, 3, 4, 4], attention_heads=3)
    with pytest.raises(ValueError, match=r"unet\.downsamples\.1: 1280 channels are more than the 256 chunks of 4 channels a fp32 row may have"):
        _mk(channels=320, num_filters=320, attention_heads=20)
    UNet1dConfig(channels=320, num_filters=320, attention_heads=20, attention_multiplier=1, multipliers=[1, 2, 4, 4], factors=[2, 4, 4], num_blocks=[1, 2, 1],
                 attentions=[False, True, True]).validate_device("bf16")        # 160 chunks of 8 channels
    with pytest.raises(ValueError, match=r"unet\.downsamples\.1\.transformer\.feed_forward: 2048 channels \(attention_multiplier = 8\)"):
        _mk(channels=64, num_filters=64, attention_multiplier=8)
    with pytest.raises(NotImplementedError, match=r"unet\.upsamples\.1\.upsample \(and unet\.downsamples\.1\.downsample\): a factor of 1 is a plain Conv1d"):
        _mk(factors=[2, 1, 4])
    with pytest.raises(NotImplementedError, match="use_nearest_upsample=True with a factor of 1"):
        _mk(factors=[2, 1, 4], use_nearest_upsample=True)
    with pytest.raises(ValueError, match=r"unet\.to_in: num_filters \* in_channels \* window_length = 16384 weights"):
        _mk(channels=256, num_filters=256, multipliers=[1, 1, 1, 1], in_channels=4, window_length=16, stride=4)
    with pytest.raises(ValueError, match=r"unet\.to_out: num_filters \* window_length = 12800 weights and the tap products do not fit"):
        _mk(channels=800, num_filters=800, attention_heads=25, multipliers=[1, 1, 1, 1], attention_multiplier=1, window_length=16, stride=4)


def test_every_sweep_configuration_and_every_preset_constructs():
    for cid, (cfg, _, _, modes) in SW.CASES.items():
        for dtype in modes:
            net = A.UNet1dBase.from_config(cfg, compute_dtype=dtype)
            assert net.cfg.out_channels == cfg.in_channels and set(net.state_dict()) == set(generate_weights(cfg, 0)), cid
    for mk in PRESETS.values():
        for dtype in ("fp32", "bf16", "f32x3"):
            A.UNet1dBase.from_config(mk(), compute_dtype=dtype)
    UNet1dConfig().validate_device("bf16")
