"""The constructor and shape sweep of the 1-D U-Net (test infrastructure, see oracle/__init__.py): the configurations that
tests/test_unet1d_sweep_gpu.py, tests/test_oracle_unet1d_sweep.py and oracle/gen_golden_unet1d_sweep.py share.

T = ``config_tiny``'s structure (multipliers [1, 2, 4, 4], factors [2, 4, 4], blocks [1, 2, 1], attentions [F, T, T], total downsample 64); every
case names what it changes.  The presets only ever use channels 16 / 64, 8 heads at head dim 32, 8 groups, kernel multiplier 2, factors 2 and 4,
window 8 / stride 2 / one waveform channel, the scaled skip and the bottleneck transformer.

f83: the 32-channel attention level has head dim 4 with the default 8 heads, which no attention kernel serves (the constructor refuses it), so the
case runs 4 heads (head dim 8, which no other case or preset has).

IO_CASES: a second table of the same layout on the smallest net that reaches the waveform transforms (to_in / to_out), the denoise epilogue and the label
path, which CASES leave at window 8 / stride 2 / one channel / 16 or 64 filters.  ``weights`` / ``float64_case`` / ``x3_case`` take the table as their
second argument (default CASES)."""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from audiodiffuser_amd.config import UNet1dConfig
from audiodiffuser_amd.weights import generate_noise, generate_weights


def _t(channels, **kw) -> UNet1dConfig:
    base = dict(channels=channels, num_filters=channels, multipliers=[1, 2, 4, 4], factors=[2, 4, 4], num_blocks=[1, 2, 1],
                attentions=[False, True, True])
    base.update(kw)
    cfg = UNet1dConfig(**base)
    cfg.out_channels = cfg.in_channels          # unet1d.py:607
    return cfg


# id -> (configuration, (B, L), weight seed, compute modes)
CASES: Dict[str, Tuple[UNet1dConfig, Tuple[int, int], int, Tuple[str, ...]]] = {
    "w24": (_t(24, attention_heads=3), (2, 448), 31, ("fp32", "bf16", "f32x3")),
    "w48": (_t(48, attention_heads=6), (3, 512), 32, ("fp32", "bf16", "f32x3")),
    "w32": (_t(32), (3, 512), 33, ("fp32", "bf16", "f32x3")),
    "h64": (_t(64, attention_heads=4), (3, 1024), 34, ("fp32", "bf16", "f32x3")),
    "h2": (_t(16, attention_heads=2), (2, 320), 35, ("fp32", "bf16", "f32x3")),
    "g1": (_t(16, resnet_groups=1), (2, 320), 36, ("fp32", "bf16", "f32x3")),
    "g16": (_t(32, resnet_groups=16), (2, 320), 37, ("fp32", "bf16", "f32x3")),
    # odd group counts at lengths whose levels (256 / 128 / 32 / 8) include the short ones (<= 32 rows, a power of two: gn_norm_apply): a group of the skip
    # concat lies across both sources -- the only group (g1s), or the middle one of three (g3s: widths 48 / 96, groups of 16 / 32 channels, 32 / 64 over a concat)
    "g1s": (_t(16, resnet_groups=1), (2, 512), 41, ("fp32", "bf16", "f32x3")),
    "g3s": (_t(24, resnet_groups=3, attention_heads=3), (2, 512), 42, ("fp32", "bf16", "f32x3")),
    "km4": (_t(16, kernel_multiplier_downsample=4), (2, 576), 38, ("fp32", "bf16", "f32x3")),
    "f83": (_t(16, multipliers=[1, 2, 4], factors=[8, 3], num_blocks=[3, 1], attentions=[True, False], use_skip_scale=False,
               use_attention_bottleneck=False, attention_multiplier=4, attention_heads=4), (3, 432), 39, ("fp32", "bf16", "f32x3")),
    "win16": (_t(16, num_filters=32, multipliers=[2, 2, 4], factors=[2, 2], num_blocks=[1, 1], attentions=[False, True], window_length=16,
                 stride=4, in_channels=2, attention_multiplier=1), (2, 176), 40, ("fp32", "bf16", "f32x3")),
}


def _io(channels, m0=1, **kw) -> UNet1dConfig:
    """The smallest net that reaches the waveform transforms: one level of one block, no attention, no bottleneck transformer."""
    return _t(channels, num_filters=channels * m0, multipliers=[m0, 2], factors=[2], num_blocks=[1], attentions=[False], use_attention_bottleneck=False, **kw)


def _cc(channels, num_classes) -> UNet1dConfig:
    return _io(channels, class_cond=True, num_classes=num_classes)


ALL3 = ("fp32", "bf16", "f32x3")
# The waveform transforms, the denoise epilogue and the label path off the preset point (tests/test_unet1d_io_gpu.py, tests/test_oracle_unet1d_io.py,
# oracle/gen_golden_unet1d_io.py); same layout as CASES.  to_out works in blocks of 256 feature rows (L / stride) with a halo of ceil(window / stride) rows.
IO_CASES: Dict[str, Tuple[UNet1dConfig, Tuple[int, int], int, Tuple[str, ...]]] = {
    "k3s1": (_io(16, window_length=3, stride=1, in_channels=4), (2, 556), 51, ALL3),          # stride 1; 556 rows: three blocks, the last of 44
    "k4s2": (_io(16, window_length=4, stride=2), (2, 1044), 52, ALL3),                          # 522 rows: last block of 10
    "k16s2": (_io(16, window_length=16, stride=2, in_channels=2), (2, 516), 53, ALL3),         # halo 8, 258 rows: a second block of 2 rows; 8 taps per output
    "k8s8": (_io(16, window_length=8, stride=8), (2, 2096), 54, ALL3),                          # pad 0, one tap per output, 2048 outputs per block
    "k9s3": (_io(16, window_length=9, stride=3, in_channels=2), (3, 1548), 55, ALL3),          # odd window and stride
    "k12s4": (_io(16, 4, window_length=12, stride=4), (2, 1184), 56, ALL3),                     # 64 filters off window 8: staged MFMA form, to_out_x3_kernel
    "k16s4n128": (_io(32, 4, window_length=16, stride=4, in_channels=2), (2, 2080), 57, ALL3),  # 128 filters: 8 K steps, the second 64-channel chunk of x3
    "k8s2n128": (_io(32, 4), (2, 1036), 58, ALL3),                                              # 128 filters at the shipped window; row form of to_in
    "k8s2n96": (_io(24, 4), (2, 524), 59, ALL3),                                                # direct MFMA form with 6 K steps; f32x3 on the general kernel
    "k8s2n160": (_io(40, 4), (2, 524), 60, ALL3),                                               # above 128 filters: the general to_out in every mode
    "k8s2st": (_io(64, in_channels=2), (2, 1036), 61, ALL3),                                    # stereo at the shipped width
    # class-conditional (labels from ``labels``: 0 and num_classes - 1 among them)
    "c24": (_cc(24, 5), (3, 512), 62, ALL3),
    "c40": (_cc(40, 7), (2, 512), 63, ALL3),
    "c320": (_cc(320, 3), (2, 256), 64, ("fp32", "bf16")),                                      # the second stride trip of class_embed_kernel (320 > 256 threads)
}


# The bar of the split-bf16 mode per launch (relative L2 of one teacher-forced tensor against oracle/unet1d.py storage="f32x3", and of the output): half the
# smallest figure a TRUNCATING hi / lo split leaves on any GEMM-fed tensor of the twelve cases (5.7e-6: g16 mid.post, a conv whose identity residual dilutes
# it most), ~7x the worst figure of the same three products summed in fp32 (4.2e-7).  Derived from the oracle alone and re-derived by
# tests/test_oracle_unet1d_x3.py; never fitted to what a device run gives.
X3_LAUNCH_TOL = 2.8e-6


def x3_gemm_fed(cfg: UNet1dConfig, taps) -> list:
    """The recorded names (plus "out") whose tensor a split-bf16 product of the device writes directly: everything but to_in, the embeddings, the three
    LayerNorm outputs of a transformer, an ``.att`` of the fp32 vector kernel and an output of the fp32 to_out kernel."""
    from oracle import unet1d as O
    fed = []
    for k, v in taps.items():
        if k in ("to_in", "temb", "class_emb") or k.endswith((".ln", ".n1", ".n2")):
            continue
        if k.endswith(".att") and not O.x3_attention(v.shape[1] // cfg.attention_heads, v.shape[2], v.shape[1]):
            continue
        fed.append(k)
    return fed + (["out"] if O.x3_to_out(cfg.num_filters) else [])


def inputs(cfg: UNet1dConfig, shape, seed: int = 0):
    """x [B, in_channels, L] and one time per sample (c_noise of the EDM wrapper lies in about [-1.6, 1.1])."""
    b, l = shape
    x = generate_noise(5000 + 17 * seed, b, l, channels=cfg.in_channels) * 0.7
    t = torch.linspace(-1.3, 0.9, b) if b > 1 else torch.tensor([0.35])
    return x, t


def denoise_inputs(cfg: UNet1dConfig, shape, seed: int = 0):
    """x_noisy [B, in_channels, L] = unit noise * sqrt(sigma^2 + 1) and one sigma per sample, (0.05, 3.0) or (0.05, 1.0, 3.0) at B = 3: at sigma_data = 1 the
    estimate is near x at the small sigma and near the net's output at the large one, and a good part of either lies beyond the clamp."""
    b, l = shape
    sig = torch.tensor([0.05, 3.0] if b == 2 else [0.05, 1.0, 3.0][:b])
    noise = generate_noise(7000 + 17 * seed, b, l, channels=cfg.in_channels)
    return noise * (sig ** 2 + 1).sqrt().view(b, 1, 1), sig


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a - b| / max |b| in float64: the metric of the fp32 bars (tests/gpu_helpers.py rel_err)."""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def labels(cfg: UNet1dConfig, b: int):
    """One label per sample for a class-conditional configuration, 0 and num_classes - 1 among them (None for an unconditional one)."""
    if not cfg.class_cond:
        return None
    return torch.tensor([(i * (cfg.num_classes - 1)) // max(b - 1, 1) for i in range(b)], dtype=torch.int64)


_CACHE: dict = {}


def _once(kind, cid, cases, make):
    """One result per (function, case of a table), computed once per session and shared by every test that needs it (the tables are module constants)."""
    key = (kind, id(cases), cid)
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def weights(cid: str, cases=None):
    cases = CASES if cases is None else cases
    cfg, _, seed, _ = cases[cid]

    def make():
        w = generate_weights(cfg, seed=seed)
        return w, {k: v.double() for k, v in w.items()}
    return _once("weights", cid, cases, make)


def float64_run(cfg, w, w64, x, t, classes=None, cond_drop_prob=0.0):
    """-> (float64 output, {name: float64 tensor} for every name the oracle records, {name: fp32-oracle-vs-float64-oracle distance} with "out")."""
    from oracle import unet1d as O
    t32, t64 = {}, {}
    with torch.no_grad():
        y32 = O.unet1d_forward(w, cfg, x, t, taps=t32, classes=classes, cond_drop_prob=cond_drop_prob)
        y64 = O.unet1d_forward(w64, cfg, x.double(), t.double(), taps=t64, classes=classes, cond_drop_prob=cond_drop_prob)
    assert y64.dtype == torch.float64 and all(v.dtype == torch.float64 for v in t64.values()) and list(t32) == list(t64)
    dist = {k: rel(t32[k], t64[k]) for k in t64}
    dist["out"] = rel(y32, y64)
    return y64, t64, dist


def x3_case(cid: str, cases=None):
    """The free-running split-bf16 oracle of a case of ``cases`` (default CASES) on its own inputs: (float64 output, {name: float64 tensor}), computed
    once per session."""
    from oracle import unet1d as O
    cases = CASES if cases is None else cases
    cfg, shape, seed, _ = cases[cid]

    def make():
        x, t = inputs(cfg, shape, seed)
        taps = {}
        with torch.no_grad():
            y = O.unet1d_forward(weights(cid, cases)[1], cfg, x.double(), t.double(), taps=taps, storage="f32x3", classes=labels(cfg, shape[0]))
        return y, taps
    return _once("x3", cid, cases, make)


def float64_case(cid: str, cases=None):
    """``float64_run`` of a case of ``cases`` (default CASES) on its own inputs (and labels), computed once per session."""
    cases = CASES if cases is None else cases
    cfg, shape, seed, _ = cases[cid]

    def make():
        w, w64 = weights(cid, cases)
        x, t = inputs(cfg, shape, seed)
        return float64_run(cfg, w, w64, x, t, classes=labels(cfg, shape[0]))
    return _once("float64", cid, cases, make)
