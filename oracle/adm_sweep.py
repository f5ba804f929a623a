"""The constructor and shape sweep of the ADM UNetModel (test infrastructure, see oracle/__init__.py): the configurations that
tests/test_oracle_adm_sweep.py and tests/test_adm_sweep_gpu.py share, their inputs and the float64 run of oracle/unet2d_oai.py they are held to.

S = ``config_c4_small`` (image_size 32, one input / output channel, widths 32 / 64, one res block, attention at the second level and in the middle, 2
heads, scale-shift conditioning, conv resampling); every case names what it changes.  The rest of the suite only ever builds S, a one-argument change of
it, or the full ``config_c4`` at 1 x 80 x 256.  Every image here has a coarsest level that is a multiple of 64 pixels (AdmNet::check_image).

  lv3        three levels, widths 32 / 64 / 96, two res blocks, 3 heads of 32 channels at the third level, fine statistics group 1; 512 and 128 tokens
  updown_ss  ResBlock(up / down=True) with the default scale-shift conditioning (the only other updown fixture is additive); head dim 64
  pool_hd8   AvgPool2d / nearest interpolation (AdmLayer kinds 5 / 6) right after an attention block; attention at level 0 (1024 tokens); head dim 8; B = 1
  one_level  one channel_mult entry: no resampling layer at all; one 64-pixel image per sample, 5 samples
  io43       4 input channels (conv2d_in_kernel<T, 0>: weights read from LDS per use), 3 output channels (launch_conv2d_out's 4 x 32 tiles), 7 labels with
             additive conditioning (per-sample bias rows), width 96 / 192; B = 7.  Run with the labels kept and dropped (cond_drop_prob 1)
  flat       4 x 64 image: level 1 is 2 x 32, ONE t2 tile per image whose every row is a border row; head dim 16
  tall       64 x 4 image: W = 4 and 2, every 3x3 conv on the gather kernel, 2-pixel-wide pooling source and upsampling target
  mult21     channel_mult (2, 1): the net narrows with depth (64 -> 32 and back), three res blocks per level, new attention order at head dim 16
  odd_h      3 x 64 image, one level: odd H declines the spatial tiles although W % 32 == 0
  one_row    1 x 64 image, one level: every vertical tap of every 3x3 conv lies outside the image
``lv3`` runs a second shape on the same handle (2 x 16 x 64).  bf16 needs widths that are multiples of 64: ``updown_ss`` and ``one_level`` as they are, and
the 64-wide variants ``flat_w64`` / ``lv3_w64`` (widths 64 / 128 and 64 / 128 / 192).  No case of the proposal was replaced."""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import torch

from audiodiffuser_amd.adm_config import ADMConfig, config_c4_small, generate_weights

# id -> (changes over config_c4_small, (B, H, W), weight seed)
CASES: Dict[str, Tuple[dict, Tuple[int, int, int], int]] = {
    "lv3": (dict(channel_mult=(1, 2, 3), num_res_blocks=2, attention_resolutions="16,8", num_head_channels=32), (3, 32, 64), 61),
    "updown_ss": (dict(model_channels=64, resblock_updown=True, num_head_channels=64), (2, 16, 32), 62),
    "pool_hd8": (dict(conv_resample=False, channel_mult=(1, 1, 2), attention_resolutions="32,16,8", num_head_channels=8), (1, 32, 32), 63),
    "one_level": (dict(model_channels=64, channel_mult=(1,), num_heads=1), (5, 8, 8), 64),
    "io43": (dict(in_channels=4, out_channels=3, num_classes=7, use_scale_shift_norm=False, model_channels=96, num_head_channels=32), (7, 16, 16), 65),
    "flat": (dict(num_heads=4), (2, 4, 64), 66),
    "tall": (dict(num_heads=4), (2, 64, 4), 67),
    "mult21": (dict(channel_mult=(2, 1), num_res_blocks=3, num_head_channels=16, use_new_attention_order=True), (3, 16, 16), 68),
    "odd_h": (dict(channel_mult=(1,), num_heads=1), (3, 3, 64), 69),
    "one_row": (dict(channel_mult=(1,), model_channels=64, num_heads=1), (2, 1, 64), 70),
    # the 64-wide variants of the bf16 runs
    "flat_w64": (dict(model_channels=64, num_heads=4), (2, 4, 64), 71),
    "lv3_w64": (dict(model_channels=64, channel_mult=(1, 2, 3), num_res_blocks=2, attention_resolutions="16,8", num_head_channels=32), (3, 32, 64), 72),
}
FP32_CASES = ("lv3", "updown_ss", "pool_hd8", "one_level", "io43", "flat", "tall", "mult21", "odd_h", "one_row")
BF16_CASES = ("updown_ss", "one_level", "flat_w64", "lv3_w64")

# run id -> (case, (B, H, W), input seed, cond_drop_prob): the twelve fp32 / f32x3 runs.  The runs of one case share a handle, in this order
RUNS: Dict[str, Tuple[str, Tuple[int, int, int], int, float]] = {cid: (cid, CASES[cid][1], CASES[cid][2], 0.0) for cid in FP32_CASES}
RUNS["io43_dropped"] = ("io43", CASES["io43"][1], CASES["io43"][2], 1.0)
RUNS["lv3_16x64"] = ("lv3", (2, 16, 64), 73, 0.0)
# one handle through four shapes, returning to the first (lv3's structure; the third has a 2 x 32 coarsest level)
FOUR_SHAPES = (("lv3", (3, 32, 64)), ("lv3", (2, 16, 64)), ("lv3", (1, 8, 128)), ("lv3", (3, 32, 64)))

FP32_TIGHT = 5e-5            # tests/test_adm.py: the project's exact-fp32 bar


def runs_of(cid: str):
    return [rid for rid, r in RUNS.items() if r[0] == cid]


def config(cid: str) -> ADMConfig:
    return ADMConfig(**{**config_c4_small().to_kwargs(), **CASES[cid][0]})


def inputs(cfg: ADMConfig, shape, seed: int = 0):
    """x [B, in_channels, H, W] = 0.5 randn, one time per sample in [-1.3, 0.9] (c_noise of the EDM wrapper lies in about [-1.6, 1.1]), one label per sample
    where the net has classes (as tests/test_unet2d_sweep_gpu.py; the label stride 3 visits every one of 7 classes)."""
    b, h, w = shape
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(b, cfg.in_channels, h, w, generator=g) * 0.5
    t = torch.linspace(-1.3, 0.9, b) if b > 1 else torch.tensor([0.35])
    cl = (torch.arange(b) * 3 + 2) % cfg.num_classes if cfg.num_classes else None
    return x, t, cl


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a - b| / max |b| in float64: the metric of the fp32 bars (tests/test_adm.py rel)."""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def bar_of(d: float) -> float:
    """FP32_TIGHT, or 4 x the tensor's own fp32-oracle-vs-float64-oracle distance where that exceeds a quarter of it (tests/test_unet2d_sweep_gpu.py)."""
    return FP32_TIGHT if d <= FP32_TIGHT / 4 else 4.0 * d


@functools.lru_cache(maxsize=None)
def weights(cid: str):
    w = generate_weights(config(cid), seed=CASES[cid][2])
    return w, {k: v.double() for k, v in w.items()}


def float64_run(cfg: ADMConfig, w, w64, x, t, cl: Optional[torch.Tensor] = None, cdp: float = 0.0):
    """-> (float64 output, {name: float64 tensor} for every name the oracle records, {name: fp32-oracle-vs-float64-oracle distance} with "out")."""
    from oracle import unet2d_oai as O
    t32, t64 = {}, {}
    with torch.no_grad():
        y32 = O.unet2d_forward(w, cfg, x, t, classes=cl, cond_drop_prob=cdp, taps=t32)
        y64 = O.unet2d_forward(w64, cfg, x.double(), t.double(), classes=cl, cond_drop_prob=cdp, taps=t64)
    assert y32.dtype == torch.float32 and all(v.dtype == torch.float32 for v in t32.values())
    assert y64.dtype == torch.float64 and all(v.dtype == torch.float64 for v in t64.values()) and list(t32) == list(t64)
    dist = {k: rel(t32[k], t64[k]) for k in t64}
    dist["out"] = rel(y32, y64)
    return y64, t64, dist


@functools.lru_cache(maxsize=None)
def float64_shape(cid: str, shape, seed: int, cdp: float = 0.0):
    """``float64_run`` of a case's structure at one shape, computed once per session and left unchanged."""
    cfg = config(cid)
    w, w64 = weights(cid)
    x, t, cl = inputs(cfg, shape, seed)
    return float64_run(cfg, w, w64, x, t, cl, cdp)


def float64_case(rid: str):
    cid, shape, seed, cdp = RUNS[rid]
    return float64_shape(cid, shape, seed, cdp)
