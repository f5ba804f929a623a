"""The width and shape sweep of WaveNetNoise (test infrastructure, see oracle/__init__.py): the configurations that
tests/test_wavenet_sweep_gpu.py, tests/test_oracle_wavenet_sweep.py and oracle/gen_golden_wavenet_sweep.py share.

The presets only ever run 32 channels (6 layers, cycle 3) and 256 channels (36 layers, cycle 12); the bf16 tests add 64 and 128 channels at 13 layers and
T = 4200.  Every case names what it leaves that point for:
  w32 .. w512   all 16 widths the library takes, 2 layers, cycle 2, 2 x 37   every block size of the fp32 kernels (one thread per channel: 96, 160, 224, ... are
                                                      no whole number of waves; 512 takes 128 KiB of dynamic LDS), T ragged against the 16-position tile;
                                                      bf16 at 64 / 128 / 256 with one partial tile
  l1, l1b       1 layer, cycle 1, 2 x 20              the only layer is the first (skip is written, not accumulated) and the last (no y_next) at once
  cyc1          160 channels, 3 layers, cycle 1       every dilation 1, a block of 2.5 waves
  cyc24, cyc24b 25 layers, cycle 24, 2 x 100          dilations up to 2^23: both outer taps in the padding (bf16: the disjoint-window staging)
  d4096         128 channels, 14 layers, cycle 13, 2 x 300   the overlapping and the disjoint staging in one net, dilation 4096 > T
  mid           64 channels, 5 layers, cycle 4, 3 x 77       a second time with every step 37.0: a large argument of sinf / expf
  b1            96 channels, 3 layers, cycle 2, 1 x 50       one sample: the addend's batch stride is 0
  deep          32 channels, 1024 layers, cycle 12, 1 x 4200  550,502,400 bytes of fp32 layer inputs, more than the 512 MiB up to which the device keeps
                                                      every layer input: two buffers alternate; 1024 is the largest residual_layers the library takes
"""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import torch

from audiodiffuser_amd.config import WaveNetConfig
from audiodiffuser_amd.weights import generate_wavenet_weights

WIDTHS = tuple(range(32, 513, 32))
BF16_WIDTHS = (64, 128, 256)


def _c(channels, layers, cycle) -> WaveNetConfig:
    return WaveNetConfig(residual_channels=channels, residual_layers=layers, dilation_cycle=cycle)


# id -> (configuration, (B, T), weight seed, compute modes, the steps of the case or None for the default of inputs())
CASES: Dict[str, Tuple[WaveNetConfig, Tuple[int, int], int, Tuple[str, ...], Optional[Tuple[float, ...]]]] = {
    **{f"w{c}": (_c(c, 2, 2), (2, 37), 100 + c // 32, ("fp32", "bf16") if c in BF16_WIDTHS else ("fp32",), None) for c in WIDTHS},
    "l1": (_c(32, 1, 1), (2, 20), 121, ("fp32",), None),
    "l1b": (_c(64, 1, 1), (2, 20), 122, ("bf16",), None),
    "cyc1": (_c(160, 3, 1), (2, 33), 123, ("fp32",), None),
    "cyc24": (_c(32, 25, 24), (2, 100), 124, ("fp32",), None),
    "cyc24b": (_c(64, 25, 24), (2, 100), 125, ("bf16",), None),
    "d4096": (_c(128, 14, 13), (2, 300), 126, ("fp32", "bf16"), None),
    "mid": (_c(64, 5, 4), (3, 77), 127, ("fp32",), None),
    "mid37": (_c(64, 5, 4), (3, 77), 127, ("fp32",), (37.0, 37.0, 37.0)),       # mid again (same weights and audio), every step 37.0
    "b1": (_c(96, 3, 2), (1, 50), 128, ("fp32",), None),
    "deep": (_c(32, 1024, 12), (1, 4200), 129, ("fp32",), None),
}
KEEP_LIMIT = 512 << 20          # WavenetNet::forward keeps every layer input up to this many bytes of them


def layer_input_bytes(cfg: WaveNetConfig, shape, mode: str = "fp32") -> int:
    return shape[0] * shape[1] * cfg.residual_channels * (2 if mode == "bf16" else 4) * cfg.residual_layers


def inputs(cfg: WaveNetConfig, shape, seed: int = 0, steps=None):
    """audio [B, T] and one diffusion step per sample (c_noise of the EDM wrapper lies in about [-1.6, 1.1])."""
    b, t = shape
    g = torch.Generator().manual_seed(7000 + 17 * seed)
    audio = torch.randn(b, t, generator=g) * 0.6
    if steps is not None:
        step = torch.tensor(steps, dtype=torch.float32)
        assert step.shape == (b,)
    else:
        step = torch.linspace(-1.3, 0.9, b) if b > 1 else torch.tensor([0.35])
    return audio, step


def case_inputs(cid: str):
    cfg, shape, seed, _, steps = CASES[cid]
    return inputs(cfg, shape, seed, steps)


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a - b| / max |b| in float64: the metric of the fp32 bars (tests/test_wavenet.py rel)."""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


@functools.lru_cache(maxsize=None)
def _weights(cfg_key, seed):
    w = generate_wavenet_weights(_c(*cfg_key), seed=seed)
    return w, {k: v.double() for k, v in w.items()}


def weights_of(cfg: WaveNetConfig, seed: int):
    return _weights((cfg.residual_channels, cfg.residual_layers, cfg.dilation_cycle), seed)


def weights(cid: str):
    cfg, _, seed, _, _ = CASES[cid]
    return weights_of(cfg, seed)


def float64_run(cfg, w, w64, audio, step, fp32_runs: bool = True):
    """-> (float64 output, {name: float64 tensor} for every name the oracle records, {name: (fp32-oracle-vs-float64 distance in the reference's
    arithmetic, the same with exact_norm)} with "out").  ``fp32_runs=False`` leaves the distances out (an empty dict)."""
    from oracle import wavenet as W
    t64, dist = {}, {}
    with torch.no_grad():
        y64 = W.wavenet_forward(w64, cfg, audio.double(), step.double(), taps=t64)
        assert y64.dtype == torch.float64 and all(v.dtype == torch.float64 for v in t64.values())
        if fp32_runs:
            tr, te = {}, {}
            yr = W.wavenet_forward(w, cfg, audio, step, taps=tr)
            ye = W.wavenet_forward(w, cfg, audio, step, taps=te, exact_norm=True)
            assert yr.dtype == ye.dtype == torch.float32 and list(tr) == list(te) == list(t64)
            dist = {k: (rel(tr[k], t64[k]), rel(te[k], t64[k])) for k in t64}
            dist["out"] = (rel(yr, y64), rel(ye, y64))
    return y64, t64, dist


@functools.lru_cache(maxsize=None)
def float64_case(cid: str):
    """``float64_run`` of a sweep case on its own inputs, computed once per session."""
    cfg = CASES[cid][0]
    w, w64 = weights(cid)
    audio, step = case_inputs(cid)
    return float64_run(cfg, w, w64, audio, step)


@functools.lru_cache(maxsize=None)
def float64_reference(cid: str):
    """The float64 run alone (no fp32 runs, an empty distance dict): what a judge of the device needs; ``deep`` takes about 3 s instead of 8."""
    cfg = CASES[cid][0]
    w, w64 = weights(cid)
    audio, step = case_inputs(cid)
    return float64_run(cfg, w, w64, audio, step, fp32_runs=False)
