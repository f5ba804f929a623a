"""Float64 restatement of the reference's DAC decoder stack over a flat weight dict: ``dac.py::Decoder`` (src/models/backbones/dac/dac.py:108-137) and
``FineTuneAutoencoder.decode`` (src/models/backbones/dac_vae.py:69-71), as ``F.conv1d`` / ``F.conv_transpose1d`` on folded weights, with the taps the
library keeps; the cases of the DAC tests and their deterministic weights.  tools/gen_golden_dac.py pins it to the reference modules.

``bug``: one deliberate mis-statement (tests/test_dac_ref.py shows that each moves the output far beyond the device bar):
``"convT_axis"`` (the weight norm of a transposed conv over axis 1), ``"no_dilation"``, ``"floor_pad"`` (floor instead of ceil in the transposed
padding), ``"no_residual"``, ``"scalar_alpha"`` (the first channel's alpha for every channel).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from audiodiffuser_amd.dac import DACConfig, autoencoder_specs, decoder_specs, up_length

# name -> (kind, constructor arguments, B, T)
CASES = OrderedDict([
    ("odd", ("dec", dict(input_channel=64, channels=256, rates=[4, 5, 2]), 2, 13)),        # 13 -> 52 -> 259 -> 518: odd stride, odd lengths, tile tails
    ("r8", ("dec", dict(input_channel=32, channels=128, rates=[8, 3]), 1, 37)),            # output length 887
    ("w96", ("dec", dict(input_channel=8, channels=192, rates=[2]), 3, 70)),               # width 96 = 3 x 32 into the output kernel; padded input K
    ("long", ("dec", dict(input_channel=32, channels=64, rates=[8]), 3, 100)),             # L = 800: dilation-9 halos over many tiles and both sample seams
    ("short", ("dec", dict(input_channel=64, channels=256, rates=[4, 5, 2]), 1, 1)),       # 1 -> 4 -> 19 -> 38: shorter than the dilation-9 halo
    ("alpha0", ("dec", dict(input_channel=8, channels=192, rates=[2]), 3, 70)),            # w96 with one alpha exactly 0 and one 1e-4 in every Snake
    ("ae", ("ae", dict(), 2, 21)),
    ("ae_small", ("ae", dict(intermediate_embedding_size=[1024, 64], latent_dim=8), 1, 5)),
])
GOLDEN_CASES = ("odd", "w96", "ae")
DECODER_CASES = tuple(k for k, v in CASES.items() if v[0] == "dec")


def kind(case):
    return CASES[case][0]


def ctor_kwargs(case):
    return {k: (list(v) if isinstance(v, list) else v) for k, v in CASES[case][1].items()}


def config(case) -> DACConfig:
    kw = CASES[case][1]
    if kind(case) == "ae":
        return DACConfig(kind=1, input_channel=kw.get("latent_dim", 32), widths=list(kw.get("intermediate_embedding_size", [1024, 512, 256, 128])))
    return DACConfig(kind=0, input_channel=kw["input_channel"], channels=kw["channels"], rates=list(kw["rates"]))


def specs(cfg: DACConfig):
    return autoencoder_specs(cfg) if cfg.kind == 1 else decoder_specs(cfg)


def _gen(name: str, seed: int) -> torch.Generator:
    h = 1469598103934665603
    for ch in f"{seed}:{name}".encode():
        h = ((h ^ ch) * 1099511628211) % (1 << 63)
    return torch.Generator().manual_seed(h)


def generate(cfg: DACConfig, seed: int = 0, alpha_edge: bool = False):
    """Weights that keep every activation O(1) (unit-normal ``weight_g`` saturates tanh: every comparison would be vacuous): ``weight_v`` ~ N(0, 1);
    ``weight_g`` = 0.7 U(0.75, 1.25) for convs, that times sqrt(s / 2) for the transposed conv of stride s, 0.35 U(0.75, 1.25) for a unit's 1x1;
    alpha ~ U(0.2, 2.2) per channel; bias ~ 0.1 N(0, 1).  ``alpha_edge``: channel 1 of every Snake is exactly 0 and channel 2 is 1e-4."""
    out = OrderedDict()
    for name, (shape, k) in specs(cfg).items():
        g = _gen(name, seed)
        if k == "alpha":
            t = 0.2 + 2.0 * torch.rand(shape, generator=g)
            if alpha_edge:
                t[0, 1, 0], t[0, 2, 0] = 0.0, 1e-4
        elif k == "bias":
            t = 0.1 * torch.randn(shape, generator=g)
        elif k == "v":
            t = torch.randn(shape, generator=g)
        else:                   # "<what>_g"
            u = 0.75 + 0.5 * torch.rand(shape, generator=g)
            t = (0.35 if k == "pw_g" else 0.7) * u
            if k.startswith("up"):
                t = t * math.sqrt(int(k[2:-2]) / 2)
        out[name] = t.float()
    return out


# `short` has 38 output samples from one latent frame: at most seeds its pre-tanh maximum stays under the 0.5 that tests/test_dac_ref.py asks of every
# tap (0.25 .. 0.45 at seeds 0, 1, 2, 5, 7), so its seed is one that meets it (0.73).  Every other case takes the seed its name gives.
SEEDS = {"short": 4}


def weights(case):
    return generate(config(case), seed=SEEDS.get(case, sum(map(ord, case))), alpha_edge=case == "alpha0")


def inputs(case) -> torch.Tensor:
    cfg, (_, _, B, T) = config(case), CASES[case]
    return torch.randn((B, cfg.input_channel, T), generator=_gen("input:" + case, 1)).float()


def output_length(case) -> int:
    return config(case).output_length(CASES[case][3])


def fold(w, pre, dtype=torch.float64, axis0=True):
    """``g v / ||v||`` with the norm over all axes but 0 (``axis0=False``: but 1, the transposed conv's mis-statement)."""
    g, v = w[pre + ".weight_g"].to(dtype), w[pre + ".weight_v"].to(dtype)
    if axis0:
        return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))
    n = v.transpose(0, 1).flatten(1).norm(dim=1).view(1, -1, 1)
    return v * (g.flatten()[: v.shape[0]].view(-1, 1, 1) / n)


def snake(x, alpha, bug=None):
    if bug == "scalar_alpha":
        alpha = alpha[:, :1]
    return x + (alpha + 1e-9).reciprocal() * torch.sin(alpha * x).pow(2)


def _conv(w, pre, x, dtype, k, dil=1):
    return F.conv1d(x, fold(w, pre, dtype), w[pre + ".bias"].to(dtype), padding=(k - 1) // 2 * dil, dilation=dil)


def decoder_forward(w, cfg: DACConfig, z, dtype=torch.float64, taps=None, bug=None):
    """``Decoder.forward``; taps: ``model.0``, ``model.<i>`` (DecoderBlock), ``model.<i>.block.1`` (transposed conv), ``model.<i>.block.{2,3,4}``
    (ResidualUnit), ``model.<n + 2>`` (before tanh)."""
    w = {k: v.to(dtype) for k, v in w.items()}
    keep = (lambda n, t: taps.__setitem__(n, t)) if taps is not None else (lambda n, t: None)
    x = _conv(w, "model.0", z.to(dtype), dtype, 7)
    keep("model.0", x)
    for i, s in enumerate(cfg.rates):
        p = f"model.{i + 1}.block"
        x = snake(x, w[f"{p}.0.alpha"], bug)
        pad = s // 2 if bug == "floor_pad" else math.ceil(s / 2)
        x = F.conv_transpose1d(x, fold(w, f"{p}.1", dtype, axis0=bug != "convT_axis"), w[f"{p}.1.bias"], stride=s, padding=pad)
        keep(f"{p}.1", x)
        for u, dil in enumerate((1, 3, 9)):
            q = f"{p}.{u + 2}.block"
            y = _conv(w, f"{q}.1", snake(x, w[f"{q}.0.alpha"], bug), dtype, 7, 1 if bug == "no_dilation" else dil)
            y = _conv(w, f"{q}.3", snake(y, w[f"{q}.2.alpha"], bug), dtype, 1)
            x = y if bug == "no_residual" else x + y
            keep(f"{p}.{u + 2}", x)
        keep(f"model.{i + 1}", x)
    n = len(cfg.rates)
    x = _conv(w, f"model.{n + 2}", snake(x, w[f"model.{n + 1}.alpha"], bug), dtype, 7)
    keep(f"model.{n + 2}", x)
    return torch.tanh(x)


def autoencoder_decode(w, cfg: DACConfig, x, dtype=torch.float64, taps=None):
    """``FineTuneAutoencoder.decode``; taps: ``decoder_layers.<2 i>`` (every conv)."""
    w = {k: v.to(dtype) for k, v in w.items()}
    x = _conv(w, "decoder_layers.0", x.to(dtype), dtype, 3)
    if taps is not None:
        taps["decoder_layers.0"] = x
    for i in range(1, len(cfg.widths)):
        x = _conv(w, f"decoder_layers.{2 * i}", snake(x, w[f"decoder_layers.{2 * i - 1}.alpha"]), dtype, 3)
        if taps is not None:
            taps[f"decoder_layers.{2 * i}"] = x
    return x


def forward(case, dtype=torch.float64, taps=None, bug=None, w=None, x=None):
    cfg = config(case)
    w = weights(case) if w is None else w
    x = inputs(case) if x is None else x
    if cfg.kind == 1:
        return autoencoder_decode(w, cfg, x, dtype, taps)
    return decoder_forward(w, cfg, x, dtype, taps, bug)


_CACHE = {}


def reference(case):
    """(output, taps) of the float64 restatement, computed once per process and shared; callers leave it unchanged."""
    if case not in _CACHE:
        taps = OrderedDict()
        with torch.no_grad():
            _CACHE[case] = (forward(case, taps=taps), taps)
    return _CACHE[case]


__all__ = ["CASES", "GOLDEN_CASES", "DECODER_CASES", "config", "ctor_kwargs", "weights", "inputs", "forward", "reference", "up_length", "output_length"]
