"""HIP-backed drop-ins for the reference's DAC stacks: ``dac.py::Decoder`` (src/models/backbones/dac/dac.py:108-137) as ``DACDecoder``,
``dac.py::Encoder`` (:57-84) as ``DACEncoder`` and ``FineTuneAutoencoder`` (src/models/backbones/dac_vae.py:11-77).  ``dec(ae.decode(latents))`` is the
path from a sampled latent to audio; ``ae.encode(enc(audio), is_train=False)`` is the path from audio to the latent a latent net is trained and validated on.

Contract kept: the positional constructor arguments and defaults, ``state_dict()`` keys / order / shapes (the old-style weight-norm pair ``weight_g`` /
``weight_v`` of every conv behind its ``bias``; ``alpha`` of every Snake as ``[1, C, 1]``), so a slice of a reference checkpoint strict-loads.  Exact fp32
on the device; every argument the kernels do not serve raises ``ValueError`` naming it.  The weight norm ``g v / ||v||`` is folded by the library
before the first pass after any tensor changed.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import List, Tuple

import torch
import torch.nn as nn

from . import _lib
from .net import HipNet, _stream_ptr

Spec = Tuple[Tuple[int, ...], str]
MAX_RATES, MAX_WIDTHS = 6, 8          # ADF_DAC_MAX_RATES, ADF_DAC_MAX_WIDTHS


def up_length(L: int, s: int) -> int:
    """Length behind ``ConvTranspose1d(kernel 2 s, stride s, padding ceil(s / 2))``: ``L s`` for even ``s``, ``L s - 1`` for odd ``s``."""
    return (L - 1) * s - 2 * math.ceil(s / 2) + 2 * s


def down_min_length(s: int) -> int:
    """Shortest input ``Conv1d(kernel 2 s, stride s, padding ceil(s / 2))`` serves: ``s`` for even ``s``, ``s - 1`` for odd ``s``."""
    return 2 * s - 2 * math.ceil(s / 2)


def down_length(L: int, s: int) -> int:
    """Length behind ``Conv1d(kernel 2 s, stride s, padding ceil(s / 2))``: ``L // s`` for even ``s``, ``(L + 1) // s`` for odd ``s``."""
    return (L + 2 * math.ceil(s / 2) - 2 * s) // s + 1


@dataclass
class DACConfig:
    """What the library is told about one DAC handle (``adf_dac_config``): ``kind`` 0 the decoder, 1 the autoencoder, 2 the encoder."""
    kind: int = 0
    input_channel: int = 1024           # decoder: input_channel; autoencoder: latent_dim; encoder: 1
    channels: int = 1536                # encoder: d_model
    rates: List[int] = field(default_factory=list)       # encoder: strides
    d_out: int = 1                      # encoder: d_latent; autoencoder: 2 (ADF_DAC_BTNK_TANH) with tanh_btnk
    widths: List[int] = field(default_factory=list)      # autoencoder: intermediate_embedding_size

    is_dac = True                       # what NativeHandle keys its create call on
    class_cond = False

    def output_length(self, T: int) -> int:
        for i, s in enumerate(self.rates):
            if self.kind == 2:
                if T < down_min_length(s):
                    raise ValueError(f"L is too short: the strided conv of stage {i} (stride {s}) needs at least {down_min_length(s)} positions, has {T}")
                T = down_length(T, s)
            else:
                T = up_length(T, s)
        return T

    @property
    def out_channels(self) -> int:
        return self.widths[0] if self.kind == 1 else self.d_out

    def validate_device(self) -> None:
        """What the kernels serve (csrc/adf_dac.h), reported against the constructor argument that sets it."""
        if self.kind == 2:
            if not 1 <= len(self.rates) <= MAX_RATES or any(int(s) != s or not 2 <= s <= 16 for s in self.rates):
                raise ValueError(f"strides={list(self.rates)} must be 1 to {MAX_RATES} integers in [2, 16]")
            if self.channels < 32 or self.channels % 32 or self.channels << len(self.rates) > 8192:
                raise ValueError(f"d_model={self.channels} must be a multiple of 32 with d_model * 2**len(strides) <= 8192")
            if self.d_out < 32 or self.d_out % 32 or self.d_out > 8192:
                raise ValueError(f"d_latent={self.d_out} must be a multiple of 32 in [32, 8192]")
            return
        ic = "latent_dim" if self.kind == 1 else "input_channel"
        if self.input_channel < 4 or self.input_channel % 4 or self.input_channel > 2048:
            raise ValueError(f"{ic}={self.input_channel} must be a multiple of 4 in [4, 2048]")
        if self.kind == 1:
            w = self.widths
            if not 2 <= len(w) <= MAX_WIDTHS or w[0] != 1024 or any(int(c) < 32 or int(c) % 32 or int(c) > 8192 for c in w):
                raise ValueError(f"intermediate_embedding_size={list(w)} must have 2 to {MAX_WIDTHS} entries, 1024 first (the DAC embedding), "
                                 "each a multiple of 32")
            return
        if not 1 <= len(self.rates) <= MAX_RATES or any(int(s) != s or not 2 <= s <= 16 for s in self.rates):
            raise ValueError(f"rates={list(self.rates)} must be 1 to {MAX_RATES} integers in [2, 16]")
        if self.channels < 1 or self.channels > 8192 or self.channels % (32 << len(self.rates)):
            raise ValueError(f"channels={self.channels}: every stage width channels / 2**i (i up to {len(self.rates)}) must be a multiple of 32")
        if self.d_out != 1:
            raise ValueError(f"d_out={self.d_out}: the output kernel writes one channel")


def _wn_conv(out: "OrderedDict[str, Spec]", pre: str, cin: int, cout: int, k: int, transposed: bool = False, kind: str = "conv") -> None:
    """``weight_norm(nn.Conv1d / nn.ConvTranspose1d)``: ``weight`` leaves the module, ``weight_g`` and ``weight_v`` join behind ``bias``."""
    out[f"{pre}.bias"] = ((cout,), "bias")
    out[f"{pre}.weight_g"] = ((cin if transposed else cout, 1, 1), kind + "_g")
    out[f"{pre}.weight_v"] = ((cin, cout, k) if transposed else (cout, cin, k), "v")


def decoder_specs(cfg: DACConfig) -> "OrderedDict[str, Spec]":
    """Every ``Decoder.state_dict()`` key with its shape, in the module's order (dac.py:118-134)."""
    out: "OrderedDict[str, Spec]" = OrderedDict()
    _wn_conv(out, "model.0", cfg.input_channel, cfg.channels, 7)
    for i, s in enumerate(cfg.rates):
        cin, cout, p = cfg.channels // 2 ** i, cfg.channels // 2 ** (i + 1), f"model.{i + 1}.block"
        out[f"{p}.0.alpha"] = ((1, cin, 1), "alpha")
        _wn_conv(out, f"{p}.1", cin, cout, 2 * s, transposed=True, kind=f"up{s}")
        for u in range(3):
            out[f"{p}.{u + 2}.block.0.alpha"] = ((1, cout, 1), "alpha")
            _wn_conv(out, f"{p}.{u + 2}.block.1", cout, cout, 7)
            out[f"{p}.{u + 2}.block.2.alpha"] = ((1, cout, 1), "alpha")
            _wn_conv(out, f"{p}.{u + 2}.block.3", cout, cout, 1, kind="pw")
    n, cl = len(cfg.rates), cfg.channels // 2 ** len(cfg.rates)
    out[f"model.{n + 1}.alpha"] = ((1, cl, 1), "alpha")
    _wn_conv(out, f"model.{n + 2}", cl, cfg.d_out, 7)
    return out


def encoder_specs(cfg: DACConfig) -> "OrderedDict[str, Spec]":
    """Every ``Encoder.state_dict()`` key with its shape, in the module's order (dac.py:66-80)."""
    out: "OrderedDict[str, Spec]" = OrderedDict()
    _wn_conv(out, "block.0", 1, cfg.channels, 7)
    for i, s in enumerate(cfg.rates):
        c, p = cfg.channels * 2 ** i, f"block.{i + 1}.block"
        for u in range(3):
            out[f"{p}.{u}.block.0.alpha"] = ((1, c, 1), "alpha")
            _wn_conv(out, f"{p}.{u}.block.1", c, c, 7)
            out[f"{p}.{u}.block.2.alpha"] = ((1, c, 1), "alpha")
            _wn_conv(out, f"{p}.{u}.block.3", c, c, 1, kind="pw")
        out[f"{p}.3.alpha"] = ((1, c, 1), "alpha")
        _wn_conv(out, f"{p}.4", c, 2 * c, 2 * s, kind="down")
    n, cl = len(cfg.rates), cfg.channels * 2 ** len(cfg.rates)
    out[f"block.{n + 1}.alpha"] = ((1, cl, 1), "alpha")
    _wn_conv(out, f"block.{n + 2}", cl, cfg.d_out, 3)
    return out


def autoencoder_specs(cfg: DACConfig) -> "OrderedDict[str, Spec]":
    """Every ``FineTuneAutoencoder.state_dict()`` key (dac_vae.py:25-44): the bottleneck, the encoder, the decoder."""
    w, out = list(cfg.widths), OrderedDict()
    out["btnk_layer.weight"] = ((2 * cfg.input_channel, w[-1], 1), "v")
    out["btnk_layer.bias"] = ((2 * cfg.input_channel,), "bias")
    for i, (a, b) in enumerate(zip(w[:-1], w[1:])):
        out[f"encoder_layers.{2 * i}.alpha"] = ((1, a, 1), "alpha")
        _wn_conv(out, f"encoder_layers.{2 * i + 1}", a, b, 3)
    _wn_conv(out, "decoder_layers.0", cfg.input_channel, w[-1], 3)
    r = w[::-1]
    for i, (a, b) in enumerate(zip(r[:-1], r[1:])):
        out[f"decoder_layers.{2 * i + 1}.alpha"] = ((1, a, 1), "alpha")
        _wn_conv(out, f"decoder_layers.{2 * i + 2}", a, b, 3)
    return out


def _init_like_reference(shape, kind: str) -> torch.Tensor:
    """Snake's alpha is 1; a weight-normed conv starts as torch's default conv with g = ||v|| (so w = v); DAC's ``init_weights`` zeroes the bias."""
    t = torch.empty(shape, dtype=torch.float32)
    if kind == "alpha":
        return t.fill_(1.0)
    if kind == "bias":
        return t.zero_()
    if kind == "v":
        nn.init.kaiming_uniform_(t, a=math.sqrt(5))
        return t
    return t.fill_(1.0)


class _DacNet(HipNet):
    """What the two classes share: the parameter tree from a spec and the one device call."""

    def _build(self, cfg: DACConfig, specs_of) -> None:
        cfg.validate_device()
        self.cfg = cfg
        specs = specs_of(cfg)
        for name, (shape, kind) in specs.items():
            self._register(name, nn.Parameter(_init_like_reference(shape, kind)))
        # g = ||v|| over all axes but 0, as weight_norm initialises it
        with torch.no_grad():
            sd = dict(self.named_parameters())
            for name in specs:
                if name.endswith(".weight_g"):
                    sd[name].copy_(sd[name[:-1] + "v"].flatten(1).norm(dim=1).view(-1, 1, 1))

    def _run(self, x: torch.Tensor, what: str) -> torch.Tensor:
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError(f"the HIP {type(self).__name__} is an inference path (no backward); call it under torch.no_grad()")
        if x.ndim != 3 or x.shape[1] != self.cfg.input_channel or x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError(f"{what} must be shaped [B, {self.cfg.input_channel}, {'L' if self.cfg.kind == 2 else 'T'}]")
        B, T = int(x.shape[0]), int(x.shape[2])
        shape = (B, self.cfg.widths[0], T) if self.cfg.kind == 1 else (B, self.cfg.d_out, self.cfg.output_length(T))      # (encoder: refuses a short L)
        hd = self.native(x.device)
        xin = x.detach().to(torch.float32).contiguous()
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            hd.check(hd.lib.adf_dac_forward(hd.h, C.c_void_p(xin.data_ptr()), B, T, C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(x.device))),
                     "adf_dac_forward")
        return out.to(x.dtype)


class DACDecoder(_DacNet):
    """HIP-backed ``dac.py::Decoder``: ``forward(z)`` takes ``[B, input_channel, T]`` on a ROCm device and returns the waveform ``[B, 1, L_out]``.
    On the device: every stage width ``channels / 2**i`` a multiple of 32 (1536 -> 96, 1024 -> 64), ``input_channel`` a multiple of 4 in [4, 2048],
    1 to 6 rates in [2, 16] (odd ones included), ``d_out = 1``, ``compute_dtype="fp32"``."""

    def __init__(self, input_channel, channels, rates, d_out: int = 1, compute_dtype: str = "fp32"):
        super().__init__()
        if compute_dtype != "fp32":
            raise ValueError(f"compute_dtype={compute_dtype!r}: the DAC decoder runs in 'fp32' (exact) only")
        self.compute_dtype = compute_dtype
        self._build(DACConfig(kind=0, input_channel=int(input_channel), channels=int(channels), rates=list(rates), d_out=int(d_out)), decoder_specs)

    def output_length(self, T: int) -> int:
        """Samples per item that ``forward`` returns for ``T`` latent frames: each rate ``s`` maps ``L`` to ``(L - 1) s - 2 ceil(s / 2) + 2 s``."""
        return self.cfg.output_length(int(T))

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        return self._run(z, "z")


class DACEncoder(_DacNet):
    """HIP-backed ``dac.py::Encoder``: ``forward(audio)`` takes ``[B, 1, L]`` on a ROCm device and returns ``[B, d_latent, output_length(L)]``.
    On the device: ``d_model`` a multiple of 32 with ``d_model * 2**len(strides) <= 8192``, ``d_latent`` a multiple of 32 in [32, 8192], 1 to 6
    strides in [2, 16] (odd ones included).  With a DAC checkpoint: ``load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if
    k.startswith("encoder.")})``."""

    def __init__(self, d_model: int = 64, strides: list = [2, 4, 8, 8], d_latent: int = 64):
        super().__init__()
        self._build(DACConfig(kind=2, input_channel=1, channels=int(d_model), rates=list(strides), d_out=int(d_latent)), encoder_specs)
        self.enc_dim = self.cfg.channels * 2 ** len(self.cfg.rates)

    def output_length(self, L: int) -> int:
        """Frames per item that ``forward`` returns for ``L`` samples: each stride ``s`` maps ``L`` to ``floor((L + 2 ceil(s / 2) - 2 s) / s) + 1``
        and needs ``L >= 2 s - 2 ceil(s / 2)`` (``ValueError`` naming ``L`` otherwise)."""
        return self.cfg.output_length(int(L))

    def forward(self, audio: torch.Tensor) -> torch.Tensor:
        return self._run(audio, "audio")


class FineTuneAutoencoder(_DacNet):
    """HIP-backed ``FineTuneAutoencoder``.  ``decode(x)`` takes ``[B, latent_dim, T]`` on a ROCm device and returns the DAC embedding ``[B, 1024, T]``.
    ``encode(x, is_train=False)`` takes that embedding and returns ``(mean [B, latent_dim, T], kl)``; ``forward(x, is_train=False)`` returns
    ``(decode(mean), kl)``.  Pass ``is_train=False``: the default ``is_train=True`` draws ``randn_like`` (training-side) and is refused."""

    def __init__(self, intermediate_embedding_size=[1024, 512, 256, 128], conv_kernel=3, tanh_btnk=False, latent_dim=32):
        super().__init__()
        if conv_kernel != 3:
            raise ValueError(f"conv_kernel={conv_kernel}: with the reference's fixed padding=1 only 3 keeps the length")
        self.tanh_btnk = tanh_btnk
        self._build(DACConfig(kind=1, input_channel=int(latent_dim), widths=[int(c) for c in intermediate_embedding_size],
                              d_out=_lib.DAC_BTNK_TANH if tanh_btnk else 1), autoencoder_specs)

    def decode(self, x: torch.Tensor) -> torch.Tensor:
        return self._run(x, "x")

    def encode(self, x, is_train=True):
        """``(mean, kl_loss_value)`` of the reference's ``encode(x, is_train=False)``: ``x`` is ``[B, 1024, T]``, mean ``[B, latent_dim, T]`` (tanh of it
        with ``tanh_btnk``), kl a 0-dim tensor.  Pass ``is_train=False``: sampling from (mean, logvar) is training-side."""
        if is_train:
            raise NotImplementedError("FineTuneAutoencoder.encode with is_train=True (VAE sampling) is training-side and not on the device path; "
                                      "pass is_train=False")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError(f"the HIP {type(self).__name__} is an inference path (no backward); call it under torch.no_grad()")
        if x.ndim != 3 or x.shape[1] != self.cfg.widths[0] or x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError(f"x must be shaped [B, {self.cfg.widths[0]}, T]")
        hd = self.native(x.device)
        xin = x.detach().to(torch.float32).contiguous()
        B, T = int(xin.shape[0]), int(xin.shape[2])
        mean = torch.empty((B, self.cfg.input_channel, T), device=x.device, dtype=torch.float32)
        kl = torch.empty((), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            hd.check(hd.lib.adf_dac_encode(hd.h, C.c_void_p(xin.data_ptr()), B, T, C.c_void_p(mean.data_ptr()), C.c_void_p(kl.data_ptr()),
                                           C.c_void_p(_stream_ptr(x.device))), "adf_dac_encode")
        return mean.to(x.dtype), kl.to(x.dtype)

    def forward(self, x, is_train=True):
        """``(decode(mean), kl_loss_value)`` of the reference's ``forward(x, is_train=False)``.  Pass ``is_train=False``."""
        if is_train:
            raise NotImplementedError("FineTuneAutoencoder.forward with is_train=True samples the latent (training-side); pass is_train=False, "
                                      "or call decode(latents)")
        mean, kl = self.encode(x, is_train=False)
        return self.decode(mean), kl


def make_dac_config(cfg: DACConfig, dtype: int) -> "_lib.AdfDacConfig":
    c = _lib.AdfDacConfig()
    c.kind, c.input_channel, c.channels, c.d_out, c.dtype = cfg.kind, cfg.input_channel, cfg.channels, cfg.d_out, dtype
    c.n_rates, c.n_widths = len(cfg.rates), len(cfg.widths)
    for i, s in enumerate(cfg.rates):
        c.rates[i] = int(s)
    for i, w in enumerate(cfg.widths):
        c.widths[i] = int(w)
    return c
