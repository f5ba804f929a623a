"""``model.net`` plugin: HIP-backed drop-in for the reference's ``DiT``, the adaLN-Zero diffusion transformer
(src/models/backbones/dit.py:278-429).

Contract kept: the constructor kwargs and defaults (hydra ``_target_`` instantiation), ``state_dict()`` keys / order / shapes (reference checkpoints
strict-load; ``attn.to_context`` is loaded and never read), ``forward(x, t, classes=None, text_embeds=None, text_mask=None, cond_drop_prob=None)``
on ``[B, C, H, W]`` with ``(H, W) == input_size`` or ``[B, C, L]`` (the same call with ``H = 1``).  On the device, in exact fp32 or in the split-bf16
mode (``compute_dtype="f32x3"``: fp32 storage, bf16 hi + lo GEMM and attention operands): unconditional nets and
``label_cond=True`` with ``num_classes``; the attention's plain branch (no text context, so no RoPE and no mask).  Every other branch raises, naming
its argument.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from .net import HipNet
from .weights import generate_tensor

Spec = Tuple[Tuple[int, ...], str]


@dataclass
class DiTConfig:
    """Constructor arguments of ``DiT`` (dit.py:282-300) that shape the device path, same names and defaults."""
    input_size: Tuple[int, int] = (256, 128)
    patch_size: Tuple[int, int] = (8, 4)
    in_channels: int = 4
    hidden_size: int = 1152
    depth: int = 28
    num_heads: int = 16
    mlp_ratio: float = 4.0
    num_classes: Optional[int] = None
    label_cond: bool = False

    is_dit = True               # what NativeHandle keys its create call and the length argument on

    @property
    def class_cond(self) -> bool:
        """What the shared denoise / sampler host code asks of a network config."""
        return bool(self.label_cond)

    @property
    def out_channels(self) -> int:
        return self.in_channels                                  # dit.py:303

    @property
    def grid(self) -> Tuple[int, int]:
        return (self.input_size[0] // self.patch_size[0], self.input_size[1] // self.patch_size[1])

    @property
    def tokens(self) -> int:
        return self.grid[0] * self.grid[1]

    @property
    def mlp_hidden(self) -> int:
        return int(self.hidden_size * self.mlp_ratio)            # dit.py:238

    @property
    def patch_dim(self) -> int:
        return self.patch_size[0] * self.patch_size[1] * self.in_channels

    def validate_device(self) -> None:
        """What the kernels serve (csrc/adf_dit.h, launch_attention), reported against the constructor argument that sets it."""
        if len(self.input_size) != 2 or len(self.patch_size) != 2:
            raise ValueError(f"input_size={self.input_size} and patch_size={self.patch_size} must have two entries each")
        if any(int(s) < 1 for s in self.input_size) or any(int(p) < 1 for p in self.patch_size) or \
                any(int(s) % int(p) for s, p in zip(self.input_size, self.patch_size)):
            raise ValueError(f"input_size={list(self.input_size)} must be divisible by patch_size={list(self.patch_size)}")
        if self.num_heads < 1 or self.hidden_size % self.num_heads or self.hidden_size // self.num_heads not in (32, 64):
            raise ValueError(f"num_heads={self.num_heads}: the attention head dim (hidden_size {self.hidden_size} / num_heads) must be 32 or 64")
        if self.hidden_size < 64 or self.hidden_size % 64 or self.hidden_size > 1024:
            raise ValueError(f"hidden_size={self.hidden_size}: the token-linear kernels serve multiples of 64 up to 1024")
        if self.mlp_hidden < 32 or self.mlp_hidden % 32 or self.mlp_hidden > 4096:
            raise ValueError(f"mlp_ratio={self.mlp_ratio}: the MLP width int(hidden_size * mlp_ratio) = {self.mlp_hidden} must be a multiple "
                             "of 32, at most 4096")
        if not 4 <= self.patch_dim <= 256:
            raise ValueError(f"patch_size={list(self.patch_size)}, in_channels={self.in_channels}: prod(patch_size) * in_channels = "
                             f"{self.patch_dim} must lie in [4, 256]")
        if self.depth < 1 or self.depth > 64:
            raise ValueError(f"depth={self.depth} must lie in [1, 64]")
        if self.label_cond and not (isinstance(self.num_classes, int) and self.num_classes > 0):
            raise ValueError("label_cond=True needs num_classes (labels; class_embed_dim inputs are not on the device path)")


def sincos_pos_embed(embed_dim: int, grid: Tuple[int, int]) -> torch.Tensor:
    """The fixed 2-D sin-cos table ``[grid_h * grid_w, embed_dim]`` exactly as dit.py:168-214 builds it: float32 aranges meshed with the w grid
    first, float64 frequencies and angles, ``[sin | cos]`` per axis, the two axes concatenated, then ``.float()``."""
    gh = np.arange(grid[0], dtype=np.float32)
    gw = np.arange(grid[1], dtype=np.float32)
    g = np.stack(np.meshgrid(gw, gh), axis=0).reshape([2, 1, grid[0], grid[1]])

    def one(dim, pos):
        omega = np.arange(dim // 2, dtype=np.float64)
        omega /= dim / 2.
        omega = 1. / 10000 ** omega
        out = np.einsum("m,d->md", pos.reshape(-1), omega)
        return np.concatenate([np.sin(out), np.cos(out)], axis=1)

    emb = np.concatenate([one(embed_dim // 2, g[0]), one(embed_dim // 2, g[1])], axis=1)
    return torch.from_numpy(emb).float()


def param_specs(cfg: DiTConfig) -> "OrderedDict[str, Spec]":
    """Every ``DiT.state_dict()`` key with its shape, in the module's order: its own parameter (``pos_embed``) first, then the children in
    registration order (dit.py:311-325)."""
    D, hid = cfg.hidden_size, cfg.mlp_hidden
    out: "OrderedDict[str, Spec]" = OrderedDict()
    out["pos_embed"] = ((1, cfg.tokens, D), "pos")
    out["x_embedder.proj.weight"] = ((D, cfg.in_channels, cfg.patch_size[0], cfg.patch_size[1]), "patch_w")
    out["x_embedder.proj.bias"] = ((D,), "bias")
    out["t_embedder.mlp.0.weight"] = ((D, D), "linear_w")
    out["t_embedder.mlp.0.bias"] = ((D,), "bias")
    out["t_embedder.mlp.2.weight"] = ((D, D), "linear_w")
    out["t_embedder.mlp.2.bias"] = ((D,), "bias")
    if cfg.label_cond:                    # LabelEmbedder(num_classes, None, hidden, hidden), conditioner.py:64-90
        out["y_embedder.null_classes_emb"] = ((1, D), "embed")
        out["y_embedder.label_emb.weight"] = ((cfg.num_classes, D), "embed")
        out["y_embedder.class_to_cond.0.weight"] = ((D,), "norm_w")
        out["y_embedder.class_to_cond.0.bias"] = ((D,), "norm_b")
        out["y_embedder.class_to_cond.1.weight"] = ((D, D), "linear_w")
        out["y_embedder.class_to_cond.1.bias"] = ((D,), "bias")
        out["y_embedder.class_to_cond.3.weight"] = ((D, D), "linear_w")
        out["y_embedder.class_to_cond.3.bias"] = ((D,), "bias")
    for i in range(cfg.depth):
        p = f"blocks.{i}"
        out[f"{p}.attn.to_q.weight"] = ((D, D), "linear_w")
        out[f"{p}.attn.to_kv.weight"] = ((2 * D, D), "linear_w")
        out[f"{p}.attn.to_context.weight"] = ((2 * D, D), "linear_w")
        out[f"{p}.attn.to_out.weight"] = ((D, D), "linear_w")
        out[f"{p}.mlp.fc1.weight"] = ((hid, D), "linear_w")
        out[f"{p}.mlp.fc1.bias"] = ((hid,), "bias")
        out[f"{p}.mlp.fc2.weight"] = ((D, hid), "linear_w")
        out[f"{p}.mlp.fc2.bias"] = ((D,), "bias")
        out[f"{p}.adaLN_modulation.1.weight"] = ((6 * D, D), "zero_w")
        out[f"{p}.adaLN_modulation.1.bias"] = ((6 * D,), "zero_b")
    out["final_layer.linear.weight"] = ((cfg.patch_dim, D), "zero_w")
    out["final_layer.linear.bias"] = ((cfg.patch_dim,), "zero_b")
    out["final_layer.adaLN_modulation.1.weight"] = ((2 * D, D), "zero_w")
    out["final_layer.adaLN_modulation.1.bias"] = ((2 * D,), "zero_b")
    return out


def generate_weights(cfg: DiTConfig, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Name-keyed deterministic weights (the generator of audiodiffuser_amd/weights.py).  ``initialize_weights`` zeroes every adaLN modulation and the
    final linear (dit.py:355-364): such a net returns zeros and every block is the identity, so a parity check on it is vacuous -- they are random
    here.  ``pos_embed`` is the fixed table."""
    out = OrderedDict()
    for k, (shape, kind) in param_specs(cfg).items():
        if kind == "pos":
            out[k] = sincos_pos_embed(cfg.hidden_size, cfg.grid).unsqueeze(0)
        elif kind == "patch_w":
            out[k] = generate_tensor(k, shape, "embed", seed) * (1.0 / (shape[1] * shape[2] * shape[3]) ** 0.5)
        elif kind == "zero_w":
            out[k] = generate_tensor(k, shape, "linear_w", seed)
        elif kind == "zero_b":
            out[k] = generate_tensor(k, shape, "bias", seed)
        else:
            out[k] = generate_tensor(k, shape, kind, seed)
    return out


def _init_like_reference(name: str, shape, kind: str, cfg: DiTConfig) -> torch.Tensor:
    """``DiT.initialize_weights`` (dit.py:328-364)."""
    t = torch.empty(shape, dtype=torch.float32)
    if kind == "pos":
        return sincos_pos_embed(cfg.hidden_size, cfg.grid).unsqueeze(0)
    if kind in ("zero_w", "zero_b", "bias", "norm_b"):
        return t.zero_()
    if kind == "norm_w":
        return t.fill_(1.0)
    if kind == "patch_w":
        nn.init.xavier_uniform_(t.view(shape[0], -1))
        return t
    if name.startswith("t_embedder.") or name == "y_embedder.label_emb.weight":
        return t.normal_(std=0.02)
    if kind == "embed":
        return t.normal_()
    nn.init.xavier_uniform_(t)
    return t


class DiT(HipNet):
    """HIP-backed ``DiT``.  Extra kwarg: ``compute_dtype`` in {"fp32", "f32x3"}: "fp32" (default) is exact fp32; "f32x3" keeps fp32 storage and every
    non-GEMM kernel and runs the q|k|v, to_out, fc1 and fc2 linears and the attention products on the bf16 matrix cores with every operand split into
    bf16 hi + lo (three MFMAs per product, ~1e-5 of exact fp32).  Both modes serve the same widths: ``hidden_size`` a multiple of 64 up to 1024, head dim 32 or
    64, ``int(hidden_size * mlp_ratio)`` a multiple of 32 up to 4096, ``prod(patch_size) * in_channels`` in [4, 256], any token count
    (DiT-S, DiT-B and DiT-L; DiT-XL's head dim 72 is refused)."""

    def __init__(self, input_size=[256, 128], patch_size=[8, 4], in_channels=4, hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4.0,
                 cond_drop_prob=0.1, num_classes=None, class_embed_dim=None, label_cond=False, text_cond=False, text_embed_dim=512,
                 max_text_len=128, use_self_text_cond=True, use_qk_l2norm=False, compute_dtype: str = "fp32"):
        super().__init__()
        if compute_dtype not in ("fp32", "f32x3"):
            raise ValueError(f"compute_dtype={compute_dtype!r}: DiT runs in 'fp32' (exact) or 'f32x3' (split-bf16 GEMM operands, fp32 storage); "
                             "there is no bf16-storage DiT")
        if text_cond:
            raise NotImplementedError("DiT(text_cond=True) is not on the device path (text conditioning, and with it RoPE and the key mask)")
        if class_embed_dim is not None:
            raise NotImplementedError("DiT(class_embed_dim) (embedding inputs instead of labels) is not on the device path")
        if use_qk_l2norm:
            raise NotImplementedError("DiT(use_qk_l2norm=True) is not on the device path")
        cfg = DiTConfig(input_size=tuple(int(s) for s in input_size), patch_size=tuple(int(p) for p in patch_size), in_channels=int(in_channels),
                        hidden_size=int(hidden_size), depth=int(depth), num_heads=int(num_heads), mlp_ratio=float(mlp_ratio),
                        num_classes=num_classes if label_cond else None, label_cond=bool(label_cond))
        cfg.validate_device()
        self.cfg = cfg
        self.compute_dtype = compute_dtype
        self.cond_drop_prob = cond_drop_prob
        self.in_channels = self.out_channels = cfg.in_channels
        self.input_size, self.patch_size = list(cfg.input_size), list(cfg.patch_size)
        for name, (shape, kind) in param_specs(cfg).items():
            self._register(name, nn.Parameter(_init_like_reference(name, shape, kind, cfg), requires_grad=kind != "pos"))

    def forward(self, x: torch.Tensor, t: torch.Tensor, classes: Optional[torch.Tensor] = None, text_embeds=None, text_mask=None,
                cond_drop_prob=None, **kwargs) -> torch.Tensor:
        if text_embeds is not None:
            raise NotImplementedError("text_embeds: text conditioning is not on the device path of DiT")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("the HIP DiT is an inference path (no backward); call it under torch.no_grad()")
        if x.ndim not in (3, 4) or x.shape[1] != self.cfg.in_channels:
            raise ValueError(f"x must be shaped [B, {self.cfg.in_channels}, H, W] or [B, {self.cfg.in_channels}, L]")
        hw = tuple(x.shape[2:]) if x.ndim == 4 else (1, x.shape[2])
        if hw != tuple(self.cfg.input_size):
            raise ValueError(f"input ({hw[0]}, {hw[1]}) doesn't match the model's input_size {list(self.cfg.input_size)}")     # PatchEmbed, dit.py:101-104
        if classes is not None:
            if not self.cfg.label_cond:
                raise ValueError("classes were given to a DiT built without label_cond=True")
            # LabelEmbedder(classes, cond_drop_prob): the label mask is deterministic only at 0 (keep all) and 1 (the null embedding for all)
            cdp = self.cond_drop_prob if cond_drop_prob is None else cond_drop_prob
            if cdp not in (0, 0.0, 1, 1.0):
                raise NotImplementedError(f"cond_drop_prob={cdp}: a value strictly between 0 and 1 draws a random label mask (training only)")
        elif self.cfg.label_cond:
            raise ValueError("a DiT built with label_cond=True needs `classes` on the device path")
        hd = self.native(x.device)
        if classes is not None:
            hd.set_condition(classes, x.device, null_labels=bool(cdp), cond_scale=1.0)
        xin = x.detach().to(torch.float32).contiguous()
        tin = t.detach().to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
        if tin.numel() != xin.shape[0]:
            raise ValueError("t must have one entry per batch element")
        with torch.cuda.device(x.device):
            return hd.net_forward(xin, tin).to(x.dtype)
