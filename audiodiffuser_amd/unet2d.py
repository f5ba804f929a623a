"""``model.net`` plugin: HIP-backed drop-in for the reference's Imagen-style 2-D U-Net ``UNet2dBase`` (src/models/backbones/unet2d.py:622-972),
the network of the shipped sc09 experiment files.

Contract kept: the constructor kwargs (hydra ``_target_`` instantiation), ``state_dict()`` keys / order / shapes (reference checkpoints
strict-load, the modules the forward never runs included), ``forward(x[B, C, H, W], time[B], classes=None, text_embeds=None, text_mask=None,
cond_drop_prob=None, inj_channels=None) -> [B, channels_out, H, W]``.  On the device, in exact fp32: the memory-efficient layout with the cross-embed
initial conv, global-context gates, pixel-shuffle upsampling, the final resnet block, either skip scaling, any level / block / attention layout,
class-conditional or not.  Every other constructor branch raises here, naming its argument.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from .net import HipNet
from .unet2d_config import UNet2dConfig, param_specs


def _cast_tuple(val, n: int, name: str):
    """utils.py:43-52 (cast_tuple): a bool for every level, or one entry per level."""
    out = tuple(val) if isinstance(val, (list, tuple)) else (val,) * n
    if len(out) != n:
        raise ValueError(f"{name} needs one entry per level of dim_mults ({n}), got {len(out)}")
    return tuple(bool(v) for v in out)


def _init_like_reference(name: str, shape, kind: str) -> torch.Tensor:
    t = torch.empty(shape, dtype=torch.float32)
    if name.startswith("final_conv."):
        return t.zero_()                                  # zero_init_(self.final_conv), :874-876
    if kind in ("conv2d_w", "linear_w"):
        nn.init.kaiming_uniform_(t, a=math.sqrt(5))
        return t
    if kind == "norm_w":
        return t.fill_(1.0)
    if kind == "norm_b":
        return t.zero_()
    if kind in ("fourier", "embed"):
        return t.normal_()
    return t.uniform_(-0.05, 0.05)


class UNet2dBase(HipNet):
    """HIP-backed ``UNet2dBase``.  Extra kwarg: ``compute_dtype``, "fp32" only (exact fp32; the reduced-precision mode is not built for this net)."""

    def __init__(self, dim, num_classes=0, cond_drop_prob=0.0, num_resnet_blocks=1, cond_dim=None, num_time_tokens=2, learned_sinu_pos_emb_dim=16,
                 dim_mults=(1, 2, 4, 8), channels=3, channels_out=None, attn_heads=8, ff_mult=2.0, layer_attns=True, layer_attns_depth=1,
                 layer_mid_attns_depth=1, attend_at_middle=True, layer_cross_attns=True, use_linear_attn=False, use_linear_cross_attn=False,
                 text_embed_dim=768, class_embed_dim=None, cond_on_text=False, max_text_len=3, init_dim=None, resnet_groups=8,
                 init_conv_kernel_size=7, init_cross_embed=True, init_cross_embed_kernel_sizes=(3, 7, 15), cross_embed_downsample=False,
                 cross_embed_downsample_kernel_sizes=(2, 4), memory_efficient=False, init_conv_to_final_conv_residual=False,
                 use_global_context_attn=True, scale_skip_connection=True, final_resnet_block=True, final_conv_kernel_size=3,
                 resize_mode="nearest", combine_upsample_fmaps=False, pixel_shuffle_upsample=True, use_condition_block=False,
                 channel_infuse_mode=None, compute_dtype: str = "fp32"):
        super().__init__()
        if compute_dtype != "fp32":
            raise ValueError(f"compute_dtype={compute_dtype!r}: UNet2dBase runs in exact fp32 only ('fp32'); bf16 is not built for this net yet")
        assert attn_heads > 1, "you need to have more than 1 attention head"                      # :670-671
        assert dim > 100
        # constructor branches the device path does not run: refuse them by name instead of computing something else
        unsupported = {
            "cond_on_text": cond_on_text, "use_linear_attn": use_linear_attn, "use_linear_cross_attn": use_linear_cross_attn,
            "cross_embed_downsample": cross_embed_downsample, "use_condition_block": use_condition_block,
            "channel_infuse_mode": channel_infuse_mode is not None, "init_conv_to_final_conv_residual": init_conv_to_final_conv_residual,
            "combine_upsample_fmaps": combine_upsample_fmaps, "class_embed_dim": class_embed_dim is not None,
            "memory_efficient=False": not memory_efficient, "pixel_shuffle_upsample=False (nearest upsampling)": not pixel_shuffle_upsample,
            "use_global_context_attn=False": not use_global_context_attn, "init_cross_embed=False": not init_cross_embed,
            "init_dim other than dim": init_dim is not None and init_dim != dim, "final_conv_kernel_size other than 3": final_conv_kernel_size != 3,
        }
        for what, on in unsupported.items():
            if on:
                raise NotImplementedError(f"UNet2dBase({what}) is not on the device path (the memory-efficient, cross-embed, "
                                          "global-context, pixel-shuffle layout of the shipped configs is)")
        n = len(dim_mults)
        cfg = UNet2dConfig(dim=dim, num_classes=int(num_classes or 0), num_resnet_blocks=num_resnet_blocks, cond_dim=cond_dim,
                           num_time_tokens=num_time_tokens, learned_sinu_pos_emb_dim=learned_sinu_pos_emb_dim,
                           dim_mults=tuple(int(m) for m in dim_mults), channels=channels, channels_out=channels_out, attn_heads=attn_heads,
                           ff_mult=float(ff_mult), layer_attns=_cast_tuple(layer_attns, n, "layer_attns"), layer_attns_depth=layer_attns_depth,
                           layer_mid_attns_depth=layer_mid_attns_depth, attend_at_middle=bool(attend_at_middle),
                           layer_cross_attns=_cast_tuple(layer_cross_attns, n, "layer_cross_attns"), resnet_groups=resnet_groups,
                           init_cross_embed_kernel_sizes=tuple(init_cross_embed_kernel_sizes), scale_skip_connection=bool(scale_skip_connection),
                           final_resnet_block=bool(final_resnet_block))
        _check_widths(cfg)
        self.cfg = cfg
        self.compute_dtype = compute_dtype
        self.cond_drop_prob = cond_drop_prob
        for name, (shape, kind) in param_specs(cfg).items():
            self._register(name, nn.Parameter(_init_like_reference(name, shape, kind)))

    def forward(self, x: torch.Tensor, time: torch.Tensor, classes: Optional[torch.Tensor] = None, text_embeds=None, text_mask=None,
                cond_drop_prob=None, inj_channels=None) -> torch.Tensor:
        if text_embeds is not None or inj_channels is not None:
            raise NotImplementedError("text embeddings / injected channels are not on the device path of UNet2dBase")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("the HIP UNet2dBase is an inference path (no backward); call it under torch.no_grad()")
        if x.ndim != 4 or x.shape[1] != self.cfg.channels:
            raise ValueError(f"x must be shaped [B, {self.cfg.channels}, H, W]")
        f = 2 ** len(self.cfg.dim_mults)
        if x.shape[2] % f or x.shape[3] % f:
            raise ValueError(f"H and W must be multiples of 2^levels = {f}")
        hd = self.native(x.device)
        if self.cfg.num_classes:
            assert classes is not None                                                               # :902
            cdp = self.cond_drop_prob if cond_drop_prob is None else cond_drop_prob
            if cdp not in (0, 0.0, 1, 1.0):
                raise NotImplementedError("cond_drop_prob other than 0 or 1 draws a random label mask (training only)")
            hd.set_condition(classes, x.device, null_labels=bool(cdp), cond_scale=1.0)
        xin = x.detach().to(torch.float32).contiguous()
        tin = time.detach().to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
        if tin.numel() != xin.shape[0]:
            raise ValueError("time must have one entry per batch element")
        with torch.cuda.device(x.device):
            return hd.net_forward(xin, tin).to(x.dtype)


def _check_widths(cfg: UNet2dConfig) -> None:
    """What the exact-fp32 kernels are built for (adf_unet2d.h, adf_conv2d.h), reported against the constructor argument that sets it."""
    if cfg.dim % 32:
        raise ValueError(f"dim={cfg.dim}: every width must be a multiple of 32 channels")
    for m in cfg.dim_mults:
        if m < 1 or (cfg.dim * m) > 512:
            raise ValueError(f"dim_mults={cfg.dim_mults}: level widths dim * mult must lie in [32, 512] (a skip concat feeds a conv of at most 1024 channels)")
        if (cfg.dim * m) % cfg.resnet_groups or (2 * cfg.dim * m) % cfg.resnet_groups:
            raise ValueError(f"resnet_groups={cfg.resnet_groups} must divide every level width")
    if cfg.cdim > 512 or (cfg.num_classes and cfg.cdim != cfg.dim):
        raise ValueError(f"cond_dim={cfg.cond_dim}: at most 512, and equal to dim with num_classes (t + the label embedding, :902-908)")
    if cfg.learned_sinu_pos_emb_dim % 2:
        raise ValueError("learned_sinu_pos_emb_dim must be even")                                  # LearnedSinusoidalPosEmb :71
    if cfg.out_channels > 4:
        raise ValueError(f"channels_out={cfg.out_channels}: the final conv kernel serves 1 to 4 channels")
    ks = sorted(cfg.init_cross_embed_kernel_sizes)
    if not 1 <= len(ks) <= 4 or any(k % 2 == 0 for k in ks):
        raise ValueError(f"init_cross_embed_kernel_sizes={tuple(cfg.init_cross_embed_kernel_sizes)}: one to four odd kernel sizes")
    widths = [cfg.dim * m for m, a in zip(cfg.dim_mults, cfg.layer_attns) if a]
    if cfg.attend_at_middle:
        widths.append(cfg.dims[-1])
    for w in widths:
        if w % cfg.attn_heads or w // cfg.attn_heads not in (32, 64, 128):
            raise ValueError(f"attn_heads={cfg.attn_heads}: the attention head dim ({w} channels / heads) must be 32, 64 or 128")
    for w, mult in [(cfg.dim * m, cfg.ff_mult) for m, a in zip(cfg.dim_mults, cfg.layer_attns) if a] + ([(cfg.dims[-1], 2)] if cfg.attend_at_middle else []):
        hid = int(w * mult)
        if hid % 32 or hid > 1024:
            raise ValueError(f"ff_mult={cfg.ff_mult}: the feed-forward width int({w} * ff_mult) = {hid} must be a multiple of 32, at most 1024")
