"""Configuration and ``state_dict`` layout of the reference's Imagen-style 2-D U-Net ``UNet2dBase`` (src/models/backbones/unet2d.py:622-876),
the ``model.net`` of the shipped sc09 experiment files.  Shared by the plugin (audiodiffuser_amd/unet2d.py) and the C-ABI registry order
(adf_net_unet2d.hip registers the same tensors in the same order)."""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import List, Optional, Tuple

Spec = Tuple[Tuple[int, ...], str]


@dataclass
class UNet2dConfig:
    """The constructor arguments (:623-667) that shape the state dict and the forward the device runs, same names and defaults."""
    dim: int = 128
    num_classes: int = 0
    num_resnet_blocks: int = 1
    cond_dim: Optional[int] = None
    num_time_tokens: int = 2
    learned_sinu_pos_emb_dim: int = 16
    dim_mults: Tuple[int, ...] = (1, 2, 4, 8)
    channels: int = 3
    channels_out: Optional[int] = None
    attn_heads: int = 8
    ff_mult: float = 2.0
    layer_attns: Tuple[bool, ...] = (True, True, True, True)
    layer_attns_depth: int = 1
    layer_mid_attns_depth: int = 1
    attend_at_middle: bool = True
    layer_cross_attns: Tuple[bool, ...] = (True, True, True, True)
    resnet_groups: int = 8
    init_cross_embed_kernel_sizes: Tuple[int, ...] = (3, 7, 15)
    scale_skip_connection: bool = True
    final_resnet_block: bool = True

    # what the shared denoise / sampler / handle code asks of a network config
    @property
    def class_cond(self) -> bool:
        return self.num_classes > 0

    @property
    def in_channels(self) -> int:
        return self.channels

    @property
    def out_channels(self) -> int:
        return self.channels_out if self.channels_out is not None else self.channels

    # derived widths (:672-676, :692-693)
    @property
    def dims(self) -> List[int]:
        return [self.dim] + [self.dim * m for m in self.dim_mults]

    @property
    def cdim(self) -> int:
        return self.cond_dim if self.cond_dim is not None else self.dim

    @property
    def time_cond_dim(self) -> int:
        return 4 * self.cdim

    @property
    def cross_embed_dims(self) -> List[int]:
        """CrossEmbedLayer (:268-272): init_dim / 2, / 4, ... over the sorted kernel sizes, the remainder to the largest."""
        n = len(self.init_cross_embed_kernel_sizes)
        s = [int(self.dim / (2 ** i)) for i in range(1, n)]
        return s + [self.dim - sum(s)]


def config_sc09(num_classes: int = 10) -> UNet2dConfig:
    """``net:`` of the shipped sc09 experiment files (e.g. sc09_inference/diffunet_complex_sc09_eval_dpm.yaml): the 2-channel complex STFT,
    256 x 128 per sample."""
    return UNet2dConfig(dim=128, num_classes=num_classes, num_resnet_blocks=2, dim_mults=(1, 2, 2, 2), channels=2, attn_heads=2, ff_mult=2.0,
                        layer_attns=(False, False, True, True), layer_cross_attns=(False, False, True, True), resnet_groups=8)


# ------------------------------------------------------------------ state_dict layout (registration order of __init__, memory-efficient layout)
def _resnet(o: "OrderedDict[str, Spec]", pre: str, din: int, dout: int, tcd: int, cross_dim: Optional[int], gca: bool) -> None:
    """ResnetBlock.__init__ :106-144: time_mlp, cross_attn (never run without text), block1, block2, gca, res_conv."""
    o[f"{pre}.time_mlp.1.weight"] = ((2 * dout, tcd), "linear_w")
    o[f"{pre}.time_mlp.1.bias"] = ((2 * dout,), "bias")
    if cross_dim is not None:
        o[f"{pre}.cross_attn.to_q.weight"] = ((dout, dout), "linear_w")
        o[f"{pre}.cross_attn.to_kv.weight"] = ((2 * dout, dout), "linear_w")
        o[f"{pre}.cross_attn.to_context.weight"] = ((2 * dout, cross_dim), "linear_w")
        o[f"{pre}.cross_attn.to_out.weight"] = ((dout, dout), "linear_w")
    for blk, ci in (("block1", din), ("block2", dout)):
        o[f"{pre}.{blk}.groupnorm.weight"] = ((ci,), "norm_w")
        o[f"{pre}.{blk}.groupnorm.bias"] = ((ci,), "norm_b")
        o[f"{pre}.{blk}.project.weight"] = ((dout, ci, 3, 3), "conv2d_w")
        o[f"{pre}.{blk}.project.bias"] = ((dout,), "bias")
    if gca:
        hid = max(3, dout // 2)
        for name, shape in (("to_k.weight", (1, dout, 1, 1)), ("to_k.bias", (1,)), ("net.0.weight", (hid, dout, 1, 1)), ("net.0.bias", (hid,)),
                            ("net.2.weight", (dout, hid, 1, 1)), ("net.2.bias", (dout,))):
            o[f"{pre}.gca.{name}"] = (shape, "bias" if name.endswith("bias") else "conv2d_w")
    if din != dout:
        o[f"{pre}.res_conv.weight"] = ((dout, din, 1, 1), "conv2d_w")
        o[f"{pre}.res_conv.bias"] = ((dout,), "bias")


def _transformer(o: "OrderedDict[str, Spec]", pre: str, dim: int, depth: int, ff_mult: float, context_dim: Optional[int]) -> None:
    """TransformerBlock.__init__ :198-217 (Attention attention_utils.py:96-110, FeedForward :186-194); ``norm`` after the layer list."""
    hid = int(dim * ff_mult)
    for d in range(depth):
        lp = f"{pre}.layers.{d}"
        o[f"{lp}.0.to_q.weight"] = ((dim, dim), "linear_w")
        o[f"{lp}.0.to_kv.weight"] = ((2 * dim, dim), "linear_w")
        if context_dim is not None:
            o[f"{lp}.0.to_context.weight"] = ((2 * dim, context_dim), "linear_w")
        o[f"{lp}.0.to_out.weight"] = ((dim, dim), "linear_w")
        o[f"{lp}.1.0.g"] = ((dim,), "norm_w")
        o[f"{lp}.1.1.weight"] = ((hid, dim), "linear_w")
        o[f"{lp}.1.3.g"] = ((hid,), "norm_w")
        o[f"{lp}.1.4.weight"] = ((dim, hid), "linear_w")
    o[f"{pre}.norm.g"] = ((dim,), "norm_w")


def param_specs(cfg: UNet2dConfig) -> "OrderedDict[str, Spec]":
    """Every ``UNet2dBase.state_dict()`` key with its shape, in registration order, for the layout the device runs (memory_efficient,
    cross-embed initial conv, global-context gates, pixel-shuffle upsampling)."""
    o: "OrderedDict[str, Spec]" = OrderedDict()
    dims, tcd, cd = cfg.dims, cfg.time_cond_dim, cfg.cdim
    n = len(cfg.dim_mults)
    for i, (k, ds) in enumerate(zip(sorted(cfg.init_cross_embed_kernel_sizes), cfg.cross_embed_dims)):       # :679-686
        o[f"init_conv.convs.{i}.weight"] = ((ds, cfg.channels, k, k), "conv2d_w")
        o[f"init_conv.convs.{i}.bias"] = ((ds,), "bias")
    o["to_time_hiddens.0.weights"] = ((cfg.learned_sinu_pos_emb_dim // 2,), "fourier")                       # :695-714
    o["to_time_hiddens.1.weight"] = ((tcd, cfg.learned_sinu_pos_emb_dim + 1), "linear_w")
    o["to_time_hiddens.1.bias"] = ((tcd,), "bias")
    o["to_time_cond.0.weight"] = ((tcd, tcd), "linear_w")
    o["to_time_cond.0.bias"] = ((tcd,), "bias")
    o["to_time_tokens.0.weight"] = ((cd * cfg.num_time_tokens, tcd), "linear_w")
    o["to_time_tokens.0.bias"] = ((cd * cfg.num_time_tokens,), "bias")
    if cfg.num_classes:                                                                                         # :717-727
        cdm = 4 * cfg.dim
        o["label_conditioner.null_classes_emb"] = ((1, cfg.dim), "embed")
        o["label_conditioner.label_emb.weight"] = ((cfg.num_classes, cfg.dim), "embed")
        o["label_conditioner.class_to_cond.0.weight"] = ((cfg.dim,), "norm_w")
        o["label_conditioner.class_to_cond.0.bias"] = ((cfg.dim,), "norm_b")
        o["label_conditioner.class_to_cond.1.weight"] = ((cdm, cfg.dim), "linear_w")
        o["label_conditioner.class_to_cond.1.bias"] = ((cdm,), "bias")
        o["label_conditioner.class_to_cond.3.weight"] = ((cdm, cdm), "linear_w")
        o["label_conditioner.class_to_cond.3.bias"] = ((cdm,), "bias")
    _resnet(o, "init_resnet_block", dims[0], dims[0], tcd, None, True)                                         # :756-762
    for i in range(n):                                                                                          # :783-815
        din, dout = dims[i], dims[i + 1]
        pre = f"downs.{i}.ds_block"
        o[f"{pre}.0.1.weight"] = ((dout, din * 4, 1, 1), "conv2d_w")
        o[f"{pre}.0.1.bias"] = ((dout,), "bias")
        _resnet(o, f"{pre}.1", dout, dout, tcd, cd if cfg.layer_cross_attns[i] else None, False)
        for j in range(cfg.num_resnet_blocks):
            _resnet(o, f"{pre}.2.{j}", dout, dout, tcd, None, True)
        if cfg.layer_attns[i]:
            _transformer(o, f"{pre}.3", dout, cfg.layer_attns_depth, cfg.ff_mult, cd)
    mid = dims[-1]                                                                                              # :817-823
    _resnet(o, "mid_block.mid_block1", mid, mid, tcd, cd, False)
    if cfg.attend_at_middle:
        _transformer(o, "mid_block.mid_attn", mid, cfg.layer_mid_attns_depth, 2, None)
    _resnet(o, "mid_block.mid_block2", mid, mid, tcd, cd, False)
    for i in range(n):                                                                                          # :831-851
        li = n - 1 - i
        din, dout = dims[li], dims[li + 1]
        pre = f"ups.{i}.us_block"
        _resnet(o, f"{pre}.0", 2 * dout, dout, tcd, cd if cfg.layer_cross_attns[li] else None, False)
        for j in range(cfg.num_resnet_blocks):
            _resnet(o, f"{pre}.1.{j}", 2 * dout, dout, tcd, None, True)
        if cfg.layer_attns[li]:
            _transformer(o, f"{pre}.2", dout, cfg.layer_attns_depth, cfg.ff_mult, cd)
        o[f"{pre}.3.net.0.weight"] = ((din * 4, dout, 1, 1), "conv2d_w")
        o[f"{pre}.3.net.0.bias"] = ((din * 4,), "bias")
    if cfg.final_resnet_block:                                                                                  # :866-872
        _resnet(o, "final_res_block", cfg.dim, cfg.dim, tcd, None, True)
    o["final_conv.weight"] = ((cfg.out_channels, cfg.dim, 3, 3), "conv2d_w")
    o["final_conv.bias"] = ((cfg.out_channels,), "bias")
    return o
