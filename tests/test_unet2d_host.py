"""CPU: the UNet2dBase plugin's contract without a device -- the state_dict layout against oracle/unet2d.py (which the reference's fixtures pin),
strict loading of reference-layout weights, the constructor's refusals of every branch the device path does not run, and the C-ABI struct."""
import ctypes as C
import json
import os

import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
from oracle import unet2d as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def three_level(num_classes=0):
    return U.UNet2dConfig(dim=128, num_classes=num_classes, dim_mults=(1, 2, 2), channels=2, num_resnet_blocks=1, resnet_groups=8,
                          layer_attns=(False, True, True), layer_cross_attns=(False, True, False), attn_heads=4, ff_mult=1.5,
                          layer_attns_depth=2, memory_efficient=True, scale_skip_connection=False, init_cross_embed_kernel_sizes=(5, 3))


@pytest.mark.parametrize("cfg", [U.config_sc09(0), U.config_sc09(10), three_level(), three_level(3)], ids=["sc09_0", "sc09_10", "l3", "l3_cls"])
def test_state_dict_layout_equals_the_oracle_and_loads_strictly(cfg):
    net = A.UNet2dBase(**cfg.to_kwargs())
    sd, specs = net.state_dict(), U.param_specs(cfg)
    assert list(sd) == list(specs)
    assert all(tuple(sd[k].shape) == specs[k][0] for k in specs)
    assert float(sd["final_conv.weight"].abs().max()) == 0.0                # zero_init_(final_conv), :874-876
    net.load_state_dict(U.generate_weights(cfg, 5), strict=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 2, 32, 32), torch.zeros(1), classes=torch.zeros(1, dtype=torch.long) if cfg.num_classes else None)


def test_shipped_net_counts_match_the_reference_report():
    rep = json.load(open(os.path.join(ROOT, "tests", "golden", "unet2d_golden_report.json")))["sc09"]
    net = A.UNet2dBase(**U.config_sc09(10).to_kwargs())
    sd = net.state_dict()
    assert (len(sd), sum(p.numel() for p in net.parameters())) == (rep["tensors"], rep["params"]) == (519, 47279260)
    # the shipped yaml passes lists and a bool for the per-level flags; a bool fans out to every level (cast_tuple)
    kw = {**U.config_sc09(0).to_kwargs(), "layer_attns": [False, False, True, True], "layer_cross_attns": False}
    assert A.UNet2dBase(**kw).cfg.layer_cross_attns == (False,) * 4


_BASE = U.config_sc09(0).to_kwargs()


@pytest.mark.parametrize("kw, what", [
    ({"cond_on_text": True}, "cond_on_text"), ({"use_linear_attn": True}, "use_linear_attn"),
    ({"use_linear_cross_attn": True}, "use_linear_cross_attn"), ({"cross_embed_downsample": True}, "cross_embed_downsample"),
    ({"use_condition_block": True}, "use_condition_block"), ({"init_conv_to_final_conv_residual": True}, "init_conv_to_final_conv_residual"),
    ({"combine_upsample_fmaps": True}, "combine_upsample_fmaps"), ({"class_embed_dim": 64}, "class_embed_dim"),
    ({"memory_efficient": False}, "memory_efficient"), ({"pixel_shuffle_upsample": False}, "pixel_shuffle_upsample"),
    ({"use_global_context_attn": False}, "use_global_context_attn"), ({"init_cross_embed": False}, "init_cross_embed"),
])
def test_unsupported_branches_raise_naming_the_argument(kw, what):
    with pytest.raises(NotImplementedError, match=what):
        A.UNet2dBase(**{**_BASE, **kw})


@pytest.mark.parametrize("dtype", ["bf16", "f32x3", "bfloat16"])
def test_only_the_exact_fp32_mode_is_built(dtype):
    with pytest.raises(ValueError, match="bf16 is not built for this net"):
        A.UNet2dBase(**_BASE, compute_dtype=dtype)
    A.UNet2dBase(**_BASE, compute_dtype="fp32")


@pytest.mark.parametrize("kw, what", [
    ({"dim": 136}, "dim"), ({"dim_mults": (1, 2, 4, 8), "layer_attns": False}, "dim_mults"),
    ({"attn_heads": 16}, "attn_heads"), ({"ff_mult": 1.1}, "ff_mult"), ({"channels_out": 5}, "channels_out"),
    ({"init_cross_embed_kernel_sizes": (3, 6)}, "init_cross_embed_kernel_sizes"),
])
def test_unsupported_widths_raise_value_error(kw, what):
    with pytest.raises(ValueError, match=what):
        A.UNet2dBase(**{**_BASE, **kw})


def test_forward_refuses_text_and_bad_shapes_before_touching_a_device():
    net = A.UNet2dBase(**_BASE)
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 2, 32, 32), torch.zeros(1), text_embeds=torch.zeros(1, 3, 768))
    with pytest.raises(ValueError, match="multiples of 2"):
        net(torch.zeros(1, 2, 24, 32), torch.zeros(1))
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 32, 32), torch.zeros(1))


def test_abi_struct_layout_and_packing():
    assert C.sizeof(_lib.AdfUNet2dConfig) == 8 + 4 * (5 + 1 + 3 * 8 + 3 + 3 + 1 + 4 + 2 + 2 + 1)          # one double, 46 int32
    cfg = A.UNet2dConfig(dim=128, num_classes=10, num_resnet_blocks=2, dim_mults=(1, 2, 2, 2), channels=2, attn_heads=2,
                         layer_attns=(False, False, True, True), layer_cross_attns=(False, False, True, True), init_cross_embed_kernel_sizes=(15, 3, 7))
    c = _lib.make_unet2d_config(cfg, _lib.DTYPE_F32)
    assert (c.dim, c.cond_dim, c.channels_out, c.n_levels, list(c.dim_mults)[:4], list(c.layer_attns)[:4]) == (128, 128, 2, 4, [1, 2, 2, 2], [0, 0, 1, 1])
    assert (c.n_init_kernels, list(c.init_kernel_sizes)[:3], c.ff_mult, c.num_classes) == (3, [3, 7, 15], 2.0, 10)
    assert [k for k, _ in A.unet2d_config.param_specs(cfg).items()] == list(U.param_specs(U.config_sc09(10)))
