"""The refusals the library itself makes per handle kind (UNet1dBase, WaveNetNoise, UNetModel, UNet2dBase), called through the C ABI.

The Python layer raises its own ``ValueError`` before any of these (``NativeHandle._length``, ``unet2d.py``), so no other test reaches them.
Every case goes through ``NativeHandle.lib`` / ``.h`` on the smallest network of its kind with its weights loaded, B = 1, and asserts the
return code and the ``adf_last_error`` text; after each refusal the pass counter has not moved and one valid forward on the same handle
still succeeds and is finite.  None of the refused calls launches anything."""
import ctypes as C

import pytest
import torch

import audiodiffuser_amd as A
from oracle import unet2d as U

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def handle_of(net):
    net = net.cuda()
    return net, net.native(torch.device("cuda", torch.cuda.current_device()))       # uploads every state_dict tensor


def raw_forward(hd, cin, cout, L, shape):
    """adf_net_forward at B = 1 without the Python layer's own checks: (rc, output); ``shape`` is what L is meant to cover."""
    g = torch.Generator().manual_seed(11)
    x = (torch.randn((1, cin) + tuple(shape), generator=g) * 0.5).cuda()
    t = torch.tensor([0.35]).cuda()
    out = torch.zeros((1, cout) + tuple(shape), device="cuda")
    rc = hd.lib.adf_net_forward(hd.h, _p(x), _p(t), _p(out), 1, L, _stream())
    torch.cuda.synchronize()
    return rc, out


def refused(hd, rc, text):
    assert rc != 0
    msg = hd.lib.adf_last_error(hd.h).decode()
    assert text in msg, msg


def still_works(hd, before, cin, cout, L, shape):
    """The refusals left the pass counter alone; one valid forward then succeeds, is finite and counts."""
    assert hd.counters()["net_passes"] == before
    rc, out = raw_forward(hd, cin, cout, L, shape)
    assert rc == 0, hd.lib.adf_last_error(hd.h).decode()
    assert bool(torch.isfinite(out).all())
    assert hd.counters()["net_passes"] > before


def test_unet1d_handle_refusals():
    cfg = A.config_tiny()
    _, hd = handle_of(A.UNet1dBase.from_config(cfg))
    total = cfg.total_downsample
    rc, _ = raw_forward(hd, 1, 1, total, (total,))                      # (a plan exists: the counter below only sees the refusals)
    assert rc == 0
    before = hd.counters()["net_passes"]
    refused(hd, hd.lib.adf_set_image_shape(hd.h, 16, 16), "not a UNetModel / UNet2dBase handle")
    rc, _ = raw_forward(hd, 1, 1, 2 * total - 1, (2 * total - 1,))
    refused(hd, rc, "positive multiple")
    if hasattr(hd.lib, "adf_bench_wavenet_layer"):
        ms, by, fl = C.c_float(), C.c_double(), C.c_double()
        rc = hd.lib.adf_bench_wavenet_layer(hd.h, 1, total, 0, 1, C.byref(ms), C.byref(by), C.byref(fl), _stream())
        refused(hd, rc, "not a WaveNetNoise handle")
    still_works(hd, before, 1, 1, 2 * total, (2 * total,))


def test_wavenet_handle_refuses_an_image_shape():
    _, hd = handle_of(A.WaveNetNoise.from_config(A.config_c5_small()))
    before = hd.counters()["net_passes"]
    refused(hd, hd.lib.adf_set_image_shape(hd.h, 16, 16), "not a UNetModel / UNet2dBase handle")
    still_works(hd, before, 1, 1, 96, (96,))


def test_adm_handle_refusals():
    _, hd = handle_of(A.UNetModel.from_config(A.config_c4_small()))
    before = hd.counters()["net_passes"]
    rc, _ = raw_forward(hd, 1, 1, 16 * 32, (16, 32))                    # no adf_set_image_shape yet
    refused(hd, rc, "call adf_set_image_shape")
    assert hd.lib.adf_set_image_shape(hd.h, 16, 32) == 0
    rc, _ = raw_forward(hd, 1, 1, 16 * 16, (16, 16))                    # H * W != L
    refused(hd, rc, "with H * W equal to the length argument")
    assert hd.lib.adf_set_image_shape(hd.h, 8, 8) == 0
    rc, _ = raw_forward(hd, 1, 1, 8 * 8, (8, 8))                        # two levels: the coarsest is 4 x 4 = 16 pixels
    refused(hd, rc, "the coarsest level a multiple of 64 pixels")
    assert hd.lib.adf_set_image_shape(hd.h, 16, 32) == 0
    still_works(hd, before, 1, 1, 16 * 32, (16, 32))


def test_unet2d_handle_refusals():
    # the `fg2` structure of tests/test_unet2d_sweep_gpu.py: two levels (H and W multiples of 4)
    cfg = U.UNet2dConfig(memory_efficient=True, dim=192, dim_mults=(1, 2), channels=4, channels_out=2, num_resnet_blocks=1, resnet_groups=32,
                         layer_attns=(False, True), layer_cross_attns=(False, True), attn_heads=3, init_cross_embed_kernel_sizes=(7,))
    _, hd = handle_of(A.UNet2dBase(**cfg.to_kwargs()))
    before = hd.counters()["net_passes"]
    rc, _ = raw_forward(hd, 4, 2, 8 * 8, (8, 8))                        # no adf_set_image_shape yet
    refused(hd, rc, "call adf_set_image_shape")
    assert hd.lib.adf_set_image_shape(hd.h, 6, 8) == 0
    rc, _ = raw_forward(hd, 4, 2, 6 * 8, (6, 8))                        # H = 6 is no multiple of 2^2
    refused(hd, rc, "H and W must be multiples of 2^levels")
    assert hd.lib.adf_set_image_shape(hd.h, 8, 8) == 0
    still_works(hd, before, 4, 2, 8 * 8, (8, 8))
