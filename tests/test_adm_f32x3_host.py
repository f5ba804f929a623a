"""The split-bf16 mode (compute_dtype="f32x3") at the plugin boundary, without a device: UNetModel takes it under the fp32 width rule, the C
configuration carries the third dtype value, and WaveNetNoise -- for which the mode is not built -- refuses it at construction instead of in
adf_wavenet_create at the first forward."""
import pytest

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib


def test_unet_model_takes_f32x3_under_the_fp32_width_rule():
    net = A.UNetModel(model_channels=48, compute_dtype="f32x3")          # (48 is refused for bf16: tests/test_adm.py)
    assert net.compute_dtype == "f32x3"
    assert "f32x3" in A.UNetModel.__doc__


def test_adm_config_carries_the_third_dtype():
    assert _lib.DTYPE_F32X3 == 2
    assert _lib.make_adm_config(A.config_c4(), _lib.DTYPE_F32X3).dtype == 2


def test_wavenet_refuses_f32x3_at_construction():
    with pytest.raises(ValueError, match="UNet1dBase and UNetModel"):
        A.WaveNetNoise(compute_dtype="f32x3")
    A.WaveNetNoise(residual_channels=64, residual_layers=2, dilation_cycle=2, compute_dtype="fp32")
