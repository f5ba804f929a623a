"""CPU: the plugin contract of ``audiodiffuser_amd.DACEncoder`` and ``FineTuneAutoencoder.encode`` / ``.forward`` without a device -- state-dict layout
against the reference's (recorded by tools/gen_golden_dac_enc.py in tests/golden/dac_enc_golden_report.json), strict load of an ``encoder.``-stripped
checkpoint slice, every refusal by exception type and named argument, ``output_length``, and the C ABI additions (``ADF_DAC_KIND_ENCODER``,
``adf_dac_encode``) against the header."""
import ctypes as C
import inspect
import json
import os
import re

import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib, build
from audiodiffuser_amd.dac import make_dac_config
import dac_enc_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report():
    with open(os.path.join(ROOT, "tests", "golden", "dac_enc_golden_report.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")) as f:
        return f.read()


def make(case):
    return A.FineTuneAutoencoder(**ER.ctor_kwargs(case)) if ER.kind(case) == "ae" else A.DACEncoder(**ER.ctor_kwargs(case))


@pytest.mark.parametrize("case", ER.GOLDEN_CASES)
def test_state_dict_names_shapes_and_order_are_the_references(report, case):
    mine = [[k, list(v.shape)] for k, v in make(case).state_dict().items()]
    assert mine == report["cases"][case]["state_dict"]


def test_state_dict_key_families_of_the_encoder():
    keys = list(A.DACEncoder(32, [2, 5], 64).state_dict())
    assert keys[:3] == ["block.0.bias", "block.0.weight_g", "block.0.weight_v"]
    assert keys[3:11] == [f"block.1.block.0.block.{k}" for k in ("0.alpha", "1.bias", "1.weight_g", "1.weight_v", "2.alpha", "3.bias", "3.weight_g", "3.weight_v")]
    assert keys[27:31] == ["block.1.block.3.alpha", "block.1.block.4.bias", "block.1.block.4.weight_g", "block.1.block.4.weight_v"]
    assert keys[-4:] == ["block.3.alpha", "block.4.bias", "block.4.weight_g", "block.4.weight_v"]
    sd = A.DACEncoder(32, [2, 5], 64).state_dict()
    assert tuple(sd["block.2.block.4.weight_v"].shape) == (128, 64, 10) and tuple(sd["block.2.block.4.weight_g"].shape) == (128, 1, 1)
    assert tuple(sd["block.0.weight_v"].shape) == (32, 1, 7) and tuple(sd["block.4.weight_v"].shape) == (64, 128, 3)


def test_constructor_signature_defaults_and_enc_dim_are_the_references(report):
    ref = [p.split(":")[0].split("=")[0].strip() for p in report["signature"]["Encoder"].strip("()").split(",")][1:]
    d = inspect.signature(A.DACEncoder.__init__).parameters
    assert [n for n in d if n != "self"] == ["d_model", "strides", "d_latent"] and ref[:1] == ["d_model"]
    assert all(n in report["signature"]["Encoder"] for n in ("d_model", "strides", "d_latent"))
    assert (d["d_model"].default, d["strides"].default, d["d_latent"].default) == (64, [2, 4, 8, 8], 64)
    assert A.DACEncoder().enc_dim == 1024 and A.DACEncoder(32, [3], 32).enc_dim == 64
    for fn in ("encode", "forward"):
        p = inspect.signature(getattr(A.FineTuneAutoencoder, fn)).parameters
        assert list(p) == ["self", "x", "is_train"] and p["is_train"].default is True
        assert "is_train=True" in report["signature"][f"FineTuneAutoencoder.{fn}"]
        assert "is_train=False" in getattr(A.FineTuneAutoencoder, fn).__doc__
    assert "is_train=False" in A.FineTuneAutoencoder.__doc__


def test_a_checkpoint_slice_strict_loads_after_the_prefix_strip_and_a_missing_key_is_refused():
    net, w = make("odd"), ER.weights("odd")
    ckpt = {"encoder." + k: v for k, v in w.items()}
    ckpt["decoder.model.0.bias"] = torch.zeros(3)
    sl = {k[len("encoder."):]: v for k, v in ckpt.items() if k.startswith("encoder.")}
    assert net.load_state_dict(sl, strict=True).missing_keys == []
    assert all(torch.equal(net.state_dict()[k], v) for k, v in w.items())
    key = "block.2.block.4.weight_g"
    sl.pop(key)
    with pytest.raises(RuntimeError, match=re.escape(key)):
        net.load_state_dict(sl, strict=True)


def test_fresh_module_is_weight_norm_at_its_initial_point():
    sd = A.DACEncoder(32, [4], 32).state_dict()
    for k, g in sd.items():
        if k.endswith(".weight_g"):
            assert torch.allclose(g.flatten(), sd[k[:-1] + "v"].flatten(1).norm(dim=1))
        if k.endswith(".alpha"):
            assert bool((g == 1).all())


@pytest.mark.parametrize("args,names", [
    ((48, [2], 64), "d_model"),
    ((16, [2], 64), "d_model"),
    ((512, [2] * 5, 64), "d_model"),                      # 512 * 32 > 8192
    ((32, [], 64), "strides"),
    ((32, [2] * 7, 64), "strides"),
    ((32, [1], 64), "strides"),
    ((32, [17], 64), "strides"),
    ((32, [2.5], 64), "strides"),
    ((32, [2], 8), "d_latent"),
    ((32, [2], 48), "d_latent"),
    ((32, [2], 16384), "d_latent"),
])
def test_encoder_refusals_name_their_argument(args, names):
    with pytest.raises(ValueError, match=names):
        A.DACEncoder(*args)


def test_served_widths_construct():
    for args in ((64, [2, 4, 8, 8], 1024), (32, [16] * 6, 32), (4096, [3], 8192), (96, [2], 32)):
        A.DACEncoder(*args)
    A.FineTuneAutoencoder(intermediate_embedding_size=[1024, 64], latent_dim=8, tanh_btnk=True)
    # latent_dim above 1024 (encode's mean is then wider than decode's result) stays served up to 2048, and refused by name beyond
    ae = A.FineTuneAutoencoder(intermediate_embedding_size=[1024, 64], latent_dim=2048)
    assert make_dac_config(ae.cfg, _lib.DTYPE_F32).input_channel == 2048 and tuple(ae.state_dict()["btnk_layer.weight"].shape) == (4096, 64, 1)
    with pytest.raises(ValueError, match="latent_dim"):
        A.FineTuneAutoencoder(intermediate_embedding_size=[1024, 64], latent_dim=2052)


def test_output_length_on_the_host():
    enc = A.DACEncoder(32, [4, 5, 2], 32)
    assert [enc.output_length(L) for L in (47, 523)] == [1, 13]
    assert A.DACEncoder().output_length(32768) == 64 and A.DACEncoder(64, [2, 4, 8, 8], 1024).output_length(44100) == 86
    assert A.DACEncoder(32, [5], 32).output_length(49) == 10          # odd s: (L + 1) // s
    for case in ER.ENCODER_CASES:
        assert make(case).output_length(ER.CASES[case][3]) == ER.LENGTHS[case][-1]
    with pytest.raises(ValueError, match=r"L is too short.*stage 2 \(stride 2\)"):
        enc.output_length(35)                                          # 35 -> 8 -> 1, and the stride-2 conv needs 2
    with pytest.raises(ValueError, match=r"L is too short.*stage 0"):
        enc.output_length(3)


def test_refusals_before_any_device_call():
    enc, ae = A.DACEncoder(32, [4], 32), A.FineTuneAutoencoder(intermediate_embedding_size=[1024, 64], latent_dim=8)
    with pytest.raises(ValueError, match="audio must be shaped"):
        enc(torch.zeros(1, 2, 64))
    with pytest.raises(ValueError, match="L is too short"):
        enc(torch.zeros(1, 1, 3))
    with pytest.raises(NotImplementedError, match="no backward"):
        enc(torch.zeros(1, 1, 64, requires_grad=True))
    with pytest.raises(NotImplementedError, match="no backward"):
        ae.encode(torch.zeros(1, 1024, 5, requires_grad=True), is_train=False)
    with pytest.raises(ValueError, match="x must be shaped"):
        ae.encode(torch.zeros(1, 8, 5), is_train=False)
    # is_train=True (the default) is refused first, whatever the tensor is: sampling is training-side
    with pytest.raises(NotImplementedError, match="is_train=False"):
        ae.encode(torch.zeros(1, 8, 5))
    with pytest.raises(NotImplementedError, match="is_train=False"):
        ae(torch.zeros(1, 8, 5), is_train=True)
    with pytest.raises(RuntimeError, match="ROCm device"):          # everything passed: the only thing missing is the device
        enc(torch.zeros(1, 1, 64))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ae.encode(torch.zeros(1, 1024, 5), is_train=False)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ae(torch.zeros(1, 1024, 5), is_train=False)


def test_header_declares_and_library_exports_adf_dac_encode(header):
    lib = _lib.load_library()
    assert hasattr(lib, "adf_dac_encode") and "adf_dac_encode" in _lib.EXPORTS
    assert re.search(r"\bint\s+adf_dac_encode\s*\(\s*adf_handle\s*\*\s*h\s*,\s*const\s+float\s*\*\s*in\s*,\s*int\s+B\s*,\s*int\s+T\s*,\s*float\s*\*\s*mean_out\s*,"
                     r"\s*float\s*\*\s*kl_out\s*,\s*void\s*\*\s*stream\s*\)", header)
    assert _lib.EXPORTS["adf_dac_encode"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    assert re.search(r"Added without a bump[^*]*\*?[^*]*adf_dac_encode and ADF_DAC_KIND_ENCODER", header)


def test_kind_constants_match_the_header_and_the_layout_is_unchanged(header):
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (ADF_DAC_\w+) (\d+)", header)}
    assert (consts["ADF_DAC_KIND_DECODER"], consts["ADF_DAC_KIND_AUTOENCODER"], consts["ADF_DAC_KIND_ENCODER"]) == \
        (_lib.DAC_KIND_DECODER, _lib.DAC_KIND_AUTOENCODER, _lib.DAC_KIND_ENCODER) == (0, 1, 2)
    assert consts["ADF_DAC_BTNK_TANH"] == _lib.DAC_BTNK_TANH
    assert [n for n, _ in _lib.AdfDacConfig._fields_] == ["kind", "input_channel", "channels", "n_rates", "rates", "d_out", "n_widths", "widths", "dtype"]
    assert C.sizeof(_lib.AdfDacConfig) == 4 * (7 + 6 + 8)


def test_make_dac_config_carries_the_constructor_arguments():
    c = make_dac_config(ER.config("odd"), _lib.DTYPE_F32)
    assert (c.kind, c.input_channel, c.channels, c.n_rates, list(c.rates)[:3], c.d_out, c.n_widths, c.dtype) == (2, 1, 32, 3, [2, 5, 4], 64, 0, 0)
    assert make_dac_config(make("odd").cfg, _lib.DTYPE_F32).kind == 2
    assert make_dac_config(make("ae_tanh").cfg, _lib.DTYPE_F32).d_out == _lib.DAC_BTNK_TANH
    assert make_dac_config(make("ae").cfg, _lib.DTYPE_F32).d_out != _lib.DAC_BTNK_TANH


def test_abi_version_stays_7(header):
    assert _lib.load_library().adf_abi_version() == 7 and _lib.ABI_VERSION == 7 and re.search(r"#define ADF_ABI_VERSION 7\b", header)


def test_exported_from_the_package_and_no_new_source_files():
    assert A.DACEncoder is A.dac.DACEncoder
    assert "adf_dac.hip" in build.SOURCES and "adf_net_dac.hip" in build.SOURCES and "adf_dac.h" in build.HEADERS


def test_create_without_a_device_or_with_bad_arguments_reports_by_name():
    lib = _lib.load_library()
    h = C.c_void_p()
    c = make_dac_config(ER.config("w96"), _lib.DTYPE_BF16)
    assert lib.adf_dac_create(C.byref(c), C.byref(h)) != 0 and not h.value
    msg = lib.adf_last_error(None).decode()
    assert msg.startswith("adf_dac_create: ") and ("dtype" in msg or "no HIP device" in msg)
