"""CPU: the plugin contract of ``audiodiffuser_amd.DACDecoder`` / ``FineTuneAutoencoder`` without a device -- state-dict layout against the reference's
(recorded by tools/gen_golden_dac.py in tests/golden/dac_golden_report.json), strict load, every refusal by exception type and named argument, and the
C ABI additions (``adf_dac_config``, ``adf_dac_create``, ``adf_dac_forward``) against the header."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib, build
from audiodiffuser_amd.dac import make_dac_config
import dac_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report():
    with open(os.path.join(ROOT, "tests", "golden", "dac_golden_report.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")) as f:
        return f.read()


def make(case):
    return A.FineTuneAutoencoder(**DR.ctor_kwargs(case)) if DR.kind(case) == "ae" else A.DACDecoder(**DR.ctor_kwargs(case))


@pytest.mark.parametrize("case", DR.GOLDEN_CASES)
def test_state_dict_names_shapes_and_order_are_the_references(report, case):
    mine = [[k, list(v.shape)] for k, v in make(case).state_dict().items()]
    assert mine == report["cases"][case]["state_dict"]


def test_constructor_signatures_are_the_references_plus_compute_dtype(report):
    ref = [p.split(":")[0].split("=")[0].strip() for p in report["signature"]["Decoder"].strip("()").split(",")][1:]
    mine = [n for n in inspect.signature(A.DACDecoder.__init__).parameters if n != "self"]
    assert ref == ["input_channel", "channels", "rates", "d_out"] and mine == ref + ["compute_dtype"]
    d = inspect.signature(A.DACDecoder.__init__).parameters
    assert (d["d_out"].default, d["compute_dtype"].default) == (1, "fp32")
    ref = re.findall(r"(\w+)=", report["signature"]["FineTuneAutoencoder"])
    d = inspect.signature(A.FineTuneAutoencoder.__init__).parameters
    assert [n for n in d if n != "self"] == ref == ["intermediate_embedding_size", "conv_kernel", "tanh_btnk", "latent_dim"]
    assert (d["intermediate_embedding_size"].default, d["conv_kernel"].default, d["tanh_btnk"].default, d["latent_dim"].default) == \
        ([1024, 512, 256, 128], 3, False, 32)


@pytest.mark.parametrize("case,key", [("odd", "model.1.block.1.weight_g"), ("ae", "encoder_layers.1.weight_v")])
def test_strict_load_and_a_missing_key_is_refused(case, key):
    net, w = make(case), DR.weights(case)
    assert net.load_state_dict(w, strict=True).missing_keys == []
    assert all(torch.equal(net.state_dict()[k], v) for k, v in w.items())
    bad = dict(w)
    bad.pop(key)
    with pytest.raises(RuntimeError, match=re.escape(key)):
        net.load_state_dict(bad, strict=True)


def test_fresh_module_is_weight_norm_at_its_initial_point():
    """weight_norm starts at g = ||v|| (w = v) and Snake at alpha = 1; a ConvTranspose1d's g is per INPUT channel."""
    sd = A.DACDecoder(8, 64, [2]).state_dict()
    assert tuple(sd["model.1.block.1.weight_g"].shape) == (64, 1, 1) and tuple(sd["model.1.block.1.weight_v"].shape) == (64, 32, 4)
    for k, g in sd.items():
        if k.endswith(".weight_g"):
            assert torch.allclose(g.flatten(), sd[k[:-1] + "v"].flatten(1).norm(dim=1))
        if k.endswith(".alpha"):
            assert bool((g == 1).all())


@pytest.mark.parametrize("args,kw,names", [
    ((64, 96, [2]), {}, "channels"),                      # 96 / 2 = 48
    ((64, 256, [2, 2, 2, 2]), {}, "channels"),            # 256 / 16 = 16
    ((6, 64, [2]), {}, "input_channel"),
    ((2, 64, [2]), {}, "input_channel"),
    ((4096, 64, [2]), {}, "input_channel"),
    ((64, 64, []), {}, "rates"),
    ((64, 8192, [2] * 7), {}, "rates"),
    ((64, 64, [1]), {}, "rates"),
    ((64, 64, [17]), {}, "rates"),
    ((64, 64, [2.5]), {}, "rates"),
    ((64, 64, [2]), dict(d_out=2), "d_out"),
    ((64, 64, [2]), dict(compute_dtype="bf16"), "compute_dtype"),
    ((64, 64, [2]), dict(compute_dtype="f32x3"), "compute_dtype"),
])
def test_decoder_refusals_name_their_argument(args, kw, names):
    with pytest.raises(ValueError, match=names):
        A.DACDecoder(*args, **kw)


@pytest.mark.parametrize("kw,names", [
    (dict(conv_kernel=5), "conv_kernel"),
    (dict(latent_dim=6), "latent_dim"),
    (dict(intermediate_embedding_size=[1024, 48]), "intermediate_embedding_size"),
    (dict(intermediate_embedding_size=[512, 128]), "intermediate_embedding_size"),
    (dict(intermediate_embedding_size=[1024]), "intermediate_embedding_size"),
])
def test_autoencoder_refusals_name_their_argument(kw, names):
    with pytest.raises(ValueError, match=names):
        A.FineTuneAutoencoder(**kw)


def test_served_widths_construct():
    for args in ((64, 1536, [2, 2, 2, 2]), (64, 1024, [5, 5, 4, 2]), (4, 32 * 64, [16] * 6), (2048, 64, [3])):
        A.DACDecoder(*args)
    A.FineTuneAutoencoder()
    A.FineTuneAutoencoder(intermediate_embedding_size=[1024, 64], latent_dim=8)


def test_output_length_against_the_fixture_shapes(report):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "dac_golden.npz"))
    for case in ("odd", "w96"):
        net = make(case)
        T = gold[f"{case}_x"].shape[-1]
        assert net.output_length(T) == gold[f"{case}_out"].shape[-1] == report["cases"][case]["out_shape"][-1]
    dec = A.DACDecoder(64, 256, [4, 5, 2])
    assert [dec.output_length(t) for t in (1, 13)] == [38, 518]
    assert A.DACDecoder(1024, 1536, [8, 8, 4, 2]).output_length(64) == 32768
    assert A.DACDecoder(64, 64, [5]).output_length(10) == 49          # odd s: L s - 1


def test_forward_refusals_before_any_device_call():
    dec, ae = A.DACDecoder(8, 64, [2]), A.FineTuneAutoencoder(intermediate_embedding_size=[1024, 64], latent_dim=8)
    with pytest.raises(ValueError, match="z must be shaped"):
        dec(torch.zeros(1, 4, 5))
    with pytest.raises(NotImplementedError, match="no backward"):
        dec(torch.zeros(1, 8, 5, requires_grad=True))
    with pytest.raises(NotImplementedError, match="no backward"):
        ae.decode(torch.zeros(1, 8, 5, requires_grad=True))
    with pytest.raises(NotImplementedError, match="encode"):
        ae.encode(torch.zeros(1, 1024, 5))
    with pytest.raises(NotImplementedError, match="decode"):
        ae(torch.zeros(1, 1024, 5))
    with pytest.raises(RuntimeError, match="ROCm device"):          # everything passed: the only thing missing is the device
        dec(torch.zeros(1, 8, 5))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ae.decode(torch.zeros(1, 8, 5))


def test_header_declares_and_library_exports_the_new_symbols(header):
    lib = _lib.load_library()
    for name in ("adf_dac_create", "adf_dac_forward", "adf_dac_output_length"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert re.search(r"\bint\s+adf_dac_create\s*\(\s*const\s+adf_dac_config\s*\*\s*cfg\s*,\s*adf_handle\s*\*\*\s*out\s*\)", header)
    assert re.search(r"\bint\s+adf_dac_forward\s*\(\s*adf_handle\s*\*\s*h\s*,\s*const\s+float\s*\*\s*in\s*,\s*int\s+B\s*,\s*int\s+T\s*,\s*float\s*\*\s*out\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", header)
    assert _lib.EXPORTS["adf_dac_create"] == (C.c_int, [C.POINTER(_lib.AdfDacConfig), C.POINTER(C.c_void_p)])
    assert "adf_dac_config, adf_dac_create, adf_dac_forward" in header and "Added without a bump" in header


def test_adf_dac_config_layout_matches_the_header(header):
    body = re.search(r"typedef struct adf_dac_config \{(.*?)\} adf_dac_config;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (ADF_DAC_\w+) (\d+)", header)}
    assert (consts["ADF_DAC_MAX_RATES"], consts["ADF_DAC_MAX_WIDTHS"]) == (_lib.ADF_DAC_MAX_RATES, _lib.ADF_DAC_MAX_WIDTHS)
    assert (consts["ADF_DAC_KIND_DECODER"], consts["ADF_DAC_KIND_AUTOENCODER"]) == (_lib.DAC_KIND_DECODER, _lib.DAC_KIND_AUTOENCODER)
    fields, words = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("int32_t "), decl
            m = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", decl[len("int32_t "):].strip())
            fields.append(m.group(1))
            words += consts[m.group(2)] if m.group(2) else 1
    assert fields == [n for n, _ in _lib.AdfDacConfig._fields_] and C.sizeof(_lib.AdfDacConfig) == 4 * words


def test_make_dac_config_carries_the_constructor_arguments():
    c = make_dac_config(DR.config("odd"), _lib.DTYPE_F32)
    assert (c.kind, c.input_channel, c.channels, c.n_rates, list(c.rates)[:3], c.d_out, c.n_widths, c.dtype) == (0, 64, 256, 3, [4, 5, 2], 1, 0, 0)
    c = make_dac_config(DR.config("ae"), _lib.DTYPE_F32)
    assert (c.kind, c.input_channel, c.n_rates, c.n_widths, list(c.widths)[:4]) == (1, 32, 0, 4, [1024, 512, 256, 128])


def test_abi_version_stays_7(header):
    assert _lib.load_library().adf_abi_version() == 7 and _lib.ABI_VERSION == 7 and re.search(r"#define ADF_ABI_VERSION 7\b", header)


def test_new_sources_are_listed_in_the_build_and_exported():
    assert "adf_dac.hip" in build.SOURCES and "adf_net_dac.hip" in build.SOURCES and "adf_dac.h" in build.HEADERS
    for f in ("adf_dac.hip", "adf_net_dac.hip", "adf_dac.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    assert A.DACDecoder is A.dac.DACDecoder and A.FineTuneAutoencoder is A.dac.FineTuneAutoencoder


def test_create_without_a_device_or_with_bad_arguments_reports_by_name():
    lib = _lib.load_library()
    h = C.c_void_p()
    c = make_dac_config(DR.config("w96"), _lib.DTYPE_BF16)
    assert lib.adf_dac_create(C.byref(c), C.byref(h)) != 0 and not h.value
    msg = lib.adf_last_error(None).decode()
    assert msg.startswith("adf_dac_create: ") and ("dtype" in msg or "no HIP device" in msg)
