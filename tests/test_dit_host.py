"""CPU: the plugin contract of ``audiodiffuser_amd.DiT`` without a device -- state-dict layout against the reference's (recorded by
tools/gen_golden_dit.py in tests/golden/dit_golden_report.json), strict load, every refusal by exception type and named argument, and the C ABI
additions (``adf_dit_config`` / ``adf_dit_create``) against the header."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib, build
import dit_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(input_size=[16, 8], hidden_size=128, depth=1, num_heads=2)


@pytest.fixture(scope="module")
def report():
    with open(os.path.join(ROOT, "tests", "golden", "dit_golden_report.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")) as f:
        return f.read()


@pytest.mark.parametrize("case", DR.GOLDEN_CASES)
def test_state_dict_names_shapes_and_order_are_the_references(report, case):
    net = A.DiT(**DR.ctor_kwargs(case))
    mine = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert mine == report["variants"][case]["state_dict"]
    assert not net.pos_embed.requires_grad and all(p.requires_grad for n, p in net.named_parameters() if n != "pos_embed")


def test_constructor_signature_is_the_references_plus_compute_dtype(report):
    import inspect
    ref = re.findall(r"(\w+)=", report["signature"])
    mine = [n for n in inspect.signature(A.DiT.__init__).parameters if n != "self"]
    assert mine == ref + ["compute_dtype"]
    d = inspect.signature(A.DiT.__init__).parameters
    assert (d["hidden_size"].default, d["depth"].default, d["num_heads"].default, d["cond_drop_prob"].default, d["text_embed_dim"].default,
            d["max_text_len"].default, d["use_self_text_cond"].default, d["compute_dtype"].default) == (1152, 28, 16, 0.1, 512, 128, True, "fp32")


def test_strict_load_of_a_reference_shaped_dict_and_random_init():
    net = A.DiT(**DR.ctor_kwargs("labels"))
    sd = net.state_dict()
    # initialize_weights (dit.py:355-364): the zero-initialised tensors stay zero in the class, pos_embed is the table
    for k, v in sd.items():
        if "adaLN_modulation" in k or k.startswith("final_layer.linear") or k.endswith(".bias") and not k.startswith("y_embedder.class_to_cond.0"):
            assert not v.any(), k
    assert torch.equal(sd["pos_embed"][0], A.dit.sincos_pos_embed(128, (2, 2)))
    w = DR.weights("labels")
    assert net.load_state_dict(w, strict=True).missing_keys == []
    assert all(torch.equal(net.state_dict()[k], v) for k, v in w.items())
    bad = dict(w)
    bad.pop("blocks.0.attn.to_context.weight")
    with pytest.raises(RuntimeError, match="to_context"):
        net.load_state_dict(bad, strict=True)


@pytest.mark.parametrize("kw,exc,names", [
    (dict(text_cond=True), NotImplementedError, "text_cond"),
    (dict(class_embed_dim=32), NotImplementedError, "class_embed_dim"),
    (dict(use_qk_l2norm=True), NotImplementedError, "use_qk_l2norm"),
    (dict(compute_dtype="bf16"), ValueError, "compute_dtype"),
    (dict(input_size=[16, 10]), ValueError, "patch_size"),
    (dict(hidden_size=1152, num_heads=16), ValueError, "num_heads"),          # DiT-XL: head dim 72
    (dict(hidden_size=96, num_heads=3), ValueError, "hidden_size"),
    (dict(hidden_size=2048, num_heads=32), ValueError, "hidden_size"),
    (dict(num_heads=8), ValueError, "num_heads"),                             # head dim 16
    (dict(mlp_ratio=4.1), ValueError, "mlp_ratio"),
    (dict(hidden_size=1024, num_heads=16, mlp_ratio=4.5), ValueError, "mlp_ratio"),
    (dict(patch_size=[1, 1], in_channels=2), ValueError, "patch_size"),
    (dict(input_size=[64, 64], patch_size=[16, 8], in_channels=4), ValueError, "patch_size"),
    (dict(label_cond=True), ValueError, "num_classes"),
])
def test_constructor_refusals_name_their_argument(kw, exc, names):
    with pytest.raises(exc, match=names):
        A.DiT(**{**SMALL, **kw})


def test_default_constructor_is_dit_xl_and_is_refused_by_its_head_dim():
    with pytest.raises(ValueError, match="num_heads"):
        A.DiT()


def test_dit_s_b_l_construct():
    for hidden, heads in ((384, 6), (768, 12), (1024, 16)):
        A.DiT(input_size=[16, 8], hidden_size=hidden, depth=1, num_heads=heads)


def test_forward_refusals_before_any_device_call():
    net = A.DiT(**SMALL)
    x, t = torch.zeros(1, 4, 16, 8), torch.zeros(1)
    with pytest.raises(NotImplementedError, match="text_embeds"):
        net(x, t, text_embeds=torch.zeros(1, 3, 512))
    with pytest.raises(ValueError, match="label_cond"):
        net(x, t, classes=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="input_size"):
        net(torch.zeros(1, 4, 16, 16), t)
    lab = A.DiT(label_cond=True, num_classes=4, **SMALL)
    with pytest.raises(NotImplementedError, match="cond_drop_prob"):       # the constructor default 0.1 draws a random mask
        lab(x, t, classes=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="cond_drop_prob"):
        lab(x, t, classes=torch.zeros(1, dtype=torch.int64), cond_drop_prob=0.5)
    with pytest.raises(RuntimeError, match="ROCm device"):                 # everything passed: the only thing missing is the device
        net(x, t)


def test_header_declares_and_library_exports_adf_dit_create(header):
    lib = _lib.load_library()
    assert hasattr(lib, "adf_dit_create") and "adf_dit_create" in _lib.EXPORTS
    assert re.search(r"\bint\s+adf_dit_create\s*\(\s*const\s+adf_dit_config\s*\*\s*cfg\s*,\s*adf_handle\s*\*\*\s*out\s*\)", header)
    assert _lib.EXPORTS["adf_dit_create"] == (C.c_int, [C.POINTER(_lib.AdfDitConfig), C.POINTER(C.c_void_p)])


def test_adf_dit_config_layout_matches_the_header(header):
    body = re.search(r"typedef struct adf_dit_config \{(.*?)\} adf_dit_config;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("int32_t "), decl
            fields += [n.strip() for n in decl[len("int32_t "):].split(",")]
    assert fields == [n for n, _ in _lib.AdfDitConfig._fields_]
    assert all(t is C.c_int32 for _, t in _lib.AdfDitConfig._fields_) and C.sizeof(_lib.AdfDitConfig) == 4 * len(fields)


def test_make_dit_config_carries_the_constructor_arguments():
    c = _lib.make_dit_config(DR.config("odd"), _lib.DTYPE_F32)
    assert (c.input_h, c.input_w, c.patch_h, c.patch_w, c.in_channels, c.hidden_size, c.depth, c.num_heads, c.mlp_hidden, c.num_classes, c.dtype) == \
        (32, 16, 4, 4, 4, 192, 2, 3, 480, 0, 0)
    assert _lib.make_dit_config(DR.config("labels"), _lib.DTYPE_F32).num_classes == 10


def test_abi_version_stays_7(header):
    assert _lib.load_library().adf_abi_version() == 7 and _lib.ABI_VERSION == 7 and re.search(r"#define ADF_ABI_VERSION 7\b", header)


def test_new_sources_are_listed_in_the_build():
    assert "adf_dit.hip" in build.SOURCES and "adf_net_dit.hip" in build.SOURCES and "adf_dit.h" in build.HEADERS
    for f in ("adf_dit.hip", "adf_net_dit.hip", "adf_dit.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))


def test_create_without_a_device_or_with_bad_widths_reports_by_name():
    lib = _lib.load_library()
    h = C.c_void_p()
    c = _lib.make_dit_config(DR.config("tiny"), _lib.DTYPE_BF16)
    assert lib.adf_dit_create(C.byref(c), C.byref(h)) != 0 and not h.value
    msg = lib.adf_last_error(None).decode()
    assert msg.startswith("adf_dit_create: ") and ("dtype" in msg or "no HIP device" in msg)
