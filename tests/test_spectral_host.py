"""CPU: the host side of SpecToWave -- the basis tables of adf_istft_basis against float64, the argument refusals of the constructor and of
adf_istft_create, the tensor checks that precede any device call, and the additive C ABI (no device is touched here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
from audiodiffuser_amd.spectral import istft_basis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(510, 128), (126, 32), (128, 96), (256, 32), (1022, 256)]


def window_case(n_fft, custom):
    """None (the library's periodic Hann) or a given fp32 window that is no Hann window."""
    return torch.hamming_window(n_fft, dtype=torch.float32) if custom else None


@pytest.mark.parametrize("normalized", [True, False], ids=["normalized", "plain"])
@pytest.mark.parametrize("custom", [False, True], ids=["hann", "given_window"])
@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_basis_is_the_windowed_inverse_real_dft_rounded_once(n_fft, hop, custom, normalized):
    """C Z_0 + S Z_1 over unit spectra against torch.fft.irfft x window x scale in float64, hop block by hop block: one fp32 rounding of
    entries of magnitude <= 2 s is at most 2 s 2^-24 < 2e-7."""
    win = window_case(n_fft, custom)
    basis, wsq = istft_basis(n_fft, hop, normalized=normalized, window=win)
    F, D = n_fft // 2 + 1, -(-n_fft // hop)
    assert basis.shape == (2, D * hop, F) and basis.dtype == np.float32 and wsq.shape == (D * hop,) and wsq.dtype == np.float32
    w64 = win.double() if custom else torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    scale = n_fft ** 0.5 if normalized else 1.0
    eye = torch.eye(F, dtype=torch.float64)
    want_c = torch.fft.irfft(torch.complex(eye, torch.zeros_like(eye)), n=n_fft, dim=0) * w64[:, None] * scale      # [m][k]: unit real spectrum e_k
    want_s = torch.fft.irfft(torch.complex(torch.zeros_like(eye), eye), n=n_fft, dim=0) * w64[:, None] * scale      # unit imaginary spectrum i e_k
    Cb, Sb = torch.from_numpy(basis[0]).double(), torch.from_numpy(basis[1]).double()
    assert float(want_c.abs().max()) <= 2 * scale / n_fft * float(w64.abs().max()) * (1 + 1e-12)        # the magnitude the bar is sized for
    for d in range(D):
        lo, hi = d * hop, min((d + 1) * hop, n_fft)
        assert float((Cb[lo:hi] - want_c[lo:hi]).abs().max()) < 2e-7, d
        assert float((Sb[lo:hi] - want_s[lo:hi]).abs().max()) < 2e-7, d
    # bit for bit: the transform ignores the imaginary part of the DC and Nyquist rows, the tail rows pad the last segment, wsq is w^2
    assert not basis[1][:, 0].any() and not basis[1][:, F - 1].any()
    assert not basis[:, n_fft:, :].any() and not wsq[n_fft:].any()
    if custom:
        assert np.array_equal(wsq[:n_fft], (win.double() ** 2).float().numpy())
    else:
        assert float(np.abs(wsq[:n_fft].astype(np.float64) - (w64 ** 2).numpy()).max()) < 6e-8      # libm's cosine against torch's: one fp32 rounding
    # a sine column other than those two is not zero (the test above is not satisfied by an empty table)
    assert float(np.abs(basis[1][:, 1]).max()) > 0.5 * scale / n_fft


REFUSALS = [
    (dict(n_fft=511), "n_fft"),
    (dict(hop_length=48), "hop_length"),
    (dict(n_fft=510, hop_length=32), "hop_length"),
    (dict(center=False), "center"),
    (dict(spec_factor=0.0), "spec_factor"),
    (dict(spec_abs_exponent=0.0), "spec_abs_exponent"),
    (dict(window=torch.hann_window(512)), "window"),
    (dict(window=torch.zeros(510)), "window"),
]


@pytest.mark.parametrize("kw,names", REFUSALS, ids=["odd_n_fft", "hop_48", "hop_32_of_510", "center_false", "factor_0", "exponent_0", "window_length",
                                                    "window_zero"])
def test_constructor_refuses_and_names_the_argument(kw, names):
    with pytest.raises(ValueError, match=names):
        A.SpecToWave(**kw)


@pytest.mark.parametrize("kw,names", [r for r in REFUSALS if r[0].get("window") is None or r[0]["window"].numel() == 510],
                         ids=["odd_n_fft", "hop_48", "hop_32_of_510", "center_false", "factor_0", "exponent_0", "window_zero"])
def test_create_refuses_before_it_looks_for_a_device(kw, names):
    """adf_istft_create checks its arguments first: the message names the argument even where there is no device to create a plan on."""
    lib = _lib.load_library()
    full = dict(n_fft=510, hop_length=128, center=True, normalized=True, spec_abs_exponent=0.2, spec_factor=0.6)
    win = kw.get("window")
    full.update({k: v for k, v in kw.items() if k != "window"})
    cfg = _lib.AdfIstftConfig(**{k: (int(v) if k in ("n_fft", "hop_length", "center", "normalized") else float(v)) for k, v in full.items()})
    wbuf = win.numpy().ctypes.data_as(C.c_void_p) if win is not None else None
    plan = C.c_void_p()
    assert lib.adf_istft_create(C.byref(cfg), wbuf, C.byref(plan)) != 0 and not plan.value
    msg = lib.adf_last_error(None).decode()
    assert msg.startswith("adf_istft_create: ") and names in msg, msg
    assert lib.adf_istft_create(None, None, C.byref(plan)) != 0 and "null" in lib.adf_last_error(None).decode()


def test_good_arguments_pass_every_check():
    for n_fft, hop in GEOMETRIES + [(62, 32), (64, 32), (1024, 128)]:
        for e, f in ((0.2, 0.6), (0.5, 0.3), (1.0, 0.6)):
            m = A.SpecToWave(n_fft=n_fft, hop_length=hop, spec_abs_exponent=e, spec_factor=f)
            assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and not m.state_dict()
    A.SpecToWave(window=torch.hamming_window(510))


def test_tensor_checks_come_before_any_device_call():
    m = A.SpecToWave()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 2, 256, 8))
    for bad in (torch.zeros(1, 2, 255, 8), torch.zeros(2, 256, 8), torch.zeros(1, 2, 256, 8, dtype=torch.float64),
                torch.zeros(1, 2, 8, 256).transpose(2, 3), torch.zeros(1, 3, 256, 8), torch.zeros(1, 2, 256, 1)):
        with pytest.raises(ValueError):
            m(bad)
    assert not m._plans                    # no plan was created: nothing reached the library's device side


def test_config_struct_layout_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")).read()
    ctype_of = {"int32_t": 4, "float": 4, "int64_t": 8, "double": 8}
    body = re.search(r"typedef struct adf_istft_config \{(.*?)\} adf_istft_config;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want, off, align = [], 0, 1
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, rest = decl.split(None, 1)
        size = ctype_of[ty]
        align = max(align, size)
        for item in rest.split(","):
            off = (off + size - 1) // size * size
            want.append((item.strip(), off, size))
            off += size
    pyc = _lib.AdfIstftConfig
    assert [(n, getattr(pyc, n).offset, getattr(pyc, n).size) for n, _ in pyc._fields_] == want
    assert [n for n, _, _ in want] == ["n_fft", "hop_length", "center", "normalized", "spec_abs_exponent", "spec_factor"]
    assert C.sizeof(pyc) == (off + align - 1) // align * align == 32


def test_the_four_symbols_are_additive_to_abi_7():
    hdr = open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")).read()
    lib = _lib.load_library()
    for sym in ("adf_istft_create", "adf_istft_basis", "adf_istft_run", "adf_istft_destroy"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTS and re.search(rf"\b{sym}\s*\(", hdr), sym
    assert lib.adf_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define ADF_ABI_VERSION (\d+)", hdr).group(1)) == 7
    assert re.search(r"^ \* 7: .*?adf_istft", hdr, flags=re.S | re.M)            # the changelog entry says so
    assert A.SpecToWave is __import__("audiodiffuser_amd.spectral", fromlist=["SpecToWave"]).SpecToWave
