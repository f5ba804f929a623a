"""CPU: the host side of WaveToSpec -- the basis table of adf_stft_basis against float64, the argument refusals of the constructor and of
adf_stft_create, the tensor checks that precede any device call, and the additive C ABI (no device is touched here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib, spectral

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(510, 128), (126, 32), (128, 96), (256, 32), (1022, 256)]


def window_case(n_fft, custom):
    """None (the library's periodic Hann) or a given fp32 window that is no Hann window."""
    return torch.hamming_window(n_fft, dtype=torch.float32) if custom else None


@pytest.mark.parametrize("normalized", [True, False], ids=["normalized", "plain"])
@pytest.mark.parametrize("custom", [False, True], ids=["hann", "given_window"])
@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_basis_is_the_windowed_real_dft_rounded_once(n_fft, hop, custom, normalized):
    """Row k of the two tables against bin k of torch.fft.rfft of w s (unit impulses) in float64: an entry has magnitude <= s max|w| and is rounded
    to fp32 once, so it is within s max|w| 2^-23 (twice the half-ulp of the largest entry: room for libm's cosine against torch's)."""
    win = window_case(n_fft, custom)
    basis = spectral.stft_basis(n_fft, hop, normalized=normalized, window=win)
    F = n_fft // 2 + 1
    assert basis.shape == (2, F, n_fft) and basis.dtype == np.float32
    w64 = win.double() if custom else torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    s = n_fft ** -0.5 if normalized else 1.0
    want = torch.fft.rfft(torch.diag(w64 * s), n=n_fft, dim=1).transpose(0, 1)          # [k][m]: bin k of the impulse at m, weight w[m] s
    bar = s * float(w64.abs().max()) * 2.0 ** -23
    got_c, got_s = torch.from_numpy(basis[0]).double(), torch.from_numpy(basis[1]).double()
    assert float(want.abs().max()) <= s * float(w64.abs().max()) * (1 + 1e-12)          # the magnitude the bar is sized for
    for k in range(F):
        assert float((got_c[k] - want.real[k]).abs().max()) <= bar, k
        assert float((got_s[k] - want.imag[k]).abs().max()) <= bar, k
    # bit for bit: the DC and Nyquist bins of a real signal have no imaginary part
    assert not basis[1][0].any() and not basis[1][F - 1].any()
    # a sine row other than those two is not zero (the test above is not satisfied by an empty table)
    assert float(np.abs(basis[1][1]).max()) > 0.5 * s * float(w64.abs().max())
    assert float(np.abs(basis[0][0]).max()) > 0.5 * s * float(w64.abs().max())


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
        A.WaveToSpec(**kw)


@pytest.mark.parametrize("kw,names", [r for r in REFUSALS if r[0].get("window") is None or r[0]["window"].numel() == 510],
                         ids=["odd_n_fft", "hop_48", "hop_32_of_510", "center_false", "factor_0", "exponent_0", "window_zero"])
def test_create_refuses_before_it_looks_for_a_device(kw, names):
    """adf_stft_create checks its arguments first: the message names the argument even where there is no device to create a plan on."""
    lib = _lib.load_library()
    full = dict(n_fft=510, hop_length=128, center=True, normalized=True, spec_abs_exponent=0.2, spec_factor=0.6)
    win = kw.get("window")
    full.update({k: v for k, v in kw.items() if k != "window"})
    cfg = _lib.AdfIstftConfig(**{k: (int(v) if k in ("n_fft", "hop_length", "center", "normalized") else float(v)) for k, v in full.items()})
    wbuf = win.numpy().ctypes.data_as(C.c_void_p) if win is not None else None
    plan = C.c_void_p()
    assert lib.adf_stft_create(C.byref(cfg), wbuf, C.byref(plan)) != 0 and not plan.value
    msg = lib.adf_last_error(None).decode()
    assert msg.startswith("adf_stft_create: ") and names in msg, msg
    assert lib.adf_stft_create(None, None, C.byref(plan)) != 0 and "null" in lib.adf_last_error(None).decode()


def test_good_arguments_pass_every_check():
    for n_fft, hop in GEOMETRIES + [(62, 32), (64, 32), (1024, 128)]:
        for e, f in ((0.2, 0.6), (0.5, 0.3), (1.0, 0.6), (0.3, 0.45)):
            m = A.WaveToSpec(n_fft=n_fft, hop_length=hop, spec_abs_exponent=e, spec_factor=f)
            assert isinstance(m, torch.nn.Module) and not list(m.parameters()) and not m.state_dict()
    A.WaveToSpec(window=torch.hamming_window(510))
    w = torch.zeros(510)
    w[17] = 1.0
    A.WaveToSpec(window=w)                 # no overlap-add condition in this direction: one non-zero value is a window


def test_tensor_checks_come_before_any_device_call():
    m = A.WaveToSpec()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 1024))
    for bad in (torch.zeros(1024), torch.zeros(1, 2, 1024), torch.zeros(2, 1024, dtype=torch.float64), torch.zeros(1024, 2).transpose(0, 1),
                torch.zeros(0, 1024)):
        with pytest.raises(ValueError):
            m(bad)
    with pytest.raises(ValueError, match="audio"):
        m(torch.zeros(2, 255))             # L = n_fft / 2: torch.stft refuses it for the reflect padding, so does WaveToSpec
    assert not m._plans                    # no plan was created: nothing reached the library's device side


def test_run_refuses_null_arguments_without_a_plan():
    lib = _lib.load_library()
    assert lib.adf_stft_run(None, None, 1, 1024, None, 9, None) != 0
    msg = lib.adf_last_error(None).decode()
    assert msg.startswith("adf_stft_run: ") and "null" in msg, msg
    lib.adf_stft_destroy(None)             # a null plan is ignored


def test_the_four_symbols_are_additive_to_abi_7():
    hdr = open(os.path.join(ROOT, "include", "audiodiffuser_amd.h")).read()
    lib = _lib.load_library()
    for sym in ("adf_stft_create", "adf_stft_basis", "adf_stft_run", "adf_stft_destroy"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTS and re.search(rf"\b{sym}\s*\(", hdr), sym
    assert lib.adf_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define ADF_ABI_VERSION (\d+)", hdr).group(1)) == 7
    assert re.search(r"^ \* 7: .*?adf_stft", hdr, flags=re.S | re.M)             # the changelog entry says so
    assert A.WaveToSpec is spectral.WaveToSpec
    assert "WaveToSpec" in A.__doc__
