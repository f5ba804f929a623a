"""CPU: what keeps the table of tests/test_spectral_sweep_gpu.py honest without a device -- every case passes the constructor's argument checks,
the census of kernel variants, tile edges, D, K padding and output alignments the table claims is recomputed from the table alone, and every case
is well conditioned (torch.istft in fp32 on the CPU stays within 5e-6 of the float64 oracle; measured at most 6.1e-7), so that a miss on the
device says something about the kernel and not about the input.

The routing rule below is written from the description in csrc/adf_istft.h, not imported from the library: a block of 4 waves covers 128 hop
blocks x 32 samples at hop 32, 64 x 64 at hop 64 and 32 x 128 at any other hop.  A silent change to the routing then fails the census here."""
import os
import re

import pytest
import torch

import audiodiffuser_amd as A
from test_spectral_gpu import oracle, spec_back
from test_spectral_sweep_gpu import CASES, IDS, case_input, window_of

CONDITIONING_BAR = 5e-6


def width_of(hop):
    """Hop blocks per block in x."""
    return 128 if hop == 32 else 64 if hop == 64 else 32


def geometry(n_fft, hop, T):
    half = n_fft // 2
    jlo = half // hop                                                   # the first hop block that holds a kept sample
    nj = (half + hop * (T - 1) - 1) // hop - jlo + 1                    # the hop blocks that hold kept samples
    width = width_of(hop)
    rows = 4096 // width                                                # samples of a hop block per block: 4 waves x (32 x 32)
    return dict(half=half, F=half + 1, D=-(-n_fft // hop), jlo=jlo, nj=nj, width=width, x_blocks=-(-nj // width),
                row_groups=-(-hop // rows), last_group_waves=(hop - 1) % rows // 32 + 1 if rows == 128 else 4)


GEO = {c[0]: geometry(c[2], c[3], c[4]) for c in CASES}


def test_names_are_unique_and_say_what_the_geometry_is():
    assert len(set(IDS)) == len(IDS) == len(CASES)
    for name, g in GEO.items():
        said = re.search(r"_nj(\d+)$", name)
        if said:
            assert g["nj"] == int(said.group(1)), (name, g)
        said = re.fullmatch(r"d(\d)(_.*)?", name)
        if said:
            assert g["D"] == int(said.group(1)), (name, g)
        said = re.fullmatch(r"f(\d+)", name)
        if said:
            assert g["F"] == int(said.group(1)), (name, g)


@pytest.mark.parametrize("name,B,n_fft,hop,T,e,f,wkind,normalized,scale", CASES, ids=IDS)
def test_every_case_passes_the_argument_checks(name, B, n_fft, hop, T, e, f, wkind, normalized, scale):
    m = A.SpecToWave(n_fft=n_fft, hop_length=hop, spec_abs_exponent=e, spec_factor=f, window=window_of(wkind, n_fft), normalized=normalized)
    assert not m._plans and B >= 1 and T >= 2


def test_census_of_the_table():
    hops = {c[3] for c in CASES}
    assert hops == set(range(32, 257, 32))                              # every hop the library accepts
    assert {g["D"] for g in GEO.values()} == set(range(1, 9))
    assert {g["F"] % 32 for g in GEO.values()} == {0, 1, 13, 17, 19, 31}
    assert any(g["F"] < 32 for g in GEO.values())                       # one chunk that is mostly zero columns
    for width in (32, 64, 128):
        of_width = [g for g in GEO.values() if g["width"] == width]
        assert any(g["nj"] % width == 0 for g in of_width), width                           # exactly full
        assert any(g["nj"] % width == 1 and g["nj"] > width for g in of_width), width       # one hop block into the next block
        assert any(g["nj"] == width - 1 for g in of_width), width                           # one short of full
        assert {g["D"] for g in of_width} >= {1, 4}, width                                  # no earlier frame, and the shipped depth
    assert any(g["x_blocks"] == 3 for g in GEO.values())
    assert {g["last_group_waves"] for g in GEO.values() if g["row_groups"] == 2} == {1, 2, 3, 4}
    assert any(g["row_groups"] == 1 and g["last_group_waves"] == 3 for g in GEO.values())
    assert any(g["jlo"] == 0 for g in GEO.values()) and any(g["jlo"] >= 2 for g in GEO.values())
    assert {g["half"] % 4 for g in GEO.values()} >= {0, 2, 3}           # aligned, half-aligned and odd output offsets of a run
    # the switches beside the geometry
    assert any(not c[8] for c in CASES if c[3] == 128) and any(not c[8] for c in CASES if c[3] == 64)
    assert {width_of(c[3]) for c in CASES if c[5] > 1} | {width_of(c[3]) for c in CASES if c[5] == 0.25} == {32, 64, 128}
    assert {c[7] for c in CASES} == {None, "hamming", "ones", "sqrt_hann"}
    assert {c[9] for c in CASES} == {0.5, 1e-3, 40.0}
    chain = {name: g["D"] * 2 * -(-g["F"] // 32) * 32 for name, g in GEO.items()}             # products per output sample
    assert max(chain, key=chain.get) == "d8_max" and chain["d8_max"] == 8704 == 4.25 * 2048     # 2048: the shipped geometry's


def test_the_width_rule_is_the_headers():
    """The rule above against the sentence it was written from: if the header's description changes, this census has to be read again."""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audiodiffuser_amd", "csrc", "adf_istft.h")).read()
    assert "inline int istft_wn(int h) { return h == 32 ? 4 : h == 64 ? 2 : 1; }" in hdr
    assert [width_of(h) for h in (32, 64, 96, 128, 256)] == [32 * 4, 32 * 2, 32, 32, 32]


@pytest.mark.parametrize("name,B,n_fft,hop,T,e,f,wkind,normalized,scale", CASES, ids=IDS)
def test_every_case_is_well_conditioned(name, B, n_fft, hop, T, e, f, wkind, normalized, scale):
    """The reference's own four lines in fp32 on the CPU against the same lines in float64.  A case that loses this proves nothing about the kernel."""
    x = case_input(name, B, n_fft, T, scale)
    assert x.dtype == torch.float32 and x.shape == (B, 2, n_fft // 2 + 1, T)
    assert torch.equal(x, case_input(name, B, n_fft, T, scale))         # the seed is len(name) + T: the same in every process
    win = window_of(wkind, n_fft)
    ref = oracle(x, n_fft, hop, e, f, window=win, normalized=normalized)
    z = spec_back(torch.view_as_complex(x.permute(0, 2, 3, 1).contiguous()), e, f)
    got = torch.istft(z, window=win if win is not None else torch.hann_window(n_fft), normalized=normalized, n_fft=n_fft, hop_length=hop, center=True)
    assert got.dtype == torch.float32 and got.shape == ref.shape == (B, hop * (T - 1))
    peak = float(ref.abs().max())
    assert peak > (0.0 if name == "quiet" else 1e-3), peak
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    print(f"spec_to_wave sweep {name}: torch.istft in fp32 on the CPU is {err:.2e} from the float64 oracle, peak {peak:.2e}")
    assert err < CONDITIONING_BAR, (name, err)
