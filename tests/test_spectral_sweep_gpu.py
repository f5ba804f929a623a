"""GPU: SpecToWave (csrc/adf_istft.hip) over the geometries its launcher and kernel distinguish, against the yardstick of test_spectral_gpu.py --
torch.istft in FLOAT64 ON THE CPU of spec_back in float64 of the same fp32 input; error = max|a - b| / max|b|; bar FP32_TIGHT (5e-5).

test_spectral_gpu.py is built around the shipped geometry (n_fft 510, hop 128).  CASES below holds the smallest shape that reaches each edge it
leaves out: istft_gemm_kernel<2> (hop 64) at all, <4> (hop 32) with more than one block in x, a partly active second row group of <1>
(hop 160 / 192 / 224), every D = ceil(n_fft / hop) in 1..8, K padding of 31, 19, 17, 13 and 1 columns, hop-block tiles one short of full, exactly
full and one past full for each kernel, normalized=False, spec_abs_exponent > 1 (a negative powf exponent), and inputs 500 times quieter and 80
times louder.  tests/test_spectral_sweep_host.py derives that census from CASES alone and holds every case to a conditioning bound on the CPU.
Beside the table: guard bands round both tensors (nothing written outside [B][audio_len], nothing read outside [B][2][F][T]), one plan over changing
B and T, and a captured and replayed call.

Worst measured value per case on an MI355X (WORST_MEASURED below is what a run prints beside its own figure; the kernel is bit-for-bit
repeatable, so a later run on the same build prints the same):
    h64_first 1.6e-6   h64_nj63 8.1e-7   h64_nj64 9.5e-7   h64_nj65 6.9e-7   h64_d8 1.5e-6   h32_nj127 6.5e-7   h32_nj128 1.3e-6   h32_nj129 8.8e-7
    h32_three_blocks 5.1e-7   h128_nj31 1.2e-6   h128_nj32 1.7e-6   h128_nj33 1.5e-6   h96 9.7e-7   h160 1.2e-6   h192 1.6e-6   h224 1.4e-6
    h256_max 1.4e-6   d1_h32 3.1e-7   d1_h64 3.4e-7   d1_h128 4.4e-7   d3 6.2e-7   d5 1.1e-6   d6 1.5e-6   d7 7.1e-7   d8_max 2.9e-6   f31 3.7e-7
    f33 4.1e-7   f51 5.0e-7   unnormalized 1.6e-6   unnormalized_h64 8.4e-7   e2 1.2e-6   e1p5_h64 1.0e-6   e0p25 5.1e-7   sqrt_hann 1.5e-6
    quiet 1.2e-6   loud 1.3e-6;   guard bands 1.3e-6 / 7.5e-7 / 1.3e-6, one plan 9.8e-7, captured and replayed 1.3e-6.
No case exceeds the 5e-6 at which test_spectral_gpu.py says a case wants a look, so none needs its K chain to explain it.  The figures do follow
the chain all the same: a sample is one k-ordered fp32 fmaf chain of D * 2 * Fp products, and the error goes with its square root -- 3e-7 .. 4e-7
at 64 .. 192 products (d1_*, at the level of torch's own fp32 istft), 1.0e-6 .. 1.7e-6 at the shipped 2048, and d8_max, the longest chain the
library accepts (8704 = 4.25 x 2048), is the largest figure at 2.9e-6 = sqrt(4.25) x 1.4e-6.  The bar stays FP32_TIGHT.
"""
import ctypes as C
import os

import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
from audiodiffuser_amd.spectral import _config
from test_gpu_parity import FP32_TIGHT
from test_spectral_gpu import make_input, oracle, rel

WORST_MEASURED = {"h64_first": 1.6e-6, "h64_nj63": 8.1e-7, "h64_nj64": 9.5e-7, "h64_nj65": 6.9e-7, "h64_d8": 1.5e-6, "h32_nj127": 6.5e-7,
                  "h32_nj128": 1.3e-6, "h32_nj129": 8.8e-7, "h32_three_blocks": 5.1e-7, "h128_nj31": 1.2e-6, "h128_nj32": 1.7e-6, "h128_nj33": 1.5e-6,
                  "h96": 9.7e-7, "h160": 1.2e-6, "h192": 1.6e-6, "h224": 1.4e-6, "h256_max": 1.4e-6, "d1_h32": 3.1e-7, "d1_h64": 3.4e-7,
                  "d1_h128": 4.4e-7, "d3": 6.2e-7, "d5": 1.1e-6, "d6": 1.5e-6, "d7": 7.1e-7, "d8_max": 2.9e-6, "f31": 3.7e-7, "f33": 4.1e-7,
                  "f51": 5.0e-7, "unnormalized": 1.6e-6, "unnormalized_h64": 8.4e-7, "e2": 1.2e-6, "e1p5_h64": 1.0e-6, "e0p25": 5.1e-7,
                  "sqrt_hann": 1.5e-6, "quiet": 1.2e-6, "loud": 1.3e-6}


def window_of(kind, n_fft):
    """None stands for the library's own periodic Hann window."""
    if kind is None:
        return None
    return {"hamming": lambda: torch.hamming_window(n_fft), "ones": lambda: torch.ones(n_fft),
            "sqrt_hann": lambda: torch.hann_window(n_fft).sqrt()}[kind]()


#        name                B  n_fft hop   T    e     factor window      normalized  input scale
CASES = [("h64_first",        2, 254,  64,   9, 0.2,  0.6,  None,        True,  0.5),     # <2> at all; D 4
         ("h64_nj63",         1, 254,  64,  63, 0.2,  0.6,  None,        True,  0.5),     # <2>: tile one short of full
         ("h64_nj64",         1, 254,  64,  64, 0.5,  0.3,  None,        True,  0.5),     #      exactly full
         ("h64_nj65",         1, 254,  64,  65, 0.2,  0.6,  None,        True,  0.5),     #      one hop block into a second block
         ("h64_d8",           2, 512,  64,   7, 0.2,  0.6,  None,        True,  0.5),     # <2> with D 8, F 257, jlo 4, aligned half
         ("h32_nj127",        1, 126,  32, 127, 0.2,  0.6,  None,        True,  0.5),     # <4>: the same three edges at 128 hop blocks
         ("h32_nj128",        1, 126,  32, 128, 0.2,  0.6,  None,        True,  0.5),
         ("h32_nj129",        1, 126,  32, 129, 0.5,  0.3,  None,        True,  0.5),
         ("h32_three_blocks", 1,  62,  32, 260, 0.2,  0.6,  None,        True,  0.5),     # <4>: three x blocks, jlo 0, D 2
         ("h128_nj31",        1, 510, 128,  31, 0.2,  0.6,  None,        True,  0.5),     # <1>: one short of full,
         ("h128_nj32",        1, 510, 128,  32, 0.2,  0.6,  None,        True,  0.5),     #      exactly full,
         ("h128_nj33",        1, 510, 128,  33, 0.2,  0.6,  None,        True,  0.5),     #      one past
         ("h96",              2, 254,  96,   6, 0.2,  0.6,  None,        True,  0.5),     # one row group, 3 of 4 waves; D 3, odd half
         ("h160",             2, 510, 160,   6, 0.2,  0.6,  None,        True,  0.5),     # second row group with 1,
         ("h192",             2, 384, 192,   5, 0.2,  0.6,  None,        True,  0.5),     #   2,
         ("h224",             2, 600, 224,   5, 0.2,  0.6,  None,        True,  0.5),     #   3 active waves; F % 32 = 0, 1, 13; D 4, 2, 3
         ("h256_max",         1, 1024, 256,  4, 0.2,  0.6,  None,        True,  0.5),     # largest n_fft, 17 K chunks, two full groups, jlo 2
         ("d1_h32",           2,  32,  32,   7, 0.2,  0.6,  "hamming",   True,  0.5),     # D 1 on <4>; F 17: one chunk, mostly zero columns
         ("d1_h64",           2,  64,  64,   5, 0.2,  0.6,  "hamming",   True,  0.5),     # D 1 on <2>; F 33
         ("d1_h128",          2, 128, 128,   4, 1.0,  0.6,  "ones",      True,  0.5),     # D 1 on <1>, envelope 1
         ("d3",               2,  96,  32,   9, 0.2,  0.6,  None,        True,  0.5),     # the D values in between; F % 32 = 17, 17, 0, 17
         ("d5",               2, 160,  32,   9, 0.2,  0.6,  None,        True,  0.5),
         ("d6",               2, 190,  32,   9, 0.2,  0.6,  None,        True,  0.5),
         ("d7",               2, 224,  32,   9, 0.2,  0.6,  None,        True,  0.5),
         ("d8_max",           1, 1024, 128, 10, 0.2,  0.6,  None,        True,  0.5),     # D 8 x 17 chunks: the longest K chain (8704 products)
         ("f31",              2,  60,  32,   6, 0.2,  0.6,  None,        True,  0.5),     # F % 32 = 31,
         ("f33",              2,  64,  32,   6, 0.2,  0.6,  None,        True,  0.5),     #   1,
         ("f51",              2, 100,  64,   6, 0.2,  0.6,  None,        True,  0.5),     #   19
         ("unnormalized",     2, 510, 128,   6, 0.2,  0.6,  None,        False, 0.5),
         ("unnormalized_h64", 2, 254,  64,   6, 0.5,  0.3,  "hamming",   False, 0.5),     # the same on <2> with a given window
         ("e2",               2, 510, 128,   5, 2.0,  0.6,  None,        True,  0.5),     # powf with exponent -0.5,
         ("e1p5_h64",         2, 254,  64,   5, 1.5,  0.45, None,        True,  0.5),     #   -1/3,
         ("e0p25",            2, 126,  32,   5, 0.25, 0.6,  None,        True,  0.5),     #   +3, one on each kernel
         ("sqrt_hann",        2, 510, 128,   6, 0.2,  0.6,  "sqrt_hann", True,  0.5),     # w^2, not w, overlap-adds to a constant
         ("quiet",            2, 510, 128,   5, 0.2,  0.6,  None,        True,  1e-3),    # output ~ 2e-12
         ("loud",             2, 510, 128,   5, 0.2,  0.6,  None,        True,  40.0)]    # output ~ 2e11
IDS = [c[0] for c in CASES]


def case_input(name, B, n_fft, T, scale):
    """make_input seeded by len(name) + T (no hash()), rescaled from its 0.5 for the quiet and the loud case."""
    x = make_input(B, n_fft, T, seed=len(name) + T)
    return x if scale == 0.5 else x * (scale / 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,n_fft,hop,T,e,f,wkind,normalized,scale", CASES, ids=IDS)
def test_parity_with_the_float64_oracle(name, B, n_fft, hop, T, e, f, wkind, normalized, scale):
    x = case_input(name, B, n_fft, T, scale)
    win = window_of(wkind, n_fft)
    ref = oracle(x, n_fft, hop, e, f, window=win, normalized=normalized)
    out = A.SpecToWave(n_fft=n_fft, hop_length=hop, spec_abs_exponent=e, spec_factor=f, window=win, normalized=normalized)(x.cuda())
    assert out.shape == (B, hop * (T - 1)) == tuple(ref.shape) and out.dtype == torch.float32 and out.is_cuda
    assert bool(torch.isfinite(out).all())
    peak = float(ref.abs().max())
    assert peak > (0.0 if name == "quiet" else 1e-3), peak
    err = rel(out, ref)
    print(f"spec_to_wave sweep {name}: rel err {err:.3e} (worst measured {WORST_MEASURED[name]:.1e}, bar {FP32_TIGHT:.0e}), "
          f"oracle peak {peak:.2e}")
    assert err < FP32_TIGHT, (name, err)


SENTINEL = -2.0 ** 127          # finite, and 27 binades above anything an audio sample of these inputs reaches
GUARD = 64                      # floats on either side of the output, and behind the input
LEAD = 61                       # NaNs in front of the input: the spectrogram then starts 4 bytes past a 16-byte boundary


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop,T", [(254, 64, 9), (126, 32, 7), (510, 160, 6)], ids=["wn2", "wn4", "wn1_two_groups"])
def test_writes_nothing_outside_the_audio_and_reads_nothing_outside_the_spec(n_fft, hop, T):
    """adf_istft_run on interior pointers of two larger allocations.  A store before or past [B][audio_len] lands in a band of sentinels, a load
    before or past [B][2][F][T] reads a NaN and turns the output NaN; neither can fault, both bands lie inside the one live allocation."""
    B, e, f = 2, 0.2, 0.6
    n = hop * (T - 1)
    x = make_input(B, n_fft, T, seed=31 + T)
    ref = oracle(x, n_fft, hop, e, f)
    m = A.SpecToWave(n_fft=n_fft, hop_length=hop, spec_abs_exponent=e, spec_factor=f)
    plain = m(x.cuda())

    obuf = torch.full((GUARD + B * n + GUARD,), SENTINEL, device="cuda", dtype=torch.float32)
    ibuf = torch.full((LEAD + x.numel() + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    ibuf[LEAD:LEAD + x.numel()] = x.cuda().reshape(-1)
    assert obuf.data_ptr() % 16 == 0 and ibuf.data_ptr() % 16 == 0 and bool(torch.isnan(ibuf[:LEAD]).all()) and bool(torch.isnan(ibuf[-GUARD:]).all())
    lib = _lib.load_library()
    cfg = _config(n_fft, hop, e, f, True, True)
    plan = C.c_void_p()
    assert lib.adf_istft_create(C.byref(cfg), None, C.byref(plan)) == 0, lib.adf_last_error(None)
    try:
        rc = lib.adf_istft_run(plan, ibuf.data_ptr() + 4 * LEAD, B, T, obuf.data_ptr() + 4 * GUARD, n, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.adf_last_error(None)
        torch.cuda.synchronize()
    finally:
        lib.adf_istft_destroy(plan)
    bits = obuf.view(torch.int32)
    sentinel_bits = torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32).item()
    assert bool((bits[:GUARD] == sentinel_bits).all()), "a store in front of the audio"
    assert bool((bits[-GUARD:] == sentinel_bits).all()), "a store past the end of the audio"
    inner = obuf[GUARD:GUARD + B * n].view(B, n)
    assert not bool((bits[GUARD:GUARD + B * n] == sentinel_bits).any()), "a sample that was never written"
    assert bool(torch.isfinite(inner).all()), "a NaN of the input's guard bands reached the output"
    err = rel(inner, ref)
    print(f"spec_to_wave guard bands n_fft {n_fft} hop {hop} T {T}: rel err {err:.3e}")
    assert err < FP32_TIGHT, err
    assert torch.equal(inner, plain)


@pytest.mark.gpu
def test_a_plan_serves_changing_T_and_B():
    """One module, hence one plan: nothing of a call's B or T may stay behind in it.  T = 2 is the shortest legal input."""
    n_fft, hop = 254, 64
    m = A.SpecToWave(n_fft, hop)
    outs = []
    for B, T in ((2, 5), (1, 70), (3, 2), (2, 5)):
        x = make_input(B, n_fft, T, seed=7 * B + T)
        ref = oracle(x, n_fft, hop, 0.2, 0.6)
        out = m(x.cuda())
        assert out.shape == (B, hop * (T - 1)) == tuple(ref.shape) and bool(torch.isfinite(out).all()) and float(ref.abs().max()) > 1e-3
        err = rel(out, ref)
        print(f"spec_to_wave one plan B {B} T {T}: rel err {err:.3e}")
        assert err < FP32_TIGHT, (B, T, err)
        outs.append(out)
    assert len(m._plans) == 1
    assert torch.equal(outs[0], outs[3])


def _hip_runtime():
    """The HIP runtime this process already runs on (the one torch's graph handle belongs to), found among the mapped files."""
    paths = []
    with open("/proc/self/maps") as fh:
        for line in fh:
            p = line.split()[-1]
            if os.path.basename(p).startswith("libamdhip64.so") and p not in paths:
                paths.append(p)
    assert paths, "no HIP runtime is loaded"
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    paths.sort(key=lambda p: not p.startswith(torch_lib))
    return C.CDLL(paths[0])


def graph_census(raw_graph):
    """(node types, number of edges, number of root nodes) of a hipGraph_t."""
    hip = _hip_runtime()
    g = C.c_void_p(raw_graph)
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, C.byref(n)) == 0
    nodes = (C.c_void_p * max(n.value, 1))()
    assert hip.hipGraphGetNodes(g, nodes, C.byref(n)) == 0
    types = []
    for i in range(n.value):
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
        types.append(t.value)
    edges, roots = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipGraphGetEdges(g, None, None, C.byref(edges)) == 0
    assert hip.hipGraphGetRootNodes(g, None, C.byref(roots)) == 0
    return types, edges.value, roots.value


HIP_GRAPH_NODE_TYPE_KERNEL = 0


@pytest.mark.gpu
def test_captured_and_replayed():
    """The call site is the tail of a graph-replayed sampler: adf_istft_run neither allocates nor synchronises, so one call is one kernel node."""
    n_fft, hop, T = 254, 64, 9
    m = A.SpecToWave(n_fft, hop)
    first, second = make_input(2, n_fft, T, seed=41), make_input(2, n_fft, T, seed=42)
    static = first.cuda()
    assert static.shape == (2, 2, 128, 9)
    m(static)                                           # the plan (two allocations, two copies) exists before the capture
    want = m(second.cuda())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        out = m(static)
    types, edges, roots = graph_census(graph.raw_cuda_graph())
    assert types == [HIP_GRAPH_NODE_TYPE_KERNEL] and edges == 0 and roots == 1, (types, edges, roots)
    static.copy_(second.cuda())
    graph.replay()
    a = out.clone()
    out.zero_()
    graph.replay()
    b = out.clone()
    torch.cuda.synchronize()
    assert torch.equal(a, want) and torch.equal(b, a)
    err = rel(a, oracle(second, n_fft, hop, 0.2, 0.6))
    print(f"spec_to_wave captured and replayed: rel err {err:.3e}")
    assert err < FP32_TIGHT, err
