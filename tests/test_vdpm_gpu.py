"""GPU: the program-driven device loop (adf_sampler_run_program) under VDPMSampler and VUniPCSampler, eager and graph-replayed, on all four networks.

What a result is compared with: the CPU restatement tests/vdpm_ref.py (pinned to the reference's classes by tools/gen_golden_vdpm.py) in FLOAT64 around
the oracle nets, on the runs of tests/vdpm_cases.py, with the same fp32 schedule scalars.  The ADM oracle only runs in fp32, so its case is compared with
the fp32 restatement.  The bar of a run is the project's max(1e-3, 4 * dist_fp32_fp64) (max-norm, relative to max |ref|) with the fp32-vs-float64
distance of the CPU restatement recorded in tests/golden/vdpm_golden.json (3.6e-7 .. 5.2e-6 for every run: 1e-3 throughout).  Every reference is
finite, has max |y| > 0.05 and at most 1 % of its entries at the closing clamp (asserted by the generator and again here).

The two shipped settings (VDPMSampler(order=3, multisteps=False, x0_pred=False) and VUniPCSampler(order=2, x0_pred=True) over VDiffusion() and
LinearSchedule(1.0, 0.0) on an unconditional UNet2dBase) are the first two runs; the conftest sets ADF_REQUIRE_NATIVE, so a run that left the device
would raise.  The WaveNet cases have 3 x 501 = 1503 elements: the vector body and the scalar tail of the update kernel, whose five-operand
instantiation the order-3 UniPC corrector is the first to reach.  The conftest's counter check wraps ``sampler_run`` only, so every run here reads the
counters itself (``counted``).

Measured on one MI355X: tests/golden/vdpm_report.json."""
import ctypes as C
import functools
import json
import os
import re

import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
import vdpm_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3                   # the project's bar for a whole run (tests/test_rf_gpu.py)
BF16_TOL = 6e-2              # tests/test_rf_gpu.py, tests/test_gpu_parity.py: bf16 storage against the fp32 mode
CLS = {"dpm": A.VDPMSampler, "unipc": A.VUniPCSampler}
EVAL, LIN = _lib.PROG_EVAL, _lib.PROG_LIN


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


@pytest.fixture(scope="module")
def runs():
    with open(os.path.join(ROOT, "tests", "golden", "vdpm_golden.json")) as f:
        return json.load(f)["runs"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The CPU result of a run of tests/vdpm_cases.py, computed once per session and never modified."""
    return DC.reference(name, DC.ref_dtype(DC.spec(name)))


def device_net(net_name, out_scale=1.0, dtype="fp32"):
    cfg, w = DC.weights(net_name, out_scale)
    if net_name in ("tiny", "tiny_cc"):
        net = A.UNet1dBase.from_config(cfg, compute_dtype=dtype)
    elif net_name in ("u2d", "u2d_un"):
        net = A.UNet2dBase(**cfg.to_kwargs())
    elif net_name == "adm":
        net = A.UNetModel.from_config(cfg)
    else:
        net = A.WaveNetNoise.from_config(cfg)
    net.load_state_dict(w, strict=True)
    return net.cuda()


def handle(net):
    return net.native(torch.device("cuda", torch.cuda.current_device()))


def program_nfe(ops, result=0):
    d = _lib.AdfProgDesc(num_ops=len(ops), result_slot=result, x0_scale=1.0, use_graph=0)
    return _lib.load_library().adf_sampler_program_nfe(C.byref(d), (_lib.AdfProgOp * len(ops))(*ops))


def counted(hd, nfe, use_graph, call):
    """``call()`` must be exactly one device loop: one more sampler run, ``nfe`` more evaluations, one graph replay or none."""
    before = hd.counters()
    out = call()
    after = hd.counters()
    assert after["sampler_runs"] == before["sampler_runs"] + 1, (before, after)
    assert nfe > 0 and after["sampler_evals"] == before["sampler_evals"] + nfe, (before, after, nfe)
    assert after["graph_replays"] - before["graph_replays"] == (1 if use_graph else 0), (before, after)
    return out


def device_run(name, use_graph, net=None, dtype="fp32"):
    """Run ``name`` of tests/vdpm_cases.py through the plugin classes on the device, counters checked."""
    sp = DC.spec(name)
    net = net if net is not None else device_net(sp["net"], sp["out_scale"], dtype)
    cl = DC.labels(sp["net"])
    kw = {} if cl is None else {"classes": cl.cuda()}
    smp = CLS[sp["sampler"]](**DC.sampler_kwargs(sp), use_graph=use_graph)
    diff, sig = A.VDiffusion(), A.LinearSchedule(sp["t0"], sp["t1"], sp["steps"])()
    assert torch.equal(sig, DC.sigmas_of(sp))
    nfe = program_nfe(smp._program(sig)[0])
    return counted(handle(net), nfe, use_graph, lambda: smp(DC.noise_of(sp).cuda(), fn=diff.denoise_fn, net=net, sigmas=sig, **kw).cpu()), nfe


# ---- parity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DC.RUNS))
def test_sampler_eager_and_graph_vs_cpu_restatement(runs, name):
    ref = reference(name)
    sp, rec = DC.spec(name), runs[name]
    assert all(rec[k] == sp[k] for k in ("out_scale", "noise_scale", "steps", "order", "t0", "t1", "noise_seed")), "the fixture belongs to other inputs"
    assert rec["dist_fp32_fp64"] is None or rec["dist_fp32_fp64"] < 2.5e-4
    bar = max(TOL, 4.0 * (rec["dist_fp32_fp64"] or 0.0))
    share, top = float((ref.abs() >= 1).double().mean()), float(ref.abs().max())
    assert bool(torch.isfinite(ref).all()) and share <= 0.01 and top > 0.05, (name, share, top)
    net = device_net(sp["net"], sp["out_scale"])
    for use_graph in (False, True):
        y, nfe = device_run(name, use_graph, net)
        e = rel(y, ref)
        print(name, "graph" if use_graph else "eager", "rel err", e, "bar", bar, "share |y| >= 1:", share, "max |y|", top, "evaluations", nfe)
        assert nfe == rec["evaluations"] == sp["steps"]
        assert y.shape == ref.shape and bool(torch.isfinite(y).all()) and float(y.abs().max()) <= 1.0
        assert e <= bar, (name, use_graph, e, bar)
    if sp["shape"] == "wn":
        assert ref.numel() % 4 == 3                                   # the update kernel's scalar tail ran
    if name == "unipc_wn_o3":
        smp = A.VUniPCSampler(**DC.sampler_kwargs(sp))
        assert max(o.n_terms for o in smp._program(DC.sigmas_of(sp))[0] if o.kind == LIN) == 5        # ... in its five-operand form


@pytest.mark.gpu
def test_bf16_storage_through_the_program_loop_stays_near_the_fp32_mode():
    name = "dpm_tiny_single3_x0"
    (y32, _), (y16, _) = device_run(name, True), device_run(name, True, dtype="bf16")
    print(name, "bf16 vs fp32 mode", rel(y16, y32))
    assert bool(torch.isfinite(y16).all()) and float(y16.abs().max()) <= 1.0
    assert rel(y16, y32) < BF16_TOL


@pytest.mark.gpu
def test_rows_of_the_run_are_the_rows_of_the_program():
    sp = DC.spec("unipc_tiny1_o2")
    net = device_net(sp["net"], sp["out_scale"])
    smp, sig = A.VUniPCSampler(**DC.sampler_kwargs(sp), use_graph=False), DC.sigmas_of(sp)
    ops = smp._program(sig)[0]
    smp(DC.noise_of(sp).cuda(), fn=A.VDiffusion().denoise_fn, net=net, sigmas=sig)
    got = handle(net).coef_rows(torch.device("cuda")).cpu()
    want = torch.tensor([[o.eval.c_in, o.eval.c_noise, o.eval.c_skip, o.eval.c_out] for o in ops if o.kind == EVAL])
    assert got.shape == want.shape == (sp["steps"], 4) and torch.equal(got, want)


# ---- the driver itself, through hand-set programs ----------------------------------------------------------------------------------------
def ev(dst, src, clip=_lib.CLIP_NONE, c_noise=0.3):
    return _lib.AdfProgOp(kind=EVAL, dst=dst, src=src, eval=_lib.AdfTableEval(c_in=1.0, c_noise=c_noise, c_skip=0.0, c_out=1.0, clip=clip))


def lin(dst, terms, clamp=0):
    op = _lib.AdfProgOp(kind=LIN, dst=dst, n_terms=len(terms), clamp=clamp)
    for j, (s, k) in enumerate(terms):
        op.slot[j], op.coef[j] = s, k
    return op


def run_program(hd, ops, noise, result=0, x0=1.0, use_graph=0, num_ops=None):
    """``ops``: a list of ops, or None for a null program pointer (num_ops 1)."""
    n = num_ops if num_ops is not None else 1 if ops is None else len(ops)
    desc = _lib.AdfProgDesc(num_ops=n, result_slot=result, x0_scale=x0, use_graph=use_graph)
    return hd.sampler_run_program(desc, None if ops is None else (_lib.AdfProgOp * len(ops))(*ops), noise)


@pytest.mark.gpu
def test_five_operands_in_place_at_the_tail_size_and_every_slot():
    """1503 elements (375 float4 + 3).  Slots 2 .. 7 are filled with multiples of the start state, then slot 0 is updated in place from five
    operands (itself among them): a closed form without the network's output.  The last slot (7) is the result of a second program; the
    evaluation's output (slot 1) arrives where a coefficient reads it."""
    net = device_net("wn", 1.0)
    hd = handle(net)
    shape = DC.SHAPES["wn"]
    noise = torch.randn(*shape, generator=torch.Generator().manual_seed(3)).cuda()
    assert noise.numel() == 1503 and noise.numel() % (4 * 256) != 0
    fill = [lin(2, [(0, 0.5)]), lin(3, [(0, -1.5)]), lin(4, [(0, 0.25)]), lin(5, [(0, 2.0)])]
    ops = [ev(1, 0)] + fill + [lin(0, [(0, 0.75), (2, 1.0), (3, 0.5), (4, -2.0), (5, 0.125)])]
    x = 4.0 * noise
    want = (0.75 + 0.5 - 0.75 - 0.5 + 0.25) * x
    for clamp in (0, 1):
        ops[-1].clamp = clamp
        y = counted(hd, 1, False, lambda: run_program(hd, ops, noise, x0=4.0))
        w = want.clamp(-1.0, 1.0) if clamp else want
        print("five operands, clamp", clamp, "max err", float((y - w).abs().max()), "max |want|", float(want.abs().max()))
        assert bool(torch.isfinite(y).all()) and float((y - w).abs().max()) <= 4e-6 * float(want.abs().max())
    assert 0.1 < float((want.abs() < 1).float().mean()) < 0.9                                      # the clamp run clamps many entries and leaves many
    y = run_program(hd, [ev(1, 0), lin(6, [(0, 2.0)]), lin(7, [(6, 1.0), (0, 1.0)], 1)], noise, result=7, x0=4.0)
    assert float((y - (3.0 * x).clamp(-1.0, 1.0)).abs().max()) <= 4e-6 * 3.0 * float(x.abs().max())
    y = run_program(hd, [ev(1, 0), lin(0, [(1, 1.0)])], noise)                                     # x = the raw network output at c_noise 0.3
    v = hd.net_forward(noise, torch.full((shape[0],), 0.3, device="cuda"))
    assert rel(y, v) <= 1e-5 and float(v.abs().max()) > 1e-3


@pytest.mark.gpu
def test_replay_without_a_new_capture_and_one_changed_coefficient_is_another_graph():
    net = device_net("wn", 1.0)
    hd = handle(net)
    noise = torch.randn(*DC.SHAPES["wn"], generator=torch.Generator().manual_seed(4)).cuda()
    prog = lambda k: [ev(1, 0), lin(0, [(0, k)])]
    caps = hd.counters()["graph_captures"]
    y1 = counted(hd, 1, True, lambda: run_program(hd, prog(0.5), noise, use_graph=1))
    assert hd.counters()["graph_captures"] - caps == 1
    y3 = counted(hd, 1, True, lambda: run_program(hd, prog(0.5), noise, use_graph=1))             # the same program: replayed, not captured again
    assert hd.counters()["graph_captures"] - caps == 1
    y2 = counted(hd, 1, True, lambda: run_program(hd, prog(0.25), noise, use_graph=1))
    assert hd.counters()["graph_captures"] - caps == 2
    assert torch.equal(y1, 0.5 * noise) and torch.equal(y2, 0.25 * noise) and torch.equal(y3, y1)
    y4 = run_program(hd, prog(0.5), noise, x0=2.0, use_graph=1)                                    # ... nor two descriptors
    assert hd.counters()["graph_captures"] - caps == 3 and torch.equal(y4, noise)
    # the plugin classes: a second call with the same program replays the first call's graph
    sp = DC.spec("dpm_wn_single3_x0")
    wn = device_net(sp["net"], sp["out_scale"])
    h2 = handle(wn)
    (ya, _) = device_run("dpm_wn_single3_x0", True, wn)
    caps = h2.counters()["graph_captures"]
    (yb, _) = device_run("dpm_wn_single3_x0", True, wn)
    assert h2.counters()["graph_captures"] == caps and torch.equal(ya, yb)


@pytest.mark.gpu
def test_malformed_programs_are_refused_by_name_and_launch_nothing():
    net = device_net("tiny", 0.05)
    hd = handle(net)
    noise = DC.noise_of(DC.spec("dpm_tiny_single3_x0")).cuda()
    good = [ev(1, 0), lin(0, [(0, 0.5), (1, 0.5)])]
    run_program(hd, good, noise)                                                              # the workspace exists from here on
    nan = float("nan")
    bad_row = _lib.AdfProgOp(kind=EVAL, dst=1, src=0, eval=_lib.AdfTableEval(c_in=1.0, c_noise=float("inf"), c_skip=0.0, c_out=1.0, clip=0))
    P = lambda ops, **kw: (lambda: run_program(hd, ops, noise, **kw))
    cases = [
        (P(None), "ops is null"),
        (lambda: hd.sampler_run_program(None, (_lib.AdfProgOp * 2)(*good), noise), "desc is null"),
        (P(good, num_ops=0), "num_ops"),
        (P(good, x0=nan), "x0_scale"),
        (P([_lib.AdfProgOp(kind=2, dst=1, src=0)] + good), r"ops\[0\]\.kind = 2"),
        (P([ev(8, 0)] + good), r"ops\[0\]\.dst = 8"),
        (P([ev(1, -1)] + good), r"ops\[0\]\.src = -1"),
        (P(good + [lin(0, [(0, 1.0), (9, 1.0)])]), r"ops\[2\]\.slot\[1\] = 9"),
        (P([ev(1, 3)]), r"ops\[0\]\.src reads slot 3.*nothing has written"),
        (P(good + [lin(0, [(0, 1.0), (4, 1.0)])]), r"ops\[2\]\.slot\[1\] reads slot 4.*nothing has written"),
        (P(good, result=5), r"result_slot reads slot 5"),
        (P(good, result=8), r"result_slot = 8"),
        (P([ev(0, 0)]), r"ops\[0\].*dst == src"),
        (P(good + [_lib.AdfProgOp(kind=LIN, dst=0, n_terms=0)]), r"ops\[2\]\.n_terms = 0"),
        (P(good + [_lib.AdfProgOp(kind=LIN, dst=0, n_terms=6)]), r"ops\[2\]\.n_terms = 6"),
        (P(good + [lin(0, [(0, 1.0), (1, 1.0), (0, 1.0)])]), r"ops\[2\]\.slot\[2\] names slot 0 a second time"),
        (P(good + [lin(0, [(0, 1.0), (1, nan)])]), r"ops\[2\]\.coef\[1\] is not finite"),
        (P([bad_row] + good), r"ops\[0\]\.eval.*non-finite"),
        (P([ev(1, 0, clip=7)]), r"ops\[0\]\.eval\.clip"),
        (P([lin(0, [(0, 0.5)])]), r"no ADF_PROG_EVAL"),
    ]
    for call, pattern in cases:
        before = hd.counters()
        with pytest.raises(_lib.AdfError, match="adf_sampler_run_program: ") as ei:
            call()
        assert re.search(pattern, str(ei.value)), (pattern, str(ei.value))
        assert hd.counters() == before, "a refused call enqueued or counted something"
    y = counted(hd, 1, False, lambda: run_program(hd, good, noise))                           # the handle is as good as before
    assert bool(torch.isfinite(y).all())
