"""GPU: the table-driven device loop (adf_sampler_run_table) under VESampler, VPSampler, VSampler and VEulerSampler, eager and graph-replayed, on all
four networks.

What a result is compared with: the CPU restatement tests/vsamp_ref.py (pinned to the reference's classes by tools/gen_golden_vsamp.py) in FLOAT64
around the oracle nets, on the runs of tests/vsamp_cases.py, with the same fp32 schedule scalars and the same injected draws.  The ADM oracle only runs
in fp32, so its case is compared with the fp32 restatement.  The bar of a run is the project's max(1e-3, 4 * dist_fp32_fp64) (max-norm, relative to
max |ref|) with the fp32-vs-float64 distance of the CPU restatement recorded in tests/golden/vsamp_golden.json (1e-7 .. 1.1e-6 for every run: 1e-3
throughout).  Every run that ends in clamp(-1, 1) has at most 1 % of its reference at the clamp and every clamped per-evaluation estimate at most
50 % (asserted by the generator and again here); the VP runs end unclamped and leave [-1, 1].

The WaveNet cases have 3 x 501 = 1503 elements: the vector body and the scalar tail of the update kernel, in one block row that is not full.  The
conftest's counter check wraps ``sampler_run`` only, so every run here reads the counters itself (``device_run``).

Measured on one MI355X: tests/golden/vsamp_report.json."""
import ctypes as C
import functools
import json
import os
import re

import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
import precond_ref as PR
import rf_cases as RC
import vsamp_cases as VC
import vsamp_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3                   # the project's bar for a whole run (tests/test_rf_gpu.py)
BF16_TOL = 6e-2              # tests/test_rf_gpu.py, tests/test_gpu_parity.py: bf16 storage against the fp32 mode
CLS = {"ve": A.VESampler, "vp": A.VPSampler, "v": A.VSampler, "veuler": A.VEulerSampler}


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


@pytest.fixture(scope="module")
def runs():
    with open(os.path.join(ROOT, "tests", "golden", "vsamp_golden.json")) as f:
        return json.load(f)["runs"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the CPU result of a run of tests/vsamp_cases.py, its largest clamped share), computed once per session and never modified."""
    info = {}
    return VC.reference(name, VC.ref_dtype(VC.spec(name)), info=info), info["clamped_share"]


def device_net(net_name, out_scale=1.0, dtype="fp32"):
    cfg, w = RC.weights(net_name, out_scale)
    if net_name in ("tiny", "tiny_cc"):
        net = A.UNet1dBase.from_config(cfg, compute_dtype=dtype)
    elif net_name == "u2d":
        net = A.UNet2dBase(**cfg.to_kwargs())
    elif net_name == "adm":
        net = A.UNetModel.from_config(cfg)
    else:
        net = A.WaveNetNoise.from_config(cfg)
    net.load_state_dict(w, strict=True)
    return net.cuda()


def handle(net):
    return net.native(torch.device("cuda", torch.cuda.current_device()))


def diffusion_of(kind):
    return {"ve": A.VEDiffusion, "vp": lambda: A.VPDiffusion(**PR.VP_ARGS)}.get(kind, A.VDiffusion)()


def table_nfe(steps):
    d = _lib.AdfTableDesc(num_steps=len(steps), x0_scale=1.0, final_clamp=0, use_graph=0)
    return _lib.load_library().adf_sampler_table_nfe(C.byref(d), (_lib.AdfTableStep * len(steps))(*steps))


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
    """Run ``name`` of tests/vsamp_cases.py through the plugin classes on the device, counters checked."""
    sp = VC.spec(name)
    net = net if net is not None else device_net(sp["net"], sp["out_scale"], dtype)
    cl = RC.labels(sp["net"])
    kw = {} if cl is None else {"classes": cl.cuda()}
    smp = CLS[sp["sampler"]](**VC.sampler_kwargs(sp), use_graph=use_graph)
    diff, sig = diffusion_of(sp["sampler"]), VC.sigmas_of(sp)
    steps = smp._table(sig, diff)[0] if sp["sampler"] in ("ve", "vp") else smp._table(sig)[0]
    inj = VC.draws_of(sp).cuda() if sp["sampler"] != "veuler" else None
    return counted(handle(net), table_nfe(steps), use_graph,
                   lambda: smp(VC.noise_of(sp).cuda(), fn=diff.denoise_fn, net=net, sigmas=sig, injected_noise=inj, **kw).cpu())


# ---- parity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VC.RUNS))
def test_sampler_eager_and_graph_vs_cpu_restatement(runs, name):
    ref, clamped = reference(name)
    sp, rec = VC.spec(name), runs[name]
    assert (rec["out_scale"], rec["noise_scale"], rec["steps"]) == (sp["out_scale"], sp["noise_scale"], sp["steps"]), "the fixture belongs to other inputs"
    assert rec["dist_fp32_fp64"] is None or rec["dist_fp32_fp64"] < 2.5e-4
    bar = max(TOL, 4.0 * (rec["dist_fp32_fp64"] or 0.0))
    share, top = float((ref.abs() >= 1).double().mean()), float(ref.abs().max())
    assert clamped <= 0.5, (name, clamped)
    if sp["sampler"] == "vp":
        assert top > 1.0 and bool(torch.isfinite(ref).all()), (name, top)          # unclamped: the run leaves [-1, 1]
    else:
        assert share <= 0.01 and top > 0.05, (name, share, top)
    net = device_net(sp["net"], sp["out_scale"])
    for use_graph in (False, True):
        y = device_run(name, use_graph, net)
        e = rel(y, ref)
        print(name, "graph" if use_graph else "eager", "rel err", e, "bar", bar, "share |y| >= 1:", share, "max |y|", top, "clamped share", clamped)
        assert y.shape == ref.shape and bool(torch.isfinite(y).all())
        assert sp["sampler"] == "vp" or float(y.abs().max()) <= 1.0
        assert e <= bar, (name, use_graph, e, bar)
    if sp["net"] == "wn":
        assert ref.numel() % 4 == 3                                   # the update kernel's scalar tail ran


@pytest.mark.gpu
def test_dynamic_threshold_is_what_clip_as_configured_means():
    """VPSampler over EluDiffusion(dynamic_threshold = 0.9) with the output layer at scale 4: the 0.9 quantile of every unclipped estimate lies
    between 1.3 and 2.4 (measured on the CPU), so every evaluation of the table is rescaled by the handle's dynamic threshold, and the sampler
    returns its state unclamped, so nothing hides behind a closing clamp.  A tenth of each estimate sits at +-1 by construction of the threshold.
    The bar is max(1e-3, 4 * the CPU's own fp32-vs-float64 distance), measured here (1.4e-6)."""
    sp = VC.spec("vp_tiny_heun")
    cfg, w = RC.weights("tiny", 4.0)
    sig, noise, draws = VC.sigmas_of(sp), VC.noise_of(sp), VC.draws_of(sp)
    kw = VC.sampler_kwargs(sp)
    q90 = []

    def cpu(dt):
        net = RC.oracle_net("tiny", cfg, w, dt)

        def fn(x, sigma):
            raw = PR.denoise("edm", net, x, sigma=sigma, unclipped=True)
            q90.append(float(torch.quantile(raw.abs().reshape(raw.shape[0], -1).double(), 0.9, dim=-1).min()))
            return PR.denoise("edm", net, x, sigma=sigma, dynamic_threshold=0.9)
        with torch.no_grad():
            return VR.vp_sampler(noise.to(dt), fn, sig, sp["steps"], kw["beta_d"], kw["beta_min"], kw["s_churn"], kw["s_noise"], kw["s_min"], kw["s_max"],
                                 True, draws)
    ref = cpu(torch.float64)
    dist = rel(cpu(torch.float32), ref)
    assert dist < 2.5e-4 and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 1.0, (dist, float(ref.abs().max()))
    assert min(q90) > 1.0, "an evaluation whose threshold is 1 is only a clamp"
    net = device_net("tiny", 4.0)
    diff = A.EluDiffusion(sigma_data=PR.SIGMA_DATA, dynamic_threshold=0.9)
    for use_graph in (False, True):
        smp = A.VPSampler(**kw, use_graph=use_graph)
        y = counted(handle(net), 2 * sp["steps"] - 1, use_graph,
                    lambda: smp(noise.cuda(), fn=diff.denoise_fn, net=net, sigmas=sig, injected_noise=draws.cuda()).cpu())
        print("dynamic threshold", "graph" if use_graph else "eager", rel(y, ref), "dist", dist, "smallest q90", min(q90))
        assert rel(y, ref) <= max(TOL, 4 * dist)


@pytest.mark.gpu
def test_bf16_storage_through_the_table_loop_stays_near_the_fp32_mode():
    for name in ("v_tiny_shift0", "ve_tiny_euler"):
        y32, y16 = device_run(name, True), device_run(name, True, dtype="bf16")
        print(name, "bf16 vs fp32 mode", rel(y16, y32))
        assert bool(torch.isfinite(y16).all()) and float(y16.abs().max()) <= 1.0
        assert rel(y16, y32) < BF16_TOL


@pytest.mark.gpu
def test_rows_of_the_run_are_the_rows_of_the_table():
    sp = VC.spec("vp_tiny_heun")
    net = device_net("tiny", sp["out_scale"])
    smp, diff, sig = A.VPSampler(**VC.sampler_kwargs(sp), use_graph=False), diffusion_of("vp"), VC.sigmas_of(sp)
    steps = smp._table(sig, diff)[0]
    smp(VC.noise_of(sp).cuda(), fn=diff.denoise_fn, net=net, sigmas=sig, injected_noise=VC.draws_of(sp).cuda())
    got = handle(net).coef_rows(torch.device("cuda")).cpu()
    want = torch.tensor([[e.c_in, e.c_noise, e.c_skip, e.c_out] for st in steps for e in ([st.eval1, st.eval2] if st.second else [st.eval1])])
    assert got.shape == want.shape == (2 * sp["steps"] - 1, 4) and torch.equal(got, want)


@pytest.mark.gpu
def test_native_draws_leave_the_generator_where_the_reference_leaves_it():
    """Without injected_noise VESampler draws one randn_like per step and VSampler one per step with t_next != 0, in order, VEulerSampler none:
    the next normal after a run is the one that follows that many draws."""
    net = device_net("tiny", 0.05)
    noise = VC.noise_of(VC.spec("ve_tiny_euler")).cuda()
    for kind, n_draws in (("ve", 5), ("v", 4), ("veuler", 0)):
        sp = VC.spec({"ve": "ve_tiny_euler", "v": "v_tiny_shift0", "veuler": "veuler_tiny_heun"}[kind])
        smp, diff = CLS[kind](**VC.sampler_kwargs(sp), use_graph=False), diffusion_of(kind)
        torch.manual_seed(5)
        y = smp(noise, fn=diff.denoise_fn, net=net, sigmas=VC.sigmas_of(sp))
        nxt = torch.randn(4, device="cuda")
        torch.manual_seed(5)
        inj = torch.stack([torch.randn_like(noise) for _ in range(n_draws)]) if n_draws else None
        assert torch.equal(torch.randn(4, device="cuda"), nxt), kind
        y2 = smp(noise, fn=diff.denoise_fn, net=net, sigmas=VC.sigmas_of(sp), injected_noise=inj)
        assert rel(y2, y) < 1e-5, (kind, rel(y2, y))               # the same draws, injected (the U-Net's GroupNorm atomics move the last bits)


# ---- the update kernel, through hand-set one- and two-record tables ---------------------------------------------------------------------
def ev(clip=_lib.CLIP_NONE):
    return _lib.AdfTableEval(c_in=1.0, c_noise=0.3, c_skip=0.0, c_out=1.0, clip=clip)


def run_table(hd, steps, noise, inj, x0=1.0, clamp=0, use_graph=0):
    """``steps``: a list of records, or None for a null table pointer (num_steps 1)."""
    desc = _lib.AdfTableDesc(num_steps=1 if steps is None else len(steps), x0_scale=x0, final_clamp=clamp, use_graph=use_graph)
    return hd.sampler_run_table(desc, None if steps is None else (_lib.AdfTableStep * len(steps))(*steps), noise, inj)


@pytest.mark.gpu
def test_update_kernel_tail_in_place_and_zero_coefficients_skip_their_operand():
    """1503 elements (375 float4 + 3), coefficients chosen so that the result has a closed form without the network's output: every operand with
    a zero coefficient is poisoned with NaN first -- the draw a record names but does not read, the estimate D1 / D2 (their coefficients are 0) and,
    by a first run on NaN draws, every state buffer a one-evaluation record never writes (x_e, D2)."""
    net = device_net("wn", 1.0)
    hd = handle(net)
    shape = VC.SHAPES["wn"]
    g = torch.Generator().manual_seed(3)
    noise, e0 = torch.randn(*shape, generator=g).cuda(), torch.randn(*shape, generator=g).cuda()
    assert noise.numel() == 1503 and noise.numel() % (4 * 256) != 0
    nan = torch.full_like(noise, float("nan"))
    S = _lib.AdfTableStep
    # poison: a two-evaluation record on NaN draws leaves NaN in the state, x_e and both estimates
    bad = run_table(hd, [S(a0=1.0, a1=1.0, eval1=ev(), b0=1.0, b1=1.0, b2=0.0, second=1, eval2=ev(), c0=1.0, c1=1.0, c2=1.0, c3=1.0, draw=0)], noise,
                    nan[None].contiguous())
    assert bool(torch.isnan(bad).all())
    inj = torch.stack([e0, nan])
    # (1) one evaluation per record; record 1 names the NaN draw and reads nothing of it; D1 is never read (b1 = 0)
    steps = [S(a0=0.5, a1=0.2, eval1=ev(), b0=2.0, b1=0.0, b2=-0.25, second=0, draw=0), S(a0=1.0, a1=0.0, eval1=ev(), b0=-1.5, b1=0.0, b2=0.0, second=0, draw=1)]
    xh = 0.5 * (0.7 * noise) + 0.2 * e0
    want = -1.5 * (2.0 * xh - 0.25 * e0)
    for clamp in (0, 1):
        before = hd.counters()
        y = run_table(hd, steps, noise, inj, x0=0.7, clamp=clamp)
        after = hd.counters()
        w = want.clamp(-1.0, 1.0) if clamp else want
        print("one-evaluation records, clamp", clamp, "max err", float((y - w).abs().max()), "max |want|", float(want.abs().max()))
        assert bool(torch.isfinite(y).all()) and float((y - w).abs().max()) <= 4e-6 * float(want.abs().max())
        assert (after["sampler_runs"] - before["sampler_runs"], after["sampler_evals"] - before["sampler_evals"]) == (1, 2)
    assert 0.1 < float((want.abs() < 1).float().mean()) < 0.9                                      # the clamp run clamps many entries and leaves many
    # (2) two evaluations, D1 and D2 unread (c1 = c3 = 0), x_e and x_hat read, the NaN draw named and unread
    steps = [S(a0=1.0, a1=0.0, eval1=ev(), b0=0.5, b1=0.0, b2=0.0, second=1, eval2=ev(_lib.CLIP_UNIT), c0=2.0, c1=0.0, c2=-3.0, c3=0.0, draw=1)]
    y = run_table(hd, steps, noise, inj)
    assert bool(torch.isfinite(y).all()) and float((y - (2.0 * noise - 3.0 * (0.5 * noise))).abs().max()) <= 4e-6 * float(noise.abs().max())
    # (3) the estimates do arrive where their coefficient is not zero: x = D1 (the raw network output at c_noise 0.3)
    y = run_table(hd, [S(a0=1.0, a1=0.0, eval1=ev(), b0=0.0, b1=1.0, b2=0.0, second=0, draw=0)], noise, None)
    v = hd.net_forward(noise, torch.full((shape[0],), 0.3, device="cuda"))
    assert rel(y, v) <= 1e-5 and float(v.abs().max()) > 1e-3


@pytest.mark.gpu
def test_two_tables_that_differ_in_one_coefficient_do_not_share_a_graph():
    net = device_net("wn", 1.0)
    hd = handle(net)
    noise = torch.randn(*VC.SHAPES["wn"], generator=torch.Generator().manual_seed(4)).cuda()
    S = _lib.AdfTableStep
    table = lambda b0: [S(a0=1.0, a1=0.0, eval1=ev(), b0=b0, b1=0.0, b2=0.0, second=0, draw=0)]
    caps = hd.counters()["graph_captures"]
    y1 = run_table(hd, table(0.5), noise, None, use_graph=1)
    y2 = run_table(hd, table(0.25), noise, None, use_graph=1)
    y3 = run_table(hd, table(0.5), noise, None, use_graph=1)
    c = hd.counters()
    assert c["graph_captures"] - caps == 2
    assert torch.equal(y1, 0.5 * noise) and torch.equal(y2, 0.25 * noise) and torch.equal(y3, y1)
    y4 = run_table(hd, table(0.5), noise, None, x0=2.0, use_graph=1)                       # ... nor two descriptors
    assert hd.counters()["graph_captures"] - caps == 3 and torch.equal(y4, noise)


@pytest.mark.gpu
def test_malformed_tables_are_refused_by_name_and_launch_nothing():
    net = device_net("tiny", 0.05)
    hd = handle(net)
    noise = VC.noise_of(VC.spec("ve_tiny_euler")).cuda()
    S = _lib.AdfTableStep
    good = S(a0=1.0, a1=0.0, eval1=ev(), b0=0.5, b1=0.5, b2=0.0, second=0, draw=0)
    run_table(hd, [good], noise, None)                                                        # the workspace exists from here on
    nan = float("nan")
    cases = [
        (lambda: run_table(hd, None, noise, None), "steps is null"),
        (lambda: hd.sampler_run_table(_lib.AdfTableDesc(num_steps=0, x0_scale=1.0), (S * 1)(good), noise, None), "num_steps"),
        (lambda: run_table(hd, [S(a0=1.0, a1=0.0, eval1=ev(), b0=0.0, b1=0.0, b2=0.0, second=1, eval2=ev(), c0=1.0, draw=0)], noise, None), r"steps\[0\]\.second.*x_e"),
        (lambda: run_table(hd, [good, S(a0=1.0, a1=0.0, eval1=ev(), b0=nan, b1=0.5, b2=0.0, second=0, draw=0)], noise, None), r"steps\[1\].*non-finite"),
        (lambda: run_table(hd, [S(a0=1.0, a1=0.0, eval1=_lib.AdfTableEval(c_in=1.0, c_noise=float("inf"), c_skip=0.0, c_out=1.0, clip=0), b0=1.0, second=0)],
                           noise, None), r"steps\[0\]\.eval1.*non-finite"),
        (lambda: run_table(hd, [S(a0=1.0, a1=0.0, eval1=ev(7), b0=1.0, second=0)], noise, None), r"eval1\.clip"),
        (lambda: run_table(hd, [good], noise, None, x0=nan), "x0_scale"),
        (lambda: run_table(hd, [S(a0=1.0, a1=0.5, eval1=ev(), b0=1.0, second=0, draw=0)], noise, None), r"injected_noise is null.*steps\[0\]"),
        (lambda: run_table(hd, [good, S(a0=1.0, a1=0.0, eval1=ev(), b0=1.0, b2=0.5, second=0, draw=2)], noise, torch.zeros(2, *noise.shape, device="cuda")),
         r"steps\[1\]\.draw = 2.*n_injected"),
    ]
    for call, pattern in cases:
        before = hd.counters()
        with pytest.raises(_lib.AdfError, match="adf_sampler_run_table: ") as ei:
            call()
        assert re.search(pattern, str(ei.value)), (pattern, str(ei.value))
        assert hd.counters() == before, "a refused call enqueued or counted something"
    y = counted(hd, 1, False, lambda: run_table(hd, [good], noise, None))                     # the handle is as good as before
    assert bool(torch.isfinite(y).all())


# ---- the two public forms are one loop: a draw-free table and its program, lowered by hand, give the same bits ------------------------------
SLOT_X, SLOT_D1, SLOT_XE, SLOT_D2 = 0, 1, 2, 3          # the slots a table's state, first estimate, x_e and second estimate live in


def lower_by_hand(steps, final_clamp):
    """The ``adf_prog_op`` list of a table none of whose records reads a draw, by the rule the library lowers a table with: the a-update unless
    a0 == 1 and a1 == 0, the evaluation into D1, the b-update (into X, or into XE where a second evaluation and the c-update follow); operands in the
    order of the step form in the header, those with a zero coefficient dropped; the closing clamp on the last op; the result in slot 0."""
    def lin(dst, terms, clamp=0):
        terms = [(s, k) for s, k in terms if k != 0.0]
        op = _lib.AdfProgOp(kind=_lib.PROG_LIN, dst=dst, n_terms=len(terms), clamp=clamp)
        for j, (s, k) in enumerate(terms):
            op.slot[j], op.coef[j] = s, k
        return op

    def evaluate(dst, src, e):
        return _lib.AdfProgOp(kind=_lib.PROG_EVAL, dst=dst, src=src, eval=e)
    ops = []
    for i, r in enumerate(steps):
        assert r.a1 == 0.0 and r.b2 == 0.0, "the program form has no draws"
        clamp = int(bool(final_clamp) and i + 1 == len(steps))
        if not (r.a0 == 1.0 and r.a1 == 0.0):
            ops.append(lin(SLOT_X, [(SLOT_X, r.a0)]))
        ops.append(evaluate(SLOT_D1, SLOT_X, r.eval1))
        if not r.second:
            ops.append(lin(SLOT_X, [(SLOT_X, r.b0), (SLOT_D1, r.b1)], clamp))
            continue
        ops.append(lin(SLOT_XE, [(SLOT_X, r.b0), (SLOT_D1, r.b1)]))
        ops.append(evaluate(SLOT_D2, SLOT_XE, r.eval2))
        ops.append(lin(SLOT_X, [(SLOT_X, r.c0), (SLOT_D1, r.c1), (SLOT_XE, r.c2), (SLOT_D2, r.c3)], clamp))
    return ops


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["veuler_tiny_heun", "veuler_wn_heun", "v_tiny_cc_guided"])
def test_a_draw_free_table_and_its_hand_lowered_program_give_the_same_bits(name):
    """adf_sampler_run_table and adf_sampler_run_program must enqueue the same launches for the same work, so the results are compared with
    torch.equal, eager and graph-replayed.  veuler_tiny_heun: two-evaluation steps, a one-evaluation last step, ADF_CLIP_NONE rows (the raw-output
    route).  veuler_wn_heun: 1503 elements, the scalar tail of the update kernel.  v_tiny_cc_guided: NOT a sampler but VSampler's table with every b2
    set to 0, so no draw is read: ADF_CLIP_UNIT rows on the class-conditional net under cond_scale = 3 (two passes and the guidance combine per
    evaluation).  Without the noise its state may sit at the clamp; bit equality is the assertion, so nothing is asked of the saturated share, only
    that the result is finite and not constant."""
    sp = VC.spec(name)
    smp = CLS[sp["sampler"]](**VC.sampler_kwargs(sp))
    steps = smp._table(VC.sigmas_of(sp))[0]
    if sp["sampler"] == "v":
        for r in steps:
            r.b2 = 0.0                       # the hand-made table: VSampler's, without its noise
    assert all(r.a1 == 0.0 and r.b2 == 0.0 for r in steps)
    clips = {e.clip for r in steps for e in ([r.eval1, r.eval2] if r.second else [r.eval1])}
    if sp["sampler"] == "veuler":
        assert any(r.second for r in steps) and not steps[-1].second and clips == {_lib.CLIP_NONE}
    else:
        assert clips == {_lib.CLIP_UNIT} and sp["cond_scale"] == 3.0
    ops = lower_by_hand(steps, final_clamp=1)
    assert ops[-1].kind == _lib.PROG_LIN and ops[-1].clamp == 1 and sum(o.clamp for o in ops) == 1
    nfe = table_nfe(steps)
    pd = _lib.AdfProgDesc(num_ops=len(ops), result_slot=SLOT_X, x0_scale=1.0, use_graph=0)
    assert nfe == sum(o.kind == _lib.PROG_EVAL for o in ops) == _lib.load_library().adf_sampler_program_nfe(C.byref(pd), (_lib.AdfProgOp * len(ops))(*ops))
    net = device_net(sp["net"], sp["out_scale"])
    hd, noise = handle(net), VC.noise_of(sp).cuda()
    if sp["net"] == "wn":
        assert noise.numel() % 4 == 3
    cl = RC.labels(sp["net"])
    if cl is not None:
        hd.set_condition(cl.cuda(), noise.device, null_labels=False, cond_scale=sp["cond_scale"])
    for use_graph in (0, 1):
        pd = _lib.AdfProgDesc(num_ops=len(ops), result_slot=SLOT_X, x0_scale=1.0, use_graph=use_graph)
        yt = counted(hd, nfe, use_graph, lambda: run_table(hd, steps, noise, None, x0=1.0, clamp=1, use_graph=use_graph).cpu())
        yp = counted(hd, nfe, use_graph, lambda: hd.sampler_run_program(pd, (_lib.AdfProgOp * len(ops))(*ops), noise).cpu())
        print(name, "graph" if use_graph else "eager", "differing entries", int((yt != yp).sum()), "of", yt.numel(), "max |y|", float(yt.abs().max()),
              "share |y| >= 1", float((yt.abs() >= 1).float().mean()))
        assert bool(torch.isfinite(yt).all()) and float(yt.min()) < float(yt.max())
        assert torch.equal(yt, yp), (name, use_graph)
