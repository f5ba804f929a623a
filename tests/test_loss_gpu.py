"""GPU: the validation loss on the device -- ``adf_diffusion_loss`` (noising, one ``adf_denoise`` evaluation, weighted per-sample squared error) and
the route ``Diffusion.forward`` takes to it, on the nets of tests/rf_cases.py at their smallest shapes and on a row-geometry sweep of the WaveNet.

What is compared with what
  * the noisy input with the CPU's fp32 tensor expression, bit for bit (the kernel rounds every operation on its own);
  * the losses with the float64 loss of the call's OWN prediction: bar 1e-6 per sample, relative (derived and emulated in tests/test_loss_host.py);
  * the prediction with ``adf_denoise`` on the returned noisy input under the same handle state: bit for bit on the WaveNet; on the U-Nets, whose
    GroupNorm statistics are summed with atomics, within 1e-4 max-norm relative, five times the largest run-to-run figure the project records for them
    (2e-5 on the ADM net, 5e-7 on the others: tests/test_rf_gpu.py);
  * the plugin classes end to end with tests/loss_ref.py in float64 around the oracle nets (fp32 for the ADM net): the project's 1e-3, per sample.

Row geometry.  N = C * L elements per sample; the kernels take 16-byte vectors on the aligned body of a row and single elements before and after it,
in chunks of ``_lib.LOSS_CHUNK`` elements.  Only the WaveNet takes any T, so the sweep runs on its handle: T in {1, 3, 5, 501, chunk - 1, chunk,
chunk + 1, 4099, 70001} x B in {1, 3}, each with the three loss kinds, the buffers placed so that all pointers share phase 0 ("aligned"), share phase 1
("shifted": every row start misaligned even at N % 4 == 0) or disagree ("mixed": the element-by-element form).  The census of what that covers is
asserted below.  Output buffers carry guard bands.

Measured on one MI355X: tests/golden/loss_report.json (with ADF_LOSS_REPORT=<path> set, this module writes its figures to that file)."""
import ctypes as C
import functools
import json
import os

import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
import loss_ref as LR
import rf_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3                   # the project's bar for one call against the float64 restatement (tests/test_rf_gpu.py)
BF16_TOL = 6e-2              # tests/test_gpu_parity.py: bf16 storage against the fp32 mode
LOSS_BAR = 1e-6              # the loss kernels against the float64 loss of the same prediction (tests/test_loss_host.py)
PRED_BAR = 1e-4              # pred against adf_denoise on the U-Nets: 5 x 2e-5, the largest recorded run-to-run figure (atomics in GroupNorm)
SENTINEL = -12345.0
CHUNK = _lib.LOSS_CHUNK
SEED = 23
REPORT = {}

# kind of tests/loss_ref.py -> (ADF_LOSS_*, arguments of set_preconditioning)
DEVICE_KIND = {"edm": (_lib.LOSS_X0_EDM, (_lib.PRECOND_EDM,)), "ve": (_lib.LOSS_X0_INV_SIGMA2, (_lib.PRECOND_VE,)),
               "vp": (_lib.LOSS_X0_INV_SIGMA2, (_lib.PRECOND_VP, 0.1, 19.9, 1000.0)), "rf": (_lib.LOSS_RF, (_lib.PRECOND_RF,))}
# (floats in front of the inputs, floats in front of the outputs): the phase of a pointer is its lead modulo 4
PLACEMENTS = {"aligned": (64, 64), "shifted": (65, 65), "mixed": (64, 65)}


def rel_b(a, b):
    """Largest per-sample relative distance of two [B] loss vectors."""
    return float(((a.double() - b.double()).abs() / b.double().abs()).max())


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("ADF_LOSS_REPORT")
    if REPORT and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def make_net(net_name, dtype="fp32"):
    cfg, w = RC.weights(net_name, 1.0)
    if net_name in ("tiny", "tiny_cc"):
        net = A.UNet1dBase.from_config(cfg, compute_dtype=dtype)
    elif net_name == "u2d":
        net = A.UNet2dBase(**cfg.to_kwargs())
    elif net_name == "adm":
        net = A.UNetModel.from_config(cfg)
    else:
        net = A.WaveNetNoise.from_config(cfg)
    net.load_state_dict(w, strict=True)
    net.cond_drop_prob = 0.0
    return net.cuda()


device_net = functools.lru_cache(maxsize=None)(make_net)          # one net (and handle) per name for the whole module


def handle(net):
    return net.native(torch.device("cuda", torch.cuda.current_device()))


@functools.lru_cache(maxsize=None)
def oracle(net_name):
    cfg, w = RC.weights(net_name, 1.0)
    dt = RC.ref_dtype(net_name)
    return RC.oracle_net(net_name, cfg, w, dt), dt


# ---- the C call with placed, guarded buffers -------------------------------------------------------------------------------------------------
def placed(src, lead):
    """A device copy of ``src`` that starts ``lead`` floats into a sentinel-filled buffer (torch's allocations are 16-byte aligned): (buffer, view)."""
    n = src.numel()
    buf = torch.full((lead + n + 64,), SENTINEL, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    view = buf[lead:lead + n]
    view.copy_(src.reshape(-1))
    return buf, view


def guards_intact(buf, lead, n):
    return bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n:] == SENTINEL).all())


def raw_call(hd, kind, x, noise, sig, placement="aligned", sigma_data=LR.SIGMA_DATA):
    """``adf_diffusion_loss`` of loss_ref kind ``kind`` with both outputs kept, on CPU inputs: (losses, x_noisy, pred) on the CPU.  The handle's
    preconditioning is set to the kind's; the clipping and the condition are the caller's."""
    loss_kind, precond = DEVICE_KIND[kind]
    hd.set_preconditioning(*precond)
    lead_in, lead_out = PLACEMENTS[placement]
    n, b = x.numel(), x.shape[0]
    _, vx = placed(x, lead_in)
    _, vz = placed(noise, lead_in)
    bxn, vxn = placed(torch.full((n,), SENTINEL), lead_out)
    bpr, vpr = placed(torch.full((n,), SENTINEL), lead_out)
    sg = sig.to(torch.float32).cuda().contiguous()
    losses = torch.full((b + 8,), SENTINEL, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    counters = hd.counters()
    with torch.cuda.device(0):
        hd.check(hd.lib.adf_diffusion_loss(hd.h, loss_kind, p(vx), p(vz), p(sg), float(sigma_data), p(losses), p(vxn), p(vpr), b, hd._length(x),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "adf_diffusion_loss")
    torch.cuda.synchronize()
    assert hd.counters() == counters, "adf_diffusion_loss moved a field of adf_run_counters"      # also where the call made a new (B, L) workspace
    assert guards_intact(bxn, lead_out, n) and guards_intact(bpr, lead_out, n), "a kernel wrote outside its output"
    assert bool((losses[b:] == SENTINEL).all())
    return losses[:b].cpu(), vxn.cpu().view(x.shape), vpr.cpu().view(x.shape)


def check_raw_case(hd, tag, kind, x, noise, sig, placement, bitwise_pred, assert_pred=True):
    """Checks 1 - 3 of the issue on one call: the mix bit for bit, the loss of the call's own prediction, the prediction against adf_denoise
    (``assert_pred=False``: that figure is only recorded)."""
    losses, x_noisy, pred = raw_call(hd, kind, x, noise, sig, placement)
    assert torch.equal(x_noisy, LR.mix(kind, x, noise, sig.to(torch.float32))), (tag, "x_noisy is not the fp32 expression bit for bit")
    want = LR.loss_of_pred(kind, x.double(), noise, pred, sig.to(torch.float32))
    e_loss = rel_b(losses, want)
    den = hd.denoise(x_noisy.cuda(), LR.SIGMA_DATA, sigmas=sig.to(torch.float32).cuda()).cpu()
    e_pred = rel(pred, den)
    rec = {"loss_vs_float64_of_own_pred": e_loss, "pred_vs_adf_denoise": e_pred}
    if not bitwise_pred:              # the denoiser's own run-to-run spread at these inputs: what pred_vs_adf_denoise is to be read against
        rec["adf_denoise_twice"] = rel(hd.denoise(x_noisy.cuda(), LR.SIGMA_DATA, sigmas=sig.to(torch.float32).cuda()).cpu(), den)
    print(tag, kind, placement, "losses", [round(float(v), 5) for v in losses], rec)
    REPORT.setdefault("raw", {})[f"{tag}/{kind}/{placement}"] = rec
    assert bool(torch.isfinite(losses).all()) and bool((losses > 0).all())
    assert e_loss <= LOSS_BAR, (tag, kind, e_loss)
    if bitwise_pred:
        assert torch.equal(pred, den), (tag, kind, e_pred)
    elif assert_pred:
        assert e_pred <= PRED_BAR, (tag, kind, e_pred)
    return losses


# ---- 1 - 3 on the U-Net shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", LR.KINDS)
@pytest.mark.parametrize("net_name", ["tiny", "tiny_cc", "u2d", "adm"])
def test_mix_loss_and_prediction_on_the_unet_shapes(net_name, kind):
    """The three U-Nets (the 1-D net also class-conditional).  The three loss kinds are edm (0), ve (1) and rf (2); they carry all three checks.  vp is
    loss kind 1 again under VPDiffusion's rows and is here for the mix and the loss at its sigmas: its prediction is compared with adf_denoise in the
    report only, next to ``adf_denoise_twice``, the distance of TWO adf_denoise calls on the same input, which every case records.  Under VP's rows that
    spread is itself above the bar on these random-weight nets (measured on one MI355X: 4.4e-4 .. 3.2e-3 on u2d, 2e-5 .. 1.7e-4 on tiny, 8e-5 on adm, against
    1e-6 / 4e-7 / 3e-7 for edm).  The time embedding is deterministic; what differs from run to run is the atomically summed GroupNorm statistics, and VP feeds
    c_noise = 999 t(sigma), several hundred, into the FiLM projections, whose large scales and shifts amplify that last-bit difference (and c_out = -sigma
    multiplies it again).  The premise of the 1e-4 bar, a run-to-run spread of at most 2e-5, does not hold there for the denoiser itself."""
    net = device_net(net_name)
    hd = handle(net)
    hd.set_dynamic_threshold(0.0)
    cl = RC.labels(net_name)
    if cl is not None:
        hd.set_condition(cl.cuda(), torch.device("cuda"), null_labels=False, cond_scale=1.0)
    shape = RC.NETS[net_name][3]
    x, noise = LR.inputs(shape)
    sig = LR.sigmas_of(kind, LR.coefs(kind, shape[0]))
    before, den_before = hd.loss_calls(), hd.counters()["denoise_calls"]
    check_raw_case(hd, net_name, kind, x, noise, sig, "aligned", bitwise_pred=False, assert_pred=kind != "vp")
    assert hd.loss_calls() == before + 1
    assert hd.counters()["denoise_calls"] == den_before + 2           # the comparison's own two adf_denoise calls; the loss call does not count as one


# ---- 1 - 3 over the row geometry (WaveNet) -----------------------------------------------------------------------------------------------------
SWEEP_T = (1, 3, 5, 501, CHUNK - 1, CHUNK, CHUNK + 1, 4099, 70001)
SWEEP_B = (1, 3)
SWEEP_KINDS = ("edm", "ve", "rf")                                     # the three ADF_LOSS_* kinds


def sweep_placement(ti, ki):
    return tuple(PLACEMENTS)[(ti + ki) % 3]


def row_geometry(phase, b, n):
    """The kernels' split of row b (csrc/adf_loss.h): (head, 16-byte vectors, tail), or None for the element-by-element form."""
    if phase < 0:
        return None
    head = min(n, (4 - (phase + b * n) % 4) % 4)
    nv = (n - head) // 4
    return head, nv, n - head - 4 * nv


def sweep_census():
    seen = set()
    for ti, t in enumerate(SWEEP_T):
        for bsz in SWEEP_B:
            for ki in range(len(SWEEP_KINDS)):
                lead_in, lead_out = PLACEMENTS[sweep_placement(ti, ki)]
                phase = lead_in % 4 if lead_in % 4 == lead_out % 4 else -1
                chunks = -(-t // CHUNK)
                if t == 1:
                    seen.add("single element")
                if chunks >= 16:
                    seen.add("many chunks")
                for b in range(bsz):
                    g = row_geometry(phase, b, t)
                    if g is None:
                        seen.add("element by element" + (", several chunks" if chunks > 1 else ""))
                        continue
                    head, nv, tail = g
                    if nv == 0 and t > 1:
                        seen.add("row shorter than one vector")
                    if head > 0 and nv > 0:
                        seen.add("misaligned row start")
                    if head == 0 and tail == 0 and nv * 4 == CHUNK:
                        seen.add("exactly full chunk")
                    if nv > 0 and nv % (CHUNK // 4) == 1:
                        seen.add("one vector into the next chunk")
                    if 0 < nv <= (chunks - 1) * (CHUNK // 4):
                        seen.add("a block without vectors")
                    if head > 0 and tail > 0:
                        seen.add("head and tail")
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("bsz", SWEEP_B)
@pytest.mark.parametrize("ti", range(len(SWEEP_T)))
def test_row_geometry_sweep_on_the_wavenet(ti, bsz):
    assert {"single element", "row shorter than one vector", "misaligned row start", "exactly full chunk", "many chunks", "element by element",
            "element by element, several chunks", "one vector into the next chunk", "a block without vectors", "head and tail"} <= sweep_census()
    assert {CHUNK - 1, CHUNK, CHUNK + 1} <= set(SWEEP_T)
    t = SWEEP_T[ti]
    hd = handle(device_net("wn"))
    hd.set_dynamic_threshold(0.0)
    x, noise = LR.inputs((bsz, 1, t), seed=5 + ti)
    for ki, kind in enumerate(SWEEP_KINDS):
        sig = LR.sigmas_of(kind, LR.coefs(kind, bsz))
        check_raw_case(hd, f"wn_T{t}_B{bsz}", kind, x, noise, sig, sweep_placement(ti, ki), bitwise_pred=True)


# ---- 4: repeatability ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_calls_give_identical_losses_on_the_wavenet():
    hd = handle(device_net("wn"))
    hd.set_dynamic_threshold(0.0)
    x, noise = LR.inputs((3, 1, 4099))
    for kind in SWEEP_KINDS:
        sig = LR.sigmas_of(kind, LR.coefs(kind, 3))
        first = raw_call(hd, kind, x, noise, sig, "aligned")
        again = raw_call(hd, kind, x, noise, sig, "aligned")
        assert all(torch.equal(a, b) for a, b in zip(first, again)), kind
        moved = raw_call(hd, kind, x, noise, sig, "shifted")          # another vector / scalar split of the same rows: same elements per block
        print("repeat", kind, [float(v) for v in first[0]], "shifted placement differs by", rel_b(moved[0], first[0]))
        assert rel_b(moved[0], first[0]) <= LOSS_BAR


# ---- 5: end to end through the plugin classes ------------------------------------------------------------------------------------------------------
E2E_DIFFS = {"edm": ("edm", lambda: A.EluDiffusion(0.2), {}), "edm_dyn": ("edm", lambda: A.EluDiffusion(0.2, dynamic_threshold=0.9), {"dynamic_threshold": 0.9}),
             "ve": ("ve", lambda: A.VEDiffusion(), {}), "vp": ("vp", lambda: A.VPDiffusion(0.1, 19.9, 1000), {}), "rf": ("rf", lambda: A.ReFlow(), {})}
E2E_NETS = [("tiny", "plain"), ("adm", "plain"), ("wn", "plain"), ("tiny_cc", "infer_cfg"), ("tiny_cc", "train_cdp0"), ("u2d", "infer_cfg"),
            ("u2d", "train_cdp0")]


def seeded_noise(x_dev):
    """The draw ``forward`` makes first: reseed and draw ``randn_like`` once on the same device."""
    torch.manual_seed(SEED)
    return torch.randn_like(x_dev).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("diff_name", list(E2E_DIFFS))
@pytest.mark.parametrize("net_name,mode", E2E_NETS)
def test_plugin_classes_end_to_end_vs_float64_restatement(net_name, mode, diff_name):
    kind, make_diff, ref_kw = E2E_DIFFS[diff_name]
    net = device_net(net_name)
    hd = handle(net)
    shape, cl = RC.NETS[net_name][3], RC.labels(net_name)
    x, _ = LR.inputs(shape)
    coef = LR.coefs(kind, shape[0])
    kw = {} if cl is None else {"classes": cl.cuda()}
    fkw = dict(inference=True, cond_scale=2.0) if mode == "infer_cfg" else {}
    before, counters = hd.loss_calls(), hd.counters()
    with torch.no_grad():
        torch.manual_seed(SEED)
        got = make_diff()(x.cuda(), net, coef.cuda(), **fkw, **kw)
    assert hd.loss_calls() == before + 1 and got.shape == (shape[0],) and got.dtype == torch.float32 and got.is_cuda
    assert hd.counters() == counters                                  # no field moves: not net_passes either, one pass or two (guidance)
    noise = seeded_noise(x.cuda())
    net_o, dt = oracle(net_name)
    with torch.no_grad():
        want = LR.forward(kind, net_o, x.to(dt), noise, coef, cond_scale=2.0 if mode == "infer_cfg" else 1.0, **ref_kw)
    e = rel_b(got.cpu(), want)
    print(net_name, mode, diff_name, "losses", [round(float(v), 5) for v in got], "vs restatement", e)
    REPORT.setdefault("end_to_end", {})[f"{net_name}/{mode}/{diff_name}"] = {"rel_err": e, "losses": [float(v) for v in got]}
    assert bool(torch.isfinite(got).all()) and e <= TOL, (net_name, mode, diff_name, e)


# ---- 6: route witness ------------------------------------------------------------------------------------------------------------------------
def both_routes(diff, x_dev, net, coef_dev, **kw):
    """(forward, _tensor_loss) with the same seed; VPDiffusion's ``_tensor_loss`` takes the mapped sigmas."""
    with torch.no_grad():
        torch.manual_seed(SEED)
        a = diff(x_dev, net, coef_dev, **kw)
        torch.manual_seed(SEED)
        b = diff._tensor_loss(x_dev, net, diff.t_to_sigma(coef_dev) if isinstance(diff, A.VPDiffusion) else coef_dev, **kw)
    return a, b


@pytest.mark.gpu
def test_routes_that_stay_on_tensor_ops_do_not_count_and_equal_tensor_loss():
    """On the WaveNet, whose passes repeat bit for bit, so 'equal' can be exact."""
    net = device_net("wn")
    hd = handle(net)
    x, _ = LR.inputs((3, 1, 501))
    xd, t = x.cuda(), torch.tensor(LR.TIMES).cuda()
    mask = (torch.arange(501) < 400).view(1, 1, 501).expand(3, 1, 501).cuda()
    before = hd.loss_calls()
    for name, diff, net_arg, kw in (("x_mask", A.EluDiffusion(0.2), net, {"x_mask": mask}), ("VDiffusion", A.VDiffusion(), net, {}),
                                    ("ReFlow(for_edm=True)", A.ReFlow(for_edm=True), net, {}), ("foreign net", A.EluDiffusion(0.2), LR.toy_net, {})):
        a, b = both_routes(diff, xd, net_arg, t, **kw)
        assert a.shape == (3,) and torch.equal(a, b), name
        assert hd.loss_calls() == before, name


@pytest.mark.gpu
@pytest.mark.compat_branch
def test_x_mask_with_inference_stays_on_the_compatibility_branch():
    """inference=True with ``x_mask``: the tensor route's ``denoise_fn`` is handed the mask too and so is no adf_denoise call either; with
    ADF_REQUIRE_NATIVE set that is an error by design, hence the marker.  ``forward`` itself never reads the variable."""
    net = device_net("wn")
    hd = handle(net)
    x, _ = LR.inputs((3, 1, 501))
    mask = (torch.arange(501) < 400).view(1, 1, 501).expand(3, 1, 501).cuda()
    before = hd.loss_calls()
    a, b = both_routes(A.EluDiffusion(0.2), x.cuda(), net, torch.tensor(LR.SIGMAS).cuda(), inference=True, x_mask=mask)
    assert torch.equal(a, b) and hd.loss_calls() == before


@pytest.mark.gpu
@pytest.mark.parametrize("diff_name", ["edm", "vp", "rf"])
def test_device_route_agrees_with_tensor_loss_on_the_same_net(diff_name):
    kind, make_diff, _ = E2E_DIFFS[diff_name]
    net = device_net("tiny")
    hd = handle(net)
    x, _ = LR.inputs(RC.NETS["tiny"][3])
    before = hd.loss_calls()
    a, b = both_routes(make_diff(), x.cuda(), net, LR.coefs(kind, 3).cuda())
    assert hd.loss_calls() == before + 1                              # forward counted, _tensor_loss did not
    e = rel_b(a.cpu(), b.cpu())
    print("device route vs _tensor_loss", diff_name, e)
    REPORT.setdefault("device_vs_tensor_route", {})[diff_name] = e
    assert e <= TOL
    # the global generator is left where the tensor route leaves it: one randn_like(x)
    torch.manual_seed(SEED)
    with torch.no_grad():
        make_diff()(x.cuda(), net, LR.coefs(kind, 3).cuda())
    after_device = torch.rand(2, device="cuda")
    torch.manual_seed(SEED)
    torch.randn_like(x.cuda())
    assert torch.equal(after_device, torch.rand(2, device="cuda"))


@pytest.mark.gpu
def test_bf16_storage_through_the_loss_stays_near_the_fp32_mode():
    x, _ = LR.inputs(RC.NETS["tiny"][3])
    out = {}
    for dtype in ("fp32", "bf16"):
        net = device_net("tiny", dtype)
        before = handle(net).loss_calls()
        with torch.no_grad():
            torch.manual_seed(SEED)
            out[dtype] = A.EluDiffusion(0.2)(x.cuda(), net, torch.tensor(LR.SIGMAS).cuda()).cpu()
        assert handle(net).loss_calls() == before + 1
    e = rel_b(out["bf16"], out["fp32"])
    print("bf16 vs fp32 mode", e)
    REPORT["bf16_vs_fp32_mode"] = e
    assert bool(torch.isfinite(out["bf16"]).all()) and e < BF16_TOL


# ---- 7: capture ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_call_is_captured_into_a_callers_graph_and_replays_bit_for_bit():
    hd = handle(device_net("wn"))
    hd.set_dynamic_threshold(0.0)
    hd.set_preconditioning(_lib.PRECOND_EDM)
    x, noise = (t.cuda() for t in LR.inputs((3, 1, 501)))
    sig = torch.tensor(LR.SIGMAS).cuda()
    eager = hd.diffusion_loss(_lib.LOSS_X0_EDM, x, noise, sig, LR.SIGMA_DATA)              # the warm call: the plan's one allocation
    torch.cuda.synchronize()
    bytes_before, calls_before = hd.lib.adf_device_bytes(hd.h), hd.loss_calls()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # fails if the call allocates device memory or synchronises
        captured = hd.diffusion_loss(_lib.LOSS_X0_EDM, x, noise, sig, LR.SIGMA_DATA)
    assert hd.lib.adf_device_bytes(hd.h) == bytes_before and hd.loss_calls() == calls_before + 1
    for _ in range(2):
        captured.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)


# ---- 8: refusals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_name_the_argument():
    hd = handle(device_net("tiny"))
    hd.set_preconditioning(_lib.PRECOND_EDM)
    x, noise = (t.cuda() for t in LR.inputs((3, 1, 256)))
    sig, losses = torch.tensor(LR.SIGMAS).cuda(), torch.empty(3, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    before = hd.loss_calls()

    def call(kind=0, x_=x, noise_=noise, sig_=sig, sd=0.2, losses_=losses, handle_=hd):
        return handle_.lib.adf_diffusion_loss(handle_.h, kind, p(x_), p(noise_), p(sig_), sd, p(losses_), p(None), p(None), 3, 256, stream)

    for kwargs, names in ((dict(kind=3), "kind"), (dict(kind=-1), "kind"), (dict(x_=None), "x is null"), (dict(noise_=None), "noise is null"),
                          (dict(sig_=None), "sigmas_dev is null"), (dict(losses_=None), "losses is null"), (dict(sd=0.0), "sigma_data"),
                          (dict(sd=-1.0), "sigma_data")):
        assert call(**kwargs) != 0, kwargs
        msg = hd.lib.adf_last_error(hd.h).decode()
        assert msg.startswith("adf_diffusion_loss") and names in msg, (kwargs, msg)
    # an output that overlaps an input or the other output (equal or shifted pointers alike)
    out_a, out_b = torch.empty(3 * 256 + 64, device="cuda"), torch.empty(3 * 256, device="cuda")
    for xn_, pr_, names in ((x, None, "x_noisy_out overlaps"), (noise, None, "x_noisy_out overlaps"), (None, x, "pred_out overlaps x or noise"),
                            (None, noise, "pred_out overlaps x or noise"), (out_a, out_a[64:], "pred_out overlaps x_noisy_out"),
                            (out_b, out_b, "pred_out overlaps x_noisy_out")):
        assert hd.lib.adf_diffusion_loss(hd.h, 0, p(x), p(noise), p(sig), 0.2, p(losses), p(xn_), p(pr_), 3, 256, stream) != 0, names
        msg = hd.lib.adf_last_error(hd.h).decode()
        assert msg.startswith("adf_diffusion_loss") and names in msg, (names, msg)
    assert call(kind=_lib.LOSS_X0_INV_SIGMA2, sd=0.0) == 0            # sigma_data is read by ADF_LOSS_X0_EDM only
    torch.cuda.synchronize()
    assert hd.loss_calls() == before + 1
    # a 2-D handle that was never told its image shape
    fresh = handle(make_net("u2d"))
    x2, n2 = (t.cuda() for t in LR.inputs((2, 2, 32, 16)))
    assert fresh.lib.adf_diffusion_loss(fresh.h, 0, p(x2), p(n2), p(sig), 0.2, p(losses), p(None), p(None), 2, 512, stream) != 0
    assert "adf_set_image_shape" in fresh.lib.adf_last_error(fresh.h).decode()
    assert fresh.loss_calls() == 0
