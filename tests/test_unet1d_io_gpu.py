"""The waveform transforms of the HIP UNet1dBase (to_in / to_out, csrc/adf_kernels.hip), the denoise epilogue of to_out, cfg_combine_kernel with the two-pass
guidance path, and label conditioning, off the point every other GPU test leaves them at: window 8 / stride 2 / one waveform channel / 16 or 64 filters (win16 of
tests/test_unet1d_sweep_gpu.py: one block of to_out), the epilogue through goldens of config_tiny only, class_embed_kernel at channels 16 and 64.

Cases: oracle/unet1d_sweep.py IO_CASES, the smallest net that reaches the transforms (multipliers [m0, 2], factors [2], one block, no attention).  to_out owns
256 feature rows (L / stride) per block plus a halo of ceil(window / stride) rows on either side.  Which kernel a case reaches is derived from the launchers' gates
in tests/test_oracle_unet1d_io.py (to_in: "rows" = to_in_rows_kernel, else to_in_kernel; to_out per mode fp32 / bf16 / f32x3, gen = to_out_kernel, mfma N = N K steps):
  k3s1       16 / 16 filters, 3 / 1 (pad 1, halo 3), 4 ch, 2 x 556     stride 1 (k0 always 0); three blocks, the last of 44 rows       to_in general; gen / mfma direct 1 / gen
  k4s2       16 / 16, 4 / 2 (1, 2), 1 ch, 2 x 1044 (522 rows)          last block of 10 rows                                            general; gen / mfma direct 1 / gen
  k16s2      16 / 16, 16 / 2 (7, 8), 2 ch, 2 x 516 (258)               largest halo; a second block of 2 rows < halo; 8 taps per output  general; gen / mfma direct 1 / gen
  k8s8       16 / 16, 8 / 8 (0, 1), 1 ch, 2 x 2096 (262)               pad 0, one tap per output, 8 trips of the output loop             general; gen / mfma direct 1 / gen
  k9s3       16 / 16, 9 / 3 (3, 3), 2 ch, 3 x 1548 (516)               odd window and stride                                            general; gen / mfma direct 1 / gen
  k12s4      16 / 64, 12 / 4 (4, 3), 1 ch, 2 x 1184 (296)              64 filters off window 8                                          general; gen / mfma staged 4 / x3 64
  k16s4n128  32 / 128, 16 / 4 (6, 4), 2 ch, 2 x 2080 (520)             window limit, three blocks, blockIdx.z = 1                       general; gen / mfma direct 8 / x3 128
  k8s2n128   32 / 128, 8 / 2, 1 ch, 2 x 1036 (518)                     128 filters at the shipped window                                rows (32 / 16 chunks); gen / mfma direct 8 / x3 128
  k8s2n96    24 / 96, 8 / 2, 1 ch, 2 x 524 (262)                       24 / 12 chunks per row                                           general; gen / mfma direct 6 / gen
  k8s2n160   40 / 160, 8 / 2, 1 ch, 2 x 524                            above 128 filters                                                general; gen / gen / gen
  k8s2st     64 / 64, 8 / 2, 2 ch, 2 x 1036 (518)                      stereo at the shipped width                                      general; gen / mfma staged 4 / x3 64
  c24, c40, c320   class-conditional, channels 24 (5 classes, 3 x 512), 40 (7, 2 x 512), 320 (3, 2 x 256; fp32 and bf16), labels with 0 and num_classes - 1:
             wave_sum over a partial wave, the second trip of the 256-thread stride loops of class_embed_kernel (320) and time_embed_kernel at 321 features.
             c320 was not refused: launch_class_embed serves up to 512 channels, which UNet1dConfig.validate_device now restates.

What is held (bars of the sweep module through its check(): fp32 FP32_TIGHT = 5e-5 of the float64 oracle, bf16 teacher-forced _bf16_tol, f32x3 forced X3_LAUNCH_TOL =
2.8e-6 and free-running F32X3_TOL = 2e-4; "to_in" and the output among the compared tensors, "class_emb" too for c*, read through adf_debug_tap_copy and also
held to FP32_TIGHT of the float64 LabelEmbedder in every mode):
  a  every tensor of every case in its modes (41 runs); b  one k16s2 handle in fp32 and one in bf16 through L = 512 / 508 / 516 / 1024 (256 / 254 / 258 / 512 rows);
  c  the epilogue: EluDiffusion(sigma_data = 1).denoise_fn on x = noise * sqrt(sigma^2 + 1), per-sample sigmas (0.05, 3) or (0.05, 1, 3) and each as a scalar, in
     all three modes, against clamp(c_skip x + c_out F, -1, 1) in float64 with the device's own rows (adf_debug_coef_rows, which now answers after adf_denoise);
  d  the same calls in fp32 against oracle/edm.py's denoiser in float64 at FP32_TIGHT;
  e  every label dropped (cond_drop_prob = 1), and denoise_fn at cond_scale = 2.5 against cfg_combine_kernel's arithmetic;
  and adf_create's own refusal of a window and stride of different parity, a stride above the window or below 1 (NativeHandle past the constructor).
Nothing goes to the device after a run that raised anything but a clean refusal (R.SWEEP_TROUBLE, _DEVICE_TROUBLE).

F taken separately is NOT reliably the fused pass's accumulator, in any mode.  to_out itself has no atomics, but the GroupNorm statistics in front of it are summed
in an order that changes from run to run (fp32 LDS atomics in gn_stats_kernel, atomics in the conv epilogues: tests/test_unet1d_sweep_gpu.py, "The split-bf16
mode").  Measured with three denoise and three raw passes per net: at widths whose rows are no power-of-two number of chunks (k8s2n160: 80 channels) every fp32 pass
differs from every other from down0.block0.h1 on (77 000 of 83 840 elements of up0.conv), which is 1.6e-6 on the output in fp32 and 2e-5 in f32x3 (the operands
split differently); at the other widths most passes agree bit for bit and one in three or four differs in a few elements, which in bf16 is a flipped rounding: up to
2.8e-2 of the output.  So the strict comparison would fail at random, and FP32_TIGHT against the denoiser on the separate F would too in bf16.  Instead (test c):
  strict   the two-rounding bar 4 * 2^-24 (|c_skip x| + |c_out F|) against the separate raw pass wherever that pass stored bit-equal rows in front of to_out (the
           recorded up0.conv of both passes; up to three raw passes are tried), and test_the_two_rounding_bar_was_held_in_every_mode asserts it was, in each mode;
  always   F = to_out in float64 on the rows the fused pass ITSELF recorded, the bar widened by the worst case of to_out's accumulation (to_out_float64: derived,
           K 2^-24 sum |h w| with K = filters * ceil(window / stride), 3 K 2^-24 + 2^-15 on the split kernel).
The guided path needs neither: the two raw passes of the SAME evaluation are read back ("cfg.cond" / "cfg.null", new names of adf_debug_tap_copy) and the bar is
6 * 2^-24 (|c_skip x| + |c_out nl| + |c_out (fc - nl) scale|): at most five roundings on a term.

Measured on one MI355X.  a, worst tensor (output), fp32 | bf16 forced | f32x3 forced, free-running worst:
  k3s1       up0.block0 6.4e-7 (6.6e-7) | up0.block0.h1 4.7e-5 (4.3e-8) | up0.block0.h1 7.0e-7 (8.1e-8), 1.3e-5
  k4s2       down0.block0 5.9e-7 (5.0e-7) | mid.pre.h1 9.0e-5 (3.6e-8) | down0.block0.h1 6.1e-7 (9.2e-8), 1.0e-5
  k16s2      up0.block0 7.0e-7 (6.2e-7) | down0.block0 4.6e-5 (7.4e-8) | up0.block0.h1 8.3e-7 (9.8e-8), 1.5e-5
  k8s8       up0.conv 7.6e-7 (6.6e-7) | down0.block0 1.5e-4 (1.4e-8) | mid.post.h1 6.8e-7 (7.3e-8), 1.3e-5
  k9s3       mid.pre.h1 7.1e-7 (5.6e-7) | up0.block0 8.1e-5 (3.9e-8) | down0.block0.h1 7.6e-7 (7.8e-8), 1.1e-5
  k12s4      up0.block0.h1 6.6e-7 (3.5e-7) | mid.post 8.7e-5 (1.0e-7) | mid.pre.h1 8.0e-7 (9.0e-8), 1.0e-5
  k16s4n128  mid.pre.h1 6.7e-7 (5.3e-7) | up0.block0 1.2e-4 (1.6e-7) | mid.pre.h1 7.5e-7 (1.1e-7), 9.8e-6
  k8s2n128   up0.conv 6.9e-7 (5.7e-7) | mid.post 1.2e-4 (1.8e-7) | mid.pre.h1 6.6e-7 (1.3e-7), 1.2e-5
  k8s2n96    down0.block0.h1 6.1e-7 (5.5e-7) | mid.post 7.5e-5 (1.4e-7) | mid.pre.h1 9.4e-7 (1.7e-7), 1.2e-5
  k8s2n160   mid.post.h1 7.2e-7 (6.7e-7) | up0.block0.h1 2.2e-4 (4.6e-7) | mid.post.h1 7.4e-7 (2.1e-7), 1.2e-5
  k8s2st     up0.conv 9.0e-7 (5.7e-7) | up0.block0 9.0e-5 (1.1e-7) | down0.block0 6.8e-7 (9.0e-8), 1.3e-5
  c24        up0.block0.h1 7.5e-7 (4.5e-7) | up0.block0.h1 9.0e-5 (1.8e-7) | down0.block0.h1 7.3e-7 (9.2e-8), 1.1e-5;  class_emb 2.8e-7, every label dropped 2.2e-7
  c40        mid.post.h1 7.1e-7 (6.7e-7) | up0.block0.h1 1.2e-4 (2.0e-7) | mid.pre.h1 8.6e-7 (9.7e-8), 1.1e-5;          class_emb 5.4e-7, dropped 2.9e-7
  c320       up0.conv 1.5e-6 (6.6e-7) | mid.post 1.2e-4 (5.8e-7);                                                           class_emb 1.5e-6, dropped 9.3e-7
  every label dropped: fp32 at most 1.4e-6 (c320 up0.block0), bf16 1.4e-4, f32x3 forced 8.0e-7.
b  fp32 at most 7.8e-7 (L = 516, up0.block0.h1; output 5.6e-7), bf16 at most 1.6e-4 (L = 1024).
c  worst ratio to the two-rounding bar over the runs of a case (strict runs of all), fp32 / bf16 / f32x3: k3s1 0.41 (3 of 3) / 0.38 (3 of 3) / 0.37 (3 of 3); k9s3 0.41
   (4 of 4) / 0.42 (3 of 4) / 0.44 (4 of 4); k12s4 0.40 / 0.41 / 0.39 (3 of 3 each); k16s4n128 0.42 / 0.42 / 0.44 (3 of 3 each); k8s2n160 - (0 of 3) / 0.42 (3 of 3) /
   - (0 of 3).  Worst ratio to the derived bar on the pass's own rows: 0.079 (k9s3 fp32); k8s2n160 0.0025 / 0.0015 / 0.0018 (K = 640 makes that bound loose).
d  fp32 denoise_fn against the float64 denoiser: k3s1 3.4e-6, k9s3 2.4e-6, k12s4 1.7e-6, k16s4n128 2.1e-6, k8s2n160 3.8e-6.
e  guided, worst ratio to the bar: c24 0.32 / 0.28 / 0.32, c40 0.29 / 0.34 / 0.26, c320 0.32 / 0.25; fp32 against the float64 guided denoiser 7.1e-6 / 6.8e-6 / 1.2e-5.
Timings: the module's 81 tests in 3.2 s; the slowest c320 fp32 (guided 0.36 s, every tensor 0.33 s), k3s1 fp32 0.17 s (the first of the module), every other under 0.15 s.

Teeth, checked once on value-only edits of adf_kernels.hip (no address or control-flow change of a load; a library per edit, not committed), whole module each:
  to_out_mfma / to_out_x3 storing acc[e] instead of 0 for rows outside [0, Lh)   caught by nothing, and by no possible case: the output loop of both kernels reads
                                              P only under its own `i >= 0 && i < Lh` guard, so those rows of P are never read -- the zeroing is redundant, not untested
  bf[ks] zeroed for ks >= 4                   every tensor k16s4n128 / k8s2n128 / k8s2n96 in bf16 (forced output 0.65 / 0.70 / 0.47 of 5e-4) and the k16s4n128 bf16
                                              epilogue (6058 times the derived bar)
  to_out_x3_kernel without al * bh            every tensor k12s4 / k16s4n128 / k8s2n128 / k8s2st in f32x3 (forced output 1.6e-3 .. 1.9e-3 of 2.8e-6) and the k12s4 /
                                              k16s4n128 f32x3 epilogue on the pass's own rows (11 / 3.5 times the derived bar)
  k0 = (l + pad) % stride replaced by 0       67 of 81: every test that compares an output with an oracle or with the pass's own rows, but those of k3s1 (stride 1, where k0 is 0)
  to_in_kernel's p >= L guard -> p >= L - 1   56 of 81: every case and mode of a, b, d and e but k8s2n128 (the row form)
  c_skip / c_out at coef_bstride = 0          28 of 81: all 15 epilogue tests, all 5 end-to-end tests, all 8 guided tests (nothing of a or b, as it should)
"""
import contextlib

import pytest
import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib
from audiodiffuser_amd.config import UNet1dConfig
from audiodiffuser_amd.net import NativeHandle
import gpu_helpers as R
from oracle import edm as E
from oracle import unet1d_sweep as SW
from test_gpu_parity import FP32_TIGHT
from test_unet1d_sweep_gpu import check

pytestmark = pytest.mark.gpu

IO = SW.IO_CASES
EPILOGUE_CASES = ("k3s1", "k9s3", "k12s4", "k16s4n128", "k8s2n160")
LABEL_CASES = ("c24", "c40", "c320")
COND_SCALE = 2.5
EPS = 2.0 ** -24                                # half an fp32 ulp, relative: one rounding
_DEVICE_TROUBLE = []                            # anything but a clean refusal of the library: nothing of this module goes to the device after it


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    _lib.load_library()


@pytest.fixture(autouse=True)
def _device_still_trusted():
    assert not R.SWEEP_TROUBLE and not _DEVICE_TROUBLE, f"not started after: {(R.SWEEP_TROUBLE + _DEVICE_TROUBLE)[0]}"


@contextlib.contextmanager
def on_device():
    """Device calls outside gpu_helpers.sweep_device_run, held to its rule: a refusal of the library leaves the device as it was; anything else may not."""
    try:
        yield
        torch.cuda.synchronize()
    except Exception as e:
        if type(e).__name__ != "AdfError" or any(s in str(e).lower() for s in ("hip", "failed", "illegal", "fault")):
            _DEVICE_TROUBLE.append(f"{type(e).__name__}: {e}")
        raise


def run_io(cid, mode, net=None, shape=None, seed=None, cond_drop_prob=None, tag=None):
    cfg, shape0, seed0, _ = IO[cid]
    own = shape is None and seed is None and not cond_drop_prob            # the case's own inputs and labels: the float64 oracle is shared
    shape, seed = shape or shape0, seed0 if seed is None else seed
    w, w64 = SW.weights(cid, IO)
    x, t = SW.inputs(cfg, shape, seed)
    cl = SW.labels(cfg, shape[0])
    net = net if net is not None else R.sweep_make(cfg, w, mode)
    kw = dict(classes=cl, cond_drop_prob=cond_drop_prob)
    if mode == "bf16":
        rep = R.sweep_bf16_report(cfg, w, x, t, net, **kw)
    elif mode == "f32x3":
        rep = R.sweep_x3_report(cfg, w, w64, x, t, net, oracle=SW.float64_case(cid, IO) if own else None, **kw)
    else:
        rep = R.sweep_fp32_report(cfg, w, w64, x, t, net, oracle=SW.float64_case(cid, IO) if own else None, **kw)
    check(rep, mode, tag or cid)
    assert "to_in" in rep["taps"] and rep["y"].shape == (shape[0], cfg.in_channels, shape[1])
    if cl is not None:
        # the label embedding is fp32 arithmetic in every mode: held to the float64 oracle at the fp32 bar whatever bar check() has for the mode
        from oracle import unet1d as O
        with torch.no_grad():
            want = O.label_embedding(w64, cl, float(cond_drop_prob or 0.0))
        e = SW.rel(rep["got"]["class_emb"], want)
        print(f"{tag or cid} {mode}: class_emb vs float64 {e:.3e}")
        assert "class_emb" in rep["taps"] and e < FP32_TIGHT
    return rep


# ------------------------------------------------------------------ a. every tensor of every case
@pytest.mark.parametrize("cid,mode", [(c, m) for c, v in IO.items() for m in v[3]])
def test_every_tensor_of_every_io_case_vs_oracle(cid, mode):
    run_io(cid, mode)


# ------------------------------------------------------------------ b. one handle across the block edge
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_one_k16s2_handle_through_the_block_edge_of_to_out(mode):
    """L = 512, 508, 516, 1024 at window 16 / stride 2 (halo 8): 256 feature rows (exactly one block), 254, 258 (a second block of 2 rows) and 512 on ONE net;
    each result to its own oracle run."""
    cfg = IO["k16s2"][0]
    net = R.sweep_make(cfg, SW.weights("k16s2", IO)[0], mode)
    for i, l in enumerate((512, 508, 516, 1024)):
        assert l // cfg.stride == (256, 254, 258, 512)[i]
        run_io("k16s2", mode, net=net, shape=(2, l), seed=80 + i, tag=f"k16s2 L = {l}")


# ------------------------------------------------------------------ c / d. the denoise epilogue
def coef_rows(net, b):
    """The device's own (c_in, c_noise, c_skip, c_out) of the denoise call that just ran, one row per sample (a scalar sigma: its one row for all)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = net.native(dev).coef_rows(dev).cpu()
    assert rows.shape in ((b, 4), (1, 4)) and bool(torch.isfinite(rows).all())
    return rows.expand(b, 4).contiguous()


def sigma_runs(sig):
    return [("per-sample", dict(sigmas=sig))] + [(f"sigma={float(s):g}", dict(sigma=float(s))) for s in sig]


_ORACLE_D = {}


def oracle_denoised(cid, name, kw, cond_scale=1.0):
    """oracle/edm.py's denoiser in float64 on the case's denoise inputs (and labels), once per (case, sigma form)."""
    key = (cid, name, cond_scale)
    if key not in _ORACLE_D:
        cfg, shape, seed, _ = IO[cid]
        x, _ = SW.denoise_inputs(cfg, shape, seed)
        with torch.no_grad():
            _ORACLE_D[key] = E.make_denoiser(SW.weights(cid, IO)[1], cfg, 1.0, classes=SW.labels(cfg, shape[0]), cond_scale=cond_scale)(x.double(), **kw)
    return _ORACLE_D[key]


def clamped_share(d):
    return (d.abs() >= 1).double().mean(dim=(1, 2))


def to_out_float64(cfg, mode, w, rows_in):
    """to_out in float64 on the feature rows the device itself stored (the recorded "up0.conv" of the SAME pass) -> (F, sum of |h| |w| per output, relative
    bound of the device's accumulation).  The bound is the worst case of its arithmetic, nothing measured: fp32 accumulation of the K = num_filters *
    ceil(window / stride) products of an output, K * 2^-24 of sum |h w|; the bf16 MFMA form multiplies bf16 rows by the bf16-rounded weight exactly and
    accumulates in fp32 (the same K); the split form accumulates three products per term (3 K) and leaves a_lo b_lo and the split residuals, at most
    (2^-18 + 2^-16) |a b| < 2^-15 |a b| (tests/test_oracle_unet1d_x3.py: hi + lo leaves at most 2^-17 |x|)."""
    import torch.nn.functional as F
    nf = cfg.num_filters
    pad = cfg.window_length // 2 - cfg.stride // 2
    wo = w["unet.to_out.to_out.weight"]
    if mode == "bf16" and nf % 16 == 0 and nf <= 128:
        wo = wo.bfloat16().float()
    k = nf * -(-cfg.window_length // cfg.stride)
    rel = k * EPS if mode != "f32x3" or not (nf % 64 == 0 and nf <= 128) else 3 * k * EPS + 2.0 ** -15
    f = F.conv_transpose1d(rows_in.double(), wo.double(), stride=cfg.stride, padding=pad)
    fabs = F.conv_transpose1d(rows_in.double().abs(), wo.double().abs(), stride=cfg.stride, padding=pad)
    return f, fabs, rel


STRICT = {}                                     # (case, mode) -> [runs held to the two-rounding bar, runs in all]


def epilogue_figures(cid, mode):
    """-> [(run, D)] after holding every run as the docstring of test_denoise_epilogue_... says."""
    cfg, shape, seed, _ = IO[cid]
    b = shape[0]
    w, _ = SW.weights(cid, IO)
    x, sig = SW.denoise_inputs(cfg, shape, seed)
    net = R.sweep_make(cfg, w, mode)
    diff = A.EluDiffusion(sigma_data=1.0)
    dev = torch.device("cuda", torch.cuda.current_device())
    x64 = x.double()
    out = []
    count = STRICT.setdefault((cid, mode), [0, 0])
    for name, kw in sigma_runs(sig):
        dkw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
        with on_device(), torch.no_grad():
            d = diff.denoise_fn(x.cuda(), net=net, inference=True, **dkw).cpu()
            rows = coef_rows(net, b)
            h_d = net.native(dev).tap("up0.conv", b, dev).cpu()                  # what to_out read in the fused pass
            xin = rows[:, 0].view(b, 1, 1) * x                                   # one fp32 product, as to_in applies c_in
            for attempt in range(3):                                             # (the statistics of a pass are summed in an order that changes: see the docstring)
                f_raw = net(xin.cuda(), rows[:, 1].contiguous().cuda()).cpu()
                same = torch.equal(net.native(dev).tap("up0.conv", b, dev).cpu(), h_d)
                if same:
                    break
        assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(f_raw).all())
        c_skip, c_out = rows[:, 2].double().view(b, 1, 1), rows[:, 3].double().view(b, 1, 1)
        count[1] += 1
        ratio = None
        if same:
            # to_out has no atomics: on bit-equal rows F is the fused pass's accumulator, and the epilogue is one fmaf and one product
            f = f_raw.double()
            want = (c_skip * x64 + c_out * f).clamp(-1.0, 1.0)
            bar = 4 * EPS * ((c_skip * x64).abs() + (c_out * f).abs())           # two fp32 roundings, a factor of two over them
            ratio = float(((d.double() - want).abs() / bar.clamp_min(1e-300)).max())
            count[0] += 1
        f64, fabs, rel = to_out_float64(cfg, mode, w, h_d)
        pre = c_skip * x64 + c_out * f64
        bar2 = 4 * EPS * ((c_skip * x64).abs() + (c_out * f64).abs()) + c_out.abs() * rel * fabs
        ratio2 = float(((d.double() - pre.clamp(-1.0, 1.0)).abs() / bar2.clamp_min(1e-300)).max())
        share = clamped_share(pre)
        print(f"{cid} {mode} {name}: raw pass on bit-equal rows {same} (attempts {attempt + 1}); |D - expected| / two-rounding bar "
              f"{'-' if ratio is None else format(ratio, '.3f')}; from the pass's own rows / derived bar {ratio2:.4f} (accumulation bound {rel:.2e}); "
              f"clamped share per sample {[round(float(s), 3) for s in share]}")
        assert 0.0 < float((pre.abs() >= 1).double().mean()) < 1.0               # both sides of the clamp are in the comparison
        assert ratio is None or ratio <= 1.0, (cid, mode, name, ratio)
        assert ratio2 <= 1.0, (cid, mode, name, ratio2)
        out.append((name, d))
    return out


@pytest.mark.parametrize("cid,mode", [(c, m) for c in EPILOGUE_CASES for m in SW.ALL3])
def test_denoise_epilogue_from_the_devices_own_raw_pass_and_rows(cid, mode):
    """EluDiffusion(sigma_data = 1).denoise_fn with per-sample sigmas and with each of them as a scalar, the epilogue alone, held two ways:
      strict   against clamp(c_skip x + c_out F, -1, 1) in float64 from the raw output F of the same net on (c_in x, c_noise) and the device's own coefficient
               rows, to two fp32 roundings -- where that raw pass stored bit-equal rows in front of to_out (up to three raw passes are tried);
      always   against the same expression with F = to_out in float64 on the rows the fused pass ITSELF stored, the bar widened by the worst case of
               to_out's own accumulation (to_out_float64)."""
    cfg, shape, seed, _ = IO[cid]
    share = clamped_share(oracle_denoised(cid, "per-sample", dict(sigmas=SW.denoise_inputs(cfg, shape, seed)[1])))
    assert bool(((share > 0.1) & (share < 0.8)).all()), share                       # on the float64 oracle, not the device
    epilogue_figures(cid, mode)


def test_the_two_rounding_bar_was_held_in_every_mode():
    """Not vacuous: in each mode at least one run of the epilogue test found a raw pass on bit-equal rows (measured: see the module docstring)."""
    for cid in EPILOGUE_CASES:
        for mode in SW.ALL3:
            if (cid, mode) not in STRICT:                                           # (this test run on its own)
                epilogue_figures(cid, mode)
    print({f"{c} {m}": f"{v[0]} of {v[1]}" for (c, m), v in STRICT.items()})
    for mode in SW.ALL3:
        assert sum(v[0] for (c, m), v in STRICT.items() if m == mode) > 0, mode


@pytest.mark.parametrize("cid", EPILOGUE_CASES)
def test_denoise_end_to_end_fp32_vs_the_float64_denoiser(cid):
    """The same cases and inputs, the whole call against oracle/edm.py's denoiser run in float64, at FP32_TIGHT."""
    cfg, shape, seed, _ = IO[cid]
    _, sig = SW.denoise_inputs(cfg, shape, seed)
    for (name, d), (name_o, kw) in zip(epilogue_figures(cid, "fp32"), sigma_runs(sig)):
        assert name == name_o
        want = oracle_denoised(cid, name, kw)
        e = SW.rel(d, want)
        print(f"{cid} fp32 {name}: denoise_fn vs float64 denoiser {e:.3e}, clamped share {[round(float(s), 3) for s in clamped_share(want)]}")
        assert d.shape == want.shape and e < FP32_TIGHT, (cid, name, e)


# ------------------------------------------------------------------ e. labels off the presets
@pytest.mark.parametrize("cid,mode", [(c, m) for c in LABEL_CASES for m in IO[c][3]])
def test_every_label_dropped(cid, mode):
    """cond_drop_prob = 1: every row of class_embed_kernel takes the null embedding; every tensor as in a."""
    rep = run_io(cid, mode, cond_drop_prob=1.0, tag=cid + " null")
    rows = rep["got"]["class_emb"]
    assert all(torch.equal(rows[0], rows[i]) for i in range(1, rows.shape[0]))


@pytest.mark.parametrize("cid,mode", [(c, m) for c in LABEL_CASES for m in IO[c][3]])
def test_guided_denoise_from_the_devices_own_two_raw_passes(cid, mode):
    """cond_scale = 2.5: denoise_fn against cfg_combine_kernel's arithmetic in float64 on the device's own two raw passes of the SAME evaluation (labels and
    null labels: the recorded "cfg.cond" / "cfg.null") and its coefficient rows -- nl + (fc - nl) * scale, then c_skip * x + c_out * pred, each operation
    rounded on its own: at most five roundings on a term, bar 6 * 2^-24 times the sum of the magnitudes of the terms.  In fp32 also the whole call against
    oracle/edm.py's guided denoiser in float64, which holds the two recorded passes to be the labelled and the null one."""
    cfg, shape, seed, _ = IO[cid]
    b = shape[0]
    x, sig = SW.denoise_inputs(cfg, shape, seed)
    cl = SW.labels(cfg, b)
    net = R.sweep_make(cfg, SW.weights(cid, IO)[0], mode)
    diff = A.EluDiffusion(sigma_data=1.0)
    dev = torch.device("cuda", torch.cuda.current_device())
    x64 = x.double()
    for name, kw in sigma_runs(sig):
        dkw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
        with on_device(), torch.no_grad():
            d = diff.denoise_fn(x.cuda(), net=net, inference=True, cond_scale=COND_SCALE, classes=cl.cuda(), **dkw).cpu()
            rows = coef_rows(net, b)
            hd = net.native(dev)
            fc, nl = hd.tap("cfg.cond", b, dev).cpu().double(), hd.tap("cfg.null", b, dev).cpu().double()
        assert fc.shape == nl.shape == d.shape and bool(torch.isfinite(d).all()) and SW.rel(fc, nl) > 1e-2          # two different passes
        c_skip, c_out = rows[:, 2].double().view(b, 1, 1), rows[:, 3].double().view(b, 1, 1)
        pre = c_skip * x64 + c_out * (nl + (fc - nl) * COND_SCALE)
        bar = 6 * EPS * ((c_skip * x64).abs() + (c_out * nl).abs() + (c_out * (fc - nl) * COND_SCALE).abs())
        ratio = float(((d.double() - pre.clamp(-1.0, 1.0)).abs() / bar.clamp_min(1e-300)).max())
        print(f"{cid} {mode} guided {name}: worst |D - expected| / bar {ratio:.3f}; clamped share per sample {[round(float(s), 3) for s in clamped_share(pre)]}")
        assert 0.0 < float((pre.abs() >= 1).double().mean()) < 1.0
        assert ratio <= 1.0, (cid, mode, name, ratio)
        if mode == "fp32":
            e = SW.rel(d, oracle_denoised(cid, name, kw, COND_SCALE))
            print(f"{cid} fp32 {name}: guided denoise_fn vs float64 denoiser {e:.3e}")
            assert e < FP32_TIGHT, (cid, name, e)
    # a plain forward afterwards: the two passes are no longer the last evaluation's, and the library says so
    with on_device(), torch.no_grad():
        net(x.cuda(), torch.zeros(b).cuda(), classes=cl.cuda())
        with pytest.raises(_lib.AdfError, match="unknown tap cfg.cond"):
            net.native(dev).tap("cfg.cond", b, dev)


# ------------------------------------------------------------------ the library's own refusals
def test_adf_create_refuses_what_validate_device_refuses_with_the_transforms_named():
    """A handle built past the constructor (NativeHandle on an unvalidated configuration): stride and window of different parity, stride above the window,
    stride below 1.  A clean refusal: nothing is launched."""
    for wl, st, what in ((6, 3, "different parity"), (7, 2, "different parity"), (8, 3, "different parity"), (4, 6, "stride above window_length"),
                         (4, 0, "stride must be at least 1")):
        cfg = UNet1dConfig(channels=16, num_filters=16, multipliers=[1, 2], factors=[2], num_blocks=[1], attentions=[False], use_attention_bottleneck=False,
                           window_length=wl, stride=st)
        with pytest.raises(_lib.AdfError, match=r"adf_create: unet\.to_in / unet\.to_out: .*" + what):
            NativeHandle(cfg, "fp32")
    for wl, st in ((6, 2), (9, 3), (4, 4), (3, 1)):
        NativeHandle(UNet1dConfig(channels=16, num_filters=16, multipliers=[1, 2], factors=[2], num_blocks=[1], attentions=[False],
                                  use_attention_bottleneck=False, window_length=wl, stride=st), "fp32").close()
