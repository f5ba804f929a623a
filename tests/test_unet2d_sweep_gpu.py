"""The HIP UNet2dBase held layer by layer to a float64 oracle over a sweep of structures and image shapes.

tests/test_unet2d_gpu.py runs one point of what the plugin accepts (config_sc09: dim 128, 8 groups, 2 heads, widths 128 / 256, images whose
pixel counts are multiples of 256).  The cases below reach what that point never does: partial last workgroups of the cross-embed and final
convs, fine-statistics groups of 1 and 2 channels, widths 160 / 192 / 320 / 384 / 512 and the 1024-channel concat, head dims 32 and 64 from the
2-D walker, head dim 128 at token counts off the 32-key tile, feed-forward widths 384 / 640 / 768 / 1024, global-context pooling over 1 to 1584
rows, the unscaled skip concat, two transformer layers per block, no middle attention, no final resnet block, one to four cross-embed kernels,
batches of 3, 5 and 7 with per-sample times and labels, and (fg2_b128: fg2's structure at B = 128, 32 x 32) the 128-pixel gather route of launch_conv2d,
which needs 512 tiles (fp32 oracle against float64 there: ups.0.0.h1 3.8e-6).

Every case compares the output AND every tensor the device walker records (``hd.tap_names()``, unsubsampled) with oracle/unet2d.py run in
float64 (``fine_taps``).  Bar per tensor: FP32_TIGHT = 5e-5 of max |reference| (the project's exact-fp32 bar), or 4 x the tensor's own
fp32-oracle-vs-float64-oracle distance where that distance exceeds FP32_TIGHT / 4 (the rule of tests/test_precond_gpu.py); the CPU test at the
top of this module shows the second clause never applies here (worst fp32-oracle tap over all cases: ups.0.0.h1 of wide3, 3.9e-6 < 1.25e-5).

Measured on one MI355X, worst device-vs-float64 tensor per case (and the output), all against the bar of 5e-5:
  wide3      ups.1.1.0.h1   3.1e-6   (out 2.8e-6)        sc09_tall   downs.1.2.0.h2  3.9e-6   (out 1.8e-6)
  fg1        downs.1.1.h1   3.1e-6   (out 1.8e-6)        sc09_wide   ups.2.1.1.h1    3.3e-6   (out 2.0e-6)
  fg2        ups.0.1.0.h1   3.9e-6   (out 2.6e-6)        sc09_cls7   ups.2.1.1.h1    3.6e-6   (out 2.3e-6)
  sc09_odd   ups.2.1.1.h1   3.7e-6   (out 2.1e-6)        sc09_cls7, labels dropped   ups.1.0.h1  3.4e-6   (out 2.0e-6)
  sc09_min   ups.2.1.1.h1   2.9e-6   (out 2.1e-6)        fg2_b128    ups.0.0.h1      4.8e-6   (out 2.2e-6)
One handle through four shapes: at most 3.4e-6.  Denoiser epilogue on wide3: EluDiffusion 1.7e-6, VDiffusion(for_edm) 1.3e-6.  fg1 sample 3 alone
against its row of the batch of 5: 2.7e-6 at worst (ups.0.1.1.h2), output 1.7e-6.  No case exposed a kernel defect.

That the sweep has teeth was checked once on four value-only edits of adf_unet2d.hip (not committed), each run against every case:
  cross-embed statistics without their ``live ?`` guard       caught by wide3 / fg1 / fg2 (init_resnet_block.h1: 3.5e-3 / 6.1e-3 / 9.4e-3) and the denoiser test
  head-dim-128 scores masked by ``j < kAttKT``, not ``j < nk``  caught by wide3, fg2 and every sc09 shape (first tensor over: the level's first .att, 0.18 to 0.88)
  scaled GroupNorm table without ``A *= scale1``              caught by every case with the skip scale on (ups.0.0.h1: 0.31 to 0.40)
  global-context merge with an unconditional ``expf(wm[w] - M)``   NOT caught, and cannot be: expf(-inf - M) is exactly 0 for the finite M a chunk always
                                                               has (one wave holds a row), so the guard is redundant and the edit changes no value
"""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import audiodiffuser_amd as A
from gpu_helpers import conv2d_trace_lines
from oracle import unet2d as U
import precond_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FP32_TIGHT = 5e-5            # tests/test_unet2d_gpu.py


def rel(a, b):
    """tests/test_unet2d_gpu.py: max abs difference over max abs of the reference."""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def _cfg(**kw):
    n = len(kw["dim_mults"])
    kw.setdefault("layer_attns", (True,) * n)
    kw.setdefault("layer_cross_attns", kw["layer_attns"])       # only sizes state-dict entries the forward never runs
    return U.UNet2dConfig(memory_efficient=True, **kw)


# id -> (constructor arguments, (B, H, W), weight seed)
CASES = {
    "wide3": (_cfg(dim=128, dim_mults=(1, 2, 4), channels=1, num_resnet_blocks=1, resnet_groups=8, layer_attns=(False, True, True),
                   layer_attns_depth=2, attn_heads=4, ff_mult=1.5, scale_skip_connection=False, final_resnet_block=False,
                   init_cross_embed_kernel_sizes=(1, 3, 7, 15)), (3, 40, 24), 21),
    "fg1": (_cfg(dim=160, dim_mults=(1, 2), channels=3, num_classes=3, num_resnet_blocks=2, resnet_groups=32, layer_attns=(True, True),
                 attn_heads=5, attend_at_middle=False, init_cross_embed_kernel_sizes=(3, 5)), (5, 12, 20), 22),
    "fg2": (_cfg(dim=192, dim_mults=(1, 2), channels=4, channels_out=2, num_resnet_blocks=1, resnet_groups=32, layer_attns=(False, True),
                 attn_heads=3, init_cross_embed_kernel_sizes=(7,)), (2, 44, 36), 23),
    "sc09_odd": (U.config_sc09(0), (3, 48, 80), 24),
    "sc09_min": (U.config_sc09(0), (1, 16, 16), 24),
    "sc09_tall": (U.config_sc09(0), (2, 160, 32), 24),
    "sc09_wide": (U.config_sc09(0), (1, 16, 208), 24),
    "sc09_cls7": (U.config_sc09(10), (7, 32, 48), 25),
}
# fg2's structure at the smallest batch x image whose first level (16 x 16, 192 channels: ny = 2) fills launch_conv2d's 128-pixel gather route:
# B*H*W/4 / 128 * 2 = 512 tiles (see test_large_batch_takes_the_128_pixel_gather_kernel)
CASES["fg2_b128"] = (CASES["fg2"][0], (128, 32, 32), 23)


def inputs(cfg, shape, seed=0):
    """x [B, channels, H, W], one time per sample (c_noise of the EDM wrapper lies in about [-1.6, 1.1]), one label per sample where the net has classes."""
    b, h, w = shape
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(b, cfg.channels, h, w, generator=g) * 0.5
    t = torch.linspace(-1.3, 0.9, b) if b > 1 else torch.tensor([0.35])
    cl = (torch.arange(b) * 7 + 2) % cfg.num_classes if cfg.num_classes else None
    return x, t, cl


@functools.lru_cache(maxsize=None)
def weights(cid):
    cfg, _, seed = CASES[cid]
    w = U.generate_weights(cfg, seed)
    return w, {k: v.double() for k, v in w.items()}


def oracle_run(cfg, w, w64, x, t, cl, cdp=0.0):
    """-> (float64 output, float64 fine taps, {name: fp32-oracle-vs-float64-oracle distance}) with "out" for the output."""
    f32, f64 = {}, {}
    with torch.no_grad():
        y32 = U.unet2d_forward(w, cfg, x, t, classes=cl, cond_drop_prob=cdp, fine_taps=f32)
        y64 = U.unet2d_forward(w64, cfg, x.double(), t.double(), classes=cl, cond_drop_prob=cdp, fine_taps=f64)
    assert y64.dtype == torch.float64 and all(v.dtype == torch.float64 for v in f64.values())
    assert list(f32) == list(f64)
    dist = {k: rel(f32[k], f64[k]) for k in f64}
    dist["out"] = rel(y32, y64)
    return y64, f64, dist


def bar_of(d):
    return FP32_TIGHT if d <= FP32_TIGHT / 4 else 4.0 * d


# ------------------------------------------------------------------ CPU: the bar is meaningful, and the oracle names every device tap
@pytest.mark.timeout(300)
@pytest.mark.parametrize("cid", list(CASES))
def test_fp32_oracle_fine_taps_within_a_quarter_of_the_bar_of_float64(cid):
    cfg, shape, seed = CASES[cid]
    w, w64 = weights(cid)
    x, t, cl = inputs(cfg, shape, seed)
    runs = [0.0, 1.0] if cid == "sc09_cls7" else [0.0]
    for cdp in runs:
        y64, f64, dist = oracle_run(cfg, w, w64, x, t, cl, cdp)
        names = U.walker_tap_names(cfg)
        assert len(set(names)) == len(names)
        missing = [k for k in names if k not in f64]
        assert not missing, missing
        b, (_, h, wd) = shape[0], shape
        assert f64["init_conv"].shape == (b, cfg.dim, h * wd) and y64.shape == (b, cfg.channels_out or cfg.channels, h, wd)
        worst = max(dist, key=dist.get)
        print(cid, "cond_drop", cdp, "taps", len(names), "worst fp32-vs-float64", worst, dist[worst])
        over = [(k, d) for k, d in dist.items() if not d <= FP32_TIGHT / 4]
        assert not over, over[:5]
        assert all(float(v.abs().max()) > 1e-3 for v in f64.values())          # nothing compared is (near) zero


# ------------------------------------------------------------------ GPU
def make(cfg, w):
    net = A.UNet2dBase(**cfg.to_kwargs())
    net.load_state_dict(w, strict=True)
    return net.cuda()


def run_and_compare(net, cfg, w, w64, x, t, cl, cdp=0.0, tag=""):
    """One device forward; the output and every recorded tensor against the float64 oracle.  Returns (device output, {name: device tap}) on the host."""
    dev = torch.device("cuda", torch.cuda.current_device())
    kw = {} if cl is None else dict(classes=cl.cuda(), cond_drop_prob=cdp)
    with torch.no_grad():
        y = net(x.cuda(), t.cuda(), **kw).cpu()
    hd = net.native(dev)
    names = hd.tap_names()
    got = {k: hd.tap(k, x.shape[0], dev).cpu() for k in names}
    y64, f64, dist = oracle_run(cfg, w, w64, x, t, cl, cdp)
    assert len(names) == len(set(names)) and names == U.walker_tap_names(cfg), (names, U.walker_tap_names(cfg))
    compared, over = 0, []
    worst = ("", 0.0)
    for k in names + ["out"]:
        assert k == "out" or k in f64, f"{tag}: the device records {k!r} and the oracle has no tensor under that name"
        a, r = (y, y64) if k == "out" else (got[k], f64[k])
        assert a.shape == r.shape, (tag, k, a.shape, r.shape)
        assert bool(torch.isfinite(a).all()), (tag, k, "not finite")
        e, bar = rel(a, r), bar_of(dist[k])
        compared += 1
        if e > worst[1]:
            worst = (k, e)
        if not e <= bar:
            over.append((k, e, bar, dist[k]))
    print(tag, "compared", compared, "tensors; worst", worst[0], worst[1], "out", rel(y, y64))
    assert compared == len(hd.tap_names()) + 1
    if over:
        k, e, bar, d = over[0]
        print(f"{tag}: FIRST tensor in walk order over its bar: {k}: {e:.3e} > {bar:.3e} (fp32-vs-float64 oracle {d:.3e}); {len(over)} of {compared} over")
        for k2, e2, b2, _ in over[:12]:
            print(f"    {k2}: {e2:.3e} (bar {b2:.3e})")
    assert not over, (tag, over[0], len(over))
    return y, got


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("cid", list(CASES))
def test_every_layer_vs_float64_oracle(cid):
    cfg, shape, seed = CASES[cid]
    w, w64 = weights(cid)
    net = make(cfg, w)
    x, t, cl = inputs(cfg, shape, seed)
    run_and_compare(net, cfg, w, w64, x, t, cl, 0.0, cid)
    if cid == "sc09_cls7":
        run_and_compare(net, cfg, w, w64, x, t, cl, 1.0, cid + " labels dropped")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_large_batch_takes_the_128_pixel_gather_kernel():
    """fg2_b128 (B = 128 at 32 x 32) is the one case of this module whose convs reach launch_conv2d's route g128 (conv2d_gemm_kernel<float, 128>: H*W % 128
    == 0 and B*H*W/128 * ceil(cout/128) >= 512), the route of the benchmarked 64 x 2 x 256 x 128 workload; every other case stays far below 512 tiles.  Its
    values are held to the float64 oracle by test_every_layer_vs_float64_oracle[fg2_b128]; here a child process with ADF_C2_TRACE=1 proves the route.  At the
    first level (16 x 16 pixels, 192 channels, W no multiple of 32, so the 3x3 convs take the gather kernel too): 128 * 256 / 128 = 256 pixel tiles x ny = 2
    = 512 for the stride-2 conv (Downsample), the 3x3 convs and res_conv (1x1 over the concat), x ny = 6 = 1536 for PixelShuffleUpsample's linear."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "diag", "gpu_conv2d_routes_report.py"), "u2d_fg2_b128"], capture_output=True, text=True,
                       env=dict(os.environ, ADF_C2_TRACE="1"), timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["finite"] and rep["shape"] == list(CASES["fg2_b128"][1])
    rows = conv2d_trace_lines(r.stderr)
    assert rows and all(q["B"] == 128 for q in rows)
    lv0 = [q for q in rows if (q["H"], q["W"]) == (16, 16)]
    assert len(lv0) >= 12 and all(q["route"] == "g128" and 128 * 256 // 128 * -(-q["cout"] // 128) >= 512 for q in lv0), lv0
    assert any(q["mode"] == 2 and q["cout"] == 192 for q in lv0)                           # Downsample: stride 2, two N tiles (the second partial), 512 tiles
    assert any(q["taps"] == 1 and q["cout"] == 192 and q["c0"] < q["cin"] for q in lv0)    # res_conv over the concat: 1x1, split source
    assert any(q["taps"] == 1 and q["cout"] == 768 for q in lv0)                           # PixelShuffleUpsample's linear: six N tiles
    assert any(q["taps"] == 9 and q["mode"] == 0 and q["ab"] and q["res"] for q in lv0)    # block2 with the GroupNorm prologue and the residual
    assert all(q["route"] != "g128" for q in rows if (q["H"], q["W"]) == (8, 8))           # the second level (64 pixels per image) stays on the 64-pixel kernel


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_one_handle_through_four_image_shapes():
    """odd, min, tall, odd on ONE net object: every change of shape re-plans the arena and the statistics slab; each result to its own oracle."""
    cfg = U.config_sc09(0)
    w, w64 = weights("sc09_odd")
    net = make(cfg, w)
    for i, cid in enumerate(("sc09_odd", "sc09_min", "sc09_tall", "sc09_odd")):
        x, t, cl = inputs(cfg, CASES[cid][1], 40 + i)
        run_and_compare(net, cfg, w, w64, x, t, cl, 0.0, f"shape {i} {cid}")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_denoiser_epilogue_on_a_partial_workgroup():
    """wide3 at 40 x 24 (960 pixels: the final conv's last workgroup is partial): EluDiffusion.denoise_fn (clamped) and
    VDiffusion(for_edm=True).denoise_fn (unclamped) with per-sample sigmas, against tests/precond_ref.py in float64."""
    cfg, shape, seed = CASES["wide3"]
    w, w64 = weights("wide3")
    net = make(cfg, w)
    sg = torch.tensor([0.3, 0.9, 2.0])
    g = torch.Generator().manual_seed(77)
    noise = torch.randn(shape[0], cfg.channels, *shape[1:], generator=g) * (1.0 + sg.view(3, 1, 1, 1) ** 2).sqrt()
    net32 = lambda xi, ti, **kw: U.unet2d_forward(w, cfg, xi, ti)
    net64 = lambda xi, ti, **kw: U.unet2d_forward(w64, cfg, xi, ti)
    for kind, diff, scale in (("edm", A.EluDiffusion(sigma_data=PR.SIGMA_DATA), 1.2), ("v", A.VDiffusion(for_edm=True), 1.2)):
        x = noise * scale
        with torch.no_grad():
            ref = PR.denoise(kind, net64, x.double(), sigmas=sg)
            d32 = rel(PR.denoise(kind, net32, x, sigmas=sg), ref)
            d = diff.denoise_fn(x.cuda(), net=net, inference=True, sigmas=sg.cuda()).cpu()
        share, e = float((ref.abs() >= 1).double().mean()), rel(d, ref)
        print(kind, "rel err", e, "fp32-vs-float64 restatement", d32, "share |ref| >= 1:", share, "max |ref|", float(ref.abs().max()))
        assert ref.dtype == torch.float64 and float(ref.abs().max()) > 0.05
        if kind == "edm":
            assert 0.0 < share <= 0.5, share                     # the clamp acts (1.6 % of the entries), and hides at most half
            assert float(d.abs().max()) <= 1.0
        else:
            over = ref.abs() > 1.0
            assert int(over.sum()) > 100 and float(d.abs().max()) > 1.0
            assert float((d[over].double() - ref[over]).abs().max()) <= bar_of(d32) * float(ref.abs().max())
        assert e <= bar_of(d32), (kind, e, d32)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_a_sample_alone_equals_its_row_in_the_batch():
    """fg1: sample 3 of the batch of 5, run alone with its own time and label.  The statistics are reduced with fp64 atomics whose order varies, so the claim
    is FP32_TIGHT, not bit equality; it holds for the output and for every recorded tensor."""
    cfg, shape, seed = CASES["fg1"]
    w, w64 = weights("fg1")
    net = make(cfg, w)
    x, t, cl = inputs(cfg, shape, seed)
    yb, tb = run_and_compare(net, cfg, w, w64, x, t, cl, 0.0, "fg1 batch")
    y1, t1 = run_and_compare(net, cfg, w, w64, x[3:4], t[3:4], cl[3:4], 0.0, "fg1 sample 3 alone")
    assert list(t1) == list(tb)
    errs = {k: rel(t1[k], tb[k][3:4]) for k in t1}
    errs["out"] = rel(y1, yb[3:4])
    worst = max(errs, key=errs.get)
    print("alone vs batch row: worst", worst, errs[worst], "out", errs["out"])
    assert errs[worst] <= FP32_TIGHT, (worst, errs[worst])
