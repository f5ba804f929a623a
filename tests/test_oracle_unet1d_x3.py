"""The split-bf16 oracle of the 1-D U-Net (oracle/unet1d.py, storage="f32x3") held to itself on the CPU: that it really inserts the split, that the
free-running bar of the f32x3 GPU tests (F32X3_TOL) is sound, and that the per-launch bar the GPU tests hold the device to (SW.X3_LAUNCH_TOL) separates
summation order from every defect the mode can have.  All twelve cases of oracle/unet1d_sweep.py; the whole module runs in about 6 s.

Free-running: emulation against the float64 oracle, max-norm relative, every recorded tensor and the output: 3.4e-6 (win16 down0.conv) .. 3.9e-5 (km4
up0.attn.att) -- inside (1e-6, F32X3_TOL / 4) for everything downstream of a split product (to_in and the embeddings are the float64 oracle's, bit for bit).

Teacher-forced ladder.  The emulation's own free-running tensors, rounded to fp32 as the device stores them, are forced into (a) the emulation and (b) a
variant of it with one deliberate defect; the figure of a tensor is the relative L2 distance of (b) from (a) -- two results of the SAME forced inputs, so
nothing but the variant is in it.  Over the twelve cases, on the GEMM-fed tensors (SW.x3_gemm_fed) and the output where to_out_x3_kernel runs (h64):
  sum_fp32   the same three products, each accumulated in fp32 by torch          largest  4.2e-7 (w24 up0.attn.att); output 1.0e-7
  keep_lolo  a_lo b_lo kept                                                     5.9e-7 .. 3.1e-6: 2^-18 of the product, NOT separable at the bar (printed only)
  trunc      hi and lo chopped instead of rounded                               smallest 5.7e-6 (g16 mid.post); largest 3.3e-5; output 2.7e-5
  drop_lohi  a_lo b_hi dropped                                                  smallest 3.4e-4 (g16 mid.post)
  drop_hilo  a_hi b_lo dropped                                                  smallest 3.2e-4 (g16 mid.post)
The tensors not fed by a split product (LayerNorm outputs, an .att of the fp32 vector kernel, the output of the fp32 to_out kernel) are bit-equal under every
variant: asserted, so a split applied where the device has none shows up here.

The bar: X3_LAUNCH_TOL = 2.8e-6, half the smallest truncation figure.  The issue that asked for this test proposed 3e-6 from a prototype whose smallest
figure was 6.3e-6 (h2); with the variants placed exactly at the device's split points the smallest is 5.7e-6 (g16 mid.post: conv2 plus an identity residual,
which dilutes it most), so the bar is half of that.  test_the_launch_bar_is_half_the_smallest_truncation_figure re-derives it."""
import functools

import pytest
import torch

from oracle import unet1d as O
from oracle import unet1d_sweep as SW

F32X3_TOL = 2e-4             # tests/test_gpu_parity.py
X3_LAUNCH_TOL = SW.X3_LAUNCH_TOL
VARIANTS = ("sum_fp32", "keep_lolo", "trunc", "drop_lohi", "drop_hilo")
NOT_SPLIT = ("to_in", "temb", "class_emb")


@functools.lru_cache(maxsize=None)
def ladder(cid):
    """-> ({variant: {name: relative L2 of the variant's forced tensor from the emulation's forced tensor}}, GEMM-fed names)."""
    cfg, shape, seed, _ = SW.CASES[cid]
    w64 = SW.weights(cid)[1]
    x, t = SW.inputs(cfg, shape, seed)
    y, taps = SW.x3_case(cid)
    force = {k: v.float() for k, v in taps.items()}

    def forced(variant):
        got = {}
        with torch.no_grad():
            got["out"] = O.unet1d_forward(w64, cfg, x.double(), t.double(), taps=got, force=force,
                                          storage="f32x3" + (":" + variant if variant else ""))
        return got

    base = forced("")
    figs = {}
    for v in VARIANTS:
        got = forced(v)
        assert list(got) == list(base)
        figs[v] = {k: O.rel_l2(got[k], base[k]) for k in base}
    return figs, SW.x3_gemm_fed(cfg, taps)


@pytest.mark.parametrize("cid", list(SW.CASES))
def test_free_running_emulation_sits_between_the_rounding_and_a_quarter_of_the_f32x3_bar(cid):
    y64, t64, _ = SW.float64_case(cid)
    y, taps = SW.x3_case(cid)
    assert list(taps) == list(t64) and y.dtype == torch.float64 and all(v.dtype == torch.float64 for v in taps.values())
    d = {k: SW.rel(taps[k], t64[k]) for k in taps}
    d["out"] = SW.rel(y, y64)
    split = {k: v for k, v in d.items() if k not in NOT_SPLIT}
    lo, hi = min(split, key=split.get), max(split, key=split.get)
    print(cid, "free-running emulation vs float64: smallest", lo, f"{split[lo]:.2e}", "largest", hi, f"{split[hi]:.2e}", "out", f"{d['out']:.2e}")
    assert all(d[k] == 0.0 for k in NOT_SPLIT if k in d), {k: d[k] for k in NOT_SPLIT if k in d}        # fp32 launches on the device: no split
    assert all(1e-6 < v < F32X3_TOL / 4 for v in split.values()), (lo, split[lo], hi, split[hi])


@pytest.mark.parametrize("cid", list(SW.CASES))
def test_forced_ladder_separates_summation_order_from_every_defect(cid):
    figs, fed = ladder(cid)
    assert len(fed) >= 30 and {k for k in fed if k.endswith(".h1")} and {k for k in fed if k.endswith(".conv")} and {k for k in fed if k.endswith(".qkv")}
    assert ("out" in fed) == (cid == "h64")                                             # the one case of 64 filters: to_out_x3_kernel
    assert bool([k for k in fed if k.endswith(".att")]) == (cid in ("w24", "w48", "h2", "g3s"))        # head dim 32
    for v in VARIANTS:
        f = {k: figs[v][k] for k in fed}
        lo, hi = min(f, key=f.get), max(f, key=f.get)
        print(f"{cid} {v:9s} GEMM-fed tensors {len(f)}: smallest {lo} {f[lo]:.2e} largest {hi} {f[hi]:.2e} out {figs[v]['out']:.2e}")
        rest = {k: e for k, e in figs[v].items() if k not in fed}
        assert all(e == 0.0 for e in rest.values()), (v, {k: e for k, e in rest.items() if e})       # no split product writes these
    assert all(e < X3_LAUNCH_TOL / 2 for e in figs["sum_fp32"].values()), max(figs["sum_fp32"].items(), key=lambda kv: kv[1])
    assert all(figs["trunc"][k] > 2 * X3_LAUNCH_TOL for k in fed), min(((k, figs["trunc"][k]) for k in fed), key=lambda kv: kv[1])
    for v in ("drop_lohi", "drop_hilo"):
        assert all(figs[v][k] > 50 * X3_LAUNCH_TOL for k in fed), (v, min(((k, figs[v][k]) for k in fed), key=lambda kv: kv[1]))
    assert all(figs["keep_lolo"][k] > 0 for k in fed)


def test_the_launch_bar_is_half_the_smallest_truncation_figure():
    """Over all twelve cases; the bar may sit up to 10 % under the half (it is written with two digits), never over it."""
    smallest = min((ladder(cid)[0]["trunc"][k], cid, k) for cid in SW.CASES for k in ladder(cid)[1])
    largest_sum = max((ladder(cid)[0]["sum_fp32"][k], cid, k) for cid in SW.CASES for k in ladder(cid)[0]["sum_fp32"])
    print("smallest truncation figure", smallest, "largest fp32-summed figure", largest_sum, "bar", X3_LAUNCH_TOL)
    assert 0.9 * smallest[0] / 2 <= X3_LAUNCH_TOL <= smallest[0] / 2, smallest
    assert largest_sum[0] < X3_LAUNCH_TOL / 5, largest_sum


def test_the_attention_and_to_out_gates_restate_the_launchers():
    """launch_attention_x3 (adf_kernels.hip:842-863) and launch_to_out (:1281) at their edges."""
    assert all(O.x3_attention(32, n, 64) for n in (1, 7, 32, 255, 256, 257, 1000, 1024))
    assert not O.x3_attention(32, 1025, 64) and not O.x3_attention(64, 256, 256) and not O.x3_attention(16, 64, 128) and not O.x3_attention(8, 27, 32)
    assert O.x3_to_out(64) and O.x3_to_out(128) and not O.x3_to_out(32) and not O.x3_to_out(192) and not O.x3_to_out(48)


def test_the_split_is_the_device_definition_and_the_other_modes_are_untouched():
    """adf_common.h:90-95: hi = rn_bf16(x), lo = rn_bf16(x - hi); hi + lo leaves at most 2^-17 |x|.  The truncating variant leaves up to 2^-15 |x|, one sign."""
    q = O.Storage("f32x3")
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    hi, lo = q.split(x)
    xf = x.float()
    assert torch.equal(hi, xf.bfloat16().float()) and torch.equal(lo, (xf - hi).bfloat16().float())
    assert float(((hi.double() + lo.double() - xf.double()).abs() / xf.double().abs()).max()) <= 2.0 ** -17
    th, tl = O.Storage("f32x3:trunc").split(x)
    r = (th.double() + tl.double() - xf.double()) / xf.double()
    assert float(r.abs().max()) <= 2.0 ** -15 and float(r.max()) <= 0.0 and float(r.abs().max()) > 2.0 ** -17
    a, b = torch.randn(8, 64, dtype=torch.float64), torch.randn(16, 64, dtype=torch.float64)
    ah, al, bh, bl = (v.double() for v in (*q.split(a), *q.split(b)))
    want = al @ bh.T + ah @ bl.T + ah @ bh.T
    assert O.rel_l2(q.prod(torch.nn.functional.linear, a, b, b_is_weight=False), want) < 1e-15
    with pytest.raises(ValueError, match="split-bf16 oracle accumulates in float64"):
        cfg, shape, seed, _ = SW.CASES["h2"]
        xx, tt = SW.inputs(cfg, shape, seed)
        O.unet1d_forward(SW.weights("h2")[0], cfg, xx, tt, storage="f32x3")
    with pytest.raises(ValueError, match="storage must be"):
        O.Storage("bf16:trunc")
