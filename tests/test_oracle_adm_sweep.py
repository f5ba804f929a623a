"""The float64 run of the ADM oracle (oracle/unet2d_oai.py on float64 weights, inputs and times) over the sweep of oracle/adm_sweep.py: what
tests/test_adm_sweep_gpu.py holds the device to.  No GPU.

Per run (the ten cases, io43 with its labels dropped, lv3 at its second shape): the fp32 oracle -- pinned to the reference's own fixtures by
tests/test_oracle_next.py -- lies within a quarter of FP32_TIGHT (5e-5, the project's exact-fp32 bar) of the float64 run on the output and on every
recorded tensor (the rule of tests/test_unet2d_sweep_gpu.py), so the device bar never needs its second clause; every tensor of the float64 run is float64
(asserted in ``float64_run``); the float64 output is finite with max |y| > 1e-3; at least 20 tensors are recorded.

Measured on 8 CPU threads, worst fp32-vs-float64 tensor per run (bar 1.25e-5) and the output:
  lv3        output_blocks.0.1.att 2.2e-6 (out 7.2e-7; 114 tensors)      lv3_16x64     output_blocks.5.1.att 2.1e-6 (out 1.1e-6; 114)
  updown_ss  output_blocks.0.1.att 1.2e-6 (out 1.1e-6; 52)               pool_hd8      output_blocks.5.1.att 2.0e-6 (out 1.3e-6; 88)
  one_level  middle_block.1.att 8.2e-7 (out 9.7e-7; 23)                  io43          output_blocks.0.1.att 1.1e-6 (out 7.9e-7; 50)
  flat       output_blocks.1.1.att 1.9e-6 (out 1.0e-6; 50)               io43_dropped  output_blocks.0.1.xn 9.2e-7 (out 7.5e-7; 50)
  tall       middle_block.1.att 2.7e-6 (out 1.2e-6; 50)                  mult21        output_blocks.1.1.att 3.5e-6 (out 6.7e-7; 94)
  odd_h      middle_block.1.att 9.4e-7 (out 7.5e-7; 23)                  one_row       output_blocks.1.0.skip 6.3e-7 (out 6.5e-7; 23)
The whole module takes about 5 s.  The edit that made the oracle follow its input's dtype left its fp32 results bit-equal (``torch.equal``, output and
every tensor) on all twelve runs.
"""
import pytest
import torch

from oracle import adm_sweep as S
from oracle import unet2d_oai as O


@pytest.mark.parametrize("rid", list(S.RUNS))
def test_fp32_oracle_within_a_quarter_of_the_bar_of_the_float64_run(rid):
    cid, shape, seed, cdp = S.RUNS[rid]
    cfg = S.config(cid)
    y64, t64, dist = S.float64_case(rid)
    b, h, w = shape
    assert y64.shape == (b, cfg.out_channels, h, w) and t64["input_blocks.0"].shape == (b, cfg.model_channels * cfg.channel_mult[0], h, w)
    worst = max((k for k in dist if k != "out"), key=dist.get)
    print(rid, "tensors", len(t64), "worst fp32-vs-float64", worst, dist[worst], "out", dist["out"])
    over = [(k, d) for k, d in dist.items() if not d <= S.FP32_TIGHT / 4]
    assert not over, over[:5]
    assert bool(torch.isfinite(y64).all()) and float(y64.abs().max()) > 1e-3
    assert len(t64) >= 20, len(t64)
    assert all(bool(torch.isfinite(v).all()) for v in t64.values())


def test_the_cases_reach_what_they_name():
    """The structure each case is in the table for, read off ``structure`` and the configuration (a later edit of the table cannot silently lose one)."""
    st = {cid: O.structure(S.config(cid)) for cid in S.CASES}
    layers = lambda s: [l for blk in s.input_blocks + [s.middle] + s.output_blocks for l in blk]
    heads = lambda cid: {(l.cin // S.config(cid).heads(l.cin), S.config(cid).heads(l.cin)) for l in layers(st[cid]) if l.kind == "attn"}   # (head dim, heads)
    assert {l.cout for l in layers(st["lv3"])} == {32, 64, 96} and (32, 3) in heads("lv3") and len(S.float64_case("lv3")[1]) == 114
    assert any(l.up for l in layers(st["updown_ss"])) and any(l.down for l in layers(st["updown_ss"])) and S.config("updown_ss").use_scale_shift_norm
    assert heads("updown_ss") == {(64, 2)}
    pool = st["pool_hd8"]
    assert not S.config("pool_hd8").conv_resample and (8, 4) in heads("pool_hd8") and pool.input_blocks[1][-1].kind == "attn"      # attention at level 0
    assert [l.kind for l in pool.output_blocks[1]][-2:] == ["attn", "up"]                          # pooled resampling right after an attention block
    assert not any(l.kind in ("up", "down") or l.up or l.down for cid in ("one_level", "odd_h", "one_row") for l in layers(st[cid]))
    io = S.config("io43")
    assert (io.in_channels, io.out_channels, io.num_classes, io.use_scale_shift_norm, io.model_channels) == (4, 3, 7, False, 96)
    assert len(set(S.inputs(io, S.CASES["io43"][1])[2].tolist())) == 7                             # every sample its own label
    assert [l.cout for l in layers(st["mult21"]) if l.kind == "res"][:6] == [64, 64, 64, 32, 32, 32] and S.config("mult21").use_new_attention_order
    assert S.CASES["flat"][1][1:] == (4, 64) and S.CASES["tall"][1][1:] == (64, 4) and S.CASES["odd_h"][1][1] == 3 and S.CASES["one_row"][1][1] == 1
    assert sorted(S.CASES[c][1][0] for c in ("pool_hd8", "lv3", "one_level", "io43")) == [1, 3, 5, 7]
    for cid in S.BF16_CASES:
        assert all(l.cin % 64 == 0 and l.cout % 64 == 0 for l in layers(st[cid]) if l.kind != "conv"), cid
    for cid, shape in [(c, S.CASES[c][1]) for c in S.CASES] + [(r[0], r[1]) for r in S.RUNS.values()] + list(S.FOUR_SHAPES):
        f = 2 ** (len(S.config(cid).channel_mult) - 1)
        assert shape[1] % f == 0 and shape[2] % f == 0 and (shape[1] // f) * (shape[2] // f) % 64 == 0, (cid, shape)   # AdmNet::check_image
