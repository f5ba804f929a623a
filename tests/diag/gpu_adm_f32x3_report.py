"""GPU diagnostic: the ADM UNetModel in the split-bf16 mode (compute_dtype="f32x3") at the shapes where launch_conv2d (adf_conv2d.hip) changes its
kernel.  ``python gpu_adm_f32x3_report.py CASE`` prints one JSON object; run by tests/test_adm_f32x3_gpu.py as a child process with ADF_C2_TRACE=1
(and, where the case says so, ADF_CONV2D_TILE=0: both switches are read once per process), so that the ``[adf conv2d]`` lines on stderr prove the
route -- and, by the ``.x3`` suffix of the label, the instantiation -- of every conv.

The comparison is gpu_conv2d_routes_report.fp32_report: free-running, the output and EVERY tensor the device records against the fp32 oracle
(oracle/unet2d_oai.py), max |a - b| / max |b|.  Every sample has its own time.  The table is also read by the test module for its in-process cases."""
import json, os, sys
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gpu_conv2d_routes_report as R

ADD = {"use_scale_shift_norm": False}
UPDOWN = {"resblock_updown": True, "use_scale_shift_norm": False}
# name -> (changes to config_c4_small(), (B, H, W), weight seed)
CASES = {
    "small": ({}, (2, 16, 32), 61),
    "t4": ({}, (8, 32, 64), 62),
    "t5": ({}, (32, 10, 128), 63),
    "g128": ({}, (512, 16, 32), 64),
    "gather": ({}, (2, 16, 32), 65),
    "add": (ADD, (2, 16, 32), 66),
    "updown": (UPDOWN, (2, 16, 32), 67),
    "updown_gather": (UPDOWN, (2, 16, 32), 67),
    "pool": ({"conv_resample": False, "attention_resolutions": "32,16", "channel_mult": (1, 1, 2)}, (2, 32, 64), 68),
    "heads16": ({"use_new_attention_order": True, "num_head_channels": 16}, (3, 16, 32), 69),
    "w96": ({"model_channels": 96, "num_head_channels": 32}, (2, 16, 32), 70),      # (32-channel heads, as the width cases of test_conv2d_routes_gpu.py: 192 channels in 2 heads is no head dim the device serves)
}


def run_case(name, dev):
    changes, shape, seed = CASES[name]
    cfg, w, x, t, net = R.make_case("f32x3", changes, shape, seed)
    rep = R.fp32_report(cfg, w, x, t, net, dev)
    rep.update(case=name, dtype="f32x3", shape=list(shape))
    return rep


if __name__ == "__main__":
    rep = run_case(sys.argv[1], torch.device("cuda", 0))
    rep.update(route_tile=os.environ.get("ADF_CONV2D_TILE", "1"))
    print(json.dumps(rep))
