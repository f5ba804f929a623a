"""Wall time of one DAC decoder pass on the device: the 44 kHz decoder ``DACDecoder(1024, 1536, [8, 8, 4, 2])`` at B = 8, T = 64 (32768 samples per
item), exact fp32.
  * ``hip``:   the library's forward (the per-unit taps are not kept at this size: every unit adds in place), captured with torch.cuda.graph;
  * ``torch``: the same forward written below with stock torch ops on the device (weights folded once, F.conv1d / F.conv_transpose1d, fp32), captured
               the same way.
The two results are compared first.  The arms alternate after two warm-up rounds; the figure of an arm is the median of its R runs.
``mfma_peak_fraction`` is the pass's GEMM FLOPs (every conv and transposed conv, 2 FLOPs per multiply-add actually needed) over its time, as a
fraction of the 157 TF f32-MFMA peak.  The per-kernel shares (profiles/README.md) come from one ``rocprofv3 --kernel-trace --stats`` run of this script.
Usage: dac_pass.py [B] [T] [repeats]; prints one JSON line."""
import argparse, json, math, os, sys
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audiodiffuser_amd as A
import dac_ref as DR

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=8)
ap.add_argument("T", nargs="?", type=int, default=64)
ap.add_argument("R", nargs="?", type=int, default=9)
args = ap.parse_args()
B, T, R = args.B, args.T, args.R
IN, CH, RATES = 1024, 1536, [8, 8, 4, 2]
PEAK_TF = 157.0
dev = torch.device("cuda", 0)
net = A.DACDecoder(IN, CH, RATES)
w = DR.generate(net.cfg, seed=7)
net.load_state_dict(w, strict=True)
net = net.to(dev)
n_params = sum(p.numel() for p in net.parameters())
# the torch arm's weights: folded once, on the device
fw = {}
for k in w:
    if k.endswith(".weight_g"):
        fw[k[:-9]] = (DR.fold(w, k[:-9], torch.float32).to(dev), w[k[:-9] + ".bias"].to(dev))
al = {k: v.to(dev) for k, v in w.items() if k.endswith(".alpha")}


def snake(x, a):
    return x + (a + 1e-9).reciprocal() * torch.sin(a * x).pow(2)


def torch_forward(z):
    x = F.conv1d(z, *fw["model.0"], padding=3)
    for i, s in enumerate(RATES):
        p = f"model.{i + 1}.block"
        x = F.conv_transpose1d(snake(x, al[f"{p}.0.alpha"]), *fw[f"{p}.1"], stride=s, padding=math.ceil(s / 2))
        for u, d in enumerate((1, 3, 9)):
            q = f"{p}.{u + 2}.block"
            y = F.conv1d(snake(x, al[f"{q}.0.alpha"]), *fw[f"{q}.1"], padding=3 * d, dilation=d)
            x = x + F.conv1d(snake(y, al[f"{q}.2.alpha"]), *fw[f"{q}.3"])
    n = len(RATES)
    return torch.tanh(F.conv1d(snake(x, al[f"model.{n + 1}.alpha"]), *fw[f"model.{n + 2}"], padding=3))


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


z = torch.randn(B, IN, T, generator=torch.Generator().manual_seed(0)).to(dev)
with torch.no_grad():
    y_hip = net(z)
    y_ref = torch_forward(z)
    torch.cuda.synchronize()
    rel = float((y_hip - y_ref).abs().max() / y_ref.abs().max())
    g_hip, o_hip = captured(lambda: net(z))
    g_torch, o_torch = captured(lambda: torch_forward(z))
    arms = {"hip": g_hip.replay, "torch": g_torch.replay}
    ms = {k: [] for k in arms}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(2):
        for fn in arms.values():
            fn()
            torch.cuda.synchronize()
    for _ in range(R):
        for k, fn in arms.items():
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[k].append(ev[0].elapsed_time(ev[1]))
    rel_replay = float((o_hip - o_torch).abs().max() / o_torch.abs().max())
med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
# GEMM FLOPs: conv = 2 L C_in C_out k; a transposed conv of kernel 2 s has two taps per output position
L, flops = T, 2.0 * T * IN * CH * 7
for i, s in enumerate(RATES):
    cin, cout = CH >> i, CH >> (i + 1)
    L = DR.up_length(L, s)
    flops += 2.0 * L * cin * cout * 2 + 3 * (2.0 * L * cout * cout * 7 + 2.0 * L * cout * cout)
flops = B * (flops + 2.0 * L * (CH >> len(RATES)) * 7)
res = {"net": f"DACDecoder({IN}, {CH}, {RATES}), fp32", "shape": [B, IN, T], "samples_per_item": L, "parameters": n_params,
       "rel_hip_vs_torch": rel, "rel_replayed": rel_replay, "ms_median": {k: round(v, 3) for k, v in med.items()},
       "ms_all": {k: [round(u, 3) for u in v] for k, v in ms.items()}, "pass_gflop": round(flops / 1e9, 1),
       "tf_whole_pass": {k: round(flops / (v * 1e-3) / 1e12, 1) for k, v in med.items()},
       "mfma_peak_fraction": {k: round(flops / (v * 1e-3) / 1e12 / PEAK_TF, 3) for k, v in med.items()},
       "hip_over_torch": round(med["hip"] / med["torch"], 3)}
print(json.dumps(res))
