"""Wall time of one DAC encoder pass and one autoencoder encode on the device, exact fp32:
  * ``encoder``: the 44 kHz encoder ``DACEncoder(64, [2, 4, 8, 8], 1024)`` at B = 8, L = 32768 (64 frames per item);
  * ``ae``:      ``FineTuneAutoencoder().encode(x, is_train=False)`` at B = 8, T = 64.
Arms, as tools/dac_pass.py:
  * ``hip``:   the library's pass (at the encoder's size the per-unit taps are not kept), captured with torch.cuda.graph;
  * ``torch``: the same pass written below with stock torch ops on the device (weights folded once, F.conv1d, fp32), captured the same way.
The two results are compared first.  The arms alternate after two warm-up rounds; the figure of an arm is the median of its R runs.
``mfma_peak_fraction`` is the pass's GEMM FLOPs (every conv, 2 FLOPs per multiply-add actually needed) over its time, as a fraction of the 157 TF
f32-MFMA peak; ``min_bytes`` is what the pass must move at least (every activation written once and read once by each conv that takes it, the
weights once) and ``hbm_fraction`` that over time, as a fraction of 8 TB/s.  The per-kernel shares (profiles/README.md) come from one
``rocprofv3 --kernel-trace --stats`` run of this script.
Usage: dac_enc_pass.py [encoder|ae] [B] [L or T] [repeats]; prints one JSON line."""
import argparse, json, math, os, sys
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audiodiffuser_amd as A
import dac_ref as DR
import dac_enc_ref as ER

ap = argparse.ArgumentParser()
ap.add_argument("what", nargs="?", default="encoder", choices=["encoder", "ae"])
ap.add_argument("B", nargs="?", type=int, default=8)
ap.add_argument("L", nargs="?", type=int, default=0)
ap.add_argument("R", nargs="?", type=int, default=9)
args = ap.parse_args()
B, R = args.B, args.R
L = args.L or (32768 if args.what == "encoder" else 64)
D, STRIDES, DL = 64, [2, 4, 8, 8], 1024
PEAK_TF, PEAK_TBS = 157.0, 8.0
dev = torch.device("cuda", 0)
net = A.DACEncoder(D, STRIDES, DL) if args.what == "encoder" else A.FineTuneAutoencoder()
w = ER.generate_enc(net.cfg, seed=7)
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


def torch_encoder(audio):
    x = F.conv1d(audio, *fw["block.0"], padding=3)
    for i, s in enumerate(STRIDES):
        p = f"block.{i + 1}.block"
        for u, d in enumerate((1, 3, 9)):
            q = f"{p}.{u}.block"
            y = F.conv1d(snake(x, al[f"{q}.0.alpha"]), *fw[f"{q}.1"], padding=3 * d, dilation=d)
            x = x + F.conv1d(snake(y, al[f"{q}.2.alpha"]), *fw[f"{q}.3"])
        x = F.conv1d(snake(x, al[f"{p}.3.alpha"]), *fw[f"{p}.4"], stride=s, padding=math.ceil(s / 2))
    n = len(STRIDES)
    return F.conv1d(snake(x, al[f"block.{n + 1}.alpha"]), *fw[f"block.{n + 2}"], padding=1)


if args.what == "ae":
    bw, bb = w["btnk_layer.weight"].to(dev), w["btnk_layer.bias"].to(dev)


def torch_encode(x):
    for i in range(len(net.cfg.widths) - 1):
        x = F.conv1d(snake(x, al[f"encoder_layers.{2 * i}.alpha"]), *fw[f"encoder_layers.{2 * i + 1}"], padding=1)
    mean, logvar = F.conv1d(x, bw, bb).chunk(2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    return mean, 0.5 * torch.mean(torch.sum(mean ** 2 + logvar.exp() - logvar - 1, dim=[1, 2]), dim=0)


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


first = (lambda o: o[0]) if args.what == "ae" else (lambda o: o)
if args.what == "encoder":
    x = 0.5 * torch.randn(B, 1, L, generator=torch.Generator().manual_seed(0)).to(dev)
    hip_fn, torch_fn = (lambda: net(x)), (lambda: torch_encoder(x))
else:
    x = torch.randn(B, 1024, L, generator=torch.Generator().manual_seed(0)).to(dev)
    hip_fn, torch_fn = (lambda: net.encode(x, is_train=False)), (lambda: torch_encode(x))
with torch.no_grad():
    y_hip, y_ref = hip_fn(), torch_fn()
    torch.cuda.synchronize()
    rel = float((first(y_hip) - first(y_ref)).abs().max() / first(y_ref).abs().max())
    rel_kl = abs(float(y_hip[1]) - float(y_ref[1])) / abs(float(y_ref[1])) if args.what == "ae" else None
    g_hip, o_hip = captured(hip_fn)
    g_torch, o_torch = captured(torch_fn)
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
    rel_replay = float((first(o_hip) - first(o_torch)).abs().max() / first(o_torch).abs().max())
med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
# GEMM FLOPs (conv = 2 L_out C_in C_out k) and the least bytes: each conv reads its input and writes its output once (a unit's 1x1 also reads the residual)
if args.what == "encoder":
    Li, flops, floats = L, 2.0 * L * D * 7, L * (1 + D)
    for i, s in enumerate(STRIDES):
        c = D << i
        flops += 3 * (2.0 * Li * c * c * 7 + 2.0 * Li * c * c)
        floats += 3 * (2 * Li * c + 3 * Li * c)
        Lo = ER.down_length(Li, s)
        flops += 2.0 * Lo * c * 2 * c * 2 * s
        floats += Li * c + Lo * 2 * c
        Li = Lo
    flops += 2.0 * Li * (D << len(STRIDES)) * DL * 3
    floats += Li * ((D << len(STRIDES)) + 2 * DL)
    out_len = Li
else:
    wd = net.cfg.widths
    flops = sum(2.0 * L * a * b * 3 for a, b in zip(wd[:-1], wd[1:])) + 2.0 * L * wd[-1] * 2 * net.cfg.input_channel
    floats = 2 * L * wd[0] + sum(L * (a + b) for a, b in zip(wd[:-1], wd[1:])) + L * (wd[-1] + 3 * net.cfg.input_channel)
    out_len = L
flops, min_bytes = B * flops, 4.0 * (B * floats + n_params)
res = {"net": f"DACEncoder({D}, {STRIDES}, {DL}), fp32" if args.what == "encoder" else "FineTuneAutoencoder().encode, fp32",
       "shape": list(x.shape), "frames_per_item": out_len, "parameters": n_params,
       "rel_hip_vs_torch": rel, "rel_kl_hip_vs_torch": rel_kl, "rel_replayed": rel_replay, "ms_median": {k: round(v, 3) for k, v in med.items()},
       "ms_all": {k: [round(u, 3) for u in v] for k, v in ms.items()}, "pass_gflop": round(flops / 1e9, 1), "min_mbytes": round(min_bytes / 1e6, 1),
       "tf_whole_pass": {k: round(flops / (v * 1e-3) / 1e12, 1) for k, v in med.items()},
       "mfma_peak_fraction": {k: round(flops / (v * 1e-3) / 1e12 / PEAK_TF, 3) for k, v in med.items()},
       "hbm_fraction": {k: round(min_bytes / (v * 1e-3) / 1e12 / PEAK_TBS, 3) for k, v in med.items()},
       "hip_over_torch": round(med["hip"] / med["torch"], 3)}
print(json.dumps(res))
