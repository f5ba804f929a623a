"""Wall time of the table-driven loop beside the network passes: the ``small`` UNet2dBase structure (oracle/unet2d.py ``config_sc09_small`` at dim 128,
class-conditional) at [B, 2, 256, 128], N steps of VSampler over VDiffusion() -- N evaluations, per step one clamped-epilogue pass and one fused update
that reads the state, the estimate and a draw -- against N Euler steps of ReflowEulerSampler(use_heun=False) over ReFlow() on the same handle: the same N
network passes through adf_sampler_run's own driver (one raw pass and one ``x + dt v`` update per step).  Both graph-replayed, in one process, the two
arms alternating after a warm-up run of each (workspace, code objects, graph capture); the figure of an arm is the median of its runs.
Usage: vsamp_pass.py [B] [steps] [repeats]; prints one JSON line."""
import argparse, dataclasses, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audiodiffuser_amd as A
from oracle import unet2d as U

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=8)
ap.add_argument("N", nargs="?", type=int, default=20)
ap.add_argument("R", nargs="?", type=int, default=9)
args = ap.parse_args()
B, N, R, H, W = args.B, args.N, args.R, 256, 128
dev = torch.device("cuda", 0)
cfg = dataclasses.replace(U.config_sc09_small(), dim=128)
w = U.generate_weights(cfg, seed=5)
for k in ("final_conv.weight", "final_conv.bias"):
    w[k] = w[k] * 0.2
net = A.UNet2dBase(**cfg.to_kwargs())
net.load_state_dict(w, strict=True)
net = net.to(dev)
g = torch.Generator().manual_seed(0)
noise = (torch.randn(B, cfg.channels, H, W, generator=g) * 0.3).to(dev)
draws = (torch.randn(N, B, cfg.channels, H, W, generator=g) * 0.3).to(dev)
classes = torch.arange(B, device=dev) % cfg.num_classes

vs, vd, ts = A.VSampler(num_steps=N, use_graph=True), A.VDiffusion(), torch.linspace(0.9, 0.1, N)
rf, flow, lin = A.ReflowEulerSampler(num_steps=N, use_heun=False, use_graph=True), A.ReFlow(), A.LinearSchedule(1.0, 0.0, N + 1)()
arms = {"vsampler_table": lambda: vs(noise, fn=vd.denoise_fn, net=net, sigmas=ts, injected_noise=draws, classes=classes),
        "reflow_euler": lambda: rf(noise, fn=flow.denoise_fn, net=net, sigmas=lin, classes=classes)}
ms = {k: [] for k in arms}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
with torch.no_grad():
    for fn in arms.values():                                  # warm-up
        y = fn()
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(y).all())
    for _ in range(R):
        for k, fn in arms.items():
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[k].append(ev[0].elapsed_time(ev[1]))
med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
c = net.native(dev).counters()
print(json.dumps({"net": "UNet2dBase small structure, dim 128, class-conditional, fp32", "shape": [B, cfg.channels, H, W], "steps": N, "evaluations": N,
                  "finite": finite, "ms_median": {k: round(v, 2) for k, v in med.items()},
                  "ms_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in ms.items()}, "ms_all": {k: [round(x, 2) for x in v] for k, v in ms.items()},
                  "graph_captures": c["graph_captures"], "graph_replays": c["graph_replays"]}))
