"""Wall time of the program-driven loop beside the network passes: the ``small`` UNet2dBase structure (oracle/unet2d.py ``config_sc09_small`` at dim 128,
unconditional, as in the two shipped sampler_vobj inference files) at [B, 2, 256, 128], N evaluations per run of
  * VDPMSampler(order=3, multisteps=False, x0_pred=False) over VDiffusion() on LinearSchedule(1, 0, N)  (diffunet_complex_sc09_eval_vobj_dpm.yaml),
  * VUniPCSampler(order=2, x0_pred=True) on the same pair                                                  (diffunet_complex_sc09_eval_vobj_unipc.yaml),
both through adf_sampler_run_program, against N Euler steps of ReflowEulerSampler(use_heun=False) over ReFlow() on the same handle: the same N network
passes through adf_sampler_run's own driver (one raw pass and one ``x + dt v`` update per step).  All graph-replayed, in one process, the arms
alternating after two warm-up rounds (workspace, code objects, and a capture under each preconditioning state the alternation leaves the handle in);
the figure of an arm is the median of its runs.  The noise is scaled by 3e-4 for the noise-prediction arm, as in tests/vdpm_cases.py.
Usage: vdpm_pass.py [B] [N] [repeats]; prints one JSON line."""
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
cfg = dataclasses.replace(U.config_sc09_small(num_classes=0), dim=128)
w = U.generate_weights(cfg, seed=5)
for k in ("final_conv.weight", "final_conv.bias"):
    w[k] = w[k] * 0.2
net = A.UNet2dBase(**cfg.to_kwargs())
net.load_state_dict(w, strict=True)
net = net.to(dev)
g = torch.Generator().manual_seed(0)
noise = (torch.randn(B, cfg.channels, H, W, generator=g) * 0.3).to(dev)
noise_eps = noise * 1e-3                                         # 3e-4 in all

vd, ts = A.VDiffusion(), A.LinearSchedule(1.0, 0.0, N)()
dpm = A.VDPMSampler(1.0, order=3, num_steps=N, multisteps=False, x0_pred=False, use_graph=True)
upc = A.VUniPCSampler(num_steps=N, order=2, x0_pred=True, use_graph=True)
rf, flow, lin = A.ReflowEulerSampler(num_steps=N, use_heun=False, use_graph=True), A.ReFlow(), A.LinearSchedule(1.0, 0.0, N + 1)()
arms = {"vdpm_program": lambda: dpm(noise_eps, fn=vd.denoise_fn, net=net, sigmas=ts),
        "vunipc_program": lambda: upc(noise, fn=vd.denoise_fn, net=net, sigmas=ts),
        "reflow_euler": lambda: rf(noise, fn=flow.denoise_fn, net=net, sigmas=lin)}
hd = net.native(dev)
ms, evals, finite = {k: [] for k in arms}, {}, {}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
with torch.no_grad():
    for _ in range(2):                                        # warm-up
        for k, fn in arms.items():
            before = hd.counters()["sampler_evals"]
            y = fn()
            torch.cuda.synchronize()
            evals[k], finite[k] = hd.counters()["sampler_evals"] - before, bool(torch.isfinite(y).all())
    caps = hd.counters()["graph_captures"]
    for _ in range(R):
        for k, fn in arms.items():
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[k].append(ev[0].elapsed_time(ev[1]))
med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
c = hd.counters()
print(json.dumps({"net": "UNet2dBase small structure, dim 128, unconditional, fp32", "shape": [B, cfg.channels, H, W], "steps": N, "evaluations": evals,
                  "finite": finite, "ms_median": {k: round(v, 2) for k, v in med.items()},
                  "ms_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in ms.items()}, "ms_all": {k: [round(x, 2) for x in v] for k, v in ms.items()},
                  "graph_captures_during_timing": c["graph_captures"] - caps, "graph_replays": c["graph_replays"]}))
