"""Wall time of a rectified-flow run on the device: the c1 UNet1dBase, class-conditional (10 labels) with guidance 2.0 -- the net and guidance of
configs/experiment/sc09/reflowunet_sc09_cfg.yaml -- in bf16 at [B, 1, 16384], 50 Heun steps of ReflowEulerSampler over ReFlow() on
LinearSchedule(1, 0, 51), graph-replayed (99 evaluations, two network passes each).  On the same handle, for comparison, EDMSampler(s_churn=0) Heun over
EluDiffusion(0.2) on KarrasSchedule(0.002, 80, 7, 50): the same 99 evaluations, so the network work is identical and only the row formulas, the
combine pass and the update kernels differ.
Usage: rf_pass.py [B] [repeats]; prints one JSON line."""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audiodiffuser_amd as A
from audiodiffuser_amd.weights import generate_noise, generate_weights

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=64)
ap.add_argument("R", nargs="?", type=int, default=5)
args = ap.parse_args()
B, R, L, N = args.B, args.R, 16384, 50
dev = torch.device("cuda", 0)
cfg = A.config_c1()
cfg.class_cond, cfg.num_classes = True, 10
net = A.UNet1dBase.from_config(cfg, compute_dtype="bf16")
net.load_state_dict(generate_weights(cfg, seed=0), strict=True)      # (the output layer is zero-initialised in the reference: keep the output non-trivial)
net = net.to(dev)
noise = generate_noise(0, B, L).to(dev)
classes = (torch.arange(B, device=dev) % 10)


def timed(fn, reps):
    fn()                                                      # warm-up (workspace, code objects, graph capture)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return sorted(ms)[len(ms) // 2], ms


rf, flow, lin = A.ReflowEulerSampler(num_steps=N, cond_scale=2.0, use_heun=True, use_graph=True), A.ReFlow(), A.LinearSchedule(1.0, 0.0, N + 1)()
edm, elu, karras = A.EDMSampler(s_churn=0, num_steps=N, cond_scale=2.0, use_heun=True, use_graph=True), A.EluDiffusion(sigma_data=0.2), A.KarrasSchedule(0.002, 80.0, 7.0, N)()
with torch.no_grad():
    rf_ms, rf_all = timed(lambda: rf(noise, fn=flow.denoise_fn, net=net, sigmas=lin, classes=classes), R)
    edm_ms, edm_all = timed(lambda: edm(noise, fn=elu.denoise_fn, net=net, sigmas=karras, classes=classes), R)
    y = rf(noise, fn=flow.denoise_fn, net=net, sigmas=lin, classes=classes)
c = net.native(dev).counters()
print(json.dumps({"net": "UNet1dBase c1, class-conditional, bf16", "shape": [B, 1, L], "cond_scale": 2.0, "steps": N, "evaluations": 2 * N - 1,
                  "finite": bool(torch.isfinite(y).all()), "ms_reflow_heun": round(rf_ms, 1), "ms_reflow_heun_all": [round(v, 1) for v in rf_all],
                  "ms_edm_heun": round(edm_ms, 1), "ms_edm_heun_all": [round(v, 1) for v in edm_all], "ratio": round(rf_ms / edm_ms, 4),
                  "graph_captures": c["graph_captures"], "graph_replays": c["graph_replays"]}))
