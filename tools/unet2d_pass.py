"""Wall time of the shipped sc09 UNet2dBase (exact fp32) on the device: ms per forward at [B, 2, 256, 128] and ms per 50-step DPM run
(DPMSampler order 3 multistep, the sc09 eval setting; graph-replayed).  --precond picks the diffusion class and its shipped schedule around the same
network and sampler (edm: EluDiffusion(0.2) + KarrasSchedule, ve: VEDiffusion + VESchedule(100, 0.02), vp: VPDiffusion(0.1, 19.9, 1000) + VPSchedule,
v: VDiffusion(for_edm=True) + VSchedule): the network work is identical, only the row formulas and the last kernel's epilogue differ.
Usage: unet2d_pass.py [B] [repeats] [--precond {edm,ve,vp,v}]; prints one JSON line."""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audiodiffuser_amd as A

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=64)
ap.add_argument("R", nargs="?", type=int, default=5)
ap.add_argument("--precond", choices=["edm", "ve", "vp", "v"], default="edm")
args = ap.parse_args()
B, R = args.B, args.R
dev = torch.device("cuda", 0)
torch.manual_seed(0)
net = A.UNet2dBase(**vars(A.unet2d_config.config_sc09(0)), memory_efficient=True).to(dev)
with torch.no_grad():
    net.final_conv.weight.normal_(0.0, 0.02)                 # (zero-initialised in the reference: keep the output non-trivial)
x = torch.randn(B, 2, 256, 128, device=dev) * 0.5
t = torch.full((B,), 0.3, device=dev)


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


with torch.no_grad():
    fwd_ms, fwd_all = timed(lambda: net(x, t), R)
    diff, sig = {"edm": lambda: (A.EluDiffusion(sigma_data=0.2), A.KarrasSchedule(0.002, 80.0, 7.0, 50)()),
                 "ve": lambda: (A.VEDiffusion(), A.VESchedule(sigma_max=100, sigma_min=0.02, num_steps=50)()),
                 "vp": lambda: (A.VPDiffusion(beta_min=0.1, beta_d=19.9, M=1000), A.VPSchedule(beta_d=19.9, beta_min=0.1, end=0.001, num_steps=50)()),
                 "v": lambda: (A.VDiffusion(for_edm=True), A.VSchedule(num_steps=50)())}[args.precond]()
    smp = A.DPMSampler(cond_scale=1.0, order=3, num_steps=50, multisteps=True, x0_pred=True, log_time_spacing=False, use_graph=True)
    noise = torch.randn(B, 2, 256, 128, device=dev)
    run_ms, run_all = timed(lambda: smp(noise, fn=diff.denoise_fn, net=net, sigmas=sig), max(1, R // 2))
print(json.dumps({"net": "UNet2dBase sc09 (fp32)", "precond": args.precond, "batch": B, "shape": [B, 2, 256, 128], "ms_per_forward": round(fwd_ms, 2),
                  "ms_per_forward_all": [round(v, 2) for v in fwd_all], "ms_per_50step_dpm": round(run_ms, 1),
                  "ms_per_50step_dpm_all": [round(v, 1) for v in run_all]}))
