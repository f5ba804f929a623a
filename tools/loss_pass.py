"""Time per ``diffusion(x, net, sigmas)`` -- the validation loss of one batch under torch.no_grad() -- on the device route (one ``adf_diffusion_loss``
call) against ``_tensor_loss`` (the tensor ops around ``denoise_fn``) on the SAME net, and the two new memory-bound kernels alone against their
byte floor.

Call time: the two arms alternate in one process (device, tensor, device, tensor, ...), each turn a batch of ``--calls`` calls issued one by one
from Python and timed with device events, after ``--warm`` seconds of the same alternation (the chip idles at a fraction of its clock).  Each figure
is the median of three batches with the best and the worst beside it; ``saved_us`` is the difference of the medians, and ``network_pass_us`` -- one
``denoise_fn`` evaluation on the noisy input, timed the same way -- is what both arms spend in the network.  Nothing is captured: the tensor arm's
``denoise_fn(inference=False)`` is a plain ``net(...)`` call and its host share is part of what the device route removes.

Kernel time: ``adf_bench_loss_kernels`` on ``--kernel-rows`` rows of the shape's N elements in buffers of their own, sized past the 256 MiB Infinity
Cache by default (three or four tensors of rows x N x 4 bytes), so the share is of the HBM byte floor at 8 TB/s; at the loss's own batch the tensors
stay in that cache.

Shapes: ``sc09`` = UNet2dBase of the shipped sc09 files at 64 x 2 x 256 x 128 in fp32 (class-conditional: labels, the net's cond_drop_prob 0);
``c2`` = the 1-D config c2 at 64 x 16384 in bf16.  Usage: loss_pass.py [sc09|c2|tiny] [--batch B] [--calls N] [--warm S]; prints one JSON line."""
import argparse, ctypes as C, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audiodiffuser_amd as A
from audiodiffuser_amd.unet2d_config import config_sc09

ap = argparse.ArgumentParser()
ap.add_argument("shape", nargs="?", default="sc09", choices=["sc09", "c2", "tiny"])
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--calls", type=int, default=0, help="calls per batch (default: 3 for sc09, 40 otherwise)")
ap.add_argument("--warm", type=float, default=2.0)
ap.add_argument("--kernel-rows", type=int, default=0, help="rows of the kernel-only measurement (default: enough for 128 MiB per tensor)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.manual_seed(0)
B = args.batch
kw = {}
if args.shape == "sc09":
    net, dtype, shape = A.UNet2dBase(**vars(config_sc09()), memory_efficient=True), "fp32", (B, 2, 256, 128)
    kw = {"classes": (torch.arange(B) % 10).to(dev)}
elif args.shape == "c2":
    net, dtype, shape = A.UNet1dBase.from_config(A.config_c2(), compute_dtype="bf16"), "bf16", (B, 1, 16384)
else:
    net, dtype, shape = A.UNet1dBase.from_config(A.config_tiny()), "fp32", (B, 1, 256)
net = net.to(dev)
net.cond_drop_prob = 0.0
calls = args.calls or (3 if args.shape == "sc09" else 40)
diff = A.EluDiffusion(sigma_data=0.2)
x = (0.3 * torch.randn(*shape, device=dev)).clamp(-1, 1)
sig = A.LogNormalDistribution(mean=-3.0, std=1.0)(num_samples=B, device=dev)
hd = net.native(dev)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def summary(us):
    us = sorted(us)
    return {"median_us": round(us[1], 1), "best_us": round(us[0], 1), "worst_us": round(us[2], 1)}


with torch.no_grad():
    x_noisy = x + sig.view(-1, *([1] * (x.ndim - 1))) * torch.randn_like(x)
    arms = {"device_route": lambda: diff(x, net, sig, **kw), "tensor_route": lambda: diff._tensor_loss(x, net, sig, **kw),
            "network_pass": lambda: diff.denoise_fn(x_noisy, net, inference=True, sigmas=sig, **kw)}
    before = hd.loss_calls()
    a, b = arms["device_route"](), arms["tensor_route"]()
    assert hd.loss_calls() == before + 1, "the device route did not run"
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.warm:
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
    us = {name: [] for name in arms}
    for _ in range(3):
        for name, fn in arms.items():                        # the arms alternate: a drift of the clock reaches both alike
            us[name].append(timed(fn, calls))
    res = {"shape": list(shape), "net": args.shape, "compute_dtype": dtype, "calls_per_batch": calls,
           "call_time": {name: summary(v) for name, v in us.items()}}
    res["saved_us"] = round(res["call_time"]["tensor_route"]["median_us"] - res["call_time"]["device_route"]["median_us"], 1)
    # the two routes draw different noise here (no reseeding between them): only the scale of the losses is comparable
    res["mean_loss"] = {"device_route": float(a.float().mean()), "tensor_route": float(b.float().mean())}

    # ---- the two kernels alone ---------------------------------------------------------------------------------------------------------
    N = int(x[0].numel())
    rows = args.kernel_rows or min(65535, max(B, (128 << 20) // (4 * N)))       # (a launch takes at most 65535 rows)
    res["kernels"] = {"rows": rows, "N": N, "floor_TBps": 8.0}
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for tag, rf in (("x0", 0), ("rf", 1)):
        ms_mix, ms_part, by_mix, by_part = C.c_float(), C.c_float(), C.c_double(), C.c_double()
        per = []
        for _ in range(3):
            hd.check(hd.lib.adf_bench_loss_kernels(hd.h, rf, rows, N, 20, C.byref(ms_mix), C.byref(ms_part), C.byref(by_mix), C.byref(by_part), stream),
                     "adf_bench_loss_kernels")
            per.append((ms_mix.value * 1e3, ms_part.value * 1e3))
        mix_us, part_us = sorted(p[0] for p in per)[1], sorted(p[1] for p in per)[1]
        res["kernels"][tag] = {"mix_kernel_us": round(mix_us, 2), "mix_share_of_byte_floor": round(by_mix.value / 8e12 * 1e6 / mix_us, 3),
                               "partial_kernel_us": round(part_us, 2), "partial_share_of_byte_floor": round(by_part.value / 8e12 * 1e6 / part_us, 3),
                               "mix_MB": round(by_mix.value / 1e6, 1), "partial_MB": round(by_part.value / 1e6, 1)}
print(json.dumps(res))
