"""Time per WaveToSpec call on the device against the three reference lines it replaces, run as torch ops on the same device (torch.stft with a Hann
window, spec_fwd, cat of real and imaginary part; src/models/diffunet_complex_module.py:109-115).  Each figure is the median of three batches of
replays timed with device events, with the best and the worst batch beside it.  A batch is a captured graph of `replays` calls replayed until it
fills 0.4 s, after 2 s of the same work back to back (the chip idles at a fraction of its clock).  torch's FFT refuses stream capture ("operation not
permitted when stream is capturing"), so that arm's calls are issued one by one ("captured": false).  `wave_to_spec_eager_us` is (a) issued one by
one from Python in the same way.  The audio stays in the 256 MiB Infinity Cache between replays.
(a) is also set against its two floors: the GEMM's flops at the 157 TF/s exact-fp32 matrix peak and the tensor traffic at 8 TB/s.
Usage: wave_to_spec_pass.py [B] [L] [n_fft] [hop] [--replays N] [--no-torch]; prints one JSON line."""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audiodiffuser_amd as A

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=64)
ap.add_argument("L", nargs="?", type=int, default=16384)
ap.add_argument("n_fft", nargs="?", type=int, default=510)
ap.add_argument("hop", nargs="?", type=int, default=128)
ap.add_argument("--replays", type=int, default=200)
ap.add_argument("--no-torch", action="store_true")
args = ap.parse_args()
B, L, n_fft, hop = args.B, args.L, args.n_fft, args.hop
E, FACTOR = 0.2, 0.6
dev = torch.device("cuda", 0)
torch.manual_seed(0)
F, T = n_fft // 2 + 1, 1 + L // hop
x = torch.randn(B, L, device=dev) * 0.1


def batches(fn, replays, capture=True):
    """us per call: (median, best, worst) of three batches.  A captured graph keeps the host's share of a call (tensor allocation, argument checks,
    the ctypes call) out of the figure."""
    for _ in range(3):
        fn()                                                  # warm-up: code objects, plan, torch's FFT plan
    torch.cuda.synchronize()
    if capture:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(replays):
                fn()
        unit = graph.replay
    else:
        def unit():
            for _ in range(replays):
                fn()
    # the chip idles at a fraction of its clock and takes its time to come up: 2 s back to back before anything is timed, then windows of >= 0.4 s
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < 2.0:
        unit()
        torch.cuda.synchronize()
        n += 1
    reps = max(1, int(0.4 / ((time.perf_counter() - t0) / n)))
    us = []
    for _ in range(3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            unit()
        ev[1].record()
        torch.cuda.synchronize()
        us.append(ev[0].elapsed_time(ev[1]) * 1e3 / (replays * reps))
    us.sort()
    return {"median_us": round(us[1], 2), "best_us": round(us[0], 2), "worst_us": round(us[2], 2), "captured": capture, "calls_per_batch": replays * reps}


def reference_lines(audio, window):
    z = torch.stft(audio, window=window, normalized=True, return_complex=True, n_fft=n_fft, hop_length=hop, center=True)
    z = (z.abs() ** E * torch.exp(1j * z.angle()) * FACTOR).unsqueeze(1)
    return torch.cat((z.real, z.imag), dim=1)


m = A.WaveToSpec(n_fft=n_fft, hop_length=hop, spec_abs_exponent=E, spec_factor=FACTOR)
res = {"shape": [B, L], "out_shape": [B, 2, F, T], "n_fft": n_fft, "hop_length": hop, "replays_per_batch": args.replays}
with torch.no_grad():
    res["wave_to_spec"] = batches(lambda: m(x), args.replays)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20 * args.replays):
        m(x)                                                  # the same calls issued one by one from Python: the host's share included
    e1.record()
    torch.cuda.synchronize()
    res["wave_to_spec_eager_us"] = round(e0.elapsed_time(e1) * 1e3 / (20 * args.replays), 2)
    flops = 2.0 * (2 * F) * n_fft * B * T                       # what the transform needs as a GEMM: cosine and sine rows x window positions x frames
    traffic = 4.0 * (x.numel() + B * 2 * F * T)
    res["gemm_gflop"] = round(flops / 1e9, 3)
    res["floor_matrix_us"] = round(flops / 157e12 * 1e6, 2)
    res["floor_traffic_us"] = round(traffic / 8e12 * 1e6, 2)
    res["share_of_matrix_peak"] = round(flops / 157e12 * 1e6 / res["wave_to_spec"]["median_us"], 3)
    if not args.no_torch:
        try:
            win = torch.hann_window(n_fft, device=dev)
            y_t = reference_lines(x, win)
            res["torch_ops_same_device"] = batches(lambda: reference_lines(x, win), max(10, args.replays // 10), capture=False)
            y = m(x)
            big = (y_t[:, 0] ** 2 + y_t[:, 1] ** 2).sqrt() >= (0.05 ** E) * float((y_t[:, 0] ** 2 + y_t[:, 1] ** 2).sqrt().max())
            keep = big.unsqueeze(1).expand_as(y_t)
            res["max_rel_diff_vs_torch_fp32"] = float((y - y_t)[keep].abs().max() / y_t.abs().max())      # over the bins with |X| >= 0.05 max|X|
        except Exception as exc:                                # this torch build's stft / FFT does not run on the device: (a) alone
            res["torch_ops_same_device"] = f"did not run: {type(exc).__name__}: {str(exc)[:200]}"
print(json.dumps(res))
