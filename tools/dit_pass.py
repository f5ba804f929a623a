"""Wall time of one DiT forward on the device: DiT-B widths (hidden 768, 12 heads, depth 12, mlp_ratio 4) at [16, 2, 256, 128] with patch [8, 4]
(1024 tokens per sample, 16384 token rows), unconditional, exact fp32.
  * ``hip``:   the library's pass, graph-replayed as a one-step ReflowEulerSampler(use_heun=False) over ReFlow() -- one raw network pass (the
               modulation rows computed at the head of the run) and one ``x + dt v`` update;
  * ``torch``: the same forward written below with stock torch ops on the device (fp32 matmul / softmax / layer_norm), captured with torch.cuda.graph.
The arms alternate after two warm-up rounds; the figure of an arm is the median of its R runs.  The two results are compared first (the block taps are
not kept at this size, so this is also the check of the in-place residual path).  ``tf_whole_pass`` counts the GEMM and attention FLOPs of the pass; the
per-kernel shares (profiles/README.md) come from one ``rocprofv3 --kernel-trace --stats`` run of this script.
With the optional fourth argument ``f32x3`` a third arm, ``hip_f32x3`` -- the same net with ``compute_dtype="f32x3"`` (split-bf16 linears and
attention), driven like ``hip`` -- alternates with the other two in the same process, and the line gains ``rel_f32x3_vs_torch``,
``f32x3_over_torch`` and ``f32x3_over_fp32``; without it the run and its keys are as before.
Usage: dit_pass.py [B] [repeats] [depth] [f32x3]; prints one JSON line."""
import argparse, json, math, os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audiodiffuser_amd as A
from audiodiffuser_amd.dit import generate_weights

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=16)
ap.add_argument("R", nargs="?", type=int, default=9)
ap.add_argument("depth", nargs="?", type=int, default=12)
ap.add_argument("compute_dtype", nargs="?", choices=["fp32", "f32x3"], default="fp32")
args = ap.parse_args()
B, R, H, W, C = args.B, args.R, 256, 128, 2
kw = dict(input_size=[H, W], patch_size=[8, 4], in_channels=C, hidden_size=768, depth=args.depth, num_heads=12, mlp_ratio=4.0)
dev = torch.device("cuda", 0)
net = A.DiT(**kw)
w = generate_weights(net.cfg, seed=7)
net.load_state_dict(w, strict=True)
net = net.to(dev)
net3 = None
if args.compute_dtype == "f32x3":
    net3 = A.DiT(compute_dtype="f32x3", **kw)
    net3.load_state_dict(w, strict=True)
    net3 = net3.to(dev)
wd = {k: v.to(dev) for k, v in w.items()}
D, heads, (p1, p2) = 768, 12, (8, 4)
gh, gw = H // p1, W // p2
T = gh * gw


def torch_forward(x, t):
    xp = x.reshape(B, C, gh, p1, gw, p2).permute(0, 2, 4, 1, 3, 5).reshape(B, T, C * p1 * p2)
    h = F.linear(xp, wd["x_embedder.proj.weight"].reshape(D, -1), wd["x_embedder.proj.bias"]) + wd["pos_embed"]
    half = D // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=dev) / half)
    args_ = t[:, None] * freqs[None]
    emb = torch.cat([torch.cos(args_), torch.sin(args_)], dim=-1)
    c = F.linear(F.silu(F.linear(emb, wd["t_embedder.mlp.0.weight"], wd["t_embedder.mlp.0.bias"])), wd["t_embedder.mlp.2.weight"], wd["t_embedder.mlp.2.bias"])
    sc_ = F.silu(c)
    for i in range(args.depth):
        p = f"blocks.{i}"
        sh1, s1, g1, sh2, s2, g2 = F.linear(sc_, wd[f"{p}.adaLN_modulation.1.weight"], wd[f"{p}.adaLN_modulation.1.bias"]).chunk(6, dim=1)
        xn = F.layer_norm(h, (D,), eps=1e-6) * (1 + s1.unsqueeze(1)) + sh1.unsqueeze(1)
        q = F.linear(xn, wd[f"{p}.attn.to_q.weight"])
        k, v = F.linear(xn, wd[f"{p}.attn.to_kv.weight"]).chunk(2, dim=-1)
        q, k, v = (u.reshape(B, T, heads, D // heads).transpose(1, 2) for u in (q, k, v))
        a = torch.softmax(q @ k.transpose(-1, -2) * (D // heads) ** -0.5, dim=-1) @ v
        h = h + g1.unsqueeze(1) * F.linear(a.transpose(1, 2).reshape(B, T, D), wd[f"{p}.attn.to_out.weight"])
        xn = F.layer_norm(h, (D,), eps=1e-6) * (1 + s2.unsqueeze(1)) + sh2.unsqueeze(1)
        f = F.linear(F.gelu(F.linear(xn, wd[f"{p}.mlp.fc1.weight"], wd[f"{p}.mlp.fc1.bias"]), approximate="tanh"), wd[f"{p}.mlp.fc2.weight"], wd[f"{p}.mlp.fc2.bias"])
        h = h + g2.unsqueeze(1) * f
    sh, s = F.linear(sc_, wd["final_layer.adaLN_modulation.1.weight"], wd["final_layer.adaLN_modulation.1.bias"]).chunk(2, dim=1)
    y = F.linear(F.layer_norm(h, (D,), eps=1e-6) * (1 + s.unsqueeze(1)) + sh.unsqueeze(1), wd["final_layer.linear.weight"], wd["final_layer.linear.bias"])
    return y.reshape(B, gh, gw, p1, p2, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)


g = torch.Generator().manual_seed(0)
x = torch.randn(B, C, H, W, generator=g).to(dev)
tt = torch.full((B,), 1.0, device=dev)
with torch.no_grad():
    y_hip = net(x, tt)
    y_ref = torch_forward(x, tt)
    torch.cuda.synchronize()
    rel = float((y_hip - y_ref).abs().max() / y_ref.abs().max())
    rel3 = float((net3(x, tt) - y_ref).abs().max() / y_ref.abs().max()) if net3 is not None else None
    # the graph-replayed arms: x_next = x + (0 - 1) v at t = 1 for the library, the bare forward for torch
    rf, flow, lin = A.ReflowEulerSampler(num_steps=1, use_heun=False, use_graph=True), A.ReFlow(), A.LinearSchedule(1.0, 0.0, 2)()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch_forward(x, tt)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g = torch_forward(x, tt)
    arms = {"hip": lambda: rf(x, fn=flow.denoise_fn, net=net, sigmas=lin), "torch": lambda: graph.replay()}
    if net3 is not None:
        arms["hip_f32x3"] = lambda: rf(x, fn=flow.denoise_fn, net=net3, sigmas=lin)
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
med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
M, hid = B * T, 4 * D
flops = args.depth * (2.0 * M * D * 3 * D + 2.0 * M * D * D + 4.0 * M * D * hid + 4.0 * B * heads * T * T * (D // heads))
res = {"net": f"DiT-B widths (768 / 12 heads / depth {args.depth} / ratio 4), unconditional, fp32", "shape": [B, C, H, W], "tokens": T,
       "rel_hip_vs_torch": rel, "ms_median": {k: round(v, 3) for k, v in med.items()},
       "ms_all": {k: [round(u, 3) for u in v] for k, v in ms.items()}, "pass_gflop": round(flops / 1e9, 1),
       "tf_whole_pass": {k: round(flops / (v * 1e-3) / 1e12, 1) for k, v in med.items()},
       "hip_over_torch": round(med["hip"] / med["torch"], 3)}
if net3 is not None:
    res.update({"rel_f32x3_vs_torch": rel3, "f32x3_over_torch": round(med["hip_f32x3"] / med["torch"], 3),
                "f32x3_over_fp32": round(med["hip_f32x3"] / med["hip"], 3)})
print(json.dumps(res))
