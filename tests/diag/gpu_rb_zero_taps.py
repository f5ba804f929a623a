"""One bf16 forward of a small UNet1d whose down / up conv is a raw launch of the resblock conv kernel (adf_gemm_rb.h), for tests/test_rb_zero_taps_gpu.py:
`gpu_rb_zero_taps.py OUT MULTIPLIERS FACTORS B L TAP[,TAP...]` (lists comma-separated, L = input samples) stores, per tap, the stored tensor, its fused
GroupNorm statistics where the launch reduced them, and the relative L2 distance to the bf16-storage oracle of that ONE layer computed from the device's own
input of it.  Run it in separate processes with ADF_RB_ZSKIP=0 / 1 (the switch is read once per process), ADF_GEMM_RB and ADF_GEMM_TRACE=1."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch


def config_of(multipliers, factors):
    from audiodiffuser_amd.config import UNet1dConfig
    n = len(factors)
    return UNet1dConfig(channels=64, num_filters=64 * multipliers[0], multipliers=list(multipliers), factors=list(factors), num_blocks=[1] * n,
                        attentions=[False] * n, use_attention_bottleneck=False)


def main(path, multipliers, factors, B, L, taps):
    from audiodiffuser_amd.weights import generate_noise
    from gpu_helpers import make_net, rel_l2
    from oracle import unet1d as O
    cfg = config_of(multipliers, factors)
    n = len(factors)
    x = generate_noise(0, B, L) * 0.7
    t = torch.linspace(-1.0, 0.5, B)
    net, w = make_net(cfg, "bf16")
    y = net(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    hd = net.native(torch.device("cuda", 0))
    q = O.Storage("bf16")
    out = {"out_finite": bool(torch.isfinite(y).all())}
    for name in taps:
        got = hd.tap(name, B, y.device).float().cpu()
        kind, idx = name.split(".")[0][:-1], int(name.split(".")[0][-1])
        with torch.no_grad():
            if kind == "down":
                src = hd.tap("to_in" if idx == 0 else f"down{idx - 1}.block0", B, y.device).float().cpu()
                want = O.downsample_conv(w, f"unet.downsamples.{idx}.downsample", src, factors[idx], cfg.kernel_multiplier_downsample, q)
            else:
                src = hd.tap(f"up{idx}.block0", B, y.device).float().cpu()
                want = O.upsample_conv(w, f"unet.upsamples.{idx}.upsample", src, factors[n - 1 - idx], q)
        out[name] = got
        out[name + "/oracle_rel_l2"] = rel_l2(got, want)
        # (the last up conv is stored without statistics: nothing normalises its output)
        out[name + "/stats"] = hd.tap_stats(name, B, y.device) if kind == "down" or idx + 1 < n else None
    torch.save(out, path)
    print("saved", sorted(out), flush=True)


if __name__ == "__main__":
    ints = lambda s: [int(v) for v in s.split(",")]
    main(sys.argv[1], ints(sys.argv[2]), ints(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6].split(","))
