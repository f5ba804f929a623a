"""Timeline of one launch of the transposed-conv kernel (diagnostic build with -DADF_UP_TL=<L>): where the cycles of its work items go.

usage (GPU box): tools/build_variant.sh uptl -DADF_UP_TL=256        (in the build container; the .so travels)
                 ADF_HIP_LIB=audiodiffuser_amd/build/variants/libadf_hip_uptl.so python tools/up_timeline.py [batch] [length]
One forward pass of the configs[1] net in bf16 (twice: the second pass is the one read); the launch whose lin equals ADF_UP_TL stamps
s_memtime per wave of workgroup 0 and of one from the middle of the grid at the phase boundaries of every work item: start / tile staged
(skipped for a further pass of the staged tile) / weight ring requested / K loop done / epilogue in LDS + barrier / stores issued / closing
barrier; s_memrealtime (100 MHz) at both ends gives the clock.  Printed per work item: cycles per phase, slowest and fastest wave."""
import ctypes as C, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audiodiffuser_amd as A
from audiodiffuser_amd.weights import generate_weights

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
length = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
ITEMS, STAMPS = 4, 7
WAVE = 8 + ITEMS * STAMPS
dev = torch.device("cuda", 0)
cfg = A.PRESETS["c2"]()
net = A.UNet1dBase.from_config(cfg, compute_dtype="bf16")
net.load_state_dict(generate_weights(cfg, seed=0))
net = net.to(dev)
x = torch.randn(B, 1, length, device=dev)
for _ in range(2):
    net(x, torch.zeros(B, device=dev))
torch.cuda.synchronize()
lib = net.native(dev).lib
buf = (C.c_ulonglong * (2 * 8 * WAVE))()
fn = lib.adf_debug_up_timeline
fn.restype = C.c_int
assert fn(buf) == 0
PHASES = ["stage the tile (+ barrier)", "request the weight ring", "K loop", "epilogue -> LDS (+ barrier)", "16-byte stores issued", "closing barrier"]
for which in (0, 1):
    S = [[buf[(which * 8 + w) * WAVE + i] for i in range(WAVE)] for w in range(8)]
    if not S[0][1]:
        continue
    nitem = int(S[0][2])
    us = (max(S[w][1] for w in range(8)) - min(S[w][0] for w in range(8))) / 100.0
    first = min(S[w][8] for w in range(8))
    last = max(S[w][8 + (min(nitem, ITEMS) - 1) * STAMPS + 6] for w in range(8))
    print(f"\n=== workgroup {'0' if which == 0 else 'grid/2 + 3'}: {nitem} work items from item {int(S[0][3])}; {last - first} cycles first stamp -> last barrier, "
          f"{us:.1f} us by s_memrealtime => {(last - first) / us / 1e3:.2f} GHz")
    for it in range(min(nitem, ITEMS)):
        o = 8 + it * STAMPS
        tot = max(S[w][o + 6] for w in range(8)) - min(S[w][o] for w in range(8))
        print(f"item {it}: {tot} cycles")
        for k, name in enumerate(PHASES):
            v = [S[w][o + k + 1] - S[w][o + k] for w in range(8)]
            print(f"    {name:34s} slowest wave {max(v):7d}  fastest {min(v):7d}   {100.0 * max(v) / tot:5.1f} %")
