"""The conv_gemm_up_kernel launches of a rocprofv3 kernel_trace.csv inside the sampler window, split by their place in the walk: the N transposed-conv
launches of one evaluation come in the same order every time (configs[1] at 16384 samples: L = 16, 64, 256), so launch k of the window belongs to level k mod N.
usage: up_launches.py kernel_trace.csv [N = 3]       -> per level: kernel, grid, launches, mean / median / min us"""
import csv, statistics, sys
path, n = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 3
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
names = [r['Kernel_Name'] for r in rows]
first = next(i for i, k in enumerate(names) if 'edm_coef' in k)
last = max(i for i, k in enumerate(names) if 'rk2_kernel' in k or 'euler_kernel' in k or 'dpm_kernel' in k)
up = [r for r in rows[first:last + 1] if 'conv_gemm_up_kernel' in r['Kernel_Name']]
assert up and len(up) % n == 0, (len(up), n)
for lvl in range(n):
    sel = up[lvl::n]
    us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in sel]
    kn = {r['Kernel_Name'].replace('adf::', '').replace('void ', '').split('(')[0] + ' g' + r['Grid_Size_X'] for r in sel}
    print(f"level {lvl}: {' | '.join(sorted(kn)):48s} launches {len(us):4d}  mean {statistics.mean(us):6.2f} us  median {statistics.median(us):6.2f}  min {min(us):6.2f}")
print(f"per evaluation: {sum((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in up) / (len(up) / n):.1f} us in {n} launches")
