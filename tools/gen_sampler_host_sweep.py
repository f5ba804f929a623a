"""Records tests/golden/sampler_host_sweep.json: descriptor bytes and adf_sampler_nfe results of the sweep in
tests/test_sampler_host_sweep.py (the case list lives there), from whatever library the package loads -- point ADF_HIP_LIB at a build of
the commit the table is to pin.  No GPU needed.

    python tools/gen_sampler_host_sweep.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_sampler_host_sweep as sweep      # noqa: E402

if __name__ == "__main__":
    table = sweep.record()
    nfe = [v for row in table.values() for v in row[1]]
    with open(sweep.GOLDEN, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(table)} descriptors, {sum(v >= 0 for v in nfe)} accepted, {sum(v == -1 for v in nfe)} rejected NFE values, "
          f"{os.path.getsize(sweep.GOLDEN)} bytes -> {sweep.GOLDEN}")
