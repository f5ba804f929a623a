"""CPU: what the ten samplers hand to the library, and what its host step logic makes of it, over a sweep of degenerate and ordinary sizes.

Per sampler of the sweep: the bytes of its ``adf_sampler_desc`` (the first part of the hipGraph cache key, adf_api.hip) and the NFE that
``adf_sampler_nfe`` -- the counting pass of the device loop, no GPU involved -- reports on seven schedules, or -1 where the driver rejects
the schedule.  The table in tests/golden/sampler_host_sweep.json was recorded once from the library as it was before the sampler drivers
were rewritten on ``SamplerCtx``'s members (tools/gen_sampler_host_sweep.py, which takes the case list from this module)."""
import base64
import ctypes as C
import json
import os

import torch

import audiodiffuser_amd as A
from audiodiffuser_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_host_sweep.json")
STEPS = (1, 2, 3, 4, 7, 10)
CHURN = dict(s_tmin=0.05, s_tmax=50.0, s_churn=30.0, s_noise=1.003)
ANCESTRAL = ((1.0, 1.0), (7.0, 0.6), (0.0, 1.0))          # (rho, eta); rho = 0 is rejected by ADPM2Sampler's driver


def sweep_cases():
    """[(id, sampler)], 96 per entry of STEPS."""
    out = []
    for n in STEPS:
        for heun in (True, False):
            out.append((f"edm-n{n}-h{int(heun)}", A.EDMSampler(s_churn=0.0, s_noise=1.0, num_steps=n, use_heun=heun)))
            out.append((f"edm-n{n}-h{int(heun)}-churn", A.EDMSampler(num_steps=n, use_heun=heun, **CHURN)))
            for alpha in (1.0, 0.5):
                out.append((f"alpha-n{n}-a{alpha}-h{int(heun)}", A.EDMAlphaSampler(alpha=alpha, num_steps=n, use_heun=heun)))
        for order in range(6):
            for logsp in (True, False):
                for x0 in (True, False):
                    for multi in (True, False):
                        out.append((f"dpm-n{n}-o{order}-l{int(logsp)}-x{int(x0)}-m{int(multi)}",
                                    A.DPMSampler(1.0, order=order, num_steps=n, multisteps=multi, x0_pred=x0, log_time_spacing=logsp)))
                    out.append((f"unipc-n{n}-o{order}-l{int(logsp)}-x{int(x0)}",
                                A.UniPCSampler(num_steps=n, order=order, x0_pred=x0, log_time_spacing=logsp)))
            out.append((f"lms-n{n}-o{order}", A.LMSSampler(num_steps=n, order=order)))
        for reflow in (False, True):
            out.append((f"dpm2m-n{n}-r{int(reflow)}", A.DPM2MSampler(num_steps=n, reflow=reflow)))
        out.append((f"dpm2-n{n}", A.DPM2Sampler(num_steps=n, s_churn=0.0)))
        out.append((f"dpm2-n{n}-churn", A.DPM2Sampler(num_steps=n, **CHURN)))
        for rho, eta in ANCESTRAL:
            out.append((f"adpm2-n{n}-r{rho}-e{eta}", A.ADPM2Sampler(rho=rho, num_steps=n, eta=eta)))
            out.append((f"adpmpp2s-n{n}-r{rho}-e{eta}", A.ADPMPP2SSampler(rho=rho, num_steps=n, eta=eta)))
    return out


def schedules():
    karras = lambda n: A.KarrasSchedule(0.002, 80.0, 7.0, n)()
    return [karras(n) for n in (1, 4, 7, 10, 11)] + [torch.cat([karras(n), torch.zeros(1)]) for n in (9, 10)]


def record():
    """{id: [base64 of the descriptor's bytes, [NFE or -1 per schedule]]} from the library that is loaded."""
    lib = _lib.load_library()
    scheds = [(C.c_float * len(s))(*s.tolist()) for s in schedules()]
    table = {}
    for cid, smp in sweep_cases():
        desc = smp._desc(0.2)
        table[cid] = [base64.b64encode(bytes(desc)).decode(), [lib.adf_sampler_nfe(C.byref(desc), arr, len(arr)) for arr in scheds]]
    return table


def test_descriptor_bytes_and_host_step_logic_over_the_sweep():
    want = json.load(open(GOLDEN))
    got = record()
    assert list(got) == list(want), "the sweep's case list and the recorded table disagree: regenerate only from an unmodified library"
    assert len(got) >= 500
    nfe = [v for row in want.values() for v in row[1]]
    assert sum(v >= 0 for v in nfe) >= 1000 and sum(v == -1 for v in nfe) >= 1000
    for cid, row in want.items():
        assert got[cid][0] == row[0], f"{cid}: descriptor bytes {base64.b64decode(got[cid][0]).hex()} != {base64.b64decode(row[0]).hex()}"
        assert got[cid][1] == row[1], f"{cid}: NFE per schedule {got[cid][1]} != {row[1]}"
