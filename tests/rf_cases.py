"""The rectified-flow sampler runs that tools/gen_golden_rf.py measures on the CPU and tests/test_rf_gpu.py runs on the device (test
infrastructure, not product code): one table, so the recorded ``dist_fp32_fp64`` of a run belongs to exactly the inputs the GPU test uses.

A run is the CPU restatement (tests/rf_ref.py for ReFlow and the Euler / Heun loop, oracle/samplers.py for the other loops) around one of the
oracle nets with deterministic random weights.  ``out_scale`` multiplies the net's output layer and ``noise_scale`` the unit noise: chosen (and
checked by the generator) so that the float64 result has max |y| > 0.05 and at most 1 % of its entries at |y| >= 1 -- a sampler that ends in
clamp(-1, 1) hides every difference in a saturated entry.  A velocity net has no c_out = sigma in front of it, so every run is well conditioned
(fp32 and float64 end 1e-7 .. 3e-6 apart, tests/golden/rf_golden.json): the scales only keep the result inside the clamp while the net still moves
the state by 0.3 .. 1.0.  The clamp run uses unit noise and scale 1 on purpose (half of its reference saturates)."""
from __future__ import annotations

import dataclasses
from collections import OrderedDict

import torch

import audiodiffuser_amd as A
from audiodiffuser_amd.adm_config import generate_weights as adm_weights
from audiodiffuser_amd.weights import generate_noise, generate_wavenet_weights, generate_weights
from oracle import samplers as S, unet1d as O1, unet2d as U, unet2d_oai as OA, wavenet as W
import rf_ref as RF

# net name -> (config, weight generator, names of the output layer's tensors, state shape [B, C, ...], labels or None)
NETS = {
    "tiny": (A.config_tiny, lambda c: generate_weights(c, seed=4), ("unet.to_out.to_out.weight",), (3, 1, 256), None),
    "tiny_cc": (A.config_tiny_cc, lambda c: generate_weights(c, seed=6), ("unet.to_out.to_out.weight",), (3, 1, 256), (7, 0, 3)),
    # the structure of the ``small`` fixture variant (three levels, attention at two) at the smallest width the device runs (a multiple of 32 channels;
    # the reference's constructor wants dim > 100) and at that variant's shape
    "u2d": (lambda: dataclasses.replace(U.config_sc09_small(), dim=128), lambda c: U.generate_weights(c, seed=5), ("final_conv.weight", "final_conv.bias"),
            (2, 2, 32, 16), (1, 4)),
    # H * W of the ADM net is a multiple of 256 (two levels, the coarsest a multiple of 64 pixels), so only the WaveNet run has a tail
    "adm": (A.config_c4_small, lambda c: adm_weights(c, seed=3), ("out.2.weight", "out.2.bias"), (3, 1, 32, 32), None),
    "wn": (A.config_c5_small, lambda c: generate_wavenet_weights(c, seed=5), ("output_projection.conv.weight", "output_projection.conv.bias"),
           (3, 1, 501), None),
}

# run name -> net, loop, steps, and what differs from the defaults below
DEFAULTS = dict(heun=True, cond_scale=1.0, out_scale=0.2, noise_scale=0.2, noise_seed=40)
RUNS = OrderedDict([
    ("tiny_euler", dict(net="tiny", loop="rf", steps=8, heun=False)),
    ("tiny_heun", dict(net="tiny", loop="rf", steps=8)),
    ("tiny_cc_euler", dict(net="tiny_cc", loop="rf", steps=6, heun=False, cond_scale=2.0, out_scale=0.15)),
    ("tiny_cc_heun", dict(net="tiny_cc", loop="rf", steps=6, cond_scale=2.0, out_scale=0.15)),
    ("u2d_euler", dict(net="u2d", loop="rf", steps=6, heun=False, out_scale=0.3)),
    ("u2d_heun", dict(net="u2d", loop="rf", steps=6, out_scale=0.3)),
    ("adm_heun", dict(net="adm", loop="rf", steps=6, out_scale=0.3)),
    ("wn_heun", dict(net="wn", loop="rf", steps=7, out_scale=2.0)),
    # pairings: DPM2MSampler(reflow=True) over the raw velocity; EDMSampler / UniPCSampler over the EDM wrapper on RFEDMSchedule(0.98, 0.02, N)
    ("tiny_dpm2m_reflow", dict(net="tiny", loop="dpm2m_reflow", steps=8)),
    ("u2d_edm_rfedm", dict(net="u2d", loop="edm_rfedm", steps=8, out_scale=0.3, noise_scale=0.005)),
    ("tiny_unipc_rfedm", dict(net="tiny", loop="unipc_rfedm", steps=8, noise_scale=0.005)),
    # the clamp run: the float64 reference leaves [-1, 1] on many entries
    ("tiny_clamp", dict(net="tiny", loop="rf", steps=6, out_scale=1.0, noise_scale=1.0)),
])


def spec(name: str) -> dict:
    return {**DEFAULTS, **RUNS[name], "name": name}


def ref_dtype(net_name: str):
    """float64, except for the ADM net, whose oracle only runs in fp32: its runs are compared with the fp32 restatement and have no ``dist_fp32_fp64``."""
    return torch.float32 if net_name == "adm" else torch.float64


def weights(net_name: str, out_scale: float = 1.0):
    """(config, fp32 state dict with the output layer scaled)."""
    make_cfg, make_w, out_keys, _, _ = NETS[net_name]
    cfg = make_cfg()
    w = make_w(cfg)
    for k in out_keys:
        w[k] = w[k] * out_scale
    return cfg, w


def labels(net_name: str):
    cl = NETS[net_name][4]
    return None if cl is None else torch.tensor(cl)


def oracle_net(net_name: str, cfg, w, dtype=torch.float32):
    """``net(x, t, cond_drop_prob=0.0)`` of the oracle restatement of the network, in ``dtype`` (the weights are widened for float64)."""
    p = w if dtype == torch.float32 else OrderedDict((k, v.to(dtype)) for k, v in w.items())
    cl = labels(net_name)
    if net_name in ("tiny", "tiny_cc"):
        return lambda x, t, cond_drop_prob=0.0: O1.unet1d_forward(p, cfg, x, t.to(x.dtype), classes=cl, cond_drop_prob=cond_drop_prob)
    if net_name == "u2d":
        return lambda x, t, cond_drop_prob=0.0: U.unet2d_forward(p, cfg, x, t.to(x.dtype), classes=cl, cond_drop_prob=cond_drop_prob)
    if net_name == "adm":
        assert dtype == torch.float32, "oracle/unet2d_oai.py is an fp32 restatement (GroupNorm32 and the sinusoidal features cast to float, as the reference does)"
        return lambda x, t, cond_drop_prob=0.0: OA.unet2d_forward(p, cfg, x, t)
    wn = W.wavenet_net(p, cfg)
    return lambda x, t, cond_drop_prob=0.0: wn(x, t.to(x.dtype))


def noise_of(sp: dict) -> torch.Tensor:
    shape = NETS[sp["net"]][3]
    return generate_noise(sp["noise_seed"], shape[0], int(torch.tensor(shape[2:]).prod()), channels=shape[1]).reshape(shape) * sp["noise_scale"]


def sigmas_of(sp: dict) -> torch.Tensor:
    n = sp["steps"]
    return RF.rfedm_schedule(0.98, 0.02, n) if sp["loop"].endswith("rfedm") else RF.linear_schedule(1.0, 0.0, n + 1)


def reference(name: str, dtype=torch.float64, clamp: bool = True) -> torch.Tensor:
    """The CPU result of run ``name`` in ``dtype``.  ``clamp=False`` (the Euler / Heun loop only): the state before the closing clamp."""
    sp = spec(name)
    cfg, w = weights(sp["net"], sp["out_scale"])
    net = oracle_net(sp["net"], cfg, w, dtype)
    noise, sig, n = noise_of(sp).to(dtype), sigmas_of(sp), sp["steps"]
    with torch.no_grad():
        if sp["loop"] == "rf":
            return RF.euler_sampler(noise, RF.make_fn(False, net, sp["cond_scale"]), sig, n, use_heun=sp["heun"], clamp=clamp)
        assert clamp
        if sp["loop"] == "dpm2m_reflow":
            return S.dpm2m_sampler(noise, RF.make_fn(False, net, sp["cond_scale"]), sig, n, reflow=True)
        fn = RF.make_fn(True, net, sp["cond_scale"])
        if sp["loop"] == "edm_rfedm":
            return S.edm_sampler(noise, fn, sig, n, s_churn=0.0, use_heun=True)
        assert sp["loop"] == "unipc_rfedm"
        return S.unipc_sampler(noise, fn, sig, n, order=2, log_time_spacing=True, x0_pred=True)
