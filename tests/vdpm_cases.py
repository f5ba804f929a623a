"""The runs of the two program-driven samplers (VDPMSampler, VUniPCSampler) that tools/gen_golden_vdpm.py measures on the CPU and
tests/test_vdpm_gpu.py runs on the device, and the host cases of tests/test_vdpm_host.py (test infrastructure, not product code): one table, so the
recorded ``dist_fp32_fp64`` of a run belongs to exactly the inputs the GPU test uses.

A run is the CPU restatement tests/vdpm_ref.py around one of the oracle nets of tests/rf_cases.py with deterministic random weights, at the shapes of
tests/vsamp_cases.py (``SHAPES``).  ``u2d_un`` is the ``small`` UNet2dBase structure of ``u2d`` WITHOUT classes, as in the two shipped files: the
reference drops ``classes`` on the single-step solver's inner evaluations and on every UniPC corrector evaluation, so only the multistep runs take the
class-conditional nets (``u2d``, ``tiny_cc``).

``out_scale`` multiplies the net's output layer, ``noise_scale`` the unit noise: chosen per run (and checked by the generator) so that the float64
result is finite, has max |y| > 0.05 and at most 1 % of its entries at the final clamp, and fp32 and float64 end less than 2.5e-4 apart -- a clamp
hides every difference in a saturated entry.  A noise-prediction run (``x0_pred=False``) multiplies the state by alpha_next / alpha_cur, over the whole
range 1 / alpha(-15) ~ 1800 in all: its noise is scaled by 3e-4 so that the result stays inside the clamp (2e-3 over the range 0.9 to 0.1, where the
gain is smaller)."""
from __future__ import annotations

import dataclasses
from collections import OrderedDict

import torch

import rf_cases as RC
import vdpm_ref as DR
import vsamp_cases as VC
import vsamp_ref as VR
from oracle import unet2d as U

SHAPES = VC.SHAPES
NET_OF = {"tiny1": "tiny"}

DEFAULTS = dict(cond_scale=1.0, out_scale=0.2, noise_scale=0.3, noise_seed=70, t0=1.0, t1=0.0, x0_pred=True, multisteps=False)
RUNS = OrderedDict([
    # the two shipped settings (configs/experiment/sc09_inference/diffunet_complex_sc09_eval_vobj_dpm.yaml, ..._unipc.yaml), over the full range
    ("dpm_u2d_shipped", dict(shape="u2d", net="u2d_un", sampler="dpm", order=3, steps=7, x0_pred=False, out_scale=0.05, noise_scale=3e-4)),
    ("unipc_u2d_shipped", dict(shape="u2d", net="u2d_un", sampler="unipc", order=2, steps=6, noise_scale=0.2)),
    # VDPMSampler, single-step
    ("dpm_tiny_single3_x0", dict(shape="tiny", sampler="dpm", order=3, steps=6, out_scale=0.1, noise_scale=0.2)),
    ("dpm_tiny_single2_x0", dict(shape="tiny", sampler="dpm", order=2, steps=5, out_scale=0.1, noise_scale=0.2)),
    ("dpm_wn_single3_x0", dict(shape="wn", sampler="dpm", order=3, steps=8, out_scale=2.0, noise_scale=0.2)),
    # ... multistep
    ("dpm_tiny_multi3_x0", dict(shape="tiny", sampler="dpm", order=3, steps=6, multisteps=True, out_scale=0.15, noise_scale=0.03)),
    ("dpm_tiny_multi3_eps", dict(shape="tiny", sampler="dpm", order=3, steps=6, multisteps=True, x0_pred=False, noise_scale=3e-4)),
    ("dpm_u2d_multi2_x0", dict(shape="u2d", sampler="dpm", order=2, steps=5, multisteps=True)),
    ("dpm_tiny_cc_multi3_guided", dict(shape="tiny_cc", sampler="dpm", order=3, steps=5, multisteps=True, cond_scale=3.0, out_scale=0.07, noise_scale=0.07)),
    ("dpm_adm_multi2_x0", dict(shape="adm", sampler="dpm", order=2, steps=4, multisteps=True)),
    # VUniPCSampler
    ("unipc_u2d_o1", dict(shape="u2d", net="u2d_un", sampler="unipc", order=1, steps=4)),
    ("unipc_u2d_o3", dict(shape="u2d", net="u2d_un", sampler="unipc", order=3, steps=5, noise_scale=0.15)),
    ("unipc_u2d_o2_eps", dict(shape="u2d", net="u2d_un", sampler="unipc", order=2, steps=5, x0_pred=False, out_scale=0.3, noise_scale=2e-3, t0=0.9, t1=0.1)),
    ("unipc_wn_o3", dict(shape="wn", sampler="unipc", order=3, steps=5, out_scale=2.0, noise_scale=0.2)),
    ("unipc_tiny1_o2", dict(shape="tiny1", sampler="unipc", order=2, steps=4, out_scale=0.1, noise_scale=0.2)),
])

# ---- host cases (tests/test_vdpm_host.py; recorded from the reference's classes by tools/gen_golden_vdpm.py) -----------------------------------
# name -> (sampler, constructor keywords, schedule).  Single-step: num_steps % 3 in {0, 1, 2} and % 2 in {0, 1}; multistep: warm-up and trailing lower
# orders, num_steps == order as the edge; UniPC: orders 1 to 3, the last step uncorrected.
_full, _part = (lambda n: torch.linspace(1.0, 0.0, n)), (lambda n: torch.linspace(0.9, 0.1, n))
CASES = OrderedDict([
    ("dpm_s3_n6", ("dpm", dict(cond_scale=1.0, order=3, num_steps=6), _full(6))),                         # [3, 2, 1]
    ("dpm_s3_n7_eps", ("dpm", dict(cond_scale=1.0, order=3, num_steps=7, x0_pred=False), _part(7))),       # [3, 3, 1]
    ("dpm_s3_n8", ("dpm", dict(cond_scale=1.0, order=3, num_steps=8), _part(8))),                          # [3, 3, 2]
    ("dpm_s3_n2_eps", ("dpm", dict(cond_scale=1.0, order=3, num_steps=2, x0_pred=False), _part(2))),       # [2]
    ("dpm_s2_n6_eps", ("dpm", dict(cond_scale=1.0, order=2, num_steps=6, x0_pred=False), _part(6))),       # [2, 2, 2]
    ("dpm_s2_n5", ("dpm", dict(cond_scale=1.0, order=2, num_steps=5), _full(5))),                          # [2, 2, 1]
    ("dpm_s1_n4", ("dpm", dict(cond_scale=1.0, order=1, num_steps=4), _part(4))),
    ("dpm_m3_n6", ("dpm", dict(cond_scale=1.0, order=3, num_steps=6, multisteps=True), _full(6))),         # 8 calls, 6 used
    ("dpm_m3_n6_eps", ("dpm", dict(cond_scale=1.0, order=3, num_steps=6, multisteps=True, x0_pred=False), _part(6))),
    ("dpm_m3_n3", ("dpm", dict(cond_scale=1.0, order=3, num_steps=3, multisteps=True), _part(3))),         # num_steps == order
    ("dpm_m2_n5_eps", ("dpm", dict(cond_scale=1.0, order=2, num_steps=5, multisteps=True, x0_pred=False), _part(5))),
    ("dpm_m2_n2", ("dpm", dict(cond_scale=1.0, order=2, num_steps=2, multisteps=True), _full(2))),
    ("dpm_m1_n3", ("dpm", dict(cond_scale=1.0, order=1, num_steps=3, multisteps=True), _part(3))),         # a dead call at every step
    ("unipc_o1_n4", ("unipc", dict(num_steps=4, order=1), _full(4))),
    ("unipc_o2_n6", ("unipc", dict(num_steps=6, order=2), _full(6))),
    ("unipc_o2_n5_eps", ("unipc", dict(num_steps=5, order=2, x0_pred=False), _part(5))),
    ("unipc_o3_n6", ("unipc", dict(num_steps=6, order=3), _part(6))),
    ("unipc_o3_n6_eps", ("unipc", dict(num_steps=6, order=3, x0_pred=False), _part(6))),
    ("unipc_o3_n3", ("unipc", dict(num_steps=3, order=3), _full(3))),                                      # num_steps == order
    ("unipc_o1_n1", ("unipc", dict(num_steps=1, order=1), _part(2))),                                      # no corrector at all
])
TOY_SHAPE, TOY_SEED = (2, 1, 4, 4), 13           # 4-D: the reference's UniPC runs orders >= 2 on nothing else
toy_fn = VC.toy_fn


def toy_noise(scale: float = 0.7) -> torch.Tensor:
    return torch.randn(*TOY_SHAPE, generator=torch.Generator().manual_seed(TOY_SEED)) * scale


def toy_scale(kw: dict) -> float:
    """The noise-prediction form multiplies the state by up to 1 / alpha(-15): a smaller start keeps the toy run inside the clamp."""
    return 0.7 if kw.get("x0_pred", True) else 0.05


def spec(name: str) -> dict:
    sp = {**DEFAULTS, **RUNS[name], "name": name}
    sp.setdefault("net", NET_OF.get(sp["shape"], sp["shape"]))
    return sp


def ref_dtype(sp: dict):
    return RC.ref_dtype(sp["net"])


def weights(net_name: str, out_scale: float = 1.0):
    """(config, fp32 state dict with the output layer scaled); ``u2d_un``: the structure and seed of rf_cases' ``u2d`` without classes."""
    if net_name != "u2d_un":
        return RC.weights(net_name, out_scale)
    cfg = dataclasses.replace(U.config_sc09_small(num_classes=0), dim=128)
    w = U.generate_weights(cfg, seed=5)
    for k in ("final_conv.weight", "final_conv.bias"):
        w[k] = w[k] * out_scale
    return cfg, w


def labels(net_name: str):
    return None if net_name == "u2d_un" else RC.labels(net_name)


def oracle_net(net_name: str, cfg, w, dtype):
    if net_name != "u2d_un":
        return RC.oracle_net(net_name, cfg, w, dtype)
    p = w if dtype == torch.float32 else OrderedDict((k, v.to(dtype)) for k, v in w.items())
    return lambda x, t, cond_drop_prob=0.0: U.unet2d_forward(p, cfg, x, t.to(x.dtype), classes=None, cond_drop_prob=cond_drop_prob)


def noise_of(sp: dict) -> torch.Tensor:
    shape = SHAPES[sp["shape"]]
    n = int(torch.tensor(shape[2:]).prod())
    return RC.generate_noise(sp["noise_seed"], shape[0], n, channels=shape[1]).reshape(shape) * sp["noise_scale"]


def sigmas_of(sp: dict) -> torch.Tensor:
    return torch.linspace(sp["t0"], sp["t1"], sp["steps"])


def sampler_kwargs(sp: dict) -> dict:
    """The constructor keywords of the plugin class (and of the reference class) of this run, without ``use_graph``."""
    kw = dict(num_steps=sp["steps"], order=sp["order"], cond_scale=sp["cond_scale"], x0_pred=sp["x0_pred"])
    if sp["sampler"] == "dpm":
        kw["multisteps"] = sp["multisteps"]
    return kw


def reference(name: str, dtype=torch.float64, clamp: bool = True, record: list = None) -> torch.Tensor:
    """The CPU result of run ``name`` with the state in ``dtype``, without the reference's discarded evaluations."""
    sp = spec(name)
    cfg, w = weights(sp["net"], sp["out_scale"])
    fn = VR.make_v_fn(oracle_net(sp["net"], cfg, w, dtype), sp["cond_scale"])
    noise, sig = noise_of(sp).to(dtype), sigmas_of(sp)
    with torch.no_grad():
        if sp["sampler"] == "dpm":
            return DR.dpm_sampler(noise, fn, sig, sp["steps"], sp["order"], sp["multisteps"], sp["x0_pred"], record=record, clamp=clamp, dead_calls=False)
        return DR.unipc_sampler(noise, fn, sig, sp["steps"], sp["order"], sp["x0_pred"], record=record, clamp=clamp)
