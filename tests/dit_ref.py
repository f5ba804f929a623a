"""CPU restatement of the reference's ``DiT.forward`` (src/models/backbones/dit.py:382-429) over a flat weight dict, in any dtype (float64 is the
reference the device is held to), with the cases the DiT tests run.  Pinned to the reference's own module by tools/gen_golden_dit.py
(tests/golden/dit_golden.npz, tests/test_dit_ref.py).

``forward`` also takes four deliberate mis-statements (``gelu="erf"``, ``eps=1e-5``, ``gate_tile=128``, ``sin_first=True``): tests/test_dit_ref.py
shows that each of them moves the output of the cases by more than the bar the device is held to, i.e. that the cases can see such a bug.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch

from audiodiffuser_amd.dit import DiTConfig, generate_weights

# case -> constructor kwargs, batch, and what else shapes its inputs.  `dims` 3: the [B, C, L] form.  `lowvar`: tiny with inputs, x_embedder weights and bias
# and pos_embed scaled down so that the rows entering blocks.0.norm1 have variance ~1e-3 (pos_embed is a state-dict tensor like any other: the
# fixed sin-cos table alone has row variance 0.5, which hides eps = 1e-6).
_TINY = dict(input_size=[16, 8], patch_size=[8, 4], in_channels=4, hidden_size=128, depth=2, num_heads=2, mlp_ratio=4.0)
CASES = OrderedDict([
    ("tiny", dict(kw=_TINY, B=3)),
    ("odd", dict(kw=dict(input_size=[32, 16], patch_size=[4, 4], in_channels=4, hidden_size=192, depth=2, num_heads=3, mlp_ratio=2.5), B=2)),
    ("wide", dict(kw=dict(input_size=[64, 32], patch_size=[8, 4], in_channels=4, hidden_size=384, depth=1, num_heads=6, mlp_ratio=4.0), B=2)),
    ("hd32", dict(kw=dict(input_size=[16, 16], patch_size=[2, 2], in_channels=2, hidden_size=128, depth=1, num_heads=4, mlp_ratio=4.0), B=1)),
    ("labels", dict(kw=dict(_TINY, label_cond=True, num_classes=10), B=3)),
    ("row", dict(kw=dict(input_size=[1, 256], patch_size=[1, 4], in_channels=4, hidden_size=128, depth=1, num_heads=2, mlp_ratio=4.0), B=2, dims=3)),
    ("lowvar", dict(kw=_TINY, B=2, x_scale=0.05, pe_scale=0.05, pb_scale=0.2, pos_scale=0.04)),
])
GOLDEN_CASES = ("tiny", "labels", "lowvar")       # the variants tools/gen_golden_dit.py runs through the reference module
TIMES = (-0.9, 0.35, 0.8)                         # c_noise-sized conditioning times, one per sample


def config(case: str) -> DiTConfig:
    kw = dict(CASES[case]["kw"])
    kw["input_size"], kw["patch_size"] = tuple(kw["input_size"]), tuple(kw["patch_size"])
    return DiTConfig(**kw)


def ctor_kwargs(case: str) -> dict:
    return dict(CASES[case]["kw"])


def weights(case: str, seed: int = 3) -> "OrderedDict[str, torch.Tensor]":
    """fp32 weights of a case: name-keyed and deterministic, the zero-initialised tensors random (audiodiffuser_amd.dit.generate_weights)."""
    sp = CASES[case]
    w = generate_weights(config(case), seed)
    w["x_embedder.proj.weight"] = w["x_embedder.proj.weight"] * sp.get("pe_scale", 1.0)
    w["x_embedder.proj.bias"] = w["x_embedder.proj.bias"] * sp.get("pb_scale", 1.0)
    w["pos_embed"] = w["pos_embed"] * sp.get("pos_scale", 1.0)
    return w


def inputs(case: str, B: int = None, seed: int = 11):
    """(x, t, classes or None) of a case, fp32 / int64 on the CPU.  Another ``B`` or ``seed`` gives another input of the same net."""
    sp, cfg = CASES[case], config(case)
    B = sp["B"] if B is None else B
    g = torch.Generator().manual_seed(seed)
    shape = (B, cfg.in_channels) + ((cfg.input_size[1],) if sp.get("dims", 4) == 3 else tuple(cfg.input_size))
    x = torch.randn(*shape, generator=g) * sp.get("x_scale", 1.0)
    t = torch.tensor([TIMES[(i + seed) % len(TIMES)] for i in range(B)], dtype=torch.float32)
    classes = torch.tensor([(3 * i + seed) % cfg.num_classes for i in range(B)], dtype=torch.int64) if cfg.label_cond else None
    return x, t, classes


def _layer_norm(x, eps, w=None, b=None):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    y = (x - mu) / torch.sqrt(var + eps)
    return y if w is None else y * w + b


def _silu(x):
    return x * torch.sigmoid(x)


def _gelu(x, kind):
    if kind == "erf":
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def forward(w, cfg: DiTConfig, x, t, classes=None, cond_drop_prob=0.0, dtype=torch.float64, taps: dict = None,
            gelu: str = "tanh", eps: float = 1e-6, gate_tile: int = 0, sin_first: bool = False):
    """``DiT.forward(x, t, classes, cond_drop_prob=0 or 1)`` in ``dtype``.  ``taps``, where given, receives "x_embedder", "c", "blocks.<i>",
    "blocks.<i>.attn", "blocks.<i>.mlp" and "final_layer"."""
    W = {k: v.to(dtype) for k, v in w.items()}
    D, heads = cfg.hidden_size, cfg.num_heads
    three = x.ndim == 3
    x = (x.unsqueeze(2) if three else x).to(dtype)
    B, C, H, Wd = x.shape
    p1, p2 = cfg.patch_size
    assert (H, Wd) == tuple(cfg.input_size)
    gh, gw = H // p1, Wd // p2
    T = gh * gw
    # PatchEmbed: conv with stride = kernel = patch, flattened to tokens (h, w), + pos_embed
    xp = x.reshape(B, C, gh, p1, gw, p2).permute(0, 2, 4, 1, 3, 5).reshape(B, T, C * p1 * p2)
    h = xp @ W["x_embedder.proj.weight"].reshape(D, -1).T + W["x_embedder.proj.bias"] + W["pos_embed"][0]
    # TimestepEmbedder(hidden, frequency_embedding_size = hidden): cos half first (conditioner.py:33-56)
    half = D // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=dtype) / half)
    args = t.to(dtype)[:, None] * freqs[None]
    emb = torch.cat([torch.sin(args), torch.cos(args)] if sin_first else [torch.cos(args), torch.sin(args)], dim=-1)
    c = _silu(emb @ W["t_embedder.mlp.0.weight"].T + W["t_embedder.mlp.0.bias"]) @ W["t_embedder.mlp.2.weight"].T + W["t_embedder.mlp.2.bias"]
    if classes is not None:
        # LabelEmbedder (conditioner.py:92-111) with the deterministic label masks: cond_drop_prob 0 keeps every label, 1 takes the null embedding
        assert cond_drop_prob in (0, 0.0, 1, 1.0)
        e = W["y_embedder.label_emb.weight"][classes]
        if cond_drop_prob:
            e = W["y_embedder.null_classes_emb"].expand(B, -1)
        e = _layer_norm(e, 1e-5, W["y_embedder.class_to_cond.0.weight"], W["y_embedder.class_to_cond.0.bias"])
        e = _silu(e @ W["y_embedder.class_to_cond.1.weight"].T + W["y_embedder.class_to_cond.1.bias"])
        c = e @ W["y_embedder.class_to_cond.3.weight"].T + W["y_embedder.class_to_cond.3.bias"] + c
    if taps is not None:
        taps["x_embedder"], taps["c"] = h.clone(), c.clone()

    def gate_rows(g):
        """[B, D] gate -> [B, T, D]; ``gate_tile``: the mis-statement that reads the gate of a GEMM tile's first row for the whole tile."""
        if not gate_tile:
            return g.unsqueeze(1)
        rows = torch.arange(B * T)
        return g[((rows // gate_tile) * gate_tile) // T].reshape(B, T, D)

    hd = D // heads
    for i in range(cfg.depth):
        p = f"blocks.{i}"
        m = _silu(c) @ W[f"{p}.adaLN_modulation.1.weight"].T + W[f"{p}.adaLN_modulation.1.bias"]
        sh1, sc1, g1, sh2, sc2, g2 = m.chunk(6, dim=1)
        xn = _layer_norm(h, eps) * (1 + sc1.unsqueeze(1)) + sh1.unsqueeze(1)
        q = xn @ W[f"{p}.attn.to_q.weight"].T
        k, v = (xn @ W[f"{p}.attn.to_kv.weight"].T).chunk(2, dim=-1)
        q, k, v = (u.reshape(B, T, heads, hd).transpose(1, 2) for u in (q, k, v))
        a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1) @ v
        a = a.transpose(1, 2).reshape(B, T, D) @ W[f"{p}.attn.to_out.weight"].T
        h = h + gate_rows(g1) * a
        xn = _layer_norm(h, eps) * (1 + sc2.unsqueeze(1)) + sh2.unsqueeze(1)
        f = _gelu(xn @ W[f"{p}.mlp.fc1.weight"].T + W[f"{p}.mlp.fc1.bias"], gelu) @ W[f"{p}.mlp.fc2.weight"].T + W[f"{p}.mlp.fc2.bias"]
        h = h + gate_rows(g2) * f
        if taps is not None:
            taps[p], taps[p + ".attn"], taps[p + ".mlp"] = h.clone(), a, f
    m = _silu(c) @ W["final_layer.adaLN_modulation.1.weight"].T + W["final_layer.adaLN_modulation.1.bias"]
    sh, sc = m.chunk(2, dim=1)
    y = (_layer_norm(h, eps) * (1 + sc.unsqueeze(1)) + sh.unsqueeze(1)) @ W["final_layer.linear.weight"].T + W["final_layer.linear.bias"]
    if taps is not None:
        taps["final_layer"] = y
    # unpatchify: nhwpqc -> nchpwq
    out = y.reshape(B, gh, gw, p1, p2, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, Wd)
    return out.squeeze(2) if three else out


def net_fn(case: str, w=None, classes=None):
    """net(x, t, cond_drop_prob=0.0) in the dtype of ``x``: what the denoiser and sampler restatements (oracle/edm.py, tests/precond_ref.py,
    tests/rf_ref.py, tests/loss_ref.py) call."""
    cfg = config(case)
    w = weights(case) if w is None else w

    def net(x, t, cond_drop_prob=0.0, **_):
        return forward(w, cfg, x, t, classes=classes, cond_drop_prob=cond_drop_prob, dtype=x.dtype)
    return net
