"""Generate tests/golden/golden_mha.npz: quantizable multi-head attention in ACTIVE mode.

The reference's `QuantizableMultiheadAttention` (aimet_torch/transformers/activation.py) is parsed from
the reference file with `ast` and executed at generation time on the CPU in float32, with stand-ins for
what it imports (the Add / Divide / MatMul modules of aimet_torch.v1.nn.modules.custom, which the
snapshot lacks). Every child the sim would wrap -- linear_Q / linear_K / linear_V / div / matmul_1 /
softmax / matmul_2 / out_proj -- is wrapped here in a stub that quantize-dequantizes the weight and the
output with preset encodings through the project's CPU oracle, which is what a StaticGridQuantWrapper
does in ACTIVE mode. Nothing of the reference's text is stored; the fixture holds data only.

Exact fixtures: inputs are multiples of 2^-3 in [-2, 2], weights of 2^-6 in [-1/2, 1/2], biases and
bias_k / bias_v of 2^-4, every encoding has a power-of-two step (ENCS below; probabilities: delta 2^-8
on [0, 255/256]), head_dim is 4 or 16 so the division by sqrt(head_dim) is exact. Every GEMM sum is then
exact in float32 in any order, every QDQ but softmax's sees exact values, and only the softmax can
differ between implementations.

Margin: U is the largest ulp distance between tests/mha_oracle.py's softmax and torch's CPU softmax
over the fixture's rows; a case is reseeded until every pre-QDQ probability lies at least 64 U float32
spacings from a rounding boundary of its QDQ. Oracle and reference then agree bit for bit on every
output (asserted), no element is excluded from any comparison, and U and the smallest margin met go
into README_mha.md.

batch_first: the reference views its [B H, L, head_dim] attention output as [B, L, E] without moving
the head axis (activation.py:428-429), which is not what nn.MultiheadAttention(batch_first=True)
computes; the project's module computes the latter. The batch_first case is therefore the reference
run sequence-first on the transposed inputs, its output transposed back.

    python tests/golden/make_golden_mha.py
"""
import ast
import json
import os
import sys
import types
import warnings
from typing import Optional, Tuple, Union

sys.dont_write_bytecode = True

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)
import mha_oracle as O  # noqa: E402

REF_ROOT = os.environ.get("AIMET_REFERENCE", "/root/reference")
SOURCE = "TrainingExtensions/torch/src/python/aimet_torch/transformers/activation.py"
F = np.float32
MARGIN = 64

ENCS = {"linear_Q": (-8.0, 127.0 / 16.0, 8), "linear_K": (-8.0, 127.0 / 16.0, 8), "linear_V": (-8.0, 127.0 / 16.0, 8),
        "div": (-4.0, 127.0 / 32.0, 8), "matmul_1": (-8.0, 127.0 / 16.0, 8), "softmax": (0.0, 255.0 / 256.0, 8),
        "matmul_2": (-8.0, 127.0 / 16.0, 8), "out_proj": (-8.0, 127.0 / 16.0, 8), "weight": (-2.0, 127.0 / 64.0, 8)}
CHILDREN = [k for k in ENCS if k != "weight"]


class Add(nn.Module):
    def forward(self, x, y):
        return x + y


class Divide(nn.Module):
    def forward(self, x, y):
        return torch.div(x, y)


class MatMul(nn.Module):
    def forward(self, x, y):
        return torch.matmul(x, y)


class StubWrapper(nn.Module):
    """ACTIVE mode of a static-grid wrapper with preset encodings: the weight and the output through
    the oracle's QDQ. `watch`: remember the inputs of the output QDQ (softmax's: the margin) and of
    the wrapped module (softmax's: the rows U is measured on)."""

    def __init__(self, module, out_enc, weight_enc, watch=False):
        super().__init__()
        self.module, self.out_enc, self.weight_enc, self.watch = module, out_enc, weight_enc, watch
        self.seen_in, self.seen_out = [], []

    def forward(self, *args):
        weight = getattr(self.module, "weight", None)
        if weight is not None:
            kept = weight.data
            weight.data = torch.from_numpy(O.qdq(kept.numpy(), self.weight_enc))
        try:
            y = self.module(*args)
        finally:
            if weight is not None:
                weight.data = kept
        if self.watch:
            self.seen_in.append(args[0].detach().numpy().copy())
            self.seen_out.append(y.detach().numpy().copy())
        return torch.from_numpy(O.qdq(y.detach().numpy(), self.out_enc))


def reference_namespace():
    ns = {"torch": torch, "Tensor": torch.Tensor, "nn": nn, "nnF": torch.nn.functional, "warnings": warnings,
          "Optional": Optional, "Tuple": Tuple, "Union": Union,
          "aimet_modules": types.SimpleNamespace(Add=Add, Divide=Divide, MatMul=MatMul)}
    path = os.path.join(REF_ROOT, SOURCE)
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if not isinstance(n, (ast.Import, ast.ImportFrom))]
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def grid(rng, shape, step_log2, lo, hi):
    """Multiples of 2^-step_log2 in [lo, hi]."""
    s = 2 ** step_log2
    return (rng.integers(int(lo * s), int(hi * s) + 1, shape) / s).astype(F)


def margin_of(p, enc):
    """The smallest distance of a pre-QDQ value inside the grid to a rounding boundary, in spacings of
    the value."""
    mn, mx, bw = enc
    delta = (mx - mn) / (2 ** bw - 1)
    inside = p[(p > mn) & (p < mx)].astype(np.float64)
    if not inside.size:
        return np.inf
    v = inside / delta
    dist = np.abs(np.abs(v - np.floor(v)) - 0.5) * delta
    return float(np.min(dist / np.spacing(np.abs(inside).astype(F)).astype(np.float64)))


B, L, S = 3, 4, 5
CASES = [
    dict(name="self_attention", E=16, H=4, self_attn=True, need_weights=True, average=True),
    dict(name="cross_kdim_vdim", E=32, H=2, kdim=8, vdim=12, need_weights=True, average=False),
    dict(name="bias_kv_padding", E=16, H=4, add_bias_kv=True, kpm=True, need_weights=True, average=True),
    dict(name="zero_attn_mask2d", E=32, H=2, add_zero_attn=True, attn_mask=2, need_weights=True, average=False),
    dict(name="mask3d_padding_nobias", E=16, H=4, bias=False, attn_mask=3, kpm=True, need_weights=True, average=True),
    dict(name="batch_first", E=16, H=4, batch_first=True, kpm=True, need_weights=False, average=True),
]


def one_case(ref, rng, case):
    """-> (arrays, smallest margin, U of this case's rows)."""
    E, H = case["E"], case["H"]
    kdim, vdim = case.get("kdim", E), case.get("vdim", E)
    bias = case.get("bias", True)
    module = ref["QuantizableMultiheadAttention"](E, H, bias=bias, add_bias_kv=case.get("add_bias_kv", False),
                                                  add_zero_attn=case.get("add_zero_attn", False), kdim=kdim, vdim=vdim)
    module.eval()
    arrays = {}
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.split(".")[0] not in ("linear_Q", "linear_K", "linear_V", "out_proj", "bias_k", "bias_v"):
                continue   # the packed projection nn.MultiheadAttention allocates; the forward never reads it
            if name.endswith("weight"):
                v = grid(rng, tuple(p.shape), 6, -0.5, 0.5)
            elif name in ("bias_k", "bias_v"):
                v = grid(rng, tuple(p.shape), 4, -2, 2)
            else:
                v = grid(rng, tuple(p.shape), 4, -1, 1)
            p.copy_(torch.from_numpy(v))
            arrays["w_" + name] = v
    wrappers = {}
    for name in CHILDREN:
        wrappers[name] = StubWrapper(getattr(module, name), ENCS[name], ENCS["weight"], watch=name == "softmax")
        setattr(module, name, wrappers[name])

    if case.get("self_attn"):
        query = key = value = grid(rng, (S, B, E), 3, -2, 2)
        Lq = S
    else:
        query, key, value = grid(rng, (L, B, E), 3, -2, 2), grid(rng, (S, B, kdim), 3, -2, 2), \
            grid(rng, (S, B, vdim), 3, -2, 2)
        Lq = L
    am = kpm = None
    if case.get("attn_mask"):
        am = rng.random((Lq, S) if case["attn_mask"] == 2 else (B * H, Lq, S)) < 0.35
        am[..., 0] = False
    if case.get("kpm"):
        kpm = rng.random((B, S)) < 0.35
        kpm[:, 0] = False
    t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    with torch.no_grad():
        out, weights = module(t(query), t(key), t(value), key_padding_mask=t(kpm), need_weights=case["need_weights"],
                              attn_mask=t(am), average_attn_weights=case["average"])
    out = out.numpy().copy()
    rows = wrappers["softmax"].seen_in[0]
    rows = rows.reshape(-1, rows.shape[-1])
    U = int(O.ulp_distance(O.softmax_rows(rows), torch.softmax(torch.from_numpy(rows), -1).numpy()).max())
    worst = margin_of(wrappers["softmax"].seen_out[0], ENCS["softmax"])

    bf = case.get("batch_first", False)
    if bf:   # see the module docstring
        query, key, value, out = (np.ascontiguousarray(np.swapaxes(a, 0, 1)) for a in (query, key, value, out))
    arrays.update(query=query, key=key, value=value, out=out)
    if am is not None:
        arrays["attn_mask"] = am
    if kpm is not None:
        arrays["key_padding_mask"] = kpm
    if weights is not None:
        arrays["weights"] = weights.numpy().copy()
    return arrays, worst, U


def generate(ref, U_required):
    rng = np.random.default_rng(20250317)
    g, meta, U_seen, worst_seen = {}, [], 0, np.inf
    for base in CASES:
        case, tries = dict(base), 0
        while True:
            tries += 1
            arrays, worst, U = one_case(ref, rng, case)
            U_seen = max(U_seen, U)
            if worst >= MARGIN * max(U_required, U):
                break
            assert tries < 20000, case
        case["tries"], case["worst"] = tries, worst
        worst_seen = min(worst_seen, worst)
        got_out, got_w = O.run_case(case, arrays, ENCS)
        assert np.array_equal(O.bits(got_out), O.bits(arrays["out"])), case
        assert (got_w is None) == ("weights" not in arrays)
        if got_w is not None:
            assert np.array_equal(O.bits(got_w), O.bits(arrays["weights"])), case
        for k, v in arrays.items():
            if k.startswith("w_"):   # multiples of 2^-6 in [-2, 2]: stored as their numerators
                n = (v * 64).astype(np.int16)
                assert np.array_equal(n.astype(F) / 64, v)
                v = n
            g["%s_%s" % (case["name"], k)] = v
        meta.append(case)
    return g, meta, U_seen, worst_seen


def main():
    ref = reference_namespace()
    U = 1
    while True:
        g, meta, U_seen, worst = generate(ref, U)
        if U_seen <= U:
            break
        U = U_seen   # a row of an accepted or rejected draw was farther from torch: once more with that
    for case in meta:
        print(case)
    g["cases"] = np.array(json.dumps(meta))
    g["encs"] = np.array(json.dumps(ENCS))
    g["margin"] = np.array([MARGIN, U], np.int64)
    path = os.path.join(HERE, "golden_mha.npz")
    np.savez_compressed(path, **g)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(g)))
    with open(os.path.join(HERE, "README_mha.md"), "w") as f:
        f.write(README % dict(U=U, margin=MARGIN, need=MARGIN * U, worst=worst, cases=len(meta),
                              size=os.path.getsize(path)))


README = """# golden_mha.npz

Written by `make_golden_mha.py` (see its docstring): %(cases)d cases of the reference's
`QuantizableMultiheadAttention` in ACTIVE mode with preset power-of-two encodings on dyadic data, %(size)d bytes.

| figure | value |
|---|---|
| U: largest ulp distance between `mha_oracle.softmax_rows` and torch's CPU softmax over the rows drawn for the fixture | %(U)d |
| margin required of every pre-QDQ probability, in float32 spacings from a rounding boundary (%(margin)d U) | %(need)d |
| smallest margin met by a stored case | %(worst).1f |

Arrays: `<case>_query / key / value / out / weights / attn_mask / key_padding_mask`, `<case>_w_<parameter>`
(int16 numerators over 64), `cases` and `encs` (JSON), `margin` = [%(margin)d, U].

On the MI355X the literal route (torch's GPU softmax) stays inside this margin: tests/test_mha_gpu.py
compares it, like the fused route, with the stored outputs bit for bit.

The batch_first case is the reference run sequence-first on the transposed inputs, its output transposed
back: the reference's own batch_first output mixes heads and positions (activation.py:428-429).
"""


if __name__ == "__main__":
    main()
