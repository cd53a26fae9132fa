"""Generate tests/golden/golden_dfq.npz from the REFERENCE's data-free-quantization arithmetic.

The reference's definitions (aimet_common/batch_norm_fold.py: batch_norm_fold;
aimet_common/cross_layer_equalization.py: compute_scaling_params_for_conv,
compute_scaling_params_for_depthwise_conv, fold_scaling_params_for_conv,
fold_scaling_params_for_depthwise_conv, _absorb_bias) are parsed from the reference files and
executed at generation time, on the CPU in float32; nothing of their text is stored. The fixture
holds data only: inputs in module layout (with the layout flags the reference's torch layer acts on:
transposed weights permuted to [out][in], 1-d weights given a trailing axis) and the reference's
outputs, brought back to module layout. tests/golden/README_dfq.md describes the cases.

    python tests/golden/make_golden_dfq.py
"""
import ast
import os
import sys
from typing import Union

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("AIMET_REFERENCE", "/root/reference")
COMMON = "TrainingExtensions/common/src/python/aimet_common"
NAMES = {"batch_norm_fold.py": ("batch_norm_fold",),
         "cross_layer_equalization.py": ("compute_scaling_params_for_conv",
                                         "compute_scaling_params_for_depthwise_conv", "fold_scaling_params_for_conv",
                                         "fold_scaling_params_for_depthwise_conv", "_absorb_bias")}
F = np.float32


def reference_functions():
    ns = {"np": np, "Union": Union}
    for fname, names in NAMES.items():
        path = os.path.join(REF_ROOT, COMMON, fname)
        tree = ast.parse(open(path).read(), path)
        fns = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(f.name for f in fns) == sorted(names), [f.name for f in fns]
        for f in fns:
            f.decorator_list = []   # static methods of abstract classes: plain functions here
        exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns


def to4d(w, transposed):
    """What the reference's torch layer hands to numpy: [out][in][kh][kw]."""
    if w.ndim == 3:
        w = w[..., None]
    if w.ndim == 2:
        w = w[..., None, None]
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3)) if transposed else w


def from4d(v, shape, transposed):
    if transposed:
        v = v.transpose(1, 0, 2, 3)
    return np.ascontiguousarray(v).reshape(shape).astype(F)


def weight(rng, shape, axis):
    """Normal weights whose channels along `axis` have log-uniform ranges over two decades."""
    w = rng.standard_normal(shape)
    r = np.exp(rng.uniform(np.log(0.05), np.log(5.0), shape[axis]))
    bshape = [1] * len(shape)
    bshape[axis] = shape[axis]
    return (w * r.reshape(bshape)).astype(F)


# (name, w0 module shape, transposed0, w1 module shape, transposed1, bias0)
PAIRS = [("p0", (5, 3, 3, 3), False, (7, 5, 3, 3), False, True),
         ("p1", (70, 4, 1, 1), False, (6, 70, 1, 1), False, False),
         ("p2", (3, 300, 3, 3), False, (130, 3, 3, 3), False, True),
         ("p3", (10, 1, 3, 3), False, (4, 10, 1, 1), False, True),      # depthwise + conv
         ("p4", (4, 6, 3, 3), True, (6, 5, 2, 2), True, True),          # ConvTranspose2d pair
         ("p5", (6, 3, 5), False, (4, 6, 3), False, True),              # Conv1d pair
         ("p6", (6, 4, 3, 3), False, (5, 6, 3, 3), False, True)]        # special channels
SPECIAL = {"zero_row": 1, "zero_col": 2, "tiny": 3}


def main():
    rng = np.random.default_rng(20241103)
    ref = reference_functions()
    g = {}

    with np.errstate(all="ignore"):
        for name, s0, t0, s1, t1, has_bias in PAIRS:
            w0 = weight(rng, s0, 1 if t0 else 0)
            w1 = weight(rng, s1, 0 if t1 else 1)
            if name == "p6":
                w0[SPECIAL["zero_row"]] = 0
                w1[:, SPECIAL["zero_col"]] = 0
                w0[SPECIAL["tiny"]] = (rng.uniform(-1, 1, w0[0].shape) * 1e-30).astype(F)
                w1[:, SPECIAL["tiny"]] = (rng.uniform(-1, 1, w1[:, 0].shape) * 1e-30).astype(F)
                w0[SPECIAL["tiny"], 0, 0, 0] = F(1e-30)
                w1[0, SPECIAL["tiny"], 0, 0] = F(-1e-30)
            C = s0[1] if t0 else s0[0]
            b0 = (rng.standard_normal(C) * 0.3).astype(F) if has_bias else None
            a0, a1 = to4d(w0, t0), to4d(w1, t1)
            s = ref["compute_scaling_params_for_conv"](a0, a1)
            n0, n1, nb = ref["fold_scaling_params_for_conv"](a0, a1, b0, s)
            g[name + "_w0"], g[name + "_w1"] = w0, w1
            g[name + "_t"] = np.array([t0, t1], np.int32)
            g[name + "_s"] = s.astype(F)
            g[name + "_w0_out"], g[name + "_w1_out"] = from4d(n0, s0, t0), from4d(n1, s1, t1)
            if has_bias:
                g[name + "_b0"], g[name + "_b0_out"] = b0, nb.astype(F)
            assert s.dtype == F and n0.dtype == F and n1.dtype == F
        g["p6_special"] = np.array([SPECIAL["zero_row"], SPECIAL["zero_col"], SPECIAL["tiny"]], np.int32)

        # triple: conv, depthwise, conv
        w0, w1, w2 = weight(rng, (10, 6, 1, 1), 0), weight(rng, (10, 1, 3, 3), 0), weight(rng, (4, 10, 1, 1), 1)
        b0, b1 = (rng.standard_normal(10) * 0.3).astype(F), (rng.standard_normal(10) * 0.3).astype(F)
        s12, s23 = ref["compute_scaling_params_for_depthwise_conv"](w0, w1, w2)
        n0, n1, n2, nb0, nb1 = ref["fold_scaling_params_for_depthwise_conv"](w0, w1, w2, b0, b1, s12, s23)
        for k, v in dict(w0=w0, w1=w1, w2=w2, b0=b0, b1=b1, s12=s12, s23=s23, w0_out=n0, w1_out=n1, w2_out=n2,
                         b0_out=nb0, b1_out=nb1).items():
            assert v.dtype == F, k
            g["t0_" + k] = v

        # BN folds: (name, weight shape, forward, has bias)
        for name, shape, forward, has_bias in [("b0", (7, 5, 3, 3), False, True), ("b1", (9, 33), False, True),
                                               ("b2", (8, 1, 3, 3), False, True), ("b3", (6, 4, 3, 3), False, False),
                                               ("b4", (6, 5, 3, 3), True, True)]:
            w = weight(rng, shape, 0)
            n = shape[1] if forward else shape[0]
            b = (rng.standard_normal(shape[0]) * 0.3).astype(F) if has_bias else np.zeros(shape[0], F)
            gamma = np.exp(rng.uniform(np.log(0.1), np.log(3.0), n)).astype(F)
            gamma[n // 2] = -gamma[n // 2]   # one negative gamma
            beta, mu = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
            var = rng.uniform(0.2, 3.0, n).astype(F)
            eps = 1e-5
            # The reference's torch layer takes sqrt(running_var + eps) where the model lives. The IEEE
            # root (np.sqrt; the GPU's too) is used here: this torch's vectorised CPU sqrt is off by one
            # ulp on about 0.7 % of values (README_dfq.md). The sum is torch's, bit for bit.
            sigma = np.sqrt((torch.from_numpy(var) + eps).numpy())
            nw, nb = ref["batch_norm_fold"](to4d(w, False), b, gamma, beta, mu, sigma, not forward)
            assert nw.dtype == F and nb.dtype == F
            for k, v in dict(w=w, b=b, gamma=gamma, beta=beta, mu=mu, var=var, sigma=sigma, w_out=nw.reshape(shape),
                             b_out=nb).items():
                g["%s_%s" % (name, k)] = v
            g[name + "_flags"] = np.array([forward, has_bias], np.int32)
            g[name + "_eps"] = np.array(eps, np.float64)

        # HBF: (name, relu between, second weight shape); the reference gets beta / s and gamma / s
        for name, relu, shape in [("h0", True, (7, 5, 3, 3)), ("h1", False, (7, 5, 3, 3)), ("h2", True, (5, 1, 3, 3)),
                                  ("h3", False, (5, 1, 3, 3))]:
            C = 5
            w2 = weight(rng, shape, 0)
            gamma = rng.uniform(0.1, 1.0, C).astype(F)
            beta = (rng.standard_normal(C) * 2.0).astype(F)
            beta[0], beta[1] = F(4.5), F(-1.0)   # one channel that absorbs, one that does not
            s = np.exp(rng.uniform(np.log(0.3), np.log(3.0), C)).astype(F)
            b1 = (rng.standard_normal(C) * 0.3).astype(F)
            b2 = (rng.standard_normal(shape[0]) * 0.3).astype(F)
            nb1, nb2 = ref["_absorb_bias"](relu, beta / s, gamma / s, w2, b2, b1)
            assert nb1.dtype == F and nb2.dtype == F
            for k, v in dict(w2=w2, gamma=gamma, beta=beta, s=s, b1=b1, b2=b2, b1_out=nb1, b2_out=nb2).items():
                g["%s_%s" % (name, k)] = v
            g[name + "_relu"] = np.array(relu, np.int32)

    path = os.path.join(HERE, "golden_dfq.npz")
    np.savez_compressed(path, **g)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(g)))


if __name__ == "__main__":
    main()
