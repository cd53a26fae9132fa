"""Generate tests/golden/golden_bc.npz from the REFERENCE's bias-correction arithmetic.

The reference's definitions (aimet_common/bias_correction.py: empirical_bias_correction,
analytical_bias_correction) are parsed from the reference file and executed at generation time, on the
CPU; nothing of their text is stored. The fixture holds data only: inputs, the reference's float32
results, and the results of the same functions on float64 inputs (README_bc.md describes the cases
and records the distances between the two). Needs scipy.

    python tests/golden/make_golden_bc.py
"""
import ast
import enum
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
from scipy.stats import norm

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bc_oracle as O  # noqa: E402

REF_ROOT = os.environ.get("AIMET_REFERENCE", "/root/reference")
PATH = "TrainingExtensions/common/src/python/aimet_common/bias_correction.py"
NAMES = ("empirical_bias_correction", "analytical_bias_correction")
F = np.float32


class ActivationType(enum.Enum):
    no_activation = 0
    relu = 1
    relu6 = 2


def reference_functions():
    ns = {"np": np, "norm": norm, "ActivationType": ActivationType}
    path = os.path.join(REF_ROOT, PATH)
    tree = ast.parse(open(path).read(), path)
    fns = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(f.name for f in fns) == sorted(NAMES)
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns


EMPIRICAL = [(1, 1, 1, 1), (2, 3, 7, 7), (3, 5, 1, 1), (2, 70, 5, 3), (4, 2, 56, 56), (257, 130, 1, 1)]
# (name, module weight shape, transposed, coded): a coded weight is stored as int8 (w = code / 16) with
# int8 4-bit codes and a delta for its quantized values, to keep the fixture small
ANALYTICAL = [("a0", (7, 5, 3, 3), False, False), ("a1", (9, 33), False, False), ("a2", (8, 1, 3, 3), False, False),
              ("a3", (130, 300, 3, 3), False, True), ("a4", (4, 6, 2, 2), True, False)]
ACTS = ("none", "relu", "relu6")


def qdq4(w):
    """Symmetric signed 4-bit quantize-dequantize of the whole tensor: (codes, delta)."""
    delta = F(np.abs(w).max() / F(7.0))
    q = np.clip(np.round(w / delta), -8, 7)
    return q.astype(np.int8), delta


def to4d(w, transposed):
    w = w.reshape(w.shape + (1,) * (4 - w.ndim))
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3)) if transposed else w


def ulps32(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / (2 * O.half_ulp32(b))))


def main():
    rng = np.random.default_rng(20241120)
    ref = reference_functions()
    g, report = {}, []

    emp_dist = 0.0
    for n, shape in enumerate(EMPIRICAL):
        N, C, H, W = shape
        x = (rng.standard_normal(shape) * rng.uniform(0.2, 3.0, (1, C, 1, 1)) + rng.standard_normal((1, C, 1, 1))).astype(F)
        # the quantized output is stored as its float16 distance from the reference output: q = ref + qdiff
        qdiff = (rng.standard_normal(shape) * 0.05 + rng.standard_normal((1, C, 1, 1)) * 0.1).astype(np.float16)
        q = x + qdiff.astype(F)
        bias = (rng.standard_normal(C) * 0.3).astype(F)
        out = ref["empirical_bias_correction"](x, q, bias)
        out64 = ref["empirical_bias_correction"](x.astype(np.float64), q.astype(np.float64), bias.astype(np.float64))
        assert out.dtype == F and out64.dtype == np.float64
        rs, _ = O.channel_sums(x.reshape(N, C, H * W))
        qs, _ = O.channel_sums(q.reshape(N, C, H * W))
        _, mine = O.apply_empirical(bias, rs, qs, N * H * W)
        d = float(np.abs(out.astype(np.float64) - out64).max())
        emp_dist = max(emp_dist, d)
        g["e%d_dist" % n] = np.array(d)
        report.append(("e%d %s" % (n, shape), d, ulps32(out, out64), float(np.abs(mine - out).max()),
                       float(np.abs(mine - out64).max())))
        for k, v in dict(ref=x, qdiff=qdiff, bias=bias, out=out, out64=out64).items():
            g["e%d_%s" % (n, k)] = v
    g["emp_dist"] = np.array(emp_dist)

    ana_dist = 0.0
    with np.errstate(all="ignore"):
        for name, shape, transposed, coded in ANALYTICAL:
            if coded:
                code = rng.integers(-15, 16, shape).astype(np.int8)
                w = code.astype(F) / F(16.0)
                g[name + "_wcode"] = code
            else:
                w = (rng.standard_normal(shape) * 0.2).astype(F)
                g[name + "_w"] = w
            qc, delta = qdq4(w)
            wq = qc.astype(F) * delta
            g[name + "_qcode"], g[name + "_delta"] = qc, np.array(delta, F)
            v = to4d(w, transposed)
            cout, cin = v.shape[0], v.shape[1]
            nch = cout if cin == 1 else cin
            gamma = np.exp(rng.uniform(np.log(0.1), np.log(3.0), nch)).astype(F)
            beta = (rng.standard_normal(nch) * 1.5).astype(F)
            gamma[nch // 2] = -gamma[nch // 2]      # one negative gamma
            gamma[nch // 3] = F(0.0)                # one gamma == 0 with beta != 0
            beta[nch // 3] = F(0.75) if nch % 2 else F(-0.75)
            bias = (rng.standard_normal(cout) * 0.3).astype(F)
            g[name + "_gamma"], g[name + "_beta"], g[name + "_bias"] = gamma, beta, bias
            g[name + "_zero"] = np.array(nch // 3, np.int32)
            g[name + "_t"] = np.array(transposed, np.int32)
            # float64 evaluation: the reference's formula on the fp32-rounded differences
            diff32 = (to4d(wq, transposed) - v).astype(F)
            for a, act in enumerate(ACTS):
                out = ref["analytical_bias_correction"](v, to4d(wq, transposed), bias, beta, gamma, ActivationType(a))
                out64 = ref["analytical_bias_correction"](np.zeros(v.shape), diff32.astype(np.float64),
                                                          bias.astype(np.float64), beta.astype(np.float64),
                                                          gamma.astype(np.float64), ActivationType(a))
                _, mine, _ = O.analytical(w, wq, bias, gamma, beta, a, transposed)
                d = float(np.abs(np.asarray(out, np.float64) - out64).max())
                ana_dist = max(ana_dist, d)
                g["%s_dist_%s" % (name, act)] = np.array(d)
                report.append(("%s %s %s" % (name, shape, act), d, ulps32(out, out64),
                               float(np.abs(mine - np.asarray(out, np.float64)).max()),
                               float(np.abs(mine - out64).max())))
                g["%s_out_%s" % (name, act)] = np.asarray(out, np.float64)
                g["%s_out64_%s" % (name, act)] = np.asarray(out64, np.float64)
    g["ana_dist"] = np.array(ana_dist)

    path = os.path.join(HERE, "golden_bc.npz")
    np.savez_compressed(path, **g)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(g)))
    print("| case | golden vs float64 (abs) | golden vs float64 (fp32 ulp) | oracle vs golden (abs) | oracle vs float64 (abs) |")
    print("|---|---|---|---|---|")
    for r in report:
        print("| %s | %.3e | %.2f | %.3e | %.3e |" % r)
    print("emp_dist %.3e ana_dist %.3e" % (emp_dist, ana_dist))


if __name__ == "__main__":
    main()
