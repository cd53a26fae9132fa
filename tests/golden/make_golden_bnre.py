"""Generate tests/golden/golden_bnre.npz: BatchNorm re-estimation and BN fold to scale.

The reference's `reestimate_bn_stats` (aimet_torch/bn_reestimation.py) with the helpers it calls
(`in_eval_mode`, `in_train_mode`, `_in_mode` of aimet_torch/utils.py, `Handle` of
aimet_common/utils.py) is parsed from the reference files and executed at generation time, on the
CPU in float32; nothing of its text is stored. The package itself is not imported: its __init__
pulls in the compiled libpymo. The fixture holds data only (tests/golden/README_bnre.md).

    python tests/golden/make_golden_bnre.py
"""
import ast
import contextlib
import itertools
import os
import sys
from typing import Any, Callable, Iterable, List, Union

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bnre_oracle as O  # noqa: E402

REF_ROOT = os.environ.get("AIMET_REFERENCE", "/root/reference")
SOURCES = {"TrainingExtensions/common/src/python/aimet_common/utils.py": ("Handle",),
           "TrainingExtensions/torch/src/python/aimet_torch/utils.py": ("in_eval_mode", "in_train_mode", "_in_mode"),
           "TrainingExtensions/torch/src/python/aimet_torch/bn_reestimation.py":
               ("_get_active_bn_modules", "_for_each_module", "_reset_bn_stats", "_reset_momentum",
                "reestimate_bn_stats")}
F = np.float32


def reference_functions():
    ns = {"torch": torch, "itertools": itertools, "contextlib": contextlib, "Union": Union, "Iterable": Iterable,
          "List": List, "Callable": Callable, "Any": Any, "DataLoader": torch.utils.data.DataLoader,
          "_BatchNorm": torch.nn.modules.batchnorm._BatchNorm, "DEFAULT_NUM_BATCHES": 100,
          "tqdm": lambda it, **_: it}
    for rel, names in SOURCES.items():
        path = os.path.join(REF_ROOT, rel)
        tree = ast.parse(open(path).read(), path)
        defs = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
        assert sorted(d.name for d in defs) == sorted(names), [d.name for d in defs]
        exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


def weight(rng, shape):
    w = rng.standard_normal(shape)
    r = np.exp(rng.uniform(np.log(0.05), np.log(2.0), shape[0]))
    return (w * r.reshape((-1,) + (1,) * (len(shape) - 1))).astype(F)


def main():
    rng = np.random.default_rng(20250215)
    ref = reference_functions()
    g = {}

    # the network: seeded parameters, drifted starting statistics, one negative gamma per BatchNorm
    net = O.TinyNet()
    state = {}
    for name, t in net.state_dict().items():
        shape = tuple(t.shape)
        if name.endswith("num_batches_tracked"):
            v = np.array(7, np.int64)
        elif name.endswith("running_var"):
            v = rng.uniform(0.3, 2.0, shape).astype(F)
        elif name.endswith("running_mean"):
            v = rng.standard_normal(shape).astype(F)
        elif ".weight" in name and len(shape) == 1:          # gamma
            v = np.exp(rng.uniform(np.log(0.2), np.log(2.0), shape)).astype(F)
            v[shape[0] // 2] = -v[shape[0] // 2]
        elif len(shape) == 1:                                 # biases and betas
            v = (rng.standard_normal(shape) * 0.3).astype(F)
        else:
            v = weight(rng, shape)
        state[name] = v
        g["param_" + name] = v
    g["batches"] = (rng.standard_normal((3, 4, 3, 8, 8)) * 1.5 + 0.25).astype(F)

    # the reference's own reestimate_bn_stats on the CPU
    net = O.tiny_net(g)
    batches = O.tiny_batches(g)
    handle = ref["reestimate_bn_stats"](net, batches, num_batches=100)
    for n in O.BN_NAMES:
        bn = getattr(net, n)
        g["ref_%s_mean" % n] = bn.running_mean.numpy().copy()
        g["ref_%s_var" % n] = bn.running_var.numpy().copy()
        g["ref_%s_tracked" % n] = bn.num_batches_tracked.numpy().copy()
    handle.remove()
    for n in O.BN_NAMES:   # the handle restores what the fixture started from
        assert np.array_equal(getattr(net, n).running_mean.numpy(), g["param_%s.running_mean" % n])
    # the restatement used on the device agrees with it bit for bit here
    twin = O.tiny_net(g)
    O.reestimate_torch(twin, batches)
    for n in O.BN_NAMES:
        assert np.array_equal(getattr(twin, n).running_mean.numpy(), g["ref_%s_mean" % n]), n
        assert np.array_equal(getattr(twin, n).running_var.numpy(), g["ref_%s_var" % n]), n

    # fold to scale: the two conv -> bn pairs, asymmetric per-channel ranges around each channel's weights
    for k, (conv, bn) in enumerate((("conv1", "bn1"), ("conv2", "bn2"))):
        w = g["param_%s.weight" % conv]
        cout = w.shape[0]
        b = g.get("param_%s.bias" % conv, np.zeros(cout, F))
        flat = w.reshape(cout, -1)
        enc_min = (flat.min(axis=1) * rng.uniform(0.9, 1.1, cout)).astype(F)
        enc_max = (flat.max(axis=1) * rng.uniform(0.9, 1.1, cout)).astype(F)
        gamma, beta = g["param_%s.weight" % bn], g["param_%s.bias" % bn]
        mean, var = g["ref_%s_mean" % bn], g["ref_%s_var" % bn]
        assert (gamma < 0).sum() == 1
        w_out, b_out, new_min, new_max, bad = O.fold_scale(w, b, gamma, beta, mean, var, 1e-5, enc_min, enc_max)
        assert not bad
        for key, v in dict(w=w, b=b, gamma=gamma, beta=beta, mean=mean, var=var, enc_min=enc_min, enc_max=enc_max,
                           w_out=w_out, b_out=b_out, min_out=new_min, max_out=new_max).items():
            assert v.dtype == F, key
            g["fs%d_%s" % (k, key)] = v
        g["fs%d_eps" % k] = np.array(1e-5, np.float64)

    path = os.path.join(HERE, "golden_bnre.npz")
    np.savez_compressed(path, **g)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(g)))


if __name__ == "__main__":
    main()
