"""Generate tests/golden/golden_fp8.npz from the REFERENCE's FP8 functions.

The reference's definitions (aimet_torch/fp_quantization.py: fake_cast_to_ieee_float,
quantize_to_fp8, init_minmax, init_mse) are parsed from the reference file and executed at
generation time, on the CPU in float32; nothing of their text is stored. The fixture holds data
only: inputs, the reference chain's outputs, the candidate tables its init_mse built
(torch.linspace, recorded as it was called) and its init_minmax / init_mse choices, for M = 3 and
M = 2 mantissa bits, per tensor and per channel.

    python tests/golden/make_golden_fp8.py
"""
import ast
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("AIMET_REFERENCE", "/root/reference")
NAMES = ("init_minmax", "mantissa_bits_to_device", "init_mse", "quantize_to_fp8", "fake_cast_to_ieee_float")


class _RecordingTorch:
    """torch, with every linspace result kept (init_mse's candidate tables)."""

    def __init__(self):
        self.linspaces = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def linspace(self, *args, **kwargs):
        out = torch.linspace(*args, **kwargs)
        self.linspaces.append(out.clone())
        return out


def reference_functions(mantissa_bits):
    path = os.path.join(REF_ROOT, "TrainingExtensions/torch/src/python/aimet_torch/fp_quantization.py")
    tree = ast.parse(open(path).read(), path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert len(fns) == len(NAMES)
    rec = _RecordingTorch()
    ns = {"torch": rec, "np": np, "NUM_MANTISSA_BITS": mantissa_bits}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns, rec


class _Quantizer:
    def __init__(self, channel_axis):
        self.channel_axis = channel_axis
        self.fp8_maxval = None


# per-tensor cast: maxvals log-uniform in 1e-3 .. 1e4, normal-distributed elements (some clipped)
N_MAXVAL, N_PER = 16, 2048
# per-channel cast and the range-setting cases: (shape, channel axis)
CHANNEL_CASES = [((24, 40), 0), ((2, 6, 50), 1)]
SEARCH_CASES = [((4096,), None), ((12, 300), 0), ((2, 5, 64), 1)]


def main():
    rng = np.random.default_rng(20240819)
    g = {"mantissa_bits": np.array([3, 2], np.int32)}
    maxvals = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), N_MAXVAL)).astype(np.float32)
    x = (rng.standard_normal((N_MAXVAL, N_PER)) * (maxvals[:, None] / 2.5)).astype(np.float32)
    g["pt_maxval"], g["pt_x"] = maxvals, x
    for ci, (shape, axis) in enumerate(CHANNEL_CASES):
        C = shape[axis]
        mv = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), C)).astype(np.float32)
        bshape = [1] * len(shape)
        bshape[axis] = C
        g["pc%d_maxval" % ci] = mv
        g["pc%d_axis" % ci] = np.array(axis, np.int32)
        g["pc%d_x" % ci] = (rng.standard_normal(shape) * (mv.reshape(bshape) / 2.5)).astype(np.float32)
    for si, (shape, axis) in enumerate(SEARCH_CASES):
        scale = np.exp(rng.uniform(np.log(1e-2), np.log(1e2)))
        g["s%d_x" % si] = (rng.standard_normal(shape) * scale).astype(np.float32)
        g["s%d_axis" % si] = np.array(-1 if axis is None else axis, np.int32)

    for M in (3, 2):
        ns, rec = reference_functions(M)
        cast = ns["quantize_to_fp8"]
        mb = torch.Tensor([M])
        out = np.stack([cast(torch.from_numpy(x[i]), torch.tensor(float(maxvals[i])), mb).numpy()
                        for i in range(N_MAXVAL)])
        g["pt_out_m%d" % M] = out.astype(np.float32)
        for ci, (shape, axis) in enumerate(CHANNEL_CASES):
            y = cast(torch.from_numpy(g["pc%d_x" % ci]), torch.from_numpy(g["pc%d_maxval" % ci]), mb, axis)
            g["pc%d_out_m%d" % (ci, M)] = y.numpy().astype(np.float32)
        for si, (shape, axis) in enumerate(SEARCH_CASES):
            t = torch.from_numpy(g["s%d_x" % si])
            per_channel = axis is not None
            q = _Quantizer(axis if per_channel else 0)
            mm = ns["init_minmax"](t, q, per_channel)
            del rec.linspaces[:]
            best = ns["init_mse"](t, q, per_channel)
            g["s%d_minmax_m%d" % (si, M)] = np.asarray(mm.numpy(), np.float32).reshape(-1)
            g["s%d_cands_m%d" % (si, M)] = torch.stack(rec.linspaces).transpose(0, 1).numpy().astype(np.float32)
            g["s%d_best_m%d" % (si, M)] = np.asarray(best.numpy(), np.float32).reshape(-1)
    path = os.path.join(HERE, "golden_fp8.npz")
    np.savez_compressed(path, **g)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
