"""The sigmoid and tanh of the fused recurrent step against torch's CPU functions, over every float32.

    python tools/studies/rnn_math_sweep.py [--out profiles/r16/rnn_math_sweep.txt] [--procs 8]

aimet_amd/csrc/rnn_math.hpp is compiled for the host (rnn_math_host.cpp, -ffp-contract=off) and
evaluated on all 2^32 bit patterns in chunks of 2^24; each chunk is compared with torch.sigmoid /
torch.tanh on the CPU:
  * the largest ulp distance over the finite inputs whose torch result is a normal number;
  * the largest absolute error over all inputs that are not NaN (the infinities included);
  * that a NaN input gives a NaN;
  * on every 257th element of the chunk, that the numpy restatement of the header
    (tests/rnn_oracle.py) gives the header's bits.
The last line of the output is one JSON object; tests/test_rnn.py reads the maxima from it.
"""
import argparse
import ctypes
import json
import multiprocessing
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
CHUNK = 1 << 24
SAMPLE = 257


def build(tmp):
    so = os.path.join(tmp, "rnn_math_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(REPO, "aimet_amd", "csrc"),
                    "-o", so, os.path.join(REPO, "tools", "studies", "rnn_math_host.cpp")], check=True)
    return so


def sweep_chunks(args):
    so, chunks = args
    import torch
    import rnn_oracle as O
    torch.set_num_threads(1)
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    res = {}
    for name, native, restated, ref in (("sigmoid", lib.rnn_sigmoid_many, O.sigmoid_r, torch.sigmoid),
                                        ("tanh", lib.rnn_tanh_many, O.tanh_r, torch.tanh)):
        native.argtypes = [fp, fp, ctypes.c_int64]
        native.restype = None
        r = dict(max_ulp=0, max_ulp_at=0, max_abs=0.0, max_abs_at=0, nan_ok=True, restated_equal=True, compared=0)
        for ch in chunks:
            x = (np.arange(CHUNK, dtype=np.uint64) + np.uint64(ch * CHUNK)).astype(np.uint32).view(np.float32)
            y = np.empty_like(x)
            native(x.ctypes.data_as(fp), y.ctypes.data_as(fp), x.size)
            want = ref(torch.from_numpy(x)).numpy()
            nan = np.isnan(x)
            r["nan_ok"] &= bool(np.isnan(y[nan]).all()) and not bool(np.isnan(y[~nan]).any())
            with np.errstate(all="ignore"):
                err = np.where(nan, 0.0, np.abs(y.astype(np.float64) - want.astype(np.float64)))
            k = int(err.argmax())
            if err[k] > r["max_abs"]:
                r["max_abs"], r["max_abs_at"] = float(err[k]), int(x.view(np.uint32)[k])
            normal = np.isfinite(x) & np.isfinite(want) & (np.abs(want) >= np.float32(2.0 ** -126))
            d = np.where(normal, O.ulp_distance(y, want), 0)
            k = int(d.argmax())
            if d[k] > r["max_ulp"]:
                r["max_ulp"], r["max_ulp_at"] = int(d[k]), int(x.view(np.uint32)[k])
            r["compared"] += int(normal.sum())
            s = x[::SAMPLE]
            got = restated(s)
            same = (O.bits(got) == O.bits(y[::SAMPLE])) | (np.isnan(got) & np.isnan(y[::SAMPLE]))
            r["restated_equal"] &= bool(same.all())
        res[name] = r
    return res


def merge(parts):
    out = {}
    for name in ("sigmoid", "tanh"):
        rs = [p[name] for p in parts]
        u = max(rs, key=lambda r: r["max_ulp"])
        a = max(rs, key=lambda r: r["max_abs"])
        out[name] = dict(max_ulp=u["max_ulp"], max_ulp_at="0x%08x" % u["max_ulp_at"], max_abs=a["max_abs"],
                         max_abs_at="0x%08x" % a["max_abs_at"], nan_ok=all(r["nan_ok"] for r in rs),
                         restated_equal=all(r["restated_equal"] for r in rs),
                         compared=sum(r["compared"] for r in rs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--chunks", type=int, default=256, help="fewer than 256: a partial sweep, for a trial run")
    a = ap.parse_args()
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        so = build(tmp)
        ids = list(range(0, 256, 256 // a.chunks))
        jobs = [(so, ids[i::a.procs]) for i in range(a.procs)]
        with multiprocessing.get_context("spawn").Pool(a.procs) as pool:
            res = merge(pool.map(sweep_chunks, jobs))
    lines = ["rnn_math.hpp against torch %s CPU sigmoid / tanh, %d chunks of 2^24 float32 bit patterns" %
             (torch.__version__, len(ids))]
    for name, r in res.items():
        lines.append("%-8s max ulp distance %d at input bits %s (over %d finite inputs with a normal result); "
                     "max abs error %.6g at %s; NaN -> NaN: %s; numpy restatement equal on every %dth input: %s"
                     % (name, r["max_ulp"], r["max_ulp_at"], r["compared"], r["max_abs"], r["max_abs_at"],
                        r["nan_ok"], SAMPLE, r["restated_equal"]))
    lines.append(json.dumps({"torch": torch.__version__, "chunks": len(ids), **res}, sort_keys=True))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
