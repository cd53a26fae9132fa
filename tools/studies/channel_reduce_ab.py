"""A/B of two builds of libaimet_amd.so on the channel reductions (csrc/channel_reduce.hpp:
aimet_bc_channel_sums, aimet_bnre_forward in its streaming and resident forms), in one process on one
MI355X; tools/studies/lg_ab.py's scheme.

1. Bit identity. Every shape of the PLANAR / INTERLEAVED / UNALIGNED lists of
   tests/test_bias_correction_gpu.py and tests/test_bn_reestimation_gpu.py, the base 0 and 1 float
   past a 16-byte boundary: `acc` of the channel sums; y, sum_mean and sum_var of the forward,
   streaming and (up to 15872 elements a channel) resident. The inputs are the test files' data()
   generators. For a moved addition to be visible the sums must depend on their order: for every
   shape with more than 300 elements a channel the float64 sum taken in index order and in reverse
   order (of x for the channel sums, of x - K and (x - K)^2 for the moments) is required to differ in
   at least one channel; an input that does not is multiplied by random powers of two until it does.
2. Timing. The two libraries alternate, 7 rounds after one warm round, each round the mean of 10
   launches between HIP events; consecutive launches read different copies of the input, spread over
   768 MiB (at most 64 copies), so that they come from HBM. Accept when new median <= parent median +
   parent spread (max - min of the parent's rounds).

usage: python tools/studies/channel_reduce_ab.py --parent PATH/libaimet_amd.so [--only SUBSTR] [--skip-timing]"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

ROUNDS, LAUNCHES = 7, 10
POOL_BYTES, MAX_COPIES = 768 << 20, 64
RESIDENT_MAX_N = 15872
STREAMING, RESIDENT = 1, 2


def load(path, prefixes=("aimet_bc_", "aimet_bnre_")):
    from aimet_amd import _native
    lib = ctypes.CDLL(path)
    for name, args in _native._PROTOTYPES.items():
        if name.startswith(prefixes):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, ctypes.c_int
    lib.aimet_last_error.restype = ctypes.c_char_p
    return lib


def ok(lib, rc):
    if rc != 0:
        raise RuntimeError(lib.aimet_last_error().decode())


def alternate(libs, stream, name, nbytes, launch, bad):
    """The timing rule: launch(lib, i) is one call on input copy i; the libraries of `libs` ("parent", "new")
    alternate, ROUNDS rounds after one warm round. A row that is slower is appended to `bad`."""
    times = {"parent": [], "new": []}
    turn = 0
    for rnd in range(ROUNDS + 1):
        for tag, lib in libs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(LAUNCHES):
                launch(lib, turn)
                turn += 1
            e1.record(stream)
            e1.synchronize()
            if rnd > 0:
                times[tag].append(e0.elapsed_time(e1) / LAUNCHES)
    print(name)
    med = {}
    for tag in ("parent", "new"):
        t = times[tag]
        med[tag] = statistics.median(t)
        print("  %-7s %s  median %.4f ms  %.1f GB/s  spread %.4f" % (
            tag, " ".join("%.4f" % v for v in t), med[tag], nbytes / (med[tag] * 1e-3) / 1e9, max(t) - min(t)))
    spread = max(times["parent"]) - min(times["parent"])
    verdict = "ok" if med["new"] <= med["parent"] + spread else "SLOWER"
    if verdict != "ok":
        bad.append(name)
    print("  new - parent = %+.4f ms (%+.2f %%), parent spread %.4f: %s\n" % (
        med["new"] - med["parent"], 100 * (med["new"] - med["parent"]) / med["parent"], spread, verdict), flush=True)


def sequential_sums(v):
    """Per row of v [C][n]: the float64 sum in index order (np.sum adds pairwise)."""
    return np.add.accumulate(v, axis=1)[:, -1]


def order_sensitive(x, shifted):
    C = x.shape[1]
    v = np.moveaxis(x.astype(np.float64), 1, 0).reshape(C, -1)
    terms = [v]
    if shifted:
        d = v - v[:, :1]
        terms = [d, d * d]
    return all(np.any(sequential_sums(t) != sequential_sums(t[:, ::-1])) for t in terms)


def sensitive_input(make, shape, seed, shifted):
    """(data()'s input, widened if need be; how many times it was widened)"""
    x, rng, widened = make(shape, seed), np.random.default_rng(seed), 0
    if shape[0] * shape[2] > 300:
        while not order_sensitive(x, shifted):
            x = (x * np.exp2(rng.integers(-4, 5, x.shape))).astype(np.float32)
            widened += 1
    return x, widened


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    from aimet_amd import _native
    import test_bias_correction_gpu as TB
    import test_bn_reestimation_gpu as TR
    libs = {"parent": load(args.parent), "new": load(_native.LIB_PATH)}
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    bad = []

    def set_form(form):
        for lib in libs.values():
            ok(lib, lib.aimet_bnre_forward_form(form, None))

    def at_offset(a, off):
        """A device copy of `a` whose first float is `off` floats past a 16-byte boundary."""
        buf = torch.empty(a.size + 8, dtype=torch.float32, device=dev)
        skip = (-buf.data_ptr() % 16) // 4 + off
        view = buf[skip:skip + a.size]
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        assert view.data_ptr() % 16 == 4 * off
        return view

    def channel_sums(lib, x, shape):
        acc = torch.zeros(shape[1], dtype=torch.float64, device=dev)
        ok(lib, lib.aimet_bc_channel_sums(P(x), shape[0], shape[1], shape[2], P(acc), sp))
        return [acc]

    def forward(lib, x, shape, gamma, beta, off):
        C = shape[1]
        y = at_offset(np.zeros(x.numel(), np.float32), off)
        sums = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        ok(lib, lib.aimet_bnre_forward(P(x), shape[0], C, shape[2], P(gamma), P(beta), 1e-5, P(y), P(sums[:C]),
                                       P(sums[C:]), sp))
        return [y, sums]

    def identical(outs):
        stream.synchronize()
        return all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs["parent"], outs["new"]))

    # ---- 1. bit identity ----------------------------------------------------------------------------
    shapes = []
    for s in (TB.PLANAR + [(r, c, 1) for r, c in TB.INTERLEAVED] + TR.PLANAR + [(r, c, 1) for r, c in TR.INTERLEAVED]
              + TR.UNALIGNED):
        if s not in shapes:
            shapes.append(s)
    print("1. Bit identity, parent against new (%d shapes x base offsets 0 and 1 float)" % len(shapes))
    print("%-16s %3s  %-22s %-30s %-30s %s" % ("shape", "off", "aimet_bc_channel_sums", "aimet_bnre_forward streaming",
                                              "aimet_bnre_forward resident", "inputs order-sensitive"))
    for shape in shapes:
        name = "x".join(map(str, shape))
        if args.only not in name:
            continue
        n = shape[0] * shape[2]
        xb, wb = sensitive_input(TB.data, shape, sum(shape), False)
        xr, wr = sensitive_input(TR.data, shape, sum(shape), True)
        if n > 300:
            note = "yes" + (" (widened %d / %d times)" % (wb, wr) if wb or wr else "")
        else:
            note = "not required (n = %d)" % n
        gamma, beta = (torch.from_numpy(v).to(dev) for v in TR.affine(shape[1], sum(shape)))
        for off in (0, 1):
            row = []
            x = at_offset(xb, off)
            row.append(identical({tag: channel_sums(lib, x, shape) for tag, lib in libs.items()}))
            x = at_offset(xr, off)
            for form, fits in ((STREAMING, n >= 2), (RESIDENT, 2 <= n <= RESIDENT_MAX_N)):
                if not fits:
                    row.append(None)
                    continue
                set_form(form)
                row.append(identical({tag: forward(lib, x, shape, gamma, beta, off) for tag, lib in libs.items()}))
            set_form(0)
            words = ["-" if r is None else ("identical" if r else "DIFFERENT") for r in row]
            if False in row:
                bad.append("%s off %d" % (name, off))
            print("%-16s %3d  %-22s %-30s %-30s %s" % (name, off, words[0], "y, sum_mean, sum_var " + words[1],
                                                      "y, sum_mean, sum_var " + words[2], note), flush=True)
    print("rows with a differing bit: %s\n" % (bad or "none"))
    if args.skip_timing:
        return 1 if bad else 0

    # ---- 2. timing ----------------------------------------------------------------------------------
    print("2. Timing: ms per call, %d rounds after one warm round, each the mean of %d launches between HIP events;\n"
          "   accept: new median <= parent median + parent spread (max - min of the parent's rounds)" % (ROUNDS, LAUNCHES))
    gen = torch.Generator(device=dev).manual_seed(0)

    def ab(name, nbytes, launch):
        if args.only in name:
            alternate(libs, stream, name, nbytes, launch, bad)

    def copies_of(shape):
        """[copies][numel] random floats, every copy 16-byte aligned"""
        numel = shape[0] * shape[1] * shape[2]
        pitch = (numel + 3) // 4 * 4
        count = max(2, min(MAX_COPIES, POOL_BYTES // (4 * pitch)))
        pool = torch.randn(count, pitch, device=dev, generator=gen) * 1.5 + 0.25
        return pool, count

    def time_sums(shape):
        pool, count = copies_of(shape)
        acc = torch.zeros(shape[1], dtype=torch.float64, device=dev)
        ab("aimet_bc_channel_sums %s (%d copies)" % ("x".join(map(str, shape)), count), 4 * pool[0].numel(),
           lambda lib, i: ok(lib, lib.aimet_bc_channel_sums(P(pool[i % count]), shape[0], shape[1], shape[2], P(acc), sp)))

    def time_forward(shape, form):
        pool, count = copies_of(shape)
        C = shape[1]
        y = torch.empty_like(pool[0])
        sums = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        gamma, beta = torch.rand(C, device=dev, generator=gen) + 0.5, torch.randn(C, device=dev, generator=gen)
        set_form(form)
        ab("aimet_bnre_forward %s %s (%d copies)" % ("streaming" if form == STREAMING else "resident",
                                                     "x".join(map(str, shape)), count),
           (12 if form == STREAMING else 8) * pool[0].numel(),
           lambda lib, i: ok(lib, lib.aimet_bnre_forward(P(pool[i % count]), shape[0], C, shape[2], P(gamma), P(beta),
                                                         1e-5, P(y), P(sums[:C]), P(sums[C:]), sp)))
        set_form(0)

    for shape in ((32, 64, 112 * 112), (32, 2048, 49), (32, 1000, 1)):
        time_sums(shape)
    for shape in ((32, 64, 112 * 112), (32, 512, 28 * 28), (32, 2048, 49), (32, 1000, 1)):
        time_forward(shape, STREAMING)
    for shape in ((32, 1024, 14 * 14), (32, 2048, 49), (32, 1000, 1)):
        time_forward(shape, RESIDENT)
    print("rows slower or not bit-identical: %s" % (bad or "none"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
