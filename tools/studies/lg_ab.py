"""A/B of two builds of libaimet_amd.so on the learned-grid kernels, in one process on one MI355X:
the two libraries alternate, 7 rounds after one warm round, each round the mean of 10 launches
between HIP events; accept when new median <= parent median + parent spread (max - min of the
parent's rounds). Every output of a row (y, grad_x, sums, range gradients) is compared bit for bit
between the two libraries.

Rows: benchmarks/kernel_roofline.py's learned-grid forward / backward (2^28 elements, C = 4096),
benchmarks/lg16_roofline.py's forward / backward at its Llama-3-8B call sizes, aimet_lg_backward_grad16
on two weight shapes, the per-tensor float32 backward, the channel x slice form and the scalar
channel form.

usage: python tools/studies/lg_ab.py --parent PATH/libaimet_amd.so [--only SUBSTR] > lg_ab.txt"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

ROUNDS, LAUNCHES = 7, 10


def load(path):
    from aimet_amd import _native
    lib = ctypes.CDLL(path)
    for name, args in _native._PROTOTYPES.items():
        if name.startswith("aimet_lg_"):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, ctypes.c_int
    lib.aimet_last_error.restype = ctypes.c_char_p
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    from aimet_amd import _native
    from aimet_amd.learned_grid import _RangeSpec, num_steps_of
    libs = {"parent": load(args.parent), "new": load(_native.LIB_PATH)}
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(0)
    f = ctypes.c_float
    slower = []

    def ok(lib, rc):
        if rc != 0:
            raise RuntimeError(lib.aimet_last_error().decode())

    def ab(name, nbytes, launch, outputs):
        """launch(lib): one call; outputs: the tensors it writes."""
        if args.only not in name:
            return
        snap = {}
        for tag, lib in libs.items():
            for t in outputs:
                t.fill_(float("nan")) if t.dtype.is_floating_point else t.zero_()
            launch(lib)
            stream.synchronize()
            snap[tag] = [t.clone() for t in outputs]
        same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(snap["parent"], snap["new"]))
        times = {"parent": [], "new": []}
        for rnd in range(ROUNDS + 1):
            for tag, lib in libs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(LAUNCHES):
                    launch(lib)
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
        if verdict != "ok" or not same:
            slower.append(name)
        print("  new - parent = %+.4f ms (%+.2f %%), parent spread %.4f: %s; outputs bit-identical: %s\n" % (
            med["new"] - med["parent"], 100 * (med["new"] - med["parent"]) / med["parent"], spread, verdict, same),
            flush=True)

    def encodings(emin, emax, bw, sym):
        d, o = torch.empty_like(emin), torch.empty_like(emin)
        ok(libs["parent"], libs["parent"].aimet_lg_encodings(P(emin), P(emax), emin.numel(), bw, int(sym), 0, 0, P(d),
                                                             P(o), sp))
        return d, o, num_steps_of(bw, sym, False)

    def spec_of(emin, emax, delta, sym):
        gmin, gmax = torch.empty_like(emin), torch.empty_like(emin)
        spec = _RangeSpec(emin.data_ptr(), emax.data_ptr(), delta.data_ptr(), gmin.data_ptr(), gmax.data_ptr(),
                          int(sym))
        return spec, gmin, gmax

    def fp32_backward(name, outer, C, K, sym, with_spec=True, bw=8):
        n = outer * C * K
        x = torch.randn(n, device=dev, generator=gen) * 2 + 0.3
        gr = torch.randn(n, device=dev, generator=gen)
        gx = torch.empty_like(x)
        c = torch.arange(C, device=dev)
        emax = 3.0 + (c % 5) * 0.2
        emin = -emax if sym else -2.5 - (c % 7) * 0.1
        delta, offset, steps = encodings(emin, emax, bw, sym)
        sums = torch.empty(3 * C, device=dev)
        spec, gmin, gmax = spec_of(emin, emax, delta, sym)
        ab(name, 12 * n,
           lambda lib: ok(lib, lib.aimet_lg_backward(P(x), P(gr), P(gx), P(sums), outer, C, K, P(delta), P(offset),
                                                     f(steps), ctypes.byref(spec) if with_spec else None, sp)),
           [gx, sums] + ([gmin, gmax] if with_spec else []))

    # benchmarks/kernel_roofline.py: learned_grid_forward / learned_grid_backward at its defaults
    N, C = 1 << 28, 4096
    K = N // C
    x = torch.randn(N, device=dev, generator=gen) * 2 + 0.3
    y = torch.empty_like(x)
    c = torch.arange(C, device=dev)
    delta, offset, steps = encodings(-2.5 - (c % 7) * 0.1, 3.0 + (c % 5) * 0.2, 8, False)
    ab("kernel_roofline aimet_lg_forward 2^28 C=4096", 8 * N,
       lambda lib: ok(lib, lib.aimet_lg_forward(P(x), P(y), 1, C, K, P(delta), P(offset), f(steps), sp)), [y])
    del x, y
    fp32_backward("kernel_roofline aimet_lg_backward 2^28 C=4096 (no range spec)", 1, C, K, False, with_spec=False)

    # benchmarks/lg16_roofline.py: bf16, 16-bit grid, asymmetric range gradients
    for label, n in (("seq2048x4096", 2048 * 4096), ("mean_call", 13_688_832), ("seq2048x14336", 2048 * 14336),
                     ("seq2048x1024", 2048 * 1024)):
        x = (torch.randn(n, device=dev, generator=gen) * 1.3 + 0.1).to(torch.bfloat16)
        gr = torch.randn(n, device=dev, generator=gen).to(torch.bfloat16)
        y, gx = torch.empty_like(x), torch.empty_like(x)
        emin, emax = torch.tensor([-4.1], device=dev), torch.tensor([4.7], device=dev)
        enc = torch.empty(4, 1, device=dev)
        sums = torch.empty(3, device=dev)
        steps = num_steps_of(16, False, False)
        ab("lg16_roofline forward_16_range %s" % label, 4 * n,
           lambda lib: ok(lib, lib.aimet_lg_forward_16_range(P(x), P(y), n, 2, P(emin), P(emax), 16, 0, 0, 0, P(enc[0]),
                                                             P(enc[1]), P(enc[2]), sp)), [y, enc])
        stream.synchronize()
        spec, gmin, gmax = spec_of(enc[2], enc[3], enc[0], False)
        ab("lg16_roofline backward_16 %s" % label, 6 * n,
           lambda lib: ok(lib, lib.aimet_lg_backward_16(P(x), P(gr), P(gx), P(sums), n, 2, P(enc[0]), P(enc[1]),
                                                        f(steps), ctypes.byref(spec), sp)), [gx, sums, gmin, gmax])

    # aimet_lg_backward_grad16: float32 weight, bf16 gradient, symmetric 4-bit range
    for Cw, Kw in ((4096, 4096), (1024, 14336)):
        n = Cw * Kw
        x = torch.randn(n, device=dev, generator=gen) * 0.02
        gr = torch.randn(n, device=dev, generator=gen).to(torch.bfloat16)
        gx = torch.empty_like(x)
        emax = x.view(Cw, Kw).abs().amax(dim=1) * 0.8
        emin = -emax
        delta, offset, steps = encodings(emin, emax, 4, True)
        sums = torch.empty(3 * Cw, device=dev)
        spec, gmin, gmax = spec_of(emin, emax, delta, True)
        ab("aimet_lg_backward_grad16 %dx%d bf16 gradient" % (Cw, Kw), 10 * n,
           lambda lib: ok(lib, lib.aimet_lg_backward_grad16(P(x), P(gr), P(gx), P(sums), 1, Cw, Kw, 2, P(delta),
                                                            P(offset), f(steps), ctypes.byref(spec), sp)),
           [gx, sums, gmin, gmax])

    fp32_backward("aimet_lg_backward C=1 2^26 (per tensor)", 1, 1, 1 << 26, False)
    fp32_backward("aimet_lg_backward (3, 16, 1000000) channel x slice form", 3, 16, 1000000, False)
    fp32_backward("aimet_lg_backward (4096, 96, 21) scalar channel form", 4096, 96, 21, True)
    print("rows slower or not bit-identical: %s" % (slower or "none"))


if __name__ == "__main__":
    main()
