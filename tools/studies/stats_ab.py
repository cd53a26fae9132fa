"""A/B of two builds of libaimet_amd.so on the statistics kernels (csrc/stats.hip: aimet_tq_update_stats,
aimet_tq_update_stats_many, aimet_tq_update_stats_channels_many, aimet_tq_reset_encoding_stats_many), in
one process on one MI355X; the scheme, the loader and the timing rule of tools/studies/channel_reduce_ab.py.

1. Bit identity. The shapes of the statistics tests of tests/test_gpu_parity.py: per-tensor quantizers of
   every scheme from 1 to 2^24 + 3 elements (4-byte offset views, an all-zero first batch, NaN / inf,
   values next to bin edges), single and batched, 70 TF-Enhanced quantizers through the walking min/max
   pass with unset ranges between fixed ones; per-channel quantizers of every scheme over ragged shapes,
   channel axes 0 and 1, all-zero channels, 65536 + 3 channels, single and batched; a reset in between.
   After every batch the quantizers' device state is read back and compared field by field: minmax,
   acc, pdf_init, iterations, hist_min, bucket_size, bin_bucket, bin_offset, active, pdf, counts. The
   fields are found through a ctypes mirror of aimet_tensor_quantizer (csrc/tq_internal.hpp), which is
   the same in both builds.
2. Timing. channel_reduce_ab.alternate: the two libraries alternate, 7 rounds after one warm round, each
   the mean of 10 launches between HIP events; the inputs of consecutive launches rotate over more than
   512 MiB. Accept when new median <= parent median + parent spread.

usage: python tools/studies/stats_ab.py --parent PATH/libaimet_amd.so [--only SUBSTR] [--skip-timing]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from channel_reduce_ab import MAX_COPIES, alternate, load, ok   # noqa: E402

TF, TFE, PERCENTILE, MSE, ENTROPY = 0, 1, 3, 4, 5
SCHEMES = {"tf": TF, "tfe": TFE, "percentile": PERCENTILE, "mse": MSE, "entropy": ENTROPY}
MM_TILE = 256 * 16          # kMmTile
POOL_BYTES = 640 << 20      # inputs of consecutive launches rotate over at least this much
_vp, _i64 = ctypes.c_void_p, ctypes.c_int64


class TqDevice(ctypes.Structure):
    """csrc/tq_state.hpp; (bytes per channel, compared) per field"""
    FIELDS = [("minmax", 8, True), ("partials", 0, False), ("acc", 16, True), ("pdf_init", 4, True),
              ("iterations", 4, True), ("hist_min", 4, True), ("bucket_size", 8, True), ("bin_bucket", 4, True),
              ("bin_offset", 4, True), ("pdf", 4096, True), ("counts", 4096, True), ("active", 4, True),
              ("enc", 0, False), ("search_part", 0, False)]
    _fields_ = [(name, _vp) for name, _, _ in FIELDS]


class Tq(ctypes.Structure):
    """csrc/tq_internal.hpp: aimet_tensor_quantizer"""
    _fields_ = [("scheme", ctypes.c_int), ("C", _i64), ("device", ctypes.c_int), ("percentile", ctypes.c_float),
                ("stats_updated", ctypes.c_bool), ("hist", ctypes.c_bool), ("kind", ctypes.c_int), ("arena", _vp),
                ("arena_bytes", ctypes.c_size_t), ("slab", _vp), ("d", TqDevice)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-identity", action="store_true")
    args = ap.parse_args()
    from aimet_amd import _native
    libs = {"parent": load(args.parent, ("aimet_tq_",)), "new": load(_native.LIB_PATH, ("aimet_tq_",))}
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [_vp, _vp, ctypes.c_size_t, ctypes.c_int]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = _vp(stream.cuda_stream)
    rng = np.random.default_rng(19)
    bad = []

    def create(lib, scheme, C=1):
        h = _vp()
        ok(lib, lib.aimet_tq_create(scheme, C, 0, ctypes.byref(h)))
        if scheme == PERCENTILE:
            ok(lib, lib.aimet_tq_set_percentile_value(h, 99.5))
        return h

    def pair(scheme, C=1):
        return {tag: create(lib, scheme, C) for tag, lib in libs.items()}

    def destroy(pairs):
        stream.synchronize()
        for p in pairs:
            for tag, lib in libs.items():
                ok(lib, lib.aimet_tq_destroy(p[tag]))

    def state(h):
        q = ctypes.cast(h, ctypes.POINTER(Tq)).contents
        out = {}
        for name, per, compared in TqDevice.FIELDS:
            p = getattr(q.d, name)
            if compared and p:
                buf = np.empty(per * q.C, np.uint8)
                assert hip.hipMemcpy(buf.ctypes.data, p, buf.nbytes, 2) == 0
                out[name] = buf
        return out

    def same_state(pairs):
        """the names of the fields that differ in any quantizer pair"""
        stream.synchronize()
        diff = set()
        for p in pairs:
            a, b = state(p["parent"]), state(p["new"])
            diff |= {k for k in a if not np.array_equal(a[k], b[k])}
        return sorted(diff)

    def dev_view(a, off):
        """a device copy of `a` that starts `off` floats past a 16-byte boundary"""
        flat = np.ascontiguousarray(a, np.float32).ravel()
        t = torch.from_numpy(np.concatenate([np.zeros(off, np.float32), flat])).to(dev)[off:]
        assert t.data_ptr() % 16 == 4 * off
        return t

    def arr(ctype, values):
        return (ctype * len(values))(*values)

    def update_many(lib, hs, ts):
        n = len(hs)
        ok(lib, lib.aimet_tq_update_stats_many(arr(_vp, [h.value for h in hs]), arr(_vp, [t.data_ptr() for t in ts]),
                                               arr(_i64, [t.numel() for t in ts]), n, sp))

    def update_channels_many(lib, hs, ts, views):
        n = len(hs)
        ok(lib, lib.aimet_tq_update_stats_channels_many(
            arr(_vp, [h.value for h in hs]), arr(_vp, [t.data_ptr() for t in ts]), arr(_i64, [v[0] for v in views]),
            arr(_i64, [v[1] for v in views]), arr(_i64, [v[2] for v in views]), n, sp))

    def update(lib, h, t, view):
        ok(lib, lib.aimet_tq_update_stats(h, t.data_ptr(), view[0], view[1], view[2], sp))

    def reset_many(lib, hs):
        ok(lib, lib.aimet_tq_reset_encoding_stats_many(arr(_vp, [h.value for h in hs]), len(hs), sp))

    def report(name, verdicts):
        """verdicts: per batch the differing fields"""
        words = ["identical" if not v else "DIFFERENT (%s)" % ", ".join(v) for v in verdicts]
        if any(verdicts):
            bad.append(name)
        print("%-78s %s" % (name, "; ".join("batch %d %s" % (i + 1, w) for i, w in enumerate(words))), flush=True)

    # ---- 1. bit identity ----------------------------------------------------------------------------
    def tensor_batches(sizes, zero_first, batches=3, edges=False):
        """per batch a list of tensors: odd ones 4-byte offset views; batch 2 wider, with NaN / inf"""
        for batch in range(batches):
            ts = []
            for i, n in enumerate(sizes):
                x = (rng.standard_normal(n) * (1 + 3 * (batch == 1) + i % 3) + 0.25).astype(np.float32)
                if batch == 0 and i in zero_first:
                    x[:] = 0.0
                if n > 100 and batch == 1:
                    x[7], x[8] = np.nan, np.inf
                if edges and n > 4096 and batch == 2:   # values at and next to the bin edges of [-8, 8) / 512
                    e = (np.arange(512, dtype=np.float32) - 256) / np.float32(32)
                    x[:1536] = np.concatenate([e, np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf))])
                if n > 1000 and i % 2 == 0:
                    x[n // 2:] = np.maximum(x[n // 2:], 0)   # exact zeros: the register zero counter
                ts.append(dev_view(x, i % 2))
            yield ts

    def identity_per_tensor(name, schemes, sizes, zero_first, many, reset_after=None):
        if args.only not in name:
            return
        specs = [(s, n) for s in schemes for n in sizes]
        pairs = [pair(s) for s, _ in specs]
        zf = {i for i in range(len(specs)) if i % len(sizes) in zero_first}
        verdicts = []
        for b, ts in enumerate(tensor_batches([n for _, n in specs], zf, edges=True)):
            for tag, lib in libs.items():
                if many:
                    update_many(lib, [p[tag] for p in pairs], ts)
                else:
                    for p, t in zip(pairs, ts):
                        update(lib, p[tag], t, (1, 1, t.numel()))
            verdicts.append(same_state(pairs))
            if reset_after == b:
                for tag, lib in libs.items():
                    reset_many(lib, [p[tag] for p in pairs])
                verdicts.append(same_state(pairs))
        report(name, verdicts)
        destroy(pairs)

    def identity_per_channel(name, schemes, shapes, many):
        if args.only not in name:
            return
        specs = [(s, sh, ax) for s in schemes for sh, ax in shapes]
        pairs = [pair(s, sh[ax]) for s, sh, ax in specs]
        views = []
        for _, sh, ax in specs:
            views.append((int(np.prod(sh[:ax])), sh[ax], int(np.prod(sh[ax + 1:]))))
        verdicts = []
        for batch in range(2):
            ts = []
            for i, (s, sh, ax) in enumerate(specs):
                x = (rng.standard_normal(sh) * (1 + 2 * batch + i % 3)).astype(np.float32)
                if batch == 0 and i % 4 == 0:
                    x[:] = 0.0
                if x.size > 100 and batch == 1:
                    x.flat[7], x.flat[8] = np.nan, np.inf
                x[(slice(None),) * ax + (min(1, sh[ax] - 1),)] = 0.0   # an all-zero channel
                if sh[ax] > 65536:
                    x[(slice(None),) * ax + (65537,)] *= 100.0      # the extremes in a channel past the grid cap
                ts.append(dev_view(x, i % 2))
            for tag, lib in libs.items():
                if many:
                    update_channels_many(lib, [p[tag] for p in pairs], ts, views)
                else:
                    for p, t, v in zip(pairs, ts, views):
                        update(lib, p[tag], t, v)
            verdicts.append(same_state(pairs))
        report(name, verdicts)
        destroy(pairs)

    if not args.skip_identity:
        print("1. Bit identity, parent against new: the quantizers' device state after every batch")
        every = [TF, TFE, PERCENTILE, MSE, ENTROPY]
        sizes = [1, 3, 1000, 4097, 65536, 65536 + 1, 3 * MM_TILE + 5, 1 << 22]
        for many in (False, True):
            identity_per_tensor("per tensor, %s, 5 schemes x %d sizes, reset after batch 2" % (
                "update_stats_many" if many else "update_stats", len(sizes)), every, sizes, {0, 2, 5}, many, reset_after=1)
            identity_per_tensor("per tensor, %s, TF / TF-E / entropy, 2^24 + 3 elements" % (
                "update_stats_many" if many else "update_stats"), [TF, TFE, ENTROPY], [(1 << 24) + 3], set(), many)
        identity_per_tensor("per tensor, update_stats_many, 70 TF-E quantizers (walk), ranges 0 / 33 / 69 unset",
                            [TFE], [(1, 4097, 3 * MM_TILE + 5)[i % 3] for i in range(70)], {0, 33, 69}, True)
        shapes = [((64, 3, 7, 7), 0), ((96, 32, 3, 3), 0), ((16, 24, 3, 3), 1), ((40, 130), 0), ((7, 1), 0), ((3, 1000), 0),
                  ((4, 6, 9, 9), 1)]
        big = [((65536 + 3, 5), 0), ((65536 + 3, 8), 0)]
        for many in (False, True):
            call = "update_stats_channels_many" if many else "update_stats"
            identity_per_channel("per channel, %s, 5 schemes x %d shapes" % (call, len(shapes)), every, shapes, many)
            identity_per_channel("per channel, %s, TF / TF-E / entropy, 65539 channels x 5 (scalar) and x 8 (vector)" % call,
                                 [TF, TFE, ENTROPY], big, many)
        print("rows with a differing bit: %s\n" % (bad or "none"))
    if args.skip_timing:
        return 1 if bad else 0

    # ---- 2. timing ----------------------------------------------------------------------------------
    print("2. Timing: ms per call; accept: new median <= parent median + parent spread (max - min of the parent's rounds)")
    gen = torch.Generator(device=dev).manual_seed(0)

    def pool(numel_per_copy):
        """[copies][pitch] floats (16-byte aligned copies), at least POOL_BYTES in all unless MAX_COPIES is reached"""
        pitch = (numel_per_copy + 3) // 4 * 4
        count = max(2, min(MAX_COPIES, -(-POOL_BYTES // (4 * pitch))))
        return torch.randn(count, pitch, device=dev, generator=gen) * 1.5 + 0.25, count

    def split(row, sizes):
        out, at = [], 0
        for n in sizes:
            out.append(row[at:at + n])
            at += (n + 3) // 4 * 4
        return out

    def time_many(njobs, scheme_name, first):
        name = "update_stats_many %d jobs %s %s batch" % (njobs, scheme_name, "first" if first else "later")
        if args.only not in name:
            return
        sizes = [int(round(2.0 ** (16 + 8 * i / (njobs - 1)))) for i in range(njobs)]
        data, count = pool(sum((n + 3) // 4 * 4 for n in sizes))
        inputs = [split(data[c], sizes) for c in range(count)]
        pairs = [pair(SCHEMES[scheme_name]) for _ in sizes]
        for tag, lib in libs.items():
            update_many(lib, [p[tag] for p in pairs], inputs[0])

        def launch(lib, i):
            tag = "parent" if lib is libs["parent"] else "new"
            hs = [p[tag] for p in pairs]
            if first:
                reset_many(lib, hs)
            update_many(lib, hs, inputs[i % count])

        alternate(libs, stream, "%s (%.0f MiB x %d copies%s)" % (name, data[0].numel() / 262144, count,
                                                                ", each after reset_encoding_stats_many" if first else ""),
                  4 * sum(sizes), launch, bad)
        destroy(pairs)
        del data, inputs

    def time_channels_many(scheme_name):
        name = "update_stats_channels_many conv weights %s" % scheme_name
        if args.only not in name:
            return
        shapes = [(64, 3, 7, 7), (64, 64, 1, 1), (64, 64, 3, 3), (256, 64, 1, 1), (128, 256, 1, 1), (128, 128, 3, 3),
                  (512, 128, 1, 1), (256, 512, 1, 1), (256, 256, 3, 3), (1024, 256, 1, 1), (512, 1024, 1, 1),
                  (512, 512, 3, 3), (2048, 512, 1, 1), (2048, 1024, 1, 1)]
        sizes = [int(np.prod(s)) for s in shapes]
        views = [(1, s[0], int(np.prod(s[1:]))) for s in shapes]
        data, count = pool(sum((n + 3) // 4 * 4 for n in sizes))
        inputs = [split(data[c], sizes) for c in range(count)]
        pairs = [pair(SCHEMES[scheme_name], s[0]) for s in shapes]

        def launch(lib, i):
            tag = "parent" if lib is libs["parent"] else "new"
            update_channels_many(lib, [p[tag] for p in pairs], inputs[i % count], views)

        alternate(libs, stream, "%s (%d shapes, %.1f MiB x %d copies)" % (name, len(shapes), data[0].numel() / 262144, count),
                  4 * sum(sizes), launch, bad)
        destroy(pairs)

    def time_single(scheme_name, view):
        name = "update_stats %s %s" % ("x".join(map(str, view)), scheme_name)
        if args.only not in name:
            return
        n = view[0] * view[1] * view[2]
        data, count = pool(n)
        p = pair(SCHEMES[scheme_name], view[1])

        def launch(lib, i):
            update(lib, p["parent" if lib is libs["parent"] else "new"], data[i % count], view)

        alternate(libs, stream, "%s (%.1f MiB x %d copies)" % (name, n / 262144, count), 4 * n, launch, bad)
        destroy([p])

    for njobs in (55, 318):
        for scheme_name in ("tf", "tfe"):
            for first in (True, False):
                time_many(njobs, scheme_name, first)
    for scheme_name in ("tf", "tfe"):
        time_channels_many(scheme_name)
    for scheme_name in ("tf", "tfe"):
        time_single(scheme_name, (1, 1, 1 << 24))
    for scheme_name in ("tf", "tfe"):
        time_single(scheme_name, (1, 512, 512 * 9))
    print("rows slower or not bit-identical: %s" % (bad or "none"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
