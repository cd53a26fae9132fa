"""BatchNorm re-estimation and BN fold to scale on whole models, and aimet_bnre_forward alone, on one GPU.

  python benchmarks/bn_reestimation_models.py [--batch 32] [--batches 8] [--size 224] [--runs 5] [--json OUT] [--txt OUT]

1. reestimate_bn_stats on the seeded ResNet-50 and the BatchNorm MobileNet-v2 against the reference's
   procedure in plain torch on the same GPU (tests/bnre_oracle.py: reestimate_torch: training-mode
   BatchNorms at momentum 1, float32 sums of the running buffers after every batch). The two
   alternate in one process; wall-clock around work that ends in a device synchronise; one warm-up
   run of each first, then the median, the least and the largest of `--runs` runs.
2. aimet_bnre_forward alone against F.batch_norm(training=True, momentum=1) plus the two adds, at
   32x64x112x112, 32x512x28x28, 32x2048x7x7 and 32x1000: device events around `iters` calls that
   rotate over copies of the input adding up to more than 512 MiB, so every call reads HBM. GB/s
   counts one read and one write of the tensor (8 bytes per element), the least any form moves.
3. The resident form against the streaming form at the shapes where both apply (a channel's
   elements fit LDS): 32x1024x14x14, 32x2048x7x7, 32x1000.
4. fold_all_batch_norms_to_scale on a range-learning W8 per-channel sim of both models against a
   per-pair loop: one aimet_dfq_bn_fold launch per pair and the reference's Python loop that builds
   each channel's new TfEncoding.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

import torch
import torch.nn.functional as F
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bnre_oracle as O  # noqa: E402
from aimet_amd import _dfq, _native  # noqa: E402
from aimet_amd import batch_norm_fold as BNF  # noqa: E402
from aimet_amd import bn_reestimation as BNRE  # noqa: E402
from aimet_amd.libpymo import TfEncoding  # noqa: E402
from aimet_amd.quantizers import QuantScheme  # noqa: E402
from aimet_amd.quantsim import DEFAULT_QUANTIZABLE_TYPES, QuantizationSimModel  # noqa: E402

DEV = "cuda"
PER_CHANNEL_CFG = {"defaults": {"ops": {"is_output_quantized": "True"},
                                "params": {"is_quantized": "True", "is_symmetric": "True"},
                                "strict_symmetric": "False", "per_channel_quantization": "True"}}


class Lines(list):
    """The report: every line is also printed as it is made."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def spread(times):
    return {"median_ms": 1e3 * statistics.median(times), "min_ms": 1e3 * min(times), "max_ms": 1e3 * max(times)}


def fmt(s):
    return "%9.2f [%9.2f .. %9.2f]" % (s["median_ms"], s["min_ms"], s["max_ms"])


def bn_stats(model):
    return torch.cat([t.detach().double().flatten() for bn in O.active_bns(model)
                      for t in (bn.running_mean, bn.running_var)])


# ---------------------------------------------------------------------------------------------------
def reestimation(lines, res, name, model, data, runs):
    paths = {"fused": lambda m: BNRE.reestimate_bn_stats(m, data), "torch": lambda m: O.reestimate_torch(m, data)}
    models = {p: copy.deepcopy(model) for p in paths}
    handle = None
    for p, fn in paths.items():                       # warm-up: code objects, the library's algorithm choice
        out = fn(models[p])
        handle = out if p == "fused" else handle
    times = {p: [] for p in paths}
    for _ in range(runs):
        for p, fn in paths.items():
            times[p].append(timed(lambda: fn(models[p])))
    w = {p: spread(times[p]) for p in paths}
    w["batch_norms"] = len(O.active_bns(model))
    w["fused_route"], w["fallback_route"] = handle.fused, handle.fallback
    diff = (bn_stats(models["fused"]) - bn_stats(models["torch"])).abs()
    w["max_stat_difference"] = float(diff.max())
    w["max_abs_stat"] = float(bn_stats(models["torch"]).abs().max())
    w["fused_over_torch"] = w["fused"]["median_ms"] / w["torch"]["median_ms"]
    res["reestimation"][name] = w
    lines.append("")
    lines.append("%s: %d BatchNorms (%d fused, %d through torch)" % (name, w["batch_norms"], handle.fused, handle.fallback))
    for p in paths:
        lines.append("  %-22s %s ms" % ("reestimate_bn_stats" if p == "fused" else "plain torch procedure", fmt(w[p])))
    lines.append("  fused / torch %.3f (medians); largest difference of a running statistic %.3e (largest statistic %.3e)"
                 % (w["fused_over_torch"], w["max_stat_difference"], w["max_abs_stat"]))


# ---------------------------------------------------------------------------------------------------
def set_form(form):
    _native.call("aimet_bnre_forward_form", form, None)


def forward_rate(shape, fn_factory, iters_min=50):
    """us per call of fn(i) over rotating copies of a [outer][C][inner] input."""
    outer, C, inner = shape
    nbytes = outer * C * inner * 4
    copies = min(max(2, -(-(512 << 20) // nbytes) + 1), 256)
    xs = [torch.randn(outer, C, inner, device=DEV) * 0.5 + 3.0 for _ in range(copies)]
    fn = fn_factory(xs)
    iters = max(2 * copies, iters_min)
    for i in range(copies):
        fn(i)
    times = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / iters)
    return statistics.median(times), min(times), max(times)


def kernel_factory(shape):
    outer, C, inner = shape
    gamma, beta = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
    acc = torch.zeros(2, C, dtype=torch.float64, device=DEV)

    def factory(xs):
        y = torch.empty_like(xs[0])
        stream = torch.cuda.current_stream().cuda_stream

        def fn(i):
            _native.call("aimet_bnre_forward", xs[i % len(xs)].data_ptr(), outer, C, inner, gamma.data_ptr(),
                         beta.data_ptr(), 1e-5, y.data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(), stream)
        return fn
    return factory


def torch_factory(shape):
    outer, C, inner = shape
    gamma, beta = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    sm, sv = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)

    def factory(xs):
        views = [x.view(outer, C) if inner == 1 else x for x in xs]

        def fn(i):
            F.batch_norm(views[i % len(views)], rm, rv, gamma, beta, True, 1.0, 1e-5)
            sm.add_(rm)
            sv.add_(rv)
        return fn
    return factory


def rate_row(shape, t):
    nbytes = shape[0] * shape[1] * shape[2] * 8
    return {"us_per_call": t[0] * 1e6, "min_us": t[1] * 1e6, "max_us": t[2] * 1e6, "gb_per_s": nbytes / t[0] / 1e9}


def kernel_rates(lines, res):
    lines.append("")
    lines.append("aimet_bnre_forward (default form) beside F.batch_norm(training, momentum 1) + two adds; "
                 "GB/s = 8 bytes per element over the time; us: median [min .. max] of 3 windows")
    for shape in ((32, 64, 112 * 112), (32, 512, 28 * 28), (32, 2048, 49), (32, 1000, 1)):
        set_form(0)
        ours = rate_row(shape, forward_rate(shape, kernel_factory(shape)))
        theirs = rate_row(shape, forward_rate(shape, torch_factory(shape)))
        res["forward"].append({"shape": list(shape), "kernel": ours, "torch": theirs})
        lines.append("  %-16s kernel %8.1f us [%8.1f .. %8.1f] %7.1f GB/s   torch %8.1f us [%8.1f .. %8.1f] %7.1f GB/s   "
                     "torch / kernel %.2f" % ("x".join(map(str, shape)), ours["us_per_call"], ours["min_us"],
                                              ours["max_us"], ours["gb_per_s"], theirs["us_per_call"], theirs["min_us"],
                                              theirs["max_us"], theirs["gb_per_s"],
                                              theirs["us_per_call"] / ours["us_per_call"]))
    lines.append("")
    lines.append("resident form (one launch, x read once) beside the streaming form (three launches), where a channel fits LDS")
    for shape in ((32, 1024, 14 * 14), (32, 2048, 49), (32, 1000, 1)):
        row = {"shape": list(shape)}
        for name, form in (("streaming", 1), ("resident", 2)):
            set_form(form)
            row[name] = rate_row(shape, forward_rate(shape, kernel_factory(shape)))
        set_form(0)
        res["forms"].append(row)
        lines.append("  %-16s streaming %8.1f us [%8.1f .. %8.1f]   resident %8.1f us [%8.1f .. %8.1f]   streaming / resident %.2f"
                     % ("x".join(map(str, shape)), row["streaming"]["us_per_call"], row["streaming"]["min_us"],
                        row["streaming"]["max_us"], row["resident"]["us_per_call"], row["resident"]["min_us"],
                        row["resident"]["max_us"], row["streaming"]["us_per_call"] / row["resident"]["us_per_call"]))


# ---------------------------------------------------------------------------------------------------
def fold_pairwise(sim):
    """The reference's _fold_to_scale, pair by pair, on this package's pieces: one aimet_dfq_bn_fold
    launch per pair, then each channel's new TfEncoding in a Python loop and the encoding setter."""
    for conv_wrapper, bn_wrapper in BNF._find_scale_pairs(sim):
        conv, bn = conv_wrapper._module_to_wrap, bn_wrapper._module_to_wrap
        q = conv_wrapper.param_quantizers["weight"]
        encodings = q.encoding
        encodings = encodings if isinstance(encodings, list) else [encodings]
        with torch.no_grad():
            if conv.bias is None:
                conv.bias = nn.Parameter(torch.zeros(conv.weight.shape[0], device=conv.weight.device))
            stage = _dfq.Stage([conv.weight])
            _dfq.bn_fold_launch(stage, [dict(module=conv, weight=stage.dev(conv.weight), bias=stage.dev(conv.bias),
                                             bn=bn, forward=False)])
            new = []
            for old, c in zip(encodings, bn.weight / torch.sqrt(bn.running_var + bn.eps)):
                e = TfEncoding()
                e.delta = old.delta * abs(c)
                if c >= 0:
                    e.max, e.min = old.max * c, old.min * c
                else:
                    e.max, e.min = old.min * c, old.max * c
                e.offset, e.bw = old.offset, old.bw
                new.append(e)
            q.encoding = new


def fold_to_scale(lines, res, name, model, data, runs):
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "cfg.json")
        with open(cfg, "w") as f:
            json.dump(PER_CHANNEL_CFG, f)
        sim = QuantizationSimModel(copy.deepcopy(model), in_place=True,
                                   quant_scheme=QuantScheme.training_range_learning_with_tf_init, config_file=cfg,
                                   quantizable_types=DEFAULT_QUANTIZABLE_TYPES + (nn.BatchNorm1d, nn.BatchNorm2d))
    pairs = BNF.prepare_for_fold_to_scale(sim)
    with torch.no_grad():
        sim.compute_encodings(lambda m, _: m(data[0]), None)
    paths = {"one launch": BNF.fold_all_batch_norms_to_scale, "pair by pair": fold_pairwise}
    times = {p: [] for p in paths}
    for k in range(runs + 1):                         # the first round is the warm-up
        for p, fn in paths.items():
            twin = copy.deepcopy(sim)
            t = timed(lambda: fn(twin))
            if k:
                times[p].append(t)
    w = {p: spread(times[p]) for p in paths}
    w["pairs"] = len(pairs)
    res["fold_to_scale"][name] = w
    lines.append("")
    lines.append("%s: fold to scale, %d pairs" % (name, len(pairs)))
    for p in paths:
        lines.append("  %-14s %s ms" % (p, fmt(w[p])))
    lines.append("  pair by pair / one launch %.2f (medians)" %
                 (w["pair by pair"]["median_ms"] / w["one launch"]["median_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "benchmarks/bn_reestimation_models.py needs an MI355X"
    from workloads.mobilenet_v2_bn import mobilenet_v2_bn
    from workloads.resnet import resnet50

    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "batches": args.batches, "size": args.size,
           "runs": args.runs, "reestimation": {}, "forward": [], "forms": [], "fold_to_scale": {}}
    lines = Lines()
    lines.append("BatchNorm re-estimation, %s; %d batches of %d at %dx%d; ms: median [min .. max] of %d runs after a warm-up"
                 % (res["device"], args.batches, args.batch, args.size, args.size, args.runs))
    g = torch.Generator().manual_seed(0)
    data = [torch.randn(args.batch, 3, args.size, args.size, generator=g).to(DEV) for _ in range(args.batches)]
    nets = (("resnet50", resnet50(device=DEV)), ("mobilenet_v2_bn", mobilenet_v2_bn(device=DEV)))
    def save():   # after every section, so that a long run leaves what it has measured
        if args.txt:
            with open(args.txt, "w") as f:
                f.write("\n".join(lines) + "\n")
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)

    for name, net in nets:
        reestimation(lines, res, name, net, data, args.runs)
        save()
    kernel_rates(lines, res)
    save()
    for name, net in nets:
        fold_to_scale(lines, res, name, net, data, args.runs)
        save()


if __name__ == "__main__":
    main()
