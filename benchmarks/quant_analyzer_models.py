"""QuantAnalyzer's per-layer MSE on whole models, the squared-error kernel alone and the histogram export,
on one GPU.

  python benchmarks/quant_analyzer_models.py [--batch 16] [--batches 2] [--size 224] [--json OUT] [--txt OUT]

1. export_per_layer_mse_loss on the seeded BatchNorm MobileNet-v2 and ResNet-50 (batch norms folded, W8
   A8, TF-Enhanced), against two alternatives on the same GPU, same sim, same batches:
     reference  the reference's literal procedure in plain torch (tests/qa_oracle.py per_layer_mse_literal):
                for every layer and batch a forward of the sim and of the FP model up to that layer,
                fp32 mse_loss(...).item();
     torch-sum  this package's schedule with ((a.double() - b.double())**2).sum() and (a.double()**2).sum()
                in place of aimet_qa_sq_err.
   Wall-clock around work that ends in a device synchronise, one warm-up run of each path first (code
   objects, MIOpen's algorithm choice), then `--runs` timed runs, interleaved. The three per-layer dicts
   are compared.
2. aimet_qa_sq_err alone at 2^28 elements, fp32 and bf16, beside the torch expression: device events
   around `iters` calls; the two inputs together (2 GiB, 1 GiB) exceed the 256 MiB Infinity Cache
   several times, so every call reads HBM. The bytes are those of the two inputs, read once; the peak
   is 8 TB/s.
   ResNet-50 layer outputs at batch 16 (51, 26 and 6.4 MB a tensor) rotate over copies adding up to
   more than 512 MiB.
3. export_per_layer_stats_histogram on the ResNet-50 sim with per-channel weights (two timed runs).
4. Per model, two forwards of the fp32 model and of the sim on one batch compared bit for bit, layer
   output by layer output: whether the forwards repeat, and where they first do not.
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import qa_oracle as O  # noqa: E402
from aimet_amd import _native  # noqa: E402
from aimet_amd import batch_norm_fold as BNF  # noqa: E402
from aimet_amd import quant_analyzer as QA  # noqa: E402
from aimet_amd.quantizers import QuantScheme  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

DEV = "cuda"
PEAK_TBS = 8.0
PER_CHANNEL = {"defaults": {"ops": {}, "params": {"is_symmetric": "True"}, "per_channel_quantization": "True"}}


class Lines(list):
    """The report: every line is also printed as it is made."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)

    def __iadd__(self, more):
        for line in more:
            self.append(line)
        return self


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def calibrate(model, data):
    with torch.no_grad():
        for x in data:
            model(x)


def build(model, data, config=None):
    sim = QuantizationSimModel(model, data[0][:1], quant_scheme=QuantScheme.post_training_tf_enhanced,
                               default_output_bw=8, default_param_bw=8, config_file=config)
    sim.compute_encodings(calibrate, data)
    ok = QA.CallbackFunc(lambda m, a: 0.0, None)
    analyzer = QA.QuantAnalyzer(model, data[0][:1], ok, ok)
    analyzer.enable_per_layer_mse_loss(data, len(data))
    return sim, analyzer


def torch_sq_err(ref, x, scale, acc):
    a, b = ref.double(), x.double()
    acc[0] += scale * ((a - b) ** 2).sum()
    acc[1] += scale * (a ** 2).sum()


def run_path(path, model, sim, analyzer, data, out_dir):
    if path == "reference":
        names = [n for n, _ in QA.get_ordered_list_of_modules(model, data[0][:1])]
        return timed(lambda: O.per_layer_mse_literal(model, sim.model, names, data))
    if path == "torch-sum":
        real = QA.add_sq_err
        QA.add_sq_err = torch_sq_err
        try:
            return timed(lambda: analyzer.export_per_layer_mse_loss(sim, out_dir))
        finally:
            QA.add_sq_err = real
    return timed(lambda: analyzer.export_per_layer_mse_loss(sim, out_dir))


def kernel_rates(lines, res):
    """2^28 elements in fp32 and bf16, and fp32 layer outputs of ResNet-50 at batch 16: below 1 GiB a call
    the inputs rotate over copies adding up to more than 512 MiB, so that every call reads HBM."""
    cases = [("2^28", 1 << 28, "fp32"), ("2^28", 1 << 28, "bf16"), ("16x64x112x112", 16 * 64 * 112 * 112, "fp32"),
             ("16x512x28x28", 16 * 512 * 28 * 28, "fp32"), ("16x2048x7x7", 16 * 2048 * 7 * 7, "fp32")]
    dtypes = {"fp32": (torch.float32, 0), "bf16": (torch.bfloat16, 2)}
    for label, n, name in cases:
        dtype, io = dtypes[name]
        nbytes = 2 * n * torch.empty(0, dtype=dtype).element_size()
        copies = 1 if nbytes >= (1 << 30) else min(64, -(-(512 << 20) // nbytes) + 1)
        refs = [torch.randn(n, device=DEV, dtype=dtype) for _ in range(copies)]
        xs = [(r.float() + 0.01 * torch.randn(n, device=DEV)).to(dtype) for r in refs]
        acc = torch.zeros(2, dtype=torch.float64, device=DEV)
        stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

        def ours(i):
            _native.call("aimet_qa_sq_err", refs[i % copies].data_ptr(), xs[i % copies].data_ptr(), n, io, 1.0 / n,
                         acc.data_ptr(), stream())

        def theirs(i):
            torch_sq_err(refs[i % copies], xs[i % copies], 1.0 / n, acc)
        row = {"shape": label, "dtype": name, "elements": n, "bytes": nbytes, "rotating_copies": copies}
        for who, fn, iters in (("kernel", ours, max(20, 2 * copies)), ("torch", theirs, max(3, copies))):
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
            t = statistics.median(times)
            row[who] = {"us_per_call": t * 1e6, "tb_per_s": nbytes / t / 1e12, "of_peak": nbytes / t / 1e12 / PEAK_TBS,
                        "iters": iters, "min_us": min(times) * 1e6, "max_us": max(times) * 1e6}
        res["sq_err"].append(row)
        lines.append("  %-14s %-5s %7.1f MB  kernel %8.1f us [%.1f .. %.1f] %6.3f TB/s (%.3f of %.0f TB/s)   torch %9.1f us "
                     "%6.3f TB/s   torch / kernel %.1fx" %
                     (label, name, nbytes / 1e6, row["kernel"]["us_per_call"], row["kernel"]["min_us"],
                      row["kernel"]["max_us"], row["kernel"]["tb_per_s"], row["kernel"]["of_peak"], PEAK_TBS,
                      row["torch"]["us_per_call"], row["torch"]["tb_per_s"],
                      row["torch"]["us_per_call"] / row["kernel"]["us_per_call"]))
        del refs, xs
        torch.cuda.empty_cache()


def forward_repeatability(model, sim, batch):
    """Two forwards of the fp32 model and two of the sim on one batch, every leaf module's first output
    compared bit for bit in execution order; in the sim a wrapped layer is listed twice, the library
    layer inside the wrapper (`<name>._module_to_wrap`: quantized input and weight in, no output
    quantizer yet) and then the wrapper."""
    names = [n for n, _ in QA.get_ordered_list_of_modules(model, batch[:1])]
    in_sim = dict(sim.model.named_modules())
    sim_names = []
    for n in names:
        if isinstance(in_sim[n], QA.QcQuantizeWrapper):
            sim_names.append(n + "._module_to_wrap")
        sim_names.append(n)
    out = {}
    for who, net, listed in (("fp32 model", model, names), ("sim", sim.model, sim_names)):
        first, second = O.capture(net, listed, batch), O.capture(net, listed, batch)
        differing = [n for n in listed if not torch.equal(first[n], second[n])]
        worst = max((float(((first[n].double() - second[n].double()).abs().max() /
                            first[n].double().abs().max().clamp_min(1e-300))) for n in differing), default=0.0)
        out[who] = {"outputs": len(listed), "differing": len(differing), "first_differing": differing[0] if differing else None,
                    "kind": type(dict(net.named_modules())[differing[0]]).__name__ if differing else None,
                    "largest_difference_over_largest_value": worst}
        del first, second
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "benchmarks/quant_analyzer_models.py needs an MI355X"
    from workloads.mobilenet_v2_bn import mobilenet_v2_bn
    from workloads.resnet import resnet50

    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "batches": args.batches, "size": args.size,
           "runs": args.runs, "workloads": {}, "sq_err": [], "stats_histogram": {}}
    lines = Lines()
    lines.append("QuantAnalyzer per-layer MSE, %s; %d batches of %d at %dx%d; ms: median [min .. max] of %d runs after a "
                 "warm-up" % (res["device"], args.batches, args.batch, args.size, args.size, args.runs))
    g = torch.Generator().manual_seed(0)
    data = [torch.randn(args.batch, 3, args.size, args.size, generator=g).to(DEV) for _ in range(args.batches)]
    out_dir = tempfile.mkdtemp(prefix="quant_analyzer_")

    paths = ("fused", "torch-sum", "reference")
    rnet = None
    for wname, make in (("mobilenet_v2_bn (BN folded)", mobilenet_v2_bn), ("resnet50 (BN folded)", resnet50)):
        model = make(device=DEV).eval()
        BNF.fold_all_batch_norms(model)
        if make is resnet50:
            rnet = model
        sim, analyzer = build(model, data)
        dicts = {}
        earlier = {p: run_path(p, model, sim, analyzer, data, out_dir)[1] for p in paths}   # the warm-up runs
        times = {p: [] for p in paths}
        for _ in range(args.runs):
            for p in paths:
                t, dicts[p] = run_path(p, model, sim, analyzer, data, out_dir)
                times[p].append(t)
        w = {p: {"median_ms": 1e3 * statistics.median(times[p]), "min_ms": 1e3 * min(times[p]),
                 "max_ms": 1e3 * max(times[p])} for p in paths}
        fused = dicts["fused"]
        w["layers"] = len(fused)
        w["max_relative_difference"] = {
            p: max(abs(dicts[p][n] - v) / v for n, v in fused.items() if v > 0.0) for p in paths[1:]}
        w["same_layers"] = all(list(dicts[p]) == list(fused) for p in paths[1:])
        # the forwards themselves from one run to the next: each path against its own warm-up run
        w["run_to_run_relative_difference"] = {
            p: max(abs(earlier[p][n] - v) / v for n, v in dicts[p].items() if v > 0.0) for p in paths}
        w["worst_layer"] = {p: max((n for n, v in fused.items() if v > 0.0), key=lambda n: abs(dicts[p][n] - fused[n]) / fused[n])
                            for p in paths[1:]}
        res["workloads"][wname] = w
        lines += ["", "%s export_per_layer_mse_loss, %d layers" % (wname, w["layers"])]
        for p in paths:
            lines.append("  %-10s %10.1f [%10.1f .. %10.1f]" % (p, w[p]["median_ms"], w[p]["min_ms"], w[p]["max_ms"]))
        lines.append("  torch-sum / fused %.2fx, reference / fused %.2fx (medians); largest relative difference of a "
                     "layer's loss to fused: torch-sum %.3e, reference %.3e; same layers in the same order: %s" %
                     (w["torch-sum"]["median_ms"] / w["fused"]["median_ms"],
                      w["reference"]["median_ms"] / w["fused"]["median_ms"], w["max_relative_difference"]["torch-sum"],
                      w["max_relative_difference"]["reference"], w["same_layers"]))
        lines.append("  the same path's loss from one run to the next, largest relative difference: " +
                     ", ".join("%s %.3e" % (p, w["run_to_run_relative_difference"][p]) for p in paths) +
                     "; layer of the largest difference to fused: torch-sum %s, reference %s" %
                     (w["worst_layer"]["torch-sum"], w["worst_layer"]["reference"]))
        w["forward_repeatability"] = forward_repeatability(model, sim, data[0])
        for who, r in w["forward_repeatability"].items():
            lines.append("  two forwards of the %s on one batch, bit for bit: %d of %d outputs differ%s" %
                         (who, r["differing"], r["outputs"],
                          "" if not r["differing"] else "; the first in execution order is %s (%s), largest "
                          "|difference| / largest |value| of an output %.3e" %
                          (r["first_differing"], r["kind"], r["largest_difference_over_largest_value"])))
        del sim, analyzer

    lines += ["", "aimet_qa_sq_err (both launches of a call) beside torch's float64 expression, inputs read from HBM"]
    kernel_rates(lines, res)

    sim, analyzer = build(copy.deepcopy(rnet), data, PER_CHANNEL)
    channels = sum(len(w.param_quantizers["weight"].encoding) for _, w in sim.quant_wrappers())
    times = [timed(lambda: analyzer.export_per_layer_stats_histogram(sim, out_dir))[0] for _ in range(1 + min(args.runs, 2))][1:]
    res["stats_histogram"] = {"median_ms": 1e3 * statistics.median(times), "min_ms": 1e3 * min(times),
                              "max_ms": 1e3 * max(times), "weight_channels": channels}
    lines += ["", "export_per_layer_stats_histogram, resnet50 with per-channel weights (%d weight channels, one "
                  "histogram read-back each): %.1f ms [%.1f .. %.1f]" %
              (channels, 1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times))]

    text = "\n".join(lines)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
