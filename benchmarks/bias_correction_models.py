"""Bias correction on whole models and the channel-sum kernel alone, on one GPU.

  python benchmarks/bias_correction_models.py [--batch 16] [--batches 2] [--size 224] [--json OUT] [--txt OUT]

1. correct_bias (empirical, every layer) on the BatchNorm MobileNet-v2 after fold_all_batch_norms +
   equalize_model and on ResNet-50 after fold_all_batch_norms, W8 A8, against two alternatives on the
   same GPU, same sim, same batches:
     reference  the reference's procedure in plain torch + numpy: for every layer and batch a forward of
                the FP model and of the sim up to that layer, both outputs copied to the host,
                concatenated, float32 numpy means, the bias written back;
     torch-sum  this package's schedule with x.sum(dims, dtype=torch.float64) in place of
                aimet_bc_channel_sums.
   Wall-clock around work that ends in a device synchronise, one warm-up run of each path first
   (code objects, MIOpen's algorithm choice), then `--runs` timed runs, interleaved.
2. aimet_bc_channel_sums alone at 32x64x112x112, 32x2048x7x7 (planar) and 32x1000 (interleaved),
   beside torch's float64 reduction: device events around `iters` calls that rotate over copies of the
   input adding up to more than 512 MiB (twice the Infinity Cache), so every call reads HBM. The
   bytes are those of the input, read once; the peak is 8 TB/s.
3. Output SQNR of the W8 and W4 seeded MobileNet-v2 (fold + CLE; weights quantized, first input at 8
   bits, output quantizers off: the sim correct_bias measures) against FP, before and after.
"""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from aimet_amd import _native  # noqa: E402
from aimet_amd import batch_norm_fold as BNF  # noqa: E402
from aimet_amd import bias_correction as BC  # noqa: E402
from aimet_amd import cross_layer_equalization as CLE  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

DEV = "cuda"
PEAK_TBS = 8.0


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


def loader(n, bs, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(bs, 3, size, size, generator=g),) for _ in range(n)]


def build_sim(model, qp, data):
    sim = QuantizationSimModel(model, dummy_input=data[0][:1], quant_scheme=qp.quant_scheme,
                               rounding_mode=qp.round_mode, default_output_bw=qp.act_bw,
                               default_param_bw=qp.weight_bw, in_place=True, config_file=qp.config_file)
    for _, w in sim.quant_wrappers():
        w.output_quantizers[0].enabled = False
    sim.compute_encodings(lambda m, _: [BC.forward_pass(m, b) for b in data], None)
    return sim


def output_to_host(layer, net, batch):
    got = []

    def hook(_, __, out):
        got.append(out.detach().cpu().numpy())
        raise BC.StopForwardException
    h = layer.register_forward_hook(hook)
    try:
        BC.forward_pass(net, batch)
    finally:
        h.remove()
    return np.vstack(got)


def reference_procedure(model, qp, data):
    """aimet_torch/bias_correction.py:370-458 (empirical only) restated: O(L^2) forwards, every layer
    output of both models on the host."""
    ordered = BC._layers_in_execution_order(model, data[0])
    fp = copy.deepcopy(model)
    for _, m in ordered:
        if m.bias is None:
            m.bias = nn.Parameter(torch.zeros(BC._out_channels(m), device=DEV))
    sim = build_sim(model, qp, data)
    wrapper_of = {w.get_original_module(): w for _, w in sim.quant_wrappers()}
    for name, module in ordered:
        refs, quants = [], []
        for b in data:
            r = output_to_host(fp.get_submodule(name), fp, b)
            q = output_to_host(wrapper_of[module], model, b)
            if isinstance(module, nn.Linear):
                r, q = r.reshape(r.shape + (1, 1)), q.reshape(q.shape + (1, 1))
            refs.append(r)
            quants.append(q)
        error = (np.concatenate(quants) - np.concatenate(refs)).mean(3).mean(2).mean(0)
        bias = module.bias.detach().cpu().numpy() - error
        with torch.no_grad():
            module.bias.copy_(torch.from_numpy(bias))
    QuantizationSimModel._remove_quantization_wrappers(model, list(model.modules()))


def torch_channel_sums(layer, out, acc):
    if isinstance(layer, nn.Linear):
        flat = out.reshape(-1, out.shape[-1])
        acc += flat.sum(0, dtype=torch.float64)
        return flat.shape[0]
    acc += out.sum([0] + list(range(2, out.dim())), dtype=torch.float64)
    return out.numel() // out.shape[1]


def run_path(path, base, qp, data):
    model = copy.deepcopy(base)
    n = sum(int(b[0].shape[0]) for b in data)
    dev_data = [b[0].to(DEV) for b in data]
    if path == "reference":
        t, _ = timed(lambda: reference_procedure(model, qp, dev_data))
    elif path == "torch-sum":
        real = BC._add_channel_sums
        BC._add_channel_sums = torch_channel_sums
        try:
            t, _ = timed(lambda: BC.correct_bias(model, qp, n, data, n))
        finally:
            BC._add_channel_sums = real
    else:
        t, _ = timed(lambda: BC.correct_bias(model, qp, n, data, n))
    return t, model


def bias_vector(model):
    return torch.cat([m.bias.detach().double().flatten() for m in model.modules()
                      if isinstance(m, BC._LAYERS) and m.bias is not None])


def sqnr_db(fp, model, qp, data):
    dev_data = [b[0].to(DEV) for b in data]
    sim = build_sim(copy.deepcopy(model), qp, dev_data)
    sig = noise = 0.0
    with torch.no_grad():
        for b in dev_data:
            want = fp(b).double()
            got = sim.model(b).double()
            sig += float((want ** 2).sum())
            noise += float(((got - want) ** 2).sum())
    return 10.0 * math.log10(sig / max(noise, 1e-300))


def kernel_rates(lines, res):
    lib_call = _native.call
    for shape in ((32, 64, 112 * 112), (32, 2048, 49), (32, 1000, 1)):
        outer, C, inner = shape
        nbytes = outer * C * inner * 4
        copies = max(2, -(-(512 << 20) // nbytes) + 1)
        copies = min(copies, 256)
        xs = [torch.randn(outer, C, inner, device=DEV) for _ in range(copies)]
        acc = torch.zeros(C, dtype=torch.float64, device=DEV)
        stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
        iters = max(2 * copies, 50)

        def ours(i):
            x = xs[i % copies]
            lib_call("aimet_bc_channel_sums", x.data_ptr(), outer, C, inner, acc.data_ptr(), stream())

        def theirs(i):
            x = xs[i % copies]
            acc.add_(x.sum((0, 2), dtype=torch.float64))
        row = {"shape": list(shape), "bytes": nbytes, "rotating_copies": copies, "iters": iters}
        for name, fn in (("kernel", ours), ("torch", theirs)):
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
            row[name] = {"us_per_call": t * 1e6, "tb_per_s": nbytes / t / 1e12, "of_peak": nbytes / t / 1e12 / PEAK_TBS}
        res["channel_sums"].append(row)
        lines.append("  %-16s %8.1f MB  kernel %8.1f us %6.3f TB/s (%.3f of %.0f TB/s)   torch %8.1f us %6.3f TB/s   "
                     "torch / kernel %.2fx" % ("x".join(map(str, shape)), nbytes / 1e6, row["kernel"]["us_per_call"],
                                               row["kernel"]["tb_per_s"], row["kernel"]["of_peak"], PEAK_TBS,
                                               row["torch"]["us_per_call"], row["torch"]["tb_per_s"],
                                               row["torch"]["us_per_call"] / row["kernel"]["us_per_call"]))
        del xs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "benchmarks/bias_correction_models.py needs an MI355X"
    from workloads.mobilenet_v2_bn import mobilenet_v2_bn
    from workloads.resnet import resnet50

    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "batches": args.batches, "size": args.size,
           "runs": args.runs, "workloads": {}, "channel_sums": [], "sqnr_db": {}}
    lines = Lines()
    lines.append("bias correction, %s; %d batches of %d at %dx%d; ms: median [min .. max] of %d runs after a warm-up" %
                 (res["device"], args.batches, args.batch, args.size, args.size, args.runs))
    data = loader(args.batches, args.batch, args.size)

    mnet = mobilenet_v2_bn(device=DEV)
    BC._dfq.replace_modules(mnet, lambda m: isinstance(m, nn.ReLU6), lambda m: nn.ReLU())
    folded = BNF.fold_all_batch_norms(mnet)
    CLE.equalize_bn_folded_model(mnet, None, folded)
    rnet = resnet50(device=DEV)
    BNF.fold_all_batch_norms(rnet)
    qp = BC.QuantParams(weight_bw=8, act_bw=8)
    paths = ("fused", "torch-sum", "reference")
    for wname, base in (("mobilenet_v2_bn (fold + CLE) correct_bias", mnet), ("resnet50 (BN folded) correct_bias", rnet)):
        models = {}
        for p in paths:
            run_path(p, base, qp, data)
        times = {p: [] for p in paths}
        for _ in range(args.runs):
            for p in paths:
                t, models[p] = run_path(p, base, qp, data)
                times[p].append(t)
        w = {p: {"median_ms": 1e3 * statistics.median(times[p]), "min_ms": 1e3 * min(times[p]),
                 "max_ms": 1e3 * max(times[p])} for p in paths}
        ref_b = bias_vector(models["fused"])
        w["max_bias_difference"] = {p: float((bias_vector(models[p]) - ref_b).abs().max()) for p in paths[1:]}
        w["max_abs_bias"] = float(ref_b.abs().max())
        w["layers"] = sum(isinstance(m, BC._LAYERS) for m in base.modules())
        res["workloads"][wname] = w
        lines += ["", "%s, %d layers" % (wname, w["layers"])]
        for p in paths:
            lines.append("  %-10s %10.1f [%10.1f .. %10.1f]" % (p, w[p]["median_ms"], w[p]["min_ms"], w[p]["max_ms"]))
        lines.append("  torch-sum / fused %.2fx, reference / fused %.2fx (medians); largest bias difference to fused: "
                     "torch-sum %.3e, reference %.3e (largest |bias| %.3e)" %
                     (w["torch-sum"]["median_ms"] / w["fused"]["median_ms"],
                      w["reference"]["median_ms"] / w["fused"]["median_ms"], w["max_bias_difference"]["torch-sum"],
                      w["max_bias_difference"]["reference"], w["max_abs_bias"]))

    lines += ["", "aimet_bc_channel_sums (both launches of a call) beside torch's float64 reduction, inputs read from HBM"]
    kernel_rates(lines, res)

    lines += ["", "mobilenet_v2_bn after fold + CLE: output SQNR (dB) of the weight-quantized model against FP, "
                  "over the correction data"]
    for bw in (8, 4):
        q = BC.QuantParams(weight_bw=bw, act_bw=8)
        n = args.batch * args.batches
        fixed = copy.deepcopy(mnet)
        BC.correct_bias(fixed, q, n, data, n)
        before, after = sqnr_db(mnet, mnet, q, data), sqnr_db(mnet, fixed, q, data)
        res["sqnr_db"]["W%d" % bw] = {"before": before, "after": after}
        lines.append("  W%d: %7.2f before bias correction, %7.2f after" % (bw, before, after))

    text = "\n".join(lines)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
