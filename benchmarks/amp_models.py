"""Automatic mixed precision on whole models, the SQNR kernel alone and the SQNR callback against the
reference's recorded values, on one GPU.

  python benchmarks/amp_models.py [--batch 16] [--batches 2] [--size 224] [--runs 5]
                                  [--sections models,kernel,callback] [--models resnet50,mobilenet_v2_bn]
                                  [--json OUT] [--txt OUT]

1. choose_mixed_precision on the seeded ResNet-50 and BatchNorm MobileNet-v2 (TF-Enhanced; candidates W8A8,
   W8A16, W16A16 int; both phases score with the SQNR callback on `--batches` x `--batch` images;
   optimized phase 1, binary search), with allowed_accuracy_drop=None and with one finite drop (half way,
   in dB, between the best and the lowest candidate), by two routes on the same GPU, same sim, same data:
     fused    EvalCallbackFactory.sqnr: aimet_amp_sqnr_add per batch, one read-back per evaluation;
     literal  the reference's literal procedure (tests/amp_oracle.py evaluate_sqnr_literal: clone, subtract,
              square twice, two means, float() per batch) as the eval callback of the same algorithm.
   Wall-clock around work that ends in a device synchronise; one warm-up run of each route first, then
   `--runs` timed runs, alternating. Phase times are the algorithm's own (amp_info_list.json).
2. aimet_amp_sqnr_add alone beside the torch expression: device events around `iters` calls; below 1 GiB
   a call the inputs rotate over copies adding up to more than 512 MiB, so every call reads HBM. The
   bytes are those of the two inputs, read once; the peak is 8 TB/s.
3. The callback on the recorded outputs of tests/golden/golden_amp.json against the reference's recorded
   float32 dB values: the largest difference.
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import amp_oracle as O  # noqa: E402
from aimet_amd import _native  # noqa: E402
from aimet_amd.amp import mixed_precision_algo as A  # noqa: E402
from aimet_amd.amp.quantizer_groups import find_quantizer_group  # noqa: E402
from aimet_amd.amp.utils import AMPSearchAlgo  # noqa: E402
from aimet_amd.mixed_precision import choose_mixed_precision  # noqa: E402
from aimet_amd.quant_analyzer import CallbackFunc  # noqa: E402
from aimet_amd.quantizers import QuantizationDataType, QuantScheme  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

DEV = "cuda"
PEAK_TBS = 8.0
INT = QuantizationDataType.int
CANDIDATES = [((8, INT), (8, INT)), ((16, INT), (8, INT)), ((16, INT), (16, INT))]     # W8A8, W8A16, W16A16


class Lines(list):
    """The report: every line is also printed as it is made."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)

    def __iadd__(self, more):
        for line in more:
            self.append(line)
        return self


class Loader(list):
    batch_size = None


def calibrate(model, data):
    with torch.no_grad():
        for x in data:
            model(x)


class LiteralFactory:
    """The reference's EvalCallbackFactory.sqnr in torch ops: the same batches, the same cached fp32
    outputs, _compute_sqnr and a float() per batch."""

    def __init__(self, loader):
        self.loader, self.fp32 = loader, []

    def sqnr(self, num_samples):
        def evaluate(model, _):
            capture = not self.fp32
            total, batch_size = 0.0, self.loader.batch_size or 1
            was = model.training
            model.eval()
            try:
                with torch.no_grad():
                    for i, x in enumerate(self.loader):
                        if i * batch_size >= num_samples:
                            break
                        if capture:
                            with A._all_quantizers_disabled(model):
                                self.fp32.append(model(x))
                        total += O.compute_sqnr_literal(self.fp32[i], model(x))
            finally:
                model.train(was)
            return 10 * np.log10(total / num_samples)
        return CallbackFunc(evaluate)


class Counted:
    """A callback that counts its calls."""

    def __init__(self, callback):
        self.callback, self.calls = callback, 0
        self.func, self.args = self, callback.args

    def __call__(self, model, args):
        self.calls += 1
        return self.callback.func(model, args)


def amp_run(sim, dummy, callback, drop, forward_pass):
    """(seconds, phase-1 s, phase-2 s, evaluations, Pareto list, each group's final candidate)"""
    counted = Counted(callback)
    out_dir = tempfile.mkdtemp(prefix="amp_")
    torch.cuda.synchronize()
    t = time.perf_counter()
    pareto = choose_mixed_precision(sim, dummy, CANDIDATES, counted, counted, drop, out_dir, True, forward_pass,
                                    phase1_optimize=True, amp_search_algo=AMPSearchAlgo.Binary)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t
    info = dict(json.load(open(os.path.join(out_dir, "amp_info_list.json")))) if pareto is not None else {}
    wrappers, groups = find_quantizer_group(sim)
    final = [g.get_candidate(wrappers) for g in groups]
    return {"s": seconds, "phase1_s": 60 * info.get("Phase1 Time", 0.0), "phase2_s": 60 * info.get("Phase2 Time", 0.0),
            "evaluations": counted.calls, "pareto": pareto, "final": final, "groups": len(groups)}


def models_section(lines, res, args):
    from workloads.mobilenet_v2_bn import mobilenet_v2_bn
    from workloads.resnet import resnet50
    makers = {"resnet50": resnet50, "mobilenet_v2_bn": mobilenet_v2_bn}
    g = torch.Generator().manual_seed(0)
    data = Loader(torch.randn(args.batch, 3, args.size, args.size, generator=g).to(DEV) for _ in range(args.batches))
    data.batch_size = args.batch
    samples = args.batch * args.batches
    lines.append("choose_mixed_precision, %s; candidates W8A8, W8A16, W16A16 int; SQNR callback on %d x %d images at "
                 "%dx%d for both phases; optimized phase 1, binary search; s: median [min .. max] of %d alternating "
                 "runs after a warm-up" % (res["device"], args.batches, args.batch, args.size, args.size, args.runs))
    for name in args.models.split(","):
        model = makers[name](device=DEV).eval()
        sim = QuantizationSimModel(model, data[0][:1], quant_scheme=QuantScheme.post_training_tf_enhanced,
                                   default_output_bw=8, default_param_bw=8)
        sim.compute_encodings(calibrate, data)
        forward_pass = CallbackFunc(calibrate, data)
        routes = {"fused": A.EvalCallbackFactory(data).sqnr(samples), "literal": LiteralFactory(data).sqnr(samples)}
        # the finite drop: half way between the best and the lowest candidate, from the fused route's scores
        probe = A.GreedyMixedPrecisionAlgo(sim, data[0][:1], CANDIDATES, routes["fused"], routes["fused"],
                                           tempfile.mkdtemp(prefix="amp_"), True, forward_pass)
        fp32, _ = probe.set_baseline()
        scores = {c: s for s, c in probe._eval_scores}
        lowest = min(scores.values())
        drop = fp32 - (max(scores.values()) + lowest) / 2
        w = {"groups": len(probe.quantizer_groups), "fp32_db": fp32, "finite_drop_db": drop,
             "candidate_db": {str(c): s for c, s in scores.items()}, "runs": {}}
        lines += ["", "%s: %d quantizer groups; fp32 %.3f dB, W8A8 %.3f dB, W8A16 %.3f dB, W16A16 %.3f dB"
                  % (name, w["groups"], fp32, scores[CANDIDATES[0]], scores[CANDIDATES[1]], scores[CANDIDATES[2]])]
        for label, d in (("allowed_accuracy_drop=None", None), ("allowed_accuracy_drop=%.3f dB" % drop, drop)):
            last = {r: amp_run(sim, data[0][:1], cb, d, forward_pass) for r, cb in routes.items()}     # warm-up
            times = {r: {"s": [], "phase1_s": [], "phase2_s": []} for r in routes}
            for _ in range(args.runs):
                for r, cb in routes.items():
                    last[r] = amp_run(sim, data[0][:1], cb, d, forward_pass)
                    for k in times[r]:
                        times[r][k].append(last[r][k])
            same_final = last["fused"]["final"] == last["literal"]["final"]
            same_pareto = [(g, c) for _, _, g, c in last["fused"]["pareto"] or []] == \
                [(g, c) for _, _, g, c in last["literal"]["pareto"] or []]
            lowered = sum(1 for f in last["fused"]["final"] if (8, INT) in f)
            row = {"same_final_candidates": same_final, "same_pareto_entries": same_pareto,
                   "groups_with_an_8_bit_half": lowered}
            lines.append("  %s" % label)
            for r in routes:
                row[r] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times[r].items()}
                row[r]["evaluations"] = last[r]["evaluations"]
                row[r]["pareto_points"] = len(last[r]["pareto"] or [])
                lines.append("    %-8s total %7.2f [%7.2f .. %7.2f]  phase 1 %7.2f [%7.2f .. %7.2f]  phase 2 %6.2f "
                             "[%6.2f .. %6.2f]  %d evaluations, %d Pareto points"
                             % (r, row[r]["s"]["median"], row[r]["s"]["min"], row[r]["s"]["max"],
                                row[r]["phase1_s"]["median"], row[r]["phase1_s"]["min"], row[r]["phase1_s"]["max"],
                                row[r]["phase2_s"]["median"], row[r]["phase2_s"]["min"], row[r]["phase2_s"]["max"],
                                row[r]["evaluations"], row[r]["pareto_points"]))
            overlap = row["fused"]["s"]["max"] >= row["literal"]["s"]["min"] and \
                row["literal"]["s"]["max"] >= row["fused"]["s"]["min"]
            row["ranges_overlap"] = overlap
            lines.append("    literal / fused %.3fx (medians); the two routes' [min .. max] %s; same final candidates: "
                         "%s; same Pareto entries in the same order: %s; %d of %d groups end with an 8-bit half"
                         % (row["literal"]["s"]["median"] / row["fused"]["s"]["median"],
                            "overlap" if overlap else "do not overlap", same_final, same_pareto, lowered, w["groups"]))
            w["runs"][label] = row
        res["workloads"][name] = w
        del sim, model, probe, routes
        torch.cuda.empty_cache()


def kernel_section(lines, res):
    cases = [("32x1000", 32 * 1000, "fp32"), ("16x21x512x512", 16 * 21 * 512 * 512, "fp32"),
             ("2x2048x128256", 2 * 2048 * 128256, "bf16"), ("2^28", 1 << 28, "fp32")]
    dtypes = {"fp32": (torch.float32, 0), "bf16": (torch.bfloat16, 2)}
    lines += ["", "aimet_amp_sqnr_add (both launches of a call) beside the reference's torch expression (_compute_sqnr "
                  "with its float()), inputs read from HBM"]
    for label, n, name in cases:
        dtype, io = dtypes[name]
        nbytes = 2 * n * torch.empty(0, dtype=dtype).element_size()
        copies = 1 if nbytes >= (1 << 30) else min(64, -(-(512 << 20) // nbytes) + 1)
        refs = [torch.randn(n, device=DEV, dtype=dtype) for _ in range(copies)]
        xs = [(r.float() + 0.01 * torch.randn(n, device=DEV)).to(dtype) for r in refs]
        acc = torch.zeros(1, dtype=torch.float64, device=DEV)
        stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
        host = [0.0]

        def ours(i):
            _native.call("aimet_amp_sqnr_add", refs[i % copies].data_ptr(), xs[i % copies].data_ptr(), n, io, O.EPS,
                         acc.data_ptr(), stream())

        def theirs(i):
            host[0] += O.compute_sqnr_literal(refs[i % copies], xs[i % copies])
        row = {"shape": label, "dtype": name, "elements": n, "bytes": nbytes, "rotating_copies": copies}
        for who, fn, iters in (("kernel", ours, max(20, 2 * copies)), ("torch", theirs, max(3, min(copies, 16)))):
            for i in range(min(copies, 4)):
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
        res["sqnr_add"].append(row)
        lines.append("  %-14s %-5s %8.1f MB  kernel %9.1f us [%.1f .. %.1f] %6.3f TB/s (%.3f of %.0f TB/s)   torch %10.1f us "
                     "[%.1f .. %.1f] %6.3f TB/s   torch / kernel %.1fx" %
                     (label, name, nbytes / 1e6, row["kernel"]["us_per_call"], row["kernel"]["min_us"],
                      row["kernel"]["max_us"], row["kernel"]["tb_per_s"], row["kernel"]["of_peak"], PEAK_TBS,
                      row["torch"]["us_per_call"], row["torch"]["min_us"], row["torch"]["max_us"],
                      row["torch"]["tb_per_s"], row["torch"]["us_per_call"] / row["kernel"]["us_per_call"]))
        del refs, xs
        torch.cuda.empty_cache()


def callback_section(lines, res):
    """The callback on the fixture's recorded (fp32, quantized) outputs against the recorded dB values."""
    golden = json.load(open(os.path.join(REPO, "tests", "golden", "golden_amp.json")))["sqnr"]["cases"]

    from aimet_amd.qc_quantize_op import QcQuantizeOpMode, StaticGridQuantWrapper

    class PassThrough(torch.nn.Module):
        """One wrapped Identity in PASSTHROUGH mode: what goes in comes out."""

        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1, device=DEV))
            self.layer = StaticGridQuantWrapper(torch.nn.Identity(), 8, 8, "nearest",
                                                QuantScheme.post_training_tf_enhanced)
            self.layer.set_mode(QcQuantizeOpMode.PASSTHROUGH)

        def forward(self, x):
            return self.layer(x)

    def forward_fn(model, batch):
        """The recorded fp32 output while the quantizers are off, the recorded quantized output otherwise."""
        ref, x = batch
        return model(x if model.layer.output_quantizers[0].enabled else ref)

    lines += ["", "EvalCallbackFactory.sqnr on the recorded outputs of tests/golden/golden_amp.json against the "
                  "reference's recorded float32 values, dB"]
    worst = 0.0
    for c in golden:
        batches = Loader(tuple(torch.from_numpy(np.frombuffer(bytes.fromhex(b[k]), dtype=">f4").astype(np.float32)
                                                .reshape(b["shape"])) for k in ("ref_bits", "x_bits"))
                         for b in c["batches"])
        batches.batch_size = c["batch_size"]
        cb = A.EvalCallbackFactory(batches, forward_fn).sqnr(c["num_samples"])
        got = cb.func(PassThrough(), None)
        n = max(r.numel() for r, _ in batches)
        allowed = 10.0 * math.log10(1.0 + 2 * (n + 4) * 2.0 ** -24)
        worst = max(worst, abs(got - c["db"]))
        res["callback"].append({"case": c["name"], "got_db": got, "recorded_db": c["db"], "allowed_db": allowed})
        lines.append("  %-14s callback %.12f  recorded %.12f  |difference| %.3e (allowed %.3e)"
                     % (c["name"], got, c["db"], abs(got - c["db"]), allowed))
    lines.append("  largest observed difference: %.3e dB" % worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sections", default="models,kernel,callback")
    ap.add_argument("--models", default="resnet50,mobilenet_v2_bn")
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "benchmarks/amp_models.py needs an MI355X"
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "batches": args.batches, "size": args.size,
           "runs": args.runs, "workloads": {}, "sqnr_add": [], "callback": []}
    lines = Lines()
    sections = args.sections.split(",")
    if "models" in sections:
        models_section(lines, res, args)
    if "kernel" in sections:
        kernel_section(lines, res)
    if "callback" in sections:
        callback_section(lines, res)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1, default=str)


if __name__ == "__main__":
    main()
