"""Quantizable multi-head attention: the fused softmax route against the literal route.

    python benchmarks/transformer_mha.py [--runs 5] [--shapes vit,long] [--out FILE]

Two attention blocks under a QuantizationSimModel built with TRANSFORMER_QUANTIZABLE_TYPES (8-bit,
post_training_tf), self-attention without masks, need_weights=False, on one GPU:
  * vit:  a ViT-L block's attention, E 1024, 16 heads, L = S = 197, batch 64;
  * long: E 1024, 16 heads, L = S = 2048, batch 4.
For each, the same module with `fused` on (one bmm and one aimet_attn_softmax launch for matmul_1's
quantizer, the softmax and softmax's quantizer) and off (the children called one by one):
  * ACTIVE: one forward;
  * ANALYSIS: one compute_encodings with a one-forward callback (what a user runs to calibrate);
  * TRAIN: one forward plus backward in ACTIVE mode with a gradient for the input and every weight,
    `fused_backward` on (AttnSoftmax: one launch each way) and off (the default: a gradient takes the
    literal route), with torch.cuda.max_memory_allocated over the step.
Medians of `--runs` alternating runs with min and max (device-synchronised host clock), the largest
output difference between the routes, and aimet_attn_softmax alone on the block's [B H, L, S] tensor:
time per launch between two events over back-to-back launches, and the 8 bytes an element it has to
move (one float32 read, one written) over that time as a fraction of the MI355X's 8 TB/s; the same for
aimet_attn_softmax_backward against its 12 bytes an element (scores and gradient read, gradient written).
  * RL-TRAIN (--rows range_learning): the same block under training_range_learning_with_tf_init, one
    forward plus backward with a gradient for the input, every weight and every range, `fused_backward`
    on (AttnSoftmaxLearned: aimet_attn_softmax_lg and aimet_attn_softmax_lg_backward, one row launch
    each way) and off (the literal route), with the peak memory and the largest differences of the input
    gradient and of the four range gradients of matmul_1 and softmax between the routes; then the two
    kernels alone, as above (8 and 12 bytes an element; the backward's time includes its fold launch).
One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from aimet_amd import transformers as T  # noqa: E402
from aimet_amd.elementwise_ops import TRANSFORMER_QUANTIZABLE_TYPES  # noqa: E402
from aimet_amd.quantizers import QuantScheme  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

SHAPES = {"vit": dict(E=1024, H=16, L=197, B=64), "long": dict(E=1024, H=16, L=2048, B=4)}
HBM_BYTES_PER_S = 8e12


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_alone(B, H, L, S, encodings, launches, backward=False):
    """Milliseconds per aimet_attn_softmax (or _backward) launch on [B H, L, S], out of place, back to back."""
    scores = torch.randn(B * H, L, S, device="cuda") * 3.0
    out = torch.empty_like(scores)
    grad = torch.randn_like(scores) if backward else None
    s_enc, p_enc = ((-8.0, 127.0 / 16.0, 8), (0.0, 255.0 / 256.0, 8)) if encodings else (None, None)

    def run(n):
        for _ in range(n):
            if backward:
                T.attn_softmax_backward(scores, grad, B, H, None, None, s_enc, p_enc, out=out)
            else:
                T.attn_softmax(scores, B, H, None, None, s_enc, p_enc, out=out)
    run(5)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    run(launches)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def learned_kernels_alone(B, H, L, S, launches):
    """Milliseconds per aimet_attn_softmax_lg launch and per aimet_attn_softmax_lg_backward call (the row launch
    and its fold) on [B H, L, S], both quantizers at 8 bits asymmetric, out of place, back to back."""
    scores = torch.randn(B * H, L, S, device="cuda") * 3.0
    grad, out = torch.randn_like(scores), torch.empty_like(scores)
    ends = [torch.tensor([v], device="cuda") for v in (-8.0, 127.0 / 16.0, 0.0, 255.0 / 256.0)]
    grids = [(ends[0], ends[1], 8, False, False, False), (ends[2], ends[3], 8, False, False, False)]
    saved = T.attn_softmax_lg(scores, B, H, None, None, *grids, out=out)[1]
    ms = []
    for run in (lambda: T.attn_softmax_lg(scores, B, H, None, None, *grids, out=out),
                lambda: T.attn_softmax_lg_backward(scores, grad, B, H, None, None, *grids, saved, out=out)):
        for _ in range(5):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / launches)
    return ms


def spread(v):
    return {"ms": statistics.median(v), "min": min(v), "max": max(v)}


def range_learning_train(name, s, runs, lines, launches):
    """The RL-TRAIN row of shape `name` and the two range-learning kernels alone -> its results."""
    E, H, L, B = s["E"], s["H"], s["L"], s["B"]
    attn = T.QuantizableMultiheadAttention(E, H).cuda().eval()
    x = torch.randn(L, B, E, device="cuda")
    sim = QuantizationSimModel(attn, dummy_input=(x, x, x),
                               quant_scheme=QuantScheme.training_range_learning_with_tf_init,
                               quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)
    sim.compute_encodings(lambda model, _: model(x, x, x, need_weights=False))
    m = sim.model
    grad_out = torch.randn(L, B, E, device="cuda")
    ranges = [getattr(getattr(m, w), "output0_encoding_" + e) for w in ("matmul_1", "softmax") for e in ("min", "max")]

    def train(fused_backward):
        m.fused_backward = fused_backward
        m.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        m(xg, xg, xg, need_weights=False)[0].backward(grad_out)
        return xg.grad, [float(p.grad) for p in ranges]
    n0 = T.attn_lg_launch_count()
    g_f, r_f = train(True)
    r = {"launches_per_train_step": [b - a for a, b in zip(n0, T.attn_lg_launch_count())]}
    g_l, r_l = train(False)
    r["grad_max_abs_diff"], r["grad_max_abs"] = float((g_f - g_l).abs().max()), float(g_l.abs().max())
    r["range_grads_fused"], r["range_grads_literal"] = r_f, r_l
    del g_f, g_l
    times, peak = {True: [], False: []}, {}
    for _ in range(runs):
        for fb in (True, False):
            torch.cuda.reset_peak_memory_stats()
            times[fb].append(timed(lambda: train(fb)))
            peak[fb] = torch.cuda.max_memory_allocated()
    r.update({"fused": spread(times[True]), "literal": spread(times[False]),
              "literal_over_fused": statistics.median(times[False]) / statistics.median(times[True]),
              "fused_peak_bytes": peak[True], "literal_peak_bytes": peak[False]})
    f, l = r["fused"], r["literal"]
    lines.append("%-4s E %d H %d L=S %d B %d  %-8s fused %8.2f [%8.2f .. %8.2f]   literal %8.2f [%8.2f .. %8.2f]   "
                 "literal / fused %.2f   peak memory fused %.0f MB, literal %.0f MB"
                 % (name, E, H, L, B, "RL-TRAIN", f["ms"], f["min"], f["max"], l["ms"], l["min"], l["max"],
                    r["literal_over_fused"], peak[True] / 1e6, peak[False] / 1e6))
    lines.append("%-4s range learning: largest input-gradient difference between the routes %.3g of %.3g; range "
                 "gradients (matmul_1 min, max, softmax min, max) fused %s, literal %s; launches per fused training "
                 "step: %d forward, %d backward" % (name, r["grad_max_abs_diff"], r["grad_max_abs"],
                                                    " ".join("%.6g" % v for v in r_f),
                                                    " ".join("%.6g" % v for v in r_l), *r["launches_per_train_step"]))
    m.fused_backward = False
    del sim, m, attn, grad_out
    torch.cuda.empty_cache()
    alone = learned_kernels_alone(B, H, L, L, launches)
    for key, ms, nbytes in zip(("lg_kernel", "lg_backward_kernel"), alone, (8, 12)):
        moved = float(nbytes) * B * H * L * L
        r[key] = {"ms": ms, "bytes": moved, "fraction_of_8TBs": moved / (ms * 1e-3) / HBM_BYTES_PER_S}
        lines.append("%-4s aimet_attn_softmax_%s alone on [%d, %d, %d], both grids: %.3f ms, %.0f MB read + written, "
                     "%.2f of 8 TB/s" % (name, "lg" if nbytes == 8 else "lg_backward (rows and fold)", B * H, L, L, ms,
                                         moved / 1e6, r[key]["fraction_of_8TBs"]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shapes", default="vit,long")
    ap.add_argument("--kernel-launches", type=int, default=50)
    ap.add_argument("--rows", default="static,range_learning")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    result = {"runs": a.runs, "device": torch.cuda.get_device_name(0)}
    lines = ["%s; milliseconds, median [min .. max] of %d alternating runs" % (result["device"], a.runs)]
    for name in a.shapes.split(","):
        s = SHAPES[name]
        E, H, L, B = s["E"], s["H"], s["L"], s["B"]
        if "static" not in a.rows.split(","):
            result[name] = dict(s, elements=B * H * L * L, range_learning_train=range_learning_train(
                name, s, a.runs, lines, a.kernel_launches))
            torch.cuda.empty_cache()
            continue
        attn = T.QuantizableMultiheadAttention(E, H).cuda().eval()
        x = torch.randn(L, B, E, device="cuda")
        sim = QuantizationSimModel(attn, dummy_input=(x, x, x), quant_scheme="tf",
                                   quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)
        m = sim.model

        def forward(model=m):
            with torch.no_grad():
                return model(x, x, x, need_weights=False)[0]

        def calibrate():
            sim.compute_encodings(lambda model, _: model(x, x, x, need_weights=False))

        def with_route(fused, fn):
            m.fused = fused
            return fn()
        calibrate()
        r = result[name] = dict(s, elements=B * H * L * L)
        for mode, fn in (("active", forward), ("analysis", calibrate)):
            if mode == "active":
                n0 = T.attn_launch_count()
                out_f = with_route(True, fn)
                r["launches_per_forward"] = T.attn_launch_count() - n0
                out_l = with_route(False, fn)
                r["max_abs_diff"] = float((out_f - out_l).abs().max())
                r["output_max_abs"] = float(out_l.abs().max())
                del out_f, out_l
            else:
                with_route(True, fn), with_route(False, fn)   # warm-up
            fused, literal = [], []
            for _ in range(a.runs):
                fused.append(timed(lambda: with_route(True, fn)))
                literal.append(timed(lambda: with_route(False, fn)))
            r[mode] = {"fused": spread(fused), "literal": spread(literal),
                       "literal_over_fused": statistics.median(literal) / statistics.median(fused)}
            f, l = r[mode]["fused"], r[mode]["literal"]
            lines.append("%-4s E %d H %d L=S %d B %d  %-8s fused %8.2f [%8.2f .. %8.2f]   literal %8.2f [%8.2f .. %8.2f]   "
                         "literal / fused %.2f" % (name, E, H, L, B, mode.upper(), f["ms"], f["min"], f["max"], l["ms"],
                                                   l["min"], l["max"], r[mode]["literal_over_fused"]))
        lines.append("%-4s largest output difference between the routes (ACTIVE) %.3g of %.3g; aimet_attn_softmax "
                     "launches per fused forward %d" % (name, r["max_abs_diff"], r["output_max_abs"],
                                                        r["launches_per_forward"]))
        m.fused = True
        # a training step in ACTIVE mode (the last compute_encodings left it there)
        grad_out = torch.randn(L, B, E, device="cuda")

        def train(fused_backward, model=m):
            model.fused_backward = fused_backward
            model.zero_grad(set_to_none=True)
            xg = x.clone().requires_grad_(True)
            model(xg, xg, xg, need_weights=False)[0].backward(grad_out)
            return xg.grad
        n0 = (T.attn_launch_count(), T.attn_backward_launch_count())
        g_f = train(True)
        r["launches_per_train_step"] = [T.attn_launch_count() - n0[0], T.attn_backward_launch_count() - n0[1]]
        g_l = train(False)
        r["train_grad_max_abs_diff"], r["train_grad_max_abs"] = float((g_f - g_l).abs().max()), float(g_l.abs().max())
        del g_f, g_l
        times, peak = {True: [], False: []}, {}
        for _ in range(a.runs):
            for fb in (True, False):
                torch.cuda.reset_peak_memory_stats()
                times[fb].append(timed(lambda: train(fb)))
                peak[fb] = torch.cuda.max_memory_allocated()
        r["train"] = {"fused": spread(times[True]), "literal": spread(times[False]),
                      "literal_over_fused": statistics.median(times[False]) / statistics.median(times[True]),
                      "fused_peak_bytes": peak[True], "literal_peak_bytes": peak[False]}
        f, l = r["train"]["fused"], r["train"]["literal"]
        lines.append("%-4s E %d H %d L=S %d B %d  %-8s fused %8.2f [%8.2f .. %8.2f]   literal %8.2f [%8.2f .. %8.2f]   "
                     "literal / fused %.2f   peak memory fused %.0f MB, literal %.0f MB"
                     % (name, E, H, L, B, "TRAIN", f["ms"], f["min"], f["max"], l["ms"], l["min"], l["max"],
                        r["train"]["literal_over_fused"], peak[True] / 1e6, peak[False] / 1e6))
        lines.append("%-4s largest input-gradient difference between the routes %.3g of %.3g; launches per fused "
                     "training step: %d forward, %d backward" % (name, r["train_grad_max_abs_diff"],
                                                                 r["train_grad_max_abs"], *r["launches_per_train_step"]))
        m.fused_backward = False
        del sim, m, attn, grad_out
        torch.cuda.empty_cache()
        for backward, encodings in ((False, True), (False, False), (True, True), (True, False)):
            ms = kernel_alone(B, H, L, L, encodings, a.kernel_launches, backward)
            bytes_moved = (12.0 if backward else 8.0) * B * H * L * L
            key = ("backward_" if backward else "") + ("kernel_both_encodings" if encodings else "kernel_no_encoding")
            r[key] = {"ms": ms, "bytes": bytes_moved, "bytes_per_s": bytes_moved / (ms * 1e-3),
                      "fraction_of_8TBs": bytes_moved / (ms * 1e-3) / HBM_BYTES_PER_S}
            lines.append("%-4s %s alone on [%d, %d, %d], %s: %.3f ms per launch, %.0f MB read + written, "
                         "%.2f TB/s = %.2f of 8 TB/s" % (name, "aimet_attn_softmax_backward" if backward else
                                                         "aimet_attn_softmax", B * H, L, L,
                                                         "both encodings" if encodings else "no encoding", ms,
                                                         bytes_moved / 1e6, r[key]["bytes_per_s"] / 1e12,
                                                         r[key]["fraction_of_8TBs"]))
        torch.cuda.empty_cache()
        if "range_learning" in a.rows.split(","):
            r["range_learning_train"] = range_learning_train(name, s, a.runs, lines, a.kernel_launches)
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n" + json.dumps(result, sort_keys=True) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
