"""Quantizable multi-head attention: the fused softmax route against the literal route.

    python benchmarks/transformer_mha.py [--runs 5] [--shapes vit,long] [--out FILE]

Two attention blocks under a QuantizationSimModel built with TRANSFORMER_QUANTIZABLE_TYPES (8-bit,
post_training_tf), self-attention without masks, need_weights=False, on one GPU:
  * vit:  a ViT-L block's attention, E 1024, 16 heads, L = S = 197, batch 64;
  * long: E 1024, 16 heads, L = S = 2048, batch 4.
For each, the same module with `fused` on (one bmm and one aimet_attn_softmax launch for matmul_1's
quantizer, the softmax and softmax's quantizer) and off (the children called one by one):
  * ACTIVE: one forward;
  * ANALYSIS: one compute_encodings with a one-forward callback (what a user runs to calibrate).
Medians of `--runs` alternating runs with min and max (device-synchronised host clock), the largest
output difference between the routes, and aimet_attn_softmax alone on the block's [B H, L, S] tensor:
time per launch between two events over back-to-back launches, and the 8 bytes an element it has to
move (one float32 read, one written) over that time as a fraction of the MI355X's 8 TB/s. One JSON line
at the end.
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
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

SHAPES = {"vit": dict(E=1024, H=16, L=197, B=64), "long": dict(E=1024, H=16, L=2048, B=4)}
HBM_BYTES_PER_S = 8e12


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_alone(B, H, L, S, encodings, launches):
    """Milliseconds per aimet_attn_softmax launch on [B H, L, S], out of place, back to back."""
    scores = torch.randn(B * H, L, S, device="cuda") * 3.0
    out = torch.empty_like(scores)
    s_enc, p_enc = ((-8.0, 127.0 / 16.0, 8), (0.0, 255.0 / 256.0, 8)) if encodings else (None, None)

    def run(n):
        for _ in range(n):
            T.attn_softmax(scores, B, H, None, None, s_enc, p_enc, out=out)
    run(5)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    run(launches)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def spread(v):
    return {"ms": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shapes", default="vit,long")
    ap.add_argument("--kernel-launches", type=int, default=50)
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
        del sim, m, attn
        torch.cuda.empty_cache()
        for encodings in (True, False):
            ms = kernel_alone(B, H, L, L, encodings, a.kernel_launches)
            bytes_moved = 8.0 * B * H * L * L
            key = "kernel_both_encodings" if encodings else "kernel_no_encoding"
            r[key] = {"ms": ms, "bytes": bytes_moved, "bytes_per_s": bytes_moved / (ms * 1e-3),
                      "fraction_of_8TBs": bytes_moved / (ms * 1e-3) / HBM_BYTES_PER_S}
            lines.append("%-4s aimet_attn_softmax alone on [%d, %d, %d], %s: %.3f ms per launch, %.0f MB read + written, "
                         "%.2f TB/s = %.2f of 8 TB/s" % (name, B * H, L, L, "both encodings" if encodings else
                                                         "no encoding", ms, bytes_moved / 1e6,
                                                         r[key]["bytes_per_s"] / 1e12, r[key]["fraction_of_8TBs"]))
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n" + json.dumps(result, sort_keys=True) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
