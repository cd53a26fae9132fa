"""Quantizable multi-head attention: the `fused_core` route (one aimet_attn_core launch, no score tensor)
against the fused softmax route and the literal route.

    python benchmarks/attention_core.py [--runs 5] [--shapes vit,long,xlong] [--out FILE]

One attention block under a QuantizationSimModel built with TRANSFORMER_QUANTIZABLE_TYPES (8-bit,
post_training_tf), self-attention without masks, need_weights=False, ACTIVE mode, no gradient, one GPU:
  * vit:   a ViT-L block's attention, E 1024, 16 heads, L = S = 197, batch 64;
  * long:  E 1024, 16 heads, L = S = 2048, batch 4;
  * xlong: E 1024, 16 heads, L = S = 32768, batch 1, calibrated at L = S = 2048. Its fp32 score tensor is
           64 GiB and a row is longer than aimet_attn_softmax keeps on chip, so only `fused_core` is run;
           the other routes are reported by the bytes of one score tensor, not attempted.
Per shape: milliseconds of one forward on each route between two device events, median [min .. max] of
`--runs` runs that alternate between the routes, and the share of output elements that differ by more than
half a step of out_proj's quantizer from the literal route. Then aimet_attn_core alone on the block's q, k,
v with the three encodings: time per launch between two events over back-to-back launches, and its
3 * 2 * B H L S D matrix FLOPs (the score product is computed twice) over that time as a fraction of the
MI355X's 157.3 TFLOP/s fp32 matrix peak. One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from aimet_amd import transformers as T  # noqa: E402
from aimet_amd.elementwise_ops import TRANSFORMER_QUANTIZABLE_TYPES  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

SHAPES = {"vit": dict(E=1024, H=16, L=197, B=64, calib=197), "long": dict(E=1024, H=16, L=2048, B=4, calib=2048),
          "xlong": dict(E=1024, H=16, L=32768, B=1, calib=2048)}
FP32_MATRIX_FLOPS = 157.3e12


def event_ms(fn, repeat=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(repeat):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeat, out


def spread(v):
    return {"ms": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shapes", default="vit,long,xlong")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    result = {"runs": a.runs, "device": torch.cuda.get_device_name(0)}
    lines = ["%s; milliseconds, median [min .. max] of %d alternating runs" % (result["device"], a.runs)]
    for name in a.shapes.split(","):
        s = SHAPES[name]
        E, H, L, B, D = s["E"], s["H"], s["L"], s["B"], s["E"] // s["H"]
        attn = T.QuantizableMultiheadAttention(E, H).cuda().eval()
        xc = torch.randn(s["calib"], B, E, device="cuda")
        sim = QuantizationSimModel(attn, dummy_input=(xc, xc, xc), quant_scheme="tf",
                                   quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)
        sim.compute_encodings(lambda model, _: model(xc, xc, xc, need_weights=False))
        m = sim.model
        x = xc if L == s["calib"] else torch.randn(L, B, E, device="cuda")
        resident = L <= T.attn_softmax_max_s()
        routes = {"core": (True, True)}
        if resident:
            routes.update({"fused": (False, True), "literal": (False, False)})

        def forward(route):
            m.fused_core, m.fused = routes[route]
            with torch.no_grad():
                return m(x, x, x, need_weights=False)[0]
        n0 = T.attn_core_launch_count()
        outs = {route: forward(route) for route in routes}   # warm-up
        r = result[name] = dict(s, score_tensor_bytes=4 * B * H * L * L,
                                core_launches_per_forward=(T.attn_core_launch_count() - n0))
        if resident:
            step = m.out_proj.output_quantizers[0].encoding.delta
            for route in ("core", "fused"):
                r[route + "_differs_from_literal"] = float(((outs[route] - outs["literal"]).abs() > step / 2)
                                                           .float().mean())
        del outs
        times = {route: [] for route in routes}
        for _ in range(a.runs):
            for route in routes:
                times[route].append(event_ms(lambda: forward(route))[0])
        for route in routes:
            r[route] = spread(times[route])
        fmt = lambda t: "%9.2f [%9.2f .. %9.2f]" % (t["ms"], t["min"], t["max"])   # noqa: E731
        line = "%-5s E %d H %d L=S %d B %d  forward: fused_core %s" % (name, E, H, L, B, fmt(r["core"]))
        if resident:
            line += "   fused %s   literal %s   fused / core %.2f   literal / core %.2f; elements beyond half an " \
                    "out_proj step of literal: core %.4f, fused %.4f" % (
                        fmt(r["fused"]), fmt(r["literal"]), r["fused"]["ms"] / r["core"]["ms"],
                        r["literal"]["ms"] / r["core"]["ms"], r["core_differs_from_literal"],
                        r["fused_differs_from_literal"])
        else:
            line += "   fused: a row of %d exceeds the %d it keeps on chip; literal: one fp32 score tensor is %.0f GiB " \
                    "(several are live), not attempted" % (L, T.attn_softmax_max_s(), r["score_tensor_bytes"] / 2 ** 30)
        lines.append(line)
        encs = [m.matmul_1.output_quantizers[0].encoding, m.softmax.output_quantizers[0].encoding,
                m.matmul_2.output_quantizers[0].encoding]
        del sim, m, attn, x, xc
        torch.cuda.empty_cache()
        q, k, v = (torch.randn(L, B * H, D, device="cuda").transpose(0, 1) for _ in range(3))
        q = q / D ** 0.5
        out = torch.empty(B * H, L, D, device="cuda")
        kernel = lambda: T.attn_core(q, k, v, B, H, None, None, *encs, out=out)   # noqa: E731
        kernel()
        ms = event_ms(kernel, repeat=3 if name == "xlong" else 20)[0]
        flops = 6.0 * B * H * L * L * D
        r["kernel"] = {"ms": ms, "flops": flops, "flops_per_s": flops / (ms * 1e-3),
                       "fraction_of_fp32_matrix_peak": flops / (ms * 1e-3) / FP32_MATRIX_FLOPS}
        lines.append("%-5s aimet_attn_core alone on q [%d, %d, %d], three encodings: %.3f ms per launch, %.3g matrix "
                     "FLOPs, %.2f TFLOP/s = %.3f of the 157.3 TFLOP/s fp32 matrix peak"
                     % (name, B * H, L, D, ms, flops, flops / (ms * 1e-3) / 1e12,
                        r["kernel"]["fraction_of_fp32_matrix_peak"]))
        del q, k, v, out
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n" + json.dumps(result, sort_keys=True) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
