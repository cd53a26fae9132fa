"""Blockwise and LPBQ weight calibration + QDQ: the fused launch against torch ops and the per-channel route.

    python benchmarks/blockwise_llama.py [--runs 5] [--dtypes bf16,fp32] [--out FILE]

One Llama-3-8B block's seven linear weights (q, k, v, o: 4096 -> 4096 / 1024 / 1024 / 4096; gate, up:
4096 -> 14336; down: 14336 -> 4096), 4-bit symmetric, block size 64, plain and LPBQ (decompressed_bw 8),
in bfloat16 and float32, on one GPU. Calibration plus quantize-dequantize of the seven weights:
  fused     one aimet_bq_encode_qdq launch a weight (aimet_amd.blockwise.encode_qdq);
  torch     the same result from torch ops: amin / amax on the [R, NB, BL] view, the encoding arithmetic
            in float64, the LPBQ compression, the QDQ in float32 (compared with the fused output: reported);
  channel   what the sim offered before: a per-channel static-grid quantizer on the weight reshaped
            to [R NB, BL], one host encoding object a block. The smallest linear (k_proj) only, plain
            only (it has no LPBQ step), its three phases apart: statistics, encodings (device search,
            host objects), QDQ (host table build + kernel).
Medians of `--runs` alternating runs with min and max (device-synchronised host clock). The kernel
alone: time per call between two events over back-to-back launches, and the bytes it has to move
(the weight in and out, the table, q and factor) over that time as a share of the MI355X's 8 TB/s.
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

from aimet_amd import blockwise as B  # noqa: E402
from aimet_amd.quantizers import QuantScheme, StaticGridPerChannelQuantizer  # noqa: E402

HIDDEN, KV, FFN = 4096, 1024, 14336
LINEARS = (("q_proj", HIDDEN, HIDDEN), ("k_proj", HIDDEN, KV), ("v_proj", HIDDEN, KV), ("o_proj", HIDDEN, HIDDEN),
           ("gate_proj", HIDDEN, FFN), ("up_proj", HIDDEN, FFN), ("down_proj", FFN, HIDDEN))
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
BW, BLOCK, DECOMPRESSED = 4, 64, 8
HBM_BYTES_PER_S = 8e12


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return {"ms": statistics.median(v), "min": min(v), "max": max(v)}


def fmt(s):
    return "%9.3f [%9.3f .. %9.3f]" % (s["ms"], s["min"], s["max"])


def torch_route(w, sbw, out):
    """Symmetric (signed) blockwise calibration + QDQ of w [R, fin] from torch ops; (table, out)."""
    R, fin = w.shape
    v = w.view(R, fin // BLOCK, BLOCK)
    lo = v.amin(2).double().clamp(max=0.0)
    hi = v.amax(2).double().clamp(min=0.0)
    hi = torch.maximum(hi, lo + 0.01)
    pos, offset = float(2 ** (BW - 1) - 1), -float(2 ** (BW - 1))
    delta = torch.maximum(hi.abs(), lo.abs()) / pos
    mn, mx = offset * delta, delta * pos
    if sbw:
        factor = delta.amax(1, keepdim=True) / 2 ** sbw
        delta = torch.round(delta / factor).clamp(1, 2 ** sbw) * factor
        mn, mx = delta * offset, (2 ** BW - 1 + offset) * delta
    table = torch.stack([mn, mx, delta, torch.full_like(delta, offset)]).float()
    mn, mx, d = (t.unsqueeze(2) for t in table[:3])
    q = torch.minimum(torch.maximum(v.float(), mn), mx) / d - offset
    q = torch.sign(q) * torch.floor(q.abs() + 0.5)   # half away from zero
    out.view_as(v).copy_(d * (q + offset))
    return table.view(4, -1)


def bench_dtype(name, dtype, runs, launches, lines):
    torch.manual_seed(0)
    weights = {n: (torch.randn(fout, fin, device="cuda") * 0.02).to(dtype) for n, fin, fout in LINEARS}
    outs = {n: torch.empty_like(w) for n, w in weights.items()}
    esz = torch.empty(0, dtype=dtype).element_size()
    r = {}
    for form, sbw in (("blockwise", 0), ("lpbq", DECOMPRESSED - BW)):
        def fused():
            for n, w in weights.items():
                B.encode_qdq(w, w.shape[0], w.shape[1] // BLOCK, BLOCK, BW, True, scale_bitwidth=sbw, out=outs[n])

        def plain():
            for n, w in weights.items():
                torch_route(w, sbw, outs[n])

        # the two routes' results, once
        same_table = same_out = True
        table_rel = out_frac = 0.0
        for n, w in weights.items():
            table, _, _ = B.encode_qdq(w, w.shape[0], w.shape[1] // BLOCK, BLOCK, BW, True, scale_bitwidth=sbw,
                                       out=outs[n])
            got = outs[n].clone()
            other = torch_route(w, sbw, outs[n])
            same_table &= bool(torch.equal(table, other))
            same_out &= bool(torch.equal(got, outs[n]))
            table_rel = max(table_rel, float(((table - other).abs() / table.abs().clamp(min=1e-30)).max()))
            out_frac = max(out_frac, float((got != outs[n]).float().mean()))
        fused(), plain()
        f_ms, t_ms = [], []
        for _ in range(runs):
            f_ms.append(timed(fused))
            t_ms.append(timed(plain))
        # the kernel alone: back-to-back launches between two events
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        k_ms = []
        for _ in range(runs):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(launches):
                fused()
            e1.record()
            torch.cuda.synchronize()
            k_ms.append(e0.elapsed_time(e1) / launches)
        nbytes = sum(2 * w.numel() * esz + (16 + (4 if sbw else 0)) * w.numel() // BLOCK + (8 if sbw else 0) * w.shape[0]
                     for w in weights.values())
        f, t, k = spread(f_ms), spread(t_ms), spread(k_ms)
        r[form] = {"fused": f, "torch": t, "torch_over_fused": t["ms"] / f["ms"], "kernels": k, "bytes": nbytes,
                   "fraction_of_8TBs": nbytes / (k["ms"] * 1e-3) / HBM_BYTES_PER_S,
                   "torch_same_table": same_table, "torch_same_output": same_out,
                   "torch_table_max_rel_diff": table_rel, "torch_output_mismatch_fraction": out_frac}
        lines.append("%-4s %-9s seven linears: fused %s   torch ops %s   torch / fused %.2f   kernels alone %s, %.0f MB, "
                     "%.2f of 8 TB/s   torch route bit-equal: table %s (largest relative difference %.1e), output %s (%.1e of the elements differ)"
                     % (name, form, fmt(f), fmt(t), r[form]["torch_over_fused"], fmt(k), nbytes / 1e6,
                        r[form]["fraction_of_8TBs"], same_table, table_rel, same_out, out_frac))
    # the per-channel route on the smallest linear
    w = weights["k_proj"]
    E = w.numel() // BLOCK
    view = w.view(E, BLOCK)

    def fused_small():
        B.encode_qdq(w, w.shape[0], w.shape[1] // BLOCK, BLOCK, BW, True, out=outs["k_proj"])

    phases = {"statistics": [], "encodings": [], "qdq": []}
    small = []
    fused_small()
    for i in range(runs + 1):
        q = StaticGridPerChannelQuantizer(BW, "nearest", QuantScheme.post_training_tf, True, E, True)
        ms = [timed(lambda: q.update_encoding_stats(view)), timed(q.compute_encoding),
              timed(lambda: q.quantize_dequantize(view, "nearest"))]
        if i:   # the first round warms up
            for key, v in zip(phases, ms):
                phases[key].append(v)
            small.append(timed(fused_small))
    total = spread([sum(v) for v in zip(*phases.values())])
    r["per_channel_k_proj"] = {"blocks": E, "total": total, "fused": spread(small),
                               **{k: spread(v) for k, v in phases.items()}}
    lines.append("%-4s k_proj alone (%d blocks): per-channel quantizer %s = statistics %.3f + encodings %.3f + QDQ %.3f"
                 "   fused %s" % (name, E, fmt(total), *[statistics.median(v) for v in phases.values()],
                                  fmt(r["per_channel_k_proj"]["fused"])))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--kernel-launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    result = {"runs": a.runs, "device": torch.cuda.get_device_name(0), "bitwidth": BW, "block_size": BLOCK}
    lines = ["%s; milliseconds, median [min .. max] of %d alternating runs" % (result["device"], a.runs)]
    for name in a.dtypes.split(","):
        result[name] = bench_dtype(name, DTYPES[name], a.runs, a.kernel_launches, lines)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n" + json.dumps(result, sort_keys=True) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
