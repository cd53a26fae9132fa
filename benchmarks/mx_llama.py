"""MX fake-quantization (MXFP8 / MXFP6 / MXFP4): the fused launch against torch ops, and the kernels alone.

    python benchmarks/mx_llama.py [--runs 5] [--dtypes bf16,fp32] [--out FILE]

Three parts, on one GPU:
  block     one Llama-3-8B block's seven linear weights (q, k, v, o: 4096 -> 4096 / 1024 / 1024 / 4096;
            gate, up: 4096 -> 14336; down: 14336 -> 4096) and a 2 x 2048 x 4096 activation, blocks along
            the last axis, in bfloat16 and float32, all five formats:
              fused   one aimet_mx_qdq launch a tensor (aimet_amd.mx.mx_quantize_dequantize);
              torch   the same result from torch ops (abs, amax, frexp, ldexp, round, clamp ...),
                      compared with the fused output once (reported).
            Medians of `--runs` alternating runs with min and max (device-synchronised host clock).
  stream    aimet_mx_qdq alone (row form) at 2^28 elements beside aimet_fp8_qdq (float32, per tensor)
            in the same run, alternating: time per call between two events over back-to-back launches,
            and the bytes a call has to move (8 B/element float32, 4 B/element bfloat16) over that time as a
            share of the MI355X's 8 TB/s.
  column    the column form alone on a 3x3 Conv weight [2048, 2048, 3, 3] (inner = 9) and an NCHW
            activation [64, 256, 56, 56] (inner = 3136), the same way. Reported, not tuned.
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

from aimet_amd import _native, fp_quantization as fp8, mx  # noqa: E402
from aimet_amd.mx import MxFormat  # noqa: E402

HIDDEN, KV, FFN = 4096, 1024, 14336
TENSORS = (("q_proj", (HIDDEN, HIDDEN)), ("k_proj", (KV, HIDDEN)), ("v_proj", (KV, HIDDEN)),
           ("o_proj", (HIDDEN, HIDDEN)), ("gate_proj", (FFN, HIDDEN)), ("up_proj", (FFN, HIDDEN)),
           ("down_proj", (HIDDEN, FFN)), ("activation", (2, 2048, HIDDEN)))
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
SPEC = {MxFormat.MXFP8_E4M3: (3, -6, 8, 448.0), MxFormat.MXFP8_E5M2: (2, -14, 15, 57344.0),
        MxFormat.MXFP6_E3M2: (2, -2, 4, 28.0), MxFormat.MXFP6_E2M3: (3, 0, 2, 7.5),
        MxFormat.MXFP4_E2M1: (1, 0, 2, 6.0)}   # M, emin, emax, max normal
HBM_BYTES_PER_S = 8e12
STREAM_ELEMENTS = 1 << 28


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


def pow2(n):
    """2^n as float32 from the exponent bits, -126 <= n <= 127 (torch.ldexp goes through pow, which
    is not exact on the device, and an error of one ulp moves every rounding tie)."""
    return ((n + 127).to(torch.int32) << 23).view(torch.float32)


def torch_route(x, f, out):
    """MX fake-quantization of x along its last axis from torch ops (finite inputs)."""
    M, emin, emax, maxn = SPEC[f]
    v = x.float().view(-1, 32)
    a = v.abs().amax(1, keepdim=True)
    s = (torch.frexp(a)[1] - 1 - emax).clamp(-127, 127)
    y = v * pow2(-s)
    E = (torch.frexp(y.abs())[1] - 1).clamp(min=emin)
    p = (torch.round(y * pow2(M - E)) * pow2(E - M)).clamp(-maxn, maxn)
    half = s >> 1
    out.copy_(((p * pow2(half)) * pow2(s - half)).view_as(x))


def events(calls, runs, launches):
    """ms per call of each of `calls`, alternating, between two events over back-to-back launches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = [[] for _ in calls]
    for fn in calls:
        fn()
    for _ in range(runs):
        for k, fn in enumerate(calls):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / launches)
    return [spread(v) for v in ms]


def share(nbytes, s):
    return nbytes / (s["ms"] * 1e-3) / HBM_BYTES_PER_S


def bench_block(name, dtype, runs, lines):
    torch.manual_seed(0)
    tensors = {n: (torch.randn(*shape, device="cuda") * (1.0 if n == "activation" else 0.02)).to(dtype)
               for n, shape in TENSORS}
    outs = {n: torch.empty_like(t) for n, t in tensors.items()}
    r = {}
    for f in MxFormat:
        def fused():
            for n, t in tensors.items():
                mx.mx_quantize_dequantize(t, f, out=outs[n])

        def plain():
            for n, t in tensors.items():
                torch_route(t, f, outs[n])

        mismatch = 0.0
        for n, t in tensors.items():
            got = mx.mx_quantize_dequantize(t, f)
            torch_route(t, f, outs[n])
            mismatch = max(mismatch, float((got != outs[n]).float().mean()))
        fused(), plain()
        f_ms, t_ms = [], []
        for _ in range(runs):
            f_ms.append(timed(fused))
            t_ms.append(timed(plain))
        fs, ts = spread(f_ms), spread(t_ms)
        r[f.name] = {"fused": fs, "torch": ts, "torch_over_fused": ts["ms"] / fs["ms"],
                     "torch_output_mismatch_fraction": mismatch}
        lines.append("%-4s %-10s block (7 weights + activation): fused %s   torch ops %s   torch / fused %.1f   "
                     "%.1e of the torch route's elements differ" % (name, f.name, fmt(fs), fmt(ts),
                                                                     r[f.name]["torch_over_fused"], mismatch))
    return r


def bench_stream(runs, launches, lines):
    r = {}
    stream = torch.cuda.current_stream().cuda_stream
    x32 = torch.randn(STREAM_ELEMENTS, device="cuda")
    out32 = torch.empty_like(x32)
    table = fp8.scale_table(x32.abs().amax().reshape(1), 3)

    def fp8_call():
        _native.call("aimet_fp8_qdq", x32.data_ptr(), out32.data_ptr(), 1, 1, STREAM_ELEMENTS, table.data_ptr(), 3,
                     stream)

    for name, dtype in DTYPES.items():
        x = x32.to(dtype).view(-1, HIDDEN)
        out = torch.empty_like(x)
        calls = [(lambda f=f: mx.mx_quantize_dequantize(x, f, out=out)) for f in MxFormat]
        got = events(calls + [fp8_call], runs, launches)
        nbytes = 2 * x.numel() * x.element_size()
        for f, s in zip(MxFormat, got):
            r["%s_%s" % (name, f.name)] = {"kernel": s, "bytes": nbytes, "fraction_of_8TBs": share(nbytes, s)}
            lines.append("%-4s %-10s aimet_mx_qdq row form, 2^28 elements: %s ms a call, %.2f of 8 TB/s"
                         % (name, f.name, fmt(s), share(nbytes, s)))
        s, nb = got[-1], 8 * STREAM_ELEMENTS
        r["%s_run_fp8_qdq_fp32" % name] = {"kernel": s, "bytes": nb, "fraction_of_8TBs": share(nb, s)}
        lines.append("fp32 aimet_fp8_qdq per tensor, 2^28 elements, same run: %s ms a call, %.2f of 8 TB/s"
                     % (fmt(s), share(nb, s)))
        del x, out
    return r


def bench_column(runs, launches, lines):
    r = {}
    for what, shape in (("conv weight, inner 9", (2048, 2048, 3, 3)), ("NCHW activation, inner 3136", (64, 256, 56, 56))):
        for name, dtype in DTYPES.items():
            x = torch.randn(*shape, device="cuda").to(dtype)
            out = torch.empty_like(x)
            (s,) = events([lambda: mx.mx_quantize_dequantize(x, MxFormat.MXFP4_E2M1, axis=1, out=out)], runs, launches)
            nbytes = 2 * x.numel() * x.element_size()
            r["%s_%s" % (name, "x".join(map(str, shape)))] = {"kernel": s, "bytes": nbytes,
                                                             "fraction_of_8TBs": share(nbytes, s)}
            lines.append("%-4s MXFP4_E2M1 column form, %s %s: %s ms a call, %.2f of 8 TB/s"
                         % (name, what, list(shape), fmt(s), share(nbytes, s)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--kernel-launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    result = {"runs": a.runs, "device": torch.cuda.get_device_name(0), "block_size": mx.MX_BLOCK_SIZE}
    lines = ["%s; milliseconds, median [min .. max] of %d alternating runs" % (result["device"], a.runs)]
    for name in a.dtypes.split(","):
        result["block_" + name] = bench_block(name, DTYPES[name], a.runs, lines)
        torch.cuda.empty_cache()
    result["stream"] = bench_stream(a.runs, a.kernel_launches, lines)
    torch.cuda.empty_cache()
    result["column"] = bench_column(a.runs, a.kernel_launches, lines)
    text = "\n".join(lines) + "\n" + json.dumps(result, sort_keys=True) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
