"""Quantized recurrent layers: the fused step path against the reference's per-step procedure.

    python benchmarks/recurrent_models.py [--hidden 1024 --steps 256 --batch 32 --runs 5] [--out FILE]

A 2-layer bidirectional LSTM and a GRU of the same size (input = hidden), ACTIVE and ANALYSIS mode, on
one GPU:
  * fused: QcQuantizeRecurrent (one input GEMM per layer; per step one bmm and one aimet_rnn_step launch);
  * plain: the reference's procedure (aimet_torch/v1/qc_quantize_recurrent.py forward) written in plain
    torch operations with the same quantizers: per layer, direction and step a `_VF` cell, this
    project's QDQ (or statistics update) of each state tensor, list appends, then flip, stack and cat.
Medians of `--runs` alternating runs with min and max (device-synchronised host clock), the step
kernel's launch count per forward, and its time per launch (back-to-back launches of the forward's
shape between two events). One JSON line at the end.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from aimet_amd import _native  # noqa: E402
from aimet_amd.libpymo import RoundingMode  # noqa: E402
from aimet_amd.qc_quantize_op import QcQuantizeOpMode  # noqa: E402
from aimet_amd.qc_quantize_recurrent import QcQuantizeRecurrent  # noqa: E402
from aimet_amd.quantizers import QuantScheme  # noqa: E402

CELLS = {"LSTM": torch._VF.lstm_cell, "GRU": torch._VF.gru_cell}


def plain_forward(w, x):
    """The per-step procedure with w's quantizers, parameters and mode; dense [T, B, I] input, no initial state."""
    lstm, mode = w.mode == "LSTM", w._mode
    T, B, _ = x.shape

    def act(q, t):
        if not q.enabled:
            return t
        if mode is QcQuantizeOpMode.ANALYSIS:
            q.update_encoding_stats(t)
            return t
        return q.quantize_dequantize(t, RoundingMode.ROUND_NEAREST)
    params = w._quantized_params()
    inp, hn = x, []
    for layer in range(w.num_layers):
        xq = act(w.input_quantizers["input_l%d" % layer], inp)
        h_q = w.output_quantizers["h_l%d" % layer]
        c_q = w.output_quantizers["c_l%d" % layer] if lstm else None
        outs = []
        for d in range(w.num_directions):
            w_ih, w_hh, *b = (params[n] for n in w._get_param_names(d, layer))
            b_ih, b_hh = b if b else (None, None)
            z = torch.zeros(B, w.hidden_size, device=x.device)
            state = (z, z) if lstm else z
            seq = torch.flip(xq, [0]).clone() if d else xq
            steps = []
            for it in range(T):
                state = CELLS[w.mode](seq[it], state, w_ih, w_hh, b_ih, b_hh)
                state = (act(h_q, state[0]), act(c_q, state[1])) if lstm else act(h_q, state)
                steps.append(state[0] if lstm else state)
            outs.append(torch.stack(steps[::-1] if d else steps))
            hn.append(state)
        inp = torch.cat(outs, 2)
    return inp, hn


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def launch_count(reset=False):
    n = ctypes.c_int64()
    _native.call("aimet_rnn_launch_count", ctypes.byref(n), int(reset))
    return n.value


def step_kernel_time(mode, B, H, launches=2000):
    """Milliseconds per aimet_rnn_step launch of two jobs at [B, H], back to back on one stream."""
    G = 4 if mode == "LSTM" else 3
    dev = "cuda"
    ig, hg = torch.randn(B, 2 * G * H, device=dev), torch.randn(2, B, G * H, device=dev)
    bias = torch.randn(2, 2, G * H, device=dev)
    h, c = torch.zeros(2, 2, B, H, device=dev), torch.zeros(2, 2, B, H, device=dev)
    out = torch.empty(B, 2 * H, device=dev)
    jobs = (_native.RnnStepJobC * 2)()
    for d in range(2):
        j = jobs[d]
        j.ig, j.ig_row_stride, j.hg, j.hg_row_stride = ig.data_ptr() + 4 * d * G * H, 2 * G * H, hg[d].data_ptr(), G * H
        j.b_ih, j.b_hh = bias[d, 0].data_ptr(), bias[d, 1].data_ptr()
        j.h_prev, j.h_next, j.c_prev, j.c_next = h[0, d].data_ptr(), h[1, d].data_ptr(), c[0, d].data_ptr(), c[1, d].data_ptr()
        j.out, j.out_row_stride, j.reverse = out.data_ptr() + 4 * d * H, 2 * H, d
    enc = _native.TfEncodingC(-1.0, 127.0 / 128.0, 1.0 / 128.0, -128.0, 8)
    lib = _native.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(n):
        for _ in range(n):
            _native.check(lib.aimet_rnn_step(0 if mode == "LSTM" else 1, jobs, 2, B, H, 1, 0, B, ctypes.byref(enc), 1,
                                             None, 0, 3, stream))
    run(50)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    run(launches)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    H, T, B = a.hidden, a.steps, a.batch
    lines, result = [], {"hidden": H, "steps": T, "batch": B, "runs": a.runs, "device": torch.cuda.get_device_name(0)}
    lines.append("%s, 2-layer bidirectional, input %d, hidden %d, %d steps, batch %d; milliseconds per forward, "
                 "median [min, max] of %d alternating runs" % (result["device"], H, H, T, B, a.runs))
    for mode, cls in (("LSTM", nn.LSTM), ("GRU", nn.GRU)):
        w = QcQuantizeRecurrent(cls(H, H, num_layers=2, bidirectional=True), 8, 8, "nearest",
                                QuantScheme.post_training_tf).cuda().eval()
        x = torch.randn(T, B, H, device="cuda")
        with torch.no_grad():
            w.set_mode(QcQuantizeOpMode.ANALYSIS)
            w(x)
            w.compute_encoding()
            for op_mode in (QcQuantizeOpMode.ACTIVE, QcQuantizeOpMode.ANALYSIS):
                w.set_mode(op_mode)
                fused_out = w(x)[0]           # warm-up of both paths
                plain_out = plain_forward(w, x)[0]
                diff = float((fused_out - plain_out).abs().max())
                launch_count(reset=True)
                w(x)
                launches = launch_count()
                fused, plain = [], []
                for _ in range(a.runs):
                    fused.append(timed(lambda: w(x)))
                    plain.append(timed(lambda: plain_forward(w, x)))
                key = "%s_%s" % (mode.lower(), op_mode.name.lower())
                result[key] = {"fused_ms": statistics.median(fused), "fused_min": min(fused), "fused_max": max(fused),
                               "plain_ms": statistics.median(plain), "plain_min": min(plain), "plain_max": max(plain),
                               "speedup": statistics.median(plain) / statistics.median(fused),
                               "step_launches": launches, "max_abs_diff": diff}
                r = result[key]
                lines.append("%-5s %-8s fused %8.2f [%8.2f, %8.2f]   plain %8.2f [%8.2f, %8.2f]   plain / fused %.2f   "
                             "step launches %d   largest output difference %.3g"
                             % (mode, op_mode.name, r["fused_ms"], r["fused_min"], r["fused_max"], r["plain_ms"],
                                r["plain_min"], r["plain_max"], r["speedup"], launches, diff))
        k = step_kernel_time(mode, B, H)
        result["%s_step_kernel_us" % mode.lower()] = k * 1e3
        lines.append("%-5s step kernel, two jobs of [%d, %d]: %.2f us per launch (back-to-back launches)"
                     % (mode, B, H, k * 1e3))
        del w
    text = "\n".join(lines) + "\n" + json.dumps(result, sort_keys=True) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
