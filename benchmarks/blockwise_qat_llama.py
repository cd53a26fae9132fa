"""Learned blockwise ranges: the block kernels against the per-channel route and torch ops.

    python benchmarks/blockwise_qat_llama.py [--runs 5] [--reps 10] [--out FILE]

One Llama-3-8B block's seven linear weights (q, k, v, o: 4096 -> 4096 / 1024 / 1024 / 4096; gate, up:
4096 -> 14336; down: 14336 -> 4096), 4-bit symmetric, block size 64, float32 weights whose
quantize-dequantized value is consumed in bfloat16 and whose gradient arrives in bfloat16 (a Linear
under autocast), on one GPU. The range-learning forward, backward (grad_x and both range gradients)
and the two together, per weight, three ways:
  block     LearnedGridBlockQuantizeDequantize: one launch each way (aimet_lg_block_forward /
            aimet_lg_block_backward), the casts in the store and the loads;
  channel   what the sim offered for the same numbers before: LearnedGridQuantizeDequantize on the
            [1, E, 64] view with float32 output, then .to(bfloat16) (and its upcast going back);
  torch     the reference's torch ops (calculate_forward_pass, symmetric_gradients) on the [E, 64] view.
Per run each route is called `--reps` times back to back between two device events; medians of
`--runs` alternating runs with min and max, in microseconds per call. The block kernels alone
(the C entries on preallocated buffers): time per launch and the bytes each has to move (x in,
bf16 y out or bf16 grad in and float32 grad_x out, the ranges, the saved encoding, the range
gradients) over that time as a share of the MI355X's 8 TB/s. One JSON line at the end.
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

from aimet_amd import _native  # noqa: E402
from aimet_amd.learned_grid import LearnedGridBlockQuantizeDequantize, LearnedGridQuantizeDequantize  # noqa: E402

HIDDEN, KV, FFN = 4096, 1024, 14336
LINEARS = (("q_proj", HIDDEN, HIDDEN), ("k_proj", HIDDEN, KV), ("v_proj", HIDDEN, KV), ("o_proj", HIDDEN, HIDDEN),
           ("gate_proj", HIDDEN, FFN), ("up_proj", HIDDEN, FFN), ("down_proj", FFN, HIDDEN))
BW, BLOCK = 4, 64
STEPS, HALF = float(2 ** BW - 1), float((2 ** BW - 1) // 2)
HBM_BYTES_PER_S = 8e12


def block_route(w, lo, hi):
    return LearnedGridBlockQuantizeDequantize.apply(w, lo, hi, BLOCK, BW, True, False, False, torch.bfloat16)


def channel_route(w, lo, hi):
    y = LearnedGridQuantizeDequantize.apply(w.view(1, -1, BLOCK), lo, hi, BW, True, False, False, 1)
    return y.to(torch.bfloat16).view(w.shape)


class TorchOps(torch.autograd.Function):
    """calculate_forward_pass + symmetric_gradients (quantsim_straight_through_grad.py:191-328), signed."""

    @staticmethod
    def forward(ctx, w, lo, hi):
        x = w.view(-1, BLOCK)
        delta = (hi / torch.full_like(hi, HALF)).unsqueeze(1)   # a tensor divisor: torch multiplies by 1 / scalar
        offset = -float(-(-(2 ** BW - 1) // 2))
        x_round = torch.round(x / delta) - offset
        x_quant = x_round.clamp(0.0, STEPS)
        mask = x_round.ge(0.0) * x_round.le(STEPS)
        ctx.save_for_backward(x, x_quant.to(torch.uint8), mask, delta)
        ctx.offset = offset
        return ((x_quant + offset) * delta).to(torch.bfloat16).view(w.shape)

    @staticmethod
    def backward(ctx, grad):
        x, x_quant, mask, delta = ctx.saved_tensors
        g = grad.float().view(x.shape)
        gmax = ((x_quant + ctx.offset) * g).sum(1) - (mask * (x / delta) * g).sum(1)
        gmax = gmax / torch.full_like(gmax, HALF)
        return (mask * g).view(grad.shape), -gmax, gmax


ROUTES = {"block": block_route, "channel": channel_route, "torch": lambda w, lo, hi: TorchOps.apply(w, lo, hi)}


def spread(v):
    return {"us": statistics.median(v), "min": min(v), "max": max(v)}


def fmt(s):
    return "%8.1f [%8.1f .. %8.1f]" % (s["us"], s["min"], s["max"])


def event_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def bench_weight(name, fin, fout, runs, reps, lines):
    torch.manual_seed(0)
    w = (torch.randn(fout, fin, device="cuda") * 0.02).requires_grad_(True)
    E = w.numel() // BLOCK
    hi = (w.detach().view(E, BLOCK).abs().amax(1) * 0.8).requires_grad_(True)
    lo = (-hi.detach()).requires_grad_(True)
    g = torch.randn(fout, fin, device="cuda").to(torch.bfloat16)
    leaves = (w, lo, hi)
    phases = {}
    for route, op in ROUTES.items():
        y = op(*leaves)
        phases[route] = {"forward": lambda op=op: op(*leaves),
                         "backward": lambda y=y: torch.autograd.grad(y, leaves, g, retain_graph=True),
                         "both": lambda op=op: torch.autograd.grad(op(*leaves), leaves, g)}
    # the routes' results, once: y and grad_x equal, the range gradients close
    ref = block_route(*leaves)
    ref_g = torch.autograd.grad(ref, leaves, g)
    same = {}
    for route in ("channel", "torch"):
        y = ROUTES[route](*leaves)
        gr = torch.autograd.grad(y, leaves, g)
        same[route] = {"y": bool(torch.equal(y, ref)), "grad_x": bool(torch.equal(gr[0], ref_g[0])),
                       "grad_max_rel": float(((gr[2] - ref_g[2]).abs().max() / ref_g[2].abs().max()))}
    times = {r: {p: [] for p in ("forward", "backward", "both")} for r in ROUTES}
    for r in ROUTES:   # warm up every shape and route
        for fn in phases[r].values():
            fn()
    for _ in range(runs):
        for p in ("forward", "backward", "both"):
            for r in ROUTES:
                times[r][p].append(event_us(phases[r][p], reps))
    # the block kernels alone
    x = w.detach()
    y = torch.empty_like(x, dtype=torch.bfloat16)
    enc = torch.empty(4, E, device="cuda")
    gx, gmin, gmax = torch.empty_like(x), torch.empty(E, device="cuda"), torch.empty(E, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lo_d, hi_d = lo.detach(), hi.detach()

    def k_fwd():
        _native.call("aimet_lg_block_forward", x.data_ptr(), y.data_ptr(), E, BLOCK, 2, lo_d.data_ptr(), hi_d.data_ptr(),
                     BW, 1, 0, 0, enc.data_ptr(), stream)

    def k_bwd():
        _native.call("aimet_lg_block_backward", x.data_ptr(), g.data_ptr(), 2, gx.data_ptr(), E, BLOCK, enc.data_ptr(),
                     STEPS, 0, gmin.data_ptr(), gmax.data_ptr(), stream)

    k_fwd(), k_bwd()
    kernels = {"forward": spread([event_us(k_fwd, 5 * reps) for _ in range(runs)]),
               "backward": spread([event_us(k_bwd, 5 * reps) for _ in range(runs)])}
    n = w.numel()
    nbytes = {"forward": 6 * n + 24 * E, "backward": 10 * n + 24 * E}
    for p, k in kernels.items():
        k["bytes"] = nbytes[p]
        k["fraction_of_8TBs"] = nbytes[p] / (k["us"] * 1e-6) / HBM_BYTES_PER_S
    r = {"blocks": E, "same": same, "kernels": kernels,
         **{route: {p: spread(v) for p, v in t.items()} for route, t in times.items()}}
    for p in ("forward", "backward", "both"):
        lines.append("%-9s %-8s block %s   channel %s   torch %s   channel / block %.2f"
                     % (name, p, fmt(r["block"][p]), fmt(r["channel"][p]), fmt(r["torch"][p]),
                        r["channel"][p]["us"] / r["block"][p]["us"]))
    lines.append("%-9s kernels  forward %s, %.0f MB, %.2f of 8 TB/s   backward %s, %.0f MB, %.2f of 8 TB/s   "
                 "channel route: y %s, grad_x %s equal; torch route: y %s, grad_x %s equal"
                 % (name, fmt(kernels["forward"]), nbytes["forward"] / 1e6, kernels["forward"]["fraction_of_8TBs"],
                    fmt(kernels["backward"]), nbytes["backward"] / 1e6, kernels["backward"]["fraction_of_8TBs"],
                    same["channel"]["y"], same["channel"]["grad_x"], same["torch"]["y"], same["torch"]["grad_x"]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    result = {"runs": a.runs, "reps": a.reps, "device": torch.cuda.get_device_name(0), "bitwidth": BW,
              "block_size": BLOCK}
    lines = ["%s; microseconds per call, median [min .. max] of %d alternating runs of %d calls"
             % (result["device"], a.runs, a.reps)]
    for name, fin, fout in LINEARS:
        result[name] = bench_weight(name, fin, fout, a.runs, a.reps, lines)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n" + json.dumps(result, sort_keys=True) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
