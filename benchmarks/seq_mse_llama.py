"""Sequential MSE on one Llama-3-8B block: the seven linears (q/k/v/o, gate/up/down) at W4
per-channel symmetric, 20 candidates, on synthetic calibration data.

  python benchmarks/seq_mse_llama.py [--tokens 2048] [--batches 2] [--runs 5] [--json OUT]

Two implementations of SequentialMse.optimize_module on the same GPU, interleaved, `--runs` times each:
  fused  aimet_amd.seq_mse (aimet_seqmse_candidate_tables / _candidate_qdq / _recon_sums, one stacked
         GEMM per batch);
  loop   the reference's candidate loop (aimet_torch/v1/seq_mse.py:467-503) restated with plain
         torch ops around the per-candidate quantizer API: per candidate reset / update / compute
         encoding, a full QDQ of W, F.linear for XW and XqWq, mse_loss(reduction="none").sum(0).
Both must choose the same candidates (printed per module). Then, per module shape, each fused stage
alone under device events: the three kernels with the bytes they must move (computed from the
shapes) over their time, and the two GEMMs, to show what the module time is made of.
Synthetic data: weights N(0, 0.02), inputs N(0, 1), seed 0.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12   # bytes/s
LINEARS = (("q_proj", 4096, 4096), ("k_proj", 4096, 1024), ("v_proj", 4096, 1024), ("o_proj", 4096, 4096),
           ("gate_proj", 4096, 14336), ("up_proj", 4096, 14336), ("down_proj", 14336, 4096))
CFG = {"defaults": {"ops": {"is_output_quantized": "True"}, "params": {"is_quantized": "True", "is_symmetric": "True"},
                    "strict_symmetric": "False", "per_channel_quantization": "True"}}


def loop_optimize_module(quant_module, x, xq, params):
    """The reference's optimize_module, candidate by candidate (plain torch + the quantizer API)."""
    from aimet_amd.libpymo import RoundingMode
    from aimet_amd.seq_mse import SequentialMse
    q = quant_module.param_quantizers["weight"]
    per_channel_min, per_channel_max = SequentialMse.get_per_channel_min_and_max(quant_module)
    candidates = SequentialMse.get_candidates(params.num_candidates, per_channel_max, per_channel_min)
    w = quant_module.weight
    total_loss = []
    with torch.no_grad():
        for cand_max, cand_min in candidates:
            SequentialMse.compute_param_encodings(q, cand_min, cand_max)
            wq = q.quantize_dequantize(w, RoundingMode.ROUND_NEAREST)
            loss = torch.zeros(len(cand_max), device=w.device)
            for b in range(params.num_batches):
                xqwq = F.linear(xq[b], wq)
                xw = F.linear(x[b], w)
                C = xqwq.shape[-1]
                loss += F.mse_loss(xqwq.reshape(-1, C), xw.reshape(-1, C), reduction="none").sum(0)
            total_loss.append(loss)
        best = torch.stack(total_loss).min(0, keepdim=True)[1]
        best_max = torch.stack([c[0] for c in candidates]).gather(0, best)[0]
        best_min = torch.stack([c[1] for c in candidates]).gather(0, best)[0]
    SequentialMse.compute_param_encodings(q, best_min, best_max)
    q.freeze_encoding()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stage_times(w, x, n_cand, reps):
    """ms of every fused stage alone for one module and one batch (median of `reps`), with the bytes
    the three kernels must move."""
    from aimet_amd import _native
    C, K = w.shape
    T = x.numel() // K
    s = torch.cuda.current_stream().cuda_stream
    mx = w.abs().amax(1).contiguous()
    tables = torch.empty((n_cand, 4, C), device=w.device)
    wq = torch.empty((n_cand, C, K), device=w.device)
    err = torch.empty((n_cand, C), device=w.device)
    nbytes = ctypes.c_int64(0)
    _native.call("aimet_seqmse_recon_sums_workspace", T, C, 1, n_cand, ctypes.byref(nbytes))
    ws = torch.empty((max(nbytes.value // 4, 1),), device=w.device)
    out = {}

    def med(name, fn, nbytes_moved=None):
        fn()
        ms = statistics.median(timed(fn) for _ in range(reps))
        out[name] = {"ms": round(ms, 4)}
        if nbytes_moved is not None:
            rate = nbytes_moved / (ms * 1e-3)
            out[name].update(bytes=nbytes_moved, TBps=round(rate / 1e12, 3), of_hbm_peak=round(rate / HBM_PEAK, 3))

    med("candidate_tables", lambda: _native.call("aimet_seqmse_candidate_tables", None, mx.data_ptr(), C, n_cand, 4, 1,
                                                 0, 0, tables.data_ptr(), s), 4 * C * (1 + 4 * n_cand))
    med("candidate_qdq", lambda: _native.call("aimet_seqmse_candidate_qdq", w.data_ptr(), wq.data_ptr(), C, K,
                                              tables.data_ptr(), n_cand, 0, n_cand, s), 4 * C * K * (1 + n_cand))
    res = {}

    def gemm_xw():
        res["xw"] = F.linear(x, w)

    def gemm_stacked():
        res["xq"] = F.linear(x, wq.view(n_cand * C, K))

    med("gemm_xw", gemm_xw)
    med("gemm_stacked", gemm_stacked)
    xw, xq = res["xw"].reshape(T, C), res["xq"].reshape(T, n_cand * C)
    med("recon_sums", lambda: _native.call("aimet_seqmse_recon_sums", xw.data_ptr(), xq.data_ptr(), T, C, 1, n_cand, 0,
                                           err.data_ptr(), None, ws.data_ptr(), nbytes.value, s),
        4 * T * C * (1 + n_cand) + 4 * n_cand * C)
    out["gemm_stacked"]["TFLOPs"] = round(2.0 * T * K * C * n_cand / (out["gemm_stacked"]["ms"] * 1e-3) / 1e12, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--candidates", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide every feature size (rehearsal at a small size)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    from aimet_amd.quantsim import QuantizationSimModel
    from aimet_amd.seq_mse import SeqMseParams, SequentialMse

    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    block = nn.ModuleDict({n: nn.Linear(fin // args.scale, fout // args.scale, bias=False) for n, fin, fout in LINEARS})
    with torch.no_grad():
        for m in block.values():
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.02)
    block = block.eval().to(dev)
    sim = QuantizationSimModel(block, quant_scheme="tf", default_param_bw=4, default_output_bw=16, config_file=CFG)
    params = SeqMseParams(num_batches=args.batches, num_candidates=args.candidates)
    inputs = {}
    for fin in sorted({fin // args.scale for _, fin, _ in LINEARS}):
        inputs[fin] = torch.randn((args.batches, args.tokens, fin), generator=g).to(dev)

    result = {"tokens": args.tokens, "batches": args.batches, "candidates": args.candidates, "runs": args.runs,
              "device": torch.cuda.get_device_name(0), "modules": {}}
    impls = (("fused", SequentialMse.optimize_module), ("loop", loop_optimize_module))
    with SequentialMse.temporarily_disable_quantizers(block, sim, None):
        SequentialMse.compute_all_param_encodings(sim)
        total = {"fused": 0.0, "loop": 0.0}
        for name, fin, fout in LINEARS:
            qm = sim.model[name]
            q = qm.param_quantizers["weight"]
            x = inputs[fin // args.scale]
            times, chosen = {"fused": [], "loop": []}, {}
            for run in range(args.runs + 1):          # run 0 warms every shape up
                for impl, fn in impls:                # interleaved
                    q._is_encoding_frozen = False
                    ms = timed(lambda: fn(qm, x, x, params))
                    if run:
                        times[impl].append(ms)
                    chosen[impl] = [e.to_tuple() for e in q.encoding]
            same = sum(a == b for a, b in zip(chosen["fused"], chosen["loop"]))
            row = {"shape": [fout // args.scale, fin // args.scale], "same_encodings": "%d/%d" % (same, len(chosen["loop"]))}
            for impl in times:
                row[impl + "_ms"] = [round(t, 2) for t in times[impl]]
                row[impl + "_ms_median"] = round(statistics.median(times[impl]), 2)
                total[impl] += statistics.median(times[impl])
            row["speedup"] = round(row["loop_ms_median"] / row["fused_ms_median"], 2)
            row["stages"] = stage_times(qm.weight.detach(), x[0], args.candidates, args.runs)
            result["modules"][name] = row
            st = row["stages"]
            print("%-9s [%5d x %5d]  fused %8.2f ms  loop %8.2f ms  x%.2f  same encodings %s" %
                  (name, row["shape"][0], row["shape"][1], row["fused_ms_median"], row["loop_ms_median"],
                   row["speedup"], row["same_encodings"]), flush=True)
            print("          per batch: tables %.3f ms | qdq %.3f ms %.2f TB/s (%.0f%% of 8 TB/s) | XW %.3f ms | "
                  "stacked GEMM %.3f ms (%.0f TFLOP/s) | recon sums %.3f ms %.2f TB/s (%.0f%%)" %
                  (st["candidate_tables"]["ms"], st["candidate_qdq"]["ms"], st["candidate_qdq"]["TBps"],
                   100 * st["candidate_qdq"]["of_hbm_peak"], st["gemm_xw"]["ms"], st["gemm_stacked"]["ms"],
                   st["gemm_stacked"]["TFLOPs"], st["recon_sums"]["ms"], st["recon_sums"]["TBps"],
                   100 * st["recon_sums"]["of_hbm_peak"]), flush=True)
    result["block_ms"] = {k: round(v, 2) for k, v in total.items()}
    result["block_speedup"] = round(total["loop"] / total["fused"], 2)
    print(json.dumps({"metric": "seq_mse_block_ms", "fused": result["block_ms"]["fused"],
                      "loop": result["block_ms"]["loop"], "speedup": result["block_speedup"]}))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
