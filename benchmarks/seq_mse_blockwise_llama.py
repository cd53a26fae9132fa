"""Blockwise Sequential MSE on one Llama-3-8B block: the seven linears at W4 symmetric, block size
64, 20 candidates, 2 batches of 2048 tokens of synthetic data (weights N(0, 0.02), inputs N(0, 1)).

  python benchmarks/seq_mse_blockwise_llama.py [--runs 5] [--loop k_proj,down_proj] [--json OUT]

Per linear, `--runs` alternating runs each, medians with [min .. max] (device events):
  fused    the search of aimet_amd.seq_mse on a blockwise quantizer: the candidates' tables, one
           aimet_bq_seqmse_losses launch a batch, the first minimum per (row, block);
  kernel   one such launch alone, with its fp32 TFLOP/s from 2 T R K_in (n + 1);
  channel  the existing per-channel search (SequentialMse._candidate_losses) on the same weights;
  loop     (the linears of --loop only: it is very slow) the reference's literal per-block loop in
           plain torch: per candidate a QDQ of W, per block and batch two F.linear of K = 64 slices
           and mse_loss(reduction="none").sum(0). It must choose the fused route's candidates
           (blocks whose best two losses are within 1e-5 relative are not counted).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LINEARS = (("q_proj", 4096, 4096), ("k_proj", 4096, 1024), ("v_proj", 4096, 1024), ("o_proj", 4096, 4096),
           ("gate_proj", 4096, 14336), ("up_proj", 4096, 14336), ("down_proj", 14336, 4096))
CFG = {"defaults": {"ops": {"is_output_quantized": "True"}, "params": {"is_quantized": "True", "is_symmetric": "True"},
                    "strict_symmetric": "False", "per_channel_quantization": "True"}}
BS, N_CAND = 64, 20


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--loop", default="k_proj,down_proj")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from aimet_amd import _native, blockwise, seq_mse
    from aimet_amd.libpymo import RoundingMode
    from aimet_amd.quantsim import QuantizationSimModel
    from aimet_amd.seq_mse import SeqMseParams, SequentialMse
    from aimet_amd.tensor_quantizer import qdq_per_channel_table
    params = SeqMseParams(num_batches=args.batches, num_candidates=N_CAND)
    results = {"tokens": args.tokens, "batches": args.batches, "runs": args.runs, "block_size": BS, "linears": {}}
    for name, K, R in LINEARS:
        torch.manual_seed(0)
        model = nn.Sequential(nn.Linear(K, R, bias=False)).eval().cuda()
        with torch.no_grad():
            model[0].weight.normal_(0, 0.02)
        x = torch.randn(args.batches, args.tokens, K, device="cuda")
        sim_c = QuantizationSimModel(model, quant_scheme="tf", default_param_bw=4, config_file=CFG)
        sim_b = QuantizationSimModel(model, quant_scheme="tf", default_param_bw=4, config_file=CFG)
        blockwise.set_blockwise_quantization_for_weights(sim_b, (nn.Linear,), 4, True, BS)
        qm_c, qm_b = sim_c.model[0], sim_b.model[0]
        q = qm_b.param_quantizers["weight"]
        w = model[0].weight.detach()
        tables = {}

        def fused():
            mn, mx = SequentialMse.get_min_and_max_for_candidate_selection(qm_b)
            tables["t"] = SequentialMse._block_candidate_tables(q, SequentialMse.get_candidates(N_CAND, mx, mn))
            total = SequentialMse._block_candidate_losses(qm_b, tables["t"], x, x, params)
            return total, seq_mse._first_argmin(total.reshape(N_CAND, -1))

        def channel():
            mn, mx = SequentialMse.get_per_channel_min_and_max(qm_c)
            return seq_mse._first_argmin(SequentialMse._candidate_losses(qm_c, mn, mx, x, x, params))

        def loop():
            total = torch.zeros((N_CAND, R, K // BS), device="cuda")
            for j in range(N_CAND):
                wq = qdq_per_channel_table(w, tables["t"][j], 1, q.num_encodings, BS, RoundingMode.ROUND_NEAREST)
                for b in range(K // BS):
                    cols = slice(b * BS, (b + 1) * BS)
                    for i in range(args.batches):
                        xw = F.linear(x[i][:, cols], w[:, cols])
                        total[j, :, b] += F.mse_loss(F.linear(x[i][:, cols], wq[:, cols]), xw, reduction="none").sum(0)
            return total

        err = torch.empty((N_CAND, R, K // BS), device="cuda")

        def kernel():
            _native.call("aimet_bq_seqmse_losses", x[0].data_ptr(), x[0].data_ptr(), K, w.data_ptr(), args.tokens, R,
                         K // BS, BS, tables["t"].data_ptr(), N_CAND, 0, N_CAND, 0, 0, err.data_ptr(), None,
                         torch.cuda.current_stream().cuda_stream)

        with torch.no_grad():
            with_loop = name in args.loop.split(",")
            ms = {"fused": [], "kernel": [], "channel": [], "loop": []}
            fused(), channel()   # warm-up
            for _ in range(args.runs):
                t, (total, chosen) = timed(fused)
                ms["fused"].append(t)
                ms["kernel"].append(timed(kernel)[0])
                ms["channel"].append(timed(channel)[0])
                if with_loop:
                    t, total_loop = timed(loop)
                    ms["loop"].append(t)
            row = {k: summary(v) for k, v in ms.items() if v}
            row["kernel_tflops"] = 2.0 * args.tokens * R * K * (N_CAND + 1) / (row["kernel"]["median_ms"] * 1e-3) / 1e12
            if with_loop:
                flat = total_loop.reshape(N_CAND, -1)
                top2 = flat.topk(2, 0, largest=False).values
                clear = (top2[1] - top2[0]) > 1e-5 * top2[0].abs()
                row["loop_speedup"] = row["loop"]["median_ms"] / row["fused"]["median_ms"]
                row["blocks_compared"] = int(clear.sum())
                row["blocks_differing"] = int((seq_mse._first_argmin(flat) != chosen)[clear].sum())
            results["linears"][name] = row
            print(name, json.dumps(row), flush=True)
        del model, x, sim_c, sim_b, err, total, tables
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
