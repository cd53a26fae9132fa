"""GPTVQ on one Llama-3-8B block: the seven linears (q/k/v/o, gate/up/down) at the default parameters
(rows_per_block 32, cols_per_block 256, vector_dim 2, 64 centroids, 100 k-means iterations, 8-bit
codebooks), on synthetic calibration data.

  python benchmarks/gptvq_llama.py [--tokens 2048] [--batches 2] [--runs 3] [--json OUT] [--txt OUT]

Two implementations of GPTVQOptimizer.weight_update on the same GPU, interleaved, `--runs` times each:
  fused  aimet_amd.gptvq (aimet_gptvq_kmeans: all Lloyd iterations of a column block in one launch;
         aimet_gptvq_block_update: the sweep inside a 128-column block in one launch);
  loop   the reference's loop (aimet_torch/gptvq/gptvq_optimizer.py:112-169, utils.py:56-78, 177-241)
         restated below with plain torch ops: per k-means iteration a [G][N][K][D] distance tensor, an
         argmin, a one-hot and an einsum; per `vector_dim` columns a distance, an argmin, a gather, a
         divide, a bmm and two slice updates.
Both share the Hessian, the group quantizer's table, the Cholesky factorisations and the
cross-block GEMM. Reported per module and in total: the Hessian accumulation, and for each path the
k-means, sweep and cross-block GEMM times (host clock around a device synchronise) and the final
Hessian-weighted loss tr((W - W_hat) H (W - W_hat)^T). Then the two lane layouts of
aimet_gptvq_block_update (a wave per row, a lane per row) on one 128-column block, interleaved.
Synthetic data: weights N(0, 0.02), inputs N(0, 1), seed 0.
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
sys.path.insert(0, REPO)

LINEARS = (("q_proj", 4096, 4096), ("k_proj", 4096, 1024), ("v_proj", 4096, 1024), ("o_proj", 4096, 4096),
           ("gate_proj", 4096, 14336), ("up_proj", 4096, 14336), ("down_proj", 14336, 4096))
CFG = {"defaults": {"ops": {"is_output_quantized": "True"}, "params": {"is_quantized": "True", "is_symmetric": "True"},
                    "strict_symmetric": "False", "per_channel_quantization": "True"}}
PHASES = ("kmeans_init", "kmeans", "sweep", "cross_block_gemm", "cholesky")


class Clock:
    """Seconds per phase: a host clock around work that ends in a device synchronise."""

    def __init__(self):
        self.times = {}

    def __call__(self, name):
        return _Phase(self.times, name)


class _Phase:
    def __init__(self, times, name):
        self.times, self.name = times, name

    def __enter__(self):
        torch.cuda.synchronize()
        self.start = time.perf_counter()

    def __exit__(self, *_):
        torch.cuda.synchronize()
        self.times[self.name] = self.times.get(self.name, 0.0) + time.perf_counter() - self.start


def loop_get_assignments(tensor, centroids):
    """utils.py:177-200 without a Hessian weighting."""
    distance = (tensor.unsqueeze(2) - centroids.unsqueeze(1)).pow(2).sum(-1)
    return distance.argmin(-1)


def loop_maximization(tensor, centroids, assignments):
    """utils.py:203-225."""
    centroid_range = torch.arange(centroids.shape[1], device=centroids.device)
    expanded = (assignments.unsqueeze(-1) == centroid_range.view(1, 1, -1)).to(tensor.dtype)
    norm = 1.0 / torch.clip(expanded.sum(1), min=1)
    return torch.einsum("gnd,gnk,gk->gkd", tensor, expanded, norm)


def loop_weight_update(weight, hessian, group_quantizer, params, clock):
    """gptvq_optimizer.py:68-184 in plain torch; returns the rounded weight (on the groups' grid)."""
    from aimet_amd import gptvq
    from aimet_amd.tensor_quantizer import qdq_per_channel_table
    num_rows, num_cols = weight.shape
    rpb, cpb, vector_dim = params.rows_per_block, params.cols_per_block, params.vector_dim
    groups, num_of_centroids = num_rows // rpb, 2 ** params.index_bw
    rounded_weight = weight.clone()
    dead = torch.diag(hessian) == 0
    hessian[dead, dead] = 1
    rounded_weight[:, dead] = 0
    group_quantizer.reset_encoding_stats()
    group_quantizer.update_encoding_stats(rounded_weight.view(groups, -1))
    group_quantizer.compute_encoding()
    table = group_quantizer.channel_table(weight.device)
    with clock("cholesky"):
        damp = gptvq.DAMPENING_PERCENTAGE * torch.mean(torch.diag(hessian))
        diag = torch.arange(num_cols, device=weight.device)
        hessian[diag, diag] += damp
        hessian_inv = gptvq.GPTVQOptimizer.compute_inverse(hessian)
    codebook = None
    for block_start in range(0, num_cols, gptvq.BLOCK_STRIDE):
        block_end = min(block_start + gptvq.BLOCK_STRIDE, num_cols)
        count = block_end - block_start
        block = rounded_weight[:, block_start:block_end]
        error_block = torch.zeros_like(block)
        hinv_block = hessian_inv[block_start:block_end, block_start:block_end]
        for i in range(count):
            if (block_start + i) % cpb == 0:
                with clock("kmeans_init"):
                    data = rounded_weight[:, block_start + i:block_start + i + cpb].reshape(groups, -1, vector_dim)
                    codebook = gptvq.hacky_mahalanobis_init(data, num_of_centroids)
                with clock("kmeans"):
                    for _ in range(params.num_of_kmeans_iterations):
                        codebook = loop_maximization(data, codebook, loop_get_assignments(data, codebook))
                codebook = gptvq.quantize_dequantize_codebook(codebook, group_quantizer, groups)
            if i % vector_dim == 0:
                with clock("sweep"):
                    chunk = block[:, i:i + vector_dim]
                    diagonal = torch.diag(hinv_block)[i:i + vector_dim].unsqueeze(0)
                    sliced = chunk.reshape(groups, -1, vector_dim)
                    indices = loop_get_assignments(sliced, codebook)
                    updated = torch.gather(codebook, dim=1, index=indices.unsqueeze(-1).expand(-1, -1, vector_dim))
                    updated = updated.view(chunk.shape)
                    err = (chunk - updated) / diagonal
                    update = torch.bmm(err.transpose(0, 1).unsqueeze(-1),
                                       hinv_block[i:i + vector_dim, i + vector_dim:].unsqueeze(1)).sum(0)
                    block[:, i:i + vector_dim] = updated
                    block[:, i + vector_dim:] -= update
                    error_block[:, i:i + vector_dim] = err
        with clock("cross_block_gemm"):
            rounded_weight[:, block_end:] -= error_block.matmul(hessian_inv[block_start:block_end, block_end:])
    return qdq_per_channel_table(rounded_weight.contiguous(), table, 1, groups, rpb * num_cols)


def hessian_loss(w0, w_hat, hessian):
    """tr((W - W_hat) H (W - W_hat)^T) in float64, the dead columns of W zeroed as both paths do."""
    w0 = w0.double().clone()
    w0[:, torch.diag(hessian) == 0] = 0
    err = w0 - w_hat.double()
    return float(((err @ hessian.double()) * err).sum())


def spread(values):
    return round(max(values) - min(values), 3)


def layout_study(rows, cols, params, reps):
    """aimet_gptvq_block_update alone on the first 128-column block of a [rows][cols] weight, the two
    lane layouts interleaved: median and spread of `reps` launches (device events), ms."""
    from aimet_amd import _native
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    w0 = (torch.randn((rows, cols), generator=g) * 0.02).to(dev)
    D, K = params.vector_dim, 2 ** params.index_bw
    groups = rows // params.rows_per_block
    codebook = w0[:, :K * D].reshape(rows, K, D)[::params.rows_per_block].contiguous()
    a = torch.randn((cols, cols), generator=g).to(dev)
    hinv = torch.linalg.cholesky(a @ a.T / cols + torch.eye(cols, device=dev), upper=True).contiguous()
    err = torch.empty((rows, 128), device=dev)
    idx = torch.empty((rows, 128 // D), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    times = {1: [], 2: []}
    outs = {}
    for rep in range(reps + 1):
        for layout in (1, 2):
            w = w0.clone()
            _native.call("aimet_gptvq_update_layout", layout, None)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            _native.call("aimet_gptvq_block_update", w.data_ptr(), cols, rows, params.rows_per_block, 0, 0, 128, 128, D, K,
                         codebook.data_ptr(), hinv.data_ptr(), cols, err.data_ptr(), idx.data_ptr(), s)
            stop.record()
            torch.cuda.synchronize()
            if rep:
                times[layout].append(start.elapsed_time(stop))
            outs[layout] = (w, err.clone(), idx.clone())
    _native.call("aimet_gptvq_update_layout", 0, None)
    same = all(torch.equal(x, y) for x, y in zip(outs[1], outs[2]))
    assert groups == codebook.shape[0]
    return {"rows": rows, "cols": cols, "block": 128, "same_bits": same,
            "wave_per_row_ms": {"median": round(statistics.median(times[1]), 4), "spread": spread(times[1])},
            "lane_per_row_ms": {"median": round(statistics.median(times[2]), 4), "spread": spread(times[2])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kmeans-iterations", type=int, default=100)
    ap.add_argument("--scale", type=int, default=1, help="divide every feature size (rehearsal at a small size)")
    ap.add_argument("--modules", default=None, help="comma-separated subset of the seven linears")
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()

    from aimet_amd import gptvq
    from aimet_amd.gptvq import GPTVQOptimizer, GPTVQParameters
    from aimet_amd.quantsim import QuantizationSimModel

    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    g = torch.Generator().manual_seed(0)
    wanted = args.modules.split(",") if args.modules else [n for n, _, _ in LINEARS]
    linears = [(n, fin // args.scale, fout // args.scale) for n, fin, fout in LINEARS if n in wanted]
    block = nn.ModuleDict({n: nn.Linear(fin, fout, bias=False) for n, fin, fout in linears})
    with torch.no_grad():
        for m in block.values():
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.02)
    block = block.eval().to(dev)
    params = GPTVQParameters(None, None, num_of_kmeans_iterations=args.kmeans_iterations)
    sim = QuantizationSimModel(block, quant_scheme="tf", default_param_bw=params.vector_bw, config_file=CFG)
    for _, w in sim.quant_wrappers():
        for q in sim._quantizers_of(w):
            q.enabled = False
    inputs = {fin: torch.randn((args.batches, args.tokens, fin), generator=g).to(dev)
              for fin in sorted({fin for _, fin, _ in linears})}

    result = {"tokens": args.tokens, "batches": args.batches, "runs": args.runs, "scale": args.scale,
              "kmeans_iterations": args.kmeans_iterations, "device": torch.cuda.get_device_name(0), "modules": {}}
    total = {"hessian": 0.0, "fused": {}, "loop": {}}
    for name, fin, fout in linears:
        wrapper = sim.model[name]
        inner = wrapper._module_to_wrap
        w0 = inner.weight.detach().clone()
        x = inputs[fin]
        hessian_s = []
        for run in range(args.runs + 1):
            hessian = torch.zeros((fin, fin), device=dev)
            clock = Clock()
            with clock("hessian"):
                for b in range(args.batches):
                    gptvq.update_hessian(inner, x[b:b + 1], b, 1, hessian)
            if run:
                hessian_s.append(clock.times["hessian"])
        samples = {"fused": [], "loop": []}
        loss = {}
        for run in range(args.runs + 1):                  # run 0 warms every shape up
            for impl in ("fused", "loop"):                # interleaved
                h = hessian.clone()
                torch.cuda.synchronize()
                start = time.perf_counter()
                if impl == "fused":
                    inner.weight.data = w0.clone()
                    GPTVQOptimizer.phase_times = {}
                    GPTVQOptimizer.weight_update(wrapper, params, h)
                    phases, GPTVQOptimizer.phase_times = GPTVQOptimizer.phase_times, None
                    w_hat = inner.weight.detach().clone()
                else:
                    clock = Clock()
                    group_quantizer = GPTVQOptimizer._group_quantizer(wrapper.param_quantizers["weight"],
                                                                      fout // params.rows_per_block)
                    w_hat = loop_weight_update(w0, h, group_quantizer, params, clock)
                    phases = clock.times
                torch.cuda.synchronize()
                phases["total"] = time.perf_counter() - start
                if run:
                    samples[impl].append(phases)
                loss[impl] = hessian_loss(w0, w_hat, hessian)
        inner.weight.data = w0
        row = {"shape": [fout, fin], "hessian_s": {"median": round(statistics.median(hessian_s), 4),
                                                   "spread": spread(hessian_s)}, "loss": loss}
        total["hessian"] += statistics.median(hessian_s)
        for impl in samples:
            row[impl] = {}
            for phase in PHASES + ("total",):
                values = [s.get(phase, 0.0) for s in samples[impl]]
                row[impl][phase + "_s"] = {"median": round(statistics.median(values), 4), "spread": spread(values)}
                total[impl][phase] = total[impl].get(phase, 0.0) + statistics.median(values)
        row["speedup"] = {p: round(row["loop"][p + "_s"]["median"] / max(row["fused"][p + "_s"]["median"], 1e-9), 1)
                          for p in ("kmeans", "sweep", "total")}
        result["modules"][name] = row
        say("%-9s [%5d x %5d]  Hessian %.3f s | k-means fused %.3f s (+-%.3f) loop %.3f s (+-%.3f) x%.1f | sweep fused "
            "%.3f s (+-%.3f) loop %.3f s (+-%.3f) x%.1f | cross-block GEMM fused %.3f s loop %.3f s | total fused %.3f s "
            "loop %.3f s x%.1f | loss fused %.6g loop %.6g" %
            (name, fout, fin, row["hessian_s"]["median"],
             row["fused"]["kmeans_s"]["median"], row["fused"]["kmeans_s"]["spread"],
             row["loop"]["kmeans_s"]["median"], row["loop"]["kmeans_s"]["spread"], row["speedup"]["kmeans"],
             row["fused"]["sweep_s"]["median"], row["fused"]["sweep_s"]["spread"],
             row["loop"]["sweep_s"]["median"], row["loop"]["sweep_s"]["spread"], row["speedup"]["sweep"],
             row["fused"]["cross_block_gemm_s"]["median"], row["loop"]["cross_block_gemm_s"]["median"],
             row["fused"]["total_s"]["median"], row["loop"]["total_s"]["median"], row["speedup"]["total"],
             loss["fused"], loss["loop"]))
    result["block_s"] = {"hessian": round(total["hessian"], 3),
                         "fused": {k: round(v, 3) for k, v in total["fused"].items()},
                         "loop": {k: round(v, 3) for k, v in total["loop"].items()}}
    result["block_speedup"] = {p: round(total["loop"][p] / max(total["fused"][p], 1e-9), 1)
                               for p in ("kmeans", "sweep", "total")}
    say("block: Hessian %.3f s | k-means fused %.3f s loop %.3f s x%.1f | sweep fused %.3f s loop %.3f s x%.1f | "
        "cross-block GEMM fused %.3f s loop %.3f s | total fused %.3f s loop %.3f s x%.1f" %
        (total["hessian"], total["fused"]["kmeans"], total["loop"]["kmeans"], result["block_speedup"]["kmeans"],
         total["fused"]["sweep"], total["loop"]["sweep"], result["block_speedup"]["sweep"],
         total["fused"]["cross_block_gemm"], total["loop"]["cross_block_gemm"],
         total["fused"]["total"], total["loop"]["total"], result["block_speedup"]["total"]))
    result["layout_study"] = [layout_study(r // args.scale, 4096 // args.scale, params, 10) for r in (1024, 4096, 14336)]
    for row in result["layout_study"]:
        say("block_update layouts [%5d rows, one 128-column block]: a wave per row %.4f ms (+-%.3f), a lane per row "
            "%.4f ms (+-%.3f), same bits %s" %
            (row["rows"], row["wave_per_row_ms"]["median"], row["wave_per_row_ms"]["spread"],
             row["lane_per_row_ms"]["median"], row["lane_per_row_ms"]["spread"], row["same_bits"]))
    print(json.dumps({"metric": "gptvq_block_s", "fused": result["block_s"]["fused"]["total"],
                      "loop": result["block_s"]["loop"]["total"], "speedup": result["block_speedup"]["total"]}))
    for path, text in ((args.json, json.dumps(result, indent=1)), (args.txt, "\n".join(lines) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
