"""FP8 fake-quantization on one MI355X (csrc/fp8.hip), next to the integer kernels in the same run.

  python benchmarks/fp8_quantsim.py [--batch 256] [--reps 7] [--steps 10] [--json OUT]

1. forward: the QDQ work of a ResNet-50 QuantSim forward at batch `--batch` -- the model input and
   the 54 conv/fc outputs per tensor, the 54 weights per channel (axis 0), resident in HBM, one HIP
   graph per data type -- with FP8 (E4M3, maxval = max|x|) and with 8-bit integer (TF encodings)
   quantizers, in Gelem/s. The two graphs alternate, `--reps` times `--steps` replays each.
2. kernel: aimet_fp8_qdq against aimet_qdq_per_tensor (tensor_vec_kernel) at 2^28 elements, and the
   per-channel forms at 256 x 64 x 12544; both move 8 B/element; TB/s and the share of 8 TB/s.
3. init_mse: the fused 111-candidate search (aimet_fp8_absmax + aimet_fp8_mse_search) against a
   plain-torch loop over the same candidates (the cast's definition in torch ops, one candidate at
   a time, all channels at once), on one activation (layer1.0.conv1's output for 32 images) and on
   all 54 weights per channel; the two must choose the same maxvals (counted). Then the search's
   variants: the IEEE divide instead of the reciprocal, and 4 / 8 / 16 elements held per lane.
Every figure is a median of `--reps` alternating runs after a warm one, with the runs' min and max.
Synthetic data: U(0,1) images (seed 1234), random-init ResNet-50 (seed 0).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12   # bytes/s
M = 3


def collect_tensors(model, x):
    """The fp32 forward once; the model input and every conv/fc output stay resident."""
    acts = [("input", x)]
    hooks = []
    for name, mod in model.named_modules():
        if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
            hooks.append(mod.register_forward_hook(
                lambda m, i, o, name=name: acts.append((name, o.detach().contiguous()))))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    weights = [(name, mod.weight.detach().contiguous()) for name, mod in model.named_modules()
               if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear))]
    return acts, weights


def events_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fns, reps, steps):
    """{name: [ms per call] * reps}: one warm round, then `reps` rounds in which the variants take turns."""
    out = {k: [] for k in fns}
    for r in range(reps + 1):
        for k, fn in fns.items():
            ms = events_ms(fn, steps)
            if r:
                out[k].append(ms)
    return out


def summary(ms_list, work=None, unit=None, scale=1.0):
    med = statistics.median(ms_list)
    d = {"ms_median": round(med, 4), "ms_min": round(min(ms_list), 4), "ms_max": round(max(ms_list), 4),
         "runs": len(ms_list)}
    if work is not None:
        d[unit] = round(work / (med * 1e-3) / scale, 3)
        d[unit + "_min"] = round(work / (max(ms_list) * 1e-3) / scale, 3)
        d[unit + "_max"] = round(work / (min(ms_list) * 1e-3) / scale, 3)
    return d


def graph_of(launch, dev):
    stream = torch.cuda.current_stream()
    cap = torch.cuda.Stream(dev)
    cap.wait_stream(stream)
    with torch.cuda.stream(cap):
        launch(ctypes.c_void_p(cap.cuda_stream))          # warm, outside the capture
    stream.wait_stream(cap)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        launch(ctypes.c_void_p(cap.cuda_stream))
    torch.cuda.synchronize()
    return g


# ---- the plain-torch yardstick of init_mse ------------------------------------------------------
def torch_cast(x, maxval, mbits):
    """The cast's definition in torch ops (maxval broadcasts against x)."""
    F = (2.0 - 2.0 ** -mbits) * 2.0 ** (2 ** (7 - mbits) - 1)
    alpha = (maxval.double() / F).float()
    xc = torch.minimum(torch.maximum(x, -maxval), maxval)
    q = xc / alpha
    e = (torch.frexp(q.abs())[1] - 1).clamp_(min=1)
    scale = torch.ldexp(torch.ones_like(q), e - mbits)
    g = (torch.round(q / scale) * scale).clamp_(-F, F)
    return g * alpha


def torch_init_mse(x, axis, mbits):
    """init_mse with plain torch: max|x|, torch.linspace per channel on the host (as the reference
    builds them), 111 casts of the whole tensor, mean squared error, first minimum."""
    if axis is None:
        mx = x.abs().amax().reshape(1)
        dims, shape = list(range(x.dim())), [1] * x.dim()
    else:
        dims = [d for d in range(x.dim()) if d != axis]
        mx = x.abs().amax(dim=dims)
        shape = [1] * x.dim()
        shape[axis] = -1
    cands = torch.stack([torch.linspace(0.1 * m, 1.2 * m, 111) for m in mx.tolist()]).to(x.device).t().contiguous()
    mses = torch.empty_like(cands)
    for i in range(cands.shape[0]):
        xq = torch_cast(x, cands[i].view(shape), mbits)
        mses[i] = ((x - xq) ** 2).mean(dim=dims)
    best = mses.argmin(0)
    return cands.gather(0, best.view(1, -1)).view(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--search-batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-elems", type=int, default=1 << 28)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    from aimet_amd import _native
    from aimet_amd import fp_quantization as F8
    from aimet_amd.libpymo import QuantizationMode, TfEncoding
    from aimet_amd.tensor_quantizer import AimetTensorQuantizer
    from workloads.resnet import resnet50

    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _native.load()
    res = {"device": torch.cuda.get_device_name(0), "mantissa_bits": M, "reps": args.reps, "steps": args.steps,
           "data": "synthetic: U(0,1) 224x224 images (seed 1234), random-init ResNet-50 (seed 0)"}

    model = resnet50(seed=0, device=dev).eval()
    x = torch.rand(args.batch, 3, 224, 224, generator=torch.Generator().manual_seed(1234)).to(dev)
    acts, weights = collect_tensors(model, x)

    # ---- 1. the forward's QDQ work, FP8 and integer ---------------------------------------------
    keep, int_acts, int_ws, fp_acts, fp_ws = [], [], [], [], []
    for _, t in acts:
        o = torch.empty_like(t)
        q = AimetTensorQuantizer(QuantizationMode.QUANTIZATION_TF)
        q.updateStats(t, True)
        enc, _ = q.getEncoding(8, False, False, False)
        table = F8.scale_table(F8.abs_max(t).reshape(1), M)
        keep += [o, table]
        int_acts.append((ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(o.data_ptr()), t.numel(), enc.to_c()))
        fp_acts.append((ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(o.data_ptr()), 1, 1, t.numel(),
                        ctypes.c_void_p(table.data_ptr())))
    for _, w in weights:
        o = torch.empty_like(w)
        C, K = w.shape[0], w[0].numel()
        q = AimetTensorQuantizer(QuantizationMode.QUANTIZATION_TF, num_channels=C)
        q.updateStatsPerChannel(w, 0, True)
        encs, _ = q.getEncoding(8, True, False, False)
        itable = q.channelTable(encs, dev)
        table = F8.scale_table(F8.abs_max(w, True, 0), M)
        keep += [o, itable, table, q]
        int_ws.append((ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(o.data_ptr()), 1, C, K,
                       ctypes.c_void_p(itable.data_ptr())))
        fp_ws.append((ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(o.data_ptr()), 1, C, K,
                      ctypes.c_void_p(table.data_ptr())))
    n_step = sum(t.numel() for _, t in acts) + sum(w.numel() for _, w in weights)

    def launch_int(sp):
        for a, o, n, e in int_acts:
            _native.check(lib.aimet_qdq_per_tensor(a, o, n, ctypes.byref(e), 0, 0, sp))
        for a, o, outer, C, K, tab in int_ws:
            _native.check(lib.aimet_qdq_per_channel(a, o, outer, C, K, tab, 0, 0, sp))

    def launch_fp8(sp):
        for a, o, outer, C, K, tab in fp_acts + fp_ws:
            _native.check(lib.aimet_fp8_qdq(a, o, outer, C, K, tab, M, sp))

    g_int, g_fp8 = graph_of(launch_int, dev), graph_of(launch_fp8, dev)
    ms = alternate({"int8": g_int.replay, "fp8": g_fp8.replay}, args.reps, args.steps)
    res["forward"] = {"batch": args.batch, "elements_per_step": n_step, "launches_per_step": len(acts) + len(weights),
                      "int8": summary(ms["int8"], n_step, "Gelem_s", 1e9),
                      "fp8": summary(ms["fp8"], n_step, "Gelem_s", 1e9)}
    print("forward QDQ, batch %d, %d elements: fp8 %.1f Gelem/s (%.1f .. %.1f)  int8 %.1f Gelem/s (%.1f .. %.1f)" %
          (args.batch, n_step, res["forward"]["fp8"]["Gelem_s"], res["forward"]["fp8"]["Gelem_s_min"],
           res["forward"]["fp8"]["Gelem_s_max"], res["forward"]["int8"]["Gelem_s"],
           res["forward"]["int8"]["Gelem_s_min"], res["forward"]["int8"]["Gelem_s_max"]), flush=True)
    act_for_search = dict(acts)["layer1.0.conv1"][:args.search_batch].contiguous() \
        if "layer1.0.conv1" in dict(acts) else acts[2][1][:args.search_batch].contiguous()
    del keep, int_acts, int_ws, fp_acts, fp_ws, g_int, g_fp8, acts
    torch.cuda.empty_cache()

    # ---- 2. the kernels alone ---------------------------------------------------------------------
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = args.kernel_elems
    xin = torch.randn(n, device=dev)
    out = torch.empty_like(xin)
    enc = TfEncoding()
    enc.min, enc.max, enc.bw = -4.0, 4.0, 8
    enc_c = enc.to_c()
    table = F8.scale_table(torch.tensor([4.0], device=dev), M)
    ms = alternate({
        "int8": lambda: _native.check(lib.aimet_qdq_per_tensor(xin.data_ptr(), out.data_ptr(), n, ctypes.byref(enc_c), 0,
                                                              0, s)),
        "fp8": lambda: _native.check(lib.aimet_fp8_qdq(xin.data_ptr(), out.data_ptr(), 1, 1, n, table.data_ptr(), M, s)),
    }, args.reps, args.steps)
    res["kernel_per_tensor"] = {"elements": n, "bytes": 8 * n}
    for k in ms:
        d = summary(ms[k], 8 * n, "TB_s", 1e12)
        d["of_hbm_peak"] = round(d["TB_s"] * 1e12 / HBM_PEAK, 3)
        res["kernel_per_tensor"][k] = d
    outer, C, K = 256, 64, 12544
    nc = outer * C * K
    enc_list = []
    for c in range(C):
        e = TfEncoding()
        e.min, e.max, e.bw = -3.0 - 0.01 * c, 3.0 + 0.01 * c, 8
        enc_list.append(e)
    qc = AimetTensorQuantizer(QuantizationMode.QUANTIZATION_TF, num_channels=C)
    itable = qc.channelTable(enc_list, dev)
    ctable = F8.scale_table(torch.linspace(3.0, 3.6, C, device=dev), M)
    ms = alternate({
        "int8": lambda: _native.check(lib.aimet_qdq_per_channel(xin.data_ptr(), out.data_ptr(), outer, C, K,
                                                               itable.data_ptr(), 0, 0, s)),
        "fp8": lambda: _native.check(lib.aimet_fp8_qdq(xin.data_ptr(), out.data_ptr(), outer, C, K, ctable.data_ptr(),
                                                       M, s)),
    }, args.reps, args.steps)
    res["kernel_per_channel"] = {"shape": [outer, C, K], "bytes": 8 * nc}
    for k in ms:
        d = summary(ms[k], 8 * nc, "TB_s", 1e12)
        d["of_hbm_peak"] = round(d["TB_s"] * 1e12 / HBM_PEAK, 3)
        res["kernel_per_channel"][k] = d
    for name in ("kernel_per_tensor", "kernel_per_channel"):
        r = res[name]
        print("%s: fp8 %.2f TB/s (%.2f .. %.2f, %.0f%% of 8 TB/s)  int8 %.2f TB/s (%.2f .. %.2f, %.0f%%)" %
              (name, r["fp8"]["TB_s"], r["fp8"]["TB_s_min"], r["fp8"]["TB_s_max"], 100 * r["fp8"]["of_hbm_peak"],
               r["int8"]["TB_s"], r["int8"]["TB_s_min"], r["int8"]["TB_s_max"], 100 * r["int8"]["of_hbm_peak"]),
              flush=True)
    del xin, out
    torch.cuda.empty_cache()

    # ---- 3. init_mse ----------------------------------------------------------------------------
    ws = [w for _, w in weights]
    chosen = {}

    def fused_act():
        chosen["fused_act"] = F8.mse_search(act_for_search, M, False)

    def torch_act():
        chosen["torch_act"] = torch_init_mse(act_for_search, None, M)

    def fused_w():
        chosen["fused_w"] = [F8.mse_search(w, M, True, 0) for w in ws]

    def torch_w():
        chosen["torch_w"] = [torch_init_mse(w, 0, M) for w in ws]

    reps = max(3, args.reps // 2)
    ms = alternate({"fused": fused_act, "torch_loop": torch_act}, reps, 1)
    same_a = int((chosen["fused_act"] == chosen["torch_act"]).sum())
    res["init_mse_activation"] = {"shape": list(act_for_search.shape), "elements": act_for_search.numel(),
                                  "fused": summary(ms["fused"]), "torch_loop": summary(ms["torch_loop"]),
                                  "speedup": round(statistics.median(ms["torch_loop"]) / statistics.median(ms["fused"]), 1),
                                  "same_maxvals": "%d/1" % same_a}
    ms = alternate({"fused": fused_w, "torch_loop": torch_w}, reps, 1)
    total = sum(w.shape[0] for w in ws)
    same_w = sum(int((a == b).sum()) for a, b in zip(chosen["fused_w"], chosen["torch_w"]))
    res["init_mse_weights"] = {"tensors": len(ws), "channels": total, "elements": sum(w.numel() for w in ws),
                               "fused": summary(ms["fused"]), "torch_loop": summary(ms["torch_loop"]),
                               "speedup": round(statistics.median(ms["torch_loop"]) / statistics.median(ms["fused"]), 1),
                               "same_maxvals": "%d/%d" % (same_w, total)}
    for name in ("init_mse_activation", "init_mse_weights"):
        r = res[name]
        print("%s (%d elements): fused %.3f ms (%.3f .. %.3f)  torch loop %.1f ms (%.1f .. %.1f)  x%.1f  same maxvals %s"
              % (name, r["elements"], r["fused"]["ms_median"], r["fused"]["ms_min"], r["fused"]["ms_max"],
                 r["torch_loop"]["ms_median"], r["torch_loop"]["ms_min"], r["torch_loop"]["ms_max"], r["speedup"],
                 r["same_maxvals"]), flush=True)

    # the four launches alone (max|x| and the search, buffers allocated beforehand) on the activation
    na = act_for_search.numel()
    nbytes = ctypes.c_int64()
    _native.call("aimet_fp8_search_workspace", 1, 1, na, ctypes.byref(nbytes))
    wsb = torch.empty(nbytes.value // 4, device=dev)
    mxb, bestb = torch.empty(1, device=dev), torch.empty(1, device=dev)

    def launches(exact):
        def run():
            _native.check(lib.aimet_fp8_absmax(act_for_search.data_ptr(), 1, 1, na, mxb.data_ptr(), wsb.data_ptr(),
                                               nbytes.value, s))
            _native.check(lib.aimet_fp8_mse_search(act_for_search.data_ptr(), 1, 1, na, mxb.data_ptr(), M, exact,
                                                   bestb.data_ptr(), None, None, None, wsb.data_ptr(), nbytes.value, s))
        return run
    ms = alternate({"reciprocal": launches(0), "divide": launches(1)}, reps, args.steps)
    res["search_launches_activation"] = {
        k: dict(summary(v), Gcasts_s=round(na * 111 / (statistics.median(v) * 1e-3) / 1e9, 1)) for k, v in ms.items()}
    print("search launches alone, activation: " + "  ".join(
        "%s %.3f ms (%.0f G casts/s)" % (k, v["ms_median"], v["Gcasts_s"])
        for k, v in res["search_launches_activation"].items()), flush=True)

    # the search's variants on the same two inputs (the Python calls as a user makes them)
    variants = {}

    def variant(elems, exact):
        def run():
            prev = ctypes.c_int()
            _native.call("aimet_fp8_search_elems", elems, ctypes.byref(prev))
            try:
                F8.mse_search(act_for_search, M, False, exact_divide=exact)
                for w in ws:
                    F8.mse_search(w, M, True, 0, exact_divide=exact)
            finally:
                _native.call("aimet_fp8_search_elems", prev.value, None)
        return run
    for elems in (4, 8, 16):
        for exact in (False, True):
            variants["elems%d_%s" % (elems, "divide" if exact else "reciprocal")] = variant(elems, exact)
    ms = alternate(variants, reps, 1)
    res["search_variants_ms"] = {k: summary(v) for k, v in ms.items()}
    print("search variants, activation + all weights, ms: " +
          "  ".join("%s %.3f" % (k, v["ms_median"]) for k, v in res["search_variants_ms"].items()), flush=True)

    print(json.dumps({"metric": "fp8 fake-quant Gelem/s (ResNet-50 forward QDQ)", "value": res["forward"]["fp8"]["Gelem_s"],
                      "int8": res["forward"]["int8"]["Gelem_s"],
                      "kernel_TB_s": res["kernel_per_tensor"]["fp8"]["TB_s"],
                      "init_mse_weights_speedup": res["init_mse_weights"]["speedup"]}))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
