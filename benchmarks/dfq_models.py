"""Data-free quantization on whole models: fold_all_batch_norms on ResNet-50 and equalize_model on the
BatchNorm MobileNet-v2 (workloads/mobilenet_v2_bn.py), on one GPU.

  python benchmarks/dfq_models.py [--runs 7] [--json OUT] [--txt OUT]

Three implementations of the same arithmetic over the same pairs and sets (found once, by the
package's graph search), interleaved, `--runs` times each on a fresh copy of the model:
  fused  aimet_amd (csrc/dfq.hip): one launch for all BN folds, one per CLS set, one per HBF pair,
         in place on the parameters;
  torch  the reference's arithmetic (aimet_common/batch_norm_fold.py:71-97,
         cross_layer_equalization.py:600-729) written with plain torch ops on the same GPU;
  numpy  its live form: every parameter copied device -> host, the arithmetic in numpy, the result
         copied host -> device, one layer at a time.
Reported per workload and path: wall-clock (host clock around work that ends in a device
synchronise; median, min and max over the runs) and launches (fused: the library's launch counter;
torch: aten operators dispatched that are no views, each at least one kernel; numpy: device <-> host
copies). The graph search (torch.fx trace and set rules), which all three share, is timed on its own,
and so are the public entry points end to end. Then, for MobileNet-v2: per-layer SQNR of a
per-tensor 8-bit QDQ of the conv weights (the package's TF min/max encoding and QDQ kernel) after
BN folding alone and after equalize_model: what the transform buys.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch import nn
from torch.utils._python_dispatch import TorchDispatchMode

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from aimet_amd import _dfq  # noqa: E402
from aimet_amd import batch_norm_fold as BNF  # noqa: E402
from aimet_amd import cross_layer_equalization as CLE  # noqa: E402

DEV = "cuda"
_VIEWS = ("view", "reshape", "detach", "alias", "expand", "unsqueeze", "squeeze", "permute", "transpose", "t.",
          "slice", "select", "as_strided", "_unsafe_view", "_reshape_alias", "lift_fresh")


class OpCounter(TorchDispatchMode):
    """aten operators dispatched that are no views: each launches at least one kernel."""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not any(v in str(func) for v in _VIEWS):
            self.n += 1
        return func(*args, **(kwargs or {}))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def ensure_bias(conv):
    if conv.bias is None:
        n = conv.out_features if isinstance(conv, nn.Linear) else conv.out_channels
        conv.bias = nn.Parameter(torch.zeros(n, device=conv.weight.device))


# ---- torch restatement ------------------------------------------------------------------------------
@torch.no_grad()
def torch_fold(pairs):
    for conv, bn in pairs:
        ensure_bias(conv)
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        conv.weight.mul_(scale.view(-1, *([1] * (conv.weight.dim() - 1))))
        conv.bias.copy_(bn.bias - (bn.running_mean - conv.bias) * scale)


def _sanitize(s):
    s = torch.nan_to_num(s, nan=1.0, posinf=1.0)
    return torch.where(s == 0, torch.ones_like(s), s)


@torch.no_grad()
def torch_cls(sets):
    out = []
    for layers in sets:
        w = [m.weight for m in layers]
        r0 = w[0].abs().amax(dim=(1, 2, 3))
        if len(layers) == 2:
            r1 = w[1].abs().amax(dim=(0, 2, 3))
            s = _sanitize(r0 / torch.pow(r0 * r1, 0.5))
            w[0].mul_((1.0 / s).view(-1, 1, 1, 1))
            w[1].mul_(s.view(1, -1, 1, 1))
            if layers[0].bias is not None:
                layers[0].bias.mul_(1.0 / s)
            out.append(s)
        else:
            r1, r2 = w[1].abs().amax(dim=(1, 2, 3)), w[2].abs().amax(dim=(0, 2, 3))
            root = torch.pow(r0 * r1 * r2, 1.0 / 3)
            s12, s23 = _sanitize(r0 / root), _sanitize(root / r2)
            w[0].mul_((1.0 / s12).view(-1, 1, 1, 1))
            w[1].mul_(s12.view(-1, 1, 1, 1)).mul_((1.0 / s23).view(-1, 1, 1, 1))
            w[2].mul_(s23.view(1, -1, 1, 1))
            if layers[0].bias is not None:
                layers[0].bias.mul_(1.0 / s12)
            if layers[1].bias is not None:
                layers[1].bias.mul_(1.0 / s23)
            out.append((s12, s23))
    return out


@torch.no_grad()
def torch_hbf(pairs, bn_of):
    for l1, l2, s, relu in pairs:
        bn = bn_of[l1]
        beta, gamma = bn.bias / s, bn.weight / s
        absorb = torch.clamp(beta - 3 * gamma.abs(), min=0) if relu else beta
        w2d = l2.weight.sum(3).sum(2)
        corr = w2d.reshape(-1) * absorb if w2d.shape[1] == 1 else w2d @ absorb
        l1.bias.sub_(absorb)
        l2.bias.add_(corr)


# ---- numpy with the host round trip -------------------------------------------------------------------
class Copies:
    n = 0


def to_host(t):
    Copies.n += 1
    return t.detach().cpu().numpy()


@torch.no_grad()
def to_dev(param, a):
    Copies.n += 1
    param.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).reshape(param.shape))


def numpy_fold(pairs):
    for conv, bn in pairs:
        ensure_bias(conv)
        gamma, beta, mu = to_host(bn.weight), to_host(bn.bias), to_host(bn.running_mean)
        sigma = to_host(torch.sqrt(bn.running_var + bn.eps))
        w, b = to_host(conv.weight), to_host(conv.bias)
        scale = gamma / sigma
        to_dev(conv.weight, w * scale[:, None, None, None])
        to_dev(conv.bias, beta - (mu - b) * scale)


def _np_sanitize(s):
    s = np.nan_to_num(s, nan=1.0, posinf=1.0)
    s[s == 0.0] = 1.0
    return s


def numpy_cls(sets):
    out = []
    with np.errstate(all="ignore"):
        for layers in sets:
            w = [to_host(m.weight) for m in layers]
            b = [None if m.bias is None else to_host(m.bias) for m in layers[:-1]]
            r0 = np.max(np.abs(w[0]), axis=(1, 2, 3))
            if len(layers) == 2:
                r1 = np.max(np.abs(w[1]), axis=(0, 2, 3))
                s = _np_sanitize(r0 / np.power(r0 * r1, 1.0 / 2))
                to_dev(layers[0].weight, w[0] * (1.0 / s[:, None, None, None]))
                to_dev(layers[1].weight, w[1] * s[None, :, None, None])
                if b[0] is not None:
                    to_dev(layers[0].bias, b[0] * (1.0 / s))
                out.append(s)
            else:
                r1, r2 = np.max(np.abs(w[1]), axis=(1, 2, 3)), np.max(np.abs(w[2]), axis=(0, 2, 3))
                root = np.power(r0 * r1 * r2, 1.0 / 3)
                s12, s23 = _np_sanitize(r0 / root), _np_sanitize(root / r2)
                to_dev(layers[0].weight, w[0] * (1.0 / s12[:, None, None, None]))
                to_dev(layers[1].weight, w[1] * s12[:, None, None, None] * (1.0 / s23[:, None, None, None]))
                to_dev(layers[2].weight, w[2] * s23[None, :, None, None])
                if b[0] is not None:
                    to_dev(layers[0].bias, b[0] * (1.0 / s12))
                if b[1] is not None:
                    to_dev(layers[1].bias, b[1] * (1.0 / s23))
                out.append((s12, s23))
    return out


def numpy_hbf(pairs, bn_of):
    for l1, l2, s, relu in pairs:
        bn = bn_of[l1]
        beta, gamma = to_host(bn.bias) / s, to_host(bn.weight) / s
        absorb = np.maximum(0, beta - 3 * np.abs(gamma)) if relu else beta
        w2d = to_host(l2.weight).sum(3).sum(2)
        corr = w2d.reshape(-1) * absorb if w2d.shape[1] == 1 else np.matmul(w2d, absorb)
        to_dev(l1.bias, to_host(l1.bias) - absorb)
        to_dev(l2.bias, to_host(l2.bias) + corr)


# ---- the workloads ------------------------------------------------------------------------------------
def pair_list(sets, scales, relus):
    out = []
    for layers, s, r in zip(sets, scales, relus):
        if len(layers) == 2:
            out.append((layers[0], layers[1], s, r))
        else:
            out += [(layers[0], layers[1], s[0], r[0]), (layers[1], layers[2], s[1], r[1])]
    return out


def prepared(make):
    """A fresh model on the GPU with its pairs, and (after the ReLU6 replacement and with the
    BatchNorms looked through) its CLS sets and ReLU flags, found before the clock starts."""
    m = make(device=DEV)
    _dfq.replace_modules(m, lambda x: isinstance(x, nn.ReLU6), lambda x: nn.ReLU())
    conv_bn, bn_conv, _ = BNF._find_all_batch_norms_to_fold(m)
    assert not bn_conv
    return m, conv_bn


_SETS = {}


def find_sets(make):
    """The CLS sets (as module names) and ReLU flags of the model as equalize_model sees it after
    folding: ReLU6 replaced, BatchNorms gone. Found once per workload, on a CPU instance."""
    if make not in _SETS:
        probe = make()
        _dfq.replace_modules(probe, lambda x: isinstance(x, nn.ReLU6), lambda x: nn.ReLU())
        _dfq.replace_modules(probe, lambda x: isinstance(x, nn.BatchNorm2d), lambda x: nn.Identity())
        search = CLE.GraphSearchUtils(probe)
        sets = [s for g in search.find_layer_groups_to_scale()
                for s in CLE.GraphSearchUtils.convert_layer_group_to_cls_sets(g)]
        names = {id(mod): name for name, mod in probe.named_modules()}
        _SETS[make] = ([[names[id(layer)] for layer in s] for s in sets],
                       search.is_relu_activation_present_in_cls_sets(sets))
    return _SETS[make]


def drop_bns(m, conv_bn):
    ids = {id(bn) for _, bn in conv_bn}
    _dfq.replace_modules(m, lambda x: id(x) in ids, lambda x: nn.Identity())


def run_fold(make, path):
    m, conv_bn = prepared(make)
    if path == "fused":
        _dfq.launch_count(reset=True)
        t, _ = timed(lambda: BNF._fold_given_batch_norms(m, conv_bn, []))
        return t, _dfq.launch_count()
    if path == "torch":
        with OpCounter() as c:
            t, _ = timed(lambda: torch_fold(conv_bn))
        return t, c.n
    Copies.n = 0
    t, _ = timed(lambda: numpy_fold(conv_bn))
    return t, Copies.n


def run_equalize(make, path):
    """BN fold + CLS + HBF over pairs and sets found beforehand; returns (seconds, launches, model)."""
    m, conv_bn = prepared(make)
    bn_of = {c: b for c, b in conv_bn}
    set_names, relus = find_sets(make)
    sets = [tuple(m.get_submodule(n) for n in s) for s in set_names]

    def fused():
        BNF._fold_given_batch_norms(m, conv_bn, [])
        scales = CLE.CrossLayerScaling.scale_cls_sets(sets)
        infos = CLE.CrossLayerScaling.create_cls_set_info_list(sets, scales, relus)
        CLE.HighBiasFold.bias_fold(infos, bn_of)

    def plain(fold, cls, hbf, host):
        fold(conv_bn)
        scales = cls(sets)
        hbf(pair_list(sets, scales, relus), bn_of)
        if not host:
            drop_bns(m, conv_bn)

    if path == "fused":
        _dfq.launch_count(reset=True)
        t, _ = timed(fused)
        return t, _dfq.launch_count(), m
    if path == "torch":
        with OpCounter() as c:
            t, _ = timed(lambda: plain(torch_fold, torch_cls, torch_hbf, False))
        return t, c.n, m
    Copies.n = 0
    t, _ = timed(lambda: plain(numpy_fold, numpy_cls, numpy_hbf, True))
    drop_bns(m, conv_bn)
    return t, Copies.n, m


def weight_sqnr(m):
    """Per conv layer: SQNR (dB) of the per-tensor 8-bit TF QDQ of its weight."""
    import aimet_amd
    from aimet_amd.libpymo import QuantizationMode, RoundingMode
    out = []
    for name, mod in m.named_modules():
        if isinstance(mod, nn.Conv2d):
            w = mod.weight.detach().contiguous()
            q = aimet_amd.AimetTensorQuantizer(QuantizationMode.QUANTIZATION_TF)
            q.updateStats(w, True)
            enc, _ = q.getEncoding(8, False, False, False)
            y = q.quantizeDequantize(w, enc, RoundingMode.ROUND_NEAREST, True)
            noise = float(((w - y).double() ** 2).sum())
            out.append((name, 10.0 * float(np.log10(float((w.double() ** 2).sum()) / max(noise, 1e-300)))))
    return out


def summary(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "benchmarks/dfq_models.py needs an MI355X"
    from workloads.mobilenet_v2_bn import mobilenet_v2_bn
    from workloads.resnet import resnet50

    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "workloads": {}}
    lines = ["DFQ on whole models, %s, %d runs per path, interleaved (ms: median [min .. max])" %
             (res["device"], args.runs)]
    paths = ("fused", "torch", "numpy")
    for wname, make, runner in (("resnet50 fold_all_batch_norms", resnet50, run_fold),
                                ("mobilenet_v2_bn equalize_model", mobilenet_v2_bn, run_equalize)):
        for p in paths:          # warm-up: code objects, allocator
            runner(make, p)
        times, launches = {p: [] for p in paths}, {}
        for _ in range(args.runs):
            for p in paths:
                r = runner(make, p)
                times[p].append(r[0])
                launches[p] = r[1]
        w = {p: dict(summary(times[p]), launches=launches[p]) for p in paths}
        # what all paths share, and the public entry point end to end
        search, entry = [], []
        for _ in range(args.runs):
            m = make(device=DEV)
            search.append(timed(lambda: BNF._find_all_batch_norms_to_fold(m))[0])
            m = make(device=DEV)
            fn = BNF.fold_all_batch_norms if runner is run_fold else CLE.equalize_model
            entry.append(timed(lambda: fn(m))[0])
        w["fx_pair_search"], w["entry_point"] = summary(search), summary(entry)
        res["workloads"][wname] = w
        lines.append("")
        lines.append(wname)
        unit = {"fused": "kernel launches", "torch": "non-view aten ops", "numpy": "device<->host copies"}
        for p in paths:
            lines.append("  %-6s %8.3f [%8.3f .. %8.3f]   %5d %s" % (p, w[p]["median_ms"], w[p]["min_ms"],
                                                                    w[p]["max_ms"], w[p]["launches"], unit[p]))
        lines.append("  torch / fused %.2fx, numpy / fused %.2fx (medians)" %
                     (w["torch"]["median_ms"] / w["fused"]["median_ms"], w["numpy"]["median_ms"] / w["fused"]["median_ms"]))
        lines.append("  BN pair search on the fx trace (shared): %.3f ms; public entry point end to end: %.3f ms" %
                     (w["fx_pair_search"]["median_ms"], w["entry_point"]["median_ms"]))

    # the three paths agree
    ms = {p: run_equalize(mobilenet_v2_bn, p)[2] for p in paths}
    worst = 0.0
    for p in ("torch", "numpy"):
        for (k, a), (_, b) in zip(ms["fused"].named_parameters(), ms[p].named_parameters()):
            worst = max(worst, float(((a - b).abs().max() / a.abs().max().clamp_min(1e-30))))
    res["max_rel_param_difference_between_paths"] = worst
    lines += ["", "largest parameter difference between the paths, relative to the tensor's range: %.3e" % worst]

    # what the transform buys: per-tensor 8-bit weight SQNR, BN folded vs equalized
    folded = mobilenet_v2_bn(device=DEV)
    BNF.fold_all_batch_norms(folded)
    before, after = weight_sqnr(folded), weight_sqnr(ms["fused"])
    res["sqnr_db"] = [{"layer": n, "folded": a, "equalized": b} for (n, a), (_, b) in zip(before, after)]
    a, b = np.array([v for _, v in before]), np.array([v for _, v in after])
    res["sqnr_summary_db"] = {"folded": {"min": float(a.min()), "median": float(np.median(a)), "mean": float(a.mean())},
                              "equalized": {"min": float(b.min()), "median": float(np.median(b)), "mean": float(b.mean())}}
    lines += ["", "mobilenet_v2_bn: per-tensor 8-bit weight QDQ SQNR (dB), %d conv layers" % len(a),
              "  BN folded only : min %6.2f  median %6.2f  mean %6.2f" % (a.min(), np.median(a), a.mean()),
              "  equalize_model : min %6.2f  median %6.2f  mean %6.2f" % (b.min(), np.median(b), b.mean()),
              "  layer                         folded  equalized"]
    lines += ["  %-28s %7.2f %9.2f" % (n, x, y) for (n, x), (_, y) in zip(before, after)]
    text = "\n".join(lines)
    print(text)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
