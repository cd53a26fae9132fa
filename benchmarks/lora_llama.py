"""Quantized PEFT LoRA layers: the fused scale / merge route against the literal route.

    python benchmarks/lora_llama.py [--runs 5] [--dtypes bf16,fp32] [--tokens 2x2048] [--out FILE]

One Llama-3-8B block's seven linears (q, k, v, o: 4096 -> 4096 / 1024 / 1024 / 4096; gate, up:
4096 -> 14336; down: 14336 -> 4096), each with one rank-16 adapter (alpha 32), as aimet_amd.peft
LoraLayers under a QuantizationSimModel built with PEFT_QUANTIZABLE_TYPES (8-bit, post_training_tf),
calibrated on the benchmark's input, the base frozen (PeftQuantUtils.freeze_base_model, base weights
without gradient), on 2 x 2048 tokens, in bfloat16 and float32, on one GPU. The same module with
`fused` on (three GEMMs, one aimet_lora_scale and one aimet_lora_merge launch per layer) and off (the
five wrapped children called one by one):
  * forward under no_grad;
  * forward + backward (the input and the adapter weights need gradients).
Medians of `--runs` alternating runs with min and max (device-synchronised host clock), and the largest
output difference between the routes, which must be 0.

The kernels alone at 2^26 elements, set against the literal launches they replace in the same run, time
per call between two events over back-to-back calls, `--runs` alternating rounds:
  * aimet_lora_merge           | three aimet_qdq_per_tensor(_16) and a torch.add
  * aimet_lora_merge_backward  | three aimet_ste_backward*
with the bytes each has to move, counted from the shapes (fused: 3 and 5 passes over the tensor;
literal: 9 and 9), over that time as a share of the MI355X's 8 TB/s. One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from aimet_amd import peft as P  # noqa: E402
from aimet_amd.libpymo import TfEncoding  # noqa: E402
from aimet_amd.quantizers import compute_dloss_by_dx  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402
from aimet_amd.tensor_quantizer import AimetTensorQuantizer  # noqa: E402

HIDDEN, KV, FFN, RANK, ALPHA = 4096, 1024, 14336, 16, 32
LINEARS = (("q_proj", HIDDEN, HIDDEN), ("k_proj", HIDDEN, KV), ("v_proj", HIDDEN, KV), ("o_proj", HIDDEN, HIDDEN),
           ("gate_proj", HIDDEN, FFN), ("up_proj", HIDDEN, FFN), ("down_proj", FFN, HIDDEN))
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
HBM_BYTES_PER_S = 8e12
KERNEL_ELEMENTS = 1 << 26


class PeftLinear(nn.Module):
    """The attributes of peft.tuners.lora.layer.Linear with one adapter (peft itself is not needed)."""

    def __init__(self, fin, fout):
        super().__init__()
        self.base_layer = nn.Linear(fin, fout, bias=False)
        self.lora_A = nn.ModuleDict({"default": nn.Linear(fin, RANK, bias=False)})
        self.lora_B = nn.ModuleDict({"default": nn.Linear(RANK, fout, bias=False)})
        nn.init.normal_(self.lora_B["default"].weight, std=0.02)   # a trained adapter, not PEFT's zero start
        self.lora_dropout = nn.ModuleDict({"default": nn.Identity()})
        self.scaling, self.r, self.lora_alpha = {"default": ALPHA / RANK}, {"default": RANK}, {"default": ALPHA}
        self.active_adapter = ["default"]
        self.in_features, self.out_features = fin, fout


class BlockLinears(nn.Module):
    """The seven adapted linears of one block, each on an input of its own width."""

    def __init__(self):
        super().__init__()
        for name, fin, fout in LINEARS:
            setattr(self, name, PeftLinear(fin, fout))

    def forward(self, x, h):
        return [getattr(self, name)(h if fin == FFN else x) for name, fin, _ in LINEARS]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return {"ms": statistics.median(v), "min": min(v), "max": max(v)}


def told_apart(a, b):
    return a["max"] < b["min"] or b["max"] < a["min"]


def fmt(s):
    return "%9.3f [%9.3f .. %9.3f]" % (s["ms"], s["min"], s["max"])


def module_bench(name, dtype, tokens, runs, lines):
    torch.manual_seed(0)
    model = BlockLinears()
    P.replace_lora_layers_with_quantizable_layers(model)
    model = model.to("cuda", dtype).eval()
    x = torch.randn(*tokens, HIDDEN, device="cuda").to(dtype)
    h = torch.randn(*tokens, FFN, device="cuda").to(dtype)
    with tempfile.TemporaryDirectory() as d:
        meta = P.track_lora_meta_data(model, d, "meta")
    sim = QuantizationSimModel(model, (x, h), quant_scheme="tf", in_place=True,
                               quantizable_types=P.PEFT_QUANTIZABLE_TYPES)
    sim.compute_encodings(lambda m, _: m(x, h), None)
    utils = P.PeftQuantUtils(meta)
    utils.freeze_base_model(sim)
    for n, p in sim.model.named_parameters():
        p.requires_grad_(".lora_A." in n or ".lora_B." in n)
    layers = [m for m in sim.model.modules() if isinstance(m, P.LoraLayer)]
    xg, hg = x.clone().requires_grad_(True), h.clone().requires_grad_(True)

    def route(fused):
        for layer in layers:
            layer.fused = fused

    def forward():
        with torch.no_grad():
            return sim.model(x, h)

    def step():
        for p in sim.model.parameters():
            p.grad = None
        xg.grad = hg.grad = None
        outs = sim.model(xg, hg)
        torch.autograd.backward([o.float().mean() for o in outs])

    r = {"tokens": list(tokens), "dtype": name}
    route(True)
    n0 = P.lora_launch_count()
    out_f = forward()
    r["launches_per_forward"] = P.lora_launch_count() - n0
    route(False)
    n0 = P.lora_launch_count()
    out_l = forward()
    r["launches_per_literal_forward"] = P.lora_launch_count() - n0
    r["max_abs_diff"] = max(float((a.float() - b.float()).abs().max()) for a, b in zip(out_f, out_l))
    r["bit_identical"] = all(torch.equal(a, b) for a, b in zip(out_f, out_l))
    del out_f, out_l
    for mode, fn in (("forward", forward), ("forward_backward", step)):
        for fused in (True, False):   # warm-up of both routes
            route(fused)
            fn()
        fused_ms, literal_ms = [], []
        for _ in range(runs):
            route(True)
            fused_ms.append(timed(fn))
            route(False)
            literal_ms.append(timed(fn))
        f, l = spread(fused_ms), spread(literal_ms)
        r[mode] = {"fused": f, "literal": l, "literal_over_fused": l["ms"] / f["ms"], "told_apart": told_apart(f, l)}
        lines.append("%-4s %d x %d tokens  %-16s fused %s   literal %s   literal / fused %.3f%s"
                     % (name, tokens[0], tokens[1], mode, fmt(f), fmt(l), r[mode]["literal_over_fused"],
                        "" if r[mode]["told_apart"] else "   (spreads overlap: not told apart)"))
    lines.append("%-4s largest output difference between the routes %.3g (bit-identical: %s); aimet_lora launches per "
                 "forward: fused %d, literal %d" % (name, r["max_abs_diff"], r["bit_identical"],
                                                    r["launches_per_forward"], r["launches_per_literal_forward"]))
    route(True)
    return r


def _enc(mn, mx, bw=8):
    e = TfEncoding()
    e.min, e.max, e.bw = mn, mx, bw
    e.delta = (mx - mn) / (2 ** bw - 1)
    e.offset = round(mn / e.delta)
    return e


def kernel_bench(name, dtype, runs, launches, lines):
    n, esz = KERNEL_ELEMENTS, torch.empty(0, dtype=dtype).element_size()
    u = (torch.randn(n, device="cuda") * 3.0).to(dtype)
    v = (torch.randn(n, device="cuda") * 3.0).to(dtype)
    g = torch.randn(n, device="cuda").to(dtype)
    eu, ev, eo = _enc(-9.0, 9.0), _enc(-8.0, 8.5), _enc(-12.0, 12.5)
    t = [torch.empty_like(u) for _ in range(4)]

    def fused_fwd():
        P.lora_merge(u, v, eu, ev, eo, out=t[0])

    def literal_fwd():
        AimetTensorQuantizer.quantize_dequantize_tensor(u, eu, out=t[0])
        AimetTensorQuantizer.quantize_dequantize_tensor(v, ev, out=t[1])
        torch.add(t[0], t[1], out=t[2])
        AimetTensorQuantizer.quantize_dequantize_tensor(t[2], eo, out=t[3])

    def fused_bwd():
        P.lora_merge_backward(u, v, g, eu, ev, eo, grad_u=t[0], grad_v=t[1])

    def literal_bwd():   # t[2] holds the forward's sum
        g1 = compute_dloss_by_dx(t[2], g, eo.min, eo.max)
        compute_dloss_by_dx(u, g1, eu.min, eu.max)
        compute_dloss_by_dx(v, g1, ev.min, ev.max)

    def per_call(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    literal_fwd()
    want = t[3].clone()
    fused_fwd()
    r = {"elements": n, "forward_bit_identical": bool(torch.equal(t[0], want))}
    literal_fwd()   # t[2]: the sum the literal backward masks on
    for key, fused, literal, passes in (("merge", fused_fwd, literal_fwd, (3, 9)),
                                        ("merge_backward", fused_bwd, literal_bwd, (5, 9))):
        for fn in (fused, literal):
            for _ in range(3):
                fn()
        f_ms, l_ms = [], []
        for _ in range(runs):
            f_ms.append(per_call(fused))
            l_ms.append(per_call(literal))
        f, l = spread(f_ms), spread(l_ms)
        fb, lb = passes[0] * esz * n, passes[1] * esz * n
        r[key] = {"fused": f, "literal": l, "literal_over_fused": l["ms"] / f["ms"], "told_apart": told_apart(f, l),
                  "fused_bytes": fb, "literal_bytes": lb,
                  "fused_fraction_of_8TBs": fb / (f["ms"] * 1e-3) / HBM_BYTES_PER_S,
                  "literal_fraction_of_8TBs": lb / (l["ms"] * 1e-3) / HBM_BYTES_PER_S}
        lines.append("%-4s aimet_lora_%-14s 2^26 elements: fused %s ms, %4.0f MB, %.2f of 8 TB/s   literal %s ms, %4.0f MB, "
                     "%.2f of 8 TB/s   literal / fused %.2f%s"
                     % (name, key, fmt(f), fb / 1e6, r[key]["fused_fraction_of_8TBs"], fmt(l), lb / 1e6,
                        r[key]["literal_fraction_of_8TBs"], r[key]["literal_over_fused"],
                        "" if r[key]["told_apart"] else "   (spreads overlap: not told apart)"))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--tokens", default="2x2048")
    ap.add_argument("--kernel-launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.backends.cuda.matmul.allow_tf32 = False
    tokens = tuple(int(t) for t in a.tokens.split("x"))
    result = {"runs": a.runs, "device": torch.cuda.get_device_name(0)}
    lines = ["%s; milliseconds, median [min .. max] of %d alternating runs" % (result["device"], a.runs)]
    for name in a.dtypes.split(","):
        result[name] = module_bench(name, DTYPES[name], tokens, a.runs, lines)
        torch.cuda.empty_cache()
        result[name]["kernels"] = kernel_bench(name, DTYPES[name], a.runs, a.kernel_launches, lines)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n" + json.dumps(result, sort_keys=True) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    identical = all(result[n]["bit_identical"] and result[n]["kernels"]["forward_bit_identical"]
                    for n in a.dtypes.split(","))
    if not identical:
        sys.exit("the fused and the literal route differ")


if __name__ == "__main__":
    main()
