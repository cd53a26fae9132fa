"""Plain references for QuantAnalyzer (aimet_amd/quant_analyzer.py, csrc/quant_analyzer.hip); none of this is
product code.

* sq_err: the two sums of aimet_qa_sq_err, float64 terms summed exactly (math.fsum);
* sensitivity_by_hand: the per-layer sensitivity analyses by toggling `enabled` by hand;
* per_layer_mse_f64: per-layer MSE on hook-captured (cloned) outputs, ((a.double() - b.double())**2).mean();
* per_layer_mse_literal: the reference's literal procedure (aimet_torch/v1/quant_analyzer.py
  _compute_mse_loss): per layer and batch a partial forward of both models and fp32 mse_loss().item().
"""
import math

import numpy as np
import torch


def as_f64(a):
    if isinstance(a, torch.Tensor):
        return a.detach().double().cpu().numpy().reshape(-1)
    return np.asarray(a, dtype=np.float64).reshape(-1)


def sq_err(ref, x):
    """(sum (ref - x)^2, sum ref^2): float64 terms, one rounding each, summed without further error."""
    r, v = as_f64(ref), as_f64(x)
    d = r - v
    return math.fsum((d * d).tolist()), math.fsum((r * r).tolist())


def bound(n, want):
    """|got - want| allowed for a double sum of n non-negative terms in any order, times a scale:
    each term has one rounding, any summation order adds at most n - 1, the scale one more."""
    return (n + 4) * 2.0 ** -53 * want


# ---------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def _forward(model, inputs):
    device = next((p.device for p in model.parameters()), torch.device("cpu"))
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            if isinstance(inputs, (list, tuple)):
                return model(*[i.to(device) for i in inputs])
            return model(inputs.to(device))
    except _Stop:
        return None
    finally:
        model.train(was)


def capture(model, names, inputs):
    """{name: a clone of the first output of module `name`} from one full forward."""
    modules = dict(model.named_modules())
    got, handles = {}, []

    def hook(name):
        def f(_, __, out):
            if name not in got:
                got[name] = out.detach().clone()
        return f
    for name in names:
        handles.append(modules[name].register_forward_hook(hook(name)))
    try:
        _forward(model, inputs)
    finally:
        for h in handles:
            h.remove()
    return got


def per_layer_mse_f64(model, sim_model, names, batches, device=None):
    """{name: (sum over batches of the float64 batch MSE, of the float64 batch mean of ref^2, samples, elements)}"""
    out = {n: [0.0, 0.0, 0, 0] for n in names}
    for inputs in batches:
        ref, quant = capture(model, names, inputs), capture(sim_model, names, inputs)
        for n in names:
            a, b = ref[n].double(), quant[n].double()
            if device is not None:
                a, b = a.to(device), b.to(device)
            out[n][0] += ((a - b) ** 2).mean().item()
            out[n][1] += (a ** 2).mean().item()
            out[n][2] += a.size(0)
            out[n][3] += a.numel()
    return {n: tuple(v) for n, v in out.items()}


def _partial(model, name, inputs):
    module = dict(model.named_modules())[name]
    got = []

    def hook(_, __, out):
        got.append(out.detach())
        raise _Stop
    h = module.register_forward_hook(hook)
    try:
        _forward(model, inputs)
    finally:
        h.remove()
    return got[0]


def per_layer_mse_literal(model, sim_model, names, batches):
    """{name: loss} as the reference computes it."""
    losses = {}
    for n in names:
        loss, total = 0.0, 0
        for inputs in batches:
            quant = _partial(sim_model, n, inputs)
            ref = _partial(model, n, inputs)
            loss += torch.nn.functional.mse_loss(ref, quant).item()
            total += ref.size(0)
        losses[n] = loss / total
    return losses


# ---------------------------------------------------------------------------------------------------
def wrapper_quantizers(wrapper):
    return list(wrapper.param_quantizers.values()) + list(wrapper.output_quantizers) + list(wrapper.input_quantizers)


def sensitivity_by_hand(sim_model, wrapper_names, score, enable_one):
    """{name: score(sim_model)} with, for each named wrapper in turn, either only that wrapper's
    quantizers on (enable_one) or only that wrapper's quantizers off."""
    modules = dict(sim_model.named_modules())
    was = {n: [q for q in wrapper_quantizers(modules[n]) if q.enabled] for n in wrapper_names}
    out = {}
    for n in wrapper_names:
        if not was[n]:
            continue
        off = [q for m in wrapper_names if (m != n) == enable_one for q in was[m]]
        for q in off:
            q.enabled = False
        was_training = sim_model.training
        sim_model.eval()
        with torch.no_grad():
            out[n] = score(sim_model)
        sim_model.train(was_training)
        for q in off:
            q.enabled = True
    return out
