"""Oracles for bias correction (aimet_amd/csrc/bias_corr.hip, aimet_amd/bias_correction.py):

* numpy float64 restatements of the three kernels: channel sums, the empirical update and the
  analytical (BN-based) update;
* a plain-torch restatement of correct_bias, layer by layer in the reference's order (analytical
  corrections where the reference makes them, not gathered up front), with torch's float64 reductions
  in place of the kernels. It builds the same QuantizationSimModel, so it needs a device.
"""
import copy
import math

import numpy as np

F = np.float32
NONE, RELU, RELU6 = 0, 1, 2


# ---------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------
def channel_sums(x, acc=None):
    """x: [outer][C][inner] float32; acc + per-channel float64 sums, and per channel sum |x|."""
    x = np.asarray(x, np.float64)
    s = x.sum(axis=(0, 2))
    return (s if acc is None else np.asarray(acc, np.float64) + s), np.abs(x).sum(axis=(0, 2))


def apply_empirical(bias, ref_sum, q_sum, count):
    """(the fp32 bias, its float64 value before the one rounding)"""
    exact = np.asarray(bias, np.float64) - (np.asarray(q_sum, np.float64) - np.asarray(ref_sum, np.float64)) / count
    return exact.astype(F), exact


def _cdf(v):
    return 0.5 * np.array([math.erfc(-t / math.sqrt(2.0)) for t in np.ravel(v)]).reshape(np.shape(v))


def _pdf(v):
    return np.exp(-(np.asarray(v, np.float64) ** 2) / 2.0) / math.sqrt(2.0 * math.pi)


def expected_input(beta, gamma, activation):
    """E[act(N(beta, gamma^2))] in float64, gamma as given (IEEE for gamma == 0)."""
    beta, gamma = np.asarray(beta, np.float64), np.asarray(gamma, np.float64)
    if activation == NONE:
        return beta.copy()
    with np.errstate(all="ignore"):
        lo = -beta / gamma
        if activation == RELU:
            return beta * (1.0 - _cdf(lo)) + gamma * _pdf(lo)
        hi = (6.0 - beta) / gamma
        z = _pdf(lo) - _pdf(hi)
        Z = _cdf(hi) - _cdf(lo)
        return (gamma * z + beta * Z) + 6.0 * (1.0 - _cdf(hi))


def logical(w, transposed=False):
    """A weight in module layout as [cout][cin][k]."""
    w = np.asarray(w)
    v = w.reshape(w.shape[0], w.shape[1], -1)
    return v.transpose(1, 0, 2) if transposed else v


def analytical(w, wq, bias, gamma, beta, activation, transposed=False):
    """(fp32 bias, float64 bias before the rounding, sum_i |eps[o,i] * E[i]|). gamma / beta None: ones
    and zeros. Each difference wq - w is one fp32 subtraction; the rest is float64."""
    v, vq = logical(np.asarray(w, F), transposed), logical(np.asarray(wq, F), transposed)
    eps = (vq - v).astype(F).astype(np.float64).sum(axis=2)            # [cout][cin]
    n = eps.shape[0] if eps.shape[1] == 1 else eps.shape[1]
    gamma = np.ones(n) if gamma is None else gamma
    beta = np.zeros(n) if beta is None else beta
    E = expected_input(beta, gamma, activation)
    with np.errstate(all="ignore"):
        terms = eps[:, 0:1] * E[:, None] if eps.shape[1] == 1 else eps * E[None, :]
    err = terms.sum(axis=1)
    exact = np.asarray(bias, np.float64) - err
    return exact.astype(F), exact, np.abs(terms).sum(axis=1)


def half_ulp32(v):
    return 0.5 * np.spacing(np.abs(np.asarray(v, np.float64)).astype(F)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------
# the schedule in plain torch
# ---------------------------------------------------------------------------------------------------
def _expected_input_torch(beta, gamma, activation):
    import torch
    beta, gamma = beta.double(), gamma.double()

    def cdf(v):
        return 0.5 * torch.special.erfc(-v / math.sqrt(2.0))

    def pdf(v):
        return torch.exp(-(v * v) / 2.0) / math.sqrt(2.0 * math.pi)
    if activation == NONE:
        return beta
    lo = -beta / gamma
    if activation == RELU:
        return beta * (1.0 - cdf(lo)) + gamma * pdf(lo)
    hi = (6.0 - beta) / gamma
    return (gamma * (pdf(lo) - pdf(hi)) + beta * (cdf(hi) - cdf(lo))) + 6.0 * (1.0 - cdf(hi))


def _sums_torch(layer, out):
    """(float64 per-channel sums, elements per channel) of a layer output, by torch's own reduction."""
    import torch
    from torch import nn
    if isinstance(layer, nn.Linear):
        flat = out.reshape(-1, out.shape[-1])
        return flat.sum(0, dtype=torch.float64), flat.shape[0]
    dims = [0] + list(range(2, out.dim()))
    return out.sum(dims, dtype=torch.float64), out.numel() // out.shape[1]


def correct_bias_torch(model, quant_params, num_quant_samples, data_loader, num_bias_correct_samples,
                       conv_bn_dict, perform_only_empirical_bias_corr=True, layers_to_ignore=()):
    """correct_bias as the reference schedules it: layers in execution order, each corrected before
    the next is measured, analytical ones in their place in that order."""
    import torch
    from torch import nn

    from aimet_amd import bias_correction as BC
    from aimet_amd.quantsim import QuantizationSimModel

    device = next(model.parameters()).device
    items = list(data_loader)
    images = [(b[0] if isinstance(b, (list, tuple)) else b).to(device) for b in items]
    bs = images[0].shape[0]
    corr = images[:int(math.ceil(num_bias_correct_samples / bs))]
    quant = images[:int(math.ceil(num_quant_samples / bs))]
    ordered = BC._layers_in_execution_order(model, corr[0])
    fp = copy.deepcopy(model)
    for _, m in ordered:
        if m.bias is None:
            n = m.out_features if isinstance(m, nn.Linear) else m.out_channels
            m.bias = nn.Parameter(torch.zeros(n, device=device))
    sim = QuantizationSimModel(model, dummy_input=corr[0][:1], quant_scheme=quant_params.quant_scheme,
                               rounding_mode=quant_params.round_mode, default_output_bw=quant_params.act_bw,
                               default_param_bw=quant_params.weight_bw, in_place=True,
                               config_file=quant_params.config_file)
    for _, w in sim.quant_wrappers():
        w.output_quantizers[0].enabled = False
    sim.compute_encodings(lambda m, _: [BC.forward_pass(m, b) for b in quant], None)
    wrapper_of = {w.get_original_module(): w for _, w in sim.quant_wrappers()}

    def analytic(module, bn, activation):
        wrapper = wrapper_of[module]
        q = wrapper.param_quantizers["weight"]
        w = module.weight.data
        wq = q.quantize_dequantize(w, q.round_mode)
        d = (wq - w).reshape(w.shape[0], w.shape[1], -1).double().sum(2)
        if isinstance(module, (nn.ConvTranspose1d, nn.ConvTranspose2d, nn.ConvTranspose3d)) and module.groups == 1:
            d = d.t()
        if bn is None:
            E = torch.zeros(d.shape[0] if d.shape[1] == 1 else d.shape[1], dtype=torch.float64, device=device)
        else:
            b = bn.get_module()
            E = _expected_input_torch(b.bias.data.to(device), b.weight.data.to(device), activation.value)
        err = d[:, 0] * E if d.shape[1] == 1 else (d * E[None, :]).sum(1)
        module.bias.data = (module.bias.data.double() - err).float()

    def measure(net, layer_module, hooked):
        total, count = None, 0
        got = {}

        def hook(_, __, out):
            got["s"], got["n"] = _sums_torch(layer_module, out)
            raise BC.StopForwardException
        h = hooked.register_forward_hook(hook)
        try:
            for b in corr:
                BC.forward_pass(net, b)
                total = got["s"] if total is None else total + got["s"]
                count += got["n"]
        finally:
            h.remove()
        return total, count

    with torch.no_grad():
        todo = list(ordered)
        if not perform_only_empirical_bias_corr and not any(todo[0][1] is m for m in layers_to_ignore):
            analytic(todo[0][1], None, None)
            todo.pop(0)
        for name, module in todo:
            if any(module is m for m in layers_to_ignore) or module not in conv_bn_dict:
                continue
            info = conv_bn_dict[module]
            if perform_only_empirical_bias_corr or info is None or info.input_bn is None:
                ref, count = measure(fp, module, fp.get_submodule(name))
                q, _ = measure(model, module, wrapper_of[module])
                module.bias.data = (module.bias.data.double() - (q - ref) / count).float()
            else:
                analytic(module, info.input_bn, info.in_activation_type)
    QuantizationSimModel._remove_quantization_wrappers(model, list(model.modules()))
