"""Bias correction (aimet_torch/bias_correction.py) on the MI355X core: the third step of data-free
quantization after batch-norm folding and cross-layer equalization. Weight quantization shifts the
mean of a layer's output; the shift is measured (empirical) or derived from the preceding BatchNorm's
statistics (analytical) and taken out of the layer's bias. Names and semantics follow the reference.

What differs is where the arithmetic runs and how often the models run. The reference, for every
layer and every batch, runs the FP model and the quantized model up to that layer, copies both
outputs to the host, stacks them and takes float32 numpy means. Here the only arithmetic on a layer
output is its per-channel sum, taken where the output was produced (``aimet_bc_channel_sums``,
aimet_amd/csrc/bias_corr.hip: one read, double accumulators, no host copy), and the schedule is:

* reference side, once: one forward of an untouched copy of the model per correction batch, with a
  hook on every layer to correct that adds the output's channel sums to the layer's ``ref_sum`` (in
  the hook, because an in-place ReLU behind the layer overwrites the output). The reference re-runs
  the FP model for every layer; its outputs never change, so the sums are the same.
* analytical layers (``perform_only_empirical_bias_corr=False``): all of them in one
  ``aimet_bc_analytical`` launch, up front;
* empirical layers, in execution order: per batch one forward of the sim up to the layer (a hook on
  its wrapper takes the channel sums into ``q_sum`` and raises ``StopForwardException``), then one
  ``aimet_bc_apply_empirical``. No tensor leaves the device and nothing is concatenated.

Both sides must see the same batches, so the first ``ceil(num_bias_correct_samples / batch_size)``
input batches of the loader are kept on the device for the duration of the call (the reference
iterates the loader again for every layer and feeds each batch to both models).

``find_all_conv_bn_with_activation`` reads the model's ``torch.fx`` trace (the project has no
ConnectedGraph); ``input_shape`` is accepted for compatibility. There is no CPU compute path: a
CPU-resident model is corrected through a copy in HBM and its biases are copied back; with no HIP
device every entry point raises. float32 only.
"""
import copy
import ctypes
import enum
import math
from typing import Dict, List, Optional, Union

import torch
import torch.nn.functional as F
from torch import nn

from aimet_amd import _dfq, _native
from aimet_amd._native import BcAnalyticalJobC
from aimet_amd.qc_quantize_op import QcQuantizeWrapper
from aimet_amd.quantsim import QuantizationSimModel, QuantParams  # noqa: F401  (re-exported)

_CONVS = (nn.Conv1d, nn.Conv2d, nn.Conv3d, nn.ConvTranspose1d, nn.ConvTranspose2d, nn.ConvTranspose3d)
_LAYERS = _CONVS + (nn.Linear,)
_BATCHNORMS = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)


class ActivationType(enum.Enum):
    """aimet_common/defs.py: the activation between a BatchNorm and the layer it feeds."""
    no_activation = 0
    relu = 1
    relu6 = 2


class ConvBnInfoType:
    """aimet_common/bias_correction.py: the BatchNorms around a conv / linear layer and the activations
    between. input_bn / output_bn are None or objects whose get_module() is the BatchNorm."""

    def __init__(self, input_bn=None, output_bn=None, in_activation_type: ActivationType = ActivationType.no_activation,
                 out_activation_type: ActivationType = ActivationType.no_activation):
        self.input_bn = input_bn
        self.output_bn = output_bn
        self.in_activation_type = in_activation_type
        self.out_activation_type = out_activation_type


class _BnRef:
    """Holds a BatchNorm module the way the reference's graph ops do. The module is kept by
    reference, so the entry still serves after fold_all_batch_norms replaced it in the model."""

    def __init__(self, module: nn.Module):
        self._module = module

    def get_module(self) -> nn.Module:
        return self._module


class StopForwardException(Exception):
    """Raised by a hook to end a forward pass at the layer of interest."""


def forward_pass(model: nn.Module, batch: torch.Tensor):
    """One eval-mode, no-grad forward of `model` on `batch` (moved to the model's device), up to the
    end or to a StopForwardException."""
    device = next((p.device for p in model.parameters()), None)
    if device is not None and batch.device != device:
        batch = batch.to(device)
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            model(batch)
    except StopForwardException:
        pass
    finally:
        model.train(was)


def get_quantized_dequantized_weight(layer: QcQuantizeWrapper) -> torch.Tensor:
    """The wrapped layer's weight as its own param quantizer quantize-dequantizes it."""
    q = layer.param_quantizers["weight"]
    return q.quantize_dequantize(layer._module_to_wrap.weight.data, q.round_mode)


def launch_count(reset: bool = False) -> int:
    """Kernel launches the bias-correction entry points have issued in this process."""
    n = ctypes.c_int64()
    _native.call("aimet_bc_launch_count", ctypes.byref(n), 1 if reset else 0)
    return n.value


# ---------------------------------------------------------------------------------------------------
# graph search
# ---------------------------------------------------------------------------------------------------
def _activation_of(g: "_dfq.TracedGraph", node) -> Optional[ActivationType]:
    m = g.module(node)
    if isinstance(m, nn.ReLU):
        return ActivationType.relu
    if isinstance(m, nn.ReLU6) or (isinstance(m, nn.Hardtanh) and m.min_val == 0 and m.max_val == 6):
        return ActivationType.relu6
    if node.op == "call_function":
        if node.target in (F.relu, torch.relu):
            return ActivationType.relu
        if node.target is F.relu6:
            return ActivationType.relu6
    if node.op == "call_method" and node.target == "relu":
        return ActivationType.relu
    return None


def find_all_conv_bn_with_activation(model: nn.Module, input_shape=None) -> Dict[nn.Module, ConvBnInfoType]:
    """Every conv / conv-transpose / linear layer of the model with the BatchNorms next to it. Patterns
    match on edges whose producer has exactly one user:

    * ``BN -> Conv|ConvTranspose`` and ``BN -> ReLU|ReLU6|Hardtanh(0, 6) -> Conv|ConvTranspose`` fill
      input_bn and in_activation_type (a BatchNorm before a Linear is not matched, as the reference);
    * ``Conv|ConvTranspose|Linear -> BN`` fills output_bn;
    * every other layer gets an empty entry.
    """
    g = _dfq.TracedGraph(model)
    found: Dict[nn.Module, ConvBnInfoType] = {}
    for node in g.nodes:
        m = g.module(node)
        if isinstance(m, _LAYERS):
            found.setdefault(m, ConvBnInfoType())
    for node in g.nodes:
        m = g.module(node)
        if isinstance(m, _LAYERS):
            user = g.sole_user(node)
            bn = g.module(user) if user is not None else None
            if isinstance(bn, _BATCHNORMS):
                found[m].output_bn = _BnRef(bn)
        elif isinstance(m, _BATCHNORMS):
            user = g.sole_user(node)
            if user is None:
                continue
            act = _activation_of(g, user)
            if act is not None:
                user = g.sole_user(user)
                if user is None:
                    continue
            layer = g.module(user)
            if isinstance(layer, _CONVS):
                found[layer].input_bn = _BnRef(m)
                found[layer].in_activation_type = act or ActivationType.no_activation
    return found


# ---------------------------------------------------------------------------------------------------
# the kernels on layer outputs and parameters
# ---------------------------------------------------------------------------------------------------
def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _out_channels(layer: nn.Module) -> int:
    return layer.out_features if isinstance(layer, nn.Linear) else layer.out_channels


def _as_outer_c_inner(layer: nn.Module, out: torch.Tensor):
    """(tensor to read, outer, C, inner) of a layer output: contiguous NCHW / NCL / NCDHW is planar,
    channels-last and Linear's [..., C] interleaved; anything else is made contiguous first."""
    _dfq.require_fp32([out], "bias correction")
    if not out.is_cuda:
        raise RuntimeError("aimet_amd: bias correction got a layer output on %s; the MI355X core has no CPU path"
                           % out.device)
    C = _out_channels(layer)
    if isinstance(layer, nn.Linear):
        if out.dim() < 1 or out.shape[-1] != C:
            raise ValueError("bias correction: %r produced an output of shape %s" % (layer, tuple(out.shape)))
        out = out if out.is_contiguous() else out.contiguous()
        return out, out.numel() // C, C, 1
    if out.dim() < 3 or out.shape[1] != C:
        raise ValueError("bias correction: %r produced an output of shape %s" % (layer, tuple(out.shape)))
    inner = out[0, 0].numel()
    if out.is_contiguous():
        return out, out.shape[0], C, inner
    last = {4: torch.channels_last, 5: torch.channels_last_3d}.get(out.dim())
    if last is not None and out.is_contiguous(memory_format=last):
        return out, out.shape[0] * inner, C, 1
    return out.contiguous(), out.shape[0], C, inner


def _add_channel_sums(layer: nn.Module, out: torch.Tensor, acc: torch.Tensor) -> int:
    """acc[c] += the sum of channel c of `out`; returns the elements per channel."""
    if out.numel() == 0:
        return 0
    x, outer, C, inner = _as_outer_c_inner(layer, out)
    with torch.cuda.device(x.device):
        _native.call("aimet_bc_channel_sums", _dfq.ptr(x), outer, C, inner, _dfq.ptr(acc), _stream(x.device))
    return outer * inner


def _apply_empirical(bias: torch.Tensor, ref_sum: torch.Tensor, q_sum: torch.Tensor, count: int):
    with torch.cuda.device(bias.device):
        _native.call("aimet_bc_apply_empirical", _dfq.ptr(bias), _dfq.ptr(ref_sum), _dfq.ptr(q_sum), bias.numel(),
                     float(count), _stream(bias.device))


def call_empirical_correct_bias(layer: nn.Module, reference_outputs: torch.Tensor, quantized_outputs: torch.Tensor):
    """Empirical correction of `layer.bias` from the layer's outputs in the FP and in the quantized
    model (device tensors of one shape, channels on axis 1; [rows, C] for a Linear layer)."""
    if reference_outputs.shape != quantized_outputs.shape:
        raise ValueError("bias correction: the reference and the quantized outputs differ in shape")
    _dfq.require_fp32([layer.bias], "bias correction")
    stage = _dfq.Stage([layer.bias, reference_outputs, quantized_outputs])
    with torch.no_grad():
        bias = stage.dev(layer.bias)
        sums = stage.new(2 * bias.numel(), torch.float64).view(2, -1)
        count = _add_channel_sums(layer, reference_outputs.to(stage.device), sums[0])
        _add_channel_sums(layer, quantized_outputs.to(stage.device), sums[1])
        _apply_empirical(bias, sums[0], sums[1], count)
        stage.finish()


def _analytical_launch(stage: "_dfq.Stage", jobs: List[tuple]):
    """One aimet_bc_analytical launch; a job is (wrapper, bn holder or None, activation type)."""
    if not jobs:
        return
    table = (BcAnalyticalJobC * len(jobs))()
    keep = []
    for slot, (wrapper, bn, activation) in zip(table, jobs):
        layer = wrapper.get_original_module()
        _dfq.require_fp32([layer.weight, layer.bias], "bias correction")
        w, bias = stage.dev(layer.weight), stage.dev(layer.bias)
        wq = get_quantized_dequantized_weight(wrapper).to(stage.device).contiguous()
        _dfq.require_fp32([wq], "bias correction")
        slot.w = _dfq.weight_desc(layer, w)
        slot.wq, slot.bias = wq.data_ptr(), bias.data_ptr()
        slot.activation = ActivationType.no_activation.value
        keep.append((w, bias, wq))
        if bn is not None:
            module = bn.get_module()
            _dfq.require_fp32([module.weight, module.bias], "bias correction")
            gamma, beta = stage.dev(module.weight), stage.dev(module.bias)
            want = slot.w.cout if slot.w.cin == 1 else slot.w.cin
            if gamma.numel() != want or beta.numel() != want:
                raise ValueError("bias correction: %r has %d features, %r takes %d input channels"
                                 % (module, gamma.numel(), layer, want))
            slot.gamma, slot.beta = gamma.data_ptr(), beta.data_ptr()
            slot.activation = ActivationType(getattr(activation, "value", 0) or 0).value
            keep.append((gamma, beta))
    with torch.cuda.device(stage.device):
        _native.call("aimet_bc_analytical", table, len(jobs), ctypes.c_void_p(stage.stream))
    del keep


def call_analytical_correct_bias(layer: QcQuantizeWrapper, bn, activation_type: Optional[ActivationType]):
    """Analytical correction of the wrapped layer's bias: `bn` is None or holds (get_module()) the
    BatchNorm that feeds the layer, activation_type what lies between them."""
    module = layer.get_original_module()
    stage = _dfq.Stage([module.weight, module.bias])
    with torch.no_grad():
        _analytical_launch(stage, [(layer, bn, activation_type)])
        stage.finish()


# ---------------------------------------------------------------------------------------------------
# correct_bias
# ---------------------------------------------------------------------------------------------------
def _images(item) -> torch.Tensor:
    return item[0] if isinstance(item, (list, tuple)) else item


def _first_batches(data_loader, n: int) -> List[torch.Tensor]:
    out = []
    for item in data_loader:
        if len(out) >= n:
            break
        out.append(_images(item))
    return out


def _layers_in_execution_order(model: nn.Module, batch: torch.Tensor) -> List[tuple]:
    """[(name, module)] of the model's conv / linear layers in the order one forward first runs them."""
    names = {m: n for n, m in model.named_modules()}
    order = []

    def hook(m, *_):
        if all(m is not seen for _, seen in order):
            order.append((names[m], m))
    hooks = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, _LAYERS)]
    try:
        forward_pass(model, batch)
    finally:
        for h in hooks:
            h.remove()
    return order


def correct_bias(model: nn.Module, quant_params: QuantParams, num_quant_samples: int, data_loader,
                 num_bias_correct_samples: int, conv_bn_dict: Union[Dict[nn.Module, ConvBnInfoType], None] = None,
                 perform_only_empirical_bias_corr: bool = True, layers_to_ignore: List[nn.Module] = None):
    """Corrects, in place, the bias of every conv / linear layer of the fp32 `model` (unless ignored)
    for the shift that quantizing its weights and the weights before it introduces.

    :param quant_params: QuantParams (weight_bw, act_bw, round_mode, quant_scheme, config_file) of the sim
    :param num_quant_samples: samples for compute_encodings, rounded up to whole batches
    :param data_loader: yields input batches, or tuples / lists whose first element is one
    :param num_bias_correct_samples: samples the corrections are measured on, rounded up to whole batches
    :param conv_bn_dict: what find_all_conv_bn_with_activation returned (found here when None); may have
           been found before the model's BatchNorms were folded
    :param perform_only_empirical_bias_corr: when False the first layer and every conv fed by a
           BatchNorm are corrected analytically, the others empirically
    :param layers_to_ignore: layers whose bias is left alone
    """
    layers_to_ignore = list(layers_to_ignore or [])
    params = list(model.parameters())
    _dfq.require_fp32(params, "bias correction")
    stage = _dfq.Stage(params)          # raises when there is no HIP device
    if any(not p.is_cuda for p in params):
        _correct_cpu_resident(model, stage.device, quant_params, num_quant_samples, data_loader,
                              num_bias_correct_samples, conv_bn_dict, perform_only_empirical_bias_corr,
                              layers_to_ignore)
        return
    device = stage.device

    first = next(iter(data_loader), None)
    if first is None:
        raise ValueError("bias correction: the data loader is empty")
    batch_size = int(_images(first).shape[0])
    n_batches_bias_correction = int(math.ceil(num_bias_correct_samples / batch_size))
    n_batches_quantization = int(math.ceil(num_quant_samples / batch_size))
    batches = [b.to(device) for b in _first_batches(data_loader, n_batches_bias_correction)]
    _dfq.require_fp32(batches, "bias correction")

    ordered = _layers_in_execution_order(model, batches[0])
    if conv_bn_dict is None:
        conv_bn_dict = find_all_conv_bn_with_activation(model)
    model_copy = copy.deepcopy(model)

    with torch.no_grad():
        for _, module in ordered:
            if module.bias is None:
                module.bias = nn.Parameter(torch.zeros(_out_channels(module), device=module.weight.device))

    sim = QuantizationSimModel(model, dummy_input=batches[0][:1], quant_scheme=quant_params.quant_scheme,
                               rounding_mode=quant_params.round_mode, default_output_bw=quant_params.act_bw,
                               default_param_bw=quant_params.weight_bw, in_place=True,
                               config_file=quant_params.config_file)
    assert sim.model is model
    try:
        for _, wrapper in sim.quant_wrappers():
            wrapper.output_quantizers[0].enabled = False

        def pass_data_through_model(m, _):
            for images in _first_batches(data_loader, n_batches_quantization):
                forward_pass(m, images)
        sim.compute_encodings(pass_data_through_model, None)
        wrapper_of = {w.get_original_module(): w for _, w in sim.quant_wrappers()}

        # which layer is corrected how (bias_correction.py:408-456 of the reference)
        analytical, empirical = [], []
        todo = list(ordered)
        if not perform_only_empirical_bias_corr and todo:
            _, module = todo[0]
            if not any(module is m for m in layers_to_ignore) and module in wrapper_of:
                analytical.append((wrapper_of[module], None, None))   # no BN: beta = 0, a zero correction
                todo.pop(0)
        for name, module in todo:
            if any(module is m for m in layers_to_ignore) or module not in conv_bn_dict or module not in wrapper_of:
                continue
            info = conv_bn_dict[module]
            if perform_only_empirical_bias_corr or info is None or info.input_bn is None:
                empirical.append((name, module))
            else:
                analytical.append((wrapper_of[module], info.input_bn, info.in_activation_type))

        with torch.no_grad():
            # The reference corrects these in execution order, between the empirical ones. An
            # analytical correction reads no data (weights, their quantized values, BN parameters),
            # and the bias of layer j does not change the output of a layer before it, so doing all
            # of them first leaves every later empirical measurement as it would be.
            _analytical_launch(stage, analytical)

            # reference side: one forward per batch collects every empirical layer's channel sums
            ref_sum = {m: torch.zeros(_out_channels(m), dtype=torch.float64, device=device) for _, m in empirical}
            count = {m: 0 for _, m in empirical}
            handles = []
            for name, module in empirical:
                ref_layer = model_copy.get_submodule(name)

                def ref_hook(layer, _, out, key=module):
                    count[key] += _add_channel_sums(layer, out, ref_sum[key])
                handles.append(ref_layer.register_forward_hook(ref_hook))
            try:
                for images in batches:
                    forward_pass(model_copy, images)
            finally:
                for h in handles:
                    h.remove()

            # quantized side, in order: the corrected biases of earlier layers feed later ones
            for name, module in empirical:
                q_sum = torch.zeros(_out_channels(module), dtype=torch.float64, device=device)

                def q_hook(wrapper, _, out, layer=module, acc=q_sum):
                    _add_channel_sums(layer, out, acc)
                    raise StopForwardException
                handle = wrapper_of[module].register_forward_hook(q_hook)
                try:
                    for images in batches:
                        forward_pass(model, images)
                finally:
                    handle.remove()
                if count[module]:
                    _apply_empirical(module.bias.data, ref_sum[module], q_sum, count[module])
    finally:
        QuantizationSimModel._remove_quantization_wrappers(model, list(model.modules()))


def _correct_cpu_resident(model, device, quant_params, num_quant_samples, data_loader, num_bias_correct_samples,
                          conv_bn_dict, perform_only_empirical_bias_corr, layers_to_ignore):
    """There is no CPU compute path: the model is corrected through a copy in HBM and the biases are
    copied back (a layer without a bias gains one). The dict's and the ignore list's layers are
    looked up in the copy by name; BatchNorms are kept by reference, their parameters staged."""
    if conv_bn_dict is None:
        conv_bn_dict = find_all_conv_bn_with_activation(model)
    twin = copy.deepcopy(model).to(device)
    mine, theirs = dict(model.named_modules()), dict(twin.named_modules())
    name_of = {m: n for n, m in mine.items()}
    dev_dict = {theirs[name_of[m]]: info for m, info in conv_bn_dict.items() if m in name_of}
    dev_ignore = [theirs[name_of[m]] for m in layers_to_ignore if m in name_of]
    correct_bias(twin, quant_params, num_quant_samples, data_loader, num_bias_correct_samples, dev_dict,
                 perform_only_empirical_bias_corr, dev_ignore)
    with torch.no_grad():
        for name, module in mine.items():
            if isinstance(module, _LAYERS) and theirs[name].bias is not None:
                if module.bias is None:
                    module.bias = nn.Parameter(torch.zeros(_out_channels(module), device=module.weight.device))
                module.bias.copy_(theirs[name].bias)
