"""PEFT LoRA adapters on a quantized base model (aimet_torch/peft.py).

A PEFT LoRA layer keeps its adapters in ModuleDicts and adds them to the base layer's output with
plain tensor arithmetic, so a sim put on it quantizes base_layer, lora_A and lora_B and leaves the
`* scaling` and the `+` unquantized. LoraLayer spells the layer out in children the sim wraps --
base_layer / lora_A[i] / lora_B[i] / mul_scale / add_lora_to_res -- and PeftQuantUtils freezes the
base, sets the adapters' bitwidths and exports, loads and disables adapter weights.

    replace_lora_layers_with_quantizable_layers(model)          # in place
    meta = track_lora_meta_data(model, path, "meta")
    sim = QuantizationSimModel(model, dummy_input, quantizable_types=PEFT_QUANTIZABLE_TYPES)
    sim.compute_encodings(...)
    utils = PeftQuantUtils(meta)
    utils.freeze_base_model(sim)

`peft` itself is never needed: a layer is recognised by its attributes (is_peft_lora_layer); where
`peft` is importable its LoraLayer and Conv2d types are matched as well.

Two routes compute an adapted layer (the same bits):

  * literal: the reference's line, per active adapter,
        result = add_lora_to_res(result, lora_B(mul_scale(lora_A(dropout(x)), scaling)))
    with the five wrappers called one by one.
  * fused: the three GEMMs through StaticGridQuantWrapper.forward_raw (input quantizers, parameter
    QDQ and STE gating as forward() runs them, no output quantizer), and the element-wise tail in
    two launches of csrc/lora.hip:
        u = base_layer.forward_raw(x);  a = lora_A.forward_raw(dropout(x))
        m = LoraScale(a, s, enc_A, enc_mul)                 aimet_lora_scale
        v = lora_B.forward_raw(m)
        out = LoraMerge(u, v, enc_base, enc_B, enc_add)      aimet_lora_merge
    with aimet_lora_scale_backward / aimet_lora_merge_backward going back. Taken when `fused` is
    set, exactly one adapter is active, all five children are StaticGridQuantWrappers in ACTIVE
    mode whose output quantizer is disabled or a per-tensor integer quantizer rounding to nearest
    (output_quantizer_fusable), mul_scale and add_lora_to_res have no enabled input or parameter
    quantizer, and x and the three weights are on the GPU in one dtype out of float32, float16 and
    bfloat16 (x contiguous, no autocast). Everything else -- ANALYSIS and PASSTHROUGH mode,
    range-learning wrappers, stochastic rounding in training, float data types, several active
    adapters, CPU tensors, a quantized scale (quantize_lora_scale_with_fixed_range) -- is literal, so
    calibration and range learning go through the wrappers unchanged.

The scale is kept as a Python float from construction (PEFT's `scaling` holds floats); no forward
reads it back from the device. If somebody writes to the scaling tensor (its _version moves) it is
read back once. _host_scale states which float the kernel gets for a 16-bit tensor.

Differs from the reference:
  * The reference's forward loops over every adapter name in `active_adapters`, whatever the flag
    says, so an inactive adapter is added too; here only adapters whose flag is set run.
  * PeftQuantUtils(name_to_module_dict=...) -- the prepared-model / ONNX name mapping -- is not
    supported: None only.
  * freeze_*: the v2 quantizers' `_allow_overwrite = False` is v1's freeze_encoding(); a quantizer
    without an encoding (disabled, 32 bits) has nothing to freeze and is passed over.
  * quantize_lora_scale_with_fixed_range enables the existing second input quantizer of mul_scale
    with a TF encoding of [scale_min, scale_max] and freezes it, instead of installing a new object.
  * A wrapper made without a dummy input has one input quantizer; mul_scale and add_lora_to_res
    take two tensors, so LoraLayer adds the missing (disabled) input quantizers on first use.
  * enable_adapter_and_load_weights loads onto the model's device (the reference: device 0) and
    splits a key at its last dot (the reference cuts at ".weight" and so mangles bias keys); its
    .bin form is torch.load(weights_only=True).
  * `scaling` follows the module through .to(device) / .cuda() (the reference's plain list stays
    behind); it stays float32 whatever dtype the module is cast to.
"""
import ctypes
import os
import pickle
from collections import defaultdict
from typing import Dict, Type

import torch
from torch import nn

from aimet_amd import _native
from aimet_amd.elementwise_ops import Add, Multiply
from aimet_amd.libpymo import getComputedEncodings
from aimet_amd.qc_quantize_op import (QcQuantizeOpMode, QcQuantizeWrapper, StaticGridQuantWrapper,
                                      tensor_quantizer_factory)
from aimet_amd.quantsim import DEFAULT_QUANTIZABLE_TYPES, _model_device
from aimet_amd.transformers import _encoding_c   # TfEncoding or (min, max, bw) -> a C struct of its own; None stays

PEFT_QUANTIZABLE_TYPES = DEFAULT_QUANTIZABLE_TYPES + (Add, Multiply)

_IO_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}   # io_dtype of aimet_lora_*


# ---- the launches --------------------------------------------------------------------------------
def lora_launch_count(reset: bool = False) -> int:
    """aimet_lora_* calls that launched on the GPU in this process."""
    n = ctypes.c_int64(0)
    _native.call("aimet_lora_launch_count", ctypes.byref(n), int(reset))
    return n.value


def _ref(enc):
    return ctypes.byref(enc) if enc is not None else None


def _check(what, *tensors):
    t0 = tensors[0]
    for t in tensors:
        if not (t.is_cuda and t.dtype in _IO_CODES and t.is_contiguous()):
            raise ValueError("%s: tensors must be contiguous float32 / float16 / bfloat16 tensors on the GPU" % what)
        if t.dtype != t0.dtype or t.numel() != t0.numel() or t.device != t0.device:
            raise ValueError("%s: tensors must share one dtype, size and device" % what)
    return _IO_CODES[t0.dtype]


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _host_scale(scale: float, dtype) -> float:
    """The float aimet_lora_scale multiplies by so that it equals `t * s` with t of `dtype` and s a
    0-dim float32 tensor on the device: torch computes that product in the common dtype, which a
    0-dim operand does not widen, so s is cast to `dtype` first (then both are widened to float32 for
    the multiply). float32(scale) for a float32 tensor, that value rounded to fp16 / bf16 otherwise."""
    return float(torch.tensor(float(scale), dtype=torch.float32).to(dtype))


def lora_merge(u, v, enc_u=None, enc_v=None, enc_out=None, out=None):
    """One aimet_lora_merge launch: Q_out(Q_u(u) + Q_v(v)). Encodings: TfEncoding, (min, max, bw) or
    None (disabled). `out` may overlap neither input. There is no other implementation behind this."""
    out = torch.empty_like(u) if out is None else out
    io = _check("lora_merge", u, v, out)
    cu, cv, co = _encoding_c(enc_u), _encoding_c(enc_v), _encoding_c(enc_out)
    with torch.cuda.device(u.device):
        _native.call("aimet_lora_merge", u.data_ptr(), v.data_ptr(), out.data_ptr(), u.numel(), io, _ref(cu),
                     _ref(cv), _ref(co), _stream(u))
    return out


def lora_merge_backward(u, v, grad, enc_u=None, enc_v=None, enc_out=None, need_u=True, need_v=True, grad_u=None,
                        grad_v=None):
    """One aimet_lora_merge_backward launch; returns (grad_u, grad_v), None for an operand that is not
    needed (nothing is written for it)."""
    grad_u = (torch.empty_like(u) if grad_u is None else grad_u) if need_u else None
    grad_v = (torch.empty_like(v) if grad_v is None else grad_v) if need_v else None
    io = _check("lora_merge_backward", u, v, grad, *[g for g in (grad_u, grad_v) if g is not None])
    cu, cv, co = _encoding_c(enc_u), _encoding_c(enc_v), _encoding_c(enc_out)
    with torch.cuda.device(u.device):
        _native.call("aimet_lora_merge_backward", u.data_ptr(), v.data_ptr(), grad.data_ptr(),
                     grad_u.data_ptr() if need_u else None, grad_v.data_ptr() if need_v else None, u.numel(), io,
                     _ref(cu), _ref(cv), _ref(co), _stream(u))
    return grad_u, grad_v


def lora_scale(a, scale: float, enc_a=None, enc_out=None, out=None):
    """One aimet_lora_scale launch: Q_out(Q_a(a) * scale), `scale` the float the kernel multiplies by
    (see _host_scale)."""
    out = torch.empty_like(a) if out is None else out
    io = _check("lora_scale", a, out)
    ca, co = _encoding_c(enc_a), _encoding_c(enc_out)
    with torch.cuda.device(a.device):
        _native.call("aimet_lora_scale", a.data_ptr(), out.data_ptr(), a.numel(), io, float(scale), _ref(ca), _ref(co),
                     _stream(a))
    return out


def lora_scale_backward(a, grad, scale: float, enc_a=None, enc_out=None, grad_a=None):
    """One aimet_lora_scale_backward launch."""
    grad_a = torch.empty_like(a) if grad_a is None else grad_a
    io = _check("lora_scale_backward", a, grad, grad_a)
    ca, co = _encoding_c(enc_a), _encoding_c(enc_out)
    with torch.cuda.device(a.device):
        _native.call("aimet_lora_scale_backward", a.data_ptr(), grad.data_ptr(), grad_a.data_ptr(), a.numel(), io,
                     float(scale), _ref(ca), _ref(co), _stream(a))
    return grad_a


class LoraScale(torch.autograd.Function):
    """m = Q_mul(Q_A(a) * s) with the straight-through gradient, one launch each way; saves a."""

    @staticmethod
    def forward(ctx, a, scale, enc_a, enc_out):
        a = a.contiguous()
        ctx.scale, ctx.encs = scale, (_encoding_c(enc_a), _encoding_c(enc_out))   # the encodings as they are now
        ctx.save_for_backward(a)
        return lora_scale(a, scale, *ctx.encs)

    @staticmethod
    def backward(ctx, grad):
        (a,) = ctx.saved_tensors
        return lora_scale_backward(a, grad.to(a.dtype).contiguous(), ctx.scale, *ctx.encs), None, None, None


class LoraMerge(torch.autograd.Function):
    """out = Q_add(Q_base(u) + Q_B(v)) with the straight-through gradients, one launch each way; saves
    u and v. An operand that needs no gradient gets none computed."""

    @staticmethod
    def forward(ctx, u, v, enc_u, enc_v, enc_out):
        u, v = u.contiguous(), v.contiguous()
        ctx.encs = (_encoding_c(enc_u), _encoding_c(enc_v), _encoding_c(enc_out))
        ctx.save_for_backward(u, v)
        return lora_merge(u, v, *ctx.encs)

    @staticmethod
    def backward(ctx, grad):
        u, v = ctx.saved_tensors
        need_u, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_u or need_v):
            return None, None, None, None, None
        gu, gv = lora_merge_backward(u, v, grad.to(u.dtype).contiguous(), *ctx.encs, need_u=need_u, need_v=need_v)
        return gu, gv, None, None, None


# ---- the layer -----------------------------------------------------------------------------------
def _dict_like(v) -> bool:
    return hasattr(v, "keys") and hasattr(v, "__getitem__")


def is_peft_lora_layer(module) -> bool:
    """True for a module with the attributes of peft.tuners.lora.layer.LoraLayer: base_layer, dict-like
    lora_A / lora_B / lora_dropout / scaling / r / lora_alpha keyed by adapter name, and active_adapter
    or active_adapters."""
    if not isinstance(module, nn.Module) or isinstance(module, LoraLayer):
        return False
    if not isinstance(getattr(module, "base_layer", None), nn.Module):
        return False
    if not all(_dict_like(getattr(module, n, None)) for n in ("lora_A", "lora_B", "lora_dropout", "scaling", "r",
                                                               "lora_alpha")):
        return False
    return hasattr(module, "active_adapters") or hasattr(module, "active_adapter")


def _active_names(lora_layer):
    active = getattr(lora_layer, "active_adapters", None)
    if active is None:
        active = lora_layer.active_adapter
    return [active] if isinstance(active, str) else list(active)


def _ensure_input_quantizers(wrapper, count):
    """A static-grid wrapper made without a dummy input has one input quantizer; give it `count`
    (the new ones disabled, with the first one's settings)."""
    qs = wrapper.input_quantizers
    while len(qs) < count:
        q0 = qs[0]
        q = tensor_quantizer_factory(q0.bitwidth, q0.round_mode, q0.quant_scheme, q0.use_symmetric_encodings,
                                     enabled_by_default=False, data_type=q0.data_type)
        q.use_strict_symmetric, q.use_unsigned_symmetric = q0.use_strict_symmetric, q0.use_unsigned_symmetric
        qs.append(q)


class LoraLayer(nn.Module):
    """aimet_torch/peft.py:61-117: a PEFT LoRA layer with the adapters in ModuleLists and the scaling and
    the addition as modules (mul_scale, add_lora_to_res). Built from any module that passes
    is_peft_lora_layer, on a Linear or a Conv2d base. `fused = False` forces the literal route."""

    def __init__(self, lora_layer):
        super().__init__()
        self.base_layer = lora_layer.base_layer
        self.r = dict(lora_layer.r)
        self.lora_alpha = dict(lora_layer.lora_alpha)
        device = _model_device(self.base_layer)
        self._scale_values = [float(s) for s in lora_layer.scaling.values()]
        self.scaling = [torch.as_tensor(s, dtype=torch.float32).to(device) for s in self._scale_values]
        self._scale_versions = [s._version for s in self.scaling]
        self.lora_dropout = nn.ModuleList([])
        self.adapter_name_to_index = {}
        self.index_to_adapter_name = {}
        self.lora_A = nn.ModuleList([])
        self.lora_B = nn.ModuleList([])
        self.active_adapters = {}
        active = _active_names(lora_layer)
        for index, name in enumerate(lora_layer.lora_A.keys()):
            self.lora_A.append(lora_layer.lora_A[name])
            self.lora_B.append(lora_layer.lora_B[name])
            self.lora_dropout.append(lora_layer.lora_dropout[name])
            self.adapter_name_to_index[name] = index
            self.index_to_adapter_name[index] = name
            self.active_adapters[name] = name in active
        base = self.base_layer
        self.in_features = getattr(lora_layer, "in_features", getattr(base, "in_features",
                                                                      getattr(base, "in_channels", None)))
        self.out_features = getattr(lora_layer, "out_features", getattr(base, "out_features",
                                                                        getattr(base, "out_channels", None)))
        self.add_lora_to_res = Add()
        self.mul_scale = Multiply()
        self.fused = True

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        moved = [s.to(fn(s).device) for s in self.scaling]   # the device only: the scale stays float32
        self._scale_versions = [v if m is s else m._version
                                for m, s, v in zip(moved, self.scaling, self._scale_versions)]
        self.scaling = moved
        return self

    def _scale_value(self, index) -> float:
        s = self.scaling[index]
        if s._version != self._scale_versions[index]:   # somebody wrote to it: one read-back
            self._scale_values[index] = float(s)
            self._scale_versions[index] = s._version
        return self._scale_values[index]

    def _fused_children(self, x, index):
        """The five wrappers when the fused route applies to x and adapter `index`, else None."""
        if not (self.fused and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in _IO_CODES and
                x.is_contiguous() and not torch.is_autocast_enabled()):
            return None
        five = (self.base_layer, self.lora_A[index], self.mul_scale, self.lora_B[index], self.add_lora_to_res)
        for w in five:
            if not (type(w) is StaticGridQuantWrapper and w._mode is QcQuantizeOpMode.ACTIVE and
                    w.output_quantizer_fusable()):
                return None
        for w in (self.mul_scale, self.add_lora_to_res):
            if any(q.enabled for q in w.input_quantizers) or any(q.enabled for q in w.param_quantizers.values()):
                return None
        for w in (self.base_layer, self.lora_A[index], self.lora_B[index]):
            weight = getattr(w._module_to_wrap, "weight", None)
            if weight is None or weight.dtype != x.dtype or weight.device != x.device:
                return None
        return five

    def forward(self, x, *args, **kwargs):
        active = [self.adapter_name_to_index[n] for n, on in self.active_adapters.items()
                  if on and n in self.adapter_name_to_index]
        for w in (self.mul_scale, self.add_lora_to_res):
            if isinstance(w, StaticGridQuantWrapper):
                _ensure_input_quantizers(w, 2)
        if len(active) == 1:
            five = self._fused_children(x, active[0])
            if five is not None:
                return self._forward_fused(five, active[0], x, *args, **kwargs)
        result = self.base_layer(x, *args, **kwargs)
        result_dtype = result.dtype
        for index in active:
            lora_A, lora_B = self.lora_A[index], self.lora_B[index]
            x = x.to(lora_A.weight.dtype)
            scaled = self.mul_scale(lora_A(self.lora_dropout[index](x)), self.scaling[index].detach())
            result = self.add_lora_to_res(result, lora_B(scaled))
        return result.to(result_dtype)

    def _forward_fused(self, five, index, x, *args, **kwargs):
        base, lora_A, mul, lora_B, add = five
        u = base.forward_raw(x, *args, **kwargs)
        a = lora_A.forward_raw(self.lora_dropout[index](x))
        enc_a, enc_mul = lora_A.fused_output_encoding(), mul.fused_output_encoding()
        m = LoraScale.apply(a, _host_scale(self._scale_value(index), a.dtype), enc_a, enc_mul)
        v = lora_B.forward_raw(m)
        enc_u, enc_v, enc_add = base.fused_output_encoding(), lora_B.fused_output_encoding(), \
            add.fused_output_encoding()
        if u.shape != v.shape or u.dtype != v.dtype:   # a broadcasting add: the wrappers' own arithmetic
            return add(base._quantize_activation(base.output_quantizers, [u])[0],
                       lora_B._quantize_activation(lora_B.output_quantizers, [v])[0])
        return LoraMerge.apply(u, v, enc_u, enc_v, enc_add)


def _peft_types():
    try:
        from peft.tuners.lora.layer import Conv2d as PeftConv2d
        from peft.tuners.lora.layer import LoraLayer as PeftLoraLayer
    except ImportError:
        return ()
    return (PeftLoraLayer, PeftConv2d)


def replace_lora_layers_with_quantizable_layers(model: nn.Module):
    """aimet_torch/peft.py:120-127: every PEFT LoRA layer of the model becomes a LoraLayer, in place."""
    types = _peft_types()
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, LoraLayer):
                continue
            if is_peft_lora_layer(child) or (types and isinstance(child, types)):
                setattr(parent, name, LoraLayer(child))


# ---- meta data -----------------------------------------------------------------------------------
class AdapterMetaData:
    """aimet_torch/peft.py:130-140: the names of an adapter's lora_A, lora_B and mul_scale modules and
    its alpha."""

    def __init__(self):
        self.lora_A = []
        self.lora_B = []
        self.alpha = None
        self.mul_scale = []


def track_lora_meta_data(model: nn.Module, path: str, filename_prefix: str,
                         replaced_module_type: Type[nn.Module] = None) -> Dict[str, AdapterMetaData]:
    """aimet_torch/peft.py:143-180: adapter name -> AdapterMetaData of every LoraLayer of the model,
    returned and pickled to `<path>/<filename_prefix>.pkl`. replaced_module_type: a module type that
    replaced the adapters' layers and keeps the layer as `.conv2d`."""
    names = {module: name for name, module in model.named_modules()}
    meta = defaultdict(AdapterMetaData)
    for module in model.modules():
        if not isinstance(module, LoraLayer):
            continue
        for kind in ("lora_A", "lora_B"):
            for index, layer in enumerate(getattr(module, kind)):
                if replaced_module_type and isinstance(layer, replaced_module_type):
                    layer = layer.conv2d
                getattr(meta[module.index_to_adapter_name[index]], kind).append(names[layer])
        for adapter, alpha in module.lora_alpha.items():
            meta[adapter].alpha = alpha
        for adapter in module.adapter_name_to_index:
            meta[adapter].mul_scale.append(names[module.mul_scale])
    with open(os.path.join(path, "%s.pkl" % filename_prefix), "wb") as f:
        pickle.dump(meta, f)
    return meta


def _load_weights(adapter_weights_path: str, use_safetensor: bool, device) -> Dict[str, torch.Tensor]:
    if not use_safetensor:
        return torch.load(adapter_weights_path, map_location=device, weights_only=True)
    from safetensors import safe_open
    with safe_open(adapter_weights_path, framework="pt", device=str(device)) as f:
        return {key: f.get_tensor(key) for key in f.keys()}


class PeftQuantUtils:
    """aimet_torch/peft.py:183-457 on the v1 wrappers of aimet_amd. name_to_module_dict (the
    prepared-model / ONNX name mapping of the reference) is not supported: pass None."""

    def __init__(self, adapater_name_to_meta_data: Dict[str, AdapterMetaData], name_to_module_dict=None):
        if name_to_module_dict is not None:
            raise NotImplementedError("PeftQuantUtils: name_to_module_dict (prepared-model names) is not supported")
        self.adapter_name_to_meta_data = adapater_name_to_meta_data
        self.lora_layers = {name for meta in adapater_name_to_meta_data.values() for name in meta.lora_A + meta.lora_B}

    # -- which wrappers ------------------------------------------------------------------------------
    def _wrappers(self, sim, adapters: bool):
        for name, w in sim.quant_wrappers():
            if (name in self.lora_layers) == adapters:
                yield name, w

    def get_quantized_lora_layer(self, sim):
        """(name, wrapper) of every lora_A / lora_B layer of the sim."""
        yield from self._wrappers(sim, True)

    def get_fp_lora_layer(self, model):
        """(name, module) of every lora_A / lora_B layer of an unquantized model."""
        for name, module in model.named_modules():
            if name in self.lora_layers:
                yield name, module

    # -- freezing ------------------------------------------------------------------------------------
    @staticmethod
    def _freeze(quantizers):
        for q in quantizers:
            if q.enabled and q.bitwidth != 32 and not q.is_encoding_frozen:
                q.freeze_encoding()   # raises where compute_encodings has not run

    def freeze_base_model_param_quantizers(self, sim):
        for _, w in self._wrappers(sim, False):
            self._freeze(w.param_quantizers.values())

    def freeze_base_model_activation_quantizers(self, sim):
        for _, w in self._wrappers(sim, False):
            self._freeze(list(w.input_quantizers) + list(w.output_quantizers))

    def freeze_base_model(self, sim):
        """freeze_encoding() on every quantizer of every wrapper that is not a lora_A or lora_B layer:
        a later compute_encodings leaves them as they are."""
        self.freeze_base_model_activation_quantizers(sim)
        self.freeze_base_model_param_quantizers(sim)

    # -- adapter settings ----------------------------------------------------------------------------
    def set_bitwidth_for_lora_adapters(self, sim, output_bw: int, param_bw: int):
        for _, w in self._wrappers(sim, True):
            for q in w.output_quantizers:
                q.bitwidth = output_bw
            for q in w.param_quantizers.values():
                q.bitwidth = param_bw

    def quantize_lora_scale_with_fixed_range(self, sim, bitwidth, scale_min=0.0, scale_max=1e-5):
        """Quantizes the scale (alpha / rank) operand of every mul_scale: its second input quantizer is
        enabled with the TF encoding of [scale_min, scale_max] at `bitwidth` and frozen. Such a layer
        takes the literal route."""
        for module in sim.model.modules():
            if not isinstance(module, LoraLayer) or not isinstance(module.mul_scale, QcQuantizeWrapper):
                continue
            _ensure_input_quantizers(module.mul_scale, 2)
            q = module.mul_scale.input_quantizers[1]
            q._is_encoding_frozen = False
            q.enabled, q.bitwidth, q.use_symmetric_encodings = True, bitwidth, False
            q.encoding = getComputedEncodings(bitwidth, float(scale_min), float(scale_max), False, False, False)
            q.freeze_encoding()

    # -- adapter weights -----------------------------------------------------------------------------
    def _adapter_params(self, sim):
        for name, w in self._wrappers(sim, True):
            for pname, param in w.get_original_module().named_parameters():
                if pname in ("weight", "bias"):
                    yield "%s.%s" % (name, pname), param

    def export_adapter_weights(self, sim, path: str, filename_prefix: str):
        """`<path>/<filename_prefix>.safetensor`: the weight and bias of every lora_A / lora_B layer
        under `<layer name>.<parameter>`."""
        from safetensors.torch import save_file
        tensors = {key: p.detach().contiguous() for key, p in self._adapter_params(sim)}
        save_file(tensors, os.path.join(path, filename_prefix + ".safetensor"))

    def enable_adapter_and_load_weights(self, sim, adapter_weights_path, use_safetensor: bool = True):
        """Loads adapter weights (a safetensors file, or a torch .bin state dict) into the sim, on the
        model's device. KeyError when a lora layer's weight is missing or a key names no lora layer."""
        tensors = _load_weights(adapter_weights_path, use_safetensor, _model_device(sim.model))
        params = dict(self._adapter_params(sim))
        missing = {key for key in params if key.endswith(".weight")} - set(tensors)
        unknown = set(tensors) - set(params)
        if missing or unknown:
            raise KeyError("Lora layer weights missing for the following names", sorted(missing), "unknown", sorted(unknown))
        with torch.no_grad():
            for key, t in tensors.items():
                params[key].copy_(t)

    def disable_lora_adapters(self, sim):
        """Zeroes the weights (and biases) of every lora_A / lora_B layer: the base model alone."""
        with torch.no_grad():
            for _, param in self._adapter_params(sim):
                param.zero_()
