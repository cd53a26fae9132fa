"""OCP Microscaling (MX) fake-quantization: MXFP8, MXFP6 and MXFP4.

A block of 32 values along one axis shares a power-of-two scale (E8M0) taken from the block's own
maximum; the elements are FP8 (E4M3, E5M2), FP6 (E3M2, E2M3) or FP4 (E2M1), rounded to nearest even and
saturated. The scale is dynamic: it is recomputed from the tensor at every call, so there is nothing
to calibrate and an MX quantizer has its "encoding" from construction. The arithmetic contract is the
header comment of csrc/mx.hip; each function here is one launch of that file's kernels, and there is no
CPU path.

* ``mx_quantize_dequantize(tensor, fmt, axis)``: the fake-quantized tensor, identity gradient;
* ``mx_quantize`` / ``mx_dequantize``: the packed form (scale bytes and element codes), last axis;
* ``MxQuantizer``: the quantizer object a StaticGridQuantWrapper holds for a parameter or an activation;
* ``set_mx_quantization(sim, module_types, weight_format, activation_format)``: Linear / Conv weights
  along their input features and, with an activation format, their inputs along the same reduction
  axis, as the hardware's scaled matrix instructions take both operands.
"""
import ctypes
import enum
import warnings
from typing import Optional, Tuple, Union

import torch
from torch import nn

from aimet_amd import _native
from aimet_amd.libpymo import TfEncoding
from aimet_amd.quantizers import QuantizationDataType, StaticGridTensorQuantizer

MX_BLOCK_SIZE = 32


class MxFormat(enum.Enum):
    """The element formats; the value is csrc/mx.hip's format code."""
    MXFP8_E4M3 = 0
    MXFP8_E5M2 = 1
    MXFP6_E3M2 = 2
    MXFP6_E2M3 = 3
    MXFP4_E2M1 = 4

    @property
    def element_bits(self) -> int:
        return (8, 8, 6, 6, 4)[self.value]


def launch_count(reset: bool = False) -> int:
    """Launches of the MX kernels in this process."""
    n = ctypes.c_int64(0)
    _native.call("aimet_mx_launch_count", ctypes.byref(n), int(reset))
    return n.value


def _check(tensor, what: str):
    """The I/O code of a float tensor; TypeError for anything else."""
    if not isinstance(tensor, torch.Tensor):
        raise TypeError("MX quantization takes a torch.Tensor, not %s" % type(tensor).__name__)
    return _native.io_code(tensor.dtype, TypeError, what + " takes float32, float16 or bfloat16 tensors (got %s)")


def _require_hip(tensor):
    if not tensor.is_cuda:
        raise RuntimeError("aimet_amd: MX quantization runs on the HIP device the tensor is on; there is no CPU path")


def _block_view(shape, axis: int) -> Tuple[int, int, int]:
    """(outer, K, inner) of a contiguous tensor with the block along `axis`."""
    if len(shape) == 0 or not -len(shape) <= axis < len(shape):
        raise ValueError("axis %d is out of range for a tensor of shape %s" % (axis, tuple(shape)))
    axis %= len(shape)
    K = int(shape[axis])
    if K == 0 or K % MX_BLOCK_SIZE != 0:
        raise ValueError("axis %d of shape %s has length %d, not a positive multiple of the MX block size %d"
                         % (axis, tuple(shape), K, MX_BLOCK_SIZE))
    outer = inner = 1
    for s in shape[:axis]:
        outer *= int(s)
    for s in shape[axis + 1:]:
        inner *= int(s)
    return outer, K, inner


def _qdq(tensor, fmt: MxFormat, axis: int, out=None):
    code = _check(tensor, "mx_quantize_dequantize")
    outer, K, inner = _block_view(tensor.shape, axis)
    _require_hip(tensor)
    t = tensor.detach()
    t = t if t.is_contiguous() else t.contiguous()
    if out is None:
        out = torch.empty_like(t)
    elif not (out.is_cuda and out.is_contiguous() and out.dtype == t.dtype and out.shape == t.shape):
        raise ValueError("the output must be a contiguous HIP tensor of the input's dtype and shape")
    if t.numel():
        with torch.cuda.device(t.device):
            _native.call("aimet_mx_qdq", t.data_ptr(), out.data_ptr(), outer, K, inner, code, fmt.value,
                         torch.cuda.current_stream(t.device).cuda_stream)
    return out


class _MxQdq(torch.autograd.Function):
    """MX fake-quantization going forward, the gradient unchanged going back (saturation only touches
    the top of a block's own range: the convention of MX training)."""

    @staticmethod
    def forward(ctx, tensor, fmt, axis):
        return _qdq(tensor, fmt, axis)

    @staticmethod
    def backward(ctx, grad):
        return grad, None, None


def mx_quantize_dequantize(tensor: torch.Tensor, fmt: MxFormat, axis: int = -1,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`tensor` fake-quantized to `fmt` in blocks of 32 along `axis`, in one launch. float32, float16 or
    bfloat16 on a HIP device (TypeError, RuntimeError); a non-contiguous tensor is made contiguous; the
    axis length must be a multiple of 32 (ValueError). Differentiable with the identity gradient. `out`
    (no gradient is recorded then) receives the result and may be `tensor` itself."""
    if out is None and torch.is_grad_enabled() and isinstance(tensor, torch.Tensor) and tensor.requires_grad:
        _check(tensor, "mx_quantize_dequantize")
        return _MxQdq.apply(tensor, fmt, axis)
    return _qdq(tensor, fmt, axis, out)


def mx_quantize(tensor: torch.Tensor, fmt: MxFormat) -> Tuple[torch.Tensor, torch.Tensor]:
    """The packed form of `tensor`, blocks along its last axis of length K: (scales, codes), uint8 tensors
    of shape [..., K / 32] (the E8M0 byte; 0xFF for a block with a NaN or an Inf, whose codes are zero) and
    [..., K w / 8] (element i of a block at bits [w i, w i + w) of the block's little-endian bit string)."""
    code = _check(tensor, "mx_quantize")
    _, K, _ = _block_view(tensor.shape, -1)
    _require_hip(tensor)
    t = tensor.detach().contiguous()
    lead = tuple(t.shape[:-1])
    scales = torch.empty(lead + (K // MX_BLOCK_SIZE,), dtype=torch.uint8, device=t.device)
    codes = torch.empty(lead + (K * fmt.element_bits // 8,), dtype=torch.uint8, device=t.device)
    if t.numel():
        with torch.cuda.device(t.device):
            _native.call("aimet_mx_quantize", t.data_ptr(), scales.data_ptr(), codes.data_ptr(), t.numel() // K, K,
                         code, fmt.value, torch.cuda.current_stream(t.device).cuda_stream)
    return scales, codes


def mx_dequantize(scales: torch.Tensor, codes: torch.Tensor, fmt: MxFormat,
                  dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The tensor mx_quantize's (scales, codes) stand for, as `dtype`:
    ``mx_dequantize(*mx_quantize(x, fmt), fmt, x.dtype)`` equals ``mx_quantize_dequantize(x, fmt)``."""
    code = _native.io_code(dtype, TypeError, "mx_dequantize produces float32, float16 or bfloat16 (got %s)")
    if scales.dtype != torch.uint8 or codes.dtype != torch.uint8:
        raise TypeError("scales and codes are uint8 tensors")
    _require_hip(scales)
    _require_hip(codes)
    if scales.dim() == 0 or scales.shape[-1] == 0:
        raise ValueError("scales needs a last axis of at least one block")
    K = scales.shape[-1] * MX_BLOCK_SIZE
    if codes.shape != scales.shape[:-1] + (K * fmt.element_bits // 8,) or codes.device != scales.device:
        raise ValueError("codes of shape %s do not belong to scales of shape %s in %s"
                         % (tuple(codes.shape), tuple(scales.shape), fmt.name))
    scales, codes = scales.contiguous(), codes.contiguous()
    out = torch.empty(tuple(scales.shape[:-1]) + (K,), dtype=dtype, device=scales.device)
    if out.numel():
        with torch.cuda.device(out.device):
            _native.call("aimet_mx_dequantize", scales.data_ptr(), codes.data_ptr(), out.data_ptr(), out.numel() // K,
                         K, code, fmt.value, torch.cuda.current_stream(out.device).cuda_stream)
    return out


class MxQuantizer(StaticGridTensorQuantizer):
    """Static-grid quantizer of a parameter or an activation in an MX format, blocks along `axis`.

    The scale comes from the tensor at every call, so the statistics interface does nothing and the
    quantizer counts as having an encoding from construction: compute_encodings leaves it enabled,
    freeze_encoding works, and a wrapper in ANALYSIS mode passes an activation through as it does for
    every quantizer still calibrating."""

    computes_own_encoding = True   # compute_encodings_batched leaves this quantizer to itself

    def __init__(self, fmt: MxFormat, axis: int = -1, round_mode="nearest", quant_scheme=None,
                 enabled_by_default: bool = True):
        super().__init__(fmt.element_bits, round_mode, quant_scheme, True, enabled_by_default,
                         QuantizationDataType.float)
        self.format, self.axis = fmt, int(axis)
        placeholder = TfEncoding()   # what a float quantizer's encoding is: a bitwidth
        placeholder.bw = fmt.element_bits
        self._encoding = [placeholder]

    def _make_op(self):
        self._cppOp = None

    def __str__(self):
        return "MX TensorQuantizer: format=%s, block_size=%d, axis=%d, enabled=%s\n" % (
            self.format.name, MX_BLOCK_SIZE, self.axis, self.enabled)

    @property
    def encoding(self):
        return self._encoding[0]

    def update_encoding_stats(self, tensor):
        pass

    def compute_encoding(self):
        pass

    def reset_encoding_stats(self):
        pass

    def set_percentile_value(self, percentile_value):
        pass

    def quantize_dequantize(self, tensor, round_mode=None):
        """MX rounds to nearest even by definition: the round mode is ignored."""
        if not self.enabled:
            return tensor
        return mx_quantize_dequantize(tensor, self.format, self.axis)

    def quantize(self, tensor, round_mode=None):
        raise NotImplementedError("quantize-only output of an MX quantizer; mx_quantize gives the packed form")

    def export_encodings(self):
        if not self.enabled:
            return None
        return [{"dtype": "float", "bitwidth": self.bitwidth, "block_size": MX_BLOCK_SIZE, "format": self.format.name,
                 "axis": self.axis}]


_CONV_TYPES = (nn.Conv1d, nn.Conv2d, nn.Conv3d)


def _reduction_length(module: nn.Module) -> int:
    """The length of `module`'s weight along axis 1, its reduction axis; ValueError for a layer MX
    quantization does not cover."""
    if isinstance(module, (nn.ConvTranspose1d, nn.ConvTranspose2d, nn.ConvTranspose3d)):
        raise ValueError("a transposed convolution reduces along axis 0 of its weight")
    if not isinstance(module, (nn.Linear,) + _CONV_TYPES):
        raise ValueError("MX quantization covers Linear and Conv weights, not %s" % type(module).__name__)
    if getattr(module, "groups", 1) != 1:
        raise ValueError("grouped and depthwise convolutions (groups=%d) are not covered" % module.groups)
    K = module.weight.shape[1]
    if K % MX_BLOCK_SIZE != 0:
        raise ValueError("its reduction length %d is not a multiple of %d" % (K, MX_BLOCK_SIZE))
    return K


def set_mx_quantization(sim, module_types: Union[type, Tuple[type, ...]], weight_format: MxFormat,
                        activation_format: Optional[MxFormat] = None):
    """The weight quantizers of the sim's wrapped Linear and Conv (groups == 1) layers of the given types
    become MxQuantizers in `weight_format`, blocks along the input features (axis 1). With
    `activation_format`, input quantizer 0 of the same layers becomes one along the activation's
    reduction axis (the last axis of a Linear's input, axis 1 of a Conv's) and is enabled, so both
    GEMM operands are blocked along the reduction. A layer of a matching type whose reduction length is
    not a multiple of 32, or that is grouped or transposed, keeps its quantizers; one warning names it.
    Returns the names of the converted wrappers.

    Static-grid sims only: a range-learning sim is refused (NotImplementedError), its wrappers hand
    every quantizer a pair of trainable ranges that an MX quantizer has no use for. Sharded calibration
    keeps refusing activation quantizers it does not know, an MX one among them, although it has no
    statistics to exchange: calibrate such a sim with ``sharded=False``."""
    from aimet_amd.qc_quantize_op import StaticGridQuantWrapper
    from aimet_amd.quantsim import _RANGE_LEARNING
    if sim._quant_scheme in _RANGE_LEARNING:
        raise NotImplementedError("MX quantization on a range-learning sim is not implemented")
    if isinstance(module_types, type):
        module_types = (module_types,)
    converted = []
    for name, w in sim.quant_wrappers():
        module = w._module_to_wrap
        old = w.param_quantizers.get("weight")
        if not isinstance(w, StaticGridQuantWrapper) or not isinstance(module, tuple(module_types)) or old is None:
            continue
        try:
            _reduction_length(module)
        except ValueError as e:
            warnings.warn("set_mx_quantization: %s keeps its quantizers: %s" % (name, e))
            continue
        w.param_quantizers["weight"] = MxQuantizer(weight_format, 1, old.round_mode, old.quant_scheme, old.enabled)
        if activation_format is not None:
            act = w.input_quantizers[0]
            axis = -1 if isinstance(module, nn.Linear) else 1
            w.input_quantizers[0] = MxQuantizer(activation_format, axis, act.round_mode, act.quant_scheme, True)
        converted.append(name)
    return converted
