"""FP8 fake-quantization and its range setting on the MI355X core.

Mirrors aimet_torch/fp_quantization.py (same names and call signatures). The reference evaluates
the cast as about a dozen elementwise torch ops per tensor and ``init_mse`` runs that chain 111
times per batch; here the cast is one streaming kernel and the 111-candidate search reads the
tensor once (csrc/fp8.hip, DESIGN.md "FP8"). The kernels compute the function the reference's
float32 log2 / pow chain approximates, so outputs agree with it to a few ulp except at rounding
ties, and a non-positive or non-finite ``maxval`` leaves the clamped input instead of NaN.

fp16 / bf16 tensors are upcast to float32 around the kernels; CPU tensors are staged through HBM.
"""
import ctypes

import torch

from aimet_amd import _native
from aimet_amd.quantizers import QuantScheme   # defined before quantizers imports this module
from aimet_amd.tensor_quantizer import _stage, _stream, per_channel_view

NUM_MANTISSA_BITS = 3
NUM_CANDIDATES = 111   # init_mse: torch.linspace(0.1 * mx, 1.2 * mx, 111)
# the search's quotient: False multiplies by the candidate's reciprocal (moves only elements at a
# rounding tie, where both neighbours are equally far), True keeps the cast's IEEE divide
SEARCH_EXACT_DIVIDE = False


def _mantissa_bits(mantissa_bits) -> int:
    m = mantissa_bits
    if isinstance(m, torch.Tensor):
        if m.numel() != 1:
            raise ValueError("mantissa_bits must be one number")
        m = m.item()
    if float(m) != int(m) or not 1 <= int(m) <= 6:
        raise ValueError("FP8 mantissa bits must be an integer in 1..6, got %r" % (mantissa_bits,))
    return int(m)


def _device_fp32(t, what):
    """(contiguous float32 HIP tensor, staged)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % what)
    if not t.is_floating_point():
        raise TypeError("aimet_amd: %s must be a floating-point tensor (got %s)" % (what, t.dtype))
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    t, staged = _stage(t, what)
    return t.contiguous(), staged


def _view(t, per_channel, ch_axis):
    if not per_channel:
        return 1, 1, t.numel()
    if t.dim() == 0:
        raise ValueError("per-channel FP8 quantization needs a tensor with a channel axis")
    return per_channel_view(t.shape, 0 if ch_axis is None else ch_axis)


def _workspace(t, outer, C, K):
    nbytes = ctypes.c_int64()
    _native.call("aimet_fp8_search_workspace", outer, C, K, ctypes.byref(nbytes))
    return torch.empty(max(1, (nbytes.value + 3) // 4), dtype=torch.float32, device=t.device), nbytes.value


def abs_max(tensor, per_channel=False, ch_axis=0):
    """max |x| per tensor (0-dim) or per channel ([C]) as a float32 HIP tensor; NaN is ignored."""
    t, _ = _device_fp32(tensor, "tensor")
    if t.numel() == 0:
        raise ValueError("abs_max of an empty tensor")
    outer, C, K = _view(t, per_channel, ch_axis)
    out = torch.empty(C, dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        ws, nbytes = _workspace(t, outer, C, K)
        _native.call("aimet_fp8_absmax", t.data_ptr(), outer, C, K, out.data_ptr(), ws.data_ptr(), nbytes,
                     _stream(t))
    return out if per_channel else out.reshape(())


def mse_search(tensor, mantissa_bits=None, per_channel=False, ch_axis=0, details=False, exact_divide=None):
    """The 111-candidate search of init_mse in two launches after max|x|: the chosen maxval per
    tensor ([1]) or per channel ([C]). ``details=True`` also returns the candidate table [111][C],
    the squared-error sums [C][111] and the chosen indices [C]."""
    M = _mantissa_bits(NUM_MANTISSA_BITS if mantissa_bits is None else mantissa_bits)
    t, _ = _device_fp32(tensor, "tensor")
    if t.numel() == 0:
        raise ValueError("FP8 range search of an empty tensor")
    outer, C, K = _view(t, per_channel, ch_axis)
    exact = SEARCH_EXACT_DIVIDE if exact_divide is None else exact_divide
    best = torch.empty(C, dtype=torch.float32, device=t.device)
    mx = torch.empty(C, dtype=torch.float32, device=t.device)
    losses = cands = index = None
    if details:
        losses = torch.empty((C, NUM_CANDIDATES), dtype=torch.float32, device=t.device)
        cands = torch.empty((NUM_CANDIDATES, C), dtype=torch.float32, device=t.device)
        index = torch.empty(C, dtype=torch.int32, device=t.device)
    with torch.cuda.device(t.device):
        ws, nbytes = _workspace(t, outer, C, K)
        s = _stream(t)
        _native.call("aimet_fp8_absmax", t.data_ptr(), outer, C, K, mx.data_ptr(), ws.data_ptr(), nbytes, s)
        _native.call("aimet_fp8_mse_search", t.data_ptr(), outer, C, K, mx.data_ptr(), M, int(bool(exact)),
                     best.data_ptr(), losses.data_ptr() if details else None,
                     cands.data_ptr() if details else None, index.data_ptr() if details else None,
                     ws.data_ptr(), nbytes, s)
    if details:
        return best, cands, losses, index
    return best


def init_minmax(tensor, tensor_quantizer, per_channel):
    """Minmax initialization: max |x| of the tensor (0-dim) or of every channel ([C])."""
    if per_channel:
        maxval = abs_max(tensor, True, tensor_quantizer.channel_axis)
        tensor_quantizer.fp8_maxval = maxval.clone()
        return maxval
    return abs_max(tensor, False)


def init_mse(tensor, tensor_quantizer, per_channel):
    """MSE initialization (nearly equivalent to tf_enhanced): of the 111 candidate maxima
    linspace(0.1 * mx, 1.2 * mx, 111) the first one of least mean squared FP8 error, per tensor
    ([1]) or per channel ([C])."""
    return mse_search(tensor, NUM_MANTISSA_BITS, per_channel, tensor_quantizer.channel_axis if per_channel else 0)


def init_percentile(*_):
    """Percentile range initialization"""
    raise NotImplementedError("Percentile scheme is not supported for FP8")


INIT_MAP = {
    QuantScheme.post_training_tf: init_minmax,            # minmax
    QuantScheme.post_training_tf_enhanced: init_mse,      # MSE
    QuantScheme.post_training_percentile: init_percentile,
}


def fp8_quantizer(tensor, tensor_quantizer, _):
    """FP8 quantization entry function."""
    if getattr(tensor_quantizer, "fp8_maxval", None) is None:
        raise ValueError("tensor_quantizer.fp8_maxval not present or not initialized!")
    return quantize_to_fp8(tensor, tensor_quantizer.fp8_maxval, NUM_MANTISSA_BITS, tensor_quantizer.channel_axis)


def scale_table(maxval, mantissa_bits=None):
    """The device table [C][2] = {maxval, alpha} the QDQ kernel reads, from a float32 HIP tensor
    of C maxvals: one small launch, nothing read back."""
    M = _mantissa_bits(NUM_MANTISSA_BITS if mantissa_bits is None else mantissa_bits)
    mv = maxval.detach().reshape(-1).to(torch.float32).contiguous()
    table = torch.empty((mv.numel(), 2), dtype=torch.float32, device=mv.device)
    with torch.cuda.device(mv.device):
        _native.call("aimet_fp8_scale_table", mv.data_ptr(), mv.numel(), M, table.data_ptr(), _stream(mv))
    return table


def quantize_to_fp8(x_float, maxval, mantissa_bits=None, per_channel_axis=0):
    """Fake-cast x to FP8 with ``mantissa_bits`` mantissa and 7 - mantissa_bits exponent bits whose
    largest value is ``maxval``: one number / one-element tensor (per tensor), or C values along
    ``per_channel_axis`` (a [C] tensor, or one shaped like x with every other axis 1)."""
    M = _mantissa_bits(NUM_MANTISSA_BITS if mantissa_bits is None else mantissa_bits)
    dtype = x_float.dtype if isinstance(x_float, torch.Tensor) else None
    t, staged = _device_fp32(x_float, "x_float")
    mv = torch.as_tensor(maxval, dtype=torch.float32).detach()
    if mv.device != t.device:
        mv = mv.to(t.device)
    if mv.numel() == 1:
        outer, C, K = 1, 1, t.numel()
    else:
        axis = 0 if per_channel_axis is None else per_channel_axis
        if mv.dim() == t.dim() and mv.dim() > 0:
            full = [i for i, s in enumerate(mv.shape) if s != 1]
            if len(full) > 1:
                raise ValueError("maxval must vary along one axis only, got shape %s" % (tuple(mv.shape),))
            axis = full[0]
        outer, C, K = per_channel_view(t.shape, axis)
        if mv.numel() != C:
            raise ValueError("expected %d per-channel maxvals, got %d" % (C, mv.numel()))
    out = torch.empty_like(t)
    if t.numel():
        table = scale_table(mv, M)
        with torch.cuda.device(t.device):
            _native.call("aimet_fp8_qdq", t.data_ptr(), out.data_ptr(), outer, C, K, table.data_ptr(), M,
                         _stream(t))
    out = out.to(dtype)
    return out.cpu() if staged else out
