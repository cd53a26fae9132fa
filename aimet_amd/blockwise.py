"""Blockwise and LPBQ (low-power blockwise) weight quantization in QuantizationSimModel.

Reference: aimet_onnx/quantsim.py:1136-1240 (set_blockwise_quantization_for_weights,
set_grouped_blockwise_quantization_for_weights), aimet_onnx/qc_quantize_op.py:139-160, 586-666
(the blockwise QcQuantizeOp and GroupedBlockQuantizeDequantize) and lpbq_utils.py. The reference
keeps one analyzer and one encoding object per block on the host; here a weight's encodings are
device arrays computed where the weight is, by one launch (aimet_bq_encode_qdq, csrc/blockwise.hip)
that also yields the quantize-dequantized weight.

Differences from the rest of the sim, all deliberate:

* calibration is min/max per block (the TF analyzer) whatever the sim's ``quant_scheme``: a
  histogram per block of 64 weights has nothing to say;
* only contiguous blocks: the weight is viewed as [out channels][blocks][block_size * kernel
  elements], which holds for Linear and Conv weights with the block along the input features. A
  transposed convolution (strided blocks) and a grouped or depthwise one are not converted;
* range learning is opt-in: ``set_blockwise_quantization_for_weights(..., learn_ranges=True)`` on a
  range-learning sim calibrates as above and then trains one (min, max) pair per block
  (LearnedBlockwiseQuantizer on the block kernels of csrc/lg_block.hip); without the keyword a
  range-learning sim is refused (NotImplementedError), and learned LPBQ scales always are.
"""
import collections.abc
import ctypes
from typing import Optional, Tuple, Union

import torch
from torch import nn

from aimet_amd import _native
from aimet_amd.learned_grid import LearnedGridTensorQuantizer, quantize_dequantize_blocks
from aimet_amd.libpymo import RoundingMode, TfEncoding
from aimet_amd.quantizers import (QuantizationDataType, StaticGridTensorQuantizer, _round_mode, compute_dloss_by_dx)
from aimet_amd.tensor_quantizer import qdq_per_channel_table

PATH_WAVE, PATH_GROUP, PATH_TWO_PASS = 0, 1, 2


def launch_count(reset: bool = False) -> int:
    """Launches of aimet_bq_encode_qdq in this process."""
    n = ctypes.c_int64(0)
    _native.call("aimet_bq_launch_count", ctypes.byref(n), int(reset))
    return n.value


def row_path(NB: int, BL: int, dtype=torch.float32) -> int:
    """Where the kernel keeps a row of NB blocks of BL elements: PATH_WAVE, PATH_GROUP or PATH_TWO_PASS."""
    p = ctypes.c_int(0)
    _native.call("aimet_bq_row_path", int(NB), int(BL), _native.IO_CODES[dtype], ctypes.byref(p))
    return p.value


def encode_qdq(t: torch.Tensor, R: int, NB: int, BL: int, bitwidth: int, symmetric: bool, strict: bool = False,
               unsigned: bool = False, scale_bitwidth: int = 0, out: Optional[torch.Tensor] = None):
    """One aimet_bq_encode_qdq launch over the contiguous HIP tensor `t` viewed as [R][NB][BL].
    Returns (table float32 [4, R NB], q int32 [R NB] or None, factor float64 [R] or None); `out`
    (may be `t`) receives the quantize-dequantized weight."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("aimet_amd: blockwise quantization computes its encodings on the HIP device the weight "
                           "is on; there is no CPU path")
    code = _native.io_code(t.dtype, TypeError, "blockwise quantization takes float32, float16 or bfloat16 weights "
                                               "(got %s)")
    if not t.is_contiguous() or t.numel() != R * NB * BL:
        raise ValueError("expected a contiguous tensor of %d x %d x %d elements" % (R, NB, BL))
    if out is not None and not (out.is_cuda and out.is_contiguous() and out.dtype == t.dtype and
                                out.numel() == t.numel()):
        raise ValueError("the output must be a contiguous HIP tensor of the input's dtype and size")
    E = R * NB
    table = torch.empty((4, E), dtype=torch.float32, device=t.device)
    q = factor = None
    if scale_bitwidth > 0:
        q = torch.empty(E, dtype=torch.int32, device=t.device)
        factor = torch.empty(R, dtype=torch.float64, device=t.device)
    with torch.cuda.device(t.device):
        _native.call("aimet_bq_encode_qdq", t.data_ptr(), None if out is None else out.data_ptr(), R, NB, BL,
                     code, int(bitwidth), int(bool(symmetric)), int(bool(strict)), int(bool(unsigned)),
                     int(scale_bitwidth), table.data_ptr(), None if q is None else q.data_ptr(),
                     None if factor is None else factor.data_ptr(), torch.cuda.current_stream(t.device).cuda_stream)
    return table, q, factor


def block_view(shape, block_size: int, channel_axis: int = 0, block_axis: int = 1) -> Tuple[int, int, int]:
    """(R, NB, BL) of a contiguous weight of `shape`; ValueError where the blocks are not contiguous
    or block_size does not divide the block axis."""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 2 or channel_axis != 0 or block_axis != 1:
        raise ValueError("blockwise quantization needs the channel on axis 0 and the block on axis 1 (contiguous "
                         "blocks); channel axis %d with block axis %d gives strided blocks" % (channel_axis, block_axis))
    if block_size <= 0 or shape[1] % block_size != 0:
        raise ValueError("input features %d of shape %s are not divisible by block size %d"
                         % (shape[1], shape, block_size))
    inner = 1
    for s in shape[2:]:
        inner *= s
    return shape[0], shape[1] // block_size, block_size * inner


class _BlockEncodings(collections.abc.Sequence):
    """The E encodings of a blockwise quantizer as host TfEncoding objects, built from the device
    table the first time one is asked for."""

    def __init__(self, table: torch.Tensor, bitwidth: int):
        self._table, self._bw, self._host = table, bitwidth, None

    def _list(self):
        if self._host is None:
            cols = self._table.detach().to("cpu", torch.float64).tolist()
            self._host = []
            for mn, mx, d, o in zip(*cols):
                e = TfEncoding()
                e.min, e.max, e.delta, e.offset, e.bw = mn, mx, d, o, self._bw
                self._host.append(e)
        return self._host

    def __len__(self):
        return self._table.shape[1]

    def __getitem__(self, i):
        return self._list()[i]


class _BlockQdq(torch.autograd.Function):
    """QDQ with the table going forward, grad * (min_b <= w <= max_b) going back."""

    @staticmethod
    def forward(ctx, tensor, quantizer, round_mode):
        ctx.quantizer = quantizer
        ctx.save_for_backward(tensor)
        return quantizer._qdq_values(tensor, round_mode)

    @staticmethod
    def backward(ctx, grad):
        (x,) = ctx.saved_tensors
        return ctx.quantizer.ste_backward(x, grad), None, None


class BlockwiseQuantizer(StaticGridTensorQuantizer):
    """Static-grid parameter quantizer with one encoding per block of `block_size` input features
    of every output channel, and with `decompressed_bw` the LPBQ form: block scales that are
    integers of decompressed_bw - bitwidth bits times one scale per output channel.

    The encodings are a device table [4][E] {min, max, delta, offset} in [channel][block] order
    (`table`; for LPBQ also `int_scale` [E] and `channel_scale` [R]). compute_encoding() is one fused
    launch on the tensor given to update_encoding_stats(); the quantize-dequantized weight it also
    yields serves the next quantize_dequantize() of that tensor."""

    computes_own_encoding = True   # compute_encodings_batched leaves this quantizer to itself

    def __init__(self, shape, bitwidth: int, round_mode, quant_scheme, use_symmetric_encodings: bool,
                 block_size: int, channel_axis: int = 0, block_axis: int = 1, decompressed_bw: Optional[int] = None,
                 enabled_by_default: bool = True):
        super().__init__(bitwidth, round_mode, quant_scheme, use_symmetric_encodings, enabled_by_default,
                         QuantizationDataType.int)
        self.R, self.NB, self.BL = block_view(shape, block_size, channel_axis, block_axis)
        if decompressed_bw is not None:
            if not use_symmetric_encodings:
                raise ValueError("LPBQ (decompressed_bw) is symmetric only")
            if decompressed_bw <= bitwidth:
                raise ValueError("decompressed_bw %d must exceed bitwidth %d" % (decompressed_bw, bitwidth))
        self.shape = tuple(int(s) for s in shape)
        self.block_size, self._ch_axis, self.block_axis = int(block_size), channel_axis, block_axis
        self.decompressed_bw = decompressed_bw
        self.learn_ranges = False   # a range-learning sim turns this quantizer into a LearnedBlockwiseQuantizer
        self.table = self.int_scale = self.channel_scale = None
        self._pending = self._fused = self._lazy = None

    # -- the parts of StaticGridTensorQuantizer that assume a native analyzer object ---------------
    def _make_op(self):
        self._cppOp = None

    def set_percentile_value(self, percentile_value):
        pass   # min/max per block whatever the scheme

    def __str__(self):
        return "Blockwise TensorQuantizer: bitwidth=%d, block_size=%d, decompressed_bw=%s, enabled=%s, %s\n" % (
            self.bitwidth, self.block_size, self.decompressed_bw, self.enabled,
            "no encoding" if self.table is None else "%d encodings" % self.table.shape[1])

    def __getstate__(self):
        state = super().__getstate__()
        for k in ("_pending", "_fused", "_lazy"):
            state[k] = None
        return state

    @property
    def channel_axis(self):
        return self._ch_axis

    @property
    def scale_bitwidth(self) -> int:
        return 0 if self.decompressed_bw is None else self.decompressed_bw - self.bitwidth

    @property
    def num_encodings(self) -> int:
        return self.R * self.NB

    @property
    def encoding(self):
        if self.table is None:
            return None
        if self._lazy is None or self._lazy._table is not self.table:
            self._lazy = _BlockEncodings(self.table, self.bitwidth)
        return self._lazy

    def reset_encoding_stats(self):
        if not self._is_encoding_frozen:
            self.table = self.int_scale = self.channel_scale = None
            self._pending = self._fused = None

    def freeze_encoding(self):
        if self.table is None:
            raise RuntimeError("Encoding can be frozen only when it is not None.")
        self._is_encoding_frozen = True

    def update_encoding_stats(self, tensor):
        """The tensor compute_encoding() will calibrate on (a weight has one batch: itself)."""
        if not self.enabled or self._is_encoding_frozen or self.bitwidth == 32:
            return
        self._pending = tensor

    def compute_encoding(self):
        """The one fused launch: block min/max, encodings, LPBQ compression and the weight's QDQ."""
        if not self.enabled or self._is_encoding_frozen or self._pending is None:
            return
        t, self._pending = self._pending, None
        if tuple(t.shape) != self.shape:
            raise ValueError("blockwise quantizer of a %s weight got a tensor of shape %s" % (self.shape, tuple(t.shape)))
        src = t.detach()
        src = src if src.is_contiguous() else src.contiguous()
        out = torch.empty_like(src)   # encode_qdq refuses a CPU tensor: there is no CPU path
        self.table, self.int_scale, self.channel_scale = encode_qdq(
            src, self.R, self.NB, self.BL, self.bitwidth, self.use_symmetric_encodings, self.use_strict_symmetric,
            self.use_unsigned_symmetric, self.scale_bitwidth, out)
        self._fused = (self._key(t), out)

    def set_block_ranges(self, mins: torch.Tensor, maxs: torch.Tensor):
        """Encodings from one chosen (min, max) range per block ([E] each, the table's order) instead
        of the weight's own, then frozen: what a blockwise quantizer computes from
        ``stack([x_min, x_max])`` (aimet_torch/v2/seq_mse.py compute_param_encodings). One
        aimet_bq_encode_qdq launch on the [R][NB][2] tensor of pairs with the quantizer's symmetry flags
        and scale bitwidth, so LPBQ compresses the chosen block scales by the calibration kernel's
        arithmetic. The quantizer's own block length (the weight's) stays."""
        if self._is_encoding_frozen:
            raise RuntimeError("Encoding can be set only when it is not frozen.")
        E = self.num_encodings
        if tuple(mins.shape) != (E,) or tuple(maxs.shape) != (E,):
            raise ValueError("expected %d block minima and maxima, got %s and %s"
                             % (E, tuple(mins.shape), tuple(maxs.shape)))
        pairs = torch.stack([mins.detach(), maxs.detach()], dim=-1).to(torch.float32).contiguous()
        self.table, self.int_scale, self.channel_scale = encode_qdq(
            pairs, self.R, self.NB, 2, self.bitwidth, self.use_symmetric_encodings, self.use_strict_symmetric,
            self.use_unsigned_symmetric, self.scale_bitwidth)
        self._pending = self._fused = None
        self.freeze_encoding()

    @staticmethod
    def _key(t):
        return (t.data_ptr(), t._version, tuple(t.shape), t.dtype, t.device)

    def _table_on(self, device):
        if self.table.device != device:
            self.table = self.table.to(device)
        return self.table

    def _qdq_values(self, tensor, round_mode):
        fused, self._fused = self._fused, None
        if fused is not None and fused[0] == self._key(tensor) and round_mode == RoundingMode.ROUND_NEAREST:
            return fused[1]
        if self.table is None:
            raise RuntimeError("the blockwise quantizer has no encoding; run compute_encodings first")
        if not tensor.is_cuda:
            raise RuntimeError("aimet_amd: blockwise quantization has no CPU path")
        dtype = tensor.dtype
        t = tensor.detach() if dtype in _native.IO_CODES else tensor.detach().to(torch.float32)
        t = t.contiguous()
        if t.numel() != self.num_encodings * self.BL:
            raise ValueError("tensor of %d elements for %d blocks of %d" % (t.numel(), self.num_encodings, self.BL))
        out = qdq_per_channel_table(t, self._table_on(t.device), 1, self.num_encodings, self.BL, round_mode)
        return out.to(dtype)

    def quantize_dequantize(self, tensor, round_mode):
        if not self.enabled or self.bitwidth == 32:
            return tensor
        round_mode = _round_mode(round_mode)
        if torch.is_grad_enabled() and tensor.requires_grad:
            return _BlockQdq.apply(tensor, self, round_mode)
        return self._qdq_values(tensor, round_mode)

    def quantize(self, tensor, round_mode):
        raise NotImplementedError("quantize-only output of a blockwise quantizer")

    def ste_backward(self, x, grad):
        """grad * (min_b <= x <= max_b) with the raw min / max of the table."""
        table = self._table_on(x.device)
        view = (1, self.num_encodings, self.BL)
        g = compute_dloss_by_dx(x.detach().contiguous().view(view), grad.contiguous().view(view), table[0], table[1], 1)
        return g.view(grad.shape)

    # -- export / import -----------------------------------------------------------------------------
    def export_encodings(self):
        """The E encodings in [channel][block] order, one entry each in the per-entry format plus
        block_size. LPBQ entries carry, under GroupedBlockQuantizeDequantize._export_1_0_0_encodings'
        names, per_block_int_scale and compressed_bw; their scale is the output channel's scale (the
        block's delta is per_block_int_scale * scale) and their bitwidth the decompressed one."""
        if not self.enabled or self.table is None:
            return None
        mins, maxs, deltas, offsets = self.table.detach().to("cpu", torch.float64).tolist()
        sym = str(bool(self.use_symmetric_encodings))
        out = [{"min": mn, "max": mx, "scale": d, "offset": int(o), "bitwidth": self.bitwidth, "is_symmetric": sym,
                "dtype": "int", "block_size": self.block_size} for mn, mx, d, o in zip(mins, maxs, deltas, offsets)]
        if self.decompressed_bw is not None:
            q = self.int_scale.cpu().tolist()
            factor = self.channel_scale.cpu().tolist()
            for i, e in enumerate(out):
                e.update(scale=factor[i // self.NB], per_block_int_scale=q[i], compressed_bw=self.bitwidth,
                         bitwidth=self.decompressed_bw)
        return out

    def import_encodings(self, entries, device=None):
        """The table (and the LPBQ arrays) from export_encodings()' entries, without a calibration pass."""
        if self._is_encoding_frozen:
            raise RuntimeError("Encoding can be set only when it is not frozen.")
        if len(entries) != self.num_encodings:
            raise AssertionError("Number of blockwise encodings provided (%d) is not the number of blocks (%d)"
                                 % (len(entries), self.num_encodings))
        if any(e.get("block_size") != self.block_size for e in entries):
            raise ValueError("the encodings' block_size does not match the quantizer's %d" % self.block_size)
        lpbq = "per_block_int_scale" in entries[0]
        if lpbq != (self.decompressed_bw is not None):
            raise ValueError("LPBQ encodings need a grouped blockwise quantizer, plain ones a plain one")
        deltas = [e["per_block_int_scale"] * e["scale"] if lpbq else e["scale"] for e in entries]
        cols = [[e["min"] for e in entries], [e["max"] for e in entries], deltas, [e["offset"] for e in entries]]
        self.table = torch.tensor(cols, dtype=torch.float64).to(torch.float32).to(device or "cpu")
        if lpbq:
            self.bitwidth, self.decompressed_bw = entries[0]["compressed_bw"], entries[0]["bitwidth"]
            self.int_scale = torch.tensor([e["per_block_int_scale"] for e in entries], dtype=torch.int32)
            self.channel_scale = torch.tensor([entries[r * self.NB]["scale"] for r in range(self.R)],
                                              dtype=torch.float64)
        else:
            self.bitwidth = entries[0]["bitwidth"]
        self.use_symmetric_encodings = entries[0]["is_symmetric"] == "True"
        self._pending = self._fused = None


class LearnedBlockwiseQuantizer(LearnedGridTensorQuantizer):
    """Range-learning parameter quantizer with one trainable (min, max) per block: the wrapper's
    ``weight_encoding_min`` / ``weight_encoding_max`` are 1-D [E] Parameters in [channel][block]
    order, the order of BlockwiseQuantizer.table's columns."""

    def __init__(self, static: BlockwiseQuantizer):
        super().__init__(static.bitwidth, static.round_mode, static.quant_scheme, static.use_symmetric_encodings,
                         static.enabled, static.data_type)
        self.R, self.NB, self.BL, self.block_size = static.R, static.NB, static.BL, static.block_size
        self.shape = static.shape
        self.use_strict_symmetric = static.use_strict_symmetric
        self.use_unsigned_symmetric = static.use_unsigned_symmetric
        self.is_const = static.is_const
        self.encoding_min_max_fixed_vals = static.encoding_min_max_fixed_vals

    @property
    def num_encodings(self) -> int:
        return self.R * self.NB

    def ranges_from_table(self, static: BlockwiseQuantizer, device):
        """The range Parameters from the static quantizer's device table, on the device, by
        initialize_learned_grid_quantizer_attributes' rule: max = table[1]; min = -max for a symmetric
        range (the learned grid is then signed), table[0] otherwise."""
        table = static.table.detach().to(device, torch.float32)
        emax = table[1].clone()
        emin = -emax if static.use_symmetric_encodings else table[0].clone()
        params = self.wrapper_ref._parameters
        params[self.name + "_encoding_min"] = nn.Parameter(emin, requires_grad=True)
        params[self.name + "_encoding_max"] = nn.Parameter(emax, requires_grad=True)

    def quantize_dequantize(self, tensor, encoding_min, encoding_max, out_dtype=None):
        if not self.enabled or self.bitwidth == 32:
            return tensor
        if encoding_min is None or encoding_max is None:
            raise RuntimeError("Forward pass used for compute_encodings differs from forward pass used during "
                               "training")
        return quantize_dequantize_blocks(tensor, encoding_min, encoding_max, self.BL, self.bitwidth,
                                          self.use_symmetric_encodings, self.use_strict_symmetric,
                                          self.is_unsigned_symmetric, out_dtype)

    def export_encodings(self):
        """BlockwiseQuantizer.export_encodings' entries from the learned ranges (the effective
        encoding: a non-strict symmetric range carries its extra bin below), one device-to-host copy."""
        tensors = self.encoding_tensors() if self.enabled else None
        if tensors is None:
            return None
        emin, emax, scale, offset = tensors
        if self.use_symmetric_encodings and not self.use_strict_symmetric and not self.is_unsigned_symmetric:
            emin = emin - scale
        mins, maxs, deltas, offsets = torch.stack([emin, emax, scale, offset]).to("cpu", torch.float64).tolist()
        sym = str(bool(self.use_symmetric_encodings))
        return [{"min": mn, "max": mx, "scale": d, "offset": int(o), "bitwidth": self.bitwidth, "is_symmetric": sym,
                 "dtype": "int", "block_size": self.block_size} for mn, mx, d, o in zip(mins, maxs, deltas, offsets)]


_CONTIGUOUS_BLOCK_TYPES = (nn.Linear, nn.Conv1d, nn.Conv2d, nn.Conv3d)


def weight_block_view(module: nn.Module, block_size: int) -> Tuple[int, int, int]:
    """(R, NB, BL) of `module`'s weight with the block along its input features and the channel along
    its output features; ValueError for a layer blockwise quantization does not cover."""
    if isinstance(module, (nn.ConvTranspose1d, nn.ConvTranspose2d, nn.ConvTranspose3d)):
        return block_view(module.weight.shape, block_size, channel_axis=1, block_axis=0)   # raises: strided
    if not isinstance(module, _CONTIGUOUS_BLOCK_TYPES):
        raise ValueError("blockwise quantization covers Linear and Conv weights, not %s" % type(module).__name__)
    if getattr(module, "groups", 1) != 1:
        raise ValueError("grouped and depthwise convolutions (groups=%d) are not quantized blockwise" % module.groups)
    return block_view(module.weight.shape, block_size)


def _configure(sim, module_types, bitwidth, symmetric, block_size, decompressed_bw, strict, learn_ranges=False):
    from aimet_amd.quantsim import _RANGE_LEARNING
    if learn_ranges and decompressed_bw is not None:
        raise NotImplementedError("learned LPBQ scales (grouped blockwise quantization with learn_ranges) are not "
                                  "implemented")
    if learn_ranges and sim._quant_scheme not in _RANGE_LEARNING:
        raise ValueError("learn_ranges=True needs a sim with a range-learning quant scheme")
    if sim._quant_scheme in _RANGE_LEARNING and not learn_ranges:
        raise NotImplementedError("blockwise quantization on a range-learning sim needs learn_ranges=True (learned "
                                  "blockwise ranges); learned LPBQ scales are not implemented")
    if decompressed_bw is not None and decompressed_bw <= bitwidth:
        raise ValueError("decompressed_bw %d must exceed bitwidth %d" % (decompressed_bw, bitwidth))
    if isinstance(module_types, type):
        module_types = (module_types,)
    converted = []
    for name, w in sim.quant_wrappers():
        module = w._module_to_wrap
        old = w.param_quantizers.get("weight")
        if not isinstance(module, tuple(module_types)) or old is None:
            continue
        try:
            weight_block_view(module, block_size)
        except ValueError as e:
            if strict:
                raise ValueError("%s: %s" % (name, e)) from e
            continue
        q = BlockwiseQuantizer(module.weight.shape, bitwidth, old.round_mode, old.quant_scheme, symmetric, block_size,
                               decompressed_bw=decompressed_bw, enabled_by_default=old.enabled)
        q.use_strict_symmetric, q.use_unsigned_symmetric = old.use_strict_symmetric, old.use_unsigned_symmetric
        q.learn_ranges = learn_ranges
        w.param_quantizers["weight"] = q
        converted.append(name)
    return converted


def set_blockwise_quantization_for_weights(sim, module_types: Union[type, Tuple[type, ...]], bitwidth: int,
                                           symmetric: bool, block_size: int, strict: bool = False,
                                           learn_ranges: bool = False):
    """aimet_onnx/quantsim.py:1136-1183 with torch module types: the weight quantizers of the given
    module types become blockwise, `block_size` input features a block, one row of blocks per output
    feature. A layer whose input features block_size does not divide, whose blocks would be strided
    (transposed convolutions) or whose weight is grouped is left as it is, or raises ValueError when
    `strict`. Returns the names of the converted wrappers.

    `learn_ranges` (a range-learning sim only, ValueError otherwise): the blocks are calibrated as
    above by compute_encodings, and each block's (min, max) then becomes a pair of trainable
    parameters of the wrapper (LearnedBlockwiseQuantizer)."""
    return _configure(sim, module_types, bitwidth, symmetric, block_size, None, strict, learn_ranges)


def set_grouped_blockwise_quantization_for_weights(sim, module_types: Union[type, Tuple[type, ...]], bitwidth: int,
                                                   decompressed_bw: int, block_size: int, strict: bool = False,
                                                   learn_ranges: bool = False):
    """aimet_onnx/quantsim.py:1186-1240 with torch module types: LPBQ, symmetric, the block scales
    compressed to integers of decompressed_bw - bitwidth bits times one scale per output feature.
    `learn_ranges=True` raises NotImplementedError: learned LPBQ scales are not implemented."""
    return _configure(sim, module_types, bitwidth, True, block_size, decompressed_bw, strict, learn_ranges)
