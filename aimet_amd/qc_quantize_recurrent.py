"""QcQuantizeRecurrent: quantization simulation of nn.RNN / nn.LSTM / nn.GRU on the fused step kernel.

Mirrors aimet_torch/v1/qc_quantize_recurrent.py (QcQuantizeRecurrent :122-976 and the packed-sequence
helpers :978-1189): the same quantizer sets (`input_quantizers`, `output_quantizers`,
`param_quantizers`, `grouped_quantizers`), grouping table and default enabled states, the same
methods, and the same per-step semantics -- but the sequence is not walked tensor by tensor. Per layer:

  * the input quantizer (QDQ or statistics) on the layer's whole input;
  * one GEMM X W_ih^T for all time steps and both directions;
  * per time step one recurrent GEMM through torch (a `bmm` over the directions) and ONE
    aimet_rnn_step launch (csrc/rnn_cell.hip) that adds the biases, applies the gates, updates the
    state, keeps the rows of ended sequences, quantize-dequantizes h and c and writes h into the
    layer's [T, B, D H] output slab. The reverse direction and packed sequences are indexing
    arguments of that launch: no flip, shift, stack or concat.

ANALYSIS mode keeps every step's state and then feeds each state quantizer exactly the tensors of the
reference's procedure in its order (direction by direction, step by step, the given initial state
last), through the quantizer's own update or the calibration's StatsBatch.

Kept from the reference on purpose: both directions of layer l start from hx[l] (not hx[l * D + d]).
Differs from it: the output slab is zero where a sequence has ended (the reference leaves stale or
random rows there, which packing drops).

Refused (NotImplementedError / RuntimeError): LEARN_ENCODINGS and range learning, autograd through
the step (the forward runs without gradient), proj_size > 0, float data types, per-channel quantizers,
stochastic rounding, and the ONNX tensor-name mapping of the export.
"""
import ctypes
from collections import defaultdict
from typing import Dict, Optional, Tuple, Union

import torch
from torch import nn
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

from aimet_amd import _native
from aimet_amd.encodings_io import create_encoding_from_dict, export_quantizer_encoding
from aimet_amd.libpymo import RoundingMode
from aimet_amd.qc_quantize_op import QcQuantizeOpMode
from aimet_amd.quantizers import (MAP_ROUND_MODE_TO_PYMO, QuantizationDataType, QuantScheme,
                                  StaticGridPerTensorQuantizer)

# v1/qc_quantize_recurrent.py:62-68: the tensors that share one quantizer
grouped_quantizer_map = {
    "hidden_l{}": ["initial_h_l{}", "h_l{}"],
    "cell_l{}": ["initial_c_l{}", "c_l{}"],
    "bias_l{}": ["bias_ih_l{}", "bias_hh_l{}", "bias_ih_l{}_reverse", "bias_hh_l{}_reverse"],
    "W_l{}": ["weight_ih_l{}", "weight_ih_l{}_reverse"],
    "R_l{}": ["weight_hh_l{}", "weight_hh_l{}_reverse"],
}
# v1/qc_quantize_recurrent.py:311-317
_DEFAULT_GROUP_STATE = {"hidden_l{}": True, "cell_l{}": False, "bias_l{}": False, "W_l{}": True, "R_l{}": True}

_MODES = {"LSTM": 0, "GRU": 1, "RNN_TANH": 2, "RNN_RELU": 3}   # aimet_rnn_mode
_GATES = {"LSTM": 4, "GRU": 3, "RNN_TANH": 1, "RNN_RELU": 1}
_RANGE_LEARNING = (QuantScheme.training_range_learning_with_tf_init,
                   QuantScheme.training_range_learning_with_tf_enhanced_init)


def _encoding_c(q) -> Optional[_native.TfEncodingC]:
    e = q.encoding
    if e is None:
        raise RuntimeError("QcQuantizeRecurrent: an enabled state quantizer has no encoding in ACTIVE mode; run "
                           "compute_encodings first")
    return _native.TfEncodingC(e.min, e.max, e.delta, e.offset, e.bw)


class QcQuantizeRecurrent(nn.Module):
    """v1/qc_quantize_recurrent.py:122."""

    def __init__(self, module_to_quantize: Union[nn.RNN, nn.LSTM, nn.GRU], weight_bw: int, activation_bw: int,
                 round_mode: str, quant_scheme: QuantScheme, is_symmetric: bool = False, num_inputs=1, num_outputs=1,
                 data_type: QuantizationDataType = QuantizationDataType.int):
        super().__init__()
        if not isinstance(module_to_quantize, (nn.RNN, nn.LSTM, nn.GRU)):
            raise TypeError("QcQuantizeRecurrent wraps nn.RNN, nn.LSTM or nn.GRU, not %s" % type(module_to_quantize))
        if getattr(module_to_quantize, "proj_size", 0):
            raise NotImplementedError("QcQuantizeRecurrent: proj_size > 0 is not supported")
        if data_type != QuantizationDataType.int:
            raise NotImplementedError("QcQuantizeRecurrent: float data types are not supported (integer QDQ only)")
        if quant_scheme in _RANGE_LEARNING:
            raise NotImplementedError("QcQuantizeRecurrent: range learning (LEARN_ENCODINGS) is not supported")
        self._round_mode = MAP_ROUND_MODE_TO_PYMO[round_mode] if isinstance(round_mode, str) else RoundingMode(round_mode)
        if self._round_mode != RoundingMode.ROUND_NEAREST:
            raise NotImplementedError("QcQuantizeRecurrent: stochastic rounding is not supported")
        self._mode = QcQuantizeOpMode.ANALYSIS
        self._clone_module_params(module_to_quantize)
        self.module_to_quantize = module_to_quantize
        self._weight_bw, self._activation_bw = weight_bw, activation_bw
        self._is_symmetric, self._data_type, self._quant_scheme = is_symmetric, data_type, quant_scheme
        self._grouped_quantizers = {}
        self._param_quantizers = {}
        lstm = isinstance(module_to_quantize, nn.LSTM)
        self._output_quantizers = self._create_activation_quantizers(["h_l{}", "c_l{}"] if lstm else ["h_l{}"])
        self._input_quantizers = self._create_activation_quantizers(
            ["input_l{}", "initial_h_l{}", "initial_c_l{}"] if lstm else ["input_l{}", "initial_h_l{}"])
        self._create_param_quantizers()
        self._set_default_eai_quantizer_state()
        # the initial state's statistics come after the time steps' (v1/qc_quantize_recurrent.py:173-188)
        self._reorder_initial_h_c_stats_update = True
        # for the tests: an ANALYSIS forward keeps, per layer, (h of every step [T, D, B, H], c likewise,
        # the given initial h [D, B, H], the given initial c) in last_analysis_states
        self.keep_analysis_states = False
        self.last_analysis_states = {}

    # -- construction -------------------------------------------------------------------------------
    def _new_quantizer(self, bw):
        return StaticGridPerTensorQuantizer(bw, self._round_mode, self._quant_scheme, self._is_symmetric,
                                            enabled_by_default=False, data_type=self._data_type)

    @staticmethod
    def _get_group_name(tensor_name: str, layer: int) -> Optional[str]:
        for group, tensors in grouped_quantizer_map.items():
            if tensor_name in [t.format(layer) for t in tensors]:
                return group.format(layer)
        return None

    def _create_activation_quantizers(self, tensor_names) -> Dict[str, StaticGridPerTensorQuantizer]:
        quantizers = {}
        for layer in range(self.num_layers):
            for name in tensor_names:
                name = name.format(layer)
                group = self._get_group_name(name, layer)
                if group:
                    if group not in self._grouped_quantizers:
                        self._grouped_quantizers[group] = self._new_quantizer(self._activation_bw)
                    quantizers[name] = self._grouped_quantizers[group]
                else:
                    quantizers[name] = self._new_quantizer(self._activation_bw)
        return quantizers

    def _create_param_quantizers(self):
        by_tensor = {}
        for layer in range(self.num_layers):
            for group, tensors in grouped_quantizer_map.items():
                group = group.format(layer)
                if group not in self._grouped_quantizers:
                    self._grouped_quantizers[group] = self._new_quantizer(self._weight_bw)
                for t in tensors:
                    by_tensor[t.format(layer)] = self._grouped_quantizers[group]
        for name, _ in self.module_to_quantize.named_parameters():
            self._param_quantizers[name] = by_tensor[name] if name in by_tensor else self._new_quantizer(self._weight_bw)

    def _set_default_eai_quantizer_state(self):
        """v1/qc_quantize_recurrent.py:306-343."""
        grouped_tensors = {t.format(layer) for layer in range(self.num_layers)
                           for tensors in grouped_quantizer_map.values() for t in tensors}
        for layer in range(self.num_layers):
            for group, state in _DEFAULT_GROUP_STATE.items():
                self._grouped_quantizers[group.format(layer)].enabled = state
        for name, q in self._output_quantizers.items():
            if name not in grouped_tensors:
                q.enabled = False
        for quantizers in (self._param_quantizers, self._input_quantizers):
            for name, q in quantizers.items():
                if name not in grouped_tensors:
                    q.enabled = True

    def _clone_module_params(self, module):
        self.hidden_size = module.hidden_size
        self.num_layers = module.num_layers
        self.batch_first = module.batch_first
        self.num_directions = 2 if module.bidirectional else 1
        self.mode = module.mode
        self.bias = module.bias
        for layer in range(module.num_layers):
            for direction in range(self.num_directions):
                for name in self._get_param_names(direction, layer):
                    setattr(self, name, nn.Parameter(getattr(module, name).data.clone()))

    def _get_param_names(self, direction: int, layer: int):
        suffix = "_reverse" if direction == 1 else ""
        names = ["weight_ih_l{}{}", "weight_hh_l{}{}"] + (["bias_ih_l{}{}", "bias_hh_l{}{}"] if self.bias else [])
        return [n.format(layer, suffix) for n in names]

    # -- the reference's surface --------------------------------------------------------------------
    @property
    def device(self):
        return self.weight_ih_l0.device

    @property
    def grouped_quantizers(self):
        return self._grouped_quantizers

    @property
    def param_quantizers(self):
        return self._param_quantizers

    @property
    def output_quantizers(self):
        return self._output_quantizers

    @property
    def input_quantizers(self):
        return self._input_quantizers

    def _all_quantizers(self):
        seen = {}
        for d in (self._grouped_quantizers, self._param_quantizers, self._input_quantizers, self._output_quantizers):
            for q in d.values():
                seen[id(q)] = q
        return list(seen.values())

    def set_output_bw(self, output_bw: int):
        for q in self._output_quantizers.values():
            q.bitwidth = output_bw

    def set_mode(self, mode: QcQuantizeOpMode):
        if mode == QcQuantizeOpMode.LEARN_ENCODINGS:
            raise NotImplementedError("QcQuantizeRecurrent: LEARN_ENCODINGS (range learning) is not supported")
        self._mode = mode

    def enable_param_quantizers(self, enabled: bool, param_name_to_exclude=("bias",)):
        for name, q in self._param_quantizers.items():
            if name not in (param_name_to_exclude or ()):
                q.enabled = enabled

    def enable_input_quantizers(self, enabled: bool):
        for q in self._input_quantizers.values():
            q.enabled = enabled

    def enable_output_quantizers(self, enabled: bool):
        for q in self._output_quantizers.values():
            q.enabled = enabled

    def enable_act_quantizers(self, enabled: bool):
        self.enable_input_quantizers(enabled)
        self.enable_output_quantizers(enabled)

    def enable_per_channel_quantization(self):
        raise NotImplementedError("QcQuantizeRecurrent: per-channel quantizers are not supported")

    def construct_and_initialize_trainable_quantizers(self, quant_scheme):
        raise NotImplementedError("QcQuantizeRecurrent: LEARN_ENCODINGS (range learning) is not supported")

    def get_activation_param_quantizers_for_onnx_tensors(self, io_tensor_map):
        raise NotImplementedError("QcQuantizeRecurrent: the ONNX tensor-name mapping of the export is not supported")

    def set_percentile_value(self, percentile_value: float):
        for q in self._all_quantizers():
            q.set_percentile_value(percentile_value)

    def reset_encodings(self):
        for q in self._all_quantizers():
            q.reset_encoding_stats()

    def compute_encoding(self):
        for q in self._all_quantizers():   # a grouped quantizer once, whatever number of tensors share it
            q.compute_encoding()

    def compute_weight_encodings(self):
        encodings = {}
        for name, q in self._param_quantizers.items():
            if "weight" in name:
                q.compute_encoding()
                encodings[name] = q.encoding
        return encodings

    def get_named_parameters(self):
        for name, _ in self.module_to_quantize.named_parameters():
            yield name, getattr(self, name)

    def update_params(self):
        for layer in range(self.num_layers):
            for direction in range(self.num_directions):
                for name in self._get_param_names(direction, layer):
                    getattr(self.module_to_quantize, name).data = getattr(self, name).data

    def get_original_module(self):
        """The wrapped module carrying this wrapper's parameters."""
        self.update_params()
        return self.module_to_quantize

    def flatten_parameters(self):
        """A no-op, for models that call it on their recurrent module."""

    # -- encodings export / import ------------------------------------------------------------------
    def export_param_encodings(self):
        return {name: export_quantizer_encoding(q) for name, q in self._param_quantizers.items()}

    def export_input_encodings(self):
        return {name: export_quantizer_encoding(q) for name, q in self._input_quantizers.items()}

    def export_output_encodings(self):
        return {name: export_quantizer_encoding(q) for name, q in self._output_quantizers.items()}

    def import_encodings(self, param_encodings: Dict, activation_encodings: Dict, strict: bool = True,
                         partial: bool = True):
        """Encodings as the export_* methods give them, keyed by parameter / tensor name, under the
        rules of the wrappers' import (qc_quantize_op.py import_param_encodings / _import_encoding): an
        enabled quantizer without an entry stays as it is (`partial`) or is disabled; an entry for a
        disabled quantizer raises (`strict`) or is skipped; no quantizer is enabled by the file."""
        named = [(n, q, param_encodings.get(n)) for n, q in self._param_quantizers.items()]
        named += [(n, q, [activation_encodings[n]] if n in activation_encodings else None)
                  for d in (self._input_quantizers, self._output_quantizers) for n, q in d.items()]
        for name, q, enc in named:
            if q._is_encoding_frozen:
                continue
            if not enc:
                if not partial:
                    q.enabled = False
                continue
            if not q.enabled:
                if strict:
                    raise RuntimeError("The quantsim passed for loading encodings does not have the same "
                                       "configuration as the quantsim which was used to export the encodings "
                                       "(%s is disabled)" % name)
                continue
            q.encoding = create_encoding_from_dict(enc[0])
            q.bitwidth = q.encoding.bw

    # -- forward ------------------------------------------------------------------------------------
    def _update_stats(self, q, t, owned=True):
        """One statistics update of q with t, through the calibration's batch where there is one.
        owned: nobody writes t again (the kept per-step states and the output slabs)."""
        if not q.enabled:
            return
        batch = self.__dict__.get("_stats_batch")
        if batch is not None and batch.accepts(q, t):
            batch.add(q, t, owned=owned)
        else:
            q.update_encoding_stats(t)

    def _quantize_activation(self, q, t, owned=True):
        """v1/qc_quantize_recurrent.py:690-736 for one tensor."""
        if not q.enabled:
            return t
        if self._mode is QcQuantizeOpMode.ANALYSIS:
            self._update_stats(q, t, owned)
        elif self._mode is QcQuantizeOpMode.ACTIVE and q.bitwidth != 32:
            return q.quantize_dequantize(t, RoundingMode.ROUND_NEAREST)
        return t

    def _quantized_params(self) -> Dict[str, torch.Tensor]:
        """v1/qc_quantize_recurrent.py:416-466: every parameter through its quantizer, once per forward;
        the encodings recomputed when absent or when training. The parameters themselves stay as they are."""
        by_quantizer = defaultdict(list)
        for name, p in self.get_named_parameters():
            by_quantizer[id(self._param_quantizers[name])].append((name, p))
        out = {}
        for items in by_quantizer.values():
            q = self._param_quantizers[items[0][0]]
            if q.enabled and (self.training or q.encoding is None):
                q.reset_encoding_stats()
                for _, p in items:
                    q.update_encoding_stats(p.data)
                q.compute_encoding()
            for name, p in items:
                if q.enabled and q.bitwidth != 32:   # in every mode, as the reference
                    out[name] = q.quantize_dequantize(p.data, RoundingMode.ROUND_NEAREST)
                else:
                    out[name] = p.data
        return out

    def forward(self, inputs: Union[torch.Tensor, PackedSequence], hx=None) -> Tuple:
        if self._mode is QcQuantizeOpMode.LEARN_ENCODINGS:
            raise NotImplementedError("QcQuantizeRecurrent: LEARN_ENCODINGS (range learning) is not supported")
        data = inputs.data if isinstance(inputs, PackedSequence) else inputs
        states = [] if hx is None else (list(hx) if isinstance(hx, tuple) else [hx])
        if torch.is_grad_enabled() and any(t.requires_grad for t in [data] + states):
            raise RuntimeError("QcQuantizeRecurrent: no autograd through the fused recurrent step; call it under "
                               "torch.no_grad() with inputs that do not require a gradient")
        if not data.is_cuda or data.dtype != torch.float32:
            raise RuntimeError("QcQuantizeRecurrent: the input must be a float32 tensor on the GPU (there is no CPU "
                               "path)")
        with torch.no_grad(), torch.cuda.device(data.device):
            return self._forward(inputs, hx)

    def _forward(self, inputs, hx):
        lstm = self.mode == "LSTM"
        lens_cpu = sorted_indices = unsorted_indices = batch_sizes = None
        if isinstance(inputs, PackedSequence):
            batch_sizes, sorted_indices, unsorted_indices = inputs.batch_sizes, inputs.sorted_indices, inputs.unsorted_indices
            x, lens_cpu = pad_packed_sequence(inputs, batch_first=False)   # rows in the caller's order
            if sorted_indices is not None:
                x = x.index_select(1, sorted_indices)
            batch_sizes = [int(b) for b in batch_sizes]
        else:
            x = inputs.transpose(0, 1) if self.batch_first else inputs
        x = x.contiguous()
        T, B, _ = x.shape
        D, H, G = self.num_directions, self.hidden_size, _GATES[self.mode]
        dev = x.device
        lens_dev = None
        if batch_sizes is not None:
            sorted_lens = torch.sort(lens_cpu, descending=True)[0]
            lens_dev = sorted_lens.to(device=dev, dtype=torch.int32)
        if hx is not None:
            h0_all, c0_all = (hx if lstm else (hx, None))
            if lstm and not isinstance(hx, tuple):
                raise RuntimeError("QcQuantizeRecurrent: an LSTM's initial state is a tuple (h_0, c_0)")
            if sorted_indices is not None:
                h0_all = h0_all.index_select(1, sorted_indices)
                c0_all = c0_all.index_select(1, sorted_indices) if lstm else None
        analysis = self._mode is QcQuantizeOpMode.ANALYSIS
        active = self._mode is QcQuantizeOpMode.ACTIVE
        params = self._quantized_params()
        if analysis and self.keep_analysis_states:
            self.last_analysis_states = {}
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        lib = _native.load()
        slots = T if analysis else min(T, 2)
        layer_in = x
        h_n, c_n = [], []
        for layer in range(self.num_layers):
            h_q = self._output_quantizers["h_l%d" % layer]
            c_q = self._output_quantizers["c_l%d" % layer] if lstm else None
            xq = self._quantize_activation(self._input_quantizers["input_l%d" % layer], layer_in, owned=layer > 0)
            names = [self._get_param_names(d, layer) for d in range(D)]
            w_ih = torch.cat([params[n[0]] for n in names]) if D > 1 else params[names[0][0]]
            ig = torch.mm(xq.reshape(T * B, -1), w_ih.t())                              # [T B, D G H]
            w_hh_t = torch.stack([params[n[1]].t() for n in names])                    # [D, H, G H]
            biases = [[params[n[2]].contiguous(), params[n[3]].contiguous()] if self.bias else [None, None]
                      for n in names]
            # the initial state of both directions: hx[layer], as the reference takes it
            h_init = torch.zeros(D, B, H, device=dev)
            c_init = torch.zeros(D, B, H, device=dev) if lstm else None
            if hx is not None:
                h0 = h0_all[layer].to(torch.float32)
                c0 = c0_all[layer].to(torch.float32) if lstm else None
                if not analysis:
                    h0 = self._quantize_activation(self._input_quantizers["initial_h_l%d" % layer], h0)
                    if lstm:
                        c0 = self._quantize_activation(self._input_quantizers["initial_c_l%d" % layer], c0)
                h_init.copy_(h0.expand(D, B, H))
                if lstm:
                    c_init.copy_(c0.expand(D, B, H))
            h_hist = torch.empty(slots, D, B, H, device=dev)
            c_hist = torch.empty(slots, D, B, H, device=dev) if lstm else None
            hg = torch.empty(D, B, G * H, device=dev)
            out = (torch.zeros if batch_sizes is not None else torch.empty)(T, B, D * H, device=dev)
            jobs = (_native.RnnStepJobC * D)()
            for d in range(D):
                j = jobs[d]
                j.ig = ig.data_ptr() + 4 * d * G * H
                j.ig_step_stride, j.ig_row_stride = B * D * G * H, D * G * H
                j.hg, j.hg_row_stride = hg[d].data_ptr(), G * H
                j.b_ih = biases[d][0].data_ptr() if self.bias else None
                j.b_hh = biases[d][1].data_ptr() if self.bias else None
                j.out = out.data_ptr() + 4 * d * H
                j.out_step_stride, j.out_row_stride = B * D * H, D * H
                j.lens = lens_dev.data_ptr() if lens_dev is not None else None
                j.reverse = d
            h_enabled = bool(h_q.enabled and h_q.bitwidth != 32)
            c_enabled = bool(lstm and c_q.enabled and c_q.bitwidth != 32)
            h_enc = _encoding_c(h_q) if active and h_enabled else None
            c_enc = _encoding_c(c_q) if active and c_enabled else None
            h_ref = ctypes.byref(h_enc) if h_enc is not None else None
            c_ref = ctypes.byref(c_enc) if c_enc is not None else None
            step_bytes = 4 * B * H
            h_base = h_hist.data_ptr()
            c_base = c_hist.data_ptr() if lstm else 0
            h_prev, c_prev = h_init, c_init
            for it in range(T):
                slot = it % slots
                h_next = h_hist[slot]
                torch.bmm(h_prev, w_hh_t, out=hg)
                for d in range(D):
                    j = jobs[d]
                    j.h_prev = h_prev.data_ptr() + d * step_bytes
                    j.h_next = h_base + (slot * D + d) * step_bytes
                    if lstm:
                        j.c_prev = c_prev.data_ptr() + d * step_bytes
                        j.c_next = c_base + (slot * D + d) * step_bytes
                valid = batch_sizes[it] if batch_sizes is not None else B
                _native.check(lib.aimet_rnn_step(_MODES[self.mode], jobs, D, B, H, T, it, valid, h_ref, h_enabled,
                                                 c_ref, c_enabled, self._mode.value, stream))
                h_prev = h_next
                if lstm:
                    c_prev = c_hist[slot]
            if analysis:
                # each state quantizer sees what the per-step procedure shows it, in its order
                for d in range(D):
                    for it in range(T):
                        self._update_stats(h_q, h_hist[it, d])
                        if lstm:
                            self._update_stats(c_q, c_hist[it, d])
                    if hx is not None:
                        self._update_stats(self._input_quantizers["initial_h_l%d" % layer], h_init[d])
                        if lstm:
                            self._update_stats(self._input_quantizers["initial_c_l%d" % layer], c_init[d])
                if self.keep_analysis_states:
                    self.last_analysis_states[layer] = (h_hist, c_hist, h_init if hx is not None else None,
                                                        c_init if hx is not None and lstm else None)
            h_n.extend(h_prev[d] for d in range(D))
            if lstm:
                c_n.extend(c_prev[d] for d in range(D))
            layer_in = out
        h_n = torch.stack(h_n)
        c_n = torch.stack(c_n) if lstm else None
        if batch_sizes is not None:
            if unsorted_indices is not None:
                out = out.index_select(1, unsorted_indices)
                h_n = h_n.index_select(1, unsorted_indices)
                c_n = c_n.index_select(1, unsorted_indices) if lstm else None
            out = pack_padded_sequence(out, lens_cpu, batch_first=False, enforce_sorted=sorted_indices is None)
        elif self.batch_first:
            out = out.transpose(0, 1)
        return out, ((h_n, c_n) if lstm else h_n)
