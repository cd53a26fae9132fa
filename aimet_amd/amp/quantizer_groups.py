"""Quantizer groups of a sim (aimet_torch/amp/quantizer_groups.py): the sets of quantizers that must
share one bitwidth because they sit on the same tensor or in the same kernel.

The reference walks its connected graph; here the graph is a torch.fx trace of ``sim.model`` with the
quantization wrappers as leaves. Wrapper (and other leaf module) calls, ``call_function`` and
``call_method`` nodes are the ops. The rules are the reference's:

* one group per model-input op: its enabled input quantizers and its parameters;
* one group per parent op: its enabled output quantizers plus the enabled input and parameter
  quantizers of all its children;
* one group per enabled output quantizer of a model-output op.

Ops that only move data (view, reshape, flatten, permute, transpose, split, chunk, getitem and
slicing, expand, pad, max-pool, upsample, pixel- and channel-shuffle, top-k) are looked through:
their children attach to the nearest parent that is not such an op. ``size`` / ``shape`` are not
traversed. A functional op such as ``operator.add`` is an op without quantizers, so the group after
it holds its children's quantizers only. Empty groups are dropped.
"""
import itertools
import operator
from collections import defaultdict
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from aimet_amd._dfq import TracedGraph
from aimet_amd.qc_quantize_op import QcQuantizeWrapper

_INPUT_TAG = "_input_quantizer_idx_"


@dataclass(frozen=True)
class QuantizerGroup:
    """Names of the wrappers whose input (``{name}_input_quantizer_idx_{i}``), output and parameter
    quantizers form one group."""
    input_quantizers: Tuple[str, ...] = field(default_factory=tuple)
    output_quantizers: Tuple[str, ...] = field(default_factory=tuple)
    parameter_quantizers: Tuple[str, ...] = field(default_factory=tuple)
    supported_kernel_ops: Tuple[str, ...] = field(default_factory=tuple)

    def get_candidate(self, name_to_quantizer_dict: Dict):
        """((activation bitwidth, data type), (parameter bitwidth, data type)) of the group's first
        activation quantizer and first enabled parameter quantizer; (None, None) where there is none."""
        activation, parameter = (None, None), (None, None)
        for quantizer in self._get_input_quantizers(name_to_quantizer_dict) + \
                self._get_output_quantizers(name_to_quantizer_dict):
            activation = (quantizer.bitwidth, quantizer.data_type)
            break
        for quantizer in self._get_param_quantizers(name_to_quantizer_dict):
            if quantizer.enabled:
                parameter = (quantizer.bitwidth, quantizer.data_type)
                break
        return activation, parameter

    def set_quantizers_to_candidate(self, name_to_quantizer_dict: Dict, candidate) -> None:
        """bitwidth and data_type of every quantizer of the group; encodings are not recomputed."""
        if len(candidate) == 1:
            (activation_bw, activation_data_type), = candidate
            param_bw, param_data_type = None, None
        else:
            (activation_bw, activation_data_type), (param_bw, param_data_type) = candidate
        for quantizer in self._get_input_quantizers(name_to_quantizer_dict) + \
                self._get_output_quantizers(name_to_quantizer_dict):
            quantizer.bitwidth = activation_bw
            quantizer.data_type = activation_data_type
        if param_bw is not None:
            for quantizer in self._get_param_quantizers(name_to_quantizer_dict):
                quantizer.bitwidth = param_bw
                quantizer.data_type = param_data_type

    def to_list(self) -> List[Tuple[str, str]]:
        """[("input" | "output" | "weight", name), ...]"""
        return list(itertools.chain((("input", name) for name in self.input_quantizers),
                                    (("output", name) for name in self.output_quantizers),
                                    (("weight", name) for name in self.parameter_quantizers)))

    def get_active_quantizers(self, name_to_quantizer_dict: Dict) -> List:
        quantizers = self._get_input_quantizers(name_to_quantizer_dict) + \
            self._get_output_quantizers(name_to_quantizer_dict) + self._get_param_quantizers(name_to_quantizer_dict)
        return [quantizer for quantizer in quantizers if quantizer.enabled]

    def get_input_quantizer_modules(self) -> Tuple[str, ...]:
        """Names of the modules the group's input quantizers belong to, sorted."""
        return tuple(sorted({self._split_input_name(name)[0] for name in self.input_quantizers}))

    @staticmethod
    def _split_input_name(quantizer_name: str) -> Tuple[str, int]:
        parts = quantizer_name.split(_INPUT_TAG)
        assert len(parts) == 2
        return parts[0], int(parts[1])

    def _get_input_quantizers(self, name_to_quantizer_dict):
        out = []
        for quantizer_name in self.input_quantizers:
            module_name, index = self._split_input_name(quantizer_name)
            out.append(name_to_quantizer_dict[module_name].input_quantizers[index])
        return out

    def _get_output_quantizers(self, name_to_quantizer_dict):
        out = []
        for module_name in self.output_quantizers:
            out += name_to_quantizer_dict[module_name].output_quantizers
        return out

    def _get_param_quantizers(self, name_to_quantizer_dict):
        out = []
        for module_name in self.parameter_quantizers:
            out += list(name_to_quantizer_dict[module_name].param_quantizers.values())
        return out


def get_module_name_to_module_dict(sim) -> Dict[str, QcQuantizeWrapper]:
    """{wrapped module's name: its quantization wrapper}"""
    return {name: module for name, module in sim.model.named_modules() if isinstance(module, QcQuantizeWrapper)}


# ---------------------------------------------------------------------------------------------------
# the reference's ops_to_skip / ops_not_to_traverse on fx targets and module types
# ---------------------------------------------------------------------------------------------------
def _existing(namespace, names):
    return {getattr(namespace, n) for n in names if hasattr(namespace, n)}


SKIPPED_FUNCTIONS = {operator.getitem} | _existing(
    torch, ("reshape", "flatten", "permute", "transpose", "t", "split", "chunk", "tile", "topk", "gather",
            "narrow", "select", "pixel_shuffle", "pixel_unshuffle", "channel_shuffle", "max_pool1d", "max_pool2d",
            "max_pool3d", "swapaxes", "movedim")) | _existing(
    F, ("pad", "max_pool1d", "max_pool2d", "max_pool3d", "interpolate", "upsample", "upsample_nearest",
        "upsample_bilinear", "pixel_shuffle", "pixel_unshuffle", "channel_shuffle"))
SKIPPED_METHODS = {"view", "view_as", "reshape", "reshape_as", "flatten", "permute", "transpose", "t", "split",
                   "chunk", "tile", "expand", "expand_as", "topk", "gather", "narrow", "select", "swapaxes", "movedim"}
SKIPPED_MODULES = tuple(_existing(nn, (
    "Flatten", "Unflatten", "MaxPool1d", "MaxPool2d", "MaxPool3d", "Upsample", "UpsamplingNearest2d",
    "UpsamplingBilinear2d", "PixelShuffle", "PixelUnshuffle", "ChannelShuffle", "ZeroPad1d", "ZeroPad2d", "ZeroPad3d",
    "ConstantPad1d", "ConstantPad2d", "ConstantPad3d", "ReflectionPad1d", "ReflectionPad2d", "ReflectionPad3d",
    "ReplicationPad1d", "ReplicationPad2d", "ReplicationPad3d", "CircularPad1d", "CircularPad2d", "CircularPad3d")))
NOT_TRAVERSED_METHODS = {"size"}
_OP_KINDS = ("call_module", "call_function", "call_method")


class _Ops:
    """The ops of a traced sim and what the rules ask of them."""

    def __init__(self, sim):
        from aimet_amd.qc_quantize_recurrent import QcQuantizeRecurrent
        try:
            self.graph = TracedGraph(sim.model, is_leaf=lambda m: isinstance(m, (QcQuantizeWrapper, QcQuantizeRecurrent)))
        except RuntimeError as e:
            cause = e.__cause__ if e.__cause__ is not None else e
            raise RuntimeError("aimet_amd: automatic mixed precision (AMP) finds its quantizer groups on a torch.fx "
                               "trace of the sim's model, and torch.fx cannot trace %s (%s: %s)"
                               % (type(sim.model).__name__, type(cause).__name__, cause)) from e
        self.ops = [n for n in self.graph.nodes if n.op in _OP_KINDS]

    def name(self, node) -> str:
        return node.target if node.op == "call_module" else node.name

    def skipped(self, node) -> bool:
        if node.op == "call_function":
            return node.target in SKIPPED_FUNCTIONS
        if node.op == "call_method":
            return node.target in SKIPPED_METHODS
        module = self.graph.module(node)
        if isinstance(module, QcQuantizeWrapper):
            module = module._module_to_wrap
        return isinstance(module, SKIPPED_MODULES)

    @staticmethod
    def not_traversed(node) -> bool:
        if node.op == "call_method":
            return node.target in NOT_TRAVERSED_METHODS
        return node.op == "call_function" and node.target is getattr and len(node.args) > 1 and node.args[1] == "shape"

    def is_input(self, node) -> bool:
        return not any(n.op in _OP_KINDS for n in node.all_input_nodes)

    @staticmethod
    def consumers(node):
        return [u for u in node.users if u.op in _OP_KINDS]

    @staticmethod
    def is_output(node) -> bool:
        return not [u for u in node.users if u.op in _OP_KINDS]


def find_op_groups(ops: "_Ops") -> Dict:
    """{parent op: [child ops]}, plus 'input_ops' and 'output_ops': an op is the parent of the ops
    that consume its output; ops that share an input share its producer as their parent."""
    groups = defaultdict(list)
    nearest_kept_parent = {}

    def attach_consumers(op):
        consumers = ops.consumers(op)
        if not consumers:
            if op in nearest_kept_parent:          # a looked-through op that ends the model
                groups[nearest_kept_parent[op]] = []
            return
        for consumer in consumers:
            if ops.not_traversed(consumer):
                continue
            parent = nearest_kept_parent.get(op, op)
            if ops.skipped(consumer):
                nearest_kept_parent[consumer] = parent
                attach_consumers(consumer)
            else:
                groups[parent].append(consumer)

    for op in ops.ops:
        if ops.is_input(op):
            groups["input_ops"].append(op)
        if ops.is_output(op):
            groups["output_ops"].append(op)
    for op in ops.ops:
        if not ops.skipped(op) and not ops.not_traversed(op):
            attach_consumers(op)
    return groups


def _input_and_param_quantizers(name: str, wrappers: Dict) -> Tuple[Tuple[str, ...], Tuple[str, ...]]:
    """The enabled input quantizers of wrapper `name`, and its name once per enabled parameter quantizer."""
    wrapper = wrappers.get(name)
    if wrapper is None:
        return (), ()
    inputs = tuple(name + _INPUT_TAG + str(i) for i, q in enumerate(wrapper.input_quantizers) if q.enabled)
    params = tuple(name for q in wrapper.param_quantizers.values() if q.enabled)
    return inputs, params


def find_quantizer_group(sim) -> Tuple[Dict[str, QcQuantizeWrapper], List[QuantizerGroup]]:
    """({wrapped module name: wrapper}, the sim's quantizer groups in graph order)."""
    ops = _Ops(sim)
    op_groups = find_op_groups(ops)
    wrappers = get_module_name_to_module_dict(sim)
    quantizer_groups = []

    for child in op_groups.get("input_ops", ()):
        name = ops.name(child)
        input_quantizers, parameter_quantizers = _input_and_param_quantizers(name, wrappers)
        if input_quantizers or parameter_quantizers:
            quantizer_groups.append(QuantizerGroup(input_quantizers=input_quantizers,
                                                   parameter_quantizers=parameter_quantizers,
                                                   supported_kernel_ops=(name,) if name in wrappers else ()))

    for parent, children in op_groups.items():
        if parent in ("input_ops", "output_ops"):
            continue
        input_quantizers, output_quantizers, parameter_quantizers, kernel_ops = (), (), (), []
        wrapper = wrappers.get(ops.name(parent))
        if wrapper is not None:
            output_quantizers += tuple(ops.name(parent) for q in wrapper.output_quantizers if q.enabled)
        for child in children:
            name = ops.name(child)
            child_inputs, child_params = _input_and_param_quantizers(name, wrappers)
            input_quantizers += child_inputs
            parameter_quantizers += child_params
            if name in wrappers:
                kernel_ops.append(name)
        if input_quantizers or output_quantizers or parameter_quantizers:
            quantizer_groups.append(QuantizerGroup(input_quantizers, output_quantizers, parameter_quantizers,
                                                   tuple(kernel_ops)))

    for parent in op_groups.get("output_ops", ()):
        name = ops.name(parent)
        wrapper = wrappers.get(name)
        if wrapper is not None:
            for quantizer in wrapper.output_quantizers:
                if quantizer.enabled:
                    quantizer_groups.append(QuantizerGroup(output_quantizers=(name,)))
    return wrappers, quantizer_groups


def find_supported_candidates(quantizer_groups: List[QuantizerGroup], amp_candidates: List,
                              use_all_amp_candidates: bool = False) -> Tuple[Dict, List]:
    """({group: its candidates}, the candidates the baseline is chosen from). The sim carries no
    `supported_kernels` configuration, so every candidate counts as supported for every group,
    whatever use_all_amp_candidates says."""
    del use_all_amp_candidates
    supported = defaultdict(list)
    for quantizer_group in quantizer_groups:
        supported[quantizer_group] = amp_candidates
    return supported, amp_candidates
