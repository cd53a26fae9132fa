"""Cross-layer equalization (aimet_torch/cross_layer_equalization.py) on the MI355X core: batch-norm
folding, cross-layer scaling (CLS) and high-bias folding (HBF), in place on the model.

Names and semantics follow the reference. Its live path is numpy on the host, every weight of every
set copied device -> host -> device; here one CLS set is one launch of ``aimet_dfq_cls_pair`` /
``aimet_dfq_cls_triple`` and one HBF pair one launch of ``aimet_dfq_bias_fold``
(aimet_amd/csrc/dfq.hip), all in place on the parameters. ``ConvTranspose{1,2}d`` with groups == 1
and ``Conv1d`` are addressed by strides: no permuted copy is made. Scale factors are returned as
numpy arrays.

Layer groups come from a ``torch.fx.symbolic_trace`` of the model: a group is a maximal chain of
supported layers separated only by supported activations in which every intermediate tensor has
exactly one user. At a fan-out (a residual branch) the chain ends at the producer and each consumer
starts a new one. (The reference's recursion shares one mutable group list between the consumers of
a fan-out; that accident is not reproduced, see DESIGN.md.) ``nn.Identity`` modules, which folded
batch norms leave behind, are looked through.
"""
import ctypes
from typing import Dict, List, Tuple, Union

import numpy as np
import torch
from torch import nn

from aimet_amd import _dfq, _native
from aimet_amd.batch_norm_fold import fold_all_batch_norms

ClsSet = Union[Tuple[nn.Conv2d, nn.Conv2d], Tuple[nn.Conv2d, nn.Conv2d, nn.Conv2d]]
ScaleFactor = Union[np.ndarray, Tuple[np.ndarray]]

cls_supported_layers = (nn.Conv2d, nn.ConvTranspose2d, nn.Conv1d, nn.ConvTranspose1d)
cls_supported_activations = (nn.ReLU, nn.PReLU)


class ClsLayerType:
    """How convert_layer_group_to_cls_sets sees a layer."""
    Unsupported = 0
    Conv = 1            # groups == 1, transposed or not
    DepthwiseConv = 2   # groups == in_channels == out_channels


def _cls_layer_type(layer) -> int:
    if layer.groups == 1:
        return ClsLayerType.Conv
    if layer.groups == layer.in_channels == layer.out_channels:
        return ClsLayerType.DepthwiseConv
    return ClsLayerType.Unsupported


class ClsSetInfo:
    """What cross-layer scaling did to one set: one ClsSetLayerPairInfo for a pair, two for a
    depthwise-separable triple (conv/depthwise and depthwise/conv). High-bias fold consumes it."""

    class ClsSetLayerPairInfo:
        """Two neighbouring layers of a set, the scale factor applied between them and whether a
        ReLU / PReLU sits between them."""

        def __init__(self, layer1, layer2, scale_factor: np.ndarray, relu_activation_between_layers: bool):
            self.layer1, self.layer2 = layer1, layer2
            self.scale_factor = scale_factor
            self.relu_activation_between_layers = relu_activation_between_layers

        def __eq__(self, other):
            if not isinstance(other, type(self)):
                return False
            return (self.layer1 is other.layer1 and self.layer2 is other.layer2
                    and self.relu_activation_between_layers == other.relu_activation_between_layers
                    and np.allclose(self.scale_factor, other.scale_factor))

        __hash__ = None

    def __init__(self, cls_pair_1: "ClsSetInfo.ClsSetLayerPairInfo", cls_pair_2: "ClsSetInfo.ClsSetLayerPairInfo" = None):
        self.cls_pair_info_list = [cls_pair_1] if cls_pair_2 is None else [cls_pair_1, cls_pair_2]

    def __eq__(self, other):
        return isinstance(other, type(self)) and self.cls_pair_info_list == other.cls_pair_info_list

    __hash__ = None


class GraphSearchUtils:
    """The layer groups, CLS sets and activations of a model, read off its torch.fx trace (pure
    Python, no device). input_shapes and dummy_input are accepted for compatibility."""

    def __init__(self, model: nn.Module, input_shapes=None, dummy_input=None):
        self._graph = _dfq.TracedGraph(model)

    def find_layer_groups_to_scale(self) -> List[List[nn.Module]]:
        """The maximal chains of supported layers (module docstring), in the order the layers run;
        chains of one layer are dropped. Each group is equalized on its own."""
        g = self._graph
        groups, taken = [], set()
        for node in g.nodes:
            first = g.module(node)
            if not isinstance(first, cls_supported_layers) or node in taken:
                continue
            taken.add(node)
            group, cur = [first], node
            while True:
                nxt = g.sole_user(cur, skip_identity=True)
                m = g.module(nxt) if nxt is not None else None
                if isinstance(m, cls_supported_activations):
                    cur = nxt
                elif isinstance(m, cls_supported_layers) and nxt not in taken:
                    taken.add(nxt)
                    group.append(m)
                    cur = nxt
                else:
                    break
            if len(group) > 1:
                groups.append(group)
        return groups

    @staticmethod
    def convert_layer_group_to_cls_sets(layer_group):
        """The CLS sets of one layer group, which is emptied as the reference empties it.

        Sets are conv + conv, depthwise + conv and conv + depthwise + conv; a layer closing one set
        opens the next. A grouped layer that is not depthwise is unsupported: the set it would be
        part of is dropped and the chain restarts after it. A conv + depthwise with nothing or no
        plain conv behind it gives no set of its own (the depthwise layer then opens the next).
        """
        layers = list(layer_group)
        del layer_group[:]
        kinds = [_cls_layer_type(layer) for layer in layers]
        n = len(layers)

        def kind(i):
            return ClsLayerType.Unsupported if i is None else kinds[i]

        cls_sets = []
        head, pos = None, 0   # the layer that opens the next set, the next unread layer
        while pos < n:
            while pos < n and kind(head) == ClsLayerType.Unsupported:
                head, pos = pos, pos + 1
            second = None
            if pos < n:
                second, pos = pos, pos + 1
            if kind(head) == ClsLayerType.Conv:
                if kind(second) == ClsLayerType.Conv:
                    cls_sets.append((layers[head], layers[second]))
                    head = second
                elif kind(second) == ClsLayerType.DepthwiseConv:
                    if pos < n:
                        if kinds[pos] == ClsLayerType.Conv:
                            cls_sets.append((layers[head], layers[second], layers[pos]))
                            head, pos = pos, pos + 1
                        else:
                            head = second
                else:
                    head = None
            elif kind(head) == ClsLayerType.DepthwiseConv:
                if kind(second) == ClsLayerType.Conv:
                    cls_sets.append((layers[head], layers[second]))
                head = second
            else:
                head = second
        return cls_sets

    def does_module_have_relu_activation(self, module: nn.Module) -> bool:
        """True if the only user of the module's output is a ReLU / PReLU module."""
        node = self._graph.node_of(module)
        if node is None:
            return False
        nxt = self._graph.sole_user(node, skip_identity=True)
        return nxt is not None and isinstance(self._graph.module(nxt), cls_supported_activations)

    def is_relu_activation_present_in_cls_sets(self, cls_sets: List[ClsSet]):
        """Per set whether a ReLU / PReLU follows each layer but the last: a bool for a pair, a tuple
        of two bools for a triple."""
        out = []
        for cls_set in cls_sets:
            flags = tuple(self.does_module_have_relu_activation(module) for module in cls_set[:-1])
            out.append(flags[0] if len(flags) == 1 else flags)
        return out


def _check_cls_layers(cls_set):
    for module in cls_set:
        if not isinstance(module, cls_supported_layers):
            raise ValueError("cross-layer scaling takes Conv1d/2d and ConvTranspose1d/2d layers, not %s"
                             % type(module).__name__)


def _set_tensors(cls_sets):
    out = []
    for cls_set in cls_sets:
        for m in cls_set:
            out += [m.weight, m.bias]
    return out


def _scale_cls_set_on_device(stage: "_dfq.Stage", cls_set):
    """One launch for one set; the scale vector(s) stay in device memory."""
    w = [stage.dev(m.weight) for m in cls_set]
    d = [_dfq.weight_desc(m, t) for m, t in zip(cls_set, w)]
    stream = ctypes.c_void_p(stage.stream)
    with torch.cuda.device(stage.device):
        if len(cls_set) == 2:
            s = stage.new(d[0].cout)
            _native.call("aimet_dfq_cls_pair", d[0], _dfq.ptr(stage.dev(cls_set[0].bias)), d[1], _dfq.ptr(s), stream)
            return s
        assert cls_set[1].groups > 1
        s12, s23 = stage.new(d[0].cout), stage.new(d[0].cout)
        _native.call("aimet_dfq_cls_triple", d[0], _dfq.ptr(stage.dev(cls_set[0].bias)), d[1],
                     _dfq.ptr(stage.dev(cls_set[1].bias)), d[2], _dfq.ptr(s12), _dfq.ptr(s23), stream)
        return s12, s23


class CrossLayerScaling:
    """Cross-layer scaling: per channel between two (or three) layers, the scale that gives both
    sides the same weight range, applied in place."""

    @staticmethod
    def scale_cls_sets(cls_sets: List[ClsSet]) -> List[ScaleFactor]:
        """Scales the given sets in order, one launch each; the scale factors are read back once at
        the end. Needs no graph. Returns per set a numpy array (pair) or a tuple of two (triple)."""
        cls_sets = list(cls_sets)
        if not cls_sets:
            return []
        for cls_set in cls_sets:
            if len(cls_set) not in (2, 3):
                raise ValueError("a CLS set has two or three layers")
            _check_cls_layers(cls_set)
        tensors = _set_tensors(cls_sets)
        _dfq.require_fp32(tensors, "cross-layer scaling")
        stage = _dfq.Stage(tensors)
        with torch.no_grad():
            on_device = [_scale_cls_set_on_device(stage, cls_set) for cls_set in cls_sets]
            stage.finish()
        out = []
        for s in on_device:
            out.append(tuple(t.cpu().numpy() for t in s) if isinstance(s, tuple) else s.cpu().numpy())
        return out

    @staticmethod
    def scale_cls_set(cls_set: ClsSet) -> ScaleFactor:
        """One set: a pair of layers, or conv + depthwise + conv. Returns what scale_cls_sets does."""
        if len(cls_set) == 3:
            return CrossLayerScaling.scale_cls_set_with_depthwise_layers(cls_set)
        return CrossLayerScaling.scale_cls_set_with_conv_layers(cls_set)

    @classmethod
    def scale_cls_set_with_conv_layers(cls, cls_set: ClsSet) -> np.ndarray:
        """A pair (conv + conv or depthwise + conv), weights and first bias updated in place; returns
        the scale factor per channel between them as a numpy array."""
        if len(cls_set) != 2:
            raise ValueError("scale_cls_set_with_conv_layers takes a pair of layers")
        return cls.scale_cls_sets([cls_set])[0]

    @classmethod
    def scale_cls_set_with_depthwise_layers(cls, cls_set: ClsSet) -> [np.ndarray, np.ndarray]:
        """A triple conv + depthwise conv + conv, the three weights and the first two biases updated in
        place; returns the two scale factors (first/second and second/third layer) as numpy arrays."""
        if len(cls_set) != 3:
            raise ValueError("scale_cls_set_with_depthwise_layers takes a triple of layers")
        return cls.scale_cls_sets([cls_set])[0]

    @staticmethod
    def create_cls_set_info_list(cls_sets: List[ClsSet], scale_factors: List[ScaleFactor],
                                 is_relu_activation_in_cls_sets):
        """
        One ClsSetInfo per set from the three parallel lists.
        :param cls_sets: List of CLS sets
        :param scale_factors: per set an array (pair) or a tuple of two arrays (triple)
        :param is_relu_activation_in_cls_sets: per set a bool (pair) or a tuple of two bools (triple)
        :return: List of ClsSetInfo
        """
        if not len(cls_sets) == len(scale_factors) == len(is_relu_activation_in_cls_sets):
            raise ValueError("cls_sets, scale_factors and relu flags differ in length")
        Pair = ClsSetInfo.ClsSetLayerPairInfo
        infos = []
        for layers, scales, relus in zip(cls_sets, scale_factors, is_relu_activation_in_cls_sets):
            if isinstance(scales, tuple):
                if not (len(layers) == 3 and len(scales) == 2 and len(relus) == 2):
                    raise ValueError("a triple needs three layers, two scale factors and two relu flags")
                infos.append(ClsSetInfo(Pair(layers[0], layers[1], scales[0], relus[0]),
                                        Pair(layers[1], layers[2], scales[1], relus[1])))
            else:
                infos.append(ClsSetInfo(Pair(layers[0], layers[1], scales, relus)))
        return infos

    @staticmethod
    def scale_model(model: nn.Module, input_shapes=None, dummy_input=None) -> List[ClsSetInfo]:
        """Finds the model's sets on its fx trace and scales them all; returns one ClsSetInfo per set,
        which HighBiasFold.bias_fold takes. input_shapes and dummy_input are not needed."""
        if isinstance(model, nn.DataParallel):
            return CrossLayerScaling.scale_model(model.module, input_shapes, dummy_input=dummy_input)
        search = GraphSearchUtils(model)
        cls_sets = [s for group in search.find_layer_groups_to_scale()
                    for s in GraphSearchUtils.convert_layer_group_to_cls_sets(group)]
        scale_factors = CrossLayerScaling.scale_cls_sets(cls_sets)
        relus = search.is_relu_activation_present_in_cls_sets(cls_sets)
        return CrossLayerScaling.create_cls_set_info_list(cls_sets, scale_factors, relus)


class HighBiasFold:
    """High-bias folding: the part of a layer's bias that lies three (scaled) BatchNorm gammas above
    zero passes the ReLU unchanged, so it is taken out of that bias and, through the next layer's
    weights, added to the next bias. Activations get smaller, the function stays (for inputs that
    follow the BatchNorm statistics)."""

    ActivationIsReluForFirstModule = bool
    ScaleForFirstModule = np.ndarray

    @classmethod
    def bias_fold(cls, cls_set_info_list: List[ClsSetInfo], bn_layers: Dict[nn.Module, nn.Module]):
        """One launch per pair of `cls_set_info_list`. bn_layers maps a layer to the BatchNorm that was
        folded into it (its gamma and beta are read). A pair is skipped when either bias is missing
        or its first layer had no folded BatchNorm."""
        if not bn_layers:
            return
        pairs = []
        for cls_set_info in cls_set_info_list:
            for p in cls_set_info.cls_pair_info_list:
                if p.layer1.bias is None or p.layer2.bias is None or p.layer1 not in bn_layers:
                    continue
                bn = bn_layers[p.layer1]
                if len(p.scale_factor) != bn.weight.numel() or len(p.scale_factor) != bn.bias.numel():
                    raise ValueError("High Bias absorption is not supported for networks with fold-forward BatchNorms")
                pairs.append((p, bn))
        if not pairs:
            return
        tensors = []
        for p, bn in pairs:
            tensors += [p.layer1.bias, p.layer2.bias, p.layer2.weight, bn.weight, bn.bias]
        _dfq.require_fp32(tensors, "high-bias fold")
        stage = _dfq.Stage(tensors)
        with torch.no_grad(), torch.cuda.device(stage.device):
            for p, bn in pairs:
                scale = torch.from_numpy(np.ascontiguousarray(p.scale_factor, dtype=np.float32)).to(stage.device)
                w2 = stage.dev(p.layer2.weight)
                _native.call("aimet_dfq_bias_fold", _dfq.ptr(stage.dev(bn.weight)), _dfq.ptr(stage.dev(bn.bias)),
                             _dfq.ptr(scale), scale.numel(), 1 if p.relu_activation_between_layers else 0,
                             _dfq.ptr(stage.dev(p.layer1.bias)), _dfq.weight_desc(p.layer2, w2),
                             _dfq.ptr(stage.dev(p.layer2.bias)), ctypes.c_void_p(stage.stream))
            stage.finish()


def equalize_model(model: nn.Module, input_shapes=None, dummy_input=None):
    """Cross-layer equalization of `model`, in place: ReLU6 becomes ReLU, batch norms are folded, then
    cross-layer scaling on the sets found and high-bias folding. input_shapes and dummy_input are
    accepted for compatibility; the graph comes from torch.fx."""
    if isinstance(model, nn.DataParallel):
        equalize_model(model.module, input_shapes, dummy_input)
        return
    _dfq.replace_modules(model, lambda m: isinstance(m, nn.ReLU6), lambda m: nn.ReLU())
    folded_pairs = fold_all_batch_norms(model, input_shapes, dummy_input=dummy_input)
    equalize_bn_folded_model(model, input_shapes, folded_pairs, dummy_input=dummy_input)


def equalize_bn_folded_model(model: nn.Module, input_shapes=None, folded_pairs=(), dummy_input=None):
    """Cross-layer scaling and high-bias folding, in place, of a model whose batch norms are folded
    already; folded_pairs is what fold_all_batch_norms returned ([(layer, bn)])."""
    if isinstance(model, nn.DataParallel):
        equalize_bn_folded_model(model.module, input_shapes, folded_pairs, dummy_input=dummy_input)
        return
    bn_dict = {conv: bn for conv, bn in folded_pairs}
    _dfq.replace_modules(model, lambda m: isinstance(m, nn.ReLU6), lambda m: nn.ReLU())
    cls_set_info_list = CrossLayerScaling.scale_model(model, input_shapes, dummy_input=dummy_input)
    HighBiasFold.bias_fold(cls_set_info_list, bn_dict)
