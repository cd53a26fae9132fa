"""Batch-norm folding (aimet_torch/batch_norm_fold.py) on the MI355X core.

Same names and semantics as the reference: a folded BatchNorm becomes ``nn.Identity`` in its parent,
a conv / linear without a bias gains a zero bias first, ``(conv, bn)`` folds backward and
``(bn, conv)`` forward, backward has priority and each BatchNorm is folded at most once. What
differs is where the arithmetic runs: the reference copies every parameter of every layer to the
host and folds in numpy, one layer at a time; here all folds of one call are one
``aimet_dfq_bn_fold`` launch (aimet_amd/csrc/dfq.hip) that updates the parameters in place.

Pairs are found on a ``torch.fx.symbolic_trace`` of the model (the project has no ConnectedGraph):
conv -> bn when the conv's output has exactly one user and that user is the BatchNorm module, and
bn -> conv the same way round. ``input_shapes`` / ``dummy_input`` are accepted for compatibility
and not needed. ``fold_all_batch_norms_to_scale`` is not implemented.
"""
from typing import Iterable, List, Tuple, Union

import torch
from torch import nn

from aimet_amd import _dfq

LayerType = Union[nn.Linear, nn.Conv1d, nn.Conv2d, nn.ConvTranspose2d]
_supported_layers = (nn.Linear, nn.Conv1d, nn.Conv2d, nn.ConvTranspose2d)
BatchNormType = Union[nn.BatchNorm1d, nn.BatchNorm2d]
_supported_batchnorms = (nn.BatchNorm1d, nn.BatchNorm2d)


def _is_valid_bn_fold(conv: LayerType, fold_backward: bool) -> bool:
    """Whether `conv` can absorb a BatchNorm without changing the model's function.
    fold_backward: the BatchNorm follows the layer. Forward folding (BatchNorm first) is refused for
    padded convs (the BatchNorm's shift would not reach the padding), for grouped and depthwise
    convs and for ConvTranspose2d; backward folding is refused for a grouped ConvTranspose2d unless
    groups is 1 or in_channels. Linear layers take both."""
    if fold_backward:
        if isinstance(conv, nn.ConvTranspose2d):
            return conv.groups in (1, conv.in_channels)
        return True
    if isinstance(conv, nn.ConvTranspose2d):
        return False
    if isinstance(conv, (nn.Conv1d, nn.Conv2d, nn.Conv3d)):
        return conv.groups == 1 and not any(conv.padding)
    return True


def _foldable_bn(bn: nn.Module) -> bool:
    return (isinstance(bn, _supported_batchnorms) and bn.weight is not None and bn.bias is not None
            and bn.running_mean is not None and bn.running_var is not None)


def _find_all_batch_norms_to_fold(model: nn.Module):
    """(conv, bn) pairs to fold backward, (bn, conv) pairs to fold forward and the set of BatchNorms
    picked, from the fx trace. A module called at more than one place of the graph is left alone."""
    g = _dfq.TracedGraph(model)
    conv_bn_pairs, bn_conv_pairs, picked = [], [], set()

    def once(m):
        return g.calls.get(m, 0) == 1

    # backward first: it has priority
    for node in g.nodes:
        conv = g.module(node)
        if not isinstance(conv, _supported_layers) or not once(conv):
            continue
        bn = g.module(g.sole_user(node)) if g.sole_user(node) is not None else None
        if _foldable_bn(bn) and once(bn) and bn not in picked and _is_valid_bn_fold(conv, True):
            conv_bn_pairs.append((conv, bn))
            picked.add(bn)
    for node in g.nodes:
        bn = g.module(node)
        if not _foldable_bn(bn) or not once(bn) or bn in picked:
            continue
        user = g.sole_user(node)
        conv = g.module(user) if user is not None else None
        if isinstance(conv, _supported_layers) and once(conv) and _is_valid_bn_fold(conv, False):
            bn_conv_pairs.append((bn, conv))
            picked.add(bn)
    return conv_bn_pairs, bn_conv_pairs, picked


def find_all_batch_norms_to_fold(model: nn.Module, input_shapes=None, dummy_input=None) -> List[Tuple]:
    """The pairs fold_all_batch_norms would fold, without folding: (layer, bn) for a backward fold,
    (bn, layer) for a forward one. input_shapes and dummy_input are accepted for compatibility."""
    conv_bn_pairs, bn_conv_pairs, _ = _find_all_batch_norms_to_fold(model)
    return conv_bn_pairs + bn_conv_pairs


def _out_channels(layer: nn.Module) -> int:
    return layer.out_features if isinstance(layer, nn.Linear) else layer.out_channels


def _fold_given_batch_norms(model: nn.Module, conv_bn_pairs: Iterable[Tuple], bn_conv_pairs: Iterable[Tuple]):
    conv_bn_pairs, bn_conv_pairs = list(conv_bn_pairs), list(bn_conv_pairs)
    folds = [(conv, bn, False) for conv, bn in conv_bn_pairs] + [(conv, bn, True) for bn, conv in bn_conv_pairs]
    if not folds:
        return
    seen = set()
    for conv, bn, forward in folds:
        if not isinstance(conv, _supported_layers):
            raise ValueError("batch norm fold: %s is not a supported layer" % type(conv).__name__)
        if not _foldable_bn(bn):
            raise ValueError("batch norm fold: %r is not a BatchNorm1d/2d with affine parameters and running "
                             "statistics" % (bn,))
        if id(bn) in seen:
            raise ValueError("batch norm fold: %r is listed twice" % (bn,))
        seen.add(id(bn))
        if not _is_valid_bn_fold(conv, not forward):
            raise ValueError("batch norm fold: %r cannot absorb a BatchNorm %s it" %
                             (conv, "before" if forward else "after"))
    tensors = []
    for conv, bn, _ in folds:
        tensors += [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    _dfq.require_fp32(tensors, "batch norm fold")
    stage = _dfq.Stage(tensors)

    with torch.no_grad():
        jobs = []
        for conv, bn, forward in folds:
            if conv.bias is None:
                conv.bias = nn.Parameter(torch.zeros(_out_channels(conv), device=conv.weight.device,
                                                     dtype=conv.weight.dtype))
            w = stage.dev(conv.weight)
            desc = _dfq.weight_desc(conv, w)
            want = desc.cin if forward else desc.cout
            if bn.num_features != want or (not forward and conv.bias.numel() != desc.cout):
                raise ValueError("batch norm fold: %r has %d features, %r needs %d" % (bn, bn.num_features, conv, want))
            jobs.append(dict(module=conv, weight=w, bias=stage.dev(conv.bias), bn=bn, forward=forward))
        # One launch for all folds. A layer that takes a BatchNorm on each side has two jobs on one
        # weight, which may not share a launch: its forward fold goes into a second one.
        first, second, used = [], [], set()
        for j in jobs:
            (second if id(j["module"]) in used else first).append(j)
            used.add(id(j["module"]))
        _dfq.bn_fold_launch(stage, first)
        _dfq.bn_fold_launch(stage, second)
        stage.finish()
    bns = {id(bn) for _, bn, _ in folds}
    _dfq.replace_modules(model, lambda m: id(m) in bns, lambda m: nn.Identity())


def fold_given_batch_norms(model: nn.Module, layer_pairs: Iterable[Tuple]):
    """Folds the listed pairs, in one launch, and replaces their BatchNorms by nn.Identity. A pair
    (layer, bn) folds backward, (bn, layer) forward. Needs no graph."""
    conv_bn_pairs, bn_conv_pairs = [], []
    for first, second in layer_pairs:
        if isinstance(first, _supported_batchnorms):
            bn_conv_pairs.append((first, second))
        else:
            conv_bn_pairs.append((first, second))
    _fold_given_batch_norms(model, conv_bn_pairs, bn_conv_pairs)   # checks the types of both sides


def fold_all_batch_norms_to_weight(model: nn.Module, input_shapes=None,
                                   dummy_input=None) -> List[Tuple[LayerType, BatchNormType]]:
    """Folds every BatchNorm that sits next to a conv or linear layer into that layer's weight and
    bias, all in one launch; returns the (layer, bn) pairs folded, backward folds first.
    input_shapes and dummy_input are accepted for compatibility."""
    if isinstance(model, nn.DataParallel):
        return fold_all_batch_norms_to_weight(model.module, input_shapes, dummy_input)
    conv_bn_pairs, bn_conv_pairs, _ = _find_all_batch_norms_to_fold(model)
    _fold_given_batch_norms(model, conv_bn_pairs, bn_conv_pairs)
    return conv_bn_pairs + [(conv, bn) for bn, conv in bn_conv_pairs]


fold_all_batch_norms = fold_all_batch_norms_to_weight


def fold_all_batch_norms_to_scale(sim):
    """Folding BatchNorms into the quantization scale of a QuantizationSimModel is out of scope."""
    raise NotImplementedError("fold_all_batch_norms_to_scale is not implemented in aimet_amd; fold into the weights "
                              "with fold_all_batch_norms before creating the QuantizationSimModel")


class BatchNormFold:
    """The reference's class-style access to the same functions."""
    fold_given_batch_norms = staticmethod(fold_given_batch_norms)
    fold_all_batch_norms_to_weight = staticmethod(fold_all_batch_norms_to_weight)
    fold_all_batch_norms_to_scale = staticmethod(fold_all_batch_norms_to_scale)
    find_all_batch_norms_to_fold = staticmethod(find_all_batch_norms_to_fold)
    _is_valid_bn_fold = staticmethod(_is_valid_bn_fold)
