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
and not needed.

``fold_all_batch_norms_to_scale(sim)`` closes the QAT recipe for models that train with live
BatchNorms (range learning, then ``bn_reestimation.reestimate_bn_stats``, then this): every
conv-wrapper -> bn-wrapper pair of the sim is folded into the conv's weight, bias and learned
per-channel weight range in one ``aimet_bnre_fold_scale`` launch; the reference folds pair by pair
through the host and builds each channel's encoding in a Python loop. The pairs come from the same
fx search with the quantization wrappers as leaf modules. ``prepare_for_fold_to_scale(sim)``, called
before ``compute_encodings``, switches off the quantizers the reference's Conv + BatchNorm supergroup
switches off (this sim reads no supergroup configuration). One difference from the reference: a
per-tensor weight quantizer on a layer with several output channels is refused with a warning (the
reference applies the first channel's scale to the one encoding).
"""
import contextlib
import logging
from typing import Iterable, List, Tuple, Union

import torch
from torch import nn

from aimet_amd import _dfq

_logger = logging.getLogger("aimet_amd.batch_norm_fold")

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


# ---------------------------------------------------------------------------------------------------
# fold to scale: BatchNorms of a QuantizationSimModel after range-learning QAT
# ---------------------------------------------------------------------------------------------------
def _find_scale_pairs(sim) -> List[Tuple]:
    """(conv wrapper, bn wrapper) pairs of sim.model, from the fx trace with the quantization wrappers
    as leaves: the conv wrapper's output has the BatchNorm wrapper as sole user and both are called
    once. A BatchNorm wrapper left over that feeds a conv wrapper raises, as in the reference."""
    from aimet_amd.qc_quantize_op import QcQuantizeWrapper

    def wraps(m, types):
        return isinstance(m, QcQuantizeWrapper) and isinstance(m._module_to_wrap, types)

    g = _dfq.TracedGraph(sim.model, is_leaf=lambda m: isinstance(m, QcQuantizeWrapper))
    pairs, picked = [], set()
    for node in g.nodes:
        conv = g.module(node)
        if not wraps(conv, _supported_layers) or g.calls.get(conv, 0) != 1:
            continue
        user = g.sole_user(node)
        bn = g.module(user) if user is not None else None
        if wraps(bn, _supported_batchnorms) and _foldable_bn(bn._module_to_wrap) and g.calls.get(bn, 0) == 1 \
                and bn not in picked:
            pairs.append((conv, bn))
            picked.add(bn)
    for node in g.nodes:
        bn = g.module(node)
        if not wraps(bn, _supported_batchnorms) or bn in picked or g.calls.get(bn, 0) != 1:
            continue
        user = g.sole_user(node)
        conv = g.module(user) if user is not None else None
        if wraps(conv, _supported_layers) and g.calls.get(conv, 0) == 1 and \
                _is_valid_bn_fold(conv._module_to_wrap, False):
            raise RuntimeError("Forward folding to scale is not possible. Got %s" % (conv,))
    return pairs


def prepare_for_fold_to_scale(sim) -> List[Tuple]:
    """To be called on a new sim, before compute_encodings: for every (conv wrapper, bn wrapper) pair
    fold_all_batch_norms_to_scale would fold, disables the conv's output quantizers and the
    BatchNorm's parameter quantizers, which is what the reference's Conv + BatchNorm supergroup does
    when it builds a sim (this sim reads no supergroup configuration). The BatchNorm types must be
    among the sim's quantizable_types. Returns the pairs."""
    pairs = _find_scale_pairs(sim)
    for conv, bn in pairs:
        conv.enable_output_quantizers(False)
        bn.enable_param_quantizers(False, param_name_to_exclude=None)
    return pairs


def _scale_fold_refusal(conv_wrapper) -> str:
    """Why this conv wrapper cannot take a BatchNorm into its scale, or None."""
    from aimet_amd.learned_grid import LearnedGridTensorQuantizer
    conv = conv_wrapper._module_to_wrap
    weight_quantizer = conv_wrapper.param_quantizers["weight"]
    if not isinstance(weight_quantizer, LearnedGridTensorQuantizer):
        return "BatchNorm folding to scale supports LearnedGridTensorQuantizer only; got %s." % type(weight_quantizer)
    if conv_wrapper.output_quantizers[0].enabled:
        return "BatchNorm should belong to the same supergroup with the layer to be folded to."
    if "bias" in conv_wrapper.param_quantizers and conv_wrapper.param_quantizers["bias"].enabled:
        return "Can't fold BatchNorm to scale if bias quantizer is enabled."
    if isinstance(conv, (nn.ConvTranspose1d, nn.ConvTranspose2d, nn.ConvTranspose3d)) and conv.groups != 1:
        return "BatchNorm folding to scale is not supported for grouped ConvTransposeNd."
    emin, _ = weight_quantizer._params()
    if emin is not None and emin.numel() == 1 and _out_channels(conv) > 1:
        # not in the reference, which pairs the one encoding with the first channel's scale only
        return "a per-tensor weight quantizer cannot follow the per-channel scales of a BatchNorm."
    return None


def fold_all_batch_norms_to_scale(sim) -> List[Tuple]:
    """Folds every BatchNorm wrapper of `sim` that follows a conv / linear wrapper into that layer's
    weight, bias and learned per-channel weight encodings: w[o] *= c[o] and (min, max)[o] *= c[o]
    (ends swapped for a negative c[o]) with c = gamma / sqrt(running_var + eps), all pairs in one
    ``aimet_bnre_fold_scale`` launch. The conv's output quantizers take over the BatchNorm's, the
    BatchNorm wrapper becomes nn.Identity. Pairs the reference refuses (a weight quantizer that does
    not learn its range, an enabled conv output or bias quantizer, a grouped ConvTransposeNd) and a
    per-tensor weight quantizer on a layer with several output channels are skipped with a warning.
    Returns the (conv wrapper, bn wrapper) pairs folded."""
    from aimet_amd.learned_grid import LearnedGridTensorQuantizer
    from aimet_amd.quantsim import QuantizationSimModel
    if not isinstance(sim, QuantizationSimModel):
        raise NotImplementedError("fold_all_batch_norms_to_scale takes a QuantizationSimModel, got %s"
                                  % type(sim).__name__)
    names = {m: n for n, m in sim.model.named_modules()}
    accepted = []
    for conv_wrapper, bn_wrapper in _find_scale_pairs(sim):
        reason = _scale_fold_refusal(conv_wrapper)
        if reason is not None:
            _logger.warning("Failed to fold %s to %s. [Reason] %s", names.get(bn_wrapper), names.get(conv_wrapper),
                            reason)
            continue
        q = conv_wrapper.param_quantizers["weight"]
        if not q.enabled or q.bitwidth == 32 or q.encoding_tensors() is None:
            raise RuntimeError("fold_all_batch_norms_to_scale: %s has no weight encoding" % names.get(conv_wrapper))
        if q.is_encoding_frozen:
            raise RuntimeError("Encoding can be set only when it is not frozen.")
        accepted.append((conv_wrapper, bn_wrapper))
    if not accepted:
        return []

    tensors = []
    for conv_wrapper, bn_wrapper in accepted:
        conv, bn = conv_wrapper._module_to_wrap, bn_wrapper._module_to_wrap
        tensors += [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    _dfq.require_fp32(tensors, "batch norm fold to scale")
    stage = _dfq.Stage(tensors)
    with torch.no_grad(), contextlib.ExitStack() as quantized_bn_params:
        jobs, ranges = [], []
        for conv_wrapper, bn_wrapper in accepted:
            conv, bn = conv_wrapper._module_to_wrap, bn_wrapper._module_to_wrap
            if conv.bias is None:
                conv.bias = nn.Parameter(torch.zeros(_out_channels(conv), device=conv.weight.device,
                                                     dtype=conv.weight.dtype))
            w = stage.dev(conv.weight)
            cout = _dfq.weight_desc(conv, w).cout
            q = conv_wrapper.param_quantizers["weight"]
            # the encoding getter's min and max, still on the device
            enc_min, enc_max = (t.to(stage.device).expand(cout).clone() for t in q.encoding_tensors()[:2])
            if bn.num_features != cout or conv.bias.numel() != cout:
                raise ValueError("batch norm fold: %r has %d features, %r needs %d" % (bn, bn.num_features, conv, cout))
            quantized_bn_params.enter_context(bn_wrapper._quantize_params())
            jobs.append(dict(module=conv, weight=w, bias=stage.dev(conv.bias), bn=bn, forward=False,
                             enc_min=enc_min, enc_max=enc_max))
            ranges.append((q, enc_min, enc_max))
        _dfq.bn_fold_scale_launch(stage, jobs)
        stage.finish()
    for q, enc_min, enc_max in ranges:
        old_min, old_max = q._params()
        params = q.wrapper_ref._parameters
        params[q.name + "_encoding_min"] = nn.Parameter(enc_min.to(old_min.device), requires_grad=old_min.requires_grad)
        params[q.name + "_encoding_max"] = nn.Parameter(enc_max.to(old_max.device), requires_grad=old_max.requires_grad)

    for conv_wrapper, bn_wrapper in accepted:
        for conv_q, bn_q in zip(conv_wrapper.output_quantizers, bn_wrapper.output_quantizers):
            conv_q.enabled = bn_q.enabled
            encoding = bn_q.encoding
            if encoding is not None:
                conv_q.encoding = encoding   # creates the wrapper's range parameters
                # then the learned range itself rather than its grid-adjusted report, so that the
                # quantizer that moved computes what it computed before, bit for bit
                with torch.no_grad():
                    for dst, src in zip(conv_q._params(), bn_q._params()):
                        dst.copy_(src)
            bn_q.enabled = False
        if "bias" not in conv_wrapper.param_quantizers:
            weight_q = conv_wrapper.param_quantizers["weight"]
            bias_q = LearnedGridTensorQuantizer(weight_q.bitwidth, weight_q.round_mode, weight_q.quant_scheme,
                                                weight_q.use_symmetric_encodings, enabled_by_default=False,
                                                data_type=weight_q.data_type)
            bias_q._ch_axis = weight_q._ch_axis
            bias_q.name, bias_q.wrapper_ref, bias_q.device = "bias", conv_wrapper, weight_q.device
            conv_wrapper.register_parameter("bias_encoding_min", None)
            conv_wrapper.register_parameter("bias_encoding_max", None)
            conv_wrapper.param_quantizers["bias"] = bias_q
    folded = {id(bn_wrapper) for _, bn_wrapper in accepted}
    _dfq.replace_modules(sim.model, lambda m: id(m) in folded, lambda m: nn.Identity())
    return accepted


class BatchNormFold:
    """The reference's class-style access to the same functions."""
    fold_given_batch_norms = staticmethod(fold_given_batch_norms)
    fold_all_batch_norms_to_weight = staticmethod(fold_all_batch_norms_to_weight)
    fold_all_batch_norms_to_scale = staticmethod(fold_all_batch_norms_to_scale)
    prepare_for_fold_to_scale = staticmethod(prepare_for_fold_to_scale)
    find_all_batch_norms_to_fold = staticmethod(find_all_batch_norms_to_fold)
    _is_valid_bn_fold = staticmethod(_is_valid_bn_fold)
