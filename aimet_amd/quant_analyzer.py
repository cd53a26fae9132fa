"""QuantAnalyzer (aimet_torch/v1/quant_analyzer.py) on the MI355X core: which part of a model is
sensitive to quantization, and where.

1. model sensitivity to weight and to activation quantization, each alone;
2. per-layer sensitivity, by enabling one quant wrapper at a time and by disabling one at a time;
3. per-layer encoding min / max ranges;
4. per-layer statistics histograms (TF-Enhanced);
5. per-layer MSE between the fp32 and the quantized output activations.

Constructor, method and file names follow the reference. Three things differ.

* Plots. The reference writes bokeh HTML next to every JSON file. Here the JSON files are always
  written and the HTML only when ``import bokeh`` succeeds (one log line otherwise).
* The sensitivity analyses restore every quantizer's ``enabled`` flag in a ``finally``: an eval
  callback that raises leaves the sim as it found it.
* The per-layer MSE schedule. The reference, for every layer and every batch, runs both models up to
  that layer, takes torch's fp32 ``mse_loss`` and reads it back with ``.item()``: about L^2 / 2 layer
  executions per model per batch and L host synchronisations per batch. Here a batch is two full
  forwards: the fp32 model once with hooks that keep every listed module's output, the sim once with
  hooks that hand (fp32 output, quantized output) to ``aimet_qa_sq_err`` (aimet_amd/csrc/
  quant_analyzer.hip: both tensors read once, double arithmetic, no atomics) and drop the fp32 output.
  Each layer owns two doubles of one device table, ``sum (ref - q)^2 / numel`` and
  ``sum ref^2 / numel`` summed over the batches; the table is read back once, after the last batch.
  ``per_layer_mse_loss.json`` holds the reference's ``sum of batch MSEs / samples``, and
  ``per_layer_sqnr.json`` the ratio of the two sums in dB, which compares across layers where an
  absolute MSE does not.

There is no CPU compute path: a CPU-resident model is analyzed with its layer outputs copied to the
current HIP device for the reduction. DataParallel and torch.distributed sharding are out of scope.
"""
import contextlib
import ctypes
import json
import logging
import math
import os
from collections import OrderedDict
from typing import Callable, Collection, Dict, List, Tuple, Union

import torch

from aimet_amd import _native
from aimet_amd.activation_sampler import _device_of, _to_device, default_forward_fn
from aimet_amd.batch_norm_fold import fold_all_batch_norms
from aimet_amd.qc_quantize_op import QcQuantizeWrapper
from aimet_amd.quantizers import QuantScheme
from aimet_amd.quantsim import _SCHEME_NAMES, QuantizationSimModel, _eval_mode
from aimet_amd.seq_mse import get_ordered_list_of_modules

_logger = logging.getLogger("aimet_amd.quant_analyzer")

_IO_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}   # aimet_qa_sq_err's io_dtype
LAUNCHES_PER_LAYER_BATCH = 2    # aimet_qa_sq_err: the partial sums and their fold

_bokeh_state = {"checked": False, "available": False}


class CallbackFunc:
    """aimet_common/utils.py CallbackFunc: a callback and its argument(s), called as func(model, args)."""

    def __init__(self, func: Callable, func_callback_args=None):
        self.func = func
        self.args = func_callback_args


def launch_count(reset: bool = False) -> int:
    """Kernel launches aimet_qa_sq_err has issued in this process."""
    n = ctypes.c_int64()
    _native.call("aimet_qa_launch_count", ctypes.byref(n), 1 if reset else 0)
    return n.value


def add_sq_err(ref: torch.Tensor, x: torch.Tensor, scale: float, acc: torch.Tensor):
    """acc[0] += scale * sum (ref - x)^2, acc[1] += scale * sum ref^2 (aimet_qa_sq_err): ref and x
    contiguous device tensors of one shape and dtype (float32 / float16 / bfloat16), acc two float64
    on the same device."""
    if ref.shape != x.shape or ref.dtype != x.dtype or ref.dtype not in _IO_DTYPES:
        raise ValueError("squared error: needs two float32 / float16 / bfloat16 tensors of one shape and dtype")
    if not (ref.is_cuda and x.is_cuda and acc.is_cuda) or not (ref.is_contiguous() and x.is_contiguous()):
        raise ValueError("squared error: needs contiguous device tensors; the MI355X core has no CPU path")
    if acc.dtype != torch.float64 or acc.numel() != 2 or not acc.is_contiguous():
        raise ValueError("squared error: the accumulator is two contiguous float64")
    with torch.cuda.device(ref.device):
        _native.call("aimet_qa_sq_err", ctypes.c_void_p(ref.data_ptr()), ctypes.c_void_p(x.data_ptr()), ref.numel(),
                     _IO_DTYPES[ref.dtype], float(scale), ctypes.c_void_p(acc.data_ptr()),
                     ctypes.c_void_p(torch.cuda.current_stream(ref.device).cuda_stream))


# ---------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------
def _json_value(v):
    if isinstance(v, dict):
        return {k: _json_value(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_json_value(x) for x in v]
    if isinstance(v, torch.Tensor):
        v = v.item()
    if isinstance(v, float) and not math.isfinite(v):
        return "nan" if math.isnan(v) else ("inf" if v > 0 else "-inf")
    return v


def save_json(data: Dict, results_dir: str, title: str):
    """aimet_common/quant_analyzer.py save_json; a non-finite float is written as a string."""
    os.makedirs(results_dir, exist_ok=True)
    with open(os.path.join(results_dir, title), "w") as f:
        json.dump(_json_value(data), f, indent=4)


def _bokeh():
    """bokeh.plotting when bokeh is installed, else None (logged once)."""
    if not _bokeh_state["checked"]:
        _bokeh_state["checked"] = True
        try:
            import bokeh.plotting  # noqa: F401
            _bokeh_state["available"] = True
        except ImportError:
            _logger.info("bokeh is not installed: QuantAnalyzer writes its JSON files only, no HTML plots")
    if not _bokeh_state["available"]:
        return None
    import bokeh.plotting
    return bokeh.plotting


def _export_line_plot(xs: List, ys: List[float], results_dir: str, title: str, x_is_category: bool = True):
    """One HTML plot of ys over xs (the reference's per-layer plots), when bokeh is installed."""
    plotting = _bokeh()
    if plotting is None:
        return
    os.makedirs(results_dir, exist_ok=True)
    plotting.output_file(os.path.join(results_dir, title + ".html"), title=title)
    if x_is_category:
        fig = plotting.figure(x_range=[str(x) for x in xs], title=title, height=300, sizing_mode="stretch_width")
        fig.line([str(x) for x in xs], ys)
        fig.xaxis.major_label_orientation = "vertical"
    else:
        fig = plotting.figure(title=title, height=300, sizing_mode="stretch_width")
        fig.line(xs, ys)
    plotting.save(fig)


def _export_range_plot(ranges: Dict, results_dir: str, title: str):
    plotting = _bokeh()
    if plotting is None or not ranges:
        return
    os.makedirs(results_dir, exist_ok=True)
    names = list(ranges)
    plotting.output_file(os.path.join(results_dir, title + ".html"), title=title)
    fig = plotting.figure(x_range=names, title=title, height=300, sizing_mode="stretch_width")
    fig.vbar(x=names, bottom=[ranges[n][0] for n in names], top=[ranges[n][1] for n in names], width=0.6)
    fig.xaxis.major_label_orientation = "vertical"
    plotting.save(fig)


# ---------------------------------------------------------------------------------------------------
# quantizer bookkeeping
# ---------------------------------------------------------------------------------------------------
def _quantized_modules(sim: QuantizationSimModel):
    for module in sim.model.modules():
        if isinstance(module, QcQuantizeWrapper):
            yield module


def _wrapper_quantizers(wrapper: QcQuantizeWrapper) -> List:
    """The wrapper's quantizers in the reference's order: parameters, outputs, inputs."""
    return list(wrapper.param_quantizers.values()) + list(wrapper.output_quantizers) + list(wrapper.input_quantizers)


def _encodings_of(quantizer) -> List:
    encoding = quantizer.encoding
    if encoding and not isinstance(encoding, list):
        return [encoding]
    return encoding


@contextlib.contextmanager
def _disabled(quantizers: List):
    """The given (enabled) quantizers disabled for the duration, whatever happens inside."""
    for q in quantizers:
        q.enabled = False
    try:
        yield
    finally:
        for q in quantizers:
            q.enabled = True


class QuantAnalyzer:
    """
    QuantAnalyzer tool provides

     1) model sensitivity to weight and activation quantization
     2) per layer sensitivity analysis
     3) per layer encoding (min - max range)
     4) per PDF analysis and
     5) per layer MSE analysis
    """

    def __init__(self, model: torch.nn.Module, dummy_input: Union[torch.Tensor, Tuple],
                 forward_pass_callback: CallbackFunc, eval_callback: CallbackFunc,
                 modules_to_ignore: List[torch.nn.Module] = None):
        """
        :param model: FP32 model to analyze for quantization.
        :param dummy_input: Dummy input to model.
        :param forward_pass_callback: CallbackFunc whose func(model, args) runs the forward passes that
                calibrate the sim (a representative subset of the data, ~1000 samples).
        :param eval_callback: CallbackFunc whose func(model, args) returns a scalar score of the model.
        :param modules_to_ignore: Excludes certain modules from being analyzed.
        """
        if not isinstance(forward_pass_callback, CallbackFunc):
            raise ValueError('forward_pass_callback and its argument(s) are not encapsulated by CallbackFunc class.')
        if not isinstance(eval_callback, CallbackFunc):
            raise ValueError('eval_callback and its argument(s) are not encapsulated by CallbackFunc class.')
        self._model = model
        self._dummy_input = dummy_input
        self._forward_pass_callback = forward_pass_callback
        self._eval_callback = eval_callback
        self._unlabeled_dataset_iterable = None
        self._num_batches = None
        self._modules_to_ignore = modules_to_ignore

    def analyze(self, quant_scheme: Union[str, QuantScheme] = QuantScheme.post_training_tf_enhanced,
                default_param_bw: int = 8, default_output_bw: int = 8, config_file: str = None,
                results_dir: str = "./tmp/"):
        """
        Folds the model's batch norms in place, builds and calibrates a QuantizationSimModel, then
            1) model sensitivity to quantization,
            2) per layer sensitivity analysis by enabling and by disabling quant wrappers,
            3) per layer encoding min - max ranges,
            4) per layer statistics histograms (PDF) when the quant scheme is TF-Enhanced,
            5) per layer MSE analysis, when enable_per_layer_mse_loss() was called.

        :param quant_scheme: QuantScheme.post_training_tf or QuantScheme.post_training_tf_enhanced.
        :param default_param_bw: Default bitwidth (4-31) to use for quantizing layer parameters.
        :param default_output_bw: Default bitwidth (4-31) to use for quantizing layer inputs and outputs.
        :param config_file: Path to configuration file for model quantizers.
        :param results_dir: Directory to save the results.
        """
        if isinstance(quant_scheme, str):
            quant_scheme = _SCHEME_NAMES.get(quant_scheme, quant_scheme)
        if quant_scheme not in (QuantScheme.post_training_tf, QuantScheme.post_training_tf_enhanced):
            raise ValueError("QuantAnalyzer supports post_training_tf and post_training_tf_enhanced, not %r"
                             % (quant_scheme,))
        sim = self._create_quantsim_and_encodings(quant_scheme, default_param_bw, default_output_bw, config_file)

        results_dir = os.path.abspath(results_dir)
        os.makedirs(results_dir, exist_ok=True)

        self.check_model_sensitivity_to_quantization(sim)
        self.perform_per_layer_analysis_by_enabling_quant_wrappers(sim, results_dir)
        self.perform_per_layer_analysis_by_disabling_quant_wrappers(sim, results_dir)
        self.export_per_layer_encoding_min_max_range(sim, results_dir)
        if quant_scheme == QuantScheme.post_training_tf_enhanced:
            self.export_per_layer_stats_histogram(sim, results_dir)
        if self._unlabeled_dataset_iterable:
            self.export_per_layer_mse_loss(sim, results_dir)

    def enable_per_layer_mse_loss(self, unlabeled_dataset_iterable: Collection, num_batches: int):
        """
        Enable per layer MSE loss analysis.

        :param unlabeled_dataset_iterable: A collection (an iterable with `__len__`) over an unlabeled
                dataset; what it yields is passed to the model as it is.
        :param num_batches: Number of batches (about 256 samples are recommended).
        """
        if len(unlabeled_dataset_iterable) < num_batches:
            raise ValueError(f'Can not fetch {num_batches} batches from '
                             f'a data loader of length {len(unlabeled_dataset_iterable)}.')
        self._unlabeled_dataset_iterable = unlabeled_dataset_iterable
        self._num_batches = num_batches

    def _create_quantsim_and_encodings(self, quant_scheme: QuantScheme, default_param_bw: int,
                                       default_output_bw: int, config_file: str) -> QuantizationSimModel:
        if isinstance(self._dummy_input, torch.Tensor):
            input_shape = tuple(self._dummy_input.shape)
        else:
            input_shape = [tuple(x.shape) for x in self._dummy_input]
        fold_all_batch_norms(self._model, input_shape, dummy_input=self._dummy_input)
        sim = QuantizationSimModel(self._model, self._dummy_input, quant_scheme=quant_scheme,
                                   default_output_bw=default_output_bw, default_param_bw=default_param_bw,
                                   config_file=config_file)
        if self._modules_to_ignore:
            self._exclude_modules_from_quantization(self._model, sim, self._modules_to_ignore)
        sim.compute_encodings(self._forward_pass_callback.func, self._forward_pass_callback.args)
        return sim

    @staticmethod
    def _exclude_modules_from_quantization(model: torch.nn.Module, sim: QuantizationSimModel,
                                           modules_to_ignore: List[torch.nn.Module]):
        """Removes the quant wrappers that stand, in the sim, where the given modules stand in the model."""
        in_sim = dict(sim.model.named_modules())
        name_of = {module: name for name, module in model.named_modules()}
        sim.exclude_layers_from_quantization([in_sim[name_of[module]] for module in modules_to_ignore])

    # -- sensitivity --------------------------------------------------------------------------------
    def _eval_model(self, model: torch.nn.Module):
        with _eval_mode(model), torch.no_grad():
            return self._eval_callback.func(model, self._eval_callback.args)

    def _sort_quant_wrappers_based_on_occurrence(self, sim: QuantizationSimModel) -> Dict[str, QcQuantizeWrapper]:
        """{wrapped module name: quant wrapper} in the order one forward of dummy_input first runs them."""
        name_of = {module: name for name, module in sim.model.named_modules()}
        ordered = OrderedDict()

        def hook(wrapper, *_):
            ordered.setdefault(name_of[wrapper], wrapper)
        handles = [w.register_forward_hook(hook) for w in _quantized_modules(sim)]
        try:
            with _eval_mode(sim.model), torch.no_grad():
                default_forward_fn(sim.model, _to_device(self._dummy_input, _device_of(sim.model)))
        finally:
            for h in handles:
                h.remove()
        return ordered

    def _perform_per_layer_analysis(self, sim: QuantizationSimModel, enable_one: bool) -> Dict:
        """enable_one: every enabled quantizer off except the visited wrapper's; else only the visited
        wrapper's off. A wrapper with no enabled quantizer is not visited."""
        ordered = self._sort_quant_wrappers_based_on_occurrence(sim)
        enabled = OrderedDict()
        for wrapper in ordered.values():
            quantizers = [q for q in _wrapper_quantizers(wrapper) if q.enabled]
            if quantizers:
                enabled[wrapper] = quantizers
        scores = {}
        for name, wrapper in ordered.items():
            if wrapper not in enabled:
                continue
            if enable_one:
                off = [q for other, quantizers in enabled.items() if other is not wrapper for q in quantizers]
            else:
                off = enabled[wrapper]
            with _disabled(off):
                scores[name] = self._eval_model(sim.model)
            _logger.debug("For layer: %s, the eval score is: %s", name, scores[name])
        return scores

    def check_model_sensitivity_to_quantization(self, sim: QuantizationSimModel) -> Tuple[float, float, float]:
        """
        The eval score of the fp32 model, of the sim with only its weights quantized and of the sim
        with only its activations quantized.

        :param sim: Quantsim model.
        :return: FP32 eval score, weight-quantized eval score, act-quantized eval score.
        """
        fp32_eval_score = self._eval_model(self._model)
        _logger.info("FP32 eval score (W32A32): %s", fp32_eval_score)

        activations = [q for w in _quantized_modules(sim) for q in list(w.input_quantizers) + list(w.output_quantizers)
                       if q.enabled]
        with _disabled(activations):
            weight_quantized_eval_score = self._eval_model(sim.model)
        _logger.info("Weight-quantized eval score (W%dA32): %s", sim._default_param_bw, weight_quantized_eval_score)

        params = [q for w in _quantized_modules(sim) for q in w.param_quantizers.values() if q.enabled]
        with _disabled(params):
            act_quantized_eval_score = self._eval_model(sim.model)
        _logger.info("Activation-quantized eval score (W32A%d): %s", sim._default_output_bw, act_quantized_eval_score)
        return fp32_eval_score, weight_quantized_eval_score, act_quantized_eval_score

    def perform_per_layer_analysis_by_enabling_quant_wrappers(self, sim: QuantizationSimModel,
                                                              results_dir: str) -> Dict:
        """
        Option 1: all quantizers disabled; in execution order each quant wrapper's quantizers are
        enabled as they were, the model is scored, and they are disabled again.

        :param sim: Quantsim model.
        :param results_dir: Directory to save the results (per_layer_quant_enabled.json).
        :return: layer wise eval score dictionary. dict[layer_name] = eval_score
        """
        results_dir = os.path.abspath(results_dir)
        scores = self._perform_per_layer_analysis(sim, enable_one=True)
        _export_line_plot(list(scores), [float(v) for v in scores.values()], results_dir, "per_layer_quant_enabled")
        save_json(scores, results_dir, title="per_layer_quant_enabled.json")
        return scores

    def perform_per_layer_analysis_by_disabling_quant_wrappers(self, sim: QuantizationSimModel,
                                                               results_dir: str) -> Dict:
        """
        Option 2: all quantizers enabled as they were; in execution order each quant wrapper's
        quantizers are disabled, the model is scored, and they are enabled again.

        :param sim: Quantsim model.
        :param results_dir: Directory to save the results (per_layer_quant_disabled.json).
        :return: layer wise eval score dictionary. dict[layer_name] = eval_score
        """
        results_dir = os.path.abspath(results_dir)
        scores = self._perform_per_layer_analysis(sim, enable_one=False)
        _export_line_plot(list(scores), [float(v) for v in scores.values()], results_dir, "per_layer_quant_disabled")
        save_json(scores, results_dir, title="per_layer_quant_disabled.json")
        return scores

    # -- ranges and histograms ----------------------------------------------------------------------
    def export_per_layer_encoding_min_max_range(self, sim: QuantizationSimModel, results_dir: str) -> Tuple[Dict, Dict]:
        """
        Encoding min and max of every enabled weight and activation quantizer, into
        results_dir/min_max_ranges/weights.json and activations.json. A per-channel parameter's entry
        is a dict {name}_{channel}: (min, max).

        :param sim: Quantsim model.
        :param results_dir: Directory to save the results.
        :return: layer wise min-max range for weights and activations.
        """
        min_max_ranges_dir = os.path.join(results_dir, "min_max_ranges")
        name_of = {module: name for name, module in sim.model.named_modules()}
        activations, weights = {}, {}
        for wrapper in _quantized_modules(sim):
            wrapped = name_of[wrapper]
            for kind, quantizers in (("input", wrapper.input_quantizers), ("output", wrapper.output_quantizers)):
                for index, quantizer in enumerate(quantizers):
                    if quantizer.enabled:
                        encoding = _encodings_of(quantizer)[0]
                        activations[f"{wrapped}_{kind}_{index}"] = (encoding.min, encoding.max)
            for param_name, quantizer in wrapper.param_quantizers.items():
                if quantizer.enabled:
                    name = f"{wrapped}_{param_name}"
                    encodings = _encodings_of(quantizer)
                    if isinstance(quantizer.encoding, list):   # per-channel, also with one channel
                        weights[name] = {f"{name}_{index}": (e.min, e.max) for index, e in enumerate(encodings)}
                    else:
                        weights[name] = (encodings[0].min, encodings[0].max)
        for name, ranges in weights.items():
            if isinstance(ranges, dict):
                _export_range_plot(ranges, min_max_ranges_dir, name)
        _export_range_plot({k: v for k, v in weights.items() if not isinstance(v, dict)}, min_max_ranges_dir, "weights")
        _export_range_plot(activations, min_max_ranges_dir, "activations")
        save_json(weights, min_max_ranges_dir, title="weights.json")
        save_json(activations, min_max_ranges_dir, title="activations.json")
        return weights, activations

    @staticmethod
    def _export_stats_histogram(quantizer, results_dir: str, title: str):
        """results_dir/{title}.json: {"{title}_{channel}": {xleft, pdf, min, max}} from get_stats_histogram()."""
        histograms = quantizer.get_stats_histogram()
        out = {}
        for index, (histogram, encoding) in enumerate(zip(histograms, _encodings_of(quantizer))):
            xleft, pdf = [b[0] for b in histogram], [b[1] for b in histogram]
            out[f"{title}_{index}"] = {"xleft": xleft, "pdf": pdf, "min": encoding.min, "max": encoding.max}
            _export_line_plot(xleft, pdf, results_dir, f"{title}_{index}", x_is_category=False)
        save_json(out, results_dir, title=title + ".json")

    def export_per_layer_stats_histogram(self, sim: QuantizationSimModel, results_dir: str):
        """
        NOTE: Not to invoke when quantization scheme is not TF-Enhanced.

        The histogram (PDF) of the statistics every quantizer with an encoding collected, one JSON
        file per quantizer:

        -results_dir
            -activations_pdf
                {name}_{input/output}_q{index}.json
            -weights_pdf
                -{name}
                    {name}_{param_name}.json

        :param sim: Quantsim model.
        :param results_dir: Directory to save the results.
        """
        weights_pdf_dir = os.path.join(results_dir, "weights_pdf")
        activations_pdf_dir = os.path.join(results_dir, "activations_pdf")
        name_of = {module: name for name, module in sim.model.named_modules()}
        for wrapper in _quantized_modules(sim):
            wrapped = name_of[wrapper]
            for kind, quantizers in (("input", wrapper.input_quantizers), ("output", wrapper.output_quantizers)):
                for index, quantizer in enumerate(quantizers):
                    if quantizer is not None and _encodings_of(quantizer):
                        self._export_stats_histogram(quantizer, activations_pdf_dir, f"{wrapped}_{kind}_q{index}")
            for param_name, quantizer in wrapper.param_quantizers.items():
                if quantizer is not None and _encodings_of(quantizer):
                    self._export_stats_histogram(quantizer, os.path.join(weights_pdf_dir, wrapped),
                                                 f"{wrapped}_{param_name}")

    # -- per-layer MSE ------------------------------------------------------------------------------
    def export_per_layer_mse_loss(self, sim: QuantizationSimModel, results_dir: str) -> Dict:
        """
        MSE between the fp32 and the quantized output activations of every leaf module, in execution
        order: for each layer the sum over the first num_batches batches of the batch MSE, divided by
        the number of samples (the reference's definition). Writes per_layer_mse_loss.json and
        per_layer_sqnr.json (10 log10(sum ref^2 / sum (ref - q)^2) in dB; "inf" for a zero error).

        Per batch: one forward of the fp32 model that keeps every listed module's output, one
        forward of the sim whose hooks reduce (fp32 output, quantized output) on the device and
        release the fp32 output. Nothing is read back before the end. Peak extra memory: one batch of
        the fp32 model's listed outputs.

        A kept output that an in-place successor (``ReLU(inplace=True)`` behind a conv) overwrites is
        found by its version counter after the fp32 forward; that forward is then run once more for
        the batch, with those layers' outputs cloned in the hook, as they are in every later batch.
        Only a module's first call in a forward counts. A layer whose output is not one float32 /
        float16 / bfloat16 tensor is left out, with one log line.

        :param sim: Quantsim model.
        :param results_dir: Directory to save the results.
        :return layer wise MSE loss. dict[layer_name] = MSE loss.
        """
        if not self._unlabeled_dataset_iterable:
            raise RuntimeError("per-layer MSE needs enable_per_layer_mse_loss() first")
        if not torch.cuda.is_available():
            raise RuntimeError("aimet_amd: per-layer MSE needs a HIP device; the MI355X core has no CPU path")
        results_dir = os.path.abspath(results_dir)
        os.makedirs(results_dir, exist_ok=True)

        in_sim = dict(sim.model.named_modules())
        dummy_input = _to_device(self._dummy_input, _device_of(self._model))
        modules = [(name, module) for name, module in get_ordered_list_of_modules(self._model, dummy_input)
                   if name in in_sim]
        row = {name: i for i, (name, _) in enumerate(modules)}
        device = next((p.device for p in sim.model.parameters() if p.is_cuda), None)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        table = torch.zeros(max(len(modules), 1), 2, dtype=torch.float64, device=device)
        samples = {name: 0 for name, _ in modules}
        skipped, to_clone = set(), set()
        kept: Dict[str, Tuple[torch.Tensor, int]] = {}
        seen_ref, seen_quant = set(), set()

        def skip(name, why):
            if name not in skipped:
                skipped.add(name)
                _logger.info("per-layer MSE: %s is left out (%s)", name, why)

        def ref_hook(name):
            def hook(_, __, out):
                if name in seen_ref or name in skipped:
                    return
                seen_ref.add(name)
                if not isinstance(out, torch.Tensor) or out.dtype not in _IO_DTYPES or out.dim() == 0:
                    skip(name, "its output is not one float32 / float16 / bfloat16 tensor")
                    return
                out = out.detach()
                if name in to_clone:
                    out = out.clone()
                kept[name] = (out, out._version)
            return hook

        def quant_hook(name):
            def hook(_, __, out):
                if name in seen_quant or name in skipped:
                    return
                seen_quant.add(name)
                ref = kept.pop(name, (None, 0))[0]
                if ref is None:
                    return
                if not isinstance(out, torch.Tensor) or out.dtype != ref.dtype or out.shape != ref.shape:
                    skip(name, "the sim's output does not match the fp32 model's")
                    return
                if out.numel() == 0:
                    return
                add_sq_err(ref.to(device).contiguous(), out.detach().to(device).contiguous(), 1.0 / out.numel(),
                           table[row[name]])
                samples[name] += out.size(0)
            return hook

        def forward(model, inputs, seen):
            seen.clear()
            with _eval_mode(model), torch.no_grad():
                default_forward_fn(model, _to_device(inputs, _device_of(model)))

        handles = [module.register_forward_hook(ref_hook(name)) for name, module in modules]
        handles += [in_sim[name].register_forward_hook(quant_hook(name)) for name, _ in modules]
        try:
            for batch_index, model_inputs in enumerate(self._unlabeled_dataset_iterable):
                if batch_index == self._num_batches:
                    break
                assert isinstance(model_inputs, (torch.Tensor, tuple, list))
                kept.clear()
                forward(self._model, model_inputs, seen_ref)
                overwritten = {name for name, (out, version) in kept.items() if out._version != version}
                if overwritten:
                    to_clone |= overwritten
                    kept.clear()
                    forward(self._model, model_inputs, seen_ref)
                forward(sim.model, model_inputs, seen_quant)
        finally:
            for h in handles:
                h.remove()
            kept.clear()

        sums = table.cpu().tolist()     # the one read-back
        mse_loss_dict, sqnr_dict = {}, {}
        for name, _ in modules:
            if name in skipped or not samples[name]:
                continue
            err, power = sums[row[name]]
            mse_loss_dict[name] = err / samples[name]
            sqnr_dict[name] = 10.0 * math.log10(power / err) if err > 0.0 and power > 0.0 else \
                (math.inf if err == 0.0 else -math.inf)

        _export_line_plot(list(mse_loss_dict), list(mse_loss_dict.values()), results_dir, "per_layer_mse_loss")
        save_json(mse_loss_dict, results_dir, title="per_layer_mse_loss.json")
        save_json(sqnr_dict, results_dir, title="per_layer_sqnr.json")
        return mse_loss_dict
