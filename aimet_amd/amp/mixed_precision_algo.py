"""The greedy mixed-precision algorithm (aimet_common/amp/mixed_precision_algo.py,
aimet_torch/amp/mixed_precision_algo.py) and its built-in SQNR eval callback.

* ``MixedPrecisionAlgoBase``: the algorithm on anything with quantizer groups, a ``compute_encodings``
  and an eval callback; needs no device. Phase 1 is the accuracy list (every group alone at every
  lower candidate, sorted by score), phase 2 the Pareto list (groups lowered cumulatively in that
  order, searched for the last point that meets ``fp32 - allowed_accuracy_drop``).
* ``GreedyMixedPrecisionAlgo``: the same on a ``QuantizationSimModel``, with the optimized phase 1.
* ``EvalCallbackFactory.sqnr``: the reference's ``_evaluate_sqnr`` with the per-batch ratio on the
  device (``aimet_amp_sqnr_add``, csrc/quant_analyzer.hip) and one read-back per evaluation; computed
  in double, so it differs from the reference's float32 expression by rounding only.

Limits: no ``supported_kernels`` configuration (every candidate counts as supported for every group;
``use_all_amp_candidates`` is accepted); phase 3 (convert-op reduction) is not built.
"""
import abc
import contextlib
import copy
import ctypes
import functools
import json
import logging
import math
import os
import pickle
import time
from collections import OrderedDict, defaultdict
from typing import Any, Callable, Dict, List, Tuple, Union

import torch

from aimet_amd import _native
from aimet_amd.activation_sampler import _device_of, _to_device, default_forward_fn
from aimet_amd.amp import utils as amp_utils
from aimet_amd.amp.quantizer_groups import QuantizerGroup, find_quantizer_group, find_supported_candidates
from aimet_amd.amp.utils import (AMPSearchAlgo, CandAttr, CandParam, binary_search, brute_force_search,
                                 calculate_starting_bit_ops, create_quant_group_to_candidate_dict, disable_quantizers,
                                 enable_quantizers, export_list, interpolation_search,
                                 modify_candidate_in_accuracy_list, sort_accuracy_list)
from aimet_amd.qc_quantize_op import QcQuantizeWrapper
from aimet_amd.quant_analyzer import CallbackFunc
from aimet_amd.quantizers import QuantizationDataType
from aimet_amd.quantsim import _eval_mode

_logger = logging.getLogger("aimet_amd.amp")

SQNR_EPS = 1e-4                 # the reference's _compute_sqnr
LAUNCHES_PER_BATCH = 2          # aimet_amp_sqnr_add: the partial sums and their fold
_IO_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}   # aimet_amp_sqnr_add's io_dtype


# ---------------------------------------------------------------------------------------------------
# the SQNR eval callback
# ---------------------------------------------------------------------------------------------------
def launch_count(reset: bool = False) -> int:
    """Kernel launches aimet_amp_sqnr_add has issued in this process."""
    n = ctypes.c_int64()
    _native.call("aimet_amp_launch_count", ctypes.byref(n), 1 if reset else 0)
    return n.value


def add_sqnr(ref: torch.Tensor, x: torch.Tensor, acc: torch.Tensor, eps: float = SQNR_EPS):
    """acc[0] += mean(ref^2) / (mean((ref - x)^2) + eps) (aimet_amp_sqnr_add): ref and x contiguous
    device tensors of one shape and dtype (float32 / float16 / bfloat16), acc one float64 on the
    same device."""
    if ref.shape != x.shape or ref.dtype != x.dtype or ref.dtype not in _IO_DTYPES:
        raise ValueError("SQNR: needs two float32 / float16 / bfloat16 tensors of one shape and dtype")
    if not (ref.is_cuda and x.is_cuda and acc.is_cuda) or not (ref.is_contiguous() and x.is_contiguous()):
        raise ValueError("SQNR: needs contiguous device tensors; the MI355X core has no CPU path")
    if acc.dtype != torch.float64 or acc.numel() != 1:
        raise ValueError("SQNR: the accumulator is one float64")
    with torch.cuda.device(ref.device):
        _native.call("aimet_amp_sqnr_add", ctypes.c_void_p(ref.data_ptr()), ctypes.c_void_p(x.data_ptr()), ref.numel(),
                     _IO_DTYPES[ref.dtype], float(eps), ctypes.c_void_p(acc.data_ptr()),
                     ctypes.c_void_p(torch.cuda.current_stream(ref.device).cuda_stream))


@contextlib.contextmanager
def _all_quantizers_disabled(model: torch.nn.Module):
    """Every enabled quantizer of every wrapper off for the duration."""
    quantizers = [q for m in model.modules() if isinstance(m, QcQuantizeWrapper)
                  for q in list(m.input_quantizers) + list(m.output_quantizers) + list(m.param_quantizers.values())
                  if q.enabled]
    disable_quantizers(quantizers)
    try:
        yield
    finally:
        enable_quantizers(quantizers)


def _staged(output, device) -> torch.Tensor:
    """A model output as the kernel takes it."""
    if not isinstance(output, torch.Tensor):
        raise ValueError("SQNR: the forward pass was expected to return a torch.Tensor, but returned %s; give "
                         "EvalCallbackFactory a forward_fn that adapts the output" % type(output))
    if output.dtype not in _IO_DTYPES:
        raise ValueError("SQNR: the model output is %s; float32, float16 and bfloat16 are supported" % output.dtype)
    return output.detach().to(device).contiguous()


class EvalCallbackFactory:
    """Built-in eval callbacks (aimet_torch/amp/mixed_precision_algo.py EvalCallbackFactory)."""

    _DEFAULT_SQNR_NUM_SAMPLES = 128

    def __init__(self, data_loader, forward_fn: Callable[[torch.nn.Module, Any], torch.Tensor] = None):
        """
        :param data_loader: Data loader (an iterable of batches; `batch_size` is read where it has one)
        :param forward_fn: Takes a model and one batch, returns the model's output tensor; default:
                ``model(batch)``, or ``model(*batch)`` for a tuple or list
        """
        self._data_loader = data_loader
        self._forward_fn = forward_fn or default_forward_fn
        self._batchwise_fp32_outputs_list = []      # captured by the first evaluation, reused afterwards
        self.stats = {"evaluations": 0, "fp32_forwards": 0, "batches": 0, "read_backs": 0}

    def sqnr(self, num_samples: int = _DEFAULT_SQNR_NUM_SAMPLES) -> CallbackFunc:
        """A callback that returns the SQNR, in dB, between the model's outputs with every quantizer
        disabled and its outputs as it is, over the first num_samples samples."""
        return CallbackFunc(functools.partial(self._evaluate_sqnr, num_samples=num_samples))

    def _evaluate_sqnr(self, model: torch.nn.Module, _: Any, num_samples: int) -> float:
        """10 log10(sum over batches of mean(fp32^2) / (mean((fp32 - quantized)^2) + 1e-4) / num_samples):
        batches are taken while i * batch_size < num_samples, and the sum is divided by num_samples,
        not by the number of samples seen (the reference's definition)."""
        if not torch.cuda.is_available():
            raise RuntimeError("aimet_amd: the SQNR callback needs a HIP device; the MI355X core has no CPU path")
        capture = not self._batchwise_fp32_outputs_list
        batch_size = getattr(self._data_loader, "batch_size", None) or 1
        device = _device_of(model)
        hip = device if device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        acc = torch.zeros(1, dtype=torch.float64, device=hip)
        self.stats["evaluations"] += 1
        with _eval_mode(model), torch.no_grad():
            for i, x in enumerate(self._data_loader):
                if i * batch_size >= num_samples:
                    break
                x = _to_device(x, device)
                if capture:
                    with _all_quantizers_disabled(model):
                        fp32_output = _staged(self._forward_fn(model, x), hip)
                    self._batchwise_fp32_outputs_list.append(fp32_output)
                    self.stats["fp32_forwards"] += 1
                else:
                    fp32_output = self._batchwise_fp32_outputs_list[i]
                quantized_output = _staged(self._forward_fn(model, x), hip)
                if quantized_output.shape != fp32_output.shape or quantized_output.dtype != fp32_output.dtype:
                    raise ValueError("SQNR: the output of batch %d is %s %s, the fp32 output was %s %s"
                                     % (i, quantized_output.dtype, tuple(quantized_output.shape), fp32_output.dtype,
                                        tuple(fp32_output.shape)))
                if quantized_output.numel() == 0:
                    raise ValueError("SQNR: the output of batch %d is empty" % i)
                add_sqnr(fp32_output, quantized_output, acc)
                self.stats["batches"] += 1
        total = self._read_back(acc)
        return 10.0 * math.log10(total / num_samples) if total > 0.0 else -math.inf

    def _read_back(self, acc: torch.Tensor) -> float:
        """The evaluation's one device-to-host copy."""
        self.stats["read_backs"] += 1
        return acc.cpu().item()


# ---------------------------------------------------------------------------------------------------
# the algorithm
# ---------------------------------------------------------------------------------------------------
class GreedyMixedPrecisionAlgoParams:
    """The callbacks and candidates of a run."""

    def __init__(self, candidates: List, forward_pass_callback: CallbackFunc, eval_callback_for_phase1: CallbackFunc,
                 eval_callback_for_phase2: CallbackFunc):
        self.candidates = candidates
        self.forward_pass_callback = forward_pass_callback.func
        self.forward_pass_callback_args = forward_pass_callback.args
        self.eval_callback_for_phase1 = eval_callback_for_phase1
        self.eval_callback_for_phase2 = eval_callback_for_phase2


class MixedPrecisionAlgoBase(abc.ABC):
    """The greedy algorithm on anything with quantizer groups: `sim` needs `compute_encodings(func,
    args)` and `model`; the groups, the reference's QuantizerGroup interface."""

    def __init__(self, sim, candidates: List, eval_callback_for_phase1: CallbackFunc,
                 eval_callback_for_phase2: CallbackFunc, forward_pass_callback: CallbackFunc, mac_dict: Dict,
                 results_dir: str, clean_start: bool, phase2_reverse: bool = False):
        """mac_dict: {module name: multiply-accumulates}; results_dir also holds the resume cache (.cache),
        which clean_start deletes; the other parameters as in the reference."""
        self._validate_inputs(candidates)
        self._sim = sim
        self.phase2_reverse = phase2_reverse
        self.time_taken_phase1 = None
        self.time_taken_phase2 = None
        self._results_dir = results_dir
        self._clean_start = clean_start
        self._module_name_dict, self.quantizer_groups = self._find_quantizer_group(sim)
        self.algo_params = GreedyMixedPrecisionAlgoParams(candidates, forward_pass_callback, eval_callback_for_phase1,
                                                          eval_callback_for_phase2)
        self._mac_dict = mac_dict
        self.fp32_accuracy = None
        self.baseline_candidate = None
        self.accuracy_list = None
        self.pareto_list = None
        self.min_accuracy = None
        self.min_candidate = None
        self._final_eval_score = None
        self._supported_candidates_per_quantizer_group, self._baseline_candidate_options = \
            find_supported_candidates(self.quantizer_groups, candidates)
        self._eval_scores = []                  # (score, candidate) of every baseline option
        self._candidate_mapping_dict = {}       # candidate -> {group: the candidate the group takes for it}

    @abc.abstractmethod
    def _find_quantizer_group(self, sim) -> Tuple[Dict, List]:
        """({name: what holds the quantizers of that name}, the quantizer groups)"""

    @property
    def baseline_candidate_options(self) -> List:
        """The candidates the baseline is chosen from."""
        return self._baseline_candidate_options

    # -- what a subclass may replace ----------------------------------------------------------------
    def _evaluate_model(self, eval_callback: CallbackFunc):
        return eval_callback.func(self._sim.model, eval_callback.args)

    def _find_bit_ops_reduction_for_acc_list(self, quantizer_group, max_candidate, candidate):
        return amp_utils.find_bit_ops_reduction(quantizer_group, self._mac_dict, max_candidate, candidate)

    def calculate_running_bit_ops(self, quantizer_group, module_bitwidth_dict: Dict, max_candidate, candidate,
                                  running_bit_ops):
        return amp_utils.calculate_running_bit_ops(self._mac_dict, quantizer_group, module_bitwidth_dict,
                                                   max_candidate, candidate, running_bit_ops)

    def _compute_encodings(self):
        self._sim.compute_encodings(self.algo_params.forward_pass_callback, self.algo_params.forward_pass_callback_args)

    def _compute_encodings_and_evaluate(self) -> float:
        self._compute_encodings()
        return self.evaluate_model(self.algo_params.eval_callback_for_phase2)

    # -- report -------------------------------------------------------------------------------------
    def __str__(self):
        if self.baseline_candidate is None:
            raise RuntimeError("Baseline bitwidth is not set. Call run() first.")
        pct_act, pct_param, pct_all, act_flipped, param_flipped, total_act, total_param, total = \
            self._count_and_get_quantizers_flipped()
        bar = "*" * 94 + "\n"
        rows = lambda flipped: "".join(f"{row}\n" for row in flipped)   # noqa: E731
        return ("\n" + bar + "Mixed Precision Statistics\n"
                f"Mixed precision model accuracy {self._final_eval_score}\n\n" + bar +
                f"\nActivation Quantizers flipped from baseline candidate - "
                f"{self.baseline_candidate[CandAttr.activation]}\n" + rows(act_flipped) +
                f"Percentage of Activation Quantizers flipped from baseline  {pct_act} \n" + bar +
                f"\nParameter Quantizers flipped from baseline candidate: - "
                f"{self.baseline_candidate[CandAttr.parameter]}\n" + rows(param_flipped) +
                f"Percentage of Parameter Quantizers flipped from baseline  {pct_param} \n" + bar +
                f"Percentage of all Quantizers flipped from baseline  {pct_all} \n" + bar +
                f"Total Number of activation quantizers are  {total_act} \n" + bar +
                f"Total Number of Param quantizers are  {total_param} \n" + bar +
                f"Total Number of quantizers are  {total} \n" + bar)

    def _count_and_get_quantizers_flipped(self):
        total_act, total_param = 0, 0
        act_flipped, param_flipped = [], []
        baseline = self.baseline_candidate
        for quantizer_group in self.quantizer_groups:
            candidate = quantizer_group.get_candidate(self._module_name_dict)
            for kind, module_name in quantizer_group.to_list():
                if kind in ("input", "output", "activation"):
                    total_act += 1
                    if tuple(candidate[CandAttr.activation]) != tuple(baseline[CandAttr.activation]):
                        act_flipped.append((kind, module_name, tuple(candidate[CandAttr.activation])))
                else:
                    total_param += 1
                    if tuple(candidate[CandAttr.parameter]) != tuple(baseline[CandAttr.parameter]):
                        param_flipped.append((kind, module_name, tuple(candidate[CandAttr.parameter])))

        def percentage(count, of):
            return (count * 100) / of if of else 0.0
        return (percentage(len(act_flipped), total_act), percentage(len(param_flipped), total_param),
                percentage(len(act_flipped) + len(param_flipped), total_act + total_param), act_flipped,
                param_flipped, total_act, total_param, total_act + total_param)

    def _export_amp_execution_info(self):
        pct_act, pct_param, pct_all, act_flipped, param_flipped, total_act, total_param, total = \
            self._count_and_get_quantizers_flipped()
        export_list([("fp32 accuray", self.fp32_accuracy), ("Phase1 Time", self.time_taken_phase1),
                     ("Phase2 Time", self.time_taken_phase2), ("final score", self._final_eval_score),
                     ("phase2 eval count", len(self.pareto_list)),
                     ("percentage_act_quantizers_flipped", pct_act),
                     ("percentage_param_quantizers_flipped", pct_param),
                     ("percentage_quantizers_flipped", pct_all),
                     ("count_act_quantizers_flipped", len(act_flipped)),
                     ("count_param_quantizers_flipped", len(param_flipped)),
                     ("total_act_quantizers", total_act), ("total_param_quantizers", total_param),
                     ("total_quantizers", total)], self._results_dir, "amp_info_list")

    # -- files --------------------------------------------------------------------------------------
    @staticmethod
    def _export_accuracy_list(accuracy_list, results_dir: str, file_name: str = "accuracy_list"):
        """.cache/{file_name}.pkl (what a later run resumes from) and .cache/{file_name}.json"""
        cache = os.path.join(results_dir, ".cache")
        os.makedirs(cache, exist_ok=True)
        rows = [(quantizer_group.to_list(), str(candidate), eval_score, bit_ops_reduction)
                for quantizer_group, candidate, eval_score, bit_ops_reduction in accuracy_list]
        with open(os.path.join(cache, file_name + ".pkl"), "wb") as f:
            pickle.dump(accuracy_list, f)
        with open(os.path.join(cache, file_name + ".json"), "w", encoding="utf-8") as f:
            json.dump(rows, f, indent=1)

    @staticmethod
    def _export_pareto_list(results_dir: str, pareto_front: List, file_name: str = "pareto_list"):
        """.cache/{file_name}.pkl, .cache/{file_name}.json and pareto_list.json"""
        cache = os.path.join(results_dir, ".cache")
        os.makedirs(cache, exist_ok=True)
        rows = [(bit_ops, score, quantizer_group.to_list(), str(candidate))
                for bit_ops, score, quantizer_group, candidate in pareto_front]
        with open(os.path.join(cache, file_name + ".pkl"), "wb") as f:
            pickle.dump(pareto_front, f)
        for path in (os.path.join(cache, file_name + ".json"), os.path.join(results_dir, "pareto_list.json")):
            with open(path, "w", encoding="utf-8") as f:
                json.dump(rows, f, indent=1)

    # -- baselines ----------------------------------------------------------------------------------
    @staticmethod
    def find_max_eval(eval_results: List[Tuple[float, Any]]) -> Tuple[float, Any]:
        """The (score, candidate) with the highest score; the first of equals."""
        best = 0
        for index, (score, _) in enumerate(eval_results):
            if score > eval_results[best][0]:
                best = index
        return eval_results[best]

    def _calc_baseline_fp32_accuracy(self) -> float:
        disabled = OrderedDict()
        for quantizer_group in self.quantizer_groups:
            quantizers = quantizer_group.get_active_quantizers(self._module_name_dict)
            disable_quantizers(quantizers)
            disabled[quantizer_group] = quantizers
        try:
            fp32_accuracy = self.evaluate_model(self.algo_params.eval_callback_for_phase2)
        finally:
            for quantizers in disabled.values():
                enable_quantizers(quantizers)
        _logger.info("Baseline FP32 accuracy: %f", fp32_accuracy)
        return fp32_accuracy

    def _valid_candidate(self, quantizer_group, candidate):
        """The candidate the group takes when the model is set to `candidate`."""
        supported = self._supported_candidates_per_quantizer_group[quantizer_group]
        if len(supported[0]) == 2 and candidate not in supported:
            return supported[0]
        if len(supported[0]) == 1:
            candidate = (candidate[0],)
            if candidate not in supported:
                return supported[0]
        return candidate

    def _get_best_candidate(self) -> Tuple[float, Any]:
        """(score, candidate) of the best baseline option; every option is scored once, in order."""
        if not self._eval_scores:
            _logger.info("Computing accuracy for maximum candidate")
            for candidate in self.baseline_candidate_options:
                mapping = {}
                for quantizer_group in self.quantizer_groups:
                    valid = self._valid_candidate(quantizer_group, candidate)
                    quantizer_group.set_quantizers_to_candidate(self._module_name_dict, valid)
                    mapping[quantizer_group] = valid
                eval_score = self._compute_encodings_and_evaluate()
                _logger.info("QuantSim accuracy with candidate %s : %f", candidate, eval_score)
                self._eval_scores.append((eval_score, candidate))
                self._candidate_mapping_dict[candidate] = copy.deepcopy(mapping)
        return self.find_max_eval(self._eval_scores)

    def _set_all_quantizer_groups_to_candidate(self, candidate):
        for quantizer_group in self.quantizer_groups:
            valid = self._candidate_mapping_dict.get(candidate, {}).get(quantizer_group, candidate)
            quantizer_group.set_quantizers_to_candidate(self._module_name_dict, valid)
        self._compute_encodings()

    def evaluate_model(self, eval_callback: CallbackFunc) -> float:
        """The callback's score as a float; RuntimeError when it cannot be one."""
        eval_score = self._evaluate_model(eval_callback)
        try:
            return float(eval_score)
        except TypeError as e:
            raise RuntimeError("eval_callback is expected to return float or a value that can be cast to float, "
                               "but returned {}.".format(type(eval_score))) from e

    def set_baseline(self, fp32_accuracy: float = None, baseline_candidate=None) -> Tuple[float, Any]:
        """Sets (and where not given, measures) the fp32 score and the baseline candidate, and sets
        every group to the baseline candidate."""
        if fp32_accuracy is None:
            fp32_accuracy = self._calc_baseline_fp32_accuracy()
        if baseline_candidate is None:
            _, baseline_candidate = self._get_best_candidate()
        self.fp32_accuracy = fp32_accuracy
        self.baseline_candidate = baseline_candidate
        if not self._candidate_mapping_dict:
            self._candidate_mapping_dict = {baseline_candidate: {g: baseline_candidate for g in self.quantizer_groups}}
        self._set_all_quantizer_groups_to_candidate(self.baseline_candidate)
        return self.fp32_accuracy, self.baseline_candidate

    def _choose_lowest_from_candidates(self) -> Tuple[float, Any]:
        """(score, candidate) with the fewest bit-ops among the scored baseline options; the better
        score among equals."""
        min_accuracy, min_candidate = self._eval_scores[0]
        min_bit_ops = calculate_starting_bit_ops(self._mac_dict, min_candidate)
        for accuracy, candidate in self._eval_scores:
            bit_ops = calculate_starting_bit_ops(self._mac_dict, candidate)
            if bit_ops < min_bit_ops or (bit_ops == min_bit_ops and accuracy > min_accuracy):
                min_bit_ops, min_accuracy, min_candidate = bit_ops, accuracy, candidate
        return min_accuracy, min_candidate

    # -- run ----------------------------------------------------------------------------------------
    def run(self, allowed_accuracy_drop: Union[None, float], search_algo: AMPSearchAlgo = AMPSearchAlgo.Binary):
        """
        :param allowed_accuracy_drop: Largest drop from the fp32 score; None builds the whole Pareto curve
        :param search_algo: The phase-2 search
        """
        searches = {AMPSearchAlgo.BruteForce: brute_force_search, AMPSearchAlgo.Interpolation: interpolation_search,
                    AMPSearchAlgo.Binary: binary_search}
        if search_algo not in searches:
            raise ValueError(f"Invalid search algo. Expected AMPSearchAlgo object, but got {search_algo}")
        search = searches[search_algo]

        if self.fp32_accuracy is None or self.baseline_candidate is None:
            self.set_baseline()
        if self.min_accuracy is None or self.min_candidate is None:
            if not self._eval_scores:
                self._get_best_candidate()
            self.min_accuracy, self.min_candidate = self._choose_lowest_from_candidates()

        if allowed_accuracy_drop is None:
            allowed_accuracy_drop = math.inf
        else:
            max_candidate_accuracy, _ = self._get_best_candidate()
            if self.fp32_accuracy - max_candidate_accuracy > allowed_accuracy_drop:
                _logger.info("The difference between baseline (%0.4f) and candidate with best accuracy (%0.4f) is"
                             " higher than the allowed accuracy drop (%0.4f)", self.fp32_accuracy,
                             max_candidate_accuracy, allowed_accuracy_drop)
                self._set_all_quantizer_groups_to_candidate(self.baseline_candidate)
                self._final_eval_score = max_candidate_accuracy
                return
            if self.fp32_accuracy - self.min_accuracy < allowed_accuracy_drop:
                self._set_all_quantizer_groups_to_candidate(self.min_candidate)
                self._final_eval_score = self.evaluate_model(self.algo_params.eval_callback_for_phase2)
                _logger.info("The difference between baseline (%0.4f) and candidate with the least accuracy (%0.4f) "
                             "is less than allowed accuracy drop (%0.4f). Early-exiting mixed precision algorithm.",
                             self.fp32_accuracy, self.min_accuracy, allowed_accuracy_drop)
                return

        start = time.time()
        self.accuracy_list = self._create_and_save_accuracy_list(self.baseline_candidate)
        self.time_taken_phase1 = (time.time() - start) / 60
        _logger.info("Time taken by phase1 is (%0.4f) mins", self.time_taken_phase1)

        start = time.time()
        self.pareto_list = self._create_pareto_front_list(allowed_accuracy_drop, self.accuracy_list,
                                                          self.fp32_accuracy, self.baseline_candidate,
                                                          self.min_candidate, search, self.phase2_reverse)
        self.time_taken_phase2 = (time.time() - start) / 60
        _logger.info("Time taken by phase2 is (%0.4f) mins", self.time_taken_phase2)
        self._export_amp_execution_info()

    def _load_cached_accuracy_list(self):
        """(accuracy list, {(group, candidate)} already in it) from .cache, or empty after clean_start."""
        file = os.path.join(self._results_dir, ".cache", "accuracy_list.pkl")
        if os.path.isfile(file):
            if self._clean_start:
                os.remove(file)
                _logger.info("Removed old cached files and restarting computation")
            else:
                with open(file, "rb") as f:
                    accuracy_list = pickle.load(f)
                return accuracy_list, {(group, candidate) for group, candidate, _, _ in accuracy_list}
        return [], set()

    def _create_and_save_accuracy_list(self, baseline_candidate) -> List:
        """Phase 1: [(group, candidate, score with only that group quantized, at that candidate,
        bit-ops reduction)], sorted."""
        index_of = {group: index for index, group in enumerate(self.quantizer_groups)}
        accuracy_list, done = self._load_cached_accuracy_list()
        disabled = OrderedDict()
        try:
            for quantizer_group in self.quantizer_groups:
                quantizers = quantizer_group.get_active_quantizers(self._module_name_dict)
                disable_quantizers(quantizers)
                disabled[quantizer_group] = quantizers
            for quantizer_group, candidates in self._supported_candidates_per_quantizer_group.items():
                quantizers = disabled[quantizer_group]
                try:
                    enable_quantizers(quantizers)
                    for candidate in candidates:
                        if candidate == baseline_candidate or (quantizer_group, candidate) in done:
                            continue
                        quantizer_group.set_quantizers_to_candidate(self._module_name_dict, candidate)
                        self._compute_encodings()
                        eval_score = self.evaluate_model(self.algo_params.eval_callback_for_phase1)
                        reduction = self._find_bit_ops_reduction_for_acc_list(quantizer_group, baseline_candidate,
                                                                              candidate)
                        accuracy_list.append((quantizer_group, candidate, eval_score, reduction))
                        accuracy_list = sort_accuracy_list(accuracy_list, index_of)
                        self._export_accuracy_list(accuracy_list, self._results_dir)
                        _logger.info("Quantizer: %s candidate: %s eval_score: %f", quantizer_group, candidate,
                                     eval_score)
                finally:
                    valid = self._candidate_mapping_dict.get(baseline_candidate, {}).get(quantizer_group,
                                                                                         baseline_candidate)
                    quantizer_group.set_quantizers_to_candidate(self._module_name_dict, valid)
                    disable_quantizers(quantizers)
        finally:
            for quantizers in disabled.values():
                enable_quantizers(quantizers)
        _logger.info("Completed Accuracy list computation")
        self._compute_encodings()
        return accuracy_list

    def _create_pareto_front_list(self, allowed_accuracy_drop: float, accuracy_list: List, fp32_accuracy: float,
                                  baseline_candidate, lowest_candidate, search_algo: Callable,
                                  phase2_reverse: bool) -> List:
        """Phase 2: [(bit-ops relative to the start, score, group, candidate)]; entry i is the model
        with the first i + 1 accuracy-list entries applied. Leaves the sim at the last entry that meets
        fp32_accuracy - allowed_accuracy_drop (the baseline candidate if none does)."""
        if phase2_reverse:
            starting_candidate = lowest_candidate
            accuracy_list.reverse()
            self._export_accuracy_list(accuracy_list, self._results_dir, "accuracy_list_reverse")
            order = create_quant_group_to_candidate_dict(accuracy_list)
            accuracy_list = modify_candidate_in_accuracy_list(accuracy_list, order, baseline_candidate)
            self._export_accuracy_list(accuracy_list, self._results_dir, "accuracy_list_reverse_modified")
        else:
            starting_candidate = baseline_candidate

        self._set_all_quantizer_groups_to_candidate(starting_candidate)
        pareto_front = [None for _ in accuracy_list]
        file_path = os.path.join(self._results_dir, ".cache", "pareto_list.pkl")
        if os.path.isfile(file_path):
            if self._clean_start:
                os.remove(file_path)
                _logger.info("Removed old pareto list pickled file and restarting computation")
            else:
                with open(file_path, "rb") as f:
                    cached = pickle.load(f)
                for relative_bit_ops, eval_score, quantizer_group, candidate in cached:
                    for i, (group_i, candidate_i, _, _) in enumerate(accuracy_list):
                        if group_i == quantizer_group and candidate_i == candidate:
                            pareto_front[i] = (relative_bit_ops, eval_score, quantizer_group, candidate)

        starting_bit_ops = calculate_starting_bit_ops(self._mac_dict, starting_candidate)

        def evaluate_pareto_point(i: int) -> float:
            if pareto_front[i] is not None:
                return pareto_front[i][1]
            module_bitwidth_dict = {}
            bit_ops = starting_bit_ops
            for quantizer_group, candidate, _, _ in accuracy_list[:i + 1]:
                quantizer_group.set_quantizers_to_candidate(self._module_name_dict, candidate)
                bit_ops = self.calculate_running_bit_ops(quantizer_group, module_bitwidth_dict, starting_candidate,
                                                         candidate, bit_ops)
            relative_bit_ops = bit_ops / starting_bit_ops
            try:
                eval_score = self._compute_encodings_and_evaluate()
            finally:
                for quantizer_group, _, _, _ in accuracy_list[:i + 1]:
                    quantizer_group.set_quantizers_to_candidate(self._module_name_dict, starting_candidate)
            quantizer_group, candidate, _, _ = accuracy_list[i]
            pareto_front[i] = (relative_bit_ops, eval_score, quantizer_group, candidate)
            _logger.info("Quantizer group: %s candidate: %s eval_score: %f Relative BitOps %f", quantizer_group,
                         candidate, eval_score, relative_bit_ops)
            self._export_pareto_list(self._results_dir, [x for x in pareto_front if x is not None])
            return eval_score

        values = [functools.partial(evaluate_pareto_point, i) for i in range(len(accuracy_list))]
        target_accuracy = fp32_accuracy - allowed_accuracy_drop
        i = search_algo(values, target_accuracy, phase2_reverse)

        if i == 0 and pareto_front[i][1] < target_accuracy and not phase2_reverse:
            pass        # no entry meets the target: the baseline candidate stays
        elif i == len(values) - 1 and pareto_front[i][1] < target_accuracy and phase2_reverse:
            self._set_all_quantizer_groups_to_candidate(baseline_candidate)
        else:
            for quantizer_group, candidate, _, _ in accuracy_list[:i + 1]:
                quantizer_group.set_quantizers_to_candidate(self._module_name_dict, candidate)
        _logger.info("Completed Pareto list computation")
        self._final_eval_score = self._compute_encodings_and_evaluate()
        _logger.info("AMP phase-2 final accuracy:%f", self._final_eval_score)
        return [x for x in pareto_front if x is not None]

    @staticmethod
    def _validate_inputs(candidates: List):
        for candidate in candidates:
            (act_bw, act_data_type), (param_bw, param_data_type) = candidate
            assert isinstance(act_bw, int), "candidate's activation bitwidth is expected to be of type int"
            assert isinstance(act_data_type, QuantizationDataType), \
                "candidate's activation data type is expected to be of type QuantizationDataType"
            assert isinstance(param_bw, int), "candidate's param bitwidth is expected to be of type int"
            assert isinstance(param_data_type, QuantizationDataType), \
                "candidate's param data type is expected to be of type QuantizationDataType"


class GreedyMixedPrecisionAlgo(MixedPrecisionAlgoBase):
    """The greedy algorithm on a QuantizationSimModel."""

    def __init__(self, sim, dummy_input: Union[torch.Tensor, Tuple], candidates: List,
                 eval_callback_for_phase1: CallbackFunc, eval_callback_for_phase2: CallbackFunc, results_dir: str,
                 clean_start: bool, forward_pass_callback: CallbackFunc, use_all_amp_candidates: bool = False,
                 phase2_reverse: bool = False, phase1_optimize: bool = False):
        """phase1_optimize: one compute_encodings per candidate in phase 1 instead of one per (group,
        candidate). use_all_amp_candidates is accepted and changes nothing (no `supported_kernels`)."""
        mac_dict = amp_utils.create_mac_dict(sim.model, dummy_input)
        self.phase1_optimize = phase1_optimize
        self.use_all_amp_candidates = use_all_amp_candidates
        self.dummy_input = dummy_input
        super().__init__(sim, candidates, eval_callback_for_phase1, eval_callback_for_phase2, forward_pass_callback,
                         mac_dict, results_dir, clean_start, phase2_reverse)

    def _find_quantizer_group(self, sim) -> Tuple[Dict, List[QuantizerGroup]]:
        return find_quantizer_group(sim)

    def _create_and_save_accuracy_list(self, baseline_candidate):
        if self.phase1_optimize:
            return self._create_and_save_accuracy_list_optimized(baseline_candidate)
        return super()._create_and_save_accuracy_list(baseline_candidate)

    def _create_and_save_accuracy_list_optimized(self, baseline_candidate) -> List:
        """Phase 1 with one compute_encodings per candidate: every group is set to the candidate and
        enabled, encodings are computed with the parameter quantizers off (an activation then sees
        what it sees when its group alone is quantized, up to the other groups' activation
        quantizers; the parameter encodings do not depend on the forward), and each group is then
        scored with only that group enabled."""
        index_of = {group: index for index, group in enumerate(self.quantizer_groups)}
        accuracy_list, done = self._load_cached_accuracy_list()
        disabled = OrderedDict()
        try:
            for quantizer_group in self.quantizer_groups:
                quantizers = quantizer_group.get_active_quantizers(self._module_name_dict)
                disable_quantizers(quantizers)
                disabled[quantizer_group] = quantizers

            groups_of = defaultdict(list)
            for quantizer_group, candidates in self._supported_candidates_per_quantizer_group.items():
                for candidate in candidates:
                    groups_of[candidate].append(quantizer_group)

            for candidate, quantizer_groups in groups_of.items():
                if candidate == baseline_candidate:
                    continue
                for quantizer_group in quantizer_groups:
                    enable_quantizers(disabled[quantizer_group])
                    quantizer_group.set_quantizers_to_candidate(self._module_name_dict, candidate)
                param_quantizers = [q for _, wrapper in self._sim.quant_wrappers()
                                    for q in wrapper.param_quantizers.values() if q.enabled]
                disable_quantizers(param_quantizers)
                try:
                    self._compute_encodings()
                finally:
                    enable_quantizers(param_quantizers)
                for quantizer_group in quantizer_groups:
                    quantizers = quantizer_group.get_active_quantizers(self._module_name_dict)
                    disable_quantizers(quantizers)
                    disabled[quantizer_group] = quantizers
                for quantizer_group in quantizer_groups:
                    if (quantizer_group, candidate) in done:
                        continue
                    quantizers = disabled[quantizer_group]
                    try:
                        enable_quantizers(quantizers)
                        eval_score = self.evaluate_model(self.algo_params.eval_callback_for_phase1)
                        reduction = self._find_bit_ops_reduction_for_acc_list(quantizer_group, baseline_candidate,
                                                                              candidate)
                        accuracy_list.append((quantizer_group, candidate, eval_score, reduction))
                        accuracy_list = sort_accuracy_list(accuracy_list, index_of)
                        self._export_accuracy_list(accuracy_list, self._results_dir)
                        _logger.info("Quantizer: %s candidate: %s eval_score: %f", quantizer_group, candidate,
                                     eval_score)
                    finally:
                        disable_quantizers(quantizers)
        finally:
            for quantizer_group in self.quantizer_groups:
                enable_quantizers(disabled.get(quantizer_group, ()))
                quantizer_group.set_quantizers_to_candidate(self._module_name_dict, baseline_candidate)
        _logger.info("Completed Accuracy list computation")
        self._compute_encodings()
        return accuracy_list

    def set_quantizer_groups_candidates(self, quantizer_group_candidates: List[Tuple]) -> None:
        """Sets each (group, candidate) and computes encodings; a candidate the group does not support
        is an AssertionError."""
        def supported(quantizer_group, candidate) -> bool:
            candidates = self._supported_candidates_per_quantizer_group.get(quantizer_group) or []
            if not quantizer_group.parameter_quantizers:
                return any(c[0] == tuple(candidate[0]) for c in candidates)
            return candidate in candidates

        for quantizer_group, candidate in quantizer_group_candidates:
            assert supported(quantizer_group, candidate), \
                "candidate %s is not supported by %s" % (candidate, quantizer_group)
            quantizer_group.set_quantizers_to_candidate(self._module_name_dict, candidate)
        self._compute_encodings()
