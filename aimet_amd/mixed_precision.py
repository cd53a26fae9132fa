"""Automatic mixed precision (aimet_torch/mixed_precision.py): choose, per quantizer group, the lowest
candidate bitwidths that keep the model within an allowed drop of its fp32 score.

    from aimet_amd.mixed_precision import choose_mixed_precision
    from aimet_amd.amp.mixed_precision_algo import EvalCallbackFactory
    from aimet_amd.quant_analyzer import CallbackFunc
    from aimet_amd.quantizers import QuantizationDataType as T

    candidates = [((16, T.int), (16, T.int)), ((16, T.int), (8, T.int)), ((8, T.int), (8, T.int))]
    sqnr = EvalCallbackFactory(data_loader).sqnr(num_samples=128)
    pareto = choose_mixed_precision(sim, dummy_input, candidates, sqnr, sqnr, allowed_accuracy_drop=3.0,
                                    results_dir="./amp", clean_start=True,
                                    forward_pass_callback=CallbackFunc(calibrate, None))

The algorithm and its limits: aimet_amd/amp/mixed_precision_algo.py.
"""
import logging
from typing import List, Tuple, Union

import torch

from aimet_amd.amp.mixed_precision_algo import GreedyMixedPrecisionAlgo
from aimet_amd.amp.quantizer_groups import QuantizerGroup
from aimet_amd.amp.utils import (AMPSearchAlgo, visualize_pareto_curve,  # noqa: F401
                                 visualize_quantizer_group_sensitivity)
from aimet_amd.quant_analyzer import CallbackFunc
from aimet_amd.quantsim import QuantizationSimModel

_logger = logging.getLogger("aimet_amd.amp")


def choose_mixed_precision(sim: QuantizationSimModel, dummy_input: Union[torch.Tensor, Tuple], candidates: List,
                           eval_callback_for_phase1: CallbackFunc, eval_callback_for_phase2: CallbackFunc,
                           allowed_accuracy_drop: Union[None, float], results_dir: str, clean_start: bool,
                           forward_pass_callback: CallbackFunc, use_all_amp_candidates: bool = False,
                           phase2_reverse: bool = False, phase1_optimize: bool = True,
                           amp_search_algo: AMPSearchAlgo = AMPSearchAlgo.Binary) -> \
        Union[List[Tuple[float, float, QuantizerGroup, tuple]], None]:
    """
    Mixed precision in place on the given sim: builds the Pareto list of (relative bit-ops, eval score),
    saves it under results_dir and leaves the sim at its lowest-cost point that meets the allowed drop.
    Parameters as in the reference (aimet_torch/mixed_precision.py) and MixedPrecisionAlgoBase.
    `use_all_amp_candidates` is accepted: the sim carries no `supported_kernels`, so every candidate
    counts as supported for every group.

    :return: [(relative bit-ops, eval score, quantizer group, candidate)]; None when the algorithm exits
            early (the best candidate already misses the allowed drop, or the lowest one meets it)
    """
    algo = GreedyMixedPrecisionAlgo(sim, dummy_input, candidates, eval_callback_for_phase1, eval_callback_for_phase2,
                                    results_dir, clean_start, forward_pass_callback, use_all_amp_candidates,
                                    phase2_reverse, phase1_optimize)
    algo.run(allowed_accuracy_drop, amp_search_algo)
    if algo.accuracy_list is not None and algo.pareto_list is not None:
        _logger.info(algo)
        visualize_quantizer_group_sensitivity(algo.accuracy_list, algo.baseline_candidate, algo.fp32_accuracy,
                                              results_dir=results_dir)
        visualize_pareto_curve(algo.pareto_list, results_dir)
        return algo.pareto_list
    return None
