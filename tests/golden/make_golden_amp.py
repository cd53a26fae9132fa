"""Generate tests/golden/golden_amp.json: automatic mixed precision against the reference.

The reference's helpers and searches (aimet_common/amp/utils.py), its base algorithm
(aimet_common/amp/mixed_precision_algo.py GreedyMixedPrecisionAlgo), its QuantizerGroup
(aimet_torch/amp/quantizer_groups.py), its bit-ops bookkeeping (aimet_torch/amp/utils.py) and its SQNR
callback (aimet_torch/amp/mixed_precision_algo.py _evaluate_sqnr, _compute_sqnr) are parsed from the
reference files with `ast` and executed at generation time, with stand-ins for what they import
(bokeh, pandas, the logger, the sim and its quantizers). Nothing of their text is stored; the fixture
holds data only:

(a) helpers: the accuracy-list order with ties on score, bitwidth sum and bit-ops; effective
    bitwidths; starting, running and reduction bit-ops for int and float candidates and for groups
    with and without parameters; the reverse-list rewrite;
(b) searches: the three searches on descending, ascending and non-monotone scores: the index
    returned and every index evaluated, in order;
(c) runs: the base algorithm on six stand-in groups, three candidates and a table-driven score
    (a deterministic function of every group's current candidate and of which quantizers are on;
    every term is a multiple of 1/64, so sums are exact in any order), for every search x
    phase2_reverse x four allowed drops;
(d) sqnr: _evaluate_sqnr on the CPU in float32 for small recorded outputs.

    python tests/golden/make_golden_amp.py
"""
import abc
import ast
import contextlib
import copy
import enum
import functools
import io
import itertools
import json
import logging
import math
import os
import pickle
import sys
import tempfile
import time
import types
from collections import OrderedDict, defaultdict, deque
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Sequence, Set, Tuple, Union

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("AIMET_REFERENCE", "/root/reference")
COMMON = "TrainingExtensions/common/src/python/aimet_common/amp/"
TORCH = "TrainingExtensions/torch/src/python/aimet_torch/amp/"
OUT = os.path.join(HERE, "golden_amp.json")


class QuantizationDataType(enum.Enum):
    undefined = 0
    int = 1
    float = 2


class CallbackFunc:
    def __init__(self, func, func_callback_args=None):
        self.func, self.args = func, func_callback_args


TYPING = {"Any": Any, "Callable": Callable, "Dict": Dict, "List": List, "Optional": Optional, "Sequence": Sequence,
          "Set": Set, "Tuple": Tuple, "Union": Union}


def run_reference(rel_path, ns, only=None):
    """Execute the reference file's definitions (no imports, no logger) in ns; `only`: just these names."""
    path = os.path.join(REF_ROOT, rel_path)
    tree = ast.parse(open(path).read(), path)
    body = []
    for n in tree.body:
        if isinstance(n, (ast.Import, ast.ImportFrom)):
            continue
        if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "logger":
            continue
        if only is not None and getattr(n, "name", None) not in only:
            continue
        body.append(n)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def reference_namespace():
    log = logging.getLogger("golden_amp")
    log.addHandler(logging.NullHandler())
    log.propagate = False
    ns = dict(TYPING)
    ns.update({"IntEnum": enum.IntEnum, "math": math, "os": os, "json": json, "np": np, "torch": torch,
               "QuantizationDataType": QuantizationDataType, "logger": log, "CallbackFunc": CallbackFunc,
               # plots are not generated: the names only have to exist where annotations name them
               "figure": object, "ColumnDataSource": None, "output_file": None, "save": None, "HoverTool": None,
               "factor_cmap": None, "color_groups": None, "pd": None,
               "abc": abc, "copy": copy, "io": io, "time": time, "pickle": pickle, "functools": functools,
               "itertools": itertools, "defaultdict": defaultdict, "OrderedDict": OrderedDict, "deque": deque,
               "dataclass": dataclass, "field": field})
    run_reference(COMMON + "utils.py", ns)
    run_reference(COMMON + "quantizer_groups.py", ns, only={"QuantizerGroupBase"})
    run_reference(COMMON + "mixed_precision_algo.py", ns)
    ns["MixedPrecisionAlgo"] = ns["GreedyMixedPrecisionAlgo"]
    run_reference(TORCH + "quantizer_groups.py", ns, only={"QuantizerGroup"})
    # the algorithm pickles its lists: the class has to be found by name in a module
    ns["QuantizerGroup"].__module__ = __name__
    globals()["QuantizerGroup"] = ns["QuantizerGroup"]
    run_reference(TORCH + "utils.py", ns, only={"find_bit_ops_reduction", "create_quantizer_module_dict",
                                                "calculate_running_bit_ops"})
    return ns


# ---------------------------------------------------------------------------------------------------
# stand-ins (tests/test_amp.py builds the same from the fixture's "model" section)
# ---------------------------------------------------------------------------------------------------
I, Fl = QuantizationDataType.int, QuantizationDataType.float
C16_16, C16_8, C8_8 = ((16, I), (16, I)), ((16, I), (8, I)), ((8, I), (8, I))
CANDIDATES = [C16_16, C16_8, C8_8]
MODEL = {
    # module: MACs, number of input quantizers (enabled), output quantizer enabled
    "modules": {"m0": {"macs": 1200, "inputs": 1, "output": True, "param": True},
                "m1": {"macs": 4000, "inputs": 0, "output": True, "param": True},
                "m2": {"macs": 2500, "inputs": 0, "output": True, "param": True},
                "m3": {"macs": 0, "inputs": 1, "output": True, "param": False},
                "m4": {"macs": 3000, "inputs": 0, "output": False, "param": True},
                "m5": {"macs": 700, "inputs": 0, "output": True, "param": True}},
    "groups": [{"input": ["m0_input_quantizer_idx_0"], "output": [], "weight": ["m0"]},
               {"input": [], "output": ["m0"], "weight": ["m1"]},
               {"input": [], "output": ["m1"], "weight": ["m2"]},
               {"input": ["m3_input_quantizer_idx_0"], "output": ["m2"], "weight": []},
               {"input": [], "output": ["m3"], "weight": ["m4", "m5"]},
               {"input": [], "output": ["m5"], "weight": []}],
    # score = base - sum over groups with an enabled quantizer of
    #         (act[g] * cost[activation bitwidth] + par[g] * cost[parameter bitwidth]) / 64
    "base": 80.0,
    "act": [40, 12, 96, 8, 64, 24],
    "par": [16, 72, 4, 0, 48, 0],
    "cost": {"16": 1, "8": 16, "4": 64},
}


class StubQuantizer:
    def __init__(self, enabled=True):
        self.enabled, self.bitwidth, self.data_type = enabled, 8, I


class StubWrapper:
    def __init__(self, spec):
        self.input_quantizers = [StubQuantizer() for _ in range(spec["inputs"])]
        self.output_quantizers = [StubQuantizer(spec["output"])]
        self.param_quantizers = {"weight": StubQuantizer()} if spec["param"] else {}


class StubSim:
    def __init__(self):
        self.model = object()
        self.encodings_computed = 0

    def compute_encodings(self, callback, args):
        self.encodings_computed += 1


def make_groups(ns):
    return [ns["QuantizerGroup"](input_quantizers=tuple(g["input"]), output_quantizers=tuple(g["output"]),
                                 parameter_quantizers=tuple(g["weight"])) for g in MODEL["groups"]]


def score_of(groups, wrappers):
    total = MODEL["base"]
    for g, group in enumerate(groups):
        if not group.get_active_quantizers(wrappers):
            continue
        (act_bw, _), (par_bw, _) = group.get_candidate(wrappers)
        total -= MODEL["act"][g] * MODEL["cost"][str(act_bw)] / 64
        if par_bw is not None:
            total -= MODEL["par"][g] * MODEL["cost"][str(par_bw)] / 64
    return total


def cand_json(c):
    return None if c is None else [[bw, None if dt is None else dt.name] for bw, dt in c]


# ---------------------------------------------------------------------------------------------------
def helpers_section(ns):
    groups = make_groups(ns)
    mac_dict = {name: spec["macs"] for name, spec in MODEL["modules"].items() if spec["macs"]}
    cands = {"i16_16": C16_16, "i16_8": C16_8, "i8_8": C8_8, "i8_4": ((8, I), (4, I)),
             "f16_16": ((16, Fl), (16, Fl)), "f16_i8": ((16, Fl), (8, I)), "f8_8": ((8, Fl), (8, Fl)),
             "a16": ((16, I),), "a8": ((8, I),), "af16": ((16, Fl),)}
    out = {"candidates": {k: cand_json(v) for k, v in cands.items()}}
    out["effective"] = [[dt.name, bw, ns["get_effective_bitwidth"](dt, bw)] for dt in (I, Fl) for bw in (4, 8, 16)]
    out["starting"] = {k: ns["calculate_starting_bit_ops"](mac_dict, c) for k, c in cands.items()}
    pairs = [("i16_16", "i16_8"), ("i16_16", "i8_8"), ("i16_16", "i8_4"), ("f16_16", "i8_8"), ("f16_16", "f8_8"),
             ("f16_16", "f16_i8"), ("i16_16", "f8_8"), ("a16", "a8"), ("af16", "a8"), ("i16_16", "a8")]
    out["reduction"] = [[g, hi, lo, ns["find_bit_ops_reduction"](groups[g], mac_dict, cands[hi], cands[lo])]
                        for hi, lo in pairs for g in range(len(groups))]
    # running bit-ops along a walk over the groups (the dict of module bitwidths is carried along)
    walks = {"int": ("i16_16", [(1, "i16_8"), (2, "i8_8"), (1, "i8_8"), (4, "i8_4"), (3, "i8_8"), (0, "i8_8"),
                                (5, "i16_8")]),
             "float": ("f16_16", [(4, "f8_8"), (0, "i8_8"), (1, "f16_i8"), (3, "f8_8"), (2, "i8_8")]),
             "act_only": ("a16", [(3, "a8"), (1, "a8"), (0, "a8"), (4, "a8")])}
    out["running"] = {}
    for name, (start, steps) in walks.items():
        total, seen, trace = ns["calculate_starting_bit_ops"](mac_dict, cands[start]), {}, []
        for g, c in steps:
            total = ns["calculate_running_bit_ops"](mac_dict, groups[g], seen, cands[start], cands[c], total)
            trace.append([g, c, total])
        out["running"][name] = {"start": start, "steps": trace}
    # the order: ties on score, then on the bitwidth sum, then on bit-ops, then on the group's place
    entries = [(0, "i8_8", 70.5, 100), (1, "i8_8", 70.5, 100), (2, "i16_8", 70.5, 100), (3, "i16_8", 70.5, 300),
               (4, "i8_8", 71.0, 5), (5, "a8", 70.5, 100), (0, "i16_8", 12.0, 900), (1, "f8_8", 70.5, 100.5),
               (2, "i8_4", 70.5, 100), (3, "a16", 70.5, 100)]
    index_of = {g: i for i, g in enumerate(groups)}
    acc = [(groups[g], cands[c], s, b) for g, c, s, b in entries]
    out["sort"] = {"entries": [list(e) for e in entries],
                   "order": [acc.index(e) for e in ns["sort_accuracy_list"](acc, index_of)]}
    # the phase2_reverse rewrite
    listed = [(0, "i8_8"), (1, "i16_8"), (0, "i16_8"), (2, "i8_8"), (1, "i8_8"), (2, "i16_8"), (3, "i8_8")]
    rev = [(groups[g], cands[c], float(10 + k), k) for k, (g, c) in enumerate(listed)]
    order = ns["create_quant_group_to_candidate_dict"](rev)
    out["reverse"] = {"entries": [[g, c] for g, c in listed],
                      "order": [[index_of[g], [cand_json(c) for c in cs]] for g, cs in order.items()],
                      "modified": [[index_of[g], cand_json(c), s, b] for g, c, s, b in
                                   ns["modify_candidate_in_accuracy_list"](rev, order, cands["i16_16"])]}
    return out


def searches_section(ns):
    lists = {"descending": [9.0, 8.5, 8.5, 7.0, 5.5, 5.0, 2.0, 1.5, 1.0],
             "ascending": [1.0, 1.5, 2.0, 5.0, 5.5, 7.0, 8.5, 8.5, 9.0],
             "non_monotone": [9.0, 6.0, 7.5, 7.0, 3.0, 4.5, 4.0, 1.0, 2.0], "one": [2.0]}
    targets = [-math.inf, 0.5, 1.75, 5.5, 8.5, 9.5]
    cases = []
    for name, vals in lists.items():
        for algo in ("brute_force_search", "interpolation_search", "binary_search"):
            for reverse in (False, True):
                for target in targets:
                    visited = []
                    values = [functools.partial(lambda i: (visited.append(i), vals[i])[1], i) for i in range(len(vals))]
                    try:
                        index = ns[algo](values, target, reverse)
                    except ZeroDivisionError:
                        index = "ZeroDivisionError"
                    cases.append([name, algo, reverse, "-inf" if target == -math.inf else target, index, visited])
    return {"lists": lists, "columns": ["list", "algo", "reverse", "target", "index", "visited"], "cases": cases}


def runs_section(ns):
    base_cls = ns["MixedPrecisionAlgo"]

    class Algo(base_cls):
        def __init__(self, sim, wrappers, groups, *args):
            self._given = (wrappers, groups)
            super().__init__(sim, *args)
            self._supported_candidates_per_quantizer_group = defaultdict(list)
            for g in groups:
                self._supported_candidates_per_quantizer_group[g] = CANDIDATES

        def _find_quantizer_group(self, sim):
            return self._given

        @property
        def baseline_candidate_options(self):
            return CANDIDATES

        def _evaluate_model(self, eval_callback):
            return eval_callback.func(self._sim.model, eval_callback.args)

        def _find_bit_ops_reduction_for_acc_list(self, quantizer_group, max_candidate, candidate):
            return ns["find_bit_ops_reduction"](quantizer_group, self._mac_dict, max_candidate, candidate)

        def calculate_running_bit_ops(self, quantizer_group, module_bitwidth_dict, max_candidate, candidate,
                                      running_bit_ops):
            return ns["calculate_running_bit_ops"](self._mac_dict, quantizer_group, module_bitwidth_dict,
                                                   max_candidate, candidate, running_bit_ops)

        def _create_op_graph(self, sim):
            return None

        def _optimize_mp_profile_and_evaluate_model(self):
            self._sim.compute_encodings(self.algo_params.forward_pass_callback,
                                        self.algo_params.forward_pass_callback_args)
            return self.evaluate_model(self.algo_params.eval_callback_for_phase2)

        def _reduce_mp_convert_ops(self):
            pass

    def fresh():
        wrappers = {name: StubWrapper(spec) for name, spec in MODEL["modules"].items()}
        return wrappers, make_groups(ns)

    wrappers, groups = fresh()
    fp32 = MODEL["base"]
    at = {}
    for c in CANDIDATES:
        for g in groups:
            g.set_quantizers_to_candidate(wrappers, c)
        at[c] = score_of(groups, wrappers)
    best_drop, lowest_drop = fp32 - max(at.values()), fp32 - at[C8_8]
    drops = {"none": None, "midway": (best_drop + lowest_drop) / 2, "below_best": best_drop / 2,
             "above_lowest": lowest_drop + 1.0}
    mac_dict = {name: spec["macs"] for name, spec in MODEL["modules"].items() if spec["macs"]}
    runs, forward_lists = [], []

    def acc_list(algo, index_of, seen):
        """None, "forward" or "reversed" (phase2_reverse reverses it in place); the list itself goes to `seen`"""
        if algo.accuracy_list is None:
            return None
        rows = [[index_of[g], CANDIDATES.index(c), s, b] for g, c, s, b in algo.accuracy_list]
        if algo.phase2_reverse:
            rows.reverse()
        if rows not in seen:
            seen.append(rows)
        return "reversed" if algo.phase2_reverse else "forward"
    for algo_name in ("BruteForce", "Interpolation", "Binary"):
        for reverse in (False, True):
            for drop_name, drop in drops.items():
                wrappers, groups = fresh()
                index_of = {g: i for i, g in enumerate(groups)}
                sim, calls = StubSim(), [0]

                def score(model, args):
                    calls[0] += 1
                    return score_of(groups, wrappers)
                cb = CallbackFunc(score, None)
                with tempfile.TemporaryDirectory() as tmp:
                    algo = Algo(sim, wrappers, groups, CANDIDATES, cb, cb, CallbackFunc(lambda m, a: None, None),
                                mac_dict, tmp, True, reverse)
                    algo.run(drop, ns["AMPSearchAlgo"][algo_name])
                runs.append({
                    "algo": algo_name, "reverse": reverse, "drop_name": drop_name, "drop": drop,
                    "fp32_accuracy": algo.fp32_accuracy, "baseline_candidate": cand_json(algo.baseline_candidate),
                    "min_candidate": cand_json(algo.min_candidate), "min_accuracy": algo.min_accuracy,
                    "accuracy_list": acc_list(algo, index_of, forward_lists),
                    "pareto_list": None if algo.pareto_list is None else
                    [[b, s, index_of[g], CANDIDATES.index(c)] for b, s, g, c in algo.pareto_list],
                    "final_candidates": [cand_json(g.get_candidate(wrappers)) for g in groups],
                    "final_score": algo._final_eval_score, "score_calls": calls[0],
                    "encodings_computed": sim.encodings_computed})
    assert len(forward_lists) == 1
    return {"model": MODEL, "candidates": [cand_json(c) for c in CANDIDATES], "accuracy_list": forward_lists[0],
            "runs": runs}


def sqnr_section():
    ns = dict(TYPING)

    class Pair(torch.nn.Module):
        """Returns the recorded fp32 output while "all quantizers" are off, else the recorded noisy one."""

        def __init__(self):
            super().__init__()
            self.fp32 = False

        def forward(self, batch):
            return batch[0] if self.fp32 else batch[1]

    @contextlib.contextmanager
    def disable_all_quantizers(model):
        model.fp32 = True
        try:
            yield
        finally:
            model.fp32 = False

    @contextlib.contextmanager
    def in_eval_mode(model):
        yield

    ns.update({"np": np, "torch": torch, "DataLoader": object,
               "utils": types.SimpleNamespace(get_device=lambda m: torch.device("cpu"), in_eval_mode=in_eval_mode,
                                              change_tensor_device_placement=lambda x, d: x,
                                              disable_all_quantizers=disable_all_quantizers)})
    run_reference(TORCH + "mixed_precision_algo.py", ns, only={"_evaluate_sqnr", "_compute_sqnr"})

    class Loader(list):
        batch_size = None

    rng = np.random.default_rng(2023)
    cases = []
    specs = [  # name, batch shapes, batch_size attribute, num_samples, noise scale (None: x == ref)
        ("below", [(4, 6)] * 4, 4, 8, 0.05), ("exact", [(4, 6)] * 4, 4, 16, 0.05),
        ("above", [(4, 6)] * 3, 4, 128, 0.05), ("ragged", [(4, 2, 3, 3), (4, 2, 3, 3), (3, 2, 3, 3)], 4, 10, 0.2),
        ("no_batch_size", [(1, 17)] * 5, None, 3, 0.01), ("equal", [(2, 20)] * 2, 2, 4, None),
        ("large_noise", [(8, 8)] * 2, 8, 16, 3.0)]
    for name, shapes, batch_size, num_samples, noise in specs:
        batches = []
        for shape in shapes:
            assert int(np.prod(shape)) <= 4096
            ref = (rng.standard_normal(shape) * 2.0 + 0.25).astype(np.float32)
            x = ref.copy() if noise is None else (ref + rng.standard_normal(shape).astype(np.float32) *
                                                  np.float32(noise)).astype(np.float32)
            batches.append((ref, x))
        loader = Loader((torch.from_numpy(r), torch.from_numpy(x)) for r, x in batches)
        loader.batch_size = batch_size
        stored, model = [], Pair()
        first = ns["_evaluate_sqnr"](model, None, loader, lambda m, b: m(b), num_samples, stored)
        again = ns["_evaluate_sqnr"](model, None, loader, lambda m, b: m(b), num_samples, stored)
        assert float(first) == float(again)
        cases.append({"name": name, "batch_size": batch_size, "num_samples": num_samples, "db": float(first),
                      # float32 values as their bit patterns, eight hex digits each, big-endian
                      "batches": [{"shape": list(r.shape), "ref_bits": r.ravel().astype(">f4").tobytes().hex(),
                                   "x_bits": x.ravel().astype(">f4").tobytes().hex()} for r, x in batches]})
    return {"eps": 1e-4, "cases": cases}


def main():
    ns = reference_namespace()
    fixture = {"helpers": helpers_section(ns), "searches": searches_section(ns), "runs": runs_section(ns),
               "sqnr": sqnr_section()}
    with open(OUT, "w") as f:
        json.dump(fixture, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
