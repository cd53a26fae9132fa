"""Automatic mixed precision without a GPU (aimet_amd/amp, aimet_amd/mixed_precision.py) against
tests/golden/golden_amp.json, which tests/golden/make_golden_amp.py records from the reference's own
helpers, searches and base algorithm:

* the helpers and the three searches equal the reference's, the searches also in the order they
  evaluate;
* the base algorithm on the fixture's six stand-in groups equals the reference's runs entry for entry:
  every search x phase2_reverse x four allowed drops;
* resume from .cache, clean_start, restored quantizer state after a raising callback;
* QuantizerGroup: hashable, picklable, to_list.
"""
import functools
import json
import math
import os
import pickle

import pytest

from conftest import REPO

from aimet_amd.amp import utils as U
from aimet_amd.amp.mixed_precision_algo import MixedPrecisionAlgoBase
from aimet_amd.amp.quantizer_groups import QuantizerGroup
from aimet_amd.amp.utils import AMPSearchAlgo
from aimet_amd.quant_analyzer import CallbackFunc
from aimet_amd.quantizers import QuantizationDataType

with open(os.path.join(REPO, "tests", "golden", "golden_amp.json")) as _f:
    GOLDEN = json.load(_f)
MODEL = GOLDEN["runs"]["model"]
DTYPES = {"int": QuantizationDataType.int, "float": QuantizationDataType.float, None: None}


def cand(j):
    """A candidate as the fixture writes it -> as the package takes it."""
    return None if j is None else tuple((bw, DTYPES[dt]) for bw, dt in j)


def cand_json(c):
    return None if c is None else [[bw, None if dt is None else dt.name] for bw, dt in c]


CANDIDATES = [cand(c) for c in GOLDEN["runs"]["candidates"]]
NAMED = {k: cand(v) for k, v in GOLDEN["helpers"]["candidates"].items()}
MAC_DICT = {name: spec["macs"] for name, spec in MODEL["modules"].items() if spec["macs"]}


# ---------------------------------------------------------------------------------------------------
# the fixture's stand-ins
# ---------------------------------------------------------------------------------------------------
class StubQuantizer:
    def __init__(self, enabled=True):
        self.enabled, self.bitwidth, self.data_type = enabled, 8, QuantizationDataType.int


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


def make_groups():
    return [QuantizerGroup(input_quantizers=tuple(g["input"]), output_quantizers=tuple(g["output"]),
                           parameter_quantizers=tuple(g["weight"])) for g in MODEL["groups"]]


def make_wrappers():
    return {name: StubWrapper(spec) for name, spec in MODEL["modules"].items()}


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


class Algo(MixedPrecisionAlgoBase):
    def __init__(self, sim, wrappers, groups, *args):
        self._given = (wrappers, groups)
        super().__init__(sim, *args)

    def _find_quantizer_group(self, sim):
        return self._given


class Run:
    """One run of the base algorithm on fresh stand-ins."""

    def __init__(self, results_dir, clean_start=True, reverse=False, raise_at=None):
        self.wrappers, self.groups = make_wrappers(), make_groups()
        self.sim, self.calls = StubSim(), 0
        self.raise_at = raise_at
        cb = CallbackFunc(self.score, None)
        self.algo = Algo(self.sim, self.wrappers, self.groups, CANDIDATES, cb, cb, CallbackFunc(lambda m, a: None, None),
                         MAC_DICT, str(results_dir), clean_start, reverse)

    def score(self, model, args):
        self.calls += 1
        if self.calls == self.raise_at:
            raise ArithmeticError("the eval callback fails")
        return score_of(self.groups, self.wrappers)

    def state(self):
        return [(q.enabled, q.bitwidth, q.data_type) for w in self.wrappers.values()
                for q in w.input_quantizers + w.output_quantizers + list(w.param_quantizers.values())]


# ---------------------------------------------------------------------------------------------------
# (a) helpers
# ---------------------------------------------------------------------------------------------------
def test_effective_bitwidth_and_starting_bit_ops():
    for dtype, bw, want in GOLDEN["helpers"]["effective"]:
        assert U.get_effective_bitwidth(DTYPES[dtype], bw) == want
    assert U.FLOATING_POINT_MULTIPLIER == math.sqrt(1.5)
    for name, want in GOLDEN["helpers"]["starting"].items():
        assert U.calculate_starting_bit_ops(MAC_DICT, NAMED[name]) == want, name


def test_bit_ops_reduction():
    groups = make_groups()
    assert len(GOLDEN["helpers"]["reduction"]) == 60
    for g, hi, lo, want in GOLDEN["helpers"]["reduction"]:
        assert U.find_bit_ops_reduction(groups[g], MAC_DICT, NAMED[hi], NAMED[lo]) == want, (g, hi, lo)


def test_running_bit_ops():
    groups = make_groups()
    for name, walk in GOLDEN["helpers"]["running"].items():
        start = NAMED[walk["start"]]
        total, seen = U.calculate_starting_bit_ops(MAC_DICT, start), {}
        for g, c, want in walk["steps"]:
            total = U.calculate_running_bit_ops(MAC_DICT, groups[g], seen, start, NAMED[c], total)
            assert total == want, (name, g, c)


def test_sort_accuracy_list():
    groups = make_groups()
    entries = [(groups[g], NAMED[c], s, b) for g, c, s, b in GOLDEN["helpers"]["sort"]["entries"]]
    got = U.sort_accuracy_list(entries, {g: i for i, g in enumerate(groups)})
    assert [entries.index(e) for e in got] == GOLDEN["helpers"]["sort"]["order"]


def test_reverse_list_rewrite():
    groups = make_groups()
    index_of = {g: i for i, g in enumerate(groups)}
    rev = [(groups[g], NAMED[c], float(10 + k), k) for k, (g, c) in enumerate(GOLDEN["helpers"]["reverse"]["entries"])]
    order = U.create_quant_group_to_candidate_dict(rev)
    assert [[index_of[g], [cand_json(c) for c in cs]] for g, cs in order.items()] == GOLDEN["helpers"]["reverse"]["order"]
    got = U.modify_candidate_in_accuracy_list(rev, order, NAMED["i16_16"])
    assert [[index_of[g], cand_json(c), s, b] for g, c, s, b in got] == GOLDEN["helpers"]["reverse"]["modified"]


def test_candidate_types():
    c = U.AmpCandidate(NAMED["i16_8"])
    assert (c.output_bw, c.output_dtype, c.param_bw, c.param_dtype) == (16, QuantizationDataType.int, 8,
                                                                      QuantizationDataType.int)
    assert U.CandAttr.activation == 0 and U.CandAttr.parameter == 1
    assert U.CandParam.bitwdith == 0 and U.CandParam.data_type == 1
    assert [a.value for a in (AMPSearchAlgo.BruteForce, AMPSearchAlgo.Interpolation, AMPSearchAlgo.Binary)] == [1, 2, 3]


def test_enable_disable_and_export_list(tmp_path):
    qs = [StubQuantizer(True), StubQuantizer(False)]
    U.disable_quantizers(qs)
    assert [q.enabled for q in qs] == [False, False]
    U.enable_quantizers(qs)
    assert [q.enabled for q in qs] == [True, True]
    U.export_list([("a", 1), ("b", None)], str(tmp_path / "new"), "info")
    assert json.load(open(tmp_path / "new" / "info.json")) == [["a", 1], ["b", None]]


# ---------------------------------------------------------------------------------------------------
# (b) searches
# ---------------------------------------------------------------------------------------------------
def test_searches_visit_the_reference_indices():
    lists = GOLDEN["searches"]["lists"]
    assert len(GOLDEN["searches"]["cases"]) == 4 * 3 * 2 * 6
    for row in GOLDEN["searches"]["cases"]:
        case = dict(zip(GOLDEN["searches"]["columns"], row))
        vals, visited = lists[case["list"]], []
        values = [functools.partial(lambda i: (visited.append(i), vals[i])[1], i) for i in range(len(vals))]
        target = -math.inf if case["target"] == "-inf" else case["target"]
        try:
            index = getattr(U, case["algo"])(values, target, case["reverse"])
        except ZeroDivisionError:
            index = "ZeroDivisionError"
        assert (index, visited) == (case["index"], case["visited"]), case


# ---------------------------------------------------------------------------------------------------
# (c) the base algorithm
# ---------------------------------------------------------------------------------------------------
RUNS = GOLDEN["runs"]["runs"]
for _r in RUNS:     # the fixture holds phase 1's list once; phase2_reverse leaves it reversed
    _way = _r["accuracy_list"]
    _r["accuracy_list"] = None if _way is None else GOLDEN["runs"]["accuracy_list"][::1 if _way == "forward" else -1]


def test_fixture_covers_every_combination():
    assert sorted((r["algo"], r["reverse"], r["drop_name"]) for r in RUNS) == sorted(
        (a, rev, d) for a in ("BruteForce", "Interpolation", "Binary") for rev in (False, True)
        for d in ("none", "midway", "below_best", "above_lowest"))
    assert len(MODEL["groups"]) == 6 and len(CANDIDATES) == 3


@pytest.mark.parametrize("want", RUNS, ids=["%s-%s-%s" % (r["algo"], "reverse" if r["reverse"] else "forward",
                                                          r["drop_name"]) for r in RUNS])
def test_base_algorithm_equals_the_reference(want, tmp_path):
    run = Run(tmp_path, reverse=want["reverse"])
    algo = run.algo
    algo.run(want["drop"], AMPSearchAlgo[want["algo"]])
    index_of = {g: i for i, g in enumerate(run.groups)}
    assert algo.fp32_accuracy == want["fp32_accuracy"]
    assert cand_json(algo.baseline_candidate) == want["baseline_candidate"]
    assert cand_json(algo.min_candidate) == want["min_candidate"] and algo.min_accuracy == want["min_accuracy"]
    got_acc = None if algo.accuracy_list is None else \
        [[index_of[g], CANDIDATES.index(c), s, b] for g, c, s, b in algo.accuracy_list]
    assert got_acc == want["accuracy_list"]
    got_pareto = None if algo.pareto_list is None else \
        [[b, s, index_of[g], CANDIDATES.index(c)] for b, s, g, c in algo.pareto_list]
    assert got_pareto == want["pareto_list"]
    assert [cand_json(g.get_candidate(run.wrappers)) for g in run.groups] == want["final_candidates"]
    assert algo._final_eval_score == want["final_score"]
    assert run.calls == want["score_calls"]
    assert run.sim.encodings_computed == want["encodings_computed"]
    if want["pareto_list"] is not None:
        assert "Mixed precision model accuracy %s" % want["final_score"] in str(algo)
        for name in ("pareto_list.json", "amp_info_list.json", ".cache/accuracy_list.json", ".cache/accuracy_list.pkl",
                     ".cache/pareto_list.pkl"):
            assert os.path.isfile(os.path.join(str(tmp_path), name)), name
        rows = json.load(open(tmp_path / "pareto_list.json"))
        assert [r[:2] for r in rows] == [p[:2] for p in want["pareto_list"]]
        assert [tuple(t) for t in rows[0][2]] == run.groups[want["pareto_list"][0][2]].to_list()
        info = dict(json.load(open(tmp_path / "amp_info_list.json")))
        assert info["final score"] == want["final_score"] and info["phase2 eval count"] == len(want["pareto_list"])
        if want["reverse"]:
            assert os.path.isfile(tmp_path / ".cache" / "accuracy_list_reverse.json")
            assert os.path.isfile(tmp_path / ".cache" / "accuracy_list_reverse_modified.json")


def test_str_needs_a_run(tmp_path):
    with pytest.raises(RuntimeError, match="Call run"):
        str(Run(tmp_path).algo)


def test_invalid_search_and_candidates(tmp_path):
    with pytest.raises(ValueError, match="Invalid search algo"):
        Run(tmp_path).algo.run(None, "binary")
    with pytest.raises(AssertionError):
        Algo(StubSim(), make_wrappers(), make_groups(), [((8, "int"), (8, "int"))], None, None,
             CallbackFunc(None, None), MAC_DICT, str(tmp_path), True)


# ---------------------------------------------------------------------------------------------------
# resume, clean start, a raising callback
# ---------------------------------------------------------------------------------------------------
def _want(algo, reverse, drop_name):
    return next(r for r in RUNS if (r["algo"], r["reverse"], r["drop_name"]) == (algo, reverse, drop_name))


def test_resume_makes_no_score_call_for_a_cached_entry(tmp_path):
    first = Run(tmp_path)
    first.algo.run(None, AMPSearchAlgo.BruteForce)
    want = _want("BruteForce", False, "none")
    assert first.calls == want["score_calls"]
    # fp32, three baseline options, the final score: everything phase 1 and phase 2 scored is cached
    again = Run(tmp_path, clean_start=False)
    again.algo.run(None, AMPSearchAlgo.BruteForce)
    assert again.calls == 1 + len(CANDIDATES) + 1
    index_of = {g: i for i, g in enumerate(again.groups)}
    assert [[index_of[g], CANDIDATES.index(c), s, b] for g, c, s, b in again.algo.accuracy_list] == want["accuracy_list"]
    assert [[b, s, index_of[g], CANDIDATES.index(c)] for b, s, g, c in again.algo.pareto_list] == want["pareto_list"]
    assert again.algo._final_eval_score == want["final_score"]


def test_resume_after_an_interrupted_phase_1(tmp_path):
    want = _want("Binary", False, "midway")
    # fp32 + 3 baseline options, then phase 1: fail at its sixth score
    broken = Run(tmp_path, raise_at=1 + len(CANDIDATES) + 6)
    with pytest.raises(ArithmeticError):
        broken.algo.run(want["drop"], AMPSearchAlgo.Binary)
    cached = pickle.load(open(tmp_path / ".cache" / "accuracy_list.pkl", "rb"))
    assert len(cached) == 5
    resumed = Run(tmp_path, clean_start=False)
    resumed.algo.run(want["drop"], AMPSearchAlgo.Binary)
    assert resumed.calls == want["score_calls"] - 5
    index_of = {g: i for i, g in enumerate(resumed.groups)}
    assert [[index_of[g], CANDIDATES.index(c), s, b] for g, c, s, b in resumed.algo.accuracy_list] == want["accuracy_list"]
    assert resumed.algo._final_eval_score == want["final_score"]


def test_clean_start_deletes_the_caches(tmp_path):
    Run(tmp_path).algo.run(None, AMPSearchAlgo.BruteForce)
    cache = tmp_path / ".cache"
    stale = [(0.5, 123.0, make_groups()[0], CANDIDATES[1])]
    pickle.dump(stale, open(cache / "pareto_list.pkl", "wb"))
    pickle.dump([(make_groups()[0], CANDIDATES[1], 123.0, 7)], open(cache / "accuracy_list.pkl", "wb"))
    again = Run(tmp_path, clean_start=True)
    again.algo.run(None, AMPSearchAlgo.BruteForce)
    want = _want("BruteForce", False, "none")
    assert again.calls == want["score_calls"]
    assert all(score != 123.0 for _, score, _, _ in again.algo.pareto_list)
    assert all(score != 123.0 for _, _, score, _ in again.algo.accuracy_list)
    assert pickle.load(open(cache / "pareto_list.pkl", "rb")) != stale


@pytest.mark.parametrize("nth", [1, 4, 12])
def test_raising_callback_restores_the_quantizers(tmp_path, nth):
    run = Run(tmp_path)
    run.algo.set_baseline()
    run.algo.min_accuracy, run.algo.min_candidate = run.algo._choose_lowest_from_candidates()
    before = run.state()
    run.raise_at = run.calls + nth      # the nth score of phase 1
    with pytest.raises(ArithmeticError):
        run.algo.run(None, AMPSearchAlgo.BruteForce)
    assert run.state() == before
    assert run.algo.pareto_list is None


# ---------------------------------------------------------------------------------------------------
# QuantizerGroup
# ---------------------------------------------------------------------------------------------------
def test_quantizer_group_is_hashable_picklable_and_lists_itself():
    g = QuantizerGroup(input_quantizers=("a_input_quantizer_idx_0", "b_input_quantizer_idx_1"),
                       output_quantizers=("c",), parameter_quantizers=("a", "b"), supported_kernel_ops=("a", "b"))
    same = QuantizerGroup(("a_input_quantizer_idx_0", "b_input_quantizer_idx_1"), ("c",), ("a", "b"), ("a", "b"))
    assert g == same and hash(g) == hash(same) and len({g, same}) == 1
    assert pickle.loads(pickle.dumps(g)) == g
    assert g.to_list() == [("input", "a_input_quantizer_idx_0"), ("input", "b_input_quantizer_idx_1"),
                           ("output", "c"), ("weight", "a"), ("weight", "b")]
    assert g.get_input_quantizer_modules() == ("a", "b")
    assert QuantizerGroup() == QuantizerGroup((), (), (), ()) and QuantizerGroup().to_list() == []
    with pytest.raises(Exception):
        g.output_quantizers = ()


def test_quantizer_group_candidates_on_stand_ins():
    wrappers, groups = make_wrappers(), make_groups()
    f16 = ((16, QuantizationDataType.float), (16, QuantizationDataType.float))
    groups[1].set_quantizers_to_candidate(wrappers, f16)
    assert groups[1].get_candidate(wrappers) == f16
    assert (wrappers["m0"].output_quantizers[0].bitwidth, wrappers["m1"].param_quantizers["weight"].data_type) == \
        (16, QuantizationDataType.float)
    assert wrappers["m0"].param_quantizers["weight"].bitwidth == 8        # not in the group
    groups[3].set_quantizers_to_candidate(wrappers, ((4, QuantizationDataType.int),))
    assert groups[3].get_candidate(wrappers) == ((4, QuantizationDataType.int), (None, None))
    wrappers["m4"].param_quantizers["weight"].enabled = False
    wrappers["m5"].param_quantizers["weight"].bitwidth = 4
    assert groups[4].get_candidate(wrappers)[1] == (4, QuantizationDataType.int)   # the first enabled one
    assert len(groups[4].get_active_quantizers(wrappers)) == 2
    assert groups[5].get_active_quantizers(wrappers) == wrappers["m5"].output_quantizers


def test_bindings_declare_the_two_entry_points():
    from aimet_amd import _native
    want = ["aimet_amp_launch_count", "aimet_amp_sqnr_add"]
    assert sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("aimet_amp_")) == want
    lib = _native.load()
    assert all(hasattr(lib, s) for s in want)


def test_sqnr_entry_point_rejects_host_memory_and_bad_arguments():
    import ctypes

    import numpy as np

    from aimet_amd import _native
    from aimet_amd.amp import mixed_precision_algo as A
    lib = _native.load()
    before = A.launch_count()
    r, x, acc = np.ones(16, np.float32), np.zeros(16, np.float32), np.zeros(1, np.float64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    assert lib.aimet_amp_sqnr_add(p(r), p(x), 0, 0, 1e-4, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(p(r), p(x), (1 << 40) + 1, 0, 1e-4, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(p(r), p(x), 16, 3, 1e-4, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(p(r), p(x), 16, 0, 1e-4, p(acc), None) != 0      # host memory
    assert lib.aimet_amp_sqnr_add(None, p(x), 16, 0, 1e-4, p(acc), None) != 0
    assert A.launch_count() == before and acc[0] == 0
