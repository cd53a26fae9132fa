"""Quantized recurrent layers without a device: the oracle (tests/rnn_oracle.py) against torch's CPU
cells and against the fixture written from the reference (tests/golden/make_golden_rnn.py), the
restated sigmoid and tanh against the recorded sweep (profiles/r16/rnn_math_sweep.txt), the bindings,
the wrapper's quantizer sets and the refusals."""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import REPO

import rnn_oracle as O
from aimet_amd import _native
from aimet_amd.qc_quantize_op import QcQuantizeOpMode, QcQuantizeWrapper
from aimet_amd.quantizers import QuantizationDataType, QuantScheme
from aimet_amd.quantsim import DEFAULT_QUANTIZABLE_TYPES, RECURRENT_TYPES, QuantizationSimModel

F = np.float32
CELLS = {"LSTM": torch._VF.lstm_cell, "GRU": torch._VF.gru_cell, "RNN_TANH": torch._VF.rnn_tanh_cell,
         "RNN_RELU": torch._VF.rnn_relu_cell}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "golden_rnn.npz"))


@pytest.fixture(scope="module")
def sweep():
    with open(os.path.join(REPO, "profiles", "r16", "rnn_math_sweep.txt")) as f:
        return json.loads(f.read().strip().splitlines()[-1])


def grid(rng, shape, step_log2, lo, hi):
    s = 2 ** step_log2
    return (rng.integers(int(lo * s), int(hi * s) + 1, shape) / s).astype(F)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("H", [5, 64, 65])
@pytest.mark.parametrize("mode", list(CELLS))
def test_oracle_cell_with_torch_functions_is_the_vf_cell(mode, H, bias):
    """Values on power-of-two grids, so both GEMMs are exact in any order and only the cell's own
    evaluation order and functions are compared: bit for bit."""
    rng = np.random.default_rng(H * 8 + bias)
    G, B, I = O.GATES[mode], 3, 7
    x, h, c = grid(rng, (B, I), 5, -2, 2), grid(rng, (B, H), 7, -1, 0.99), grid(rng, (B, H), 4, -2, 2)
    w_ih, w_hh = grid(rng, (G * H, I), 6, -1, 1), grid(rng, (G * H, H), 6, -1, 1)
    b_ih, b_hh = (grid(rng, (G * H,), 6, -1, 1), grid(rng, (G * H,), 6, -1, 1)) if bias else (None, None)

    def t(a):
        return None if a is None else torch.from_numpy(a)
    want = CELLS[mode](t(x), (t(h), t(c)) if mode == "LSTM" else t(h), t(w_ih), t(w_hh), t(b_ih), t(b_hh))
    want = want if mode == "LSTM" else (want, None)
    got = O.cell(mode, x @ w_ih.T, h @ w_hh.T, b_ih, b_hh, h, c, O.TORCH_FUNCS)
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(O.bits(a), O.bits(b.numpy()))


def test_oracle_layer_equals_the_reference_fixture_bit_for_bit(golden):
    cases = json.loads(str(golden["cases"]))
    assert len(cases) == 20 and {c["mode"] for c in cases} == set(CELLS)
    assert {(c["packed"], c["state"]) for c in cases} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(c["H"] == 65 for c in cases)
    for case in cases:
        a = O.case_arrays(golden, case["name"])
        if case["packed"]:   # the sorting permutation is not its own inverse: a swap of the two would show
            order = np.argsort(-a["lens"], kind="stable")
            assert not np.array_equal(order, np.argsort(order))
        out, hn, cn = O.run_case(case, a, O.RESTATED_FUNCS, golden["encs"])
        assert np.array_equal(O.bits(out), O.bits(a["out"])), case
        assert np.array_equal(O.bits(hn), O.bits(a["hn"])), case
        if case["mode"] == "LSTM":
            assert np.array_equal(O.bits(cn), O.bits(a["cn"])), case
        # the fixture's own condition: every pre-QDQ state 64 x U spacings from a rounding boundary
        margin, U = (int(v) for v in golden["margin"])
        assert float(a["worst"]) >= margin * U


def test_restated_functions_stay_within_the_recorded_sweep(sweep):
    """Every 65521st float32 bit pattern (a prime stride: all exponents, both signs) against torch's
    CPU functions: no ulp distance and no absolute error above the maxima the full sweep recorded."""
    assert sweep["chunks"] == 256 and sweep["sigmoid"]["restated_equal"] and sweep["tanh"]["restated_equal"]
    x = np.arange(0, 1 << 32, 65521, dtype=np.uint64).astype(np.uint32).view(F)
    x = x[~np.isnan(x)]
    for name, fn, ref in (("sigmoid", O.sigmoid_r, torch.sigmoid), ("tanh", O.tanh_r, torch.tanh)):
        got = fn(x)
        want = ref(torch.from_numpy(x)).numpy()
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        normal = np.isfinite(x) & (np.abs(want) >= F(2.0 ** -126))
        ulp = int(O.ulp_distance(got, want)[normal].max())
        print("%s: sampled max ulp %d (recorded %d), max abs %.3g (recorded %.3g)"
              % (name, ulp, sweep[name]["max_ulp"], err, sweep[name]["max_abs"]))
        assert ulp <= sweep[name]["max_ulp"]
        assert err <= sweep[name]["max_abs"]
        # the input the sweep found worst reproduces its figure
        worst = np.array([int(sweep[name]["max_ulp_at"], 16)], np.uint32).view(F)
        assert int(O.ulp_distance(fn(worst), ref(torch.from_numpy(worst)).numpy())[0]) == sweep[name]["max_ulp"]


def test_c_abi_names_are_exported():
    lib = _native.load()
    for name in ("aimet_rnn_step", "aimet_rnn_launch_count"):
        assert name in _native.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    with open(os.path.join(REPO, "include", "aimet_amd.h")) as f:
        header = f.read()
    assert "int aimet_rnn_step(" in header and "aimet_rnn_step_job" in header
    assert ctypes_size(_native.RnnStepJobC) == 10 * 8 + 5 * 8 + 8   # ten pointers, five strides, the flag padded


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


class Net(nn.Module):
    def __init__(self, rnn):
        super().__init__()
        self.a, self.rnn, self.b = nn.Linear(7, 7), rnn, nn.Linear(2 * rnn.hidden_size, 3)

    def forward(self, x):
        return self.b(self.rnn(self.a(x))[0])


def structure(w):
    groups = w.grouped_quantizers

    def group_of(q):
        return next((g for g, gq in groups.items() if gq is q), None)
    return {kind: {name: {"enabled": bool(q.enabled), "group": group_of(q)} for name, q in d.items()}
            for kind, d in (("input_quantizers", w.input_quantizers), ("output_quantizers", w.output_quantizers),
                            ("param_quantizers", w.param_quantizers), ("grouped_quantizers", groups))}


@pytest.mark.parametrize("mode", ["LSTM", "GRU"])
def test_sim_wraps_recurrent_layers_with_the_reference_quantizer_sets(golden, mode):
    import aimet_amd.qc_quantize_recurrent as R
    assert RECURRENT_TYPES == (nn.RNN, nn.LSTM, nn.GRU)
    assert not any(t in DEFAULT_QUANTIZABLE_TYPES for t in RECURRENT_TYPES)
    rnn = (nn.LSTM if mode == "LSTM" else nn.GRU)(7, 5, num_layers=2, bidirectional=True)
    net = Net(rnn)
    sim = QuantizationSimModel(net, quant_scheme="tf")
    w = sim.model.rnn
    assert isinstance(w, R.QcQuantizeRecurrent) and not isinstance(w, QcQuantizeWrapper)
    assert [n for n, _ in sim.quant_wrappers()] == ["a", "b"]
    assert [n for n, _ in sim.recurrent_wrappers()] == ["rnn"]
    want = json.loads(str(golden["structure"]))[mode]
    assert structure(w) == want
    # the few facts the issue names, spelled out
    assert w.input_quantizers["initial_h_l1"] is w.output_quantizers["h_l1"] is w.grouped_quantizers["hidden_l1"]
    assert w.param_quantizers["weight_ih_l0"] is w.param_quantizers["weight_ih_l0_reverse"] is w.grouped_quantizers["W_l0"]
    assert w.grouped_quantizers["hidden_l0"].enabled and w.grouped_quantizers["R_l0"].enabled
    assert not w.grouped_quantizers["bias_l0"].enabled and w.input_quantizers["input_l1"].enabled
    if mode == "LSTM":
        assert not w.grouped_quantizers["cell_l0"].enabled
    # the wrapper holds clones; update_params / get_original_model hand them back
    with torch.no_grad():
        w.weight_hh_l0.add_(1.0)
    assert not torch.equal(w.weight_hh_l0, w.module_to_quantize.weight_hh_l0)
    original = QuantizationSimModel.get_original_model(sim.model)
    assert type(original.rnn) is type(rnn) and torch.equal(original.rnn.weight_hh_l0, w.weight_hh_l0)
    assert [n for n, _ in w.get_named_parameters()] == [n for n, _ in rnn.named_parameters()]
    sim.exclude_layers_from_quantization([sim.model.rnn])
    assert type(sim.model.rnn) is type(rnn) and list(sim.recurrent_wrappers()) == []


def test_model_without_recurrent_layers_builds_the_same_sim():
    net = nn.Sequential(nn.Linear(7, 7), nn.ReLU(), nn.Linear(7, 3))
    sim = QuantizationSimModel(net, quant_scheme="tf")
    assert [n for n, _ in sim.quant_wrappers()] == ["0", "2"] and list(sim.recurrent_wrappers()) == []
    assert sim.model[0].input_quantizers[0].enabled and not sim.model[2].input_quantizers[0].enabled


def test_sim_applies_its_config_to_recurrent_wrappers():
    cfg = {"defaults": {"ops": {"is_symmetric": "True"}, "params": {"is_symmetric": "False"},
                        "strict_symmetric": "True", "unsigned_symmetric": "True"}}
    w = QuantizationSimModel(Net(nn.GRU(7, 5, bidirectional=True)), quant_scheme="tf", config_file=cfg).model.rnn
    assert not w.grouped_quantizers["W_l0"].use_symmetric_encodings and not w.grouped_quantizers["R_l0"].use_symmetric_encodings
    assert w.grouped_quantizers["hidden_l0"].use_symmetric_encodings and w.input_quantizers["input_l0"].use_symmetric_encodings
    assert all(q.use_strict_symmetric and q.use_unsigned_symmetric for q in w._all_quantizers())
    w = QuantizationSimModel(Net(nn.GRU(7, 5, bidirectional=True)), quant_scheme="tf").model.rnn
    assert w.grouped_quantizers["W_l0"].use_symmetric_encodings and not w.grouped_quantizers["hidden_l0"].use_symmetric_encodings
    assert not w.grouped_quantizers["W_l0"].use_strict_symmetric
    with pytest.raises(NotImplementedError, match="per-channel"):
        QuantizationSimModel(Net(nn.GRU(7, 5, bidirectional=True)), quant_scheme="tf",
                             config_file={"defaults": {"per_channel_quantization": "True"}})
    # without a recurrent layer the setting is as before
    QuantizationSimModel(nn.Sequential(nn.Linear(7, 3)), quant_scheme="tf",
                         config_file={"defaults": {"per_channel_quantization": "True"}})


def test_import_encodings_follows_the_wrappers_rules():
    from aimet_amd.qc_quantize_recurrent import QcQuantizeRecurrent as Q
    w = Q(nn.LSTM(7, 5), 8, 8, "nearest", QuantScheme.post_training_tf)
    enc = {"min": -1.0, "max": 127.0 / 128.0, "scale": 1.0 / 128.0, "offset": -128, "bitwidth": 8,
           "is_symmetric": "False", "dtype": "int"}
    w.grouped_quantizers["cell_l0"].enabled = True   # on here, absent from the file
    w.import_encodings({"weight_ih_l0": [enc]}, {"h_l0": enc, "initial_h_l0": enc}, strict=True, partial=True)
    assert w.output_quantizers["h_l0"].encoding.min == -1.0 and w.param_quantizers["weight_ih_l0"].encoding.bw == 8
    assert w.grouped_quantizers["cell_l0"].enabled and w.grouped_quantizers["R_l0"].enabled   # partial: kept
    assert not w.grouped_quantizers["bias_l0"].enabled                                        # nothing enabled by a file
    with pytest.raises(RuntimeError, match="same configuration"):
        w.import_encodings({"bias_ih_l0": [enc]}, {}, strict=True, partial=True)
    w.import_encodings({"bias_ih_l0": [enc]}, {}, strict=False, partial=True)
    assert not w.grouped_quantizers["bias_l0"].enabled and w.grouped_quantizers["bias_l0"].encoding is None
    w.import_encodings({"weight_ih_l0": [enc]}, {"h_l0": enc, "initial_h_l0": enc}, strict=True, partial=False)
    assert not w.grouped_quantizers["cell_l0"].enabled and not w.grouped_quantizers["R_l0"].enabled
    assert w.grouped_quantizers["hidden_l0"].enabled and w.grouped_quantizers["W_l0"].enabled


def test_refusals():
    from aimet_amd.qc_quantize_recurrent import QcQuantizeRecurrent as Q
    lstm = nn.LSTM(7, 5)
    with pytest.raises(NotImplementedError, match="proj_size"):
        Q(nn.LSTM(7, 5, proj_size=3), 8, 8, "nearest", QuantScheme.post_training_tf)
    with pytest.raises(NotImplementedError, match="float"):
        Q(lstm, 8, 8, "nearest", QuantScheme.post_training_tf, data_type=QuantizationDataType.float)
    with pytest.raises(NotImplementedError, match="stochastic"):
        Q(lstm, 8, 8, "stochastic", QuantScheme.post_training_tf)
    with pytest.raises(NotImplementedError, match="range learning"):
        Q(lstm, 8, 8, "nearest", QuantScheme.training_range_learning_with_tf_init)
    with pytest.raises(NotImplementedError, match="range learning"):
        QuantizationSimModel(Net(nn.LSTM(7, 5, bidirectional=True)),
                             quant_scheme=QuantScheme.training_range_learning_with_tf_init)
    w = Q(lstm, 8, 8, "nearest", QuantScheme.post_training_tf)
    with pytest.raises(NotImplementedError, match="LEARN_ENCODINGS"):
        w.set_mode(QcQuantizeOpMode.LEARN_ENCODINGS)
    with pytest.raises(NotImplementedError, match="LEARN_ENCODINGS"):
        w.construct_and_initialize_trainable_quantizers(QuantScheme.training_range_learning_with_tf_init)
    with pytest.raises(NotImplementedError, match="per-channel"):
        w.enable_per_channel_quantization()
    with pytest.raises(NotImplementedError, match="ONNX"):
        w.get_activation_param_quantizers_for_onnx_tensors([])
    with pytest.raises(RuntimeError, match="autograd"):
        w(torch.zeros(4, 3, 7, requires_grad=True))
    with pytest.raises(RuntimeError, match="no CPU path"):
        w(torch.zeros(4, 3, 7))
    w.set_mode(QcQuantizeOpMode.PASSTHROUGH)
    assert w._mode is QcQuantizeOpMode.PASSTHROUGH
