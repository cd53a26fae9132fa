"""Generate tests/golden/golden_rnn.npz: quantized RNN / LSTM / GRU layers in ACTIVE mode.

The reference's `QcQuantizeRecurrent` (aimet_torch/v1/qc_quantize_recurrent.py) -- its forward, its
packed-sequence, reverse-pass and hidden-row helpers, its quantizer grouping and default states -- is
parsed from the reference file with `ast` and executed at generation time on the CPU in float32, with
torch's `_VF` cells, and with stand-ins for what it imports: quantizers that hold a preset encoding and
quantize-dequantize with the project's CPU oracle. Nothing of its text is stored; the fixture holds
data only.

Exact fixtures: weights, biases and the given h0 are multiples of 2^-6 / 2^-7 in [-1, 1], inputs
multiples of 2^-5, the encodings preset to power-of-two steps (h: delta 2^-7, offset -128; inputs:
delta 2^-5; parameters: delta 2^-6, which leaves them as they are), so every GEMM sum is exact in
float32 in any order and the only CPU / GPU difference left is the activation functions. Every
pre-QDQ h of every step is kept at least 64 x U float32 spacings away from a rounding boundary of its
QDQ (U: the largest ulp distance of profiles/r16/rnn_math_sweep.txt); a case is reseeded until that
holds. The LSTM fixtures also enable the cell quantizer (delta 2^-5, the same margin): an unquantized
c_n would carry the last bits of whichever sigmoid and tanh computed it. tests/rnn_oracle.py with the
restated functions must then give the reference's outputs bit for bit (asserted). No element is
excluded from any comparison.

    python tests/golden/make_golden_rnn.py
"""
import ast
import contextlib
import enum
import json
import logging
import os
import sys
import types
from collections import defaultdict
from typing import Dict, List, Tuple, Union

sys.dont_write_bytecode = True

import numpy as np
import torch
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)
import rnn_oracle as O  # noqa: E402

REF_ROOT = os.environ.get("AIMET_REFERENCE", "/root/reference")
SOURCE = "TrainingExtensions/torch/src/python/aimet_torch/v1/qc_quantize_recurrent.py"
SWEEP = os.path.join(REPO, "profiles", "r16", "rnn_math_sweep.txt")
F = np.float32

ENC_INPUT = (-4.0, 127.0 / 32.0, 8)      # delta 2^-5, offset -128
ENC_HIDDEN = (-1.0, 127.0 / 128.0, 8)    # delta 2^-7, offset -128
ENC_PARAM = (-2.0, 127.0 / 64.0, 8)      # delta 2^-6, offset -128
ENC_CELL = (-4.0, 127.0 / 32.0, 8)       # delta 2^-5: the LSTM fixtures enable the cell quantizer
ENCS = (ENC_INPUT, ENC_HIDDEN, ENC_PARAM, ENC_CELL)
MARGIN = 64


class OpMode(enum.Enum):
    PASSTHROUGH = 1
    ANALYSIS = 2
    ACTIVE = 3
    LEARN_ENCODINGS = 4


class StubQuantizer:
    """What the reference's forward needs of a tensor quantizer: an enabled flag, an encoding, and a
    QDQ (the project's oracle). Remembers how close a pre-QDQ value came to a rounding boundary."""

    def __init__(self, bitwidth, round_mode, quant_scheme, use_symmetric_encodings=False, enabled_by_default=False,
                 data_type=None):
        self.bitwidth, self.round_mode, self.enabled = bitwidth, round_mode, enabled_by_default
        self.encoding = None
        self.worst = np.inf   # smallest (distance to a boundary) / (spacing of the value)

    def quantize_dequantize(self, tensor, round_mode):
        if not self.enabled:
            return tensor
        x = tensor.detach().numpy().astype(F)
        mn, mx, bw = self.encoding
        delta = (mx - mn) / (2 ** bw - 1)
        inside = x[(x > mn) & (x < mx)].astype(np.float64)
        if inside.size:
            v = inside / delta
            dist = np.abs(np.abs(v - np.floor(v)) - 0.5) * delta
            self.worst = min(self.worst, float(np.min(dist / np.spacing(np.abs(inside).astype(F)).astype(np.float64))))
        return torch.from_numpy(O.qdq(x, self.encoding))

    def update_encoding_stats(self, tensor):
        pass

    def reset_encoding_stats(self):
        pass

    def compute_encoding(self):
        pass


def reference_namespace():
    ns = {"torch": torch, "contextlib": contextlib, "defaultdict": defaultdict, "Tuple": Tuple, "List": List,
          "Union": Union, "Dict": Dict, "PackedSequence": PackedSequence, "pad_packed_sequence": pad_packed_sequence,
          "pack_padded_sequence": pack_padded_sequence,
          "libpymo": types.SimpleNamespace(RoundingMode=types.SimpleNamespace(ROUND_NEAREST=0, ROUND_STOCHASTIC=1),
                                           TfEncoding=object),
          "QuantScheme": object, "QuantizationDataType": types.SimpleNamespace(int=0, float=1),
          "MAP_ROUND_MODE_TO_PYMO": {"nearest": 0, "stochastic": 1}, "OpToIOTensors": object,
          "QcQuantizeOpMode": OpMode, "tensor_quantizer_factory": StubQuantizer,
          "StaticGridPerTensorQuantizer": object, "LearnedGridTensorQuantizer": object, "ParameterQuantizer": None,
          "initialize_learned_grid_quantizer_attributes": None, "set_encoding_min_max_gating_threshold": None,
          "get_device": lambda m: next(m.parameters()).device, "_logger": logging.getLogger("golden_rnn")}
    path = os.path.join(REF_ROOT, SOURCE)
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if not isinstance(n, (ast.Import, ast.ImportFrom)) and
            not (isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "_logger")]
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def grid(rng, shape, step_log2, lo, hi):
    """Multiples of 2^-step_log2 in [lo, hi]."""
    s = 2 ** step_log2
    return (rng.integers(int(lo * s), int(hi * s) + 1, shape) / s).astype(F)


def make_module(rng, mode, I, H, bias, batch_first=False):
    cls = {"LSTM": torch.nn.LSTM, "GRU": torch.nn.GRU}.get(mode, torch.nn.RNN)
    kw = {"nonlinearity": "tanh" if mode == "RNN_TANH" else "relu"} if cls is torch.nn.RNN else {}
    m = cls(I, H, num_layers=2, bidirectional=True, bias=bias, batch_first=batch_first, **kw)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.from_numpy(grid(rng, tuple(p.shape), 6, -1, 1)))
    return m.eval()


def preset(wrapper):
    for name, q in wrapper.grouped_quantizers.items():
        q.encoding = ENC_HIDDEN if name.startswith("hidden") else ENC_CELL if name.startswith("cell") else ENC_PARAM
        if name.startswith("cell"):
            q.enabled = True   # off by default; on here, or c_n could not be compared bit for bit
    for name, q in wrapper.input_quantizers.items():
        if name.startswith("input"):
            q.encoding = ENC_INPUT


def structure(wrapper):
    """The quantizer sets of a wrapper as data: names, enabled flags, and the group each shares."""
    groups = wrapper.grouped_quantizers

    def group_of(q):
        return next((g for g, gq in groups.items() if gq is q), None)
    return {kind: {name: {"enabled": bool(q.enabled), "group": group_of(q)} for name, q in d.items()}
            for kind, d in (("input_quantizers", wrapper.input_quantizers),
                            ("output_quantizers", wrapper.output_quantizers),
                            ("param_quantizers", wrapper.param_quantizers), ("grouped_quantizers", groups))}


def check_cells(rng):
    """The oracle's cell with torch's CPU sigmoid and tanh is torch's _VF cell, bit for bit."""
    cells = {"LSTM": torch._VF.lstm_cell, "GRU": torch._VF.gru_cell, "RNN_TANH": torch._VF.rnn_tanh_cell,
             "RNN_RELU": torch._VF.rnn_relu_cell}
    for mode, fn in cells.items():
        for H, bias in ((5, True), (65, True), (5, False)):
            G, B, I = O.GATES[mode], 3, 7
            x, h, c = grid(rng, (B, I), 5, -2, 2), grid(rng, (B, H), 7, -1, 0.99), grid(rng, (B, H), 4, -2, 2)
            w_ih, w_hh = grid(rng, (G * H, I), 6, -1, 1), grid(rng, (G * H, H), 6, -1, 1)
            b_ih, b_hh = (grid(rng, (G * H,), 6, -1, 1), grid(rng, (G * H,), 6, -1, 1)) if bias else (None, None)
            t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
            hx = (t(h), t(c)) if mode == "LSTM" else t(h)
            want = fn(t(x), hx, t(w_ih), t(w_hh), t(b_ih), t(b_hh))
            got = O.cell(mode, x @ w_ih.T, h @ w_hh.T, b_ih, b_hh, h, c, O.TORCH_FUNCS)
            want = want if mode == "LSTM" else (want, None)
            for a, b in zip(got, want):
                assert (a is None) == (b is None)
                if a is not None:
                    assert np.array_equal(O.bits(a), O.bits(b.numpy())), (mode, H, bias)


CASES = [dict(mode="LSTM", H=5, bias=True, batch_first=False), dict(mode="LSTM", H=65, bias=True, batch_first=False),
         dict(mode="GRU", H=5, bias=True, batch_first=True), dict(mode="RNN_TANH", H=5, bias=True, batch_first=False),
         dict(mode="RNN_RELU", H=5, bias=False, batch_first=False)]
I_SIZE, B, T = 7, 3, 4
LENS = [2, 1, 4]   # unsorted; sorting it is a 3-cycle, so the sorting permutation and its inverse differ


def main():
    sweep = json.loads(open(SWEEP).read().strip().splitlines()[-1])
    U = max(sweep["sigmoid"]["max_ulp"], sweep["tanh"]["max_ulp"])
    rng = np.random.default_rng(20250316)
    check_cells(rng)
    ref = reference_namespace()
    g, meta = {}, []
    g["encs"] = np.array(ENCS, np.float64)   # rows: input, hidden, parameters, cell; columns: min, max, bitwidth

    # the reference's quantizer sets, grouping and default states, as data
    structures = {}
    for mode in ("LSTM", "GRU"):
        w = ref["QcQuantizeRecurrent"](make_module(rng, mode, I_SIZE, 5, True), 8, 8, "nearest", None)
        structures[mode] = structure(w)
    g["structure"] = np.array(json.dumps(structures, sort_keys=True))

    for base in CASES:
        for packed in (False, True):
            for state in (False, True):
                case = dict(base, packed=packed, state=state, name="c%d" % len(meta))
                tries = 0
                while True:
                    tries += 1
                    arrays = one_case(ref, rng, case, U)
                    if arrays is not None:
                        break
                    assert tries < 20000, case
                case["tries"] = tries
                for k, v in arrays.items():
                    if k.startswith("w_"):   # multiples of 2^-6 in [-1, 1]: stored as their int8 numerators
                        assert np.array_equal((v * 64).astype(np.int8).astype(F) / 64, v)
                        v = (v * 64).astype(np.int8)
                    g["%s_%s" % (case["name"], k)] = v
                meta.append(case)
                print(case)
    g["cases"] = np.array(json.dumps(meta))
    g["margin"] = np.array([MARGIN, U], np.int64)
    path = os.path.join(HERE, "golden_rnn.npz")
    np.savez_compressed(path, **g)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(g)))


def one_case(ref, rng, case, U):
    mode, H, bf = case["mode"], case["H"], case["batch_first"]
    module = make_module(rng, mode, I_SIZE, H, case["bias"], bf)
    x = grid(rng, (B, T, I_SIZE) if bf else (T, B, I_SIZE), 5, -2, 2)
    arrays = {"x": x}
    for name, p in module.named_parameters():
        arrays["w_" + name] = p.detach().numpy().copy()
    hx = None
    if case["state"]:
        arrays["h0"] = grid(rng, (4, B, H), 7, -1, 0.99)
        hx = torch.from_numpy(arrays["h0"])
        if mode == "LSTM":
            arrays["c0"] = grid(rng, (4, B, H), 4, -2, 2)
            hx = (hx, torch.from_numpy(arrays["c0"]))
    inp = torch.from_numpy(x)
    if case["packed"]:
        arrays["lens"] = np.array(LENS, np.int64)
        if bf:
            for b, n in enumerate(LENS):
                x[b, n:] = 0
        else:
            for b, n in enumerate(LENS):
                x[n:, b] = 0
        inp = pack_padded_sequence(torch.from_numpy(x), torch.tensor(LENS), batch_first=bf, enforce_sorted=False)

    wrapper = ref["QcQuantizeRecurrent"](module, 8, 8, "nearest", None).eval()
    wrapper.set_mode(OpMode.ACTIVE)
    preset(wrapper)
    with torch.no_grad():
        out, hn = wrapper(inp, hx)
    if case["packed"]:
        out, _ = pad_packed_sequence(out, batch_first=bf, total_length=T)
    worst = min(q.worst for n, q in wrapper.grouped_quantizers.items() if n.startswith(("hidden", "cell")))
    if worst < MARGIN * U:
        return None
    arrays["out"] = out.numpy().copy()
    arrays["hn"] = (hn[0] if mode == "LSTM" else hn).numpy().copy()
    if mode == "LSTM":
        arrays["cn"] = hn[1].numpy().copy()
    got = O.run_case(case, arrays, O.RESTATED_FUNCS, ENCS)
    for k, v in zip(("out", "hn", "cn"), got):
        assert v is None or np.array_equal(O.bits(v), O.bits(arrays[k])), (case, k)
    arrays["worst"] = np.array(worst)
    return arrays


if __name__ == "__main__":
    main()
