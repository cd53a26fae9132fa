"""QuantAnalyzer on the GPU (csrc/quant_analyzer.hip, aimet_amd/quant_analyzer.py) against tests/qa_oracle.py:

1. aimet_qa_sq_err in fp32 / fp16 / bf16, every load path (equal and different base misalignment, head
   and tail, one workgroup to the grid cap): the float64 bound for double summation in any order,
   repeatability bit for bit, an exact zero, 1e30-scale inputs, accumulation, rejected arguments;
2. the analyzer on a small conv net: per-layer MSE and SQNR against the float64 restatement and the
   reference's literal procedure, an in-place ReLU behind a conv, the number of forwards and launches,
   both sensitivity analyses against toggling by hand, restored `enabled` flags, min/max and histogram
   JSON, analyze() end to end, a CPU-resident model.
Needs an MI355X."""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import gpu_available

import qa_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _native  # noqa: E402
from aimet_amd import quant_analyzer as QA  # noqa: E402
from aimet_amd.qc_quantize_op import QcQuantizeWrapper  # noqa: E402
from aimet_amd.quantizers import QuantScheme  # noqa: E402

DEV = "cuda"
GUARD = 8          # elements: 16 or 32 bytes, so the guard keeps the 16-byte phase
DTYPES = {"fp32": (torch.float32, 0), "fp16": (torch.float16, 1), "bf16": (torch.bfloat16, 2)}

# The launcher's constants (csrc/quant_analyzer.hip, common.hpp): the grid stops growing at
# kMaxStreamBlocks = 2048 workgroups of 256 lanes, reached at kQaVecPerLane = 2 16-byte vectors a lane.
# At AT_CAP elements (16-bit: 8 a vector) the grid is at its cap in every dtype and on both load
# paths, and every lane of every workgroup loops at least twice (fp32: four times).
AT_CAP = 2048 * 256 * 2 * 8 + 4099
SIZES = [1, 3, 4, 255, 256, 257, 1023, 4099, 65541, AT_CAP]
OFFSETS = {"fp32": [(0, 0), (1, 1), (1, 0)],
           "fp16": [(0, 0), (1, 1), (1, 0), (3, 3), (5, 2)],
           "bf16": [(0, 0), (1, 1), (1, 0), (3, 3), (5, 2)]}
KERNEL_CASES = [(n, d, o) for n in SIZES for d in DTYPES for o in OFFSETS[d]]

# Largest relative difference, over the layers of the net below, between the reference's literal
# procedure (tests/qa_oracle.py per_layer_mse_literal: partial forwards, fp32 mse_loss().item()) and its
# float64 restatement (per_layer_mse_f64), measured on an MI355X (tests/golden/README_qa.md); the test
# allows twice that.
MEASURED_MAX_LITERAL_DIFF = 5.217e-08

# Largest relative difference, over the layers of the net below, between the per-layer MSE of a
# CPU-resident copy of the model (its layers run on the host) and of the GPU-resident model, measured on
# an MI355X and its host (tests/golden/README_qa.md); the test allows twice that.
MEASURED_MAX_CPU_GPU_DIFF = 1.310e-07


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def dev_at(values: torch.Tensor, off: int):
    """A device copy of `values` whose first element is `off` elements past a 16-byte boundary, between guards."""
    n = values.numel()
    buf = torch.full((2 * GUARD + off + n,), 777.0, dtype=values.dtype, device=DEV)
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(values)
    assert view.data_ptr() % 16 == (values.element_size() * off) % 16
    return view


@functools.lru_cache(maxsize=4)
def case(n, dtype_name, scale=1.0):
    """(ref, x) host tensors in the dtype and the oracle's sums of them: computed once per (n, dtype)."""
    dtype = DTYPES[dtype_name][0]
    g = torch.Generator().manual_seed(n % 100003 + len(dtype_name))
    ref = (torch.randn(n, generator=g) * 3.0 + 0.5).mul_(scale).to(dtype)
    x = (ref.float() + torch.randn(n, generator=g) * 0.05 * scale).to(dtype)
    return ref, x, O.sq_err(ref, x)


def run(ref, x, dtype_name, offs=(0, 0), scale=1.0, acc0=(0.0, 0.0), n=None):
    """aimet_qa_sq_err into an accumulator that starts at acc0 and sits between guards."""
    acc = torch.tensor([555.0, acc0[0], acc0[1], 555.0], dtype=torch.float64, device=DEV)
    r, v = dev_at(ref, offs[0]), dev_at(x, offs[1])
    _native.call("aimet_qa_sq_err", p(r), p(v), ref.numel() if n is None else n, DTYPES[dtype_name][1], scale,
                 p(acc[1:3]), stream())
    torch.cuda.synchronize()
    h = acc.cpu().numpy()
    assert h[0] == 555.0 and h[3] == 555.0, "wrote outside the accumulator"
    return h[1:3].copy()


# ---------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype_name,offs", KERNEL_CASES,
                         ids=["%d-%s-%d_%d" % (n, d, o[0], o[1]) for n, d, o in KERNEL_CASES])
def test_sq_err(n, dtype_name, offs):
    ref, x, (want_err, want_pow) = case(n, dtype_name)
    scale = 1.0 / n
    first = run(ref, x, dtype_name, offs, scale)
    second = run(ref, x, dtype_name, offs, scale)
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64)), "two runs differ"
    for got, want in zip(first, (want_err * scale, want_pow * scale)):
        print("n=%d %s %s: |got - want| / want = %.3e (allowed %.3e)"
              % (n, dtype_name, offs, abs(got - want) / want, (n + 4) * 2.0 ** -53))
        assert abs(got - want) <= O.bound(n, want)
    # x == ref: an exact zero, and the same second sum
    same = run(ref, ref.clone(), dtype_name, offs, scale)
    assert same[0] == 0.0 and not np.signbit(same[0])
    assert abs(same[1] - want_pow * scale) <= O.bound(n, want_pow * scale)


@pytest.mark.parametrize("dtype_name,magnitude", [("fp32", 1e30), ("bf16", 1e30), ("fp16", 4e3)])
@pytest.mark.parametrize("n", [257, 65541])
def test_sq_err_large_magnitudes(n, dtype_name, magnitude):
    """1e30-scale activations (fp16: near its largest values): fp32 squares would overflow."""
    ref, x, (want_err, want_pow) = case(n, dtype_name, magnitude)
    got = run(ref, x, dtype_name, scale=1.0 / n)
    assert np.all(np.isfinite(got)) and (dtype_name == "fp16" or want_pow > 1e59 * n)
    assert abs(got[0] - want_err / n) <= O.bound(n, want_err / n)
    assert abs(got[1] - want_pow / n) <= O.bound(n, want_pow / n)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_sq_err_accumulates_over_calls(dtype_name):
    acc0 = (37.5, 1234.0)
    acc, want, n_total = acc0, list(acc0), 0
    for n in (4099, 257, 65541):
        ref, x, (e, q) = case(n, dtype_name)
        acc = tuple(run(ref, x, dtype_name, scale=1.0 / n, acc0=acc))
        want = [want[0] + e / n, want[1] + q / n]
        n_total += n + 4
    for got, w, a0 in zip(acc, want, acc0):
        assert abs(got - w) <= (n_total + 4) * 2.0 ** -53 * (w + abs(a0))


def test_sq_err_rejects_bad_arguments():
    lib = _native.load()
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    acc = torch.zeros(4, dtype=torch.float64, device=DEV)
    host = np.zeros(16, np.float32)
    before = QA.launch_count()
    ok = (p(buf), p(buf[16:]))
    assert lib.aimet_qa_sq_err(*ok, 0, 0, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(*ok, -1, 0, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(*ok, (1 << 40) + 1, 0, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(*ok, 16, 3, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(ctypes.c_void_p(buf.data_ptr() + 2), ok[1], 16, 0, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(ok[0], ctypes.c_void_p(buf.data_ptr() + 65), 16, 1, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(*ok, 16, 0, 1.0, ctypes.c_void_p(acc.data_ptr() + 4), None) != 0
    assert lib.aimet_qa_sq_err(ctypes.c_void_p(host.ctypes.data), ok[1], 16, 0, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(*ok, 16, 0, 1.0, ctypes.c_void_p(host.ctypes.data), None) != 0
    torch.cuda.synchronize()
    assert QA.launch_count() == before and torch.all(acc == 0)
    assert lib.aimet_qa_sq_err(*ok, 16, 0, 1.0, p(acc), stream()) == 0
    assert QA.launch_count() == before + QA.LAUNCHES_PER_LAYER_BATCH


# ---------------------------------------------------------------------------------------------------
# the analyzer
# ---------------------------------------------------------------------------------------------------
NAMES = [str(i) for i in range(8)]      # the leaf modules in execution order
WRAPPED = ["0", "2", "7"]               # conv, conv, linear
NUM_BATCHES = 3
PER_CHANNEL = {"defaults": {"ops": {}, "params": {"is_symmetric": "True"}, "per_channel_quantization": "True"}}


def seeded_net(inplace=True):
    """conv - ReLU(inplace) - conv - BN - ReLU - pool - flatten - linear"""
    g = torch.Generator().manual_seed(11)
    net = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(inplace=inplace), nn.Conv2d(8, 8, 3, padding=1),
                        nn.BatchNorm2d(8), nn.ReLU(), nn.MaxPool2d(2), nn.Flatten(), nn.Linear(8 * 8 * 8, 10))
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / m.weight[0].numel()) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.exp(torch.rand(8, generator=g) - 0.5))
                m.bias.copy_(torch.randn(8, generator=g) * 0.3)
                m.running_mean.copy_(torch.randn(8, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(8, generator=g) + 0.5)
    return net.eval()


def batches(device=DEV):
    g = torch.Generator().manual_seed(13)
    return [torch.randn(b, 3, 16, 16, generator=g).to(device) for b in (8, 8, 5)]


def calibrate(model, data):
    for x in data:
        model(x)


def score(model, args):
    """Deterministic eval callback: minus the MSE of the model's outputs against stored ones."""
    data, targets = args
    return -sum(float(((model(x) - t) ** 2).mean()) for x, t in zip(data, targets))


class Setup:
    def __init__(self, inplace=True, device=DEV, scheme=QuantScheme.post_training_tf_enhanced, config=None):
        self.data = batches(device)
        self.model = seeded_net(inplace).to(device)
        self.targets = []
        self.analyzer = QA.QuantAnalyzer(self.model, self.data[0], QA.CallbackFunc(calibrate, self.data),
                                         QA.CallbackFunc(score, (self.data, self.targets)))
        self.analyzer.enable_per_layer_mse_loss(self.data, NUM_BATCHES)
        self.sim = self.analyzer._create_quantsim_and_encodings(scheme, 4, 8, config)
        with torch.no_grad():       # of the model as the analyzer left it: batch norms folded
            self.targets.extend(self.model(x).clone() for x in self.data)

    def quantizers(self):
        return [q for _, w in self.sim.quant_wrappers() for q in O.wrapper_quantizers(w)]


@pytest.fixture(scope="module")
def setup():
    return Setup()


@pytest.fixture(scope="module")
def mse(setup, tmp_path_factory):
    """(the analyzer's per-layer MSE dict, its SQNR file, the float64 restatement)"""
    out = str(tmp_path_factory.mktemp("mse"))
    got = setup.analyzer.export_per_layer_mse_loss(setup.sim, out)
    torch.cuda.synchronize()
    sqnr = json.load(open(os.path.join(out, "per_layer_sqnr.json")))
    assert json.load(open(os.path.join(out, "per_layer_mse_loss.json"))) == got
    return got, sqnr, O.per_layer_mse_f64(setup.model, setup.sim.model, NAMES, setup.data)


def check_against_f64(got, sqnr, want):
    for name in NAMES:
        err, power, samples, elements = want[name]
        loss = err / samples
        print("%s: mse %.6e (float64 restatement %.6e), sqnr %s dB" % (name, got[name], loss, sqnr[name]))
        assert abs(got[name] - loss) <= O.bound(elements, loss), name
        if err == 0.0:
            assert sqnr[name] == "inf"
            continue
        want_db = 10.0 * math.log10(power / err)
        # d(10 log10 r) = 10 / ln 10 * dr / r, the ratio's two sums each within the bound; log10 and the
        # product a few roundings of the result
        allowed = 10.0 / math.log(10.0) * 2 * (elements + 4) * 2.0 ** -53 + 4 * 2.0 ** -53 * abs(want_db)
        assert abs(sqnr[name] - want_db) <= allowed, name


def test_the_net_is_what_the_tests_assume(setup):
    assert [n for n, _ in setup.model.named_modules() if n] == NAMES
    assert isinstance(setup.model[3], nn.Identity), "analyze folds batch norms in place"
    assert [n for n, _ in setup.sim.quant_wrappers()] == WRAPPED
    assert setup.model[1].inplace


def test_per_layer_mse_and_sqnr_equal_the_float64_restatement(mse):
    got, sqnr, want = mse
    assert list(got) == NAMES and list(sqnr) == NAMES
    check_against_f64(got, sqnr, want)
    assert got["0"] > 0.0 and got["7"] > 0.0


def test_per_layer_mse_against_the_references_literal_procedure(setup, mse):
    got, _, want = mse
    literal = O.per_layer_mse_literal(setup.model, setup.sim.model, NAMES, setup.data)
    diffs = {n: abs(literal[n] - want[n][0] / want[n][2]) / (want[n][0] / want[n][2]) for n in NAMES if want[n][0] > 0}
    worst = max(diffs.values())
    print("literal procedure vs float64 restatement: largest relative difference %.3e" % worst)
    for n, d in diffs.items():
        print("  %s %.3e" % (n, d))
    assert worst <= 2 * MEASURED_MAX_LITERAL_DIFF
    for n in diffs:
        assert abs(got[n] - literal[n]) <= 2 * MEASURED_MAX_LITERAL_DIFF * literal[n] + O.bound(want[n][3], got[n]), n


def test_inplace_relu_does_not_change_the_convs_loss(setup, mse, tmp_path):
    got, _, f64 = mse
    plain = Setup(inplace=False)
    assert not plain.model[1].inplace
    want = plain.analyzer.export_per_layer_mse_loss(plain.sim, str(tmp_path))
    for name in NAMES:
        assert abs(got[name] - want[name]) <= O.bound(f64[name][3], want[name]), name


def count_forwards(module, counter, key):
    def hook(*_):
        counter[key] += 1
    return module.register_forward_hook(hook)


@pytest.mark.parametrize("inplace", [True, False])
def test_forwards_and_launches_per_batch(inplace, tmp_path):
    s = Setup(inplace=inplace)
    counter = {"fp32": 0, "sim": 0}
    handles = [count_forwards(s.model, counter, "fp32"), count_forwards(s.sim.model, counter, "sim")]
    before = QA.launch_count()
    try:
        s.analyzer.export_per_layer_mse_loss(s.sim, str(tmp_path))
    finally:
        for h in handles:
            h.remove()
    assert counter["sim"] == NUM_BATCHES
    # the fp32 model also runs once on dummy_input to put the modules in execution order, and, when a
    # kept output was overwritten in place, the first batch once more with that output cloned
    assert counter["fp32"] == NUM_BATCHES + 1 + (1 if inplace else 0)
    assert QA.launch_count() - before == QA.LAUNCHES_PER_LAYER_BATCH * len(NAMES) * NUM_BATCHES


def test_sensitivity_dicts_equal_toggling_by_hand(setup, tmp_path):
    was = [q.enabled for q in setup.quantizers()]
    enabled = setup.analyzer.perform_per_layer_analysis_by_enabling_quant_wrappers(setup.sim, str(tmp_path))
    disabled = setup.analyzer.perform_per_layer_analysis_by_disabling_quant_wrappers(setup.sim, str(tmp_path))
    assert [q.enabled for q in setup.quantizers()] == was
    by_hand = functools.partial(O.sensitivity_by_hand, setup.sim.model, WRAPPED,
                                lambda m: score(m, (setup.data, setup.targets)))
    assert list(enabled) == WRAPPED and list(disabled) == WRAPPED
    assert enabled == by_hand(enable_one=True)          # float equality: bit-equal scores
    assert disabled == by_hand(enable_one=False)
    assert len(set(enabled.values())) == 3 and all(v < 0.0 for v in enabled.values())
    assert json.load(open(tmp_path / "per_layer_quant_enabled.json")) == enabled
    assert json.load(open(tmp_path / "per_layer_quant_disabled.json")) == disabled
    fp32, weights_only, acts_only = setup.analyzer.check_model_sensitivity_to_quantization(setup.sim)
    assert fp32 <= 0.0 and weights_only < fp32 and acts_only < fp32
    assert [q.enabled for q in setup.quantizers()] == was


def test_enabled_flags_survive_a_raising_eval_callback(setup, tmp_path):
    was = [q.enabled for q in setup.quantizers()]
    assert any(was) and not all(was)
    calls = []

    def raising(model, _):
        calls.append(1)
        if len(calls) == 2:
            raise KeyError("second layer")
        return 0.0
    analyzer = QA.QuantAnalyzer(setup.model, setup.data[0], QA.CallbackFunc(calibrate, setup.data),
                                QA.CallbackFunc(raising, None))
    for analysis in (analyzer.perform_per_layer_analysis_by_enabling_quant_wrappers,
                     analyzer.perform_per_layer_analysis_by_disabling_quant_wrappers):
        del calls[:]
        with pytest.raises(KeyError):
            analysis(setup.sim, str(tmp_path))
        assert len(calls) == 2
        assert [q.enabled for q in setup.quantizers()] == was


@pytest.mark.parametrize("config", [None, PER_CHANNEL], ids=["per_tensor", "per_channel"])
def test_min_max_json_equals_the_encodings(config, tmp_path):
    s = Setup(config=config)
    weights, activations = s.analyzer.export_per_layer_encoding_min_max_range(s.sim, str(tmp_path))
    want_w, want_a = {}, {}
    for name, w in s.sim.quant_wrappers():
        for kind, qs in (("input", w.input_quantizers), ("output", w.output_quantizers)):
            for i, q in enumerate(qs):
                if q.enabled:
                    want_a["%s_%s_%d" % (name, kind, i)] = [q.encoding.min, q.encoding.max]
        q = w.param_quantizers["weight"]
        if config is None:
            want_w[name + "_weight"] = [q.encoding.min, q.encoding.max]
        else:
            assert len(q.encoding) == w.get_original_module().weight.shape[0]
            want_w[name + "_weight"] = {"%s_weight_%d" % (name, c): [e.min, e.max] for c, e in enumerate(q.encoding)}
    assert sorted(want_a) == ["0_input_0", "0_output_0", "2_output_0", "7_output_0"]
    assert json.load(open(tmp_path / "min_max_ranges" / "weights.json")) == want_w
    assert json.load(open(tmp_path / "min_max_ranges" / "activations.json")) == want_a
    assert json.loads(json.dumps(weights)) == want_w and json.loads(json.dumps(activations)) == want_a


@pytest.mark.parametrize("config", [None, PER_CHANNEL], ids=["per_tensor", "per_channel"])
def test_histogram_json_equals_get_stats_histogram(config, tmp_path):
    s = Setup(config=config)
    s.analyzer.export_per_layer_stats_histogram(s.sim, str(tmp_path))
    files = 0
    for name, w in s.sim.quant_wrappers():
        entries = [(tmp_path / "weights_pdf" / name / ("%s_weight.json" % name), w.param_quantizers["weight"])]
        entries += [(tmp_path / "activations_pdf" / ("%s_output_q%d.json" % (name, i)), q)
                    for i, q in enumerate(w.output_quantizers)]
        entries += [(tmp_path / "activations_pdf" / ("%s_input_q%d.json" % (name, i)), q)
                    for i, q in enumerate(w.input_quantizers) if q.enabled]
        for path, q in entries:
            got, stem = json.load(open(path)), path.name[:-len(".json")]
            histograms = q.get_stats_histogram()
            encodings = q.encoding if isinstance(q.encoding, list) else [q.encoding]
            assert list(got) == ["%s_%d" % (stem, c) for c in range(len(histograms))]
            for c, (h, e) in enumerate(zip(histograms, encodings)):
                entry = got["%s_%d" % (stem, c)]
                assert entry["xleft"] == [b[0] for b in h] and entry["pdf"] == [b[1] for b in h]
                assert entry["min"] == e.min and entry["max"] == e.max
            files += 1
    assert files == 3 + 3 + 1
    assert not (tmp_path / "activations_pdf" / "2_input_q0.json").exists(), "a quantizer without an encoding"


@pytest.mark.parametrize("scheme", [QuantScheme.post_training_tf_enhanced, QuantScheme.post_training_tf],
                         ids=["tf_enhanced", "tf"])
def test_analyze_end_to_end(scheme, tmp_path):
    data = batches()
    model = seeded_net().to(DEV)
    with torch.no_grad():
        targets = [model(x).clone() for x in data]
    analyzer = QA.QuantAnalyzer(model, data[0], QA.CallbackFunc(calibrate, data), QA.CallbackFunc(score, (data, targets)))
    analyzer.enable_per_layer_mse_loss(data, NUM_BATCHES)
    analyzer.analyze(quant_scheme=scheme, default_param_bw=4, default_output_bw=8, results_dir=str(tmp_path))
    assert isinstance(model[3], nn.Identity) and not any(isinstance(m, QcQuantizeWrapper) for m in model.modules())
    for name in ("per_layer_quant_enabled.json", "per_layer_quant_disabled.json", "per_layer_mse_loss.json",
                 "per_layer_sqnr.json", os.path.join("min_max_ranges", "weights.json"),
                 os.path.join("min_max_ranges", "activations.json")):
        assert json.load(open(tmp_path / name)), name
    assert list(json.load(open(tmp_path / "per_layer_mse_loss.json"))) == NAMES
    if scheme == QuantScheme.post_training_tf:
        assert not (tmp_path / "activations_pdf").exists() and not (tmp_path / "weights_pdf").exists()
    else:
        assert (tmp_path / "activations_pdf" / "0_output_q0.json").exists()
        assert (tmp_path / "weights_pdf" / "7" / "7_weight.json").exists()


def test_cpu_resident_model(mse, tmp_path):
    """The analyzer on a CPU-resident copy: its layers run where the model lives, the reduction on the
    device. The dict is the same, within the bound, as the float64 restatement gives on that same copy.
    The layers' fp32 arithmetic on the host is not the GPU's (other kernels, other summation orders, and
    a quantizer turns a last-bit difference of an activation into a whole step), so the double bound
    does not hold against the GPU-resident dict: that difference was measured, and twice the measured
    figure is allowed, as for the literal procedure."""
    on_gpu, _, _ = mse
    s = Setup(device="cpu")
    assert all(not t.is_cuda for t in s.model.parameters())
    got = s.analyzer.export_per_layer_mse_loss(s.sim, str(tmp_path))
    sqnr = json.load(open(tmp_path / "per_layer_sqnr.json"))
    check_against_f64(got, sqnr, O.per_layer_mse_f64(s.model, s.sim.model, NAMES, s.data, device=DEV))
    for name in NAMES:
        print("%s: CPU-resident %.9e, GPU-resident %.9e, relative difference %.3e"
              % (name, got[name], on_gpu[name], abs(got[name] - on_gpu[name]) / on_gpu[name]))
        assert abs(got[name] - on_gpu[name]) <= 2 * MEASURED_MAX_CPU_GPU_DIFF * on_gpu[name], name
