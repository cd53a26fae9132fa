"""QuantAnalyzer without a GPU: the bindings of csrc/quant_analyzer.hip, tests/qa_oracle.py against closed
forms, and the argument checks that need no device."""
import ctypes

import numpy as np
import pytest
import torch

import qa_oracle as O


def test_bindings_declare_the_two_entry_points():
    from aimet_amd import _native
    want = ["aimet_qa_launch_count", "aimet_qa_sq_err"]
    assert sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("aimet_qa_")) == want
    lib = _native.load()
    assert all(hasattr(lib, s) for s in want)


def test_exported_from_the_package():
    import aimet_amd
    from aimet_amd import quant_analyzer as QA
    assert aimet_amd.QuantAnalyzer is QA.QuantAnalyzer and aimet_amd.CallbackFunc is QA.CallbackFunc
    for method in ("analyze", "enable_per_layer_mse_loss", "check_model_sensitivity_to_quantization",
                   "perform_per_layer_analysis_by_enabling_quant_wrappers",
                   "perform_per_layer_analysis_by_disabling_quant_wrappers",
                   "export_per_layer_encoding_min_max_range", "export_per_layer_stats_histogram",
                   "export_per_layer_mse_loss"):
        assert callable(getattr(QA.QuantAnalyzer, method))


@pytest.mark.parametrize("n", [1, 3, 257, 4099])
@pytest.mark.parametrize("r,x", [(1.5, 0.25), (-3.0, 5.0), (1e30, -1e30), (0.1, 0.1)])
def test_oracle_constant_tensors(n, r, x):
    err, power = O.sq_err(np.full(n, r), np.full(n, x))
    d = float(r) - float(x)
    # n equal float64 terms, each rounded once; fsum adds one rounding, the closed form here two
    assert abs(err - n * (d * d)) <= 4 * 2.0 ** -53 * n * d * d
    assert abs(power - n * (float(r) * float(r))) <= 4 * 2.0 ** -53 * n * float(r) ** 2
    assert np.isfinite(err) and np.isfinite(power)
    if n == 1:
        assert err == d * d and power == float(r) * float(r)


def test_oracle_equal_tensors_give_exactly_zero():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(1000).astype(np.float32)
    err, power = O.sq_err(a, a.copy())
    assert err == 0.0 and power > 0.0
    err, _ = O.sq_err(torch.from_numpy(a).to(torch.bfloat16), torch.from_numpy(a).to(torch.bfloat16))
    assert err == 0.0


def test_oracle_widens_before_subtracting():
    """float32 1e30 - (-1e30) overflows nothing in double; 16-bit values are taken as stored."""
    err, _ = O.sq_err(np.array([3e38], np.float32), np.array([-3e38], np.float32))
    assert np.isfinite(err) and err == (2.0 * float(np.float32(3e38))) ** 2
    h = torch.tensor([0.1], dtype=torch.float16)
    _, power = O.sq_err(h, h)
    assert power == float(h.double()[0]) ** 2


def test_callbacks_must_be_wrapped():
    from aimet_amd.quant_analyzer import CallbackFunc, QuantAnalyzer
    model, dummy = torch.nn.Linear(2, 2), torch.zeros(1, 2)
    ok = CallbackFunc(lambda m, a: 0.0, None)
    with pytest.raises(ValueError, match="forward_pass_callback"):
        QuantAnalyzer(model, dummy, lambda m, a: None, ok)
    with pytest.raises(ValueError, match="eval_callback"):
        QuantAnalyzer(model, dummy, ok, lambda m, a: 0.0)
    analyzer = QuantAnalyzer(model, dummy, ok, CallbackFunc(lambda m, a: 1.0, func_callback_args=3))
    assert analyzer._eval_callback.args == 3 and analyzer._forward_pass_callback.args is None


def test_enable_per_layer_mse_loss_needs_enough_batches():
    from aimet_amd.quant_analyzer import CallbackFunc, QuantAnalyzer
    ok = CallbackFunc(lambda m, a: 0.0, None)
    analyzer = QuantAnalyzer(torch.nn.Linear(2, 2), torch.zeros(1, 2), ok, ok)
    data = [torch.zeros(1, 2)] * 3
    with pytest.raises(ValueError, match="Can not fetch 4 batches"):
        analyzer.enable_per_layer_mse_loss(data, 4)
    analyzer.enable_per_layer_mse_loss(data, 3)
    assert analyzer._num_batches == 3


def test_unsupported_quant_scheme():
    from aimet_amd.quant_analyzer import CallbackFunc, QuantAnalyzer
    from aimet_amd.quantizers import QuantScheme
    ok = CallbackFunc(lambda m, a: 0.0, None)
    analyzer = QuantAnalyzer(torch.nn.Linear(2, 2), torch.zeros(1, 2), ok, ok)
    with pytest.raises(ValueError, match="post_training_tf"):
        analyzer.analyze(quant_scheme=QuantScheme.post_training_percentile)


def test_bad_kernel_arguments_return_non_zero():
    from aimet_amd import _native
    from aimet_amd import quant_analyzer as QA
    lib = _native.load()
    before = QA.launch_count()
    r, x, acc = np.ones(16, np.float32), np.zeros(16, np.float32), np.zeros(2, np.float64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    assert lib.aimet_qa_sq_err(p(r), p(x), 0, 0, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(p(r), p(x), -5, 0, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(p(r), p(x), (1 << 40) + 1, 0, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(p(r), p(x), 16, 3, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(p(r), p(x), 16, -1, 1.0, p(acc), None) != 0
    assert lib.aimet_qa_sq_err(p(r), p(x), 16, 0, 1.0, p(acc), None) != 0      # host memory
    assert lib.aimet_qa_sq_err(None, p(x), 16, 0, 1.0, p(acc), None) != 0
    assert QA.launch_count() == before and np.all(acc == 0)
    with pytest.raises(ValueError):
        QA.add_sq_err(torch.zeros(4), torch.zeros(5), 1.0, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError):
        QA.add_sq_err(torch.zeros(4), torch.zeros(4), 1.0, torch.zeros(2, dtype=torch.float64))   # host tensors
