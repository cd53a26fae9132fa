"""Sequential MSE (aimet_amd/seq_mse.py), the parts that need no GPU: the library exports the
aimet_seqmse_* entry points, the public surface and its defaults, the candidate grid bit for bit,
neg_sqnr, and the argument checks that run before any kernel. The kernels and the end-to-end search
are in test_seq_mse_gpu.py."""
import dataclasses

import numpy as np
import pytest
import torch
from torch import nn

from conftest import bits

import aimet_amd
from aimet_amd import _native, seq_mse
from aimet_amd.activation_sampler import default_forward_fn
from aimet_amd.quantsim import QuantizationSimModel
from aimet_amd.seq_mse import SeqMseParams, SequentialMse

SEQMSE_SYMBOLS = ("aimet_seqmse_candidate_tables", "aimet_seqmse_candidate_qdq", "aimet_seqmse_recon_sums_workspace",
                  "aimet_seqmse_recon_sums")


def test_library_exports_seqmse_symbols():
    lib = aimet_amd.native_library()
    for s in SEQMSE_SYMBOLS:
        assert hasattr(lib, s), "libaimet_amd.so does not export %s" % s
        assert s in _native.EXPORTED_SYMBOLS
    assert sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("aimet_seqmse_")) == sorted(SEQMSE_SYMBOLS)


def test_workspace_query_runs_on_the_host():
    import ctypes
    n = ctypes.c_int64(-1)
    _native.call("aimet_seqmse_recon_sums_workspace", 1024, 48, 1, 20, ctypes.byref(n))
    assert n.value > 0 and n.value % 4 == 0
    with pytest.raises(ValueError):
        _native.call("aimet_seqmse_recon_sums_workspace", 4, 0, 1, 20, ctypes.byref(n))


def test_params_defaults_and_surface():
    p = SeqMseParams(num_batches=4)
    assert dataclasses.asdict(p) == dict(num_batches=4, num_candidates=20, inp_symmetry="symqt", loss_fn="mse",
                                         forward_fn=default_forward_fn)
    assert seq_mse.SUPPORTED_MODULES == (nn.Linear, nn.Conv2d) and seq_mse.SUPPORTED_PARAM_BW == 4
    for name in ("apply_seq_mse", "run_seq_mse", "get_module_inp_acts", "temporarily_disable_quantizers",
                 "compute_all_param_encodings", "get_per_channel_min_and_max", "get_candidates", "optimize_module",
                 "compute_param_encodings", "compute_outputs", "compute_recon_loss"):
        assert callable(getattr(SequentialMse, name)), name
    assert seq_mse.apply_seq_mse == SequentialMse.apply_seq_mse
    assert seq_mse.get_candidates is SequentialMse.get_candidates
    assert seq_mse.optimize_module == SequentialMse.optimize_module
    assert isinstance(seq_mse.CANDIDATE_WINDOW_BYTES, int) and seq_mse.CANDIDATE_WINDOW_BYTES > 0


@pytest.mark.parametrize("n", [1, 7, 20])
@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
def test_get_candidates_is_the_fp32_expression(n, symmetric):
    rng = np.random.default_rng(n)
    mx = np.abs(rng.standard_normal(37)).astype(np.float32)
    mx[3] = 0.0
    mn = None if symmetric else (-np.abs(rng.standard_normal(37))).astype(np.float32)
    cands = seq_mse.get_candidates(n, torch.from_numpy(mx), None if symmetric else torch.from_numpy(mn))
    assert len(cands) == n
    for j, (cand_max, cand_min) in enumerate(cands):
        want_max = (mx / np.float32(n)).astype(np.float32) * np.float32(j + 1)
        want_min = -want_max if symmetric else (mn / np.float32(n)).astype(np.float32) * np.float32(j + 1)
        assert cand_max.dtype == torch.float32 and cand_min.dtype == torch.float32
        np.testing.assert_array_equal(bits(cand_max.numpy()), bits(want_max))
        np.testing.assert_array_equal(bits(cand_min.numpy()), bits(want_min))
        # and the torch expression of the reference, as the CPU evaluates it
        ref = torch.from_numpy(mx) / n * (j + 1)
        np.testing.assert_array_equal(bits(cand_max.numpy()), bits(ref.numpy()))


def test_neg_sqnr_formula():
    g = torch.Generator().manual_seed(1)
    target = torch.randn(50, 6, generator=g, dtype=torch.float64)
    pred = target + 0.01 * torch.randn(50, 6, generator=g, dtype=torch.float64)
    got = seq_mse.neg_sqnr(pred, target)
    noise = ((target - pred) ** 2).mean(0, keepdim=True) + 1e-10
    want = -10 * torch.log10((target ** 2).mean(0, keepdim=True) / noise)
    assert got.shape == (1, 6)
    torch.testing.assert_close(got, want, rtol=0, atol=0)
    assert torch.equal(seq_mse.neg_sqnr(pred, target, reduction="none"), got)


def tiny():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(8, 6), nn.ReLU(), nn.Linear(6, 5)).eval()


def batches(n=2):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(4, 8, generator=g) for _ in range(n)]


def test_invalid_inp_symmetry_and_loss_fn_raise():
    model = tiny()
    sim = QuantizationSimModel(model, quant_scheme="tf", default_param_bw=4)
    with pytest.raises(ValueError, match="inp_symmetry"):
        seq_mse.apply_seq_mse(model, sim, batches(), SeqMseParams(num_batches=2, inp_symmetry="sym"))
    with pytest.raises(ValueError, match="loss function"):
        seq_mse.apply_seq_mse(model, sim, batches(), SeqMseParams(num_batches=2, loss_fn="mae"))
    with pytest.raises(ValueError, match="loss function"):
        SequentialMse.compute_recon_loss(torch.zeros(3, 2), torch.zeros(3, 2), SeqMseParams(2, loss_fn="mae"))
    with pytest.raises(ValueError, match="inp_symmetry"):
        SequentialMse.run_seq_mse([], model, sim.model, SeqMseParams(2, inp_symmetry="x"), default_forward_fn,
                                  batches())


def test_non_tf_sim_raises():
    model = tiny()
    sim = QuantizationSimModel(model, quant_scheme="tf_enhanced", default_param_bw=4)
    flags = [q.enabled for _, w in sim.quant_wrappers() for q in sim._quantizers_of(w)]
    with pytest.raises(AssertionError, match="TF quant-scheme"):
        seq_mse.apply_seq_mse(model, sim, batches(), SeqMseParams(num_batches=2))
    assert flags == [q.enabled for _, w in sim.quant_wrappers() for q in sim._quantizers_of(w)]


def test_checkpoints_config_is_not_implemented():
    model = tiny()
    sim = QuantizationSimModel(model, quant_scheme="tf", default_param_bw=4)
    with pytest.raises(NotImplementedError):
        seq_mse.apply_seq_mse(model, sim, batches(), SeqMseParams(num_batches=2), checkpoints_config="ckpts.json")


def test_quantizers_are_restored_when_the_search_raises():
    """temporarily_disable_quantizers puts every flag back when its body raises."""
    model = tiny()
    sim = QuantizationSimModel(model, quant_scheme="tf", default_param_bw=4)
    quantizers = [q for _, w in sim.quant_wrappers() for q in sim._quantizers_of(w)]
    before = [q.enabled for q in quantizers]
    assert any(before)
    with pytest.raises(RuntimeError, match="boom"):
        with SequentialMse.temporarily_disable_quantizers(model, sim, [model[2]]):
            inside = [q.enabled for q in quantizers]
            raise RuntimeError("boom")
    assert before == [q.enabled for q in quantizers]
    # inside: every activation quantizer and the excluded module's weight quantizer were off
    off =[q for q, was, now in zip(quantizers, before, inside) if was and not now]
    assert sim.model[2].param_quantizers["weight"] in off
    assert sim.model[0].param_quantizers["weight"] not in off
    assert all(q in off for _, w in sim.quant_wrappers() for q in w.input_quantizers + w.output_quantizers
               if before[quantizers.index(q)])
