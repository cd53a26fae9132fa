"""Sequential MSE for blockwise weights, the parts that need no GPU: the fused loss entry point is
exported and declared, BlockwiseQuantizer.set_block_ranges checks its arguments, grouped blockwise
convolutions are left out of the search and a blockwise quantizer never enters the per-channel path.
The kernel and the search are in test_seq_mse_block_gpu.py."""
import os

import pytest
import torch
from torch import nn

import aimet_amd
from aimet_amd import _native
from aimet_amd.blockwise import BlockwiseQuantizer
from aimet_amd.quantsim import QuantizationSimModel
from aimet_amd.seq_mse import SeqMseParams, SequentialMse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blockwise_sim(model, block_size):
    """A sim whose first wrapper carries a hand-made blockwise weight quantizer."""
    sim = QuantizationSimModel(model, quant_scheme="tf", default_param_bw=4)
    old = sim.model[0].param_quantizers["weight"]
    q = BlockwiseQuantizer(model[0].weight.shape, 4, old.round_mode, old.quant_scheme, True, block_size)
    sim.model[0].param_quantizers["weight"] = q
    return sim, q


def test_block_losses_symbol_is_exported_and_declared():
    name = "aimet_bq_seqmse_losses"
    with open(os.path.join(REPO, "include", "aimet_amd.h")) as f:
        assert "int %s(" % name in f.read()
    assert name in _native.EXPORTED_SYMBOLS and hasattr(aimet_amd.native_library(), name)


def test_set_block_ranges_refuses_wrong_lengths_and_a_frozen_quantizer():
    _, q = blockwise_sim(nn.Sequential(nn.Linear(8, 3)), 4)
    assert q.num_encodings == 6
    for n_min, n_max in ((5, 6), (6, 7), (3, 3)):
        with pytest.raises(ValueError, match="6 block minima"):
            q.set_block_ranges(torch.zeros(n_min), torch.ones(n_max))
    assert q.table is None and not q.is_encoding_frozen
    q._is_encoding_frozen = True
    with pytest.raises(RuntimeError, match="frozen"):
        q.set_block_ranges(torch.zeros(6), torch.ones(6))


def test_grouped_blockwise_convs_are_excluded():
    model = nn.Sequential(nn.Conv2d(8, 16, 3, groups=2), nn.Conv2d(16, 4, 1))
    sim, _ = blockwise_sim(model, 2)
    assert SequentialMse._get_grouped_convs_with_blockwise_quantization(model, sim) == [model[0]]
    plain = QuantizationSimModel(model, quant_scheme="tf", default_param_bw=4)
    assert SequentialMse._get_grouped_convs_with_blockwise_quantization(model, plain) == []


def test_blockwise_quantizer_skips_the_per_channel_path(monkeypatch):
    sim, _ = blockwise_sim(nn.Sequential(nn.Linear(8, 3)), 4)
    seen = []

    def per_channel(*_):
        raise AssertionError("the per-channel path was entered")

    monkeypatch.setattr(SequentialMse, "get_per_channel_min_and_max", per_channel)
    monkeypatch.setattr(SequentialMse, "_candidate_losses", per_channel)
    monkeypatch.setattr(SequentialMse, "_optimize_blockwise_module", classmethod(lambda cls, *a: seen.append(a[0])))
    x = torch.zeros(1, 2, 8)
    SequentialMse.optimize_module(sim.model[0], x, x, SeqMseParams(num_batches=1))
    assert seen == [sim.model[0]]
