"""BatchNorm re-estimation and BN fold to scale without a device: the oracle against the fixture
written from the reference (tests/golden/README_bnre.md), the bindings, and the pair search on a
sim's fx trace with the quantization wrappers as leaves."""
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import REPO

import bnre_oracle as O
from aimet_amd import _native
from aimet_amd import batch_norm_fold as BNF
from aimet_amd import bn_reestimation as BNRE
from aimet_amd.quantizers import QuantScheme
from aimet_amd.quantsim import DEFAULT_QUANTIZABLE_TYPES, QuantizationSimModel

F = np.float32
PER_CHANNEL_CFG = {"defaults": {"ops": {"is_output_quantized": "True"},
                                "params": {"is_quantized": "True", "is_symmetric": "True"},
                                "strict_symmetric": "False", "per_channel_quantization": "True"}}
BN_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "golden_bnre.npz")))


def config_file(tmp_path, cfg=PER_CHANNEL_CFG):
    import json
    path = tmp_path / "quantsim_config.json"
    path.write_text(json.dumps(cfg))
    return str(path)


def tiny_sim(golden, tmp_path, device="cpu", scheme=QuantScheme.training_range_learning_with_tf_init, cfg=PER_CHANNEL_CFG):
    return QuantizationSimModel(O.tiny_net(golden, device=device), quant_scheme=scheme, in_place=True,
                                config_file=config_file(tmp_path, cfg),
                                quantizable_types=DEFAULT_QUANTIZABLE_TYPES + BN_TYPES)


def test_oracle_reproduces_the_reference_on_the_cpu(golden):
    net = O.tiny_net(golden)
    O.reestimate_torch(net, O.tiny_batches(golden))
    for n in O.BN_NAMES:
        bn = getattr(net, n)
        assert np.array_equal(bn.running_mean.numpy().view(np.uint32), golden["ref_%s_mean" % n].view(np.uint32)), n
        assert np.array_equal(bn.running_var.numpy().view(np.uint32), golden["ref_%s_var" % n].view(np.uint32)), n
        assert int(bn.num_batches_tracked) == int(golden["ref_%s_tracked" % n]) == 3
        assert bn.momentum == 0.1 and bn.training   # as before the call


def test_fold_scale_oracle_matches_the_fixture_and_swaps_negative_channels(golden):
    for k in (0, 1):
        g = {key[4:]: v for key, v in golden.items() if key.startswith("fs%d_" % k)}
        w, b, lo, hi, bad = O.fold_scale(g["w"], g["b"], g["gamma"], g["beta"], g["mean"], g["var"], float(g["eps"]),
                                         g["enc_min"], g["enc_max"])
        assert not bad
        for got, key in ((w, "w_out"), (b, "b_out"), (lo, "min_out"), (hi, "max_out")):
            assert np.array_equal(got.view(np.uint32), g[key].view(np.uint32)), key
        neg = g["gamma"] < 0
        assert neg.sum() == 1 and np.all(lo <= hi)
        c = g["gamma"] / np.sqrt(g["var"] + F(g["eps"]))
        assert np.array_equal(lo[neg], (g["enc_max"] * c)[neg]) and np.array_equal(hi[neg], (g["enc_min"] * c)[neg])
    # a channel without a spread is left alone and reported
    out = O.fold_scale(np.ones((2, 3), F), np.zeros(2, F), np.ones(2, F), np.zeros(2, F), np.zeros(2, F),
                       np.array([0, 1], F), 0.0, -np.ones(2, F), np.ones(2, F))
    assert out[4] and np.all(out[0][0] == 1) and out[2][0] == -1 and out[3][0] == 1


def test_modules_import_and_bindings_declare_the_entry_points():
    want = ["aimet_bnre_finish", "aimet_bnre_fold_scale", "aimet_bnre_forward", "aimet_bnre_forward_form",
            "aimet_bnre_launch_count"]
    assert sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("aimet_bnre_")) == want
    lib = _native.load()
    assert all(hasattr(lib, s) for s in want)
    assert callable(BNRE.reestimate_bn_stats) and callable(BNF.prepare_for_fold_to_scale)
    assert BNF.BatchNormFold.fold_all_batch_norms_to_scale is BNF.fold_all_batch_norms_to_scale
    assert BNF.BatchNormFold.prepare_for_fold_to_scale is BNF.prepare_for_fold_to_scale
    calls = []
    h = BNRE.Handle(lambda: calls.append(1))
    h.remove()
    h.remove()
    assert calls == [1]


def test_entry_points_reject_host_memory():
    """No CPU path: host pointers are refused before any launch and nothing is counted or written."""
    lib = _native.load()
    before = BNRE.launch_count()
    x = np.ones((2, 4, 2), F)
    y = np.zeros_like(x)
    acc = np.zeros((2, 4), np.float64)
    assert lib.aimet_bnre_forward(x.ctypes.data, 2, 4, 2, None, None, 1e-5, y.ctypes.data, acc[0].ctypes.data,
                                  acc[1].ctypes.data, None) != 0
    rm, rv = np.zeros(4, F), np.zeros(4, F)
    job = (_native.BnreFinishJobC * 1)()
    job[0].sum_mean, job[0].sum_var = acc[0].ctypes.data, acc[1].ctypes.data
    job[0].running_mean, job[0].running_var, job[0].C, job[0].count = rm.ctypes.data, rv.ctypes.data, 4, 2.0
    assert lib.aimet_bnre_finish(job, 1, None) != 0
    w, v = np.ones((4, 4), F), np.ones(4, F)
    status = np.zeros(1, np.int32)
    fold = (_native.BnreFoldScaleJobC * 1)()
    fold[0].fold.w = _native.DfqWeightC(w.ctypes.data, 4, 4, 1, 4, 1)
    fold[0].fold.bias = fold[0].fold.gamma = fold[0].fold.beta = fold[0].fold.mean = fold[0].fold.var = v.ctypes.data
    fold[0].fold.eps, fold[0].fold.forward = 1e-5, 0
    fold[0].enc_min, fold[0].enc_max = rm.ctypes.data, rv.ctypes.data
    assert lib.aimet_bnre_fold_scale(fold, 1, status.ctypes.data, None) != 0
    assert BNRE.launch_count() == before
    assert np.all(y == 0) and np.all(acc == 0) and np.all(w == 1) and np.all(rm == 0) and status[0] == 0


def test_fold_to_scale_wants_a_sim():
    with pytest.raises(NotImplementedError, match="takes a QuantizationSimModel, got object"):
        BNF.fold_all_batch_norms_to_scale(object())


def test_pair_search_with_wrappers_as_leaves(golden, tmp_path):
    sim = tiny_sim(golden, tmp_path)
    m = sim.model
    pairs = BNF._find_scale_pairs(sim)
    assert [(id(a), id(b)) for a, b in pairs] == [(id(m.conv1), id(m.bn1)), (id(m.conv2), id(m.bn2)),
                                                  (id(m.fc), id(m.bn3))]
    assert all(isinstance(a._module_to_wrap, (nn.Conv2d, nn.Linear)) for a, _ in pairs)
    # the default search (no leaf predicate) is what it was: the bare modules of a bare model
    bare = BNF.find_all_batch_norms_to_fold(O.TinyNet())
    assert [type(a) for a, _ in bare] == [nn.Conv2d, nn.Conv2d, nn.Linear]
    # prepare switches off what a Conv + BatchNorm supergroup would
    assert BNF.prepare_for_fold_to_scale(sim) == pairs
    for conv, bn in pairs:
        assert not any(q.enabled for q in conv.output_quantizers)
        assert not any(q.enabled for q in bn.param_quantizers.values())
        assert all(q.enabled for q in bn.output_quantizers)
        assert conv.param_quantizers["weight"].enabled


def test_pair_search_leaves_alone_what_is_no_pair(tmp_path):
    class Fan(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.bn, self.other = nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4), nn.Conv2d(4, 4, 1)

        def forward(self, x):
            y = self.conv(x)
            return self.bn(y) + self.other(y)   # the conv's output has two users
    sim = QuantizationSimModel(Fan(), quant_scheme=QuantScheme.training_range_learning_with_tf_init,
                               config_file=config_file(tmp_path), quantizable_types=DEFAULT_QUANTIZABLE_TYPES + BN_TYPES)
    assert BNF._find_scale_pairs(sim) == []


def test_pair_search_raises_on_forward_fold(tmp_path):
    net = nn.Sequential(nn.BatchNorm2d(3), nn.Conv2d(3, 4, 1))
    sim = QuantizationSimModel(net, quant_scheme=QuantScheme.training_range_learning_with_tf_init,
                               config_file=config_file(tmp_path), quantizable_types=DEFAULT_QUANTIZABLE_TYPES + BN_TYPES)
    with pytest.raises(RuntimeError, match="Forward folding to scale is not possible"):
        BNF._find_scale_pairs(sim)
    with pytest.raises(RuntimeError, match="Forward folding to scale is not possible"):
        BNF.fold_all_batch_norms_to_scale(sim)


def test_without_a_device_reestimation_raises(golden, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    net = O.tiny_net(golden)
    with pytest.raises(RuntimeError, match="no CPU path"):
        BNRE.reestimate_bn_stats(net, O.tiny_batches(golden))
    assert np.array_equal(net.bn1.running_mean.numpy(), golden["param_bn1.running_mean"])
