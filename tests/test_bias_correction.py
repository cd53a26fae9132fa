"""Bias correction on the CPU: the float64 oracle of the kernels (tests/bc_oracle.py) against the
reference's own arithmetic (tests/golden/golden_bc.npz, README_bc.md), the graph search on CPU models,
and the API's behaviour without a device and on non-fp32 parameters. No kernel runs here."""
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import REPO

import bc_oracle as O

EMPIRICAL = ["e%d" % i for i in range(6)]
ANALYTICAL = ["a%d" % i for i in range(5)]
ACTS = ("none", "relu", "relu6")
F = np.float32


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "golden_bc.npz")))


def empirical_case(g, n):
    ref = g[n + "_ref"]
    q = ref + g[n + "_qdiff"].astype(F)
    N, C = ref.shape[:2]
    return ref.reshape(N, C, -1), q.reshape(N, C, -1), g[n + "_bias"]


def analytical_case(g, n):
    """(w, wq, bias, gamma, beta, transposed) in module layout."""
    w = g[n + "_wcode"].astype(F) / F(16.0) if n + "_wcode" in g else g[n + "_w"]
    wq = g[n + "_qcode"].astype(F) * F(g[n + "_delta"])
    return w, wq, g[n + "_bias"], g[n + "_gamma"], g[n + "_beta"], bool(g[n + "_t"])


# ---------------------------------------------------------------------------------------------------
# oracle against the reference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EMPIRICAL)
def test_oracle_empirical_within_the_references_own_error(golden, n):
    """The reference subtracts and averages in float32; its distance from its own float64 evaluation is
    recorded per case (README_bc.md). The oracle may be that far from the golden plus one fp32 ulp."""
    ref, q, bias = empirical_case(golden, n)
    rs, _ = O.channel_sums(ref)
    qs, _ = O.channel_sums(q)
    got32, got = O.apply_empirical(bias, rs, qs, ref.shape[0] * ref.shape[2])
    bound = float(golden[n + "_dist"]) + 2 * O.half_ulp32(got)
    assert np.all(np.abs(got - golden[n + "_out"].astype(np.float64)) <= bound)
    assert np.all(np.abs(got - golden[n + "_out64"]) <= 2 * O.half_ulp32(got))
    assert np.all(np.abs(got32.astype(np.float64) - got) <= O.half_ulp32(got))


@pytest.mark.parametrize("act", range(3), ids=ACTS)
@pytest.mark.parametrize("n", ANALYTICAL)
def test_oracle_analytical_within_the_references_own_error(golden, n, act):
    w, wq, bias, gamma, beta, t = analytical_case(golden, n)
    _, got, terms = O.analytical(w, wq, bias, gamma, beta, act, t)
    assert np.all(np.isfinite(got)), "gamma == 0 with beta != 0 has a finite IEEE result"
    bound = float(golden["%s_dist_%s" % (n, ACTS[act])]) + 2 * O.half_ulp32(got)
    assert np.all(np.abs(got - golden["%s_out_%s" % (n, ACTS[act])]) <= bound)
    assert np.all(np.abs(got - golden["%s_out64_%s" % (n, ACTS[act])]) <= 2 * O.half_ulp32(got))


def test_oracle_expected_input_special_channels():
    """gamma == 0: the distribution is a point at beta; a negative gamma is used as given."""
    beta = np.array([0.75, -0.75, 7.0], F)
    zero = np.zeros(3, F)
    assert np.array_equal(O.expected_input(beta, zero, O.RELU), [0.75, 0.0, 7.0])
    assert np.array_equal(O.expected_input(beta, zero, O.RELU6), [0.75, 0.0, 6.0])
    pos, neg = O.expected_input([0.3], [0.5], O.RELU), O.expected_input([0.3], [-0.5], O.RELU)
    assert pos[0] > 0.3 and neg[0] != pos[0]
    # a wide clipped normal centred in [0, 6] has mean 3
    assert abs(O.expected_input([3.0], [2.0], O.RELU6)[0] - 3.0) < 1e-12


# ---------------------------------------------------------------------------------------------------
# graph search
# ---------------------------------------------------------------------------------------------------
class Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.c1, self.b1, self.r1 = nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU()
        self.c2, self.b2, self.r2 = nn.Conv2d(8, 8, 3, padding=1, groups=8), nn.BatchNorm2d(8), nn.ReLU6()
        self.c3 = nn.Conv2d(8, 8, 1)
        self.b3, self.h3 = nn.BatchNorm2d(8), nn.Hardtanh(0, 6)
        self.t4 = nn.ConvTranspose2d(8, 4, 2)
        self.b4 = nn.BatchNorm2d(4)
        self.c5, self.c6 = nn.Conv2d(4, 4, 1), nn.Conv2d(4, 4, 1)
        self.b7 = nn.BatchNorm1d(4)
        self.fc = nn.Linear(4, 3)

    def forward(self, x):
        x = self.r1(self.b1(self.c1(x)))
        x = self.r2(self.b2(self.c2(x)))
        x = self.h3(self.b3(self.c3(x)))
        y = self.b4(self.t4(x))             # fans out: feeds c5 and c6
        x = self.c5(y) + self.c6(y)
        return self.fc(self.b7(x.mean((2, 3))))


def test_search_on_a_small_model():
    from aimet_amd import bias_correction as BC
    m = Small().eval()
    d = BC.find_all_conv_bn_with_activation(m, (1, 3, 8, 8))
    assert set(d) == {m.c1, m.c2, m.c3, m.t4, m.c5, m.c6, m.fc}
    A = BC.ActivationType
    assert d[m.c1].input_bn is None and d[m.c1].output_bn.get_module() is m.b1
    assert d[m.c2].input_bn.get_module() is m.b1 and d[m.c2].in_activation_type == A.relu
    assert d[m.c3].input_bn.get_module() is m.b2 and d[m.c3].in_activation_type == A.relu6
    assert d[m.c3].output_bn.get_module() is m.b3
    assert d[m.t4].input_bn.get_module() is m.b3 and d[m.t4].in_activation_type == A.relu6   # Hardtanh(0, 6)
    assert d[m.t4].output_bn.get_module() is m.b4
    # the fan-out behind b4 breaks the match
    for c in (m.c5, m.c6):
        assert d[c].input_bn is None and d[c].in_activation_type == A.no_activation and d[c].output_bn is None
    # a BatchNorm before a Linear is not an input BN
    assert d[m.fc].input_bn is None and d[m.fc].output_bn is None


def test_search_bn_to_conv_without_activation_and_other_hardtanh():
    from aimet_amd import bias_correction as BC
    m = nn.Sequential(nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4), nn.Conv2d(4, 4, 1), nn.BatchNorm2d(4), nn.Hardtanh(-1, 1),
                      nn.Conv2d(4, 2, 1)).eval()
    d = BC.find_all_conv_bn_with_activation(m, None)
    assert d[m[2]].input_bn.get_module() is m[1] and d[m[2]].in_activation_type == BC.ActivationType.no_activation
    assert d[m[5]].input_bn is None, "Hardtanh(-1, 1) is no ReLU6"


def test_search_on_mobilenet_v2_bn_and_the_dict_outlives_the_fold():
    from aimet_amd import bias_correction as BC
    from workloads.mobilenet_v2_bn import mobilenet_v2_bn
    m = mobilenet_v2_bn()
    d = BC.find_all_conv_bn_with_activation(m, (1, 3, 224, 224))
    convs = [x for x in m.modules() if isinstance(x, nn.Conv2d)]
    assert len(d) == len(convs) + 1 and m.classifier in d
    g = BC._dfq.TracedGraph(m)
    fed_by_relu6 = 0
    for conv in convs:
        node = g.node_of(conv)
        src = node.args[0]
        if isinstance(g.module(src), nn.ReLU6) and len(src.users) == 1:
            bn = g.module(src.args[0])
            assert isinstance(bn, nn.BatchNorm2d)
            assert d[conv].input_bn.get_module() is bn and d[conv].in_activation_type == BC.ActivationType.relu6
            fed_by_relu6 += 1
        assert d[conv].output_bn is not None
    assert fed_by_relu6 >= 30
    assert d[convs[0]].input_bn is None
    assert d[m.classifier].input_bn is None and d[m.classifier].output_bn is None
    # the entry holds the module, not a place in the model
    held = d[convs[1]].input_bn.get_module()
    first_bn_name = next(n for n, x in m.named_modules() if x is held)
    parent, _, leaf = first_bn_name.rpartition(".")
    setattr(m.get_submodule(parent), leaf, nn.Identity())
    assert d[convs[1]].input_bn.get_module() is held and held.weight.numel() == convs[1].weight.shape[0]


# ---------------------------------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------------------------------
def test_names_of_the_reference_module():
    from aimet_amd import bias_correction as BC
    from aimet_amd import quantsim
    for name in ("correct_bias", "find_all_conv_bn_with_activation", "call_empirical_correct_bias",
                 "call_analytical_correct_bias", "get_quantized_dequantized_weight", "StopForwardException",
                 "forward_pass", "ConvBnInfoType", "ActivationType", "QuantParams"):
        assert hasattr(BC, name), name
    assert BC.QuantParams is quantsim.QuantParams
    p = BC.QuantParams(weight_bw=4)
    assert p._fields == ("weight_bw", "act_bw", "round_mode", "quant_scheme", "config_file")
    assert (p.weight_bw, p.act_bw, p.round_mode, p.config_file) == (4, 8, "nearest", None)
    assert [a.value for a in BC.ActivationType] == [0, 1, 2]
    info = BC.ConvBnInfoType()
    assert info.input_bn is None and info.in_activation_type == BC.ActivationType.no_activation


def loader(n=2, bs=2):
    g = torch.Generator().manual_seed(0)
    return [(torch.randn(bs, 3, 8, 8, generator=g), torch.zeros(bs)) for _ in range(n)]


def test_without_a_device_everything_raises(monkeypatch):
    from aimet_amd import bias_correction as BC
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = nn.Sequential(nn.Conv2d(3, 4, 3), nn.ReLU(), nn.Conv2d(4, 2, 1)).eval()
    before = [p.detach().clone() for p in m.parameters()]
    with pytest.raises(RuntimeError, match="no CPU path"):
        BC.correct_bias(m, BC.QuantParams(weight_bw=4), 4, loader(), 4)
    assert all(torch.equal(a, b) for a, b in zip(before, m.parameters()))
    assert not any(isinstance(x, BC.QcQuantizeWrapper) for x in m.modules())
    x = torch.randn(2, 4, 6, 6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        BC.call_empirical_correct_bias(m[0], x, x + 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        BC._add_channel_sums(m[0], x, torch.zeros(4, dtype=torch.float64))


def test_fp16_parameters_are_a_type_error():
    from aimet_amd import bias_correction as BC
    m = nn.Sequential(nn.Conv2d(3, 4, 3), nn.ReLU(), nn.Conv2d(4, 2, 1)).half().eval()
    with pytest.raises(TypeError, match="float32"):
        BC.correct_bias(m, BC.QuantParams(), 4, loader(), 4)
    with pytest.raises(TypeError, match="float32"):
        BC.call_empirical_correct_bias(m[0], torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2))
    with pytest.raises(TypeError, match="float32"):
        BC._as_outer_c_inner(m[0], torch.zeros(1, 4, 2, 2, dtype=torch.float16))


def test_bindings_declare_the_bias_correction_entry_points():
    from aimet_amd import _native
    from aimet_amd import bias_correction as BC
    want = ["aimet_bc_analytical", "aimet_bc_apply_empirical", "aimet_bc_channel_sums", "aimet_bc_launch_count"]
    assert sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("aimet_bc_")) == want
    lib = _native.load()
    assert all(hasattr(lib, s) for s in want)
    # host memory is refused before any launch, and nothing is counted
    before = BC.launch_count()
    x, acc = np.ones(16, F), np.zeros(4, np.float64)
    assert lib.aimet_bc_channel_sums(x.ctypes.data, 2, 4, 2, acc.ctypes.data, None) != 0
    b = np.zeros(4, F)
    assert lib.aimet_bc_apply_empirical(b.ctypes.data, acc.ctypes.data, acc.ctypes.data, 4, 8.0, None) != 0
    job = (_native.BcAnalyticalJobC * 1)()
    job[0].w = _native.DfqWeightC(x.ctypes.data, 4, 4, 1, 4, 1)
    job[0].wq, job[0].bias = x.ctypes.data, b.ctypes.data
    assert lib.aimet_bc_analytical(job, 1, None) != 0
    assert BC.launch_count() == before and np.all(acc == 0) and np.all(b == 0)
