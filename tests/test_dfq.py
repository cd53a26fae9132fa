"""Data-free quantization on the CPU: the numpy oracle of the DFQ kernels (tests/dfq_oracle.py) against
the reference's own arithmetic (tests/golden/golden_dfq.npz, README_dfq.md), the graph search on CPU
models with the sets stated by hand, and the API's behaviour without a device. No kernel runs here.

`python tests/test_dfq.py` prints the measured oracle-vs-golden distances that README_dfq.md records
and the bounds below are made of."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

from conftest import REPO, bits

import dfq_oracle as O

PAIR_CASES = ["p%d" % i for i in range(7)]
BN_BACKWARD = ["b0", "b1", "b2", "b3"]
HBF_CASES = ["h0", "h1", "h2", "h3"]

# Largest ulp distance between the oracle and the reference golden, measured with numpy 2.2.6
# (tests/golden/README_dfq.md). numpy's float32 np.power(x, 0.5) is not correctly rounded (it is one
# ulp from np.sqrt on about 21 % of values), the quotient carries that on. The tests allow exactly
# these values plus one ulp, for the one further rounding every folded value takes; a scale more
# than 4 ulp off is a wrong formula whatever was measured.
MEASURED_ULP = {"pair_s": 2, "pair_w": 2, "pair_b": 2,
                "triple_s12": 1, "triple_s23": 1, "triple_w": 4, "triple_b": 2}
SCALE_ULP_LIMIT = 4


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "golden_dfq.npz")))


def pair_case(g, n):
    t0, t1 = (bool(v) for v in g[n + "_t"])
    return dict(w0=g[n + "_w0"], b0=g.get(n + "_b0"), w1=g[n + "_w1"], t0=t0, t1=t1)


def bn_case(g, n):
    return (g[n + "_w"], g[n + "_b"], g[n + "_gamma"], g[n + "_beta"], g[n + "_mu"], g[n + "_var"],
            float(g[n + "_eps"]))


def hbf_case(g, n):
    return (g[n + "_gamma"], g[n + "_beta"], g[n + "_s"], bool(g[n + "_relu"]), g[n + "_b1"], g[n + "_w2"],
            g[n + "_b2"])


def measure(g):
    """The figures of README_dfq.md: ulp distances oracle vs golden, and the bias sums' distances to
    the float64 evaluation (golden's and oracle's), per kind of case."""
    m = {k: 0 for k in MEASURED_ULP}
    for n in PAIR_CASES:
        c = pair_case(g, n)
        s, w0, b0, w1 = O.cls_pair(**c)
        m["pair_s"] = max(m["pair_s"], O.ulp_distance(s, g[n + "_s"]))
        m["pair_w"] = max(m["pair_w"], O.ulp_distance(w0, g[n + "_w0_out"]), O.ulp_distance(w1, g[n + "_w1_out"]))
        if b0 is not None:
            m["pair_b"] = max(m["pair_b"], O.ulp_distance(b0, g[n + "_b0_out"]))
    s12, s23, w0, b0, w1, b1, w2 = O.cls_triple(g["t0_w0"], g["t0_b0"], g["t0_w1"], g["t0_b1"], g["t0_w2"])
    m["triple_s12"] = O.ulp_distance(s12, g["t0_s12"])
    m["triple_s23"] = O.ulp_distance(s23, g["t0_s23"])
    m["triple_w"] = max(O.ulp_distance(w0, g["t0_w0_out"]), O.ulp_distance(w1, g["t0_w1_out"]),
                        O.ulp_distance(w2, g["t0_w2_out"]))
    m["triple_b"] = max(O.ulp_distance(b0, g["t0_b0_out"]), O.ulp_distance(b1, g["t0_b1_out"]))
    _, b32, _ = O.bn_fold_forward(*bn_case(g, "b4"))
    _, b64, _ = O.bn_fold_forward(*bn_case(g, "b4"), f64=True)
    m["forward_golden_vs_f64"] = float(np.max(np.abs(g["b4_b_out"] - b64)))
    m["forward_oracle_vs_f64"] = float(np.max(np.abs(b32 - b64)))
    gold = orac = 0.0
    for n in HBF_CASES:
        _, b32, _ = O.bias_fold(*hbf_case(g, n))
        _, b64, _ = O.bias_fold(*hbf_case(g, n), f64=True)
        gold = max(gold, float(np.max(np.abs(g[n + "_b2_out"] - b64))))
        orac = max(orac, float(np.max(np.abs(b32 - b64))))
    m["hbf_golden_vs_f64"], m["hbf_oracle_vs_f64"] = gold, orac
    return m


# ---------------------------------------------------------------------------------------------------
# oracle against the reference golden
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BN_BACKWARD)
def test_oracle_bn_backward_fold_bit_equal(golden, n):
    """Every operation is elementwise fp32 with an IEEE root: the same bits."""
    w, b = O.bn_fold_backward(*bn_case(golden, n))
    assert np.array_equal(bits(w), bits(golden[n + "_w_out"]))
    assert np.array_equal(bits(b), bits(golden[n + "_b_out"]))
    assert np.array_equal(bits(O.bn_scale(golden[n + "_gamma"], golden[n + "_var"], float(golden[n + "_eps"]))),
                          bits(golden[n + "_gamma"] / golden[n + "_sigma"]))
    assert np.any(golden[n + "_gamma"] < 0)
    if n == "b3":   # the layer without a bias: a zero bias made first
        assert int(golden[n + "_flags"][1]) == 0 and not np.any(golden[n + "_b"])


def test_oracle_cls_within_measured_ulps(golden):
    m = measure(golden)
    print("measured:", m)
    for k, want in MEASURED_ULP.items():
        assert m[k] <= want + 1, (k, m[k], want)
    for k in ("pair_s", "triple_s12", "triple_s23"):
        assert m[k] <= SCALE_ULP_LIMIT, "a scale %d ulp off is a wrong formula, not a rounding" % m[k]


def test_oracle_special_channels_scale_exactly_one(golden):
    """An all-zero row (0/0), an all-zero column (x/0) and a channel at 1e-30 in both layers, whose
    product underflows to zero (x/0): all give scale 1, in the reference and in the oracle."""
    s = O.cls_pair(**pair_case(golden, "p6"))[0]
    special = golden["p6_special"]
    assert np.array_equal(bits(s[special]), bits(np.ones(3, np.float32)))
    assert np.array_equal(bits(golden["p6_s"][special]), bits(np.ones(3, np.float32)))
    w0, w1 = golden["p6_w0"], golden["p6_w1"]
    assert not np.any(w0[special[0]]) and not np.any(w1[:, special[1]])
    r0, r1 = np.abs(w0[special[2]]).max(), np.abs(w1[:, special[2]]).max()
    assert r0 > 0 and r1 > 0 and np.float32(r0) * np.float32(r1) == 0
    others = np.setdiff1d(np.arange(s.size), special)
    assert np.all(s[others] != 1)


def test_oracle_forward_fold_and_hbf_bias_vs_float64(golden):
    """The sums: the yardstick is the golden's own float32-vs-float64 difference (the largest over
    the cases of a kind: a single case has five or six outputs, too few for a yardstick of its
    own); the oracle's float32 sums must be within twice that. Weight parts are elementwise."""
    m = measure(golden)
    print("measured:", m)
    assert m["forward_oracle_vs_f64"] <= 2 * m["forward_golden_vs_f64"]
    assert m["hbf_oracle_vs_f64"] <= 2 * m["hbf_golden_vs_f64"]
    w, _, _ = O.bn_fold_forward(*bn_case(golden, "b4"))
    assert np.array_equal(bits(w), bits(golden["b4_w_out"]))
    absorbed = []
    for n in HBF_CASES:
        b1, _, _ = O.bias_fold(*hbf_case(golden, n))
        assert np.array_equal(bits(b1), bits(golden[n + "_b1_out"]))
        if golden[n + "_relu"]:
            absorbed.append(O.absorb(*hbf_case(golden, n)[:4]))
    # with a ReLU some channels absorb a positive amount and some nothing
    assert all(np.any(a > 0) and np.any(a == 0) for a in absorbed) and len(absorbed) == 2


# ---------------------------------------------------------------------------------------------------
# graph search, on CPU models
# ---------------------------------------------------------------------------------------------------
from aimet_amd import batch_norm_fold as BNF  # noqa: E402
from aimet_amd import cross_layer_equalization as CLE  # noqa: E402


def sets_of(model):
    groups = CLE.GraphSearchUtils(model).find_layer_groups_to_scale()
    return [s for grp in groups for s in CLE.GraphSearchUtils.convert_layer_group_to_cls_sets(grp)]


def same_sets(got, want):
    return len(got) == len(want) and all(len(a) == len(b) and all(x is y for x, y in zip(a, b))
                                         for a, b in zip(got, want))


def test_conv_chain_gives_two_pairs():
    c = [nn.Conv2d(3, 8, 3), nn.Conv2d(8, 6, 3), nn.Conv2d(6, 4, 1)]
    m = nn.Sequential(c[0], nn.ReLU(), c[1], nn.ReLU(), c[2])
    assert same_sets(sets_of(m), [(c[0], c[1]), (c[1], c[2])])
    g = CLE.GraphSearchUtils(m)
    assert g.is_relu_activation_present_in_cls_sets([(c[0], c[1]), (c[1], c[2])]) == [True, True]


def test_depthwise_chain_gives_one_triple():
    c = [nn.Conv2d(3, 8, 1), nn.Conv2d(8, 8, 3, groups=8), nn.Conv2d(8, 4, 1)]
    m = nn.Sequential(c[0], nn.PReLU(), c[1], c[2])
    assert same_sets(sets_of(m), [tuple(c)])
    assert CLE.GraphSearchUtils(m).is_relu_activation_present_in_cls_sets([tuple(c)]) == [(True, False)]


class Residual(nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b, self.c, self.d = (nn.Conv2d(4, 4, 3, padding=1) for _ in range(4))
        self.r1, self.r2 = nn.ReLU(), nn.ReLU()

    def forward(self, x):
        y = self.r1(self.a(x))                 # y feeds b and the add: a fan-out
        z = self.c(self.r2(self.b(y)))
        return self.d(z + y)


def test_residual_add_ends_the_chain_at_the_producer():
    m = Residual()
    # a's chain ends at the fan-out; b starts a new one that ends at the add; d stands alone
    assert same_sets(sets_of(m), [(m.b, m.c)])


def test_relu6_blocks_sets_until_replaced():
    c = [nn.Conv2d(3, 8, 3), nn.Conv2d(8, 6, 3)]
    m = nn.Sequential(c[0], nn.ReLU6(), c[1])
    assert sets_of(m) == []
    from aimet_amd import _dfq
    _dfq.replace_modules(m, lambda x: isinstance(x, nn.ReLU6), lambda x: nn.ReLU())   # equalize_model's first step
    assert same_sets(sets_of(m), [(c[0], c[1])])


def test_grouped_conv_restarts_the_chain():
    c = [nn.Conv2d(4, 8, 1), nn.Conv2d(8, 8, 3, groups=2), nn.Conv2d(8, 6, 1), nn.Conv2d(6, 4, 1)]
    m = nn.Sequential(c[0], nn.ReLU(), c[1], nn.ReLU(), c[2], nn.ReLU(), c[3])
    assert same_sets(sets_of(m), [(c[2], c[3])])
    # conv + depthwise with an unsupported third layer: the depthwise one opens the next set
    d = [nn.Conv2d(4, 8, 1), nn.Conv2d(8, 8, 3, groups=8), nn.Conv2d(8, 8, 3, groups=2), nn.Conv2d(8, 4, 1)]
    assert same_sets(CLE.GraphSearchUtils.convert_layer_group_to_cls_sets(list(d)), [])
    e = [nn.Conv2d(8, 8, 3, groups=8), nn.Conv2d(8, 4, 1), nn.Conv2d(4, 4, 1)]
    assert same_sets(CLE.GraphSearchUtils.convert_layer_group_to_cls_sets(list(e)), [(e[0], e[1]), (e[1], e[2])])


def test_resnet50_batch_norm_pairs():
    from workloads.resnet import resnet50
    m = resnet50()
    conv_bn, bn_conv, picked = BNF._find_all_batch_norms_to_fold(m)
    assert len(conv_bn) == 53 and len(bn_conv) == 0 and len(picked) == 53
    assert len({id(bn) for _, bn in conv_bn}) == 53
    assert all(isinstance(c, nn.Conv2d) and isinstance(b, nn.BatchNorm2d) and b.num_features == c.out_channels
               for c, b in conv_bn)
    assert len(BNF.find_all_batch_norms_to_fold(m)) == 53


def test_mobilenet_v2_bn_pairs_and_sets():
    from workloads.mobilenet_v2_bn import mobilenet_v2_bn
    from aimet_amd import _dfq
    m = mobilenet_v2_bn()
    convs = [x for x in m.modules() if isinstance(x, nn.Conv2d)]
    bns = [x for x in m.modules() if isinstance(x, nn.BatchNorm2d)]
    conv_bn, bn_conv, _ = BNF._find_all_batch_norms_to_fold(m)
    assert len(convs) == len(bns) == 52 and not bn_conv
    assert [id(c) for c, _ in conv_bn] == [id(c) for c in convs]      # every conv followed by a BN is paired
    assert all(b.num_features == c.out_channels for c, b in conv_bn)
    g = mobilenet_v2_bn()
    assert all(torch.equal(a.weight.detach(), b.weight.detach()) and torch.equal(a.running_var, b.running_var)
               for a, b in zip(bns, (x for x in g.modules() if isinstance(x, nn.BatchNorm2d))))   # seeded
    gam = torch.cat([b.weight.detach() for b in bns])
    assert gam.min() > 0 and gam.max() / gam.min() > 50 and all(float(b.running_var.min()) > 0 for b in bns)
    # the sets, as equalize_model sees them: ReLU6 replaced, BatchNorms gone (Identity is looked through)
    _dfq.replace_modules(m, lambda x: isinstance(x, nn.ReLU6), lambda x: nn.ReLU())
    _dfq.replace_modules(m, lambda x: isinstance(x, nn.BatchNorm2d), lambda x: nn.Identity())
    sets = sets_of(m)
    assert len(sets) == 19 and sum(len(s) == 3 for s in sets) == 17   # one triple per inverted residual
    for s in sets:
        if len(s) == 2:
            assert s[0].out_channels == s[1].in_channels and s[1].groups == 1
            assert s[0].groups in (1, s[0].in_channels)
        else:
            assert s[0].groups == 1 and s[2].groups == 1
            assert s[1].groups == s[1].in_channels == s[1].out_channels == s[0].out_channels == s[2].in_channels


def test_untraceable_model_points_at_the_explicit_entry_points():
    class Branchy(nn.Module):
        def __init__(self):
            super().__init__()
            self.c = nn.Conv2d(3, 3, 1)

        def forward(self, x):
            return self.c(x) if x.sum() > 0 else x

    with pytest.raises(RuntimeError, match="fold_given_batch_norms"):
        BNF.find_all_batch_norms_to_fold(Branchy())
    with pytest.raises(RuntimeError, match="scale_cls_sets"):
        CLE.GraphSearchUtils(Branchy())


# ---------------------------------------------------------------------------------------------------
# API behaviour
# ---------------------------------------------------------------------------------------------------
def test_is_valid_bn_fold_truth_table():
    v = BNF._is_valid_bn_fold
    assert v(nn.Conv2d(4, 4, 3), True) and v(nn.Conv2d(4, 4, 3, padding=1), True)
    assert v(nn.Conv2d(4, 4, 3, groups=4), True) and v(nn.Linear(4, 4), True) and v(nn.Conv1d(4, 4, 3), True)
    assert v(nn.ConvTranspose2d(4, 4, 3), True) and v(nn.ConvTranspose2d(4, 8, 3, groups=4), True)
    assert not v(nn.ConvTranspose2d(4, 8, 3, groups=2), True)
    assert v(nn.Conv2d(4, 4, 3), False) and v(nn.Linear(4, 4), False) and v(nn.Conv1d(4, 4, 3), False)
    assert not v(nn.Conv2d(4, 4, 3, padding=1), False) and not v(nn.Conv1d(4, 4, 3, padding=1), False)
    assert not v(nn.Conv2d(4, 4, 3, groups=2), False) and not v(nn.Conv2d(4, 4, 3, groups=4), False)
    assert not v(nn.ConvTranspose2d(4, 4, 3), False)
    assert BNF.BatchNormFold._is_valid_bn_fold(nn.Conv2d(4, 4, 3), True)


def test_fold_to_scale_is_not_implemented():
    with pytest.raises(NotImplementedError, match="fold_all_batch_norms_to_scale"):
        BNF.fold_all_batch_norms_to_scale(None)
    assert BNF.fold_all_batch_norms is BNF.fold_all_batch_norms_to_weight


def test_non_fp32_parameters_are_a_type_error():
    m = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.ReLU(), nn.Conv2d(4, 4, 1)).double()
    with pytest.raises(TypeError, match="float32"):
        BNF.fold_all_batch_norms(m)
    assert isinstance(m[1], nn.BatchNorm2d)
    with pytest.raises(TypeError, match="float32"):
        CLE.CrossLayerScaling.scale_cls_set((m[0], m[3]))
    with pytest.raises(TypeError, match="float32"):
        BNF.fold_given_batch_norms(m.half(), [(m[0], m[1])])
    with pytest.raises(ValueError):
        CLE.CrossLayerScaling.scale_cls_set((nn.Linear(3, 3), nn.Linear(3, 3)))


def test_bindings_declare_the_dfq_entry_points():
    from aimet_amd import _native
    want = ["aimet_dfq_bias_fold", "aimet_dfq_bn_fold", "aimet_dfq_cls_pair", "aimet_dfq_cls_triple",
            "aimet_dfq_launch_count"]
    assert sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("aimet_dfq_")) == want
    lib = _native.load()
    assert all(hasattr(lib, s) for s in want)
    # host memory is refused before any launch, and nothing is counted
    from aimet_amd import _dfq
    before = _dfq.launch_count()
    w = np.ones((4, 4), np.float32)
    d = _native.DfqWeightC(w.ctypes.data, 4, 4, 1, 4, 1)
    s = np.zeros(4, np.float32)
    assert lib.aimet_dfq_cls_pair(d, None, d, s.ctypes.data, None) != 0
    bad = _native.DfqWeightC(w.ctypes.data, 4, 4, 1, 5, 1)   # strides that are no layout of a 4x4x1 weight
    assert lib.aimet_dfq_cls_pair(bad, None, bad, s.ctypes.data, None) != 0
    assert _dfq.launch_count() == before and np.all(w == 1)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    for k, v in measure(dict(np.load(os.path.join(REPO, "tests", "golden", "golden_dfq.npz")))).items():
        print("%-24s %r" % (k, v))
