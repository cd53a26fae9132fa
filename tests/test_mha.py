"""Quantizable multi-head attention without a device: the oracle (tests/mha_oracle.py) against the
fixture written from the reference (tests/golden/make_golden_mha.py) and against torch's CPU softmax,
the bindings, the float equivalence of the converted modules, what the sim wraps, the refusals and the
cache of the float-mask check."""
import copy
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import REPO

import mha_oracle as O
from aimet_amd import _native
from aimet_amd import transformers as T
from aimet_amd.elementwise_ops import TRANSFORMER_QUANTIZABLE_TYPES, Add, Divide, MatMul
from aimet_amd.qc_quantize_op import StaticGridQuantWrapper
from aimet_amd.quantsim import DEFAULT_QUANTIZABLE_TYPES, QuantizationSimModel

F = np.float32
MHA_CHILDREN = ["linear_Q", "linear_K", "linear_V", "out_proj", "div", "matmul_1", "matmul_2", "softmax"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "golden_mha.npz"))


def cases(golden):
    return json.loads(str(golden["cases"]))


def encs(golden):
    return {k: tuple(v) for k, v in json.loads(str(golden["encs"])).items()}


def test_fixture_covers_the_cases_and_is_small(golden):
    names = [c["name"] for c in cases(golden)]
    assert names == ["self_attention", "cross_kdim_vdim", "bias_kv_padding", "zero_attn_mask2d",
                     "mask3d_padding_nobias", "batch_first"]
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "golden_mha.npz")) < 100 * 1024
    assert {c["E"] // c["H"] for c in cases(golden)} == {4, 16}
    margin, U = (int(v) for v in golden["margin"])
    assert margin == 64 and U >= 1
    assert all(c["worst"] >= margin * U for c in cases(golden))


def test_oracle_module_equals_the_fixture_bit_for_bit(golden):
    for case in cases(golden):
        a = O.case_arrays(golden, case["name"])
        out, weights = O.run_case(case, a, encs(golden))
        assert np.array_equal(O.bits(out), O.bits(a["out"])), case["name"]
        assert (weights is None) == ("weights" not in a)
        if weights is not None:
            assert weights.shape == a["weights"].shape
            assert np.array_equal(O.bits(weights), O.bits(a["weights"])), case["name"]


def test_oracle_softmax_stays_within_the_recorded_distance_of_torch(golden):
    """Fresh rows of the fixture's kind: values on matmul_1's grid, 5 or 6 columns, some masked."""
    U = int(golden["margin"][1])
    rng = np.random.default_rng(5)
    for S in (5, 6):
        x = (rng.integers(-128, 128, (256, S)) / 16).astype(F)
        x[rng.random(x.shape) < 0.2] = -np.inf
        x[:, 0] = 0.0
        d = O.ulp_distance(O.softmax_rows(x), torch.softmax(torch.from_numpy(x), -1).numpy())
        print("S %d: max ulp %d (recorded %d)" % (S, d.max(), U))
        assert d.max() <= U


def test_oracle_sum_order_is_the_documented_one():
    """Powers of two far apart make the order visible: 2^24 + 1 + 1 is 2^24 when the ones arrive one
    by one and 2^24 + 2 when they arrive together."""
    big, one = F(2 ** 24), F(1)
    e = np.zeros((1, 130), F)
    e[0, 0], e[0, 64], e[0, 128] = big, one, one            # one lane: (2^24 + 1) + 1
    assert O.row_sums(e)[0] == big
    e[:] = 0
    e[0, 0], e[0, 1], e[0, 33] = big, one, one              # lanes 0, 1, 33: step 32 pairs 1 with 33
    assert O.row_sums(e)[0] == big + F(2)
    e = np.zeros((1, 1025), F)
    e[0, 0], e[0, 128], e[0, 192] = big, one, one           # 256 threads now; waves 0, 2, 3: (2^24 + 0) + (1 + 1)
    assert O.row_sums(e)[0] == big + F(2)
    e[:] = 0
    e[0, 0], e[0, 64], e[0, 192] = big, one, one            # waves 0, 1, 3: (2^24 + 1) + (0 + 1)
    assert O.row_sums(e)[0] == big


def test_c_abi_names_are_exported():
    lib = _native.load()
    for name in ("aimet_attn_softmax", "aimet_attn_softmax_max_s", "aimet_attn_launch_count"):
        assert name in _native.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    with open(os.path.join(REPO, "include", "aimet_amd.h")) as f:
        header = f.read()
    assert "int aimet_attn_softmax(" in header and "int aimet_attn_launch_count(" in header
    assert "#define AIMET_ATTN_SOFTMAX_MAX_S %d" % O.MAX_S in header
    assert T.attn_softmax_max_s() == O.MAX_S >= 4096
    assert T.attn_launch_count() >= 0


@pytest.mark.parametrize("add_bias_kv", [False, True], ids=["", "bias_kv"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_converted_attention_reproduces_torch_in_float(bias, add_bias_kv):
    torch.manual_seed(10)
    mha = nn.MultiheadAttention(128, 8, bias=bias, add_bias_kv=add_bias_kv).eval()
    with torch.no_grad():
        for p in mha.parameters():
            p.copy_(torch.randn_like(p) * 0.2)   # biases are zero-initialised: make them count
    q = T.create_quantizable_multihead_attention(mha)
    assert isinstance(q, nn.MultiheadAttention) and sorted(n for n, _ in q.named_children()) == sorted(MHA_CHILDREN)
    assert q.in_proj_weight is None and q.in_proj_bias is None and not q._qkv_same_embed_dim and not q.training
    x = torch.rand(27, 32, 128)
    kpm = torch.rand(32, 27) > 0.7
    kpm[:, 0] = False
    with torch.no_grad():
        for kw in ({}, {"key_padding_mask": kpm}, {"need_weights": False},
                   {"attn_mask": torch.ones(27, 27, dtype=torch.bool).triu(1), "average_attn_weights": False}):
            want, got = mha(x, x, x, **kw), q(x, x, x, **kw)
            assert torch.allclose(want[0], got[0], atol=1e-5), kw
            assert (want[1] is None) == (got[1] is None)
            if want[1] is not None:
                assert want[1].shape == got[1].shape and torch.allclose(want[1], got[1], atol=1e-6), kw


@pytest.mark.parametrize("kw", [dict(batch_first=True), dict(add_zero_attn=True), dict(kdim=24, vdim=40)],
                         ids=["batch_first", "zero_attn", "kdim_vdim"])
def test_converted_attention_variants_reproduce_torch_in_float(kw):
    torch.manual_seed(11)
    mha = nn.MultiheadAttention(32, 4, **kw).eval()
    q = T.create_quantizable_multihead_attention(mha)
    query, key, value = torch.rand(4, 3, 32), torch.rand(5, 3, kw.get("kdim", 32)), torch.rand(5, 3, kw.get("vdim", 32))
    if kw.get("batch_first"):
        query, key, value = (t.transpose(0, 1).contiguous() for t in (query, key, value))
    with torch.no_grad():
        want, got = mha(query, key, value), q(query, key, value)
    assert want[0].shape == got[0].shape and torch.allclose(want[0], got[0], atol=1e-5)
    assert torch.allclose(want[1], got[1], atol=1e-6)


def test_transformer_transformation_keeps_the_float_output():
    """The reference's test_transformer_transformation."""
    torch.manual_seed(10)
    src = torch.rand(10, 32, 512)
    model = nn.Transformer(num_encoder_layers=2, num_decoder_layers=2).eval()
    with torch.no_grad():
        want = model(src, src)
    second = copy.deepcopy(model)
    T.get_quantizable_pt_transformer_model(model)
    mhas = [m for m in model.modules() if isinstance(m, nn.MultiheadAttention)]
    assert len(mhas) == 6 and all(isinstance(m, T.QuantizableMultiheadAttention) for m in mhas)
    assert all(isinstance(l.activation, nn.ReLU) for l in list(model.encoder.layers) + list(model.decoder.layers))
    with torch.no_grad():
        assert torch.allclose(want, model(src, src), atol=1e-4)
    # with the quantizable encoder / decoder layers as well
    for i, l in enumerate(second.encoder.layers):
        second.encoder.layers[i] = T.create_quantizable_transformer_encoder_layer(l)
    for i, l in enumerate(second.decoder.layers):
        second.decoder.layers[i] = T.create_quantizable_transformer_decoder_layer(l)
    T.get_quantizable_pt_transformer_model(second)
    assert {"add1", "add2", "add3", "activation"} <= {n for n, _ in second.decoder.layers[0].named_children()}
    with torch.no_grad():
        assert torch.allclose(want, second(src, src), atol=1e-4)


def test_batch_first_encoder_in_eval_mode_leaves_torchs_fast_paths():
    torch.manual_seed(3)
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(32, 4, 64, batch_first=True), 2).eval()
    x = torch.rand(2, 5, 32)
    kpm = torch.tensor([[False] * 5, [False, False, False, True, True]])
    with torch.no_grad():
        want = enc(x, src_key_padding_mask=kpm)
    T.get_quantizable_pt_transformer_model(enc)
    calls = []
    hooks = [l.self_attn.linear_Q.register_forward_hook(lambda *a: calls.append(1)) for l in enc.layers]
    with torch.no_grad():
        got = enc(x, src_key_padding_mask=kpm)
    for h in hooks:
        h.remove()
    assert len(calls) == 2 and not got.is_nested
    assert torch.allclose(want[~kpm], got[~kpm], atol=1e-5)   # the nested-tensor path zero-fills padded positions


def test_sim_wraps_every_child_of_every_attention_block():
    assert TRANSFORMER_QUANTIZABLE_TYPES[:len(DEFAULT_QUANTIZABLE_TYPES)] == DEFAULT_QUANTIZABLE_TYPES
    assert TRANSFORMER_QUANTIZABLE_TYPES[len(DEFAULT_QUANTIZABLE_TYPES):] == \
        (Add, Divide, MatMul, nn.Softmax, nn.LayerNorm, nn.GELU, nn.ReLU)
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(32, 4, 64, batch_first=True), 2).eval()
    T.get_quantizable_pt_transformer_model(enc)
    sim = QuantizationSimModel(enc, quant_scheme="tf", quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)
    names = [n for n, _ in sim.quant_wrappers()]
    for layer in range(2):
        attn = sim.model.layers[layer].self_attn
        assert isinstance(attn, T.QuantizableMultiheadAttention)
        for child in MHA_CHILDREN:
            assert isinstance(getattr(attn, child), StaticGridQuantWrapper), child
            assert "layers.%d.self_attn.%s" % (layer, child) in names
        for child in ("linear1", "linear2", "norm1", "norm2", "activation"):
            assert "layers.%d.%s" % (layer, child) in names
        assert attn.matmul_1.output_fusable() and attn.softmax.output_fusable()
        assert not attn.linear_Q.output_fusable()   # it has a weight quantizer
    # with the default types only the linears are wrapped
    enc2 = nn.TransformerEncoder(nn.TransformerEncoderLayer(32, 4, 64), 1).eval()
    T.get_quantizable_pt_transformer_model(enc2)
    sim2 = QuantizationSimModel(enc2, quant_scheme="tf")
    assert sorted(n.split(".")[-1] for n, _ in sim2.quant_wrappers()) == \
        sorted(["linear_Q", "linear_K", "linear_V", "out_proj", "linear1", "linear2"])


def test_model_without_attention_builds_the_same_sim():
    net = nn.Sequential(nn.Linear(7, 7), nn.ReLU(), nn.Linear(7, 3))
    sim = QuantizationSimModel(net, quant_scheme="tf")
    assert [n for n, _ in sim.quant_wrappers()] == ["0", "2"] and list(sim.recurrent_wrappers()) == []
    assert sim.model[0].input_quantizers[0].enabled and not sim.model[2].input_quantizers[0].enabled
    before = copy.deepcopy(net)
    T.get_quantizable_pt_transformer_model(net)
    assert [type(m) for m in net] == [type(m) for m in before]


def test_refusals():
    q = T.QuantizableMultiheadAttention(16, 4).eval()
    x = torch.rand(4, 3, 16)
    additive = torch.zeros(4, 4)
    additive[0, 1] = -1.5
    with pytest.raises(NotImplementedError, match="discards the result"):
        q(x, x, x, attn_mask=additive)
    with pytest.raises(NotImplementedError, match="key_padding_mask"):
        q(x, x, x, key_padding_mask=torch.full((3, 4), 0.5))
    with pytest.raises(TypeError, match="attn_mask"):
        q(x, x, x, attn_mask=torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="2D attn_mask"):
        q(x, x, x, attn_mask=torch.zeros(4, 5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="3D attn_mask"):
        q(x, x, x, attn_mask=torch.zeros(3, 4, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="GPU"):
        T.attn_softmax(torch.zeros(12, 4, 4), 3, 4)   # no CPU implementation behind the fused launch
    with pytest.raises(NotImplementedError, match="activation function"):
        T.prepare_pt_transformer_for_quantsim(nn.TransformerEncoderLayer(16, 4, 32, activation=torch.tanh))


def test_float_mask_of_zero_and_minus_infinity_is_its_bool_form_and_the_check_is_cached():
    torch.manual_seed(4)
    q = T.QuantizableMultiheadAttention(16, 4).eval()
    x = torch.rand(4, 3, 16)
    causal = torch.ones(4, 4, dtype=torch.bool).triu(1)
    as_float = torch.zeros(4, 4).masked_fill_(causal, float("-inf"))
    with torch.no_grad():
        want = q(x, x, x, attn_mask=causal)
        n = T.float_mask_checks
        got = q(x, x, x, attn_mask=as_float)
        assert T.float_mask_checks == n + 1
        for _ in range(3):
            q(x, x, x, attn_mask=as_float)
        assert T.float_mask_checks == n + 1            # same tensor, unmodified: no second read-back
        as_float[0, 1] = 0.0                           # an in-place write moves the version: checked again
        q(x, x, x, attn_mask=as_float)
        assert T.float_mask_checks == n + 2
        q(x, x, x, attn_mask=as_float.clone())         # another tensor: checked
        assert T.float_mask_checks == n + 3
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
