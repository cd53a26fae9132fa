"""Quantizable multi-head attention on the GPU (csrc/attn_softmax.hip, aimet_amd/transformers.py, the
QuantSim integration) against tests/mha_oracle.py and tests/golden/golden_mha.npz:

1. aimet_attn_softmax against the oracle bit for bit on guarded buffers: every S that changes the code
   taken (the 64-column steps of the wave path's instantiations, the wave / LDS boundary at 1024, the
   resident bound), L in {1, 3}, B = 2, H = 3, five mask layouts x four encoding layouts, bases
   aligned and off by one float, in place and out of place; a fully masked row; the refusal past
   the resident bound;
2. the module in ACTIVE mode against the fixture written from the reference, bit for bit, on the fused
   route and with fused = False;
3. ANALYSIS mode: the two fused quantizers' encodings against fresh quantizers fed the raw scores and
   the kernel's unquantized probabilities; outputs equal to PASSTHROUGH;
4. QuantizationSimModel over a 2-layer batch_first nn.TransformerEncoder in eval mode;
5. which inputs take the literal route, and that they run.
Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import REPO, gpu_available

import mha_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import transformers as T  # noqa: E402
from aimet_amd.elementwise_ops import TRANSFORMER_QUANTIZABLE_TYPES  # noqa: E402
from aimet_amd.libpymo import TfEncoding  # noqa: E402
from aimet_amd.qc_quantize_op import QcQuantizeOpMode, StaticGridQuantWrapper  # noqa: E402
from aimet_amd.quantizers import QuantScheme, StaticGridPerTensorQuantizer  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

DEV = "cuda"
F = np.float32
GUARD = 8
SENTINEL = F(-777.25)
SCORE_ENC, PROB_ENC = (-6.3, 7.1, 8), (0.0, 255.0 / 256.0, 8)
B, H = 2, 3
# 64 k and 64 k + 1: the wave path's instantiations hold 1, 2, 4, 8 and 16 values a lane; 1024 | 1025: the
# wave path | the LDS path; MAX_S: the resident bound
SIZES = [1, 2, 5, 63, 64, 65, 128, 129, 197, 256, 257, 512, 513, 1024, 1025, O.MAX_S]


@pytest.fixture(scope="module", autouse=True)
def exact_fp32_gemm():
    was = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = was


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "golden_mha.npz"))


class Guarded:
    """A device buffer of n floats between two guards, its base aligned to 256 bytes or off by one float."""

    def __init__(self, n, misaligned, fill=None):
        self.n, self.lead = n, GUARD + (1 if misaligned else 0)
        host = np.full(self.lead + n + GUARD, SENTINEL, F)
        if fill is not None:
            host[self.lead:self.lead + n] = np.asarray(fill, F).ravel()
        self.t = torch.from_numpy(host).to(DEV)

    def view(self, *shape):
        return self.t[self.lead:self.lead + self.n].view(*shape)

    def bits(self):
        return self.t.cpu().numpy().view(np.uint32)

    def expect(self, body):
        want = np.full(self.lead + self.n + GUARD, SENTINEL, F)
        want[self.lead:self.lead + self.n] = np.asarray(body, F).ravel()
        return want.view(np.uint32)


def _masks(rng, L, S):
    """name -> (attn_mask or None, key_padding_mask or None); column 0 is never masked."""
    am2, am3, kpm = rng.random((L, S)) < 0.3, rng.random((B * H, L, S)) < 0.3, rng.random((B, S)) < 0.3
    am2[..., 0] = am3[..., 0] = kpm[..., 0] = False
    return {"none": (None, None), "attn2d": (am2, None), "attn_bh": (am3, None), "padding": (None, kpm),
            "both": (am3, kpm)}


def _dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


# ---- 1. the kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_kernel_equals_the_oracle_bit_for_bit(S):
    assert O.MAX_S == T.attn_softmax_max_s()
    for L in (1, 3):
        rng = np.random.default_rng(7 * S + L)
        scores = (rng.standard_normal((B * H, L, S)) * 3.0).astype(F)
        for mname, (am, kpm) in _masks(rng, L, S).items():
            am_d, kpm_d = _dev(am), _dev(kpm)
            for s_enc, p_enc in ((SCORE_ENC, PROB_ENC), (SCORE_ENC, None), (None, PROB_ENC), (None, None)):
                want = O.attn_softmax(scores, B, H, L, S, am, am is not None and am.ndim == 3, kpm, s_enc, p_enc)
                assert np.isfinite(want).all()
                for misaligned in (False, True):
                    for in_place in (False, True):
                        src = Guarded(scores.size, misaligned, scores)
                        dst = src if in_place else Guarded(scores.size, misaligned)
                        T.attn_softmax(src.view(B * H, L, S), B, H, am_d, kpm_d, s_enc, p_enc,
                                       out=dst.view(B * H, L, S))
                        where = (S, L, mname, s_enc is not None, p_enc is not None, misaligned, in_place)
                        assert np.array_equal(dst.bits(), dst.expect(want)), where
                        if not in_place:
                            assert np.array_equal(src.bits(), src.expect(scores)), where


@pytest.mark.parametrize("S", [5, 197, 1025])
def test_a_fully_masked_row_is_nan_and_quantizes_as_the_per_tensor_qdq_does(S):
    L = 3
    rng = np.random.default_rng(S)
    scores = (rng.standard_normal((B * H, L, S)) * 3.0).astype(F)
    am = rng.random((B * H, L, S)) < 0.3
    am[..., 0] = False
    am[4, 1, :] = True
    for p_enc in (None, PROB_ENC):
        want = O.attn_softmax(scores, B, H, L, S, am, True, None, SCORE_ENC, p_enc)
        dst = Guarded(scores.size, True)
        T.attn_softmax(_dev(scores), B, H, _dev(am), None, SCORE_ENC, p_enc, out=dst.view(B * H, L, S))
        got = dst.view(B * H, L, S).cpu().numpy()
        if p_enc is None:
            assert np.isnan(got[4, 1]).all() and np.isnan(want[4, 1]).all()
            got[4, 1] = want[4, 1] = 0.0
            assert np.isfinite(got).all()
            assert np.array_equal(O.bits(got), O.bits(want))
        else:
            # aimet_qdq_per_tensor sends a NaN to the grid's upper end (min(NaN, max) = max)
            assert np.array_equal(O.bits(got), O.bits(want))
            assert np.array_equal(got[4, 1], O.qdq(np.full(S, np.nan, F), PROB_ENC))
        assert np.array_equal(dst.bits()[:dst.lead], dst.expect(want)[:dst.lead])
        assert np.array_equal(dst.bits()[dst.lead + dst.n:], dst.expect(want)[dst.lead + dst.n:])


def test_a_row_past_the_resident_bound_is_refused_and_nothing_is_written():
    S = O.MAX_S + 1
    scores = torch.zeros(1, 1, S, device=DEV)
    dst = Guarded(S, False)
    n = T.attn_launch_count()
    with pytest.raises(ValueError, match="not resident"):
        T.attn_softmax(scores, 1, 1, out=dst.view(1, 1, S))
    assert T.attn_launch_count() == n
    assert np.array_equal(dst.bits(), dst.expect(np.full(S, SENTINEL, F)))


# ---- 2. the module in ACTIVE mode against the reference fixture --------------------------------------
def encoding(enc):
    e = TfEncoding()
    e.min, e.max, e.bw = enc[0], enc[1], int(enc[2])
    e.delta = (enc[1] - enc[0]) / (2 ** int(enc[2]) - 1)
    e.offset = round(enc[0] / e.delta)
    return e


def build_module(case, a):
    E = case["E"]
    m = T.QuantizableMultiheadAttention(E, case["H"], bias=case.get("bias", True),
                                        add_bias_kv=case.get("add_bias_kv", False),
                                        add_zero_attn=case.get("add_zero_attn", False), kdim=case.get("kdim"),
                                        vdim=case.get("vdim"), batch_first=case.get("batch_first", False))
    with torch.no_grad():
        for k, v in a.items():
            if k.startswith("w_"):
                m.get_parameter(k[2:]).copy_(torch.from_numpy(v))
    return m.to(DEV).eval()


def case_inputs(a):
    args = tuple(torch.from_numpy(a[k]).to(DEV) for k in ("query", "key", "value"))
    kw = {"attn_mask": _dev(a.get("attn_mask")), "key_padding_mask": _dev(a.get("key_padding_mask"))}
    return args, kw


def sim_of(module, args, scheme="tf"):
    return QuantizationSimModel(module, dummy_input=args, quant_scheme=scheme,
                                quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)


def wrappers_of(attn):
    return {n: getattr(attn, n) for n in ("linear_Q", "linear_K", "linear_V", "div", "matmul_1", "softmax", "matmul_2",
                                          "out_proj")}


def set_mode(attn, mode):
    for w in wrappers_of(attn).values():
        w.set_mode(mode)


def test_active_module_equals_the_reference_fixture_bit_for_bit(golden):
    cases = json.loads(str(golden["cases"]))
    encs = json.loads(str(golden["encs"]))
    assert len(cases) == 6
    for case in cases:
        a = O.case_arrays(golden, case["name"])
        args, kw = case_inputs(a)
        sim = sim_of(build_module(case, a), args)
        attn = sim.model
        for name, w in wrappers_of(attn).items():
            assert isinstance(w, StaticGridQuantWrapper), name
            assert len(w.input_quantizers) == (2 if name in ("div", "matmul_1", "matmul_2") else 1), name
            w.enable_input_quantizers(False)   # the sim quantizes the model's input at its first wrapper
            w.output_quantizers[0].encoding = encoding(encs[name])
            if "weight" in w.param_quantizers:
                w.param_quantizers["weight"].encoding = encoding(encs["weight"])
                assert "bias" not in w.param_quantizers or not w.param_quantizers["bias"].enabled
        set_mode(attn, QcQuantizeOpMode.ACTIVE)
        for fused in (True, False):
            attn.fused = fused
            n = T.attn_launch_count()
            with torch.no_grad():
                out, weights = attn(*args, need_weights=case["need_weights"],
                                    average_attn_weights=case["average"], **kw)
            assert T.attn_launch_count() - n == (1 if fused else 0), (case["name"], fused)
            assert np.array_equal(O.bits(out.cpu().numpy()), O.bits(a["out"])), (case["name"], fused)
            assert (weights is None) == ("weights" not in a)
            if weights is not None:
                assert np.array_equal(O.bits(weights.cpu().numpy()), O.bits(a["weights"])), (case["name"], fused)


# ---- 3. ANALYSIS mode ------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [QuantScheme.post_training_tf, QuantScheme.post_training_tf_enhanced],
                         ids=["tf", "tf_enhanced"])
def test_analysis_encodings_and_outputs(golden, scheme):
    case = next(c for c in json.loads(str(golden["cases"])) if c["name"] == "mask3d_padding_nobias")
    a = O.case_arrays(golden, case["name"])
    args, kw = case_inputs(a)
    batches = [args, tuple(t.flip(1) * 0.5 for t in args)]
    sim = sim_of(build_module(case, a), args, scheme)
    attn = sim.model
    seen = []

    def calibrate(m, _):
        for b in batches:
            seen.append(m(*b, **kw))
    n = T.attn_launch_count()
    sim.compute_encodings(calibrate)
    assert T.attn_launch_count() - n == 2
    # PASSTHROUGH gives the same outputs, fused or not, and shows the raw scores
    set_mode(attn, QcQuantizeOpMode.PASSTHROUGH)
    raw = []
    hook = attn.matmul_1.get_original_module().register_forward_hook(lambda m, i, o: raw.append(o.detach().clone()))
    with torch.no_grad():
        for i, b in enumerate(batches):
            out, weights = attn(*b, **kw)
            assert torch.equal(out, seen[i][0]) and torch.equal(weights, seen[i][1])
            attn.fused = False
            out, weights = attn(*b, **kw)
            attn.fused = True
            assert torch.allclose(out, seen[i][0], atol=1e-5) and torch.allclose(weights, seen[i][1], atol=1e-6)
    hook.remove()
    assert len(raw) == 2 and raw[0].shape == (3 * case["H"], 4, 5)
    fresh_scores = StaticGridPerTensorQuantizer(8, "nearest", scheme, False, enabled_by_default=True)
    fresh_probs = StaticGridPerTensorQuantizer(8, "nearest", scheme, False, enabled_by_default=True)
    for scores in raw:
        fresh_scores.update_encoding_stats(scores)
        fresh_probs.update_encoding_stats(T.attn_softmax(scores, 3, case["H"], kw["attn_mask"], kw["key_padding_mask"]))
    fresh_scores.compute_encoding()
    fresh_probs.compute_encoding()
    assert attn.matmul_1.output_quantizers[0].encoding.to_tuple() == fresh_scores.encoding.to_tuple()
    assert attn.softmax.output_quantizers[0].encoding.to_tuple() == fresh_probs.encoding.to_tuple()


# ---- 4. QuantizationSimModel over a transformer encoder --------------------------------------------
def test_quantsim_over_a_batch_first_encoder_in_eval_mode():
    torch.manual_seed(11)
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(32, 4, 64, batch_first=True), 2).to(DEV).eval()
    x = torch.randn(2, 5, 32, device=DEV)
    kpm = torch.tensor([[False] * 5, [False, False, False, True, True]], device=DEV)
    with torch.no_grad():
        want = enc(x, src_key_padding_mask=kpm)
    T.get_quantizable_pt_transformer_model(enc)
    sim = QuantizationSimModel(enc, dummy_input=x, quant_scheme="tf_enhanced",
                               quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)
    T.attn_launch_count(reset=True)
    sim.compute_encodings(lambda m, _: m(x, src_key_padding_mask=kpm))
    assert T.attn_launch_count() == 2   # one launch per attention block and forward
    for layer in sim.model.layers:
        for name, w in wrappers_of(layer.self_attn).items():
            assert w._mode is QcQuantizeOpMode.ACTIVE
            assert w.output_quantizers[0].enabled and w.output_quantizers[0].encoding is not None, name
            for q in list(w.input_quantizers) + list(w.param_quantizers.values()):
                assert not q.enabled or q.encoding is not None, name
    with torch.no_grad():
        y = sim.model(x, src_key_padding_mask=kpm)
    assert T.attn_launch_count() == 4
    assert y.shape == want.shape and bool(torch.isfinite(y).all())
    # torch's fused encoder path would have returned the float output, quantizers or not
    assert float((y - want)[~kpm].abs().max()) > 1e-3
    d = sim.get_encodings_dict()
    m1 = sim.model.layers[1].self_attn.matmul_1.output_quantizers[0].encoding
    assert d["activation_encodings"]["layers.1.self_attn.matmul_1"]["output"]["0"]["max"] == m1.max
    assert d["activation_encodings"]["layers.0.self_attn.softmax"]["output"]["0"]["min"] == 0.0
    assert "layers.0.self_attn.linear_K.weight" in d["param_encodings"]
    json.dumps(d)
    sim2 = QuantizationSimModel(enc, dummy_input=x, quant_scheme="tf_enhanced",
                                quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)
    sim2.load_encodings(d)
    assert sim2.model.layers[1].self_attn.matmul_1.output_quantizers[0].encoding.to_tuple() == m1.to_tuple()
    n = T.attn_launch_count()   # the new sim's check of the dummy input launched too (PASSTHROUGH, no encodings)
    with torch.no_grad():
        assert torch.equal(sim2.model(x, src_key_padding_mask=kpm), y)
    assert T.attn_launch_count() == n + 2


# ---- 5. route choice -------------------------------------------------------------------------------
def _small_sim(scheme):
    torch.manual_seed(5)
    attn = T.QuantizableMultiheadAttention(16, 4).to(DEV).eval()
    x = torch.randn(5, 3, 16, device=DEV)
    sim = sim_of(attn, (x, x, x), scheme)
    sim.compute_encodings(lambda m, _: m(x, x, x))
    return sim, x


def _runs_without_a_launch(attn, x):
    n = T.attn_launch_count()
    out, weights = attn(x, x, x)
    assert T.attn_launch_count() == n
    assert out.shape == x.shape and weights.shape == (3, 5, 5)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(weights.float()).all())
    return out


def test_inputs_that_take_the_literal_route():
    sim, x = _small_sim("tf")
    attn = sim.model
    n = T.attn_launch_count()
    with torch.no_grad():
        fused_out, _ = attn(x, x, x)
    assert T.attn_launch_count() == n + 1
    # a gradient is wanted
    xg = x.clone().requires_grad_(True)
    out = _runs_without_a_launch(attn, xg)
    assert torch.allclose(out, fused_out, atol=1e-5)
    out.sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
    # fused switched off
    attn.fused = False
    with torch.no_grad():
        assert torch.allclose(_runs_without_a_launch(attn, x), fused_out, atol=1e-5)
    attn.fused = True
    # 16-bit tensors
    attn.to(torch.bfloat16)
    with torch.no_grad():
        assert _runs_without_a_launch(attn, x.to(torch.bfloat16)).dtype == torch.bfloat16


def test_a_range_learning_sim_takes_the_literal_route():
    sim, x = _small_sim(QuantScheme.training_range_learning_with_tf_init)
    from aimet_amd.qc_quantize_op import LearnedGridQuantWrapper
    assert isinstance(sim.model.matmul_1, LearnedGridQuantWrapper)
    with torch.no_grad():
        _runs_without_a_launch(sim.model, x)
    out = _runs_without_a_launch(sim.model, x)
    out.sum().backward()
    assert sim.model.softmax.output0_encoding_max.grad is not None
