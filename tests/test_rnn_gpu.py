"""Quantized recurrent layers on the GPU (csrc/rnn_cell.hip, aimet_amd/qc_quantize_recurrent.py, the
QuantSim integration) against tests/rnn_oracle.py and tests/golden/golden_rnn.npz:

1. aimet_rnn_step against the oracle's step, bit for bit: four modes x {bias, none} x {QDQ on, off} x
   valid_rows in {B, 1}, B = 3 with H = 5, 64 and 65, both directions in one launch, bases aligned and
   misaligned by one element, every byte around every output checked untouched (the kept rows and
   the other direction's columns of the slab included);
2. the whole layer in ACTIVE mode against the fixture written from the reference, bit for bit;
3. ANALYSIS mode: the state quantizers' encodings against fresh quantizers fed the kept per-step
   states in the reference's order, and the outputs against the plain-torch per-step procedure
   within the measured tolerance (4 x the procedure's own GPU / CPU difference);
4. QuantizationSimModel over Linear -> LSTM -> Linear, and a model without recurrent layers.
Needs an MI355X."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from conftest import REPO, gpu_available

import rnn_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _native  # noqa: E402
from aimet_amd import quantsim as QS  # noqa: E402
from aimet_amd._native import RnnStepJobC, TfEncodingC  # noqa: E402
from aimet_amd.libpymo import TfEncoding  # noqa: E402
from aimet_amd.qc_quantize_op import QcQuantizeOpMode  # noqa: E402
from aimet_amd.qc_quantize_recurrent import QcQuantizeRecurrent  # noqa: E402
from aimet_amd.quantizers import QuantScheme, StaticGridPerTensorQuantizer  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

DEV = "cuda"
F = np.float32
GUARD = 8
SENTINEL = F(-777.25)
H_ENC, C_ENC = (-1.0, 127.0 / 128.0, 8), (-4.0, 127.0 / 32.0, 8)
CELLS = {"LSTM": torch._VF.lstm_cell, "GRU": torch._VF.gru_cell, "RNN_TANH": torch._VF.rnn_tanh_cell,
         "RNN_RELU": torch._VF.rnn_relu_cell}


@pytest.fixture(scope="module", autouse=True)
def exact_fp32_gemm():
    was = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = was


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "golden_rnn.npz"))


def encoding(enc):
    e = TfEncoding()
    e.min, e.max, e.bw = enc[0], enc[1], int(enc[2])
    e.delta = (enc[1] - enc[0]) / (2 ** int(enc[2]) - 1)
    e.offset = round(enc[0] / e.delta)
    return e


class Guarded:
    """A device buffer of n floats between two guards, its base aligned to 256 bytes or off by one float."""

    def __init__(self, n, misaligned, fill=None):
        self.n, self.lead = n, GUARD + (1 if misaligned else 0)
        host = np.full(self.lead + n + GUARD, SENTINEL, F)
        if fill is not None:
            host[self.lead:self.lead + n] = np.asarray(fill, F).ravel()
        self.t = torch.from_numpy(host).to(DEV)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.lead

    def host(self):
        return self.t.cpu().numpy()

    def expect(self, body):
        want = np.full(self.lead + self.n + GUARD, SENTINEL, F)
        want[self.lead:self.lead + self.n] = np.asarray(body, F).ravel()
        return want


# ---- 1. the step kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("valid_rows", [3, 1])
@pytest.mark.parametrize("qdq", [True, False], ids=["qdq", "noqdq"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("H", [5, 64, 65])
@pytest.mark.parametrize("mode", list(CELLS))
def test_step_equals_the_oracle_bit_for_bit(mode, H, bias, qdq, valid_rows):
    B, T, it, D = 3, 4, 1, 2
    G, lstm = O.GATES[mode], mode == "LSTM"
    rng = np.random.default_rng(1000 * H + 100 * bias + 10 * qdq + valid_rows)
    lens = np.array([4, 1, 1], np.int32) if valid_rows == 1 else None
    ig_all = (rng.standard_normal((T, B, D * G * H)) * 1.5).astype(F)
    hg = (rng.standard_normal((D, B, G * H)) * 1.5).astype(F)
    b_ih = (rng.standard_normal((D, G * H)) * 0.5).astype(F) if bias else None
    b_hh = (rng.standard_normal((D, G * H)) * 0.5).astype(F) if bias else None
    h_prev = (rng.standard_normal((D, B, H)) * 0.6).astype(F)
    c_prev = (rng.standard_normal((D, B, H)) * 1.2).astype(F)
    for misaligned in (False, True):
        bufs = dict(ig=Guarded(ig_all.size, misaligned, ig_all), hg=Guarded(hg.size, misaligned, hg),
                    h_prev=Guarded(h_prev.size, misaligned, h_prev), c_prev=Guarded(c_prev.size, misaligned, c_prev),
                    h_next=Guarded(D * B * H, misaligned), c_next=Guarded(D * B * H, misaligned),
                    out=Guarded(T * B * D * H, misaligned))
        if bias:
            bufs["b_ih"], bufs["b_hh"] = Guarded(b_ih.size, misaligned, b_ih), Guarded(b_hh.size, misaligned, b_hh)
        lens_dev = torch.from_numpy(lens).to(DEV) if lens is not None else None
        jobs = (RnnStepJobC * D)()
        want_h, want_c = np.empty((D, B, H), F), np.empty((D, B, H), F)
        want_out = np.full((T, B, D * H), SENTINEL, F)
        for d in range(D):
            j = jobs[d]
            j.ig, j.ig_step_stride, j.ig_row_stride = bufs["ig"].ptr + 4 * d * G * H, B * D * G * H, D * G * H
            j.hg, j.hg_row_stride = bufs["hg"].ptr + 4 * d * B * G * H, G * H
            j.b_ih = bufs["b_ih"].ptr + 4 * d * G * H if bias else None
            j.b_hh = bufs["b_hh"].ptr + 4 * d * G * H if bias else None
            j.h_prev, j.c_prev = bufs["h_prev"].ptr + 4 * d * B * H, bufs["c_prev"].ptr + 4 * d * B * H
            j.h_next, j.c_next = bufs["h_next"].ptr + 4 * d * B * H, bufs["c_next"].ptr + 4 * d * B * H
            j.out, j.out_step_stride, j.out_row_stride = bufs["out"].ptr + 4 * d * H, B * D * H, D * H
            j.lens = lens_dev.data_ptr() if lens is not None else None
            j.reverse = d
            # the oracle: row b at time t_b
            row_len = lens if lens is not None else np.full(B, T)
            t_of = np.where(np.arange(B) < valid_rows, (row_len - 1 - it) if d else it, 0)
            ig = ig_all[t_of, np.arange(B), d * G * H:(d + 1) * G * H]
            h2, c2 = O.step(mode, ig, hg[d], b_ih[d] if bias else None, b_hh[d] if bias else None, h_prev[d],
                            c_prev[d] if lstm else None, valid_rows, H_ENC if qdq else None, C_ENC if qdq else None)
            want_h[d] = h2
            if lstm:
                want_c[d] = c2
            for b in range(valid_rows):
                want_out[t_of[b], b, d * H:(d + 1) * H] = h2[b]
        h_enc, c_enc = TfEncodingC(*encoding(H_ENC).to_tuple()), TfEncodingC(*encoding(C_ENC).to_tuple())
        _native.call("aimet_rnn_step", O.MODE_IDS[mode], jobs, D, B, H, T, it, valid_rows, ctypes.byref(h_enc),
                     int(qdq), ctypes.byref(c_enc), int(qdq), QcQuantizeOpMode.ACTIVE.value, None)
        torch.cuda.synchronize()
        assert np.array_equal(O.bits(bufs["h_next"].host()), O.bits(bufs["h_next"].expect(want_h))), misaligned
        assert np.array_equal(O.bits(bufs["out"].host()), O.bits(bufs["out"].expect(want_out))), misaligned
        if lstm:
            assert np.array_equal(O.bits(bufs["c_next"].host()), O.bits(bufs["c_next"].expect(want_c))), misaligned
        else:   # never written
            assert np.array_equal(O.bits(bufs["c_next"].host()), O.bits(bufs["c_next"].expect(np.full(D * B * H, SENTINEL))))
        for name, src in (("ig", ig_all), ("hg", hg), ("h_prev", h_prev), ("c_prev", c_prev)):   # inputs as they were
            assert np.array_equal(O.bits(bufs[name].host()), O.bits(bufs[name].expect(src))), name


def test_step_analysis_mode_does_not_quantize_and_counts_launches():
    B, H = 3, 5
    rng = np.random.default_rng(5)
    ig, hg = (torch.from_numpy(rng.standard_normal((B, H)).astype(F)).to(DEV) for _ in range(2))
    h = torch.from_numpy((rng.standard_normal((B, H)) * 0.5).astype(F)).to(DEV)
    h2, out = torch.empty_like(h), torch.empty_like(h)
    job = (RnnStepJobC * 1)()
    job[0].ig, job[0].ig_row_stride, job[0].hg, job[0].hg_row_stride = ig.data_ptr(), H, hg.data_ptr(), H
    job[0].h_prev, job[0].h_next, job[0].out, job[0].out_row_stride = h.data_ptr(), h2.data_ptr(), out.data_ptr(), H
    enc = TfEncodingC(*encoding(H_ENC).to_tuple())
    n0 = ctypes.c_int64()
    _native.call("aimet_rnn_launch_count", ctypes.byref(n0), 0)
    _native.call("aimet_rnn_step", O.MODE_IDS["RNN_TANH"], job, 1, B, H, 1, 0, B, ctypes.byref(enc), 1, None, 0,
                 QcQuantizeOpMode.ANALYSIS.value, None)
    n1 = ctypes.c_int64()
    _native.call("aimet_rnn_launch_count", ctypes.byref(n1), 0)
    assert n1.value == n0.value + 1
    want, _ = O.step("RNN_TANH", ig.cpu().numpy(), hg.cpu().numpy(), None, None, h.cpu().numpy(), None, B)
    assert np.array_equal(O.bits(h2.cpu().numpy()), O.bits(want)) and torch.equal(h2, out)
    with pytest.raises(ValueError, match="valid_rows"):
        _native.call("aimet_rnn_step", 2, job, 1, B, H, 1, 0, B + 1, None, 0, None, 0, 3, None)
    with pytest.raises(ValueError, match="jobs"):
        _native.call("aimet_rnn_step", 2, job, 3, B, H, 1, 0, B, None, 0, None, 0, 3, None)
    with pytest.raises(ValueError, match="encoding"):
        _native.call("aimet_rnn_step", 2, job, 1, B, H, 1, 0, B, None, 1, None, 0, 3, None)


# ---- 2. the layer against the fixture ----------------------------------------------------------
def module_of(case, arrays, device=DEV):
    cls = {"LSTM": nn.LSTM, "GRU": nn.GRU}.get(case["mode"], nn.RNN)
    kw = {"nonlinearity": "tanh" if case["mode"] == "RNN_TANH" else "relu"} if cls is nn.RNN else {}
    m = cls(7, case["H"], num_layers=2, bidirectional=True, bias=case["bias"], batch_first=case["batch_first"], **kw)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.from_numpy(arrays["w_" + name]))
    return m.to(device).eval()


def preset_wrapper(case, arrays, encs):
    w = QcQuantizeRecurrent(module_of(case, arrays), 8, 8, "nearest", QuantScheme.post_training_tf).to(DEV).eval()
    enc_in, enc_h, enc_p, enc_c = encs
    for name, q in w.grouped_quantizers.items():
        q.encoding = encoding(enc_h if name.startswith("hidden") else enc_c if name.startswith("cell") else enc_p)
        if name.startswith("cell"):
            q.enabled = True   # as the fixture (tests/golden/make_golden_rnn.py)
    for name, q in w.input_quantizers.items():
        if name.startswith("input"):
            q.encoding = encoding(enc_in)
    w.set_mode(QcQuantizeOpMode.ACTIVE)
    return w


def case_inputs(case, a):
    x = torch.from_numpy(a["x"]).to(DEV)
    if case["packed"]:
        x = pack_padded_sequence(x, torch.from_numpy(a["lens"]), batch_first=case["batch_first"], enforce_sorted=False)
    hx = None
    if case["state"]:
        hx = torch.from_numpy(a["h0"]).to(DEV)
        if case["mode"] == "LSTM":
            hx = (hx, torch.from_numpy(a["c0"]).to(DEV))
    return x, hx


def test_active_layer_equals_the_reference_fixture_bit_for_bit(golden):
    cases = json.loads(str(golden["cases"]))
    assert len(cases) == 20
    for case in cases:
        a = O.case_arrays(golden, case["name"])
        w = preset_wrapper(case, a, golden["encs"])
        before = {n: p.detach().clone() for n, p in w.get_named_parameters()}
        x, hx = case_inputs(case, a)
        out, hn = w(x, hx)
        if case["packed"]:
            out, lens = pad_packed_sequence(out, batch_first=case["batch_first"], total_length=4)
            assert lens.tolist() == a["lens"].tolist()
        cn = None
        if case["mode"] == "LSTM":
            hn, cn = hn
        assert np.array_equal(O.bits(out.cpu().numpy()), O.bits(a["out"])), case
        assert np.array_equal(O.bits(hn.cpu().numpy()), O.bits(a["hn"])), case
        if cn is not None:
            assert np.array_equal(O.bits(cn.cpu().numpy()), O.bits(a["cn"])), case
        for n, p in w.get_named_parameters():   # the originals as they were
            assert torch.equal(p, before[n])


# ---- 3. ANALYSIS mode ----------------------------------------------------------------------------
def plain_procedure(mode, params, x, hx, bias, device):
    """The reference's per-step procedure in plain torch operations for a dense [T, B, I] input, without
    activation quantizers: _VF cells, lists, flip, stack and cat. params: name -> tensor, as given."""
    p = {k: v.to(device) for k, v in params.items()}
    x = x.to(device)
    T, B, _ = x.shape
    lstm = mode == "LSTM"
    layers = len([k for k in p if k.startswith("weight_ih") and not k.endswith("reverse")])
    H = p["weight_hh_l0"].shape[1]
    hn, cn, inp = [], [], x
    for layer in range(layers):
        outs = []
        for d in range(2):
            names = O.param_names(layer, d, bias)
            w_ih, w_hh = p[names[0]], p[names[1]]
            b_ih, b_hh = (p[names[2]], p[names[3]]) if bias else (None, None)
            if hx is None:
                z = torch.zeros(B, H, device=device)
                state = (z, z) if lstm else z
            else:
                state = (hx[0][layer].to(device), hx[1][layer].to(device)) if lstm else hx[layer].to(device)
            seq = torch.flip(inp, [0]) if d else inp
            steps = []
            for it in range(T):
                state = CELLS[mode](seq[it], state, w_ih, w_hh, b_ih, b_hh)
                steps.append(state[0] if lstm else state)
            if d:
                steps = steps[::-1]
            outs.append(torch.stack(steps))
            hn.append(state[0] if lstm else state)
            if lstm:
                cn.append(state[1])
        inp = torch.cat(outs, 2)
    return inp, torch.stack(hn), (torch.stack(cn) if lstm else None)


@pytest.fixture(scope="module")
def analysis_problem():
    """An LSTM (7 -> 5, two layers, bidirectional) with its default initialisation, a normal input, a
    given initial state; and the measured tolerance: 4 x the largest difference between the plain
    procedure on the GPU and on the CPU (4: the fused path groups its GEMMs differently)."""
    torch.manual_seed(7)
    lstm = nn.LSTM(7, 5, num_layers=2, bidirectional=True).eval()
    x = torch.randn(4, 3, 7)
    hx = (torch.randn(4, 3, 5) * 0.5, torch.randn(4, 3, 5))
    return lstm, x, hx


def measured_tolerance(mode, params, x, hx, bias=True):
    gpu = plain_procedure(mode, params, x, hx, bias, DEV)
    cpu = plain_procedure(mode, params, x, hx, bias, "cpu")
    diff = max(float((g.cpu() - c).abs().max()) for g, c in zip(gpu, cpu) if g is not None)
    print("plain procedure, GPU against CPU: largest difference %.3g; tolerance %.3g" % (diff, 4 * diff))
    return 4 * diff, gpu


@pytest.mark.parametrize("scheme", [QuantScheme.post_training_tf, QuantScheme.post_training_tf_enhanced],
                         ids=["tf", "tf_enhanced"])
def test_analysis_encodings_and_outputs(analysis_problem, scheme):
    lstm, x, hx = analysis_problem
    w = QcQuantizeRecurrent(lstm, 8, 8, "nearest", scheme).to(DEV).eval()
    w.grouped_quantizers["cell_l0"].enabled = w.grouped_quantizers["cell_l1"].enabled = True
    w.keep_analysis_states = True
    w.set_mode(QcQuantizeOpMode.ANALYSIS)
    xg, hxg = x.to(DEV), tuple(t.to(DEV) for t in hx)
    out, (hn, cn) = w(xg, hxg)
    # the parameters the forward used: through their quantizers, as the reference quantizes them in every mode
    params = w._quantized_params()
    tol, (p_out, p_hn, p_cn) = measured_tolerance("LSTM", {k: v.cpu() for k, v in params.items()}, x, hx)
    for name, got, want in (("out", out, p_out), ("h_n", hn, p_hn), ("c_n", cn, p_cn)):
        diff = float((got - want).abs().max())
        print("%s: fused against the plain procedure on the GPU: %.3g (tolerance %.3g)" % (name, diff, tol))
        assert diff <= tol, name
    # each state quantizer: the encoding of a fresh quantizer fed the kept states in the reference's order
    w.compute_encoding()
    for layer in range(2):
        h_hist, c_hist, h_init, c_init = w.last_analysis_states[layer]
        assert h_hist.shape == (4, 2, 3, 5) and torch.equal(h_hist[3, 0], hn[2 * layer]) and torch.equal(h_hist[3, 1], hn[2 * layer + 1])
        for q, hist, init in ((w.output_quantizers["h_l%d" % layer], h_hist, h_init),
                              (w.output_quantizers["c_l%d" % layer], c_hist, c_init)):
            fresh = StaticGridPerTensorQuantizer(8, "nearest", scheme, False, enabled_by_default=True)
            for d in range(2):
                for it in range(4):
                    fresh.update_encoding_stats(hist[it, d].clone())
                fresh.update_encoding_stats(init[d].clone())
            fresh.compute_encoding()
            assert q.encoding is not None and q.encoding.to_tuple() == fresh.encoding.to_tuple()
    assert w.input_quantizers["initial_h_l0"] is w.output_quantizers["h_l0"]


# ---- 4. QuantizationSimModel ---------------------------------------------------------------------
class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.rnn, self.b = nn.Linear(7, 7), nn.LSTM(7, 5, num_layers=2, bidirectional=True), nn.Linear(10, 3)

    def forward(self, x):
        return self.b(self.rnn(self.a(x))[0])


def test_quantsim_over_linear_lstm_linear():
    torch.manual_seed(11)
    net = Net().to(DEV).eval()
    x = torch.randn(4, 3, 7, device=DEV)
    sim = QuantizationSimModel(net, dummy_input=x, quant_scheme="tf_enhanced")
    assert [n for n, _ in sim.recurrent_wrappers()] == ["rnn"] and [n for n, _ in sim.quant_wrappers()] == ["a", "b"]
    n0 = ctypes.c_int64()
    _native.call("aimet_rnn_launch_count", ctypes.byref(n0), 1)
    seen = []
    hook = sim.model.rnn.register_forward_pre_hook(lambda m, args: seen.append(args[0].detach().clone()))
    sim.compute_encodings(lambda m, _: m(x))
    hook.remove()
    _native.call("aimet_rnn_launch_count", ctypes.byref(n0), 0)
    assert n0.value == 2 * 4   # one launch per layer and step, both directions in it
    w = sim.model.rnn
    # through the calibration's StatsBatch every quantizer ends where the per-step updates of a wrapper
    # used on its own end: the encodings of T sequential updates per direction
    alone = QcQuantizeRecurrent(copy.deepcopy(net.rnn), 8, 8, "nearest", QuantScheme.post_training_tf_enhanced).eval()
    for q in set(alone.param_quantizers.values()):
        q.use_symmetric_encodings = True   # the sim's default config for parameters
    assert len(seen) == 1
    alone(seen[0])
    alone.compute_encoding()
    for name in ("hidden_l0", "hidden_l1", "W_l0", "W_l1", "R_l0", "R_l1"):
        assert w.grouped_quantizers[name].encoding.to_tuple() == alone.grouped_quantizers[name].encoding.to_tuple(), name
    for name in ("input_l0", "input_l1"):
        assert w.input_quantizers[name].encoding.to_tuple() == alone.input_quantizers[name].encoding.to_tuple(), name
    assert w._mode is QcQuantizeOpMode.ACTIVE
    with torch.no_grad():
        y = sim.model(x)
    assert y.shape == (4, 3, 3) and bool(torch.isfinite(y).all())
    enabled = ["hidden_l0", "hidden_l1", "W_l0", "W_l1", "R_l0", "R_l1"]
    for name in enabled:
        assert w.grouped_quantizers[name].encoding is not None, name
    assert w.input_quantizers["input_l0"].encoding is not None and w.input_quantizers["input_l1"].encoding is not None
    assert w.grouped_quantizers["cell_l0"].encoding is None and w.grouped_quantizers["bias_l0"].encoding is None
    d = sim.get_encodings_dict()
    for p in ("weight_ih_l0", "weight_hh_l1_reverse"):
        assert d["param_encodings"]["rnn." + p][0]["min"] == w.param_quantizers[p].encoding.min
    assert "rnn.bias_ih_l0" not in d["param_encodings"]
    assert d["activation_encodings"]["rnn.h_l0"]["output"]["0"]["max"] == w.output_quantizers["h_l0"].encoding.max
    assert d["activation_encodings"]["rnn.input_l1"]["input"]["0"]["scale"] == w.input_quantizers["input_l1"].encoding.delta
    assert "rnn.c_l0" not in d["activation_encodings"] and "a" in d["activation_encodings"]
    # the exported encodings load into a fresh sim, which then computes the same
    sim2 = QuantizationSimModel(net, dummy_input=x, quant_scheme="tf_enhanced")
    sim2.load_encodings(d)
    assert sim2.model.rnn._mode is QcQuantizeOpMode.ACTIVE
    assert sim2.model.rnn.output_quantizers["h_l1"].encoding.to_tuple() == w.output_quantizers["h_l1"].encoding.to_tuple()
    with torch.no_grad():
        assert torch.equal(sim2.model(x), y)
    # the quantized layer differs from the float one; with every recurrent quantizer off it is the float one
    xin = torch.randn(4, 3, 7, device=DEV)
    with torch.no_grad():
        want, (want_h, want_c) = net.rnn(xin)
        quant, _ = w(xin)
    assert float((quant - want).abs().max()) > 1e-4
    for q in w._all_quantizers():
        q.enabled = False
    params = {k: v.detach().cpu() for k, v in net.rnn.named_parameters()}
    tol, _ = measured_tolerance("LSTM", params, xin.cpu(), None)
    with torch.no_grad():
        got, (got_h, got_c) = w(xin)
    for name, a, b in (("out", got, want), ("h_n", got_h, want_h), ("c_n", got_c, want_c)):
        diff = float((a - b).abs().max())
        print("%s: every quantizer off, against nn.LSTM on the GPU: %.3g (tolerance %.3g)" % (name, diff, tol))
        assert diff <= tol, name
    original = QuantizationSimModel.get_original_model(sim.model)
    assert type(original.rnn) is nn.LSTM and torch.equal(original.rnn.weight_ih_l0, net.rnn.weight_ih_l0)


def test_model_without_recurrent_layers_is_as_before(monkeypatch):
    """The same wrapper names and encodings as the walk that knows no recurrent types."""
    torch.manual_seed(3)
    net = nn.Sequential(nn.Linear(7, 9), nn.ReLU(), nn.Linear(9, 3)).to(DEV).eval()
    x = torch.randn(16, 7, device=DEV)

    def run():
        sim = QuantizationSimModel(net, dummy_input=x, quant_scheme="tf_enhanced")
        sim.compute_encodings(lambda m, _: m(x))
        return [n for n, _ in sim.quant_wrappers()], sim.get_encodings_dict(), sim.model(x)
    names, encs, y = run()
    monkeypatch.setattr(QS, "RECURRENT_TYPES", ())
    names0, encs0, y0 = run()
    assert names == names0 == ["0", "2"] and encs == encs0 and torch.equal(y, y0)
    assert set(encs["param_encodings"]) == {"0.weight", "2.weight"}
