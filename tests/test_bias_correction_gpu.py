"""Bias correction on the GPU (csrc/bias_corr.hip, aimet_amd/bias_correction.py) against tests/bc_oracle.py:

1. aimet_bc_channel_sums on both layouts, every load path and split count: the float64 bound for
   double summation in any order, repeatability bit for bit, an unaligned base, accumulation;
2. aimet_bc_apply_empirical and aimet_bc_analytical on every case of tests/golden/golden_bc.npz;
3. correct_bias end to end on a small network: against the plain-torch restatement of the schedule,
   the mean output error before and after, the analytical path's launches, ignored layers, and a
   CPU-resident model.
Needs an MI355X."""
import copy
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

from conftest import bits, gpu_available

import bc_oracle as O
from test_bias_correction import ACTS, ANALYTICAL, EMPIRICAL, analytical_case, empirical_case
from test_bias_correction import golden  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _native  # noqa: E402
from aimet_amd import bias_correction as BC  # noqa: E402
from aimet_amd._native import BcAnalyticalJobC, DfqWeightC  # noqa: E402
from aimet_amd.qc_quantize_op import QcQuantizeWrapper  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

DEV = "cuda"
F = np.float32
GUARD = 8

# Largest |bias difference| between correct_bias and the plain-torch restatement of the schedule
# (tests/bc_oracle.py: correct_bias_torch) on the network below, measured on an MI355X
# (tests/golden/README_bc.md); the test allows twice that.
MEASURED_MAX_BIAS_DIFF = 0.0


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_f32(a, off=0):
    """A device copy of `a` whose first float is `off` floats past a 16-byte boundary, between guards."""
    a = np.ascontiguousarray(a, F)
    buf = torch.full((2 * GUARD + off + a.size,), 777.0, dtype=torch.float32, device=DEV)
    view = buf[GUARD + off:GUARD + off + a.size]
    view.copy_(torch.from_numpy(a.reshape(-1)))
    assert view.data_ptr() % 16 == 4 * off
    return view


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def sums(x, acc0=None, off=0):
    """aimet_bc_channel_sums of x [outer][C][inner] into an accumulator that starts at acc0."""
    outer, C, inner = x.shape
    acc = torch.zeros(C + 2, dtype=torch.float64, device=DEV)
    acc[0], acc[-1] = 555.0, 555.0
    if acc0 is not None:
        acc[1:-1] = torch.from_numpy(np.asarray(acc0, np.float64))
    d = dev_f32(x, off)
    _native.call("aimet_bc_channel_sums", p(d), outer, C, inner, p(acc[1:-1]), stream())
    torch.cuda.synchronize()
    h = acc.cpu().numpy()
    assert h[0] == 555.0 and h[-1] == 555.0, "wrote outside the accumulator"
    return h[1:-1].copy()


def data(shape, seed):
    rng = np.random.default_rng(seed)
    C = shape[1]
    return (rng.standard_normal(shape) * rng.uniform(0.1, 10.0, (1, C, 1)) + rng.standard_normal((1, C, 1))).astype(F)


def check_sums(x, off=0):
    want, mag = O.channel_sums(x)
    n = x.shape[0] * x.shape[2]
    first, second = sums(x, off=off), sums(x, off=off)
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64)), "two runs differ"
    assert np.all(np.abs(first - want) <= n * 2.0 ** -53 * mag), np.abs(first - want).max()


# ---------------------------------------------------------------------------------------------------
# channel sums
# ---------------------------------------------------------------------------------------------------
# (200, 2, 49): the flat path in two splits. n = 9800 a channel and two channels give
# split_count = min(2048 / 2, ceil(9800 / 8192)) = 2 and chunk = ceil(4900 / 256) * 256 = 5120, so the
# second split holds 4680 elements: `hi` clipped to n, and 4680 = 9 * 512 + 72 leaves lanes 0..71 an odd step.
PLANAR = [(1, 1, 1), (2, 3, 49), (3, 5, 1), (2, 70, 15), (1, 300, 7), (4, 2, 3136), (2, 3, 12544),
          (3, 4, 127), (3, 4, 128), (2, 2, 4097), (40, 3, 961), (200, 2, 49), (32, 7, 196)]
INTERLEAVED = [(1, 1), (5, 3), (3, 1000), (257, 130), (4096, 7), (64, 8), (700, 12), (9, 1028)]


@pytest.mark.parametrize("shape", PLANAR, ids=lambda s: "x".join(map(str, s)))
def test_channel_sums_planar(shape):
    check_sums(data(shape, sum(shape)))


@pytest.mark.parametrize("shape", INTERLEAVED, ids=lambda s: "x".join(map(str, s)))
def test_channel_sums_interleaved(shape):
    check_sums(data((shape[0], shape[1], 1), sum(shape)))


@pytest.mark.parametrize("shape", [(2, 3, 12544), (4, 2, 3136), (3, 4, 128), (2, 70, 15), (3, 1000, 1), (64, 8, 1),
                                   (5, 3, 1)], ids=lambda s: "x".join(map(str, s)))
def test_channel_sums_unaligned_base(shape):
    """A base pointer one float past a 16-byte boundary: a slice of a larger buffer."""
    x = data(shape, 7 + sum(shape))
    check_sums(x, off=1)
    # the choice of load width may depend on the alignment, the value barely: both within the bound
    want, mag = O.channel_sums(x)
    assert np.all(np.abs(sums(x, off=0) - want) <= shape[0] * shape[2] * 2.0 ** -53 * mag)


@pytest.mark.parametrize("C,inner", [(3, 3136), (70, 15), (130, 1), (8, 1)])
def test_channel_sums_accumulate_over_batches(C, inner):
    rng = np.random.default_rng(C + inner)
    parts = [data((outer, C, inner), 100 + outer) for outer in (2, 1, 3)]
    acc0 = rng.standard_normal(C) * 50.0
    acc = acc0
    for x in parts:
        acc = sums(x, acc)
    whole = np.concatenate(parts)
    want, mag = O.channel_sums(whole, acc0)
    n = whole.shape[0] * inner + 1
    assert np.all(np.abs(acc - want) <= n * 2.0 ** -53 * (mag + np.abs(acc0)))


def test_channel_sums_rejects_bad_sizes():
    x = dev_f32(np.zeros(16, F))
    acc = torch.zeros(4, dtype=torch.float64, device=DEV)
    lib = _native.load()
    before = BC.launch_count()
    assert lib.aimet_bc_channel_sums(p(x), 0, 4, 2, p(acc), None) != 0
    assert lib.aimet_bc_channel_sums(p(x), 1 << 20, 4, 1 << 12, p(acc), None) != 0
    assert BC.launch_count() == before


# ---------------------------------------------------------------------------------------------------
# the two updates on the golden cases
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EMPIRICAL)
def test_apply_empirical_golden(golden, n):
    ref, q, bias = empirical_case(golden, n)
    count = ref.shape[0] * ref.shape[2]
    rs, rmag = O.channel_sums(ref)
    qs, qmag = O.channel_sums(q)
    _, want = O.apply_empirical(bias, rs, qs, count)
    d_rs = torch.from_numpy(sums(ref)).to(DEV)
    d_qs = torch.from_numpy(sums(q)).to(DEV)
    b = dev_f32(bias)
    _native.call("aimet_bc_apply_empirical", p(b), p(d_rs), p(d_qs), bias.size, float(count), stream())
    torch.cuda.synchronize()
    got = b.cpu().numpy().astype(np.float64)
    bound = O.half_ulp32(want) + 2.0 ** -40 * (np.abs(bias) + (rmag + qmag) / count)
    assert np.all(np.abs(got - want) <= bound), np.abs(got - want).max()
    # and it is the reference's result as far as the reference's float32 means go
    assert np.all(np.abs(got - golden[n + "_out"]) <= float(golden[n + "_dist"]) + 2 * O.half_ulp32(want))


def make_job(slot, w, wq, bias, gamma, beta, act, transposed, keep):
    dw, dq, db = dev_f32(w, 1), dev_f32(wq, 1), dev_f32(bias)
    s = w.shape
    k = int(np.prod(s[2:], dtype=np.int64))
    if transposed:
        slot.w = DfqWeightC(dw.data_ptr(), s[1], s[0], k, k, s[1] * k)
    else:
        slot.w = DfqWeightC(dw.data_ptr(), s[0], s[1], k, s[1] * k, k)
    slot.wq, slot.bias, slot.activation = dq.data_ptr(), db.data_ptr(), act
    if gamma is not None:
        dg, dbeta = dev_f32(gamma), dev_f32(beta)
        slot.gamma, slot.beta = dg.data_ptr(), dbeta.data_ptr()
        keep += [dg, dbeta]
    keep += [dw, dq]
    return db


def run_analytical(cases):
    """One launch over `cases` [(w, wq, bias, gamma, beta, act, transposed)]; the new biases."""
    table = (BcAnalyticalJobC * len(cases))()
    keep = []
    out = [make_job(slot, *c, keep) for slot, c in zip(table, cases)]
    _native.call("aimet_bc_analytical", table, len(cases), stream())
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in out]


@pytest.mark.parametrize("act", range(3), ids=ACTS)
@pytest.mark.parametrize("n", ANALYTICAL)
def test_analytical_golden(golden, n, act):
    w, wq, bias, gamma, beta, t = analytical_case(golden, n)
    _, want, terms = O.analytical(w, wq, bias, gamma, beta, act, t)
    got = run_analytical([(w, wq, bias, gamma, beta, act, t)])[0].astype(np.float64)
    assert np.all(np.isfinite(got))
    bound = O.half_ulp32(want) + 2.0 ** -40 * (np.abs(bias) + terms)
    assert np.all(np.abs(got - want) <= bound), np.abs(got - want).max()
    assert np.all(np.abs(got - golden["%s_out_%s" % (n, ACTS[act])])
                  <= float(golden["%s_dist_%s" % (n, ACTS[act])]) + 2 * O.half_ulp32(want))


@pytest.mark.parametrize("act", [1, 2], ids=ACTS[1:])
def test_analytical_gamma_zero_channel_follows_ieee(golden, act):
    """Only the gamma == 0 channel carries a weight difference: the correction is eps * E of a point
    distribution at beta, clipped by the activation, as the oracle's IEEE evaluation gives it."""
    w, wq, bias, gamma, beta, t = analytical_case(golden, "a0")
    z = int(golden["a0_zero"])
    wq2 = w.copy()
    wq2[:, z] = wq[:, z]
    _, want, terms = O.analytical(w, wq2, bias, gamma, beta, act, t)
    E = O.expected_input(beta, gamma, act)[z]
    assert E == max(0.0, float(beta[z])) and np.any(want != bias)
    got = run_analytical([(w, wq2, bias, gamma, beta, act, t)])[0].astype(np.float64)
    assert np.all(np.abs(got - want) <= O.half_ulp32(want) + 2.0 ** -40 * (np.abs(bias) + terms))
    # depthwise: channel z of the output
    w, wq, bias, gamma, beta, t = analytical_case(golden, "a2")
    z = int(golden["a2_zero"])
    _, want, terms = O.analytical(w, wq, bias, gamma, beta, act, t)
    got = run_analytical([(w, wq, bias, gamma, beta, act, t)])[0].astype(np.float64)
    assert abs(got[z] - want[z]) <= O.half_ulp32(want[z]) + 2.0 ** -40 * (abs(bias[z]) + terms[z])


def test_analytical_without_bn_is_a_zero_correction(golden):
    w, wq, bias, _, _, t = analytical_case(golden, "a0")
    got = run_analytical([(w, wq, bias, None, None, 0, t)])[0]
    assert np.array_equal(bits(got), bits(bias))


def test_analytical_five_jobs_in_one_launch(golden):
    cases = []
    for i, n in enumerate(ANALYTICAL):
        w, wq, bias, gamma, beta, t = analytical_case(golden, n)
        cases.append((w, wq, bias, gamma, beta, i % 3, t))
    before = BC.launch_count()
    together = run_analytical(cases)
    assert BC.launch_count() == before + 1
    for c, got in zip(cases, together):
        alone = run_analytical([c])[0]
        assert np.array_equal(bits(got), bits(alone))
    assert BC.launch_count() == before + 1 + len(cases)


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
class Net(nn.Module):
    """conv3x3 - BN - ReLU - depthwise3x3 - BN - ReLU6 - conv1x1 - (+ residual) - ConvTranspose2d - BN -
    conv3x3 stride 2 - flatten - Linear - ReLU - Linear. The first two convs have no bias."""

    def __init__(self):
        super().__init__()
        self.c1, self.b1, self.r1 = nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8), nn.ReLU()
        self.dw, self.b2, self.r2 = nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=False), nn.BatchNorm2d(8), nn.ReLU6()
        self.pw = nn.Conv2d(8, 8, 1)
        self.up, self.b3 = nn.ConvTranspose2d(8, 6, 2, stride=2), nn.BatchNorm2d(6)
        self.c5 = nn.Conv2d(6, 4, 3, stride=2)
        self.fc1, self.r6, self.fc2 = nn.Linear(4 * 31 * 31, 16), nn.ReLU(), nn.Linear(16, 5)

    def forward(self, x):
        y = self.c1(x)
        x = self.r2(self.b2(self.dw(self.r1(self.b1(y)))))
        x = self.pw(x) + y
        x = self.c5(self.b3(self.up(x)))
        return self.fc2(self.r6(self.fc1(x.flatten(1))))


LAYERS = ["c1", "dw", "pw", "up", "c5", "fc1", "fc2"]
QP = dict(weight_bw=4, act_bw=8)


def seeded_net():
    g = torch.Generator().manual_seed(5)
    m = Net()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
                fan_in = mod.weight[0].numel() if not isinstance(mod, nn.ConvTranspose2d) else mod.weight[:, 0].numel()
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                if mod.bias is not None:
                    mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
            elif isinstance(mod, nn.BatchNorm2d):
                n = mod.num_features
                mod.weight.copy_(torch.exp(torch.rand(n, generator=g) * 2.0 - 1.5))
                mod.bias.copy_(torch.randn(n, generator=g) * 0.5)
                mod.running_mean.copy_(torch.randn(n, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(n, generator=g) + 0.5)
    return m.eval()


def batches():
    g = torch.Generator().manual_seed(9)
    return [(torch.randn(4, 3, 32, 32, generator=g), torch.zeros(4)) for _ in range(4)]


def biases(model):
    return {n: getattr(model, n).bias.detach().cpu().numpy().copy() for n in LAYERS}


@pytest.fixture(scope="module")
def corrected():
    """(the untouched model, the model after correct_bias, both on the device)"""
    original = seeded_net().to(DEV)
    model = copy.deepcopy(original)
    BC.correct_bias(model, BC.QuantParams(**QP), 16, batches(), 16)
    torch.cuda.synchronize()
    return original, model


def test_end_to_end_no_wrappers_and_new_biases(corrected):
    original, model = corrected
    assert not any(isinstance(m, QcQuantizeWrapper) for m in model.modules())
    assert [n for n, _ in model.named_children()] == [n for n, _ in original.named_children()]
    assert original.c1.bias is None and original.dw.bias is None
    for n in LAYERS:
        b = getattr(model, n).bias
        assert b is not None and b.dtype == torch.float32 and b.is_cuda and torch.isfinite(b).all()
        w0 = getattr(original, n).weight
        assert torch.equal(getattr(model, n).weight, w0), "weights are not touched"
        b0 = getattr(original, n).bias
        assert not torch.equal(b, torch.zeros_like(b) if b0 is None else b0), n


def test_end_to_end_equals_the_plain_torch_schedule(corrected):
    original, model = corrected
    twin = copy.deepcopy(original)
    d = BC.find_all_conv_bn_with_activation(twin)
    O.correct_bias_torch(twin, BC.QuantParams(**QP), 16, batches(), 16, d)
    got, want = biases(model), biases(twin)
    worst = max(float(np.abs(got[n].astype(np.float64) - want[n]).max()) for n in LAYERS)
    print("correct_bias vs plain-torch schedule: largest bias difference %.3e" % worst)
    for n in LAYERS:
        print("  %-4s %.3e (|bias| up to %.3e)" % (n, np.abs(got[n].astype(np.float64) - want[n]).max(),
                                                 np.abs(want[n]).max()))
    assert worst <= 2 * MEASURED_MAX_BIAS_DIFF


def mean_output_errors(fp_model, model):
    """Per layer, the largest over channels of |mean(quantized - FP output)| over the correction data,
    in the sim that correct_bias builds (weights quantized, output quantizers off)."""
    data_ = [b.to(DEV) for b, _ in batches()]
    sim = QuantizationSimModel(copy.deepcopy(model), dummy_input=data_[0][:1], default_param_bw=QP["weight_bw"],
                               default_output_bw=QP["act_bw"])
    for _, w in sim.quant_wrappers():
        w.output_quantizers[0].enabled = False
    sim.compute_encodings(lambda m, _: [BC.forward_pass(m, b) for b in data_], None)
    outs = {}
    hooks = []
    for n in LAYERS:
        hooks.append(getattr(fp_model, n).register_forward_hook(
            lambda _, __, out, key=n: outs.__setitem__(("fp", key), out.detach().clone())))
        hooks.append(getattr(sim.model, n).register_forward_hook(
            lambda _, __, out, key=n: outs.__setitem__(("q", key), out.detach().clone())))
    total, count = {}, {}
    for b in data_:
        BC.forward_pass(fp_model, b)
        BC.forward_pass(sim.model, b)
        for n in LAYERS:
            d = (outs[("q", n)].double() - outs[("fp", n)].double())
            dims = [0] + list(range(2, d.dim()))
            total[n] = total.get(n, 0) + d.sum(dims)
            count[n] = count.get(n, 0) + d.numel() // d.shape[1]
    for h in hooks:
        h.remove()
    return {n: float((total[n] / count[n]).abs().max()) for n in LAYERS}


def test_end_to_end_mean_output_error_falls_hundredfold(corrected):
    original, model = corrected
    before = mean_output_errors(original, original)
    after = mean_output_errors(original, model)
    for n in LAYERS:
        print("%-4s mean output error %.3e -> %.3e" % (n, before[n], after[n]))
    for n in LAYERS:
        assert after[n] <= before[n] / 100, n


def test_analytical_layers_go_through_one_launch(monkeypatch, corrected):
    original, _ = corrected
    model = copy.deepcopy(original)
    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith("aimet_bc_"):
            calls.append((name, args[1] if name == "aimet_bc_analytical" else None))
        return real(name, *args)
    monkeypatch.setattr(_native, "call", counting)
    d = BC.find_all_conv_bn_with_activation(model)
    assert [n for n in LAYERS if d[getattr(model, n)].input_bn is not None] == ["dw", "pw", "c5"]
    A = BC.ActivationType
    assert [d[getattr(model, n)].in_activation_type for n in ("dw", "pw", "c5")] == [A.relu, A.relu6, A.no_activation]
    BC.correct_bias(model, BC.QuantParams(**QP), 16, batches(), 16, conv_bn_dict=d,
                    perform_only_empirical_bias_corr=False)
    monkeypatch.undo()
    # the first layer and the three BN-fed convs in one launch; up, fc1 and fc2 measured
    assert [c for c in calls if c[0] == "aimet_bc_analytical"] == [("aimet_bc_analytical", 4)]
    assert sum(c[0] == "aimet_bc_apply_empirical" for c in calls) == 3
    assert sum(c[0] == "aimet_bc_channel_sums" for c in calls) == 3 * 4 * 2
    assert not any(isinstance(m, QcQuantizeWrapper) for m in model.modules())

    twin = copy.deepcopy(original)
    O.correct_bias_torch(twin, BC.QuantParams(**QP), 16, batches(), 16, BC.find_all_conv_bn_with_activation(twin),
                         perform_only_empirical_bias_corr=False)
    got, want = biases(model), biases(twin)
    assert np.array_equal(got["c1"], np.zeros(8, F)), "no BN before the first layer: a zero correction"
    for n in ("dw", "pw", "c5"):
        # two double evaluations of one formula, each rounded to fp32 once
        assert np.all(np.abs(got[n].astype(np.float64) - want[n]) <= 2 * O.half_ulp32(want[n])), n
        b0 = getattr(original, n).bias
        assert not np.array_equal(got[n], np.zeros_like(got[n]) if b0 is None else b0.detach().cpu().numpy())
    for n in ("up", "fc1", "fc2"):
        assert not np.array_equal(got[n], getattr(original, n).bias.detach().cpu().numpy())
        assert np.allclose(got[n], want[n], rtol=0, atol=1e-4 * np.abs(want[n]).max())


def test_layers_to_ignore_keep_their_bits(corrected):
    original, full = corrected
    model = copy.deepcopy(original)
    BC.correct_bias(model, BC.QuantParams(**QP), 16, batches(), 16, layers_to_ignore=[model.up, model.fc2])
    got = biases(model)
    for n in ("up", "fc2"):
        assert np.array_equal(bits(got[n]), bits(getattr(original, n).bias.detach().cpu().numpy()))
    ref = biases(full)
    for n in ("c1", "dw", "pw"):        # before the first ignored layer: as in the full run
        assert np.allclose(got[n], ref[n], rtol=0, atol=1e-6 * np.abs(ref[n]).max()), n
    assert not np.array_equal(got["fc1"], original.fc1.bias.detach().cpu().numpy())


def test_cpu_resident_model_gets_the_same_biases(corrected):
    original, full = corrected
    host = copy.deepcopy(original).cpu()
    BC.correct_bias(host, BC.QuantParams(**QP), 16, batches(), 16)
    assert all(not p.is_cuda for p in host.parameters())
    assert not any(isinstance(m, QcQuantizeWrapper) for m in host.modules())
    got, want = biases(host), biases(full)
    for n in LAYERS:
        assert np.all(np.abs(got[n].astype(np.float64) - want[n]) <= 2 * MEASURED_MAX_BIAS_DIFF), n


def test_channels_last_and_linear_outputs_take_the_interleaved_layout():
    conv, fc = nn.Conv2d(3, 8, 3).to(DEV), nn.Linear(6, 5).to(DEV)
    x = torch.randn(2, 8, 5, 7, device=DEV)
    assert BC._as_outer_c_inner(conv, x)[1:] == (2, 8, 35)
    cl = x.contiguous(memory_format=torch.channels_last)
    got = BC._as_outer_c_inner(conv, cl)
    assert got[0] is cl and got[1:] == (70, 8, 1)
    sliced = x[:, :, :, ::2]
    got = BC._as_outer_c_inner(conv, sliced)
    assert got[0].is_contiguous() and got[1:] == (2, 8, 20)
    y = torch.randn(3, 4, 5, device=DEV)
    assert BC._as_outer_c_inner(fc, y)[1:] == (12, 5, 1)
    for layer, t in ((conv, x), (conv, cl), (conv, sliced), (fc, y)):
        acc = torch.zeros(layer.weight.shape[0], dtype=torch.float64, device=DEV)
        n = BC._add_channel_sums(layer, t, acc)
        dims = [0, 1] if layer is fc else [0, 2, 3]
        want = t.double().sum(dims)
        assert n == t.numel() // layer.weight.shape[0]
        assert torch.allclose(acc, want, rtol=0, atol=1e-12 * float(t.abs().sum()))


def test_call_empirical_correct_bias_on_tensors():
    conv = nn.Conv2d(3, 6, 3).to(DEV)
    b0 = conv.bias.detach().clone()
    ref = torch.randn(4, 6, 9, 9, device=DEV)
    q = ref + torch.randn(1, 6, 1, 1, device=DEV) * 0.1 + torch.randn(4, 6, 9, 9, device=DEV) * 0.01
    BC.call_empirical_correct_bias(conv, ref, q)
    want = (b0.double() - (q.double() - ref.double()).mean((0, 2, 3))).float()
    assert torch.allclose(conv.bias, want, rtol=0, atol=1e-7)
