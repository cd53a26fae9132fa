"""Data-free quantization on the GPU (csrc/dfq.hip) against the numpy oracle tests/dfq_oracle.py:

1. the kernels bit for bit on the fixture shapes of tests/golden/golden_dfq.npz (BN backward fold,
   CLS pair and triple with special channels, transposed and 1-d layouts, misaligned rows, missing
   biases); the forward fold's and HBF's bias sums against float64 within the fp32 summation bound,
   two runs bit-identical;
2. properties of a scaled pair (equal ranges, a second scaling is the identity);
3. end to end: fold + equalize on a small conv/BN/ReLU network against the oracle driven over the
   same pairs and sets, function preserved; QuantizationSimModel on folded ResNet-50; equalize_model
   on the BN MobileNet-v2 with its launches counted.
Needs an MI355X."""
import copy
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

from conftest import bits, gpu_available

import dfq_oracle as O
from test_dfq import BN_BACKWARD, HBF_CASES, PAIR_CASES, bn_case, hbf_case, pair_case, sets_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _dfq, _native  # noqa: E402
from aimet_amd import batch_norm_fold as BNF  # noqa: E402
from aimet_amd import cross_layer_equalization as CLE  # noqa: E402
from aimet_amd._native import DfqBnFoldJobC, DfqWeightC  # noqa: E402
from test_dfq import golden  # noqa: E402,F401  (fixture)

DEV = "cuda"
GUARD = 8
SENTINEL = 12345.0
F = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """A device copy of `a` between guard floats; off = 1 breaks the 16-byte alignment of the rows."""

    def __init__(self, a, off=0):
        a = np.ascontiguousarray(a, F)
        self.shape, self.off, self.n = a.shape, off, a.size
        self.buf = torch.full((2 * GUARD + off + a.size,), SENTINEL, dtype=torch.float32, device=DEV)
        self.view = self.buf[GUARD + off:GUARD + off + a.size]
        self.view.copy_(torch.from_numpy(a.reshape(-1)))
        assert (self.view.data_ptr() % 16 == 0) == (off == 0)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def get(self):
        h = self.buf.cpu().numpy()
        assert np.all(h[:GUARD + self.off] == SENTINEL) and np.all(h[GUARD + self.off + self.n:] == SENTINEL), \
            "wrote outside the tensor"
        return h[GUARD + self.off:GUARD + self.off + self.n].reshape(self.shape).copy()


def desc(buf, transposed=False):
    s = buf.shape
    k = int(np.prod(s[2:], dtype=np.int64))
    if transposed:
        return DfqWeightC(buf.view.data_ptr(), s[1], s[0], k, k, s[1] * k)
    return DfqWeightC(buf.view.data_ptr(), s[0], s[1], k, s[1] * k, k)


def opt(buf):
    return None if buf is None else buf.ptr


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def run_pair(w0, b0, w1, t0=False, t1=False, off=0):
    W0, W1 = Buf(w0, off), Buf(w1, off)
    B0 = None if b0 is None else Buf(b0)
    C = w0.shape[1] if t0 else w0.shape[0]
    S = Buf(np.zeros(C, F))
    _native.call("aimet_dfq_cls_pair", desc(W0, t0), opt(B0), desc(W1, t1), S.ptr, stream())
    torch.cuda.synchronize()
    return S.get(), W0.get(), None if B0 is None else B0.get(), W1.get()


# ---------------------------------------------------------------------------------------------------
# kernels against the oracle
# ---------------------------------------------------------------------------------------------------
def test_bn_fold_one_launch_bit_equal(golden):
    """The four backward folds, one into a transposed layout and the forward fold as six jobs of one
    launch: backward bit-equal to the oracle and to the reference golden."""
    cases = [(n,) + bn_case(golden, n) for n in BN_BACKWARD + ["b4"]]
    rng = np.random.default_rng(5)
    wt = golden["p4_w0"]                       # ConvTranspose2d layout [in 4][out 6][3][3]
    tcase = ("tr", wt, rng.standard_normal(6).astype(F), rng.uniform(0.2, 2, 6).astype(F),
             rng.standard_normal(6).astype(F), rng.standard_normal(6).astype(F), rng.uniform(0.3, 2, 6).astype(F), 1e-5)
    cases.append(tcase)
    before = _dfq.launch_count()
    table = (DfqBnFoldJobC * len(cases))()
    bufs = []
    for slot, (n, w, b, gamma, beta, mu, var, eps) in zip(table, cases):
        bw = [Buf(w, 1 if n == "b0" else 0)] + [Buf(v) for v in (b, gamma, beta, mu, var)]
        bufs.append(bw)
        slot.w = desc(bw[0], n == "tr")
        slot.bias, slot.gamma, slot.beta, slot.mean, slot.var = (x.view.data_ptr() for x in bw[1:])
        slot.eps, slot.forward = eps, 1 if n == "b4" else 0
    status = torch.zeros(len(cases), dtype=torch.int32, device=DEV)
    _native.call("aimet_dfq_bn_fold", table, len(cases), ctypes.c_void_p(status.data_ptr()), stream())
    torch.cuda.synchronize()
    assert _dfq.launch_count() == before + 1
    assert not status.cpu().any()
    for (n, w, b, gamma, beta, mu, var, eps), bw in zip(cases, bufs):
        got_w, got_b = bw[0].get(), bw[1].get()
        for x, v in zip(bw[2:], (gamma, beta, mu, var)):
            assert same(x.get(), v)
        if n == "b4":
            want_w, want_b, _ = O.bn_fold_forward(w, b, gamma, beta, mu, var, eps)
            _, b64, terms = O.bn_fold_forward(w, b, gamma, beta, mu, var, eps, f64=True)
            assert same(got_w, want_w) and same(got_w, golden["b4_w_out"])
            nterms = 2 * w[0].size + 1
            assert np.all(np.abs(got_b - b64) <= nterms * EPS32 * terms)
            assert same(got_b, want_b), "the oracle adds in the kernel's order"
            continue
        want_w, want_b = O.bn_fold_backward(w, b, gamma, beta, mu, var, eps, transposed=(n == "tr"))
        assert same(got_w, want_w) and same(got_b, want_b), n
        if n != "tr":
            assert same(got_w, golden[n + "_w_out"]) and same(got_b, golden[n + "_b_out"]), n


def test_bn_forward_fold_wide_sum_repeats():
    """More input channels than lanes: the striding partials and the tree; float64 bound; two runs equal."""
    rng = np.random.default_rng(11)
    cin, cout, k = 300, 5, 4
    w = rng.standard_normal((cout, cin, 2, 2)).astype(F)
    b = rng.standard_normal(cout).astype(F)
    gamma, beta, mu = (rng.standard_normal(cin).astype(F) for _ in range(3))
    var = rng.uniform(0.2, 2, cin).astype(F)
    outs = []
    for _ in range(2):
        bw = [Buf(v) for v in (w, b, gamma, beta, mu, var)]
        job = (DfqBnFoldJobC * 1)()
        job[0].w = desc(bw[0])
        job[0].bias, job[0].gamma, job[0].beta, job[0].mean, job[0].var = (x.view.data_ptr() for x in bw[1:])
        job[0].eps, job[0].forward = 1e-5, 1
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        _native.call("aimet_dfq_bn_fold", job, 1, ctypes.c_void_p(status.data_ptr()), stream())
        torch.cuda.synchronize()
        outs.append((bw[0].get(), bw[1].get()))
    assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1])
    want_w, want_b, _ = O.bn_fold_forward(w, b, gamma, beta, mu, var, 1e-5)
    _, b64, terms = O.bn_fold_forward(w, b, gamma, beta, mu, var, 1e-5, f64=True)
    assert same(outs[0][0], want_w)
    assert np.all(np.abs(outs[0][1] - b64) <= (2 * cin * k + 1) * EPS32 * terms)
    assert same(outs[0][1], want_b)


def test_bn_fold_zero_sigma_is_reported():
    conv, bn = nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4)
    m = nn.Sequential(conv, bn).to(DEV).eval()
    with torch.no_grad():
        bn.running_var[2] = -float(np.float32(bn.eps))
    w = conv.weight.detach().clone()
    with pytest.raises(ValueError, match="zero"):
        BNF.fold_given_batch_norms(m, [(conv, bn)])
    assert torch.equal(conv.weight[2], w[2]) and isinstance(m[1], nn.BatchNorm2d)


@pytest.mark.parametrize("n", PAIR_CASES)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
def test_cls_pair_bit_equal(golden, n, off):
    c = pair_case(golden, n)
    want = O.cls_pair(**c)
    got = run_pair(c["w0"], c["b0"], c["w1"], c["t0"], c["t1"], off)
    assert same(got[0], want[0]), "scales"
    assert same(got[1], want[1]) and same(got[3], want[3]), "weights"
    assert (c["b0"] is None and got[2] is None) or same(got[2], want[2])
    if n == "p6":
        assert same(got[0][golden["p6_special"]], np.ones(3, F))
        for ch in golden["p6_special"]:     # scale 1: the channel's bits are untouched
            assert same(got[1][ch], c["w0"][ch]) and same(got[3][:, ch], c["w1"][:, ch])


@pytest.mark.parametrize("biases", [(True, True), (False, True), (True, False), (False, False)])
def test_cls_triple_bit_equal(golden, biases):
    g = golden
    b0 = g["t0_b0"] if biases[0] else None
    b1 = g["t0_b1"] if biases[1] else None
    want = O.cls_triple(g["t0_w0"], b0, g["t0_w1"], b1, g["t0_w2"])
    W = [Buf(g["t0_w0"]), Buf(g["t0_w1"], 1), Buf(g["t0_w2"])]
    B = [None if b is None else Buf(b) for b in (b0, b1)]
    S = [Buf(np.zeros(10, F)), Buf(np.zeros(10, F))]
    _native.call("aimet_dfq_cls_triple", desc(W[0]), opt(B[0]), desc(W[1]), opt(B[1]), desc(W[2]), S[0].ptr, S[1].ptr,
                 stream())
    torch.cuda.synchronize()
    s12, s23 = S[0].get(), S[1].get()
    # a device cbrt that rounds differently from np.cbrt on a fixture value would show here first
    assert same(s12, want[0]) and same(s23, want[1]), (s12, want[0], s23, want[1])
    assert same(W[0].get(), want[2]) and same(W[1].get(), want[4]) and same(W[2].get(), want[6])
    for buf, w in zip(B, (want[3], want[5])):
        assert buf is None or same(buf.get(), w)


def run_hbf(case, t2=False):
    gamma, beta, s, relu, b1, w2, b2 = case
    bufs = [Buf(v) for v in (gamma, beta, s, b1, w2, b2)]
    _native.call("aimet_dfq_bias_fold", bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, gamma.size, int(relu), bufs[3].ptr,
                 desc(bufs[4], t2), bufs[5].ptr, stream())
    torch.cuda.synchronize()
    assert same(bufs[4].get(), w2)
    return bufs[3].get(), bufs[5].get()


def check_hbf(case, t2=False):
    v = O._logical(case[5], t2)
    nterms = v.shape[1] * v.shape[2] + 1
    want_b1, want_b2, _ = O.bias_fold(*case, t2=t2)
    _, b64, terms = O.bias_fold(*case, t2=t2, f64=True)
    first, second = run_hbf(case, t2), run_hbf(case, t2)
    assert same(first[0], second[0]) and same(first[1], second[1])
    assert same(first[0], want_b1)
    assert np.all(np.abs(first[1] - b64) <= nterms * EPS32 * terms)
    assert same(first[1], want_b2), "the oracle adds in the kernel's order"


@pytest.mark.parametrize("n", HBF_CASES)
def test_bias_fold_fixture(golden, n):
    check_hbf(hbf_case(golden, n))
    assert same(run_hbf(hbf_case(golden, n))[0], golden[n + "_b1_out"])


@pytest.mark.parametrize("relu", [True, False])
def test_bias_fold_wide_and_transposed(relu):
    rng = np.random.default_rng(23)
    C = 300
    gamma, s = rng.uniform(0.1, 1, C).astype(F), rng.uniform(0.3, 3, C).astype(F)
    beta, b1 = (rng.standard_normal(C) * 2).astype(F), rng.standard_normal(C).astype(F)
    check_hbf((gamma, beta, s, relu, b1, rng.standard_normal((7, C, 3)).astype(F), rng.standard_normal(7).astype(F)))
    # ConvTranspose layout [in C][out 7][k]
    check_hbf((gamma, beta, s, relu, b1, rng.standard_normal((C, 7, 2, 2)).astype(F),
               rng.standard_normal(7).astype(F)), t2=True)


# ---------------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------------
def test_scaled_pair_has_equal_ranges_and_rescaling_is_identity(golden):
    for n in PAIR_CASES:
        c = pair_case(golden, n)
        s, w0, b0, w1 = run_pair(c["w0"], c["b0"], c["w1"], c["t0"], c["t1"])
        r0 = np.abs(O._logical(w0, c["t0"])).max(axis=(1, 2))
        r1 = np.abs(O._logical(w1, c["t1"])).max(axis=(0, 2))
        normal = np.ones(s.size, bool)
        if n == "p6":
            normal[golden["p6_special"]] = False
        # five roundings, each at most half an ulp on either side
        assert O.ulp_distance(r0[normal], r1[normal]) <= 8, n
        s2 = run_pair(w0, b0, w1, c["t0"], c["t1"])[0]
        assert O.ulp_distance(s2[normal], np.ones(int(normal.sum()), F)) <= 8, n
        assert same(s2[~normal], np.ones(int((~normal).sum()), F))


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
class SmallNet(nn.Module):
    """Three conv/BN/ReLU blocks: a plain chain, a residual block and a depthwise-separable triple."""

    def __init__(self):
        super().__init__()
        def bn(c):
            return nn.BatchNorm2d(c)
        self.c1, self.b1, self.r1 = nn.Conv2d(3, 12, 3, padding=1, bias=False), bn(12), nn.ReLU()
        self.c2, self.b2, self.r2 = nn.Conv2d(12, 16, 3, padding=1), bn(16), nn.ReLU()
        self.c3, self.b3, self.r3 = nn.Conv2d(16, 16, 3, padding=1, bias=False), bn(16), nn.ReLU()
        self.c4, self.b4 = nn.Conv2d(16, 16, 1, bias=False), bn(16)
        self.r4 = nn.ReLU()
        self.c5, self.b5, self.r5 = nn.Conv2d(16, 10, 1, bias=False), bn(10), nn.ReLU6()
        self.c6, self.b6, self.r6 = nn.Conv2d(10, 10, 3, padding=1, groups=10, bias=False), bn(10), nn.ReLU6()
        self.c7, self.b7 = nn.Conv2d(10, 7, 1, bias=False), bn(7)

    def forward(self, x):
        x = self.r1(self.b1(self.c1(x)))
        y = self.r2(self.b2(self.c2(x)))                      # y: the residual branch
        z = self.b4(self.c4(self.r3(self.b3(self.c3(y)))))
        x = self.r4(z + y)
        x = self.r6(self.b6(self.c6(self.r5(self.b5(self.c5(x))))))
        return self.b7(self.c7(x))


def seeded(model, seed=3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / m.weight[0].numel()) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(torch.exp(torch.rand(n, generator=g) * 3.0 - 2.0))
                m.bias.copy_(torch.randn(n, generator=g) * 0.5)
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
    return model.eval()


def np_(t):
    return t.detach().cpu().numpy()


def put(param, a):
    with torch.no_grad():
        param.copy_(torch.from_numpy(np.ascontiguousarray(a, F)).reshape(param.shape))


def oracle_equalize(model, hbf=True):
    """fold_all_batch_norms then equalize_model, on a CPU model, by the numpy oracle, over the pairs
    and sets the product's graph search finds. hbf=False stops before the high-bias fold: up to
    there the transform keeps the function exactly (HBF moves what it takes for the bulk of a
    ReLU's input into the next bias, which inputs far from the BatchNorm statistics do not honour)."""
    _dfq.replace_modules(model, lambda m: isinstance(m, nn.ReLU6), lambda m: nn.ReLU())
    conv_bn, bn_conv, _ = BNF._find_all_batch_norms_to_fold(model)
    assert not bn_conv
    for conv, bn in conv_bn:
        if conv.bias is None:
            conv.bias = nn.Parameter(torch.zeros(conv.out_channels))
        w, b = O.bn_fold_backward(np_(conv.weight), np_(conv.bias), np_(bn.weight), np_(bn.bias), np_(bn.running_mean),
                                  np_(bn.running_var), bn.eps)
        put(conv.weight, w)
        put(conv.bias, b)
    folded = {id(bn) for _, bn in conv_bn}
    _dfq.replace_modules(model, lambda m: id(m) in folded, lambda m: nn.Identity())
    bn_of = {conv: bn for conv, bn in conv_bn}
    search = CLE.GraphSearchUtils(model)
    sets = [s for grp in search.find_layer_groups_to_scale()
            for s in CLE.GraphSearchUtils.convert_layer_group_to_cls_sets(grp)]
    relus = search.is_relu_activation_present_in_cls_sets(sets)
    pairs = []
    for layers, relu in zip(sets, relus):
        if len(layers) == 2:
            s, w0, b0, w1 = O.cls_pair(np_(layers[0].weight), np_(layers[0].bias), np_(layers[1].weight))
            put(layers[0].weight, w0), put(layers[0].bias, b0), put(layers[1].weight, w1)
            pairs.append((layers[0], layers[1], s, relu))
        else:
            s12, s23, w0, b0, w1, b1, w2 = O.cls_triple(np_(layers[0].weight), np_(layers[0].bias),
                                                        np_(layers[1].weight), np_(layers[1].bias),
                                                        np_(layers[2].weight))
            put(layers[0].weight, w0), put(layers[0].bias, b0), put(layers[1].weight, w1)
            put(layers[1].bias, b1), put(layers[2].weight, w2)
            pairs += [(layers[0], layers[1], s12, relu[0]), (layers[1], layers[2], s23, relu[1])]
    for l1, l2, s, relu in pairs if hbf else []:
        bn = bn_of[l1]
        b1, b2, _ = O.bias_fold(np_(bn.weight), np_(bn.bias), s, relu, np_(l1.bias), np_(l2.weight), np_(l2.bias))
        put(l1.bias, b1), put(l2.bias, b2)
    return sets


def rel_err(out, ref64):
    return float((out.double() - ref64).abs().max() / ref64.abs().max())


def function_errors(original, transformed_cpu, x):
    """(error of the transformed fp32 model, error of the untouched fp32 model), both against a float64
    evaluation of the original (its ReLU6 replaced by ReLU, as equalize_model does first)."""
    base = copy.deepcopy(original)
    _dfq.replace_modules(base, lambda m: isinstance(m, nn.ReLU6), lambda m: nn.ReLU())
    with torch.no_grad():
        ref64 = copy.deepcopy(base).double()(x.double())
        return rel_err(transformed_cpu(x), ref64), rel_err(base(x), ref64)


def assert_same_parameters(got, want):
    g, w = dict(got.named_parameters()), dict(want.named_parameters())
    assert sorted(g) == sorted(w)
    for k in w:
        assert same(np_(g[k]), np_(w[k])), k


def test_small_model_equals_oracle_and_keeps_its_function():
    original = seeded(SmallNet())
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    want = copy.deepcopy(original)
    sets = oracle_equalize(want)
    # c1-c2 (the chain ends where y fans out), c3-c4 (it ends at the add), c5-c6-c7
    assert [len(s) for s in sets] == [2, 2, 3]
    assert sets[0] == (want.c1, want.c2) and sets[1] == (want.c3, want.c4) and sets[2][1] is want.c6

    m = copy.deepcopy(original).to(DEV)
    _dfq.launch_count(reset=True)
    folded = BNF.fold_all_batch_norms(m)
    assert len(folded) == 7 and _dfq.launch_count() == 1
    assert not any(isinstance(x_, nn.BatchNorm2d) for x_ in m.modules()) and m.c1.bias is not None
    bn_dict = {conv: bn for conv, bn in folded}
    CLE.equalize_bn_folded_model(m, None, folded)
    # one launch per set, one per HBF pair (a pair has one, the triple two)
    assert _dfq.launch_count() == 1 + 3 + 4
    assert not any(isinstance(x_, nn.ReLU6) for x_ in m.modules()) and len(bn_dict) == 7
    got = copy.deepcopy(m).cpu()
    assert_same_parameters(got, want)

    # the same through equalize_model on a CPU-resident model (staged through HBM and copied back)
    host = copy.deepcopy(original)
    CLE.equalize_model(host)
    assert next(host.parameters()).device.type == "cpu"
    assert_same_parameters(host, want)

    e_oracle, e_fp32 = function_errors(original, want, x)
    e_gpu, _ = function_errors(original, got, x)
    print("small model: oracle-transformed %.3e, untouched fp32 %.3e, ratio %.3f; GPU-transformed %.3e, ratio %.3f"
          % (e_oracle, e_fp32, e_oracle / e_fp32, e_gpu, e_gpu / e_fp32))
    assert e_gpu / e_fp32 <= 2 * (e_oracle / e_fp32)

    # fold + cross-layer scaling alone keep the function to rounding: the same criterion, which here bites
    want_cls = copy.deepcopy(original)
    oracle_equalize(want_cls, hbf=False)
    m2 = copy.deepcopy(original).to(DEV)
    _dfq.replace_modules(m2, lambda x_: isinstance(x_, nn.ReLU6), lambda x_: nn.ReLU())
    BNF.fold_all_batch_norms(m2)
    infos = CLE.CrossLayerScaling.scale_model(m2)
    assert [len(i.cls_pair_info_list) for i in infos] == [1, 1, 2]
    assert [p.relu_activation_between_layers for i in infos for p in i.cls_pair_info_list] == [True] * 4
    got_cls = copy.deepcopy(m2).cpu()
    assert_same_parameters(got_cls, want_cls)
    c_oracle, _ = function_errors(original, want_cls, x)
    c_gpu, _ = function_errors(original, got_cls, x)
    print("small model, fold + CLS: oracle-transformed %.3e (ratio %.3f), GPU-transformed %.3e"
          % (c_oracle, c_oracle / e_fp32, c_gpu))
    assert c_oracle / e_fp32 < 16 and c_gpu / e_fp32 <= 2 * (c_oracle / e_fp32)


def test_scale_factors_are_numpy_and_explicit_sets_need_no_graph():
    a, b = nn.Conv2d(3, 5, 3).to(DEV), nn.ConvTranspose2d(5, 4, 3).to(DEV)
    wa, ba, wb = np_(a.weight), np_(a.bias), np_(b.weight)
    s = CLE.CrossLayerScaling.scale_cls_set((a, b))
    want = O.cls_pair(wa, ba, wb, False, True)
    assert isinstance(s, np.ndarray) and s.dtype == np.float32 and same(s, want[0])
    assert same(np_(a.weight), want[1]) and same(np_(a.bias), want[2]) and same(np_(b.weight), want[3])
    info = CLE.CrossLayerScaling.create_cls_set_info_list([(a, b)], [s], [True])
    bn = nn.BatchNorm2d(4)           # a BatchNorm whose length differs from the scale's: fold-forward networks
    with pytest.raises(ValueError, match="fold-forward"):
        CLE.HighBiasFold.bias_fold(info, {a: bn})
    a1 = nn.Conv1d(3, 6, 5, bias=False).to(DEV)
    b1 = nn.Conv1d(6, 4, 3).to(DEV)
    w0, w1 = np_(a1.weight), np_(b1.weight)
    s1 = CLE.CrossLayerScaling.scale_cls_set_with_conv_layers((a1, b1))
    w = O.cls_pair(w0, None, w1)
    assert same(s1, w[0]) and same(np_(a1.weight), w[1]) and same(np_(b1.weight), w[3]) and a1.bias is None


def test_quantsim_on_folded_resnet50_sees_no_batch_norm():
    from aimet_amd.quantsim import QuantizationSimModel
    from workloads.resnet import resnet50
    m = resnet50(device=DEV)
    x = torch.randn(2, 3, 64, 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    with torch.no_grad():
        before = m(x)
    _dfq.launch_count(reset=True)
    pairs = BNF.fold_all_batch_norms(m)
    assert len(pairs) == 53 and _dfq.launch_count() == 1
    with torch.no_grad():
        after = m(x)
    assert float((after - before).abs().max()) <= 1e-3 * float(before.abs().max())
    sim = QuantizationSimModel(m, x)
    wrapped = [w.get_original_module() for _, w in sim.quant_wrappers()]
    assert wrapped and not any(isinstance(w, nn.BatchNorm2d) for w in wrapped)
    sim.compute_encodings(lambda model, _: model(x), None)
    with torch.no_grad():
        assert torch.isfinite(sim.model(x)).all()


def test_equalize_mobilenet_v2_bn():
    from workloads.mobilenet_v2_bn import mobilenet_v2_bn
    original = mobilenet_v2_bn()
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    want = copy.deepcopy(original)
    sets = oracle_equalize(want)
    n_pairs = sum(len(s) - 1 for s in sets)
    m = copy.deepcopy(original).to(DEV)
    _dfq.launch_count(reset=True)
    CLE.equalize_model(m)
    torch.cuda.synchronize()
    # one BN-fold launch, one launch per CLS set, one per high-bias-fold pair
    assert len(sets) == 19 and _dfq.launch_count() == 1 + len(sets) + n_pairs
    got = copy.deepcopy(m).cpu()
    assert all(torch.isfinite(p).all() for p in got.parameters())
    assert not any(isinstance(x_, (nn.BatchNorm2d, nn.ReLU6)) for x_ in got.modules())
    e_oracle, e_fp32 = function_errors(original, want, x)
    e_gpu, _ = function_errors(original, got, x)
    print("mobilenet_v2_bn: oracle-transformed %.3e, untouched fp32 %.3e, ratio %.3f; GPU-transformed %.3e"
          % (e_oracle, e_fp32, e_oracle / e_fp32, e_gpu))
    assert e_gpu / e_fp32 <= 2 * (e_oracle / e_fp32)
