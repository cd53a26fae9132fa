"""BatchNorm re-estimation and BN fold to scale on the GPU (csrc/bn_reest.hip, the fold to scale of
csrc/dfq.hip, aimet_amd/bn_reestimation.py, batch_norm_fold.fold_all_batch_norms_to_scale) against
tests/bnre_oracle.py:

1. aimet_bnre_forward's statistics on both layouts, every load path and split count: the forward
   error bounds of the shifted double sums, repeatability bit for bit, an unaligned base,
   accumulation over calls;
2. its output against the float64 evaluation, in place and out of place;
3. its rejections;
4. aimet_bnre_finish, several BatchNorms in one launch;
5. aimet_bnre_fold_scale against aimet_dfq_bn_fold and the oracle's range rule;
6. reestimate_bn_stats end to end on the fixture network;
7. the recipe (prepare, calibrate, re-estimate, fold to scale) end to end, and the refusals.
Needs an MI355X."""
import ctypes
import json
import logging
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import REPO, bits, gpu_available

import bnre_oracle as O
from test_dfq import BN_BACKWARD, bn_case

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _dfq, _native  # noqa: E402
from aimet_amd import batch_norm_fold as BNF  # noqa: E402
from aimet_amd import bn_reestimation as BNRE  # noqa: E402
from aimet_amd._native import BnreFinishJobC, BnreFoldScaleJobC, DfqBnFoldJobC, DfqWeightC  # noqa: E402
from aimet_amd.qc_quantize_op import LearnedGridQuantWrapper, QcQuantizeWrapper  # noqa: E402
from aimet_amd.quantizers import QuantScheme  # noqa: E402
from aimet_amd.quantsim import DEFAULT_QUANTIZABLE_TYPES, QuantizationSimModel  # noqa: E402
from oracle import torch_ref as T  # noqa: E402

DEV = "cuda"
F = np.float32
GUARD = 8
U = 2.0 ** -53
BN_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "golden_bnre.npz")))


@pytest.fixture(scope="module")
def golden_dfq():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "golden_dfq.npz")))


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Buf:
    """A device copy of `a` whose first element is `off` floats past a 16-byte boundary, between guards."""

    def __init__(self, a, off=0, dtype=torch.float32, guard=777.0):
        a = np.ascontiguousarray(a)
        self.shape, self.off, self.n, self.guard = a.shape, off, a.size, guard
        self.buf = torch.full((2 * GUARD + off + a.size,), guard, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD + off:GUARD + off + a.size]
        self.view.copy_(torch.from_numpy(a.reshape(-1)).to(dtype))
        if dtype == torch.float32:
            assert self.view.data_ptr() % 16 == 4 * off

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def get(self):
        h = self.buf.cpu().numpy()
        lo = GUARD + self.off
        assert np.all(h[:lo] == self.guard) and np.all(h[lo + self.n:] == self.guard), "wrote outside the tensor"
        return h[lo:lo + self.n].reshape(self.shape).copy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def same64(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


SPREADS = [(0.0, 1.0), (64.0, 0.25), (-300.0, 0.05), (1e4, 1e-3)]


def data(shape, seed):
    """Channel c: offset + scale * N(0, 1), (offset, scale) cycling through SPREADS."""
    rng = np.random.default_rng(seed)
    C = shape[1]
    off = np.array([SPREADS[c % 4][0] for c in range(C)]).reshape(1, C, 1)
    scale = np.array([SPREADS[c % 4][1] for c in range(C)]).reshape(1, C, 1)
    return (off + scale * rng.standard_normal(shape)).astype(F)


def affine(C, seed):
    """Random gamma with one negative and one zero entry (where there are channels for them), and beta."""
    rng = np.random.default_rng(seed)
    gamma = rng.uniform(0.5, 2.0, C).astype(F)
    gamma[0] = -gamma[0]
    if C > 1:
        gamma[1] = 0.0
    return gamma, rng.standard_normal(C).astype(F)


def forward(x, gamma=None, beta=None, eps=1e-5, off=0, acc0=None, inplace=False):
    """aimet_bnre_forward on x [outer][C][inner]; returns (y, sum_mean, sum_var), guards checked."""
    outer, C, inner = x.shape
    acc = np.zeros((2, C)) if acc0 is None else np.asarray(acc0, np.float64)
    X = Buf(x, off)
    Y = X if inplace else Buf(np.zeros_like(x), off)
    A = Buf(acc, dtype=torch.float64, guard=555.0)
    G = None if gamma is None else Buf(gamma)
    B = None if beta is None else Buf(beta)
    _native.call("aimet_bnre_forward", X.ptr, outer, C, inner, None if G is None else G.ptr,
                 None if B is None else B.ptr, eps, Y.ptr, p(A.view[:C]), p(A.view[C:]), stream())
    torch.cuda.synchronize()
    if not inplace:
        assert same(X.get(), x), "the input changed"
    a = A.get()
    return Y.get(), a[0], a[1]


def mean_bound(m):
    return (2 * U * m["A_K"] + U * np.abs(m["mean"])).astype(np.float64)


def var_bound(m):
    n = m["n"]
    return (6 * n * U * m["Q_K"] / (n - 1)).astype(np.float64)


def check_statistics(x, off=0):
    m = O.moments(x)
    _, mean1, var1 = forward(x, off=off)
    _, mean2, var2 = forward(x, off=off)
    assert same64(mean1, mean2) and same64(var1, var2), "two runs differ"
    err_m = np.abs(mean1 - m["mean"]).astype(np.float64)
    err_v = np.abs(var1 - m["var_u"]).astype(np.float64)
    print("shape %s off %d: mean err / bound %.3g, var err / bound %.3g"
          % (x.shape, off, (err_m / mean_bound(m)).max(), (err_v / var_bound(m)).max()))
    assert np.all(err_m <= mean_bound(m)), (err_m / mean_bound(m)).max()
    assert np.all(err_v <= var_bound(m)), (err_v / var_bound(m)).max()


# ---------------------------------------------------------------------------------------------------
# 1. statistics
# ---------------------------------------------------------------------------------------------------
# (200, 2, 49): the flat path in two splits. n = 9800 a channel and two channels give
# split_count = min(2048 / 2, ceil(9800 / 8192)) = 2 and chunk = ceil(4900 / 256) * 256 = 5120, so the
# second split holds 4680 elements: `hi` clipped to n, and 4680 = 9 * 512 + 72 leaves lanes 0..71 an odd step.
PLANAR = [(1, 1, 2), (2, 3, 1), (2, 5, 49), (3, 4, 127), (3, 4, 128), (2, 2, 4097), (4, 3, 3136), (32, 7, 196),
          (2, 70, 15), (1, 300, 7), (40, 3, 961), (200, 2, 49)]
# (3, 1000) and (700, 12): vector columns; (700, 12) has LX = 4 and two row splits
INTERLEAVED = [(2, 1), (5, 3), (257, 130), (4096, 7), (64, 8), (9, 1028), (3, 1000), (700, 12)]
UNALIGNED = [(4, 3, 3136), (3, 4, 128), (2, 70, 15), (64, 8, 1), (3, 1000, 1), (5, 3, 1)]
ALL_SHAPES = PLANAR + [(r, c, 1) for r, c in INTERLEAVED]


def ident(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", PLANAR, ids=ident)
@pytest.mark.usefixtures("streaming_form")
def test_statistics_planar(shape):
    check_statistics(data(shape, sum(shape)))


@pytest.mark.parametrize("shape", INTERLEAVED, ids=ident)
@pytest.mark.usefixtures("streaming_form")
def test_statistics_interleaved(shape):
    check_statistics(data((shape[0], shape[1], 1), sum(shape)))


@pytest.mark.parametrize("shape", UNALIGNED, ids=ident)
@pytest.mark.usefixtures("streaming_form")
def test_statistics_unaligned_base(shape):
    check_statistics(data(shape, 7 + sum(shape)), off=1)


@pytest.mark.parametrize("C,inner,unit", [(3, 3136, 1), (70, 15, 1), (130, 1, 64), (8, 1, 64)])
@pytest.mark.usefixtures("streaming_form")
def test_statistics_accumulate_over_calls(C, inner, unit):
    """Three calls (outer 2, 1 and 3 units) onto nonzero accumulators: within the sum of the three
    calls' bounds, plus 2^-53 of the running sum for each of the three additions into it."""
    rng = np.random.default_rng(C + inner)
    acc = np.stack([rng.standard_normal(C) * 50.0, rng.uniform(1.0, 9.0, C)])
    acc0 = acc.copy()
    want = acc0.astype(np.longdouble)
    slack = np.zeros((2, C), np.longdouble)
    for outer in (2, 1, 3):
        x = data((outer * unit, C, inner), 100 + outer)
        m = O.moments(x)
        _, acc_mean, acc_var = forward(x, acc0=acc)
        acc = np.stack([acc_mean, acc_var])
        want = want + np.stack([m["mean"], m["var_u"]])
        slack = slack + np.stack([mean_bound(m), var_bound(m)]) + U * np.abs(want)
    assert np.all(np.abs(acc - want) <= slack), (np.abs(acc - want) / slack).max()
    assert not np.array_equal(acc, acc0)


# ---------------------------------------------------------------------------------------------------
# 2. output
# ---------------------------------------------------------------------------------------------------
def check_output(x, gamma, beta, off=0):
    eps = 1e-5
    a64, b64, y64 = O.forward64(x, gamma, beta, eps)
    y, _, _ = forward(x, gamma, beta, eps, off=off)
    bound = 2.0 ** -22 * (np.abs(x.astype(np.float64) * a64[None, :, None]) + np.abs(b64)[None, :, None])
    err = np.abs(y.astype(np.float64) - y64)
    print("shape %s off %d affine %s: output err / bound %.3g" % (x.shape, off, gamma is not None,
                                                                   (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound), (err / np.maximum(bound, 1e-300)).max()
    y_in, _, _ = forward(x, gamma, beta, eps, off=off, inplace=True)
    assert same(y_in, y), "in place differs from out of place"


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=ident)
@pytest.mark.usefixtures("streaming_form")
def test_output(shape):
    x = data(shape, 3 + sum(shape))
    check_output(x, *affine(shape[1], sum(shape)))
    check_output(x, None, None)


@pytest.mark.parametrize("shape", UNALIGNED, ids=ident)
@pytest.mark.usefixtures("streaming_form")
def test_output_unaligned_base(shape):
    x = data(shape, 11 + sum(shape))
    check_output(x, *affine(shape[1], sum(shape)), off=1)


@pytest.mark.usefixtures("streaming_form")
def test_output_with_differently_aligned_input_and_output():
    """x on a 16-byte boundary, y one float past one: the 4-byte path."""
    x = data((3, 5, 33), 5)
    X, Y = Buf(x), Buf(np.zeros_like(x), 1)
    A = Buf(np.zeros((2, 5)), dtype=torch.float64, guard=555.0)
    _native.call("aimet_bnre_forward", X.ptr, 3, 5, 33, None, None, 1e-5, Y.ptr, p(A.view[:5]), p(A.view[5:]), stream())
    torch.cuda.synchronize()
    want, _, _ = forward(x)
    assert same(Y.get(), want)


@pytest.fixture
def streaming_form():
    _native.call("aimet_bnre_forward_form", 1, None)
    yield
    _native.call("aimet_bnre_forward_form", 0, None)


@pytest.fixture
def resident_form():
    _native.call("aimet_bnre_forward_form", 2, None)
    yield
    _native.call("aimet_bnre_forward_form", 0, None)


RESIDENT = [s for s in ALL_SHAPES if s[0] * s[2] <= 15872]


@pytest.mark.parametrize("shape", RESIDENT, ids=ident)
def test_resident_form(shape, resident_form):
    """One launch per call with the channel held in LDS: the same bounds as the streaming form."""
    x = data(shape, 17 + sum(shape))
    before = BNRE.launch_count()
    check_statistics(x)
    assert BNRE.launch_count() == before + 2
    check_output(x, *affine(shape[1], sum(shape)))


@pytest.mark.parametrize("shape", UNALIGNED, ids=ident)
def test_resident_form_unaligned_base(shape, resident_form):
    x = data(shape, 19 + sum(shape))
    check_statistics(x, off=1)
    check_output(x, None, None, off=1)


def test_forward_form_is_validated():
    lib = _native.load()
    prev = ctypes.c_int(-1)
    assert lib.aimet_bnre_forward_form(3, None) != 0 and lib.aimet_bnre_forward_form(-1, None) != 0
    assert lib.aimet_bnre_forward_form(1, ctypes.byref(prev)) == 0 and prev.value == 0
    assert lib.aimet_bnre_forward_form(0, ctypes.byref(prev)) == 0 and prev.value == 1


# ---------------------------------------------------------------------------------------------------
# 3. rejections
# ---------------------------------------------------------------------------------------------------
def test_forward_rejects_bad_sizes():
    x = Buf(np.ones(64, F))
    y = Buf(np.zeros(64, F))
    acc = Buf(np.zeros(8), dtype=torch.float64)
    lib = _native.load()
    before = BNRE.launch_count()

    def call(outer, C, inner):
        return lib.aimet_bnre_forward(x.ptr, outer, C, inner, None, None, 1e-5, y.ptr, p(acc.view[:4]),
                                      p(acc.view[4:]), None)
    assert call(1, 4, 1) != 0                       # n = 1
    assert call(0, 4, 2) != 0 and call(2, 0, 2) != 0 and call(2, 4, 0) != 0 and call(-2, 4, 2) != 0
    assert call(1 << 20, 4, 1 << 11) != 0           # 2^31 elements per channel
    assert call(2, 4, 2) == 0
    torch.cuda.synchronize()
    assert BNRE.launch_count() == before + 1
    assert np.all(y.get()[16:] == 0)


# ---------------------------------------------------------------------------------------------------
# 4. finish
# ---------------------------------------------------------------------------------------------------
def test_finish_several_batch_norms_in_one_launch():
    rng = np.random.default_rng(4)
    sizes, counts = (1, 3, 130, 2048), (3.0, 100.0, 7.0, 1.0)
    table = (BnreFinishJobC * len(sizes))()
    bufs = []
    for slot, C, count in zip(table, sizes, counts):
        sums = np.stack([rng.standard_normal(C) * 300.0, rng.uniform(0.0, 50.0, C)])
        S = Buf(sums, dtype=torch.float64, guard=555.0)
        M, V = Buf(np.full(C, 9.0, F)), Buf(np.full(C, 9.0, F), 1)
        slot.sum_mean, slot.sum_var = S.view[:C].data_ptr(), S.view[C:].data_ptr()
        slot.running_mean, slot.running_var, slot.C, slot.count = M.view.data_ptr(), V.view.data_ptr(), C, count
        bufs.append((sums, S, M, V))
    before = BNRE.launch_count()
    _native.call("aimet_bnre_finish", table, len(sizes), stream())
    torch.cuda.synchronize()
    assert BNRE.launch_count() == before + 1
    for (sums, S, M, V), count in zip(bufs, counts):
        assert same64(S.get(), sums)
        assert same(M.get(), (sums[0] / count).astype(F)) and same(V.get(), (sums[1] / count).astype(F))


# ---------------------------------------------------------------------------------------------------
# 5. fold to scale
# ---------------------------------------------------------------------------------------------------
def fold_cases(golden, golden_dfq):
    """(name, w, b, gamma, beta, mean, var, eps, enc_min, enc_max, off)"""
    rng = np.random.default_rng(9)
    cases = []
    for k in (0, 1):
        g = {key[4:]: v for key, v in golden.items() if key.startswith("fs%d_" % k)}
        cases.append(("fs%d" % k, g["w"], g["b"], g["gamma"], g["beta"], g["mean"], g["var"], float(g["eps"]),
                      g["enc_min"], g["enc_max"], k))
    for n in BN_BACKWARD:
        w, b, gamma, beta, mu, var, eps = bn_case(golden_dfq, n)
        flat = w.reshape(w.shape[0], -1)
        lo = (flat.min(axis=1) * rng.uniform(0.8, 1.2, w.shape[0])).astype(F)
        hi = (flat.max(axis=1) * rng.uniform(0.8, 1.2, w.shape[0])).astype(F)
        cases.append((n, w, b, gamma, beta, mu, var, eps, lo, hi, 1 if n in ("b0", "b2") else 0))
    return cases


def desc(buf):
    s = buf.shape
    k = int(np.prod(s[2:], dtype=np.int64))
    return DfqWeightC(buf.view.data_ptr(), s[0], s[1], k, s[1] * k, k)


def fill_fold(slot, case):
    name, w, b, gamma, beta, mean, var, eps, lo, hi, off = case
    bufs = [Buf(w, off)] + [Buf(v) for v in (b, gamma, beta, mean, var)]
    slot.w = desc(bufs[0])
    slot.bias, slot.gamma, slot.beta, slot.mean, slot.var = (x.view.data_ptr() for x in bufs[1:])
    slot.eps, slot.forward = eps, 0
    return bufs


def test_fold_scale_equals_the_weight_fold_and_the_range_rule(golden, golden_dfq):
    cases = fold_cases(golden, golden_dfq)
    plain = (DfqBnFoldJobC * len(cases))()
    plain_bufs = [fill_fold(slot, c) for slot, c in zip(plain, cases)]
    status = torch.zeros(len(cases), dtype=torch.int32, device=DEV)
    _native.call("aimet_dfq_bn_fold", plain, len(cases), p(status), stream())

    scaled = (BnreFoldScaleJobC * len(cases))()
    scaled_bufs, ranges = [], []
    for slot, c in zip(scaled, cases):
        scaled_bufs.append(fill_fold(slot.fold, c))
        lo, hi = Buf(c[8]), Buf(c[9], 1)
        slot.enc_min, slot.enc_max = lo.view.data_ptr(), hi.view.data_ptr()
        ranges.append((lo, hi))
    status2 = torch.zeros(len(cases), dtype=torch.int32, device=DEV)
    before, before_dfq = BNRE.launch_count(), _dfq.launch_count()
    _native.call("aimet_bnre_fold_scale", scaled, len(cases), p(status2), stream())
    torch.cuda.synchronize()
    assert BNRE.launch_count() == before + 1 and _dfq.launch_count() == before_dfq
    assert not status.cpu().any() and not status2.cpu().any()
    swapped = 0
    for c, pb, sb, (lo, hi) in zip(cases, plain_bufs, scaled_bufs, ranges):
        name, w, b, gamma, beta, mean, var, eps, enc_min, enc_max, off = c
        assert same(sb[0].get(), pb[0].get()) and same(sb[1].get(), pb[1].get()), name
        for x, v in zip(sb[2:], (gamma, beta, mean, var)):
            assert same(x.get(), v)
        w_out, b_out, want_lo, want_hi, bad = O.fold_scale(w, b, gamma, beta, mean, var, eps, enc_min, enc_max)
        assert not bad and same(sb[0].get(), w_out) and same(sb[1].get(), b_out), name
        assert same(lo.get(), want_lo) and same(hi.get(), want_hi), name
        neg = gamma < 0
        scale = gamma / np.sqrt(var + F(eps))
        assert same(lo.get()[neg], (enc_max * scale)[neg]) and same(hi.get()[neg], (enc_min * scale)[neg])
        swapped += int(neg.sum())
        if name.startswith("fs"):
            assert same(lo.get(), golden[name + "_min_out"]) and same(sb[0].get(), golden[name + "_w_out"])
    assert swapped >= len(cases)


def test_fold_scale_leaves_a_channel_without_spread_alone():
    rng = np.random.default_rng(13)
    w, b = rng.standard_normal((4, 3, 3, 3)).astype(F), rng.standard_normal(4).astype(F)
    gamma, beta, mean = (rng.standard_normal(4).astype(F) for _ in range(3))
    var = np.array([0.5, 0.0, 2.0, 1.0], F)
    lo, hi = -np.arange(1, 5, dtype=F), np.arange(1, 5, dtype=F) * 2
    case = ("z", w, b, gamma, beta, mean, var, 0.0, lo, hi, 0)
    table = (BnreFoldScaleJobC * 1)()
    bufs = fill_fold(table[0].fold, case)
    L, H = Buf(lo), Buf(hi)
    table[0].enc_min, table[0].enc_max = L.view.data_ptr(), H.view.data_ptr()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _native.call("aimet_bnre_fold_scale", table, 1, p(status), stream())
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [1]
    w_out, b_out, want_lo, want_hi, bad = O.fold_scale(w, b, gamma, beta, mean, var, 0.0, lo, hi)
    assert bad and same(bufs[0].get(), w_out) and same(bufs[1].get(), b_out)
    assert same(L.get(), want_lo) and same(H.get(), want_hi)
    assert same(bufs[0].get()[1], w[1]) and bufs[1].get()[1] == b[1] and L.get()[1] == lo[1] and H.get()[1] == hi[1]


# ---------------------------------------------------------------------------------------------------
# 6. reestimate_bn_stats end to end
# ---------------------------------------------------------------------------------------------------
def stats_of(net):
    return {n: tuple(t.detach().cpu().numpy().copy() for t in (getattr(net, n).running_mean, getattr(net, n).running_var,
                                                              getattr(net, n).num_batches_tracked))
            for n in O.BN_NAMES}


def bn_of(net, name):
    m = getattr(net, name)
    return m._module_to_wrap if isinstance(m, QcQuantizeWrapper) else m


def distance(net, exact):
    return max(float(np.abs(t.detach().cpu().numpy().astype(np.float64) - want).max())
               for n in O.BN_NAMES for t, want in zip((bn_of(net, n).running_mean, bn_of(net, n).running_var), exact[n]))


def test_reestimate_end_to_end(golden):
    exact = O.reestimate_float64(golden)
    batches = O.tiny_batches(golden, device=DEV)
    net = O.tiny_net(golden, device=DEV)
    start = stats_of(net)
    flags = [(bn_of(net, n).momentum, bn_of(net, n).training) for n in O.BN_NAMES]
    BNRE.launch_count(reset=True)
    handle = BNRE.reestimate_bn_stats(net, batches)            # num_batches = 100 > len(loader) = 3
    torch.cuda.synchronize()
    assert BNRE.launch_count() == 3 * 3 * 1 + 1                # one launch per fused BN and batch (each channel fits LDS), one finish
    assert handle.fused == 3 and handle.fallback == 0
    assert all(int(getattr(net, n).num_batches_tracked) == 3 for n in O.BN_NAMES)
    assert flags == [(bn_of(net, n).momentum, bn_of(net, n).training) for n in O.BN_NAMES]
    assert all("forward" not in getattr(net, n).__dict__ for n in O.BN_NAMES)

    ref = O.tiny_net(golden, device=DEV)
    O.reestimate_torch(ref, batches)
    d_ours, d_ref = distance(net, exact), distance(ref, exact)
    print("distance to the float64 evaluation: ours %.4g, plain torch %.4g" % (d_ours, d_ref))
    assert d_ours <= 2 * d_ref

    handle.remove()
    after = stats_of(net)
    for n in O.BN_NAMES:
        assert all(np.array_equal(a, b) for a, b in zip(after[n], start[n])), n
        assert same(after[n][0], golden["param_%s.running_mean" % n])


def test_reestimate_uses_the_requested_number_of_batches(golden):
    batches = O.tiny_batches(golden, device=DEV)
    net, ref = O.tiny_net(golden, device=DEV), O.tiny_net(golden, device=DEV)
    BNRE.reestimate_bn_stats(net, batches, num_batches=2)
    BNRE.reestimate_bn_stats(ref, batches[:2])
    for n in O.BN_NAMES:
        assert torch.equal(getattr(net, n).running_mean, getattr(ref, n).running_mean)
        assert torch.equal(getattr(net, n).running_var, getattr(ref, n).running_var)
        assert int(getattr(net, n).num_batches_tracked) == 2


def test_reestimate_restores_everything_when_the_forward_raises(golden):
    batches = O.tiny_batches(golden, device=DEV)
    net = O.tiny_net(golden, device=DEV).eval()
    net.bn2.train()
    net.bn1.momentum = 0.3
    start = stats_of(net)
    calls = []

    def forward_fn(model, batch):
        calls.append(1)
        if len(calls) == 2:
            raise KeyError("second batch")
        return model(batch)
    with pytest.raises(KeyError, match="second batch"):
        BNRE.reestimate_bn_stats(net, batches, forward_fn=forward_fn)
    after = stats_of(net)
    for n in O.BN_NAMES:
        assert all(np.array_equal(a, b) for a, b in zip(after[n], start[n])), n
        assert "forward" not in getattr(net, n).__dict__
    assert [m.training for m in (net, net.conv1, net.bn1, net.bn2, net.bn3)] == [False, False, False, True, False]
    assert (net.bn1.momentum, net.bn2.momentum) == (0.3, 0.1)


class HalfInput(nn.Module):
    """One BatchNorm fed a 16-bit tensor, one fed float32."""

    def __init__(self):
        super().__init__()
        self.conv, self.bn16, self.bn32 = nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.BatchNorm2d(4)

    def forward(self, x):
        y = self.conv(x)
        return self.bn16(y.half()).float() + self.bn32(y)


def test_reestimate_sends_a_half_input_through_torch(golden):
    torch.manual_seed(3)
    net = HalfInput().to(DEV)
    ref = HalfInput().to(DEV)
    ref.load_state_dict(net.state_dict())
    batches = O.tiny_batches(golden, device=DEV)
    handle = BNRE.reestimate_bn_stats(net, batches)
    O.reestimate_torch(ref, batches)
    assert (handle.fused, handle.fallback) == (1, 1)
    # the reference route, the same torch calls in the same order: the same bits
    assert torch.equal(net.bn16.running_mean, ref.bn16.running_mean)
    assert torch.equal(net.bn16.running_var, ref.bn16.running_var)
    # a strided input and an autocast region take that route too
    strided = nn.Sequential(nn.BatchNorm2d(3)).to(DEV)
    h = BNRE.reestimate_bn_stats(strided, [b[:, :, ::2] for b in batches])
    assert (h.fused, h.fallback) == (0, 1)
    with torch.autocast("cuda", dtype=torch.float16):
        h = BNRE.reestimate_bn_stats(O.tiny_net(golden, device=DEV), batches)
    assert (h.fused, h.fallback) == (0, 3)


def test_reestimate_channels_last_and_cpu_resident_models(golden):
    batches = O.tiny_batches(golden, device=DEV)
    net = O.tiny_net(golden, device=DEV)
    BNRE.reestimate_bn_stats(net, batches)
    last = O.tiny_net(golden, device=DEV).to(memory_format=torch.channels_last)
    h = BNRE.reestimate_bn_stats(last, [b.contiguous(memory_format=torch.channels_last) for b in batches])
    assert h.fused == 3
    exact = O.reestimate_float64(golden)
    ref = O.tiny_net(golden, device=DEV)
    O.reestimate_torch(ref, batches)
    assert distance(last, exact) <= 2 * distance(ref, exact)

    cpu = O.tiny_net(golden)
    h = BNRE.reestimate_bn_stats(cpu, O.tiny_batches(golden))
    assert h.fused == 3 and cpu.bn1.running_mean.device.type == "cpu"
    for n in O.BN_NAMES:
        assert same(getattr(cpu, n).running_mean.numpy(), getattr(net, n).running_mean.cpu().numpy())
        assert same(getattr(cpu, n).running_var.numpy(), getattr(net, n).running_var.cpu().numpy())
    h.remove()
    assert same(cpu.bn3.running_var.numpy(), golden["param_bn3.running_var"])


# ---------------------------------------------------------------------------------------------------
# 7. the recipe
# ---------------------------------------------------------------------------------------------------
def config(tmp_path, per_channel=True, symmetric=True):
    cfg = {"defaults": {"ops": {"is_output_quantized": "True"},
                        "params": {"is_quantized": "True", "is_symmetric": str(symmetric)},
                        "strict_symmetric": "False", "per_channel_quantization": str(per_channel)}}
    path = tmp_path / "quantsim_config.json"
    path.write_text(json.dumps(cfg))
    return str(path)


def calibrated_sim(golden, tmp_path, prepare=True, **cfg):
    sim = QuantizationSimModel(O.tiny_net(golden, device=DEV), in_place=True,
                               quant_scheme=QuantScheme.training_range_learning_with_tf_init,
                               config_file=config(tmp_path, **cfg),
                               quantizable_types=DEFAULT_QUANTIZABLE_TYPES + BN_TYPES)
    if prepare:
        assert len(BNF.prepare_for_fold_to_scale(sim)) == 3
    batches = O.tiny_batches(golden, device=DEV)
    sim.compute_encodings(lambda m, _: [m(b) for b in batches], None)
    return sim, batches


def lg_cpu(t, q):
    """The learned-grid quantize-dequantize of a CPU tensor with the quantizer's current range."""
    emin, emax = (v.detach().float().cpu() for v in q._params())
    return T.lg_forward(t, emin, emax, q.bitwidth, q.use_symmetric_encodings, q.use_strict_symmetric,
                        q.is_unsigned_symmetric, q._ch_axis)[0]


class CpuWrapper(nn.Module):
    """A quantization wrapper's eval-mode function in float32 torch on the CPU (oracle/torch_ref.py)."""

    def __init__(self, wrapper):
        super().__init__()
        import copy
        self.wrapper = [wrapper]
        self.module = copy.deepcopy(wrapper._module_to_wrap).cpu().eval()
        with torch.no_grad():
            for name, param in self.module.named_parameters():
                q = wrapper.param_quantizers[name]
                if q.enabled:
                    param.copy_(lg_cpu(param.detach(), q))

    def forward(self, x):
        w = self.wrapper[0]
        if w.input_quantizers[0].enabled:
            x = lg_cpu(x, w.input_quantizers[0])
        y = self.module(x)
        return lg_cpu(y, w.output_quantizers[0]) if w.output_quantizers[0].enabled else y


def cpu_eval(model, x):
    """The sim's eval-mode output re-evaluated on the CPU from its current parameters and ranges."""
    twin = O.TinyNet().eval()
    for name in ("conv1", "bn1", "conv2", "bn2", "fc", "bn3"):
        m = getattr(model, name)
        setattr(twin, name, CpuWrapper(m) if isinstance(m, QcQuantizeWrapper) else nn.Identity())
    with torch.no_grad():
        return twin(x.cpu()).numpy()


def differing(a, b):
    return float(np.mean(a != b)), float(np.abs(a.astype(np.float64) - b).max())


@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "asymmetric"])
def test_recipe_end_to_end(golden, tmp_path, symmetric):
    sim, batches = calibrated_sim(golden, tmp_path, symmetric=symmetric)
    m = sim.model
    assert all(isinstance(getattr(m, n), LearnedGridQuantWrapper) for n in ("conv1", "bn1", "fc", "bn3"))
    with torch.no_grad():                       # what training would have moved
        m.conv1.weight_encoding_max.mul_(1.05)
        m.conv2.weight_encoding_min.mul_(0.96)
        for n in O.BN_NAMES:
            bn_of(m, n).running_mean.add_(0.05)
            bn_of(m, n).running_var.mul_(1.3)
    handle = BNRE.reestimate_bn_stats(m, batches)
    assert handle.fused == 3 and handle.fallback == 0
    x = torch.cat(batches)
    m.eval()
    with torch.no_grad():
        out_before = m(x).cpu().numpy()
    cpu_before = cpu_eval(m, x)

    pairs = [("conv1", "bn1"), ("conv2", "bn2"), ("fc", "bn3")]
    pre = {}
    for conv, bn in pairs:
        cw, b = getattr(m, conv), bn_of(m, bn)
        q = cw.param_quantizers["weight"]
        enc = q.encoding
        lo, hi = (np.array([getattr(e, k) for e in enc], F) for k in ("min", "max"))
        bias = np.zeros(lo.size, F) if cw._module_to_wrap.bias is None else cw._module_to_wrap.bias.detach().cpu().numpy()
        out_q = getattr(m, bn).output_quantizers[0]
        assert out_q.enabled and not cw.output_quantizers[0].enabled
        pre[conv] = dict(w=cw._module_to_wrap.weight.detach().cpu().numpy(), b=bias, lo=lo, hi=hi,
                         bn=[t.detach().cpu().numpy() for t in (b.weight, b.bias, b.running_mean, b.running_var)],
                         eps=b.eps, out=out_q.encoding.to_tuple(), grad=cw.weight_encoding_min.requires_grad)

    before = BNRE.launch_count()
    folded = BNF.fold_all_batch_norms_to_scale(sim)
    torch.cuda.synchronize()
    assert BNRE.launch_count() == before + 1, "one launch for all pairs"
    assert [id(a) for a, _ in folded] == [id(getattr(m, c)) for c, _ in pairs]
    for conv, bn in pairs:
        cw, s = getattr(m, conv), pre[conv]
        assert isinstance(getattr(m, bn), nn.Identity)
        w, b, lo, hi, bad = O.fold_scale(s["w"], s["b"], *s["bn"], s["eps"], s["lo"], s["hi"])
        assert not bad
        assert same(cw._module_to_wrap.weight.detach().cpu().numpy(), w), conv
        assert same(cw._module_to_wrap.bias.detach().cpu().numpy(), b), conv
        assert same(cw.weight_encoding_min.detach().cpu().numpy(), lo), conv
        assert same(cw.weight_encoding_max.detach().cpu().numpy(), hi), conv
        assert cw.weight_encoding_min.requires_grad == s["grad"] and isinstance(cw.weight_encoding_min, nn.Parameter)
        out_q = cw.output_quantizers[0]
        assert out_q.enabled and out_q.encoding.to_tuple() == s["out"]
        assert "bias" in cw.param_quantizers and not cw.param_quantizers["bias"].enabled
        assert cw.param_quantizers["bias"].wrapper_ref is cw and cw.bias_encoding_min is None
    with torch.no_grad():
        out_after = m(x).cpu().numpy()
    cpu_after = cpu_eval(m, x)
    share_dev, max_dev = differing(out_after, out_before)
    share_cpu, max_cpu = differing(cpu_after, cpu_before)
    step = float(m.fc.output_quantizers[0].encoding.delta)
    print("eval output after the fold vs before (%s): device %.4f of %d elements differ, largest %.4g; "
          "CPU evaluation %.4f differ, largest %.4g; output step %.4g; device vs CPU evaluation after: %s"
          % ("symmetric" if symmetric else "asymmetric", share_dev, out_after.size, max_dev, share_cpu, max_cpu, step,
             differing(out_after, cpu_after)))
    assert share_dev <= share_cpu and max_dev <= max_cpu


def test_fold_to_scale_refusals(golden, tmp_path, caplog):
    # the conv's output quantizer enabled (no prepare): warned and skipped, the BatchNorm stays
    sim, _ = calibrated_sim(golden, tmp_path, prepare=False)
    w = sim.model.conv1._module_to_wrap.weight.detach().clone()
    with caplog.at_level(logging.WARNING, logger="aimet_amd.batch_norm_fold"):
        assert BNF.fold_all_batch_norms_to_scale(sim) == []
    assert caplog.text.count("same supergroup") == 3
    assert isinstance(sim.model.bn1, LearnedGridQuantWrapper) and torch.equal(sim.model.conv1._module_to_wrap.weight, w)

    # a per-tensor weight quantizer on a layer with several output channels
    caplog.clear()
    sim, _ = calibrated_sim(golden, tmp_path, per_channel=False)
    with caplog.at_level(logging.WARNING, logger="aimet_amd.batch_norm_fold"):
        assert BNF.fold_all_batch_norms_to_scale(sim) == []
    assert caplog.text.count("per-tensor weight quantizer") == 3 and isinstance(sim.model.bn3, LearnedGridQuantWrapper)

    # an enabled bias quantizer
    caplog.clear()
    sim, _ = calibrated_sim(golden, tmp_path)
    sim.model.conv1.param_quantizers["bias"].enabled = True
    with caplog.at_level(logging.WARNING, logger="aimet_amd.batch_norm_fold"):
        folded = BNF.fold_all_batch_norms_to_scale(sim)
    assert "bias quantizer is enabled" in caplog.text and len(folded) == 2
    assert isinstance(sim.model.bn1, LearnedGridQuantWrapper) and isinstance(sim.model.bn2, nn.Identity)

    # a frozen weight encoding: an error before anything is modified
    sim, _ = calibrated_sim(golden, tmp_path)
    sim.model.conv2.param_quantizers["weight"].freeze_encoding()
    w = sim.model.conv1._module_to_wrap.weight.detach().clone()
    with pytest.raises(RuntimeError, match="frozen"):
        BNF.fold_all_batch_norms_to_scale(sim)
    assert torch.equal(sim.model.conv1._module_to_wrap.weight, w) and isinstance(sim.model.bn1, LearnedGridQuantWrapper)
