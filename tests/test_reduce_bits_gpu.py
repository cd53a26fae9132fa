"""The kernels whose reductions moved onto csrc/reduce.hpp, and whose element code moved onto io16.hpp's
Io<IO>, give the bits that tests/golden/reduce_bits.json records.

The fixture holds one sha256 per case, recorded from the library as it stood before the move
(tests/golden/make_golden_reduce.py). So that a hash cannot enshrine a wrong answer, each case also
checks its output against a host restatement, with the tolerance of the family's own test (equality
wherever the family is exact).

Shapes are the smallest at which the moved code can go wrong: a reduced extent of 1, below 64 (one
partly filled wave), 64 and 65, 255 and 257 (a ragged last wave; a second pass or workgroup), sizes past
a kernel's own threshold (attention's 1024-element wave path, the analyzer's one-workgroup grid, the FP8
search's several workgroups a row), blockwise blocks of 1, 2, 16 and 64 vectors (the lanes of a
segment), and 16-bit tensors that start 2 bytes past a 16-byte boundary with a ragged head and tail.
Inputs that define a combine's outcome: a NaN in a non-first lane (the statistics drop it, the FP8
argmin makes a NaN loss the least, attention's `o > v` never takes it), and equal minima in different
waves (constant, zero and two-valued channels for the MSE and entropy searches; a zero channel for the
FP8 argmin: the first index must win), and a NaN in one channel's span of a cross-layer-scaling pair and
triple (dfq's nan_max keeps it: the channel's scale is 1 and its weights keep their bits). With 12
channels the TF-Enhanced search runs its one-wave workgroups, whose ties the last-arriving workgroup
settles; its multi-wave kernels, with zero and constant channels among 600, are held to the oracle by
test_gpu_parity.py::test_device_search_many_channels.

Hash only, because the restatement cannot express the NaN: `attn_nan_*` (numpy's max propagates a NaN
where the kernel's `o > v` ignores it; the rows without a NaN are still compared).

Not expressible through the C ABI: -0.0 as the whole of wave 0 in adaround.hip's block_sum. Its inputs
are round-loss terms 1 - |2h - 1|^beta >= +0 and partial sums that start from +0, so no wave sum is -0;
the kernel's order (from +0, waves 0..3) is the parent's, and test_adaround_golden holds its bits."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduce_bits.json")
EXTENTS = (1, 37, 64, 65, 255, 257)
FLAGS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1)]
F = np.float32


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def enc_array(encs):
    return np.array([e.to_tuple()[:4] for e in encs], np.float64)


# ---- stats.hip: block_minmax, the statistics' folds ------------------------------------------------
def stats_tensor(n):
    """Per-tensor TF statistics of n values with a NaN in a non-first lane: the NaN is dropped."""
    from aimet_amd import AimetTensorQuantizer
    from aimet_amd.libpymo import QuantizationMode
    from oracle import oracle as O
    x = (np.random.default_rng(100 + n).standard_normal(n) * 3 + 0.25).astype(F)
    if n > 1:
        x[min(n - 1, 33)] = np.nan
    q = AimetTensorQuantizer(QuantizationMode.QUANTIZATION_TF)
    q.updateStats(torch.from_numpy(x).to(DEV), True)
    enc, valid = q.getEncoding(8, False, False, False)
    o = O.Analyzer(O.QUANTIZATION_TF)
    o.update(x[~np.isnan(x)])
    assert valid and enc.to_tuple() == o.compute(8).as_tuple()
    return sha(enc_array([enc]))


def stats_channels(K):
    """Per-channel TF statistics: one workgroup per channel of [2][5][K], a NaN in channels 1 and 3."""
    from aimet_amd import AimetTensorQuantizer
    from aimet_amd.libpymo import QuantizationMode
    from oracle import oracle as O
    C = 5
    x = (np.random.default_rng(200 + K).standard_normal((2, C, K)) * 2 - 0.5).astype(F)
    x[1, 1, K // 2] = np.nan
    x[0, 3, K - 1] = np.nan
    q = AimetTensorQuantizer(QuantizationMode.QUANTIZATION_TF, num_channels=C)
    q.updateStatsPerChannel(torch.from_numpy(x).to(DEV), 1, True)
    encs, valid = q.getEncoding(8, True, False, False)
    assert valid
    for c in range(C):
        o = O.Analyzer(O.QUANTIZATION_TF)
        v = x[:, c].ravel()
        v = v[~np.isnan(v)]
        if v.size:
            o.update(v)
            assert encs[c].to_tuple() == o.compute(8, True).as_tuple(), c
    return sha(enc_array(encs))


# ---- tfe_search.hip, mse_search.hip, entropy_search.hip: the record butterflies ---------------------
def search(scheme_name):
    """Channels whose candidates tie (constant, zero, two-valued, one outlier) beside ordinary ones: the
    first minimum must win. Equal to the oracle's host search."""
    from aimet_amd import AimetTensorQuantizer
    from aimet_amd.libpymo import QuantizationMode
    from oracle import oracle as O
    scheme = getattr(QuantizationMode, scheme_name)
    rng = np.random.default_rng(7)
    C, K = 12, 96
    x = rng.standard_t(3, (C, K)) * rng.uniform(1e-3, 30, (C, 1))
    x[1] = 0.0
    x[3] = 2.5
    x[5] = np.where(np.arange(K) % 2 == 0, -1.0, 1.0)
    x[7] = 0.0
    x[7, 11] = 4.0
    x[9] = np.abs(x[9])
    x = x.astype(F)
    q = AimetTensorQuantizer(scheme, num_channels=C)
    q.updateStatsPerChannel(torch.from_numpy(x).to(DEV), 0, True)
    orcs = []
    for c in range(C):
        o = O.Analyzer(int(scheme))
        o.update(x[c])
        orcs.append(o)
    got = []
    for bw in (4, 8):
        for fl in FLAGS:
            encs, valid = q.getEncoding(bw, *fl)
            assert valid
            for c in range(C):
                assert encs[c].to_tuple() == orcs[c].compute(bw, *fl).as_tuple(), (c, bw, fl)
            got.append(enc_array(encs))
    return sha(*got)


# ---- fp8.hip: absmax fold, the search's wave sums, the argmin ---------------------------------------
def fp8_search(K):
    """[6][K]: channel 1 has a NaN in a non-first lane (max|x| ignores it, every loss is NaN and NaN is the
    least: index 0), channel 2 is zero (every loss equal: index 0), channel 4 two values."""
    from aimet_amd import fp_quantization as FP
    rng = np.random.default_rng(300 + K)
    x = (rng.standard_normal((6, K)) * 1.5).astype(F)
    x[1, K // 2] = np.nan if K > 1 else x[1, 0]
    x[2] = 0.0
    x[4] = np.where(np.arange(K) % 2 == 0, -0.75, 0.75)
    t = torch.from_numpy(x).to(DEV)
    mx = FP.abs_max(t, True, 0).cpu().numpy()
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(mx, np.nanmax(np.abs(x), axis=1))
    best, cands, losses, index = [v.cpu().numpy() for v in FP.mse_search(t, 3, True, 0, details=True)]
    want = torch.argmin(torch.from_numpy(losses), dim=1).numpy()   # first least; a NaN is the least
    np.testing.assert_array_equal(index, want)
    np.testing.assert_array_equal(best, cands[index, np.arange(6)])
    assert index[2] == 0 and (K == 1 or index[1] == 0)
    import test_fp8 as R
    from test_fp8_gpu import loss_bound
    clean = [0, 2, 3, 4, 5]   # the float64 restatement and the bound of test_fp8_gpu.check_search
    want, want_cands, want_mx = R.search_losses(x[clean], 3, 0)
    np.testing.assert_array_equal(mx[clean], want_mx)
    np.testing.assert_array_equal(cands[:, clean].view(np.uint32), want_cands.view(np.uint32))
    err = np.abs(losses[clean].T.astype(np.float64) - want)
    rel = loss_bound(K, 3, FP.SEARCH_EXACT_DIVIDE)
    assert np.all(err <= rel * want), float(np.max(err / np.maximum(want, 1e-300)))
    assert (losses[2] == 0).all()
    return sha(mx, best, cands, losses, index)


# ---- dfq.hip: block_tree with nan_max ----------------------------------------------------------------
def dfq_cls_nan(n, triple):
    """Cross-layer scaling of 4 channels whose spans are n (first layer) and 5 n (last layer) long; a NaN at
    a lane other than 0 in channel 1's first span and channel 3's last span (and channel 0's middle span):
    nan_max keeps it, the scale is 1 and the channel keeps its bits. Equal to dfq_oracle."""
    import dfq_oracle as D
    import test_dfq_gpu as T
    rng = np.random.default_rng(700 + n)
    C, at = 4, min(n - 1, 33)
    w0 = rng.standard_normal((C, n, 1)).astype(F)
    b0 = rng.standard_normal(C).astype(F)
    w2 = rng.standard_normal((5, C, n)).astype(F)
    w0[1, at, 0] = np.nan
    w2[2, 3, at] = np.nan
    if not triple:
        want = D.cls_pair(w0, b0, w2)
        got = T.run_pair(w0, b0, w2, off=1)
        for g, w in zip(got, want):
            assert T.same(g, w)
        assert T.same(got[0][[1, 3]], np.ones(2, F)) and T.same(got[1][1], w0[1]) and T.same(got[3][:, 3], w2[:, 3])
        return sha(*[T.bits(g) for g in got])
    w1 = rng.standard_normal((C, 1, n)).astype(F)
    b1 = rng.standard_normal(C).astype(F)
    w1[0, 0, at] = np.nan
    want = D.cls_triple(w0, b0, w1, b1, w2)
    W = [T.Buf(w0), T.Buf(w1, 1), T.Buf(w2)]
    B = [T.Buf(b0), T.Buf(b1)]
    S = [T.Buf(np.zeros(C, F)), T.Buf(np.zeros(C, F))]
    T._native.call("aimet_dfq_cls_triple", T.desc(W[0]), B[0].ptr, T.desc(W[1]), B[1].ptr, T.desc(W[2]), S[0].ptr,
                   S[1].ptr, T.stream())
    torch.cuda.synchronize()
    got = [S[0].get(), S[1].get(), W[0].get(), B[0].get(), W[1].get(), B[1].get(), W[2].get()]
    for g, w in zip(got, want):
        assert T.same(g, w)
    assert T.same(got[0][[0, 1]], np.ones(2, F)) and T.same(got[1][[0, 3]], np.ones(2, F))
    return sha(*[T.bits(g) for g in got])


# ---- attn_softmax.hip: wave_max (`o > v`), wave_sum, head_of ----------------------------------------
def attn(S, nan):
    import mha_oracle as M
    from aimet_amd.transformers import attn_softmax
    B, H, L = 1, 2, 3
    x = (np.random.default_rng(400 + S).standard_normal((B * H, L, S)) * 2).astype(F)
    if nan:
        x[1, 1, min(S - 1, 40)] = np.nan
    buf = torch.empty(x.size + 4, dtype=torch.float32, device=DEV)
    src = buf[1:1 + x.size].view(B * H, L, S)   # 4 bytes past a 16-byte boundary: ragged head and tail
    src.copy_(torch.from_numpy(x))
    got = attn_softmax(src, B, H, score_enc=(-6.0, 6.0, 8), prob_enc=(0.0, 1.0, 8)).cpu().numpy()
    want = M.attn_softmax(x, B, H, L, S, score_enc=(-6.0, 6.0, 8), prob_enc=(0.0, 1.0, 8))
    clean = ~np.isnan(x).any(axis=2)
    np.testing.assert_array_equal(got[clean].view(np.uint32), np.asarray(want, F)[clean].view(np.uint32))
    return sha(got)


# ---- blockwise.hip: the segmented fold, dmax, Io<IO>, head_of ---------------------------------------
def blockwise(dtype, BL, sbw):
    import test_blockwise_sim_gpu as T
    R, NB = 5, 3
    rng = np.random.default_rng(500 + BL)
    x, x32 = T.data(rng, R * NB * BL, T.DTYPES[dtype])
    flags = T.SYMMETRY["symmetric" if sbw else "asymmetric"]
    got_t, got_y, q, factor = T.device_run(x, R, NB, BL, 4, flags, "out", 1, sbw)   # 1 element past 16 bytes
    if not sbw:
        want_t = T.table_of(T.host_encodings(x32, R * NB, BL, 4, *flags))
        np.testing.assert_array_equal(T.bits(got_t), T.bits(want_t))
    np.testing.assert_array_equal(T.raw(got_y), T.raw(T.host_qdq(x32, got_t, T.DTYPES[dtype])))
    extra = [] if q is None else [q.cpu().numpy(), factor.cpu().numpy()]
    if sbw:   # the row's factor is its largest block delta over 2^sbw; every block scale an integer of it
        np.testing.assert_array_equal(got_t[2].reshape(R, NB).astype(np.float64),
                                      (extra[0].reshape(R, NB) * extra[1][:, None]).astype(F).astype(np.float64))
        assert extra[0].reshape(R, NB).max(axis=1).tolist() == [2 ** sbw] * R
    return sha(got_t, T.raw(got_y), *extra)


# ---- quant_analyzer.hip: block_tree2, Io<IO> ---------------------------------------------------------
def sq_err(n, dtype, offs):
    import test_quant_analyzer_gpu as QA
    g = torch.Generator().manual_seed(600 + n)
    ref = (torch.randn(n, generator=g) * 3.0 + 0.5).to(QA.DTYPES[dtype][0])
    x = (ref.float() + torch.randn(n, generator=g) * 0.05).to(QA.DTYPES[dtype][0])
    got = QA.run(ref, x, dtype, offs, 1.0)
    for v, want in zip(got, QA.O.sq_err(ref, x)):
        assert abs(v - want) <= QA.O.bound(n, want)
    return sha(got)


CASES = {}
for _n in EXTENTS + (70001,):
    CASES["stats_tensor_%d" % _n] = (stats_tensor, _n)
for _n in EXTENTS:
    CASES["stats_channels_%d" % _n] = (stats_channels, _n)
for _s in ("QUANTIZATION_TF_ENHANCED", "QUANTIZATION_MSE", "QUANTIZATION_ENTROPY"):
    CASES["search_" + _s] = (search, _s)
for _n in EXTENTS + (9001,):
    CASES["fp8_search_%d" % _n] = (fp8_search, _n)
for _n in EXTENTS:
    CASES["dfq_cls_nan_pair_%d" % _n] = (dfq_cls_nan, _n, False)
    CASES["dfq_cls_nan_triple_%d" % _n] = (dfq_cls_nan, _n, True)
for _n in EXTENTS + (1024, 1025):   # 1024: the last row length of the wave path
    CASES["attn_%d" % _n] = (attn, _n, False)
for _n in (65, 257, 1025):
    CASES["attn_nan_%d" % _n] = (attn, _n, True)
for _d, _bls in (("bf16", (8, 16, 128, 512, 37)), ("fp32", (4, 8, 64, 256, 37)), ("fp16", (128, 37))):
    for _bl in _bls:   # 1, 2, 16 and 64 vectors a block; 37: a ragged head and tail
        CASES["blockwise_%s_%d" % (_d, _bl)] = (blockwise, _d, _bl, 0)
CASES["blockwise_lpbq_bf16_128"] = (blockwise, "bf16", 128, 4)
CASES["blockwise_lpbq_fp32_37"] = (blockwise, "fp32", 37, 4)
for _n in EXTENTS + (600001,):
    CASES["sq_err_bf16_%d" % _n] = (sq_err, _n, "bf16", (1, 1))
    CASES["sq_err_fp32_%d" % _n] = (sq_err, _n, "fp32", (0, 0))
CASES["sq_err_fp16_elem_257"] = (sq_err, 257, "fp16", (1, 0))

RAN = set()


def run_case(name):
    fn, *args = CASES[name]
    return fn(*args)


@pytest.mark.parametrize("name", list(CASES))
def test_reduce_bits(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(CASES)
    got = run_case(name)
    RAN.add(name)
    assert got == golden[name]


def test_every_case_ran():
    assert RAN == set(CASES)
