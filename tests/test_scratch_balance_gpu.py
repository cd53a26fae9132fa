"""Every entry point that takes temporary device blocks hands them back before it returns.

aimet_scratch_live counts the blocks of the scratch cache that are handed out and not yet released.
Each case here reads it, makes one call at the smallest shape that takes a scratch-using path of the
library, and reads it again without synchronising: the count must not have moved. The call's result
is compared, bit for bit, with the oracle where an existing test has that comparison a line away,
and otherwise with a second run of the same call on the same inputs. aimet_scratch_taken, the blocks
handed out since the process began, says that the call took the path the case means: each case
names the blocks that path takes, and a shape that drifted onto a path without them fails.

Error paths are not run here (nothing provokes a failing launch): tests/test_scratch_handle.py checks
the owner's behaviour under an exception on the host."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import bits, gpu_available
from oracle import oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _native  # noqa: E402
from aimet_amd._native import (BcAnalyticalJobC, BnreFinishJobC, BnreFoldScaleJobC, DfqBnFoldJobC,  # noqa: E402
                               DfqWeightC, TfEncodingC)

DEV = "cuda"


def live():
    blocks, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _native.call("aimet_scratch_live", ctypes.byref(blocks), ctypes.byref(nbytes))
    assert (blocks.value == 0) == (nbytes.value == 0) and blocks.value >= 0
    return blocks.value


def taken():
    blocks = ctypes.c_int64(-1)
    _native.call("aimet_scratch_taken", ctypes.byref(blocks))
    return blocks.value


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def rand(seed, *shape, off=0):
    """N(0, 1) of `shape` whose first element sits `off` floats past a 16-byte boundary."""
    n = int(np.prod(shape))
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.randn(n + 4, device=DEV, generator=g)
    assert buf.data_ptr() % 16 == 0
    return buf[off:off + n].view(*shape)


def raw(t):
    return t.detach().contiguous().cpu().view(torch.uint8)


def balanced(case, blocks):
    """case() -> (call, outputs): fresh inputs, the one library call, the tensors it wrote. Twice: the
    call takes `blocks` scratch blocks, the live count is unchanged right behind it, and both runs'
    outputs are equal; returns the first's."""
    runs = []
    for _ in range(2):
        call, outputs = case()
        before, had = live(), taken()
        call()
        assert live() == before
        assert taken() - had == blocks
        runs.append(list(outputs))
    assert len(runs[0]) > 0
    for a, b in zip(*runs):
        assert torch.equal(raw(a), raw(b))
    return runs[0]


# ---------------------------------------------------------------------------------------------------
# QuantAnalyzer, bias correction, BatchNorm re-estimation, data-free quantization
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_off", [1, 2], ids=["equal_phase", "different_phase"])
def test_qa_sq_err(x_off):
    n = 1000

    def case():
        ref, x = rand(1, n, off=1), rand(2, n, off=x_off)
        acc = torch.zeros(2, dtype=torch.float64, device=DEV)
        return (lambda: _native.call("aimet_qa_sq_err", p(ref), p(x), n, 0, 1.0 / n, p(acc), stream())), [acc]

    acc, = balanced(case, 1)   # the workgroups' partial sums
    assert bool((acc > 0).all())


def test_bc_channel_sums():
    def case():
        x = rand(3, 2, 3, 5)
        acc = torch.zeros(3, dtype=torch.float64, device=DEV)
        return (lambda: _native.call("aimet_bc_channel_sums", p(x), 2, 3, 5, p(acc), stream())), [acc, x]

    acc, x = balanced(case, 1)   # the channel partials
    # ten float32 values per channel added in float64, here and there: nine roundings each, every
    # one at most 2^-53 of the channel's sum of magnitudes
    xd = x.double()
    assert bool(((acc - xd.sum(dim=(0, 2))).abs() <= 18 * 2.0 ** -53 * xd.abs().sum(dim=(0, 2))).all())


def test_bnre_forward_streaming():
    def case():
        x = rand(4, 2, 3, 5)
        y = torch.empty_like(x)
        sums = torch.zeros(2, 3, dtype=torch.float64, device=DEV)
        return (lambda: _native.call("aimet_bnre_forward", p(x), 2, 3, 5, None, None, 1e-5, p(y), p(sums[0]),
                                     p(sums[1]), stream())), [y, sums]

    prev = ctypes.c_int()
    _native.call("aimet_bnre_forward_form", 1, ctypes.byref(prev))   # streaming at every size
    try:
        y, sums = balanced(case, 2)   # the channel partials and the scale / shift pairs (resident: none)
    finally:
        _native.call("aimet_bnre_forward_form", prev.value, None)
    assert bool(torch.isfinite(y).all()) and bool((sums[1] > 0).all())


def test_bnre_finish_one_job():
    C = 3

    def case():
        sums = rand(5, 2, C).double().abs().contiguous()
        mean, var = torch.full((C,), 9.0, device=DEV), torch.full((C,), 9.0, device=DEV)
        table = (BnreFinishJobC * 1)()
        table[0].sum_mean, table[0].sum_var = sums[0].data_ptr(), sums[1].data_ptr()
        table[0].running_mean, table[0].running_var, table[0].C, table[0].count = mean.data_ptr(), var.data_ptr(), C, 2.0
        return (lambda: _native.call("aimet_bnre_finish", table, 1, stream())), [mean, var, sums]

    mean, var, sums = balanced(case, 1)   # the job table
    assert torch.equal(mean, (sums[0] / 2.0).float()) and torch.equal(var, (sums[1] / 2.0).float())


def _fold_job(slot, seed):
    """One backward BatchNorm fold on a (4, 3, 3, 3) weight; returns the tensors it reads and writes."""
    cout, cin, k = 4, 3, 9
    w, b, gamma, beta, mean = (rand(seed + i, *s) for i, s in enumerate([(cout, cin, 3, 3)] + [(cout,)] * 4))
    var = rand(seed + 5, cout).abs() + 0.5
    slot.w = DfqWeightC(w.data_ptr(), cout, cin, k, cin * k, k)
    slot.bias, slot.gamma, slot.beta, slot.mean, slot.var = (t.data_ptr() for t in (b, gamma, beta, mean, var))
    slot.eps, slot.forward = 1e-5, 0
    return [w, b, gamma, beta, mean, var]


def test_dfq_bn_fold_and_fold_scale_one_job():
    def plain():
        table = (DfqBnFoldJobC * 1)()
        t = _fold_job(table[0], 10)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        return (lambda: _native.call("aimet_dfq_bn_fold", table, 1, p(status), stream())), t + [status]

    def scaled():
        table = (BnreFoldScaleJobC * 1)()
        t = _fold_job(table[0].fold, 10)
        lo, hi = -rand(20, 4).abs() - 0.1, rand(21, 4).abs() + 0.1
        table[0].enc_min, table[0].enc_max = lo.data_ptr(), hi.data_ptr()
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        return (lambda: _native.call("aimet_bnre_fold_scale", table, 1, p(status), stream())), t + [status, lo, hi]

    a, b = balanced(plain, 1), balanced(scaled, 1)   # the job table
    assert a[6].item() == 0 and b[6].item() == 0
    # the fold to scale folds the weight and the bias as the plain fold does
    assert torch.equal(raw(a[0]), raw(b[0])) and torch.equal(raw(a[1]), raw(b[1]))
    assert not torch.equal(a[0], rand(10, 4, 3, 3, 3))


def test_bc_analytical_one_job():
    cout, cin, k = 4, 3, 9

    def case():
        w = rand(30, cout, cin, 3, 3)
        wq = (w * 16).round() / 16
        bias = rand(31, cout)
        table = (BcAnalyticalJobC * 1)()
        table[0].w = DfqWeightC(w.data_ptr(), cout, cin, k, cin * k, k)
        table[0].wq, table[0].bias, table[0].gamma, table[0].beta, table[0].activation = \
            wq.data_ptr(), bias.data_ptr(), None, None, 0
        return (lambda: _native.call("aimet_bc_analytical", table, 1, stream())), [bias, w, wq]

    balanced(case, 1)   # the job table


# ---------------------------------------------------------------------------------------------------
# learned grid: the three partial-sum paths of the backward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outer,C,K", [(1, 1, 4096), (1, 2, 1024), (1, 2, 1028)],
                         ids=["per_tensor", "channel_tiles", "channel_split"])
def test_learned_grid_backward(outer, C, K):
    """(1, 2, 1028): K % 1024 != 0 keeps it off the tile form, K % 4 == 0 and 257 quads per channel
    (more than one workgroup's 256) give two slices per channel -- the smallest such C and K."""
    steps = 15.0

    def case():
        x, g = rand(40, outer, C, K) * 0.3, rand(41, outer, C, K)
        delta = torch.rand(C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(42)) * 0.01 + 0.002
        offset = torch.full((C,), -8.0, device=DEV)
        gx, sums = torch.empty_like(x), torch.empty(3 * C, device=DEV)
        return (lambda: _native.call("aimet_lg_backward", p(x), p(g), p(gx), p(sums), outer, C, K, p(delta), p(offset),
                                     ctypes.c_float(steps), None, stream())), [gx, sums, x, g, delta, offset]

    # the partial triples; the scalar channel form and a one-slice split take none
    gx, sums, x, g, delta, offset = balanced(case, 1)
    xr = torch.round(x / delta.view(1, C, 1)) - offset.view(1, C, 1)
    mask = (xr >= 0) & (xr <= steps)
    assert torch.equal(gx, mask.float() * g) and 0 < int(mask.sum()) < mask.numel()
    assert bool(torch.isfinite(sums).all())


# ---------------------------------------------------------------------------------------------------
# AdaRound: backward with the round loss, fused Adam step, one-pass steps without a workspace
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1], ids=["vector_kernel", "scalar_kernel"])
def test_adaround_backward_with_round_loss(off):
    C, K = 4, 256

    def case():
        w, alpha, grad = (rand(0, C, K, off=off).copy_(t) for t in
                          (rand(50, C, K) * 0.05, rand(51, C, K) * 2, rand(52, C, K)))
        out = rand(53, C, K, off=off)
        delta = (w.abs().amax(1) / 127).contiguous()
        offset = torch.full((C,), -128.0, device=DEV)
        loss = torch.zeros(1, device=DEV)
        assert all(t.data_ptr() % 16 == 4 * off for t in (w, alpha, grad, out))
        return (lambda: _native.call("aimet_adaround_backward", p(w), p(alpha), p(grad), p(out), 1, C, K, p(delta),
                                     p(offset), 8, ctypes.c_double(0.01), ctypes.c_double(8.0), p(loss),
                                     stream())), [out, loss]

    out, loss = balanced(case, 1)   # the round loss's partials
    assert bool(torch.isfinite(out).all()) and loss.item() > 0.0


def test_adaround_fused_adam_step():
    C, K, step = 24, 40, 7

    def case():
        w = rand(60, C, K) * 0.05
        alpha, grad = rand(61, C, K), rand(62, C, K) * 1e-3
        d, o = (w.abs().amax(1) / 7).contiguous(), torch.full((C,), -8.0, device=DEV)
        m, v, wq = torch.full_like(alpha, 1e-4), torch.full_like(alpha, 1e-7), torch.empty_like(alpha)
        rb = torch.tensor([[0.01, 10.0, 9.0]] * step, device=DEV)
        ctr = torch.tensor([step - 1, step], dtype=torch.long, device=DEV)
        loss = torch.zeros(1, device=DEV)
        return (lambda: _native.call("aimet_adaround_backward_adam", p(w), p(alpha), p(grad), p(m), p(v), 1, C, K,
                                     p(d), p(o), 4, p(rb), ctypes.c_void_p(ctr.data_ptr() + 8), p(ctr),
                                     ctypes.c_double(1e-3), ctypes.c_double(0.9), ctypes.c_double(0.999),
                                     ctypes.c_double(1e-8), p(loss), p(wq), stream())), [alpha, m, v, wq, loss, ctr]

    alpha, m, v, wq, loss, ctr = balanced(case, 1)   # the round loss's partials
    assert ctr.tolist() == [step, step] and loss.item() > 0.0
    assert not torch.equal(alpha, rand(61, C, K))


def test_adaround_pointwise_step_without_workspace():
    N, Cin, Cout, HW, act, it = 5, 3, 5, 12, 2, 1

    def case():
        x_cache = rand(70, N + 3, Cin, HW).abs()
        w, b, t_cache = rand(71, Cout, Cin), rand(72, Cout) * 0.1, rand(73, N + 3, Cout, HW) * 0.5
        idx = torch.stack([torch.arange(N, device=DEV), torch.arange(N, device=DEV) + 3]).contiguous()
        ctr = torch.tensor([it, -1], dtype=torch.long, device=DEV)
        gw = torch.empty(Cout, Cin, device=DEV)
        return (lambda: _native.call("aimet_adaround_pw_step", p(x_cache), p(t_cache), p(idx), p(ctr),
                                     ctypes.c_void_p(ctr.data_ptr() + 8), p(w), p(b), p(gw), None, N, Cin, Cout, HW,
                                     act, stream())), [gw, ctr]

    gw, ctr = balanced(case, 1)   # the slices a workspace would hold
    assert ctr.tolist() == [it, it + 1] and bool(gw.abs().sum() > 0)


def test_adaround_depthwise_step_without_workspace():
    N, C, H, K, stride, pad, dil, act, it = 5, 7, 13, 3, 2, 0, 1, 0, 1
    OH = (H + 2 * pad - dil * (K - 1) - 1) // stride + 1

    def case():
        x_cache, t_cache = rand(80, N + 3, C, H, H), rand(81, N + 3, C, OH, OH) * 2 + 1
        w, b = rand(82, C, 1, K, K) * 0.3, rand(83, C)
        idx = torch.stack([torch.arange(N, device=DEV), torch.arange(N, device=DEV) + 3]).contiguous()
        ctr = torch.tensor([it, -1], dtype=torch.long, device=DEV)
        gw = torch.empty_like(w)
        return (lambda: _native.call("aimet_adaround_dw_step", p(x_cache), p(t_cache), p(idx), p(ctr),
                                     ctypes.c_void_p(ctr.data_ptr() + 8), p(w), p(b), p(gw), None, N, C, H, H, OH, OH,
                                     K, stride, pad, dil, act, stream())), [gw, ctr]

    gw, ctr = balanced(case, 1)   # the slices a workspace would hold
    assert ctr.tolist() == [it, it + 1] and bool(gw.abs().sum() > 0)


# ---------------------------------------------------------------------------------------------------
# batched encoding searches: TF-Enhanced (split search), MSE, entropy (window walk)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [O.QUANTIZATION_TF_ENHANCED, O.QUANTIZATION_MSE, O.QUANTIZATION_ENTROPY],
                         ids=["tf_enhanced", "mse", "entropy"])
def test_get_encodings_four_channels(scheme):
    """Blocks of the batched search: the job table and the encodings side by side for every scheme;
    TF-Enhanced below 512 channels splits each channel's candidates over workgroups and adds their
    partials (3, one workgroup per channel: 2); the asymmetric entropy search adds the window walks
    (3, symmetric: 2)."""
    C, K = 4, 1000
    blocks = {O.QUANTIZATION_TF_ENHANCED: 3, O.QUANTIZATION_MSE: 2, O.QUANTIZATION_ENTROPY: 3}[scheme]
    x = (rand(90, C, K) * 1.7 + 0.2).contiguous()
    got = []
    for _ in range(2):   # a fresh quantizer each: a second request on one may reuse the first's search
        q = ctypes.c_void_p()
        _native.call("aimet_tq_create", scheme, C, 0, ctypes.byref(q))
        try:
            _native.call("aimet_tq_update_stats", q, p(x), 1, C, K, stream())
            qs = (ctypes.c_void_p * 1)(q)
            encs, valid = (TfEncodingC * C)(), (ctypes.c_int * 1)()
            before, had = live(), taken()
            _native.call("aimet_tq_get_encodings", qs, 1, 8, 0, 0, 0, encs, valid, stream())
            assert live() == before
            assert taken() - had == blocks
            assert valid[0] == 1
            got.append([(e.min, e.max, e.delta, e.offset, e.bw) for e in encs])
        finally:
            _native.call("aimet_tq_destroy", q)
    assert got[0] == got[1]
    xh = x.cpu().numpy()
    for c in range(C):
        a = O.Analyzer(scheme)
        a.update(xh[c])
        assert got[0][c] == a.compute(8, False, False, False).as_tuple(), c


# ---------------------------------------------------------------------------------------------------
# the QcQuantize op: per-channel QDQ (the encoding table) and a one-shot on a permuted block layout
# ---------------------------------------------------------------------------------------------------
def test_qc_op_per_channel_and_permuted_one_shot():
    from aimet_amd.libpymo import TensorQuantizerOpMode as M
    from aimet_amd.onnx_op import qc_quantize_op
    from test_blockwise import _fresh, _info, _tq
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((4, 6, 25)) * 2 + 0.5).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    # per-channel (axis 1) one-shot, then QDQ alone with the encodings it left
    encs = _fresh(6)
    info = _info(encs, _tq(6), M.oneShotQuantizeDequantize, sym=False, per_channel=True, ch=1)
    before = live()
    y0 = qc_quantize_op(info, xt)
    assert live() == before and info.opMode == M.quantizeDequantize
    had = taken()
    y1 = qc_quantize_op(info, xt)
    assert live() == before and taken() - had == 1   # the encoding table
    tab = np.array([[e.min, e.max, e.delta, e.offset] for e in encs], np.float32).T.ravel()
    want = bits(O.qdq_per_channel(x.ravel(), 6, 25, tab))
    np.testing.assert_array_equal(bits(y0.cpu().numpy().ravel()), want)
    np.testing.assert_array_equal(bits(y1.cpu().numpy().ravel()), want)
    # blocks not contiguous: (6, 2), block axis 0 size 2, channel axis 1 -> statistics from a permuted copy
    data = np.asarray([-5.4, 10, -2, 3.5, 23.1, 2., -10, -2, -1, -.1, 0.3, 0.1], np.float32)
    # (against the same one-shot on contiguous blocks, (2, 6), block axis 1 size 3: one block more)
    had = taken()
    qc_quantize_op(_info(_fresh(4), _tq(4), M.oneShotQuantizeDequantize, False, True, 0, 1, 3),
                   torch.from_numpy(data.reshape(2, 6)).cuda())
    contiguous = taken() - had
    encs = _fresh(6)
    info = _info(encs, _tq(6), M.oneShotQuantizeDequantize, False, True, 1, 0, 2)
    before, had = live(), taken()
    y = qc_quantize_op(info, torch.from_numpy(data.reshape(6, 2)).cuda())
    assert live() == before and taken() - had == contiguous + 1
    blocks = data.reshape(3, 2, 2).transpose(0, 2, 1).reshape(6, 2)     # block (b, c) = x[2b:2b+2, c]
    for i, e in enumerate(encs):
        a = O.Analyzer(O.QUANTIZATION_TF)
        a.update(blocks[i])
        w = a.compute(8, False)
        assert (e.min, e.max, e.delta, e.offset, e.bw) == (w.min, w.max, w.delta, w.offset, 8)
    oi = O.broadcast_shape_info((6, 2), 1, 0, 2)
    t = np.array([[e.min, e.max, e.delta, e.offset] for e in encs], np.float32)
    np.testing.assert_array_equal(bits(y.cpu().numpy().ravel()),
                                  bits(O.qdq_broadcast(data, oi["tensor_strides"], oi["encoding_strides"], *t.T)))
