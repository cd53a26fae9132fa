"""FP8 fake-quantization on the GPU (csrc/fp8.hip), against the numpy oracle of tests/test_fp8.py:

1. aimet_fp8_scale_table + aimet_fp8_qdq bit for bit, M = 1..6, at the sizes where a tile ends,
   aligned and offset by one element, under every tile shape, per tensor and per channel, special
   values and degenerate maxvals, guard elements around every output;
2. aimet_fp8_absmax + aimet_fp8_mse_search: candidate tables bit for bit, loss sums against float64
   within the float32 summation bound, two runs bit-identical, the chosen candidate against the
   float64 oracle's first minimum wherever best and runner-up are at least GAP apart;
3. end to end through QuantizationSimModel(default_data_type=float), tf and tf_enhanced.
Needs an MI355X."""
import ctypes
import functools
import json
import sys

import numpy as np
import pytest
import torch

from conftest import bits, gpu_available
from test_fp8 import (NUM_CANDIDATES, first_min_and_gap, fp8_alpha, fp8_cast, fp8_cast_channels, fp8_largest,
                      search_losses)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _native  # noqa: E402
from aimet_amd import fp_quantization as F  # noqa: E402

DEV = "cuda"
SHAPES = (64, 128, 256)
GUARD = 8                  # floats before and after every buffer (keeps the payload 16-B aligned)
SENTINEL = 12345.0
MAXVAL = np.float32(3.7)
SIZES = (1, 3, 4, 5, 255, 256, 257, 1027)


@pytest.fixture(params=SHAPES, ids=["lanes%d" % L for L in SHAPES])
def lanes(request):
    prev = ctypes.c_int()
    _native.call("aimet_qdq_tile_lanes", request.param, ctypes.byref(prev))
    yield request.param
    _native.call("aimet_qdq_tile_lanes", prev.value, None)


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded_dev(payload, off=0):
    """A device buffer [guard | off | payload | guard] filled with SENTINEL; returns (buffer, view)."""
    n = payload if isinstance(payload, int) else payload.size
    buf = torch.full((2 * GUARD + off + n,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[GUARD + off:GUARD + off + n]
    if not isinstance(payload, int):
        view.copy_(torch.from_numpy(np.array(payload, np.float32).reshape(-1)))
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return buf, view


def check_guards(buf, off, n, what):
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD + off] == SENTINEL) and np.all(h[GUARD + off + n:] == SENTINEL), \
        "%s: wrote outside its output" % what


def specials(maxval, M):
    """+-0, NaN, +-Inf, the clamps and their neighbours, values on exact rounding ties of the
    quotient (normal and subnormal range) and values far below the smallest step."""
    mv = np.float32(maxval)
    alpha = np.float64(fp8_alpha(mv, M)) if fp8_alpha(mv, M) != 0 else 1.0
    step0 = 2.0 ** (1 - M)                       # the grid step below 2 (the subnormal range and the first binade)
    ties = [0.5 * step0, 1.5 * step0, 2.5 * step0, 2 + 2.0 ** (1 - M) * 0.5, 2 + 2.0 ** (1 - M) * 1.5,
            4 - 2.0 ** (1 - M) * 0.5, fp8_largest(M) * 0.999]
    vals = [0.0, -0.0, np.nan, np.inf, -np.inf, mv, -mv, np.nextafter(mv, np.float32(np.inf)),
            np.nextafter(mv, np.float32(0)), 100 * mv, -100 * mv, 1e-40, -1e-40, 1e-30]
    vals += [t * alpha for t in ties] + [-t * alpha for t in ties] + [0.01 * step0 * alpha, 0.49 * step0 * alpha]
    with np.errstate(all="ignore"):
        return np.array(vals, np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def base(M, maxval=float(MAXVAL)):
    """One seeded host array per M that every case slices: N(0, maxval / 2.5) with the special values
    at its start and strewn through it."""
    n = 1027 + 2
    x = (np.random.default_rng(M).standard_normal(n) * maxval / 2.5).astype(np.float32)
    s = specials(maxval, M)
    x[1:1 + s.size] = s
    k = np.arange(s.size + 7, n, 53)
    x[k] = s[np.arange(k.size) % s.size]
    x.setflags(write=False)
    return x


def scale_table(maxvals, M):
    mv = torch.from_numpy(np.asarray(maxvals, np.float32).reshape(-1)).to(DEV)
    tbuf, table = guarded_dev(2 * mv.numel())
    _native.call("aimet_fp8_scale_table", mv.data_ptr(), mv.numel(), M, table.data_ptr(), stream())
    check_guards(tbuf, 0, 2 * mv.numel(), "scale table")
    return table


# ------------------------------------------------------------------------------------------------
# 1. QDQ
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 6])
def test_scale_table(M):
    mv = np.array([3.7, 1e-3, 1e4, 0.0, -1.0, np.inf, np.nan, 1e-42, 2e-40, 61440.0, 3.4e38], np.float32)
    table = scale_table(mv, M).cpu().numpy().reshape(-1, 2)
    np.testing.assert_array_equal(bits(table[:, 0]), bits(mv))
    np.testing.assert_array_equal(bits(table[:, 1]), bits(fp8_alpha(mv, M)))
    assert fp8_alpha(np.float32(1e-42), 3) == 0 and fp8_alpha(np.float32(2e-40), 3) > 0


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 6])
def test_qdq_per_tensor(lanes, M):
    table = scale_table([MAXVAL], M)
    for n in SIZES:
        for off in (0, 1):   # 16-B aligned (vector kernel + scalar tail) / offset by one element (scalar)
            xh = base(M)[off:off + n]
            _, x = guarded_dev(xh, off)
            obuf, y = guarded_dev(n, off)
            _native.call("aimet_fp8_qdq", x.data_ptr(), y.data_ptr(), 1, 1, n, table.data_ptr(), M, stream())
            what = "M %d lanes %d n %d offset %d" % (M, lanes, n, off)
            np.testing.assert_array_equal(bits(y.cpu().numpy()), bits(fp8_cast(xh, MAXVAL, M)), err_msg=what)
            check_guards(obuf, off, n, what)


@pytest.mark.parametrize("maxval", [0.0, -1.0, float("inf"), float("nan"), 1e-42, 2e-40, 61440.0, 1e-3, 1e4],
                         ids=lambda v: "maxval%g" % v)
def test_qdq_special_maxvals(maxval):
    """No grid (0, negative, Inf, NaN, an alpha that underflows): the clamped input, no NaN made;
    a subnormal alpha, alpha == 1 (values on exact ties) and ordinary ranges: the oracle's bits."""
    for M in (3, 2):
        mv = np.float32(maxval)
        scale = float(mv) if np.isfinite(mv) and mv > 0 else 1.0
        xh = base(M, scale)
        table = scale_table([mv], M)
        _, x = guarded_dev(xh)
        obuf, y = guarded_dev(xh.size)
        _native.call("aimet_fp8_qdq", x.data_ptr(), y.data_ptr(), 1, 1, xh.size, table.data_ptr(), M, stream())
        got = y.cpu().numpy()
        np.testing.assert_array_equal(bits(got), bits(fp8_cast(xh, mv, M)), err_msg="maxval %r M %d" % (maxval, M))
        assert np.array_equal(np.isnan(got), np.isnan(xh)), "NaN exactly where the input is NaN"
        check_guards(obuf, 0, xh.size, "maxval %r" % maxval)


@functools.lru_cache(maxsize=None)
def channel_case(C, K, outer, M):
    rng = np.random.default_rng(1000 * C + 10 * K + outer)
    mv = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), C)).astype(np.float32)
    if C > 2:
        mv[1] = 0.0          # a channel without a grid among the others
    x = (rng.standard_normal((outer, C, K)) * np.maximum(mv, 1e-3)[None, :, None] / 2.5).astype(np.float32)
    flat = x.reshape(-1)
    for c in range(min(C, 4)):
        s = specials(mv[c], M)
        k = np.arange(min(K, s.size))
        x[outer - 1, c, k] = s[k]
    flat.setflags(write=False)
    return x, mv


@pytest.mark.parametrize("M", [3, 2])
@pytest.mark.parametrize("outer", [1, 2])
@pytest.mark.parametrize("K", [1, 3, 4, 8])
@pytest.mark.parametrize("C", [1, 3, 130])
def test_qdq_per_channel(lanes, C, K, outer, M):
    """[outer][C][K]: outer == 2 is a channel axis of 1; K % 4 == 0 takes the vector kernel."""
    x, mv = channel_case(C, K, outer, M)
    table = scale_table(mv, M)
    want = fp8_cast_channels(x, mv, M, 1)
    for off in (0, 1):
        _, xd = guarded_dev(x, off)
        obuf, y = guarded_dev(x.size, off)
        _native.call("aimet_fp8_qdq", xd.data_ptr(), y.data_ptr(), outer, C, K, table.data_ptr(), M, stream())
        what = "C %d K %d outer %d M %d offset %d lanes %d" % (C, K, outer, M, off, lanes)
        np.testing.assert_array_equal(bits(y.cpu().numpy()), bits(want.reshape(-1)), err_msg=what)
        check_guards(obuf, off, x.size, what)


def test_quantize_to_fp8_python():
    """The public function: per tensor, per channel along an inner axis, fp16 / bf16 upcast around
    the kernel, a CPU tensor staged through HBM, the reference's broadcast-shaped maxval."""
    x, mv = channel_case(3, 8, 2, 3)
    xt = torch.from_numpy(np.array(x))
    want = fp8_cast_channels(x, mv, 3, 1)
    got = F.quantize_to_fp8(xt.to(DEV), torch.from_numpy(mv).to(DEV), 3, 1)
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(want))
    got = F.quantize_to_fp8(xt, torch.from_numpy(mv).view(1, 3, 1), torch.Tensor([3]))
    assert not got.is_cuda
    np.testing.assert_array_equal(bits(got.numpy()), bits(want))
    for dt in (torch.float16, torch.bfloat16):
        xh = torch.from_numpy(np.array(base(3)[40:])).to(DEV).to(dt)
        got = F.quantize_to_fp8(xh, torch.tensor(float(MAXVAL)), 3)
        assert got.dtype == dt
        w = torch.from_numpy(fp8_cast(xh.float().cpu().numpy(), MAXVAL, 3)).to(dt)
        np.testing.assert_array_equal(bits(got.float().cpu().numpy()), bits(w.float().numpy()))
    with pytest.raises(ValueError, match="per-channel maxvals"):
        F.quantize_to_fp8(xt.to(DEV), torch.ones(4, device=DEV), 3, 1)


# ------------------------------------------------------------------------------------------------
# 2. range search
# ------------------------------------------------------------------------------------------------
# EPS: the largest relative difference between the kernel's float32 loss sums and the float64
# oracle's over every case, candidate and channel of measure_eps() below, on an MI355X
# (profiles/r09/fp8_eps.txt). GAP = 4 * EPS; channels whose oracle best and runner-up are closer than
# GAP (relative) are not compared, at most MAX_EXCLUDED of a case's channels.
# Measured: 5.637e-6 (a K = 1 channel under the reciprocal, an element on a rounding tie; 1.2e-7 ..
# 3.7e-6 over the other cases; at most 2.4e-7 with the divide), rounded up. The smallest
# best-to-runner-up gap of any channel of the test cases was 6.1e-5.
EPS = 5.7e-6
GAP = 4 * EPS
MAX_EXCLUDED = 0.02
SEARCH_K = (1, 63, 64, 65, 1024)
SEARCH_C = (1, 3, 130)


@functools.lru_cache(maxsize=None)
def search_case(outer, C, K, M, seed=0):
    """(x [outer][C][K], float64 losses [111][C], candidates [111][C], max|x| [C]) -- computed once."""
    rng = np.random.default_rng(100003 * C + 17 * K + outer + 7919 * seed)
    scale = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), C)).astype(np.float32)
    x = (rng.standard_normal((outer, C, K)) * scale[None, :, None]).astype(np.float32)
    if C > 2 and K > 1:
        x[:, 2, :] = 0.0        # an all-zero channel: every candidate is 0, every loss 0, index 0
    losses, cands, mx = search_losses(x, M, 1)
    for a in (x, losses, cands, mx):
        a.setflags(write=False)
    return x, losses, cands, mx


def run_search(x, outer, C, K, M, exact, off=0):
    _, xd = guarded_dev(x, off)
    nbytes = ctypes.c_int64(-1)
    _native.call("aimet_fp8_search_workspace", outer, C, K, ctypes.byref(nbytes))
    assert nbytes.value > 0 and nbytes.value % 4 == 0
    wbuf, ws = guarded_dev(nbytes.value // 4)
    mbuf, mx = guarded_dev(C)
    bbuf, best = guarded_dev(C)
    lbuf, losses = guarded_dev(C * NUM_CANDIDATES)
    cbuf, cands = guarded_dev(C * NUM_CANDIDATES)
    index = torch.full((C + 2,), -7, dtype=torch.int32, device=DEV)
    _native.call("aimet_fp8_absmax", xd.data_ptr(), outer, C, K, mx.data_ptr(), ws.data_ptr(), nbytes.value, stream())
    _native.call("aimet_fp8_mse_search", xd.data_ptr(), outer, C, K, mx.data_ptr(), M, int(exact), best.data_ptr(),
                 losses.data_ptr(), cands.data_ptr(), index[1:].data_ptr(), ws.data_ptr(), nbytes.value, stream())
    torch.cuda.synchronize()
    what = "search %s" % ((outer, C, K, M, exact, off),)
    check_guards(wbuf, 0, nbytes.value // 4, what + " workspace")
    check_guards(mbuf, 0, C, what + " absmax")
    check_guards(bbuf, 0, C, what + " best")
    check_guards(lbuf, 0, C * NUM_CANDIDATES, what + " losses")
    check_guards(cbuf, 0, C * NUM_CANDIDATES, what + " candidates")
    idx = index.cpu().numpy()
    assert idx[0] == -7 and idx[-1] == -7
    return (mx.cpu().numpy(), best.cpu().numpy(), losses.cpu().numpy().reshape(C, NUM_CANDIDATES).T,
            cands.cpu().numpy().reshape(NUM_CANDIDATES, C), idx[1:-1])


def loss_bound(n, M, exact):
    """n non-negative terms per sum, each the square of one rounded subtraction (two roundings),
    fused into the sum, added in any order with n - 1 roundings: (n + 3) * 2^-24 relative, as
    tests/test_seq_mse_gpu.py derives it. With the reciprocal a term may also land on the other
    neighbour of a rounding tie: the quotient is within 2 * 2^-24 relative of the exact one, so the
    two distances differ by at most 4 * 2^-24 * |q| of a half step that is at least 2^-(M+2) * |q|,
    the squares by a factor within 1 + 2^(M+5) * 2^-24, and such terms add up to at most the sum."""
    return (n + 3 + (0 if exact else 2 ** (M + 5))) * 2.0 ** -24


def check_search(outer, C, K, M, exact, off=0):
    x, want, cands, mx = search_case(outer, C, K, M)
    got_mx, best, losses, got_cands, index = run_search(x, outer, C, K, M, exact, off)
    what = "outer %d C %d K %d M %d exact %d offset %d" % (outer, C, K, M, exact, off)
    np.testing.assert_array_equal(bits(got_mx), bits(mx), err_msg=what)
    np.testing.assert_array_equal(bits(got_cands), bits(cands), err_msg=what)
    rel = loss_bound(outer * K, M, exact)
    err = np.abs(losses.astype(np.float64) - want)
    print(what, "max rel err %.3g (bound %.3g)" % (float(np.max(err / np.maximum(want, 1e-300))), rel))
    assert np.all(err <= rel * want), what
    # the kernel's own choice: the first minimum of its own sums, and the candidate at that index
    np.testing.assert_array_equal(index, losses.argmin(0), err_msg=what)
    np.testing.assert_array_equal(bits(best), bits(cands[index, np.arange(C)]), err_msg=what)
    # against the float64 oracle wherever the choice is clear
    first, gap = first_min_and_gap(want)
    compared = (gap >= GAP) | (want.max(0) == 0)     # an all-zero channel: every loss is exactly 0, index 0
    assert int((~compared).sum()) <= MAX_EXCLUDED * C, (what, gap.min())
    np.testing.assert_array_equal(index[compared], first[compared], err_msg=what)
    again = run_search(x, outer, C, K, M, exact, off)
    for a, b in zip((got_mx, best, losses, got_cands), again):
        assert np.array_equal(bits(a), bits(b)), "two runs must give the same bits"
    return float(np.max(err / np.maximum(want, 1e-300))), float(gap.min())


@pytest.mark.parametrize("exact", [1, 0], ids=["divide", "reciprocal"])
@pytest.mark.parametrize("K", SEARCH_K)
@pytest.mark.parametrize("C", SEARCH_C)
def test_search_per_channel(C, K, exact):
    check_search(1, C, K, 3, exact)


@pytest.mark.parametrize("exact", [1, 0], ids=["divide", "reciprocal"])
def test_search_outer_axis_offset_and_m2(exact):
    check_search(2, 3, 65, 3, exact)          # a channel axis of 1
    check_search(2, 130, 63, 2, exact)
    check_search(1, 3, 1024, 2, exact, off=1)  # input offset by one element


@pytest.mark.parametrize("exact", [1, 0], ids=["divide", "reciprocal"])
def test_search_per_tensor_several_workgroups(exact):
    check_search(1, 1, 70001, 3, exact)       # 69 tiles, one workgroup each
    check_search(1, 1, 3 * 1024 + 5, 2, exact)


@pytest.mark.parametrize("elems", [4, 8])
def test_search_with_fewer_elements_per_lane(elems):
    """aimet_fp8_search_elems: the other forms of the pass-one kernel (the default holds 16)."""
    prev = ctypes.c_int()
    _native.call("aimet_fp8_search_elems", elems, ctypes.byref(prev))
    try:
        assert prev.value == 0
        for exact in (1, 0):
            check_search(1, 3, 1024, 3, exact)
            check_search(1, 1, 3 * 1024 + 5, 2, exact)
            check_search(1, 130, 65, 3, exact)
    finally:
        _native.call("aimet_fp8_search_elems", prev.value, None)


def test_search_rejects_bad_arguments():
    x, _, _, _ = search_case(1, 3, 64, 3)
    _, xd = guarded_dev(x)
    nbytes = ctypes.c_int64()
    _native.call("aimet_fp8_search_workspace", 1, 3, 64, ctypes.byref(nbytes))
    ws = torch.empty(nbytes.value // 4, device=DEV)
    mx = torch.empty(3, device=DEV)
    best = torch.empty(3, device=DEV)
    with pytest.raises(ValueError, match="workspace"):
        _native.call("aimet_fp8_mse_search", xd.data_ptr(), 1, 3, 64, mx.data_ptr(), 3, 0, best.data_ptr(), None, None,
                     None, ws.data_ptr(), nbytes.value - 4, stream())
    with pytest.raises(ValueError, match="mantissa"):
        _native.call("aimet_fp8_mse_search", xd.data_ptr(), 1, 3, 64, mx.data_ptr(), 7, 0, best.data_ptr(), None, None,
                     None, ws.data_ptr(), nbytes.value, stream())
    host = np.zeros(8, np.float32)
    with pytest.raises((ValueError, RuntimeError)):
        _native.call("aimet_fp8_absmax", host.ctypes.data, 1, 1, 8, mx.data_ptr(), ws.data_ptr(), nbytes.value,
                     stream())
    torch.cuda.synchronize()


class _Quantizer:
    def __init__(self, channel_axis=0):
        self.channel_axis = channel_axis
        self.fp8_maxval = None


def test_init_functions():
    """init_minmax / init_mse as the reference calls them (tensor, quantizer, per_channel)."""
    x, want, cands, mx = search_case(2, 3, 65, 3)
    xt = torch.from_numpy(np.array(x)).to(DEV)
    q = _Quantizer(1)
    got = F.init_minmax(xt, q, True)
    np.testing.assert_array_equal(got.cpu().numpy(), mx)
    np.testing.assert_array_equal(q.fp8_maxval.cpu().numpy(), mx)     # fp_quantization.py:60
    got = F.init_minmax(xt, _Quantizer(), False)
    assert got.dim() == 0 and float(got) == float(mx.max())
    first, gap = first_min_and_gap(want)
    assert np.all((gap >= GAP) | (want.max(0) == 0))      # channel 2 is all zero: index 0
    got = F.init_mse(xt, q, True)
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(cands[first, np.arange(3)]))
    got = F.init_mse(xt.cpu(), q, True)                               # staged through HBM
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(cands[first, np.arange(3)]))
    xp, wantp, candsp, _ = search_case(1, 1, 70001, 3)
    firstp, gapp = first_min_and_gap(wantp)
    assert gapp[0] >= GAP
    got = F.init_mse(torch.from_numpy(np.array(xp)).to(DEV).view(1, 70001, 1), _Quantizer(), False)
    assert got.shape == (1,) and bits(got.cpu().numpy())[0] == bits(candsp[firstp[0], 0])


def measure_eps(out=sys.stdout):
    """EPS of the comment above: every test case plus longer channels (K up to 16384)."""
    worst, smallest = 0.0, np.inf
    cases = [(1, C, K, 3) for C in SEARCH_C for K in SEARCH_K]
    cases += [(2, 3, 65, 3), (2, 130, 63, 2), (1, 3, 1024, 2), (1, 1, 70001, 3), (1, 1, 3 * 1024 + 5, 2),
              (1, 16, 4096, 3), (1, 8, 16384, 3), (1, 8, 16384, 2), (4, 16, 3136, 3)]
    for exact in (1, 0):
        for outer, C, K, M in cases:
            x, want, cands, mx = search_case(outer, C, K, M)
            _, _, losses, _, index = run_search(x, outer, C, K, M, exact)
            rel = float(np.max(np.abs(losses.astype(np.float64) - want) / np.maximum(want, 1e-300)))
            first, gap = first_min_and_gap(want)
            live = gap[np.isfinite(gap) & (want.min(0) > 0)]
            print("case outer %d C %d K %d M %d %s: eps %.3e min gap %.3e chosen != oracle on %d channels"
                  % (outer, C, K, M, "divide" if exact else "reciprocal", rel, live.min() if live.size else np.inf,
                     int((index != first).sum())), file=out)
            worst = max(worst, rel)
            if live.size:
                smallest = min(smallest, float(live.min()))
    print("EPS %.3e  GAP=4*EPS %.3e  smallest gap %.3e" % (worst, 4 * worst, smallest), file=out)
    return worst


# ------------------------------------------------------------------------------------------------
# 3. end to end
# ------------------------------------------------------------------------------------------------
def make_model():
    torch.manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.Flatten(),
                                torch.nn.Linear(8 * 6 * 6, 10)).to(DEV).eval()
    g = torch.Generator().manual_seed(11)
    batches = [(torch.randn(4, 3, 6, 6, generator=g) * s).to(DEV) for s in (1.0, 2.5)]
    return model, batches


def np_cast(t, maxval, axis=None):
    """The oracle applied to a HIP tensor with the given maxval tensor."""
    x = t.detach().cpu().numpy()
    mv = maxval.detach().cpu().numpy().reshape(-1)
    if mv.size == 1:
        out = fp8_cast(x, mv[0], 3)
    else:
        out = fp8_cast_channels(x, mv, 3, axis)
    return torch.from_numpy(out).to(t.device)


def oracle_choice(t, axis):
    x = t.detach().cpu().numpy()
    losses, cands, _ = search_losses(x, 3, axis)
    first, gap = first_min_and_gap(losses)
    return cands[first, np.arange(first.size)], gap


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("scheme", ["tf", "tf_enhanced"])
def test_quantsim_end_to_end(scheme, per_channel, tmp_path):
    from aimet_amd.quantizers import QuantizationDataType, StaticGridPerChannelQuantizer
    from aimet_amd.quantsim import QuantizationSimModel
    model, batches = make_model()
    cfg = {"defaults": {"ops": {"is_output_quantized": "True"}, "params": {"is_quantized": "True"},
                        "per_channel_quantization": str(per_channel)}}
    sim = QuantizationSimModel(model, batches[0], quant_scheme=scheme, default_output_bw=8, default_param_bw=8,
                               default_data_type=QuantizationDataType.float, config_file=cfg)

    def calibrate(m, _):
        for b in batches:
            m(b)
    sim.compute_encodings(calibrate, None)
    conv, fc = sim.model[0], sim.model[2]

    # the running value: the first batch's, then 0.9 * old + 0.1 * new, in float32 on the device
    def per_batch(t, axis=None):
        if scheme == "tf":
            mv = t.abs().amax() if axis is None else t.abs().amax(dim=[d for d in range(t.dim()) if d != axis])
            return mv.reshape(-1)
        chosen, gap = oracle_choice(t, axis)
        assert np.all(gap >= GAP)
        return torch.from_numpy(chosen).to(DEV)
    m1, m2 = per_batch(batches[0]), per_batch(batches[1])
    want_in = 0.9 * m1 + 0.1 * m2
    got_in = conv.input_quantizers[0].fp8_maxval.reshape(-1)
    np.testing.assert_array_equal(bits(got_in.cpu().numpy()), bits(want_in.cpu().numpy()))
    for w in (conv, fc):
        q = w.param_quantizers["weight"]
        assert isinstance(q, StaticGridPerChannelQuantizer) == per_channel
        want_w = per_batch(w._module_to_wrap.weight.detach(), 0 if per_channel else None)
        if scheme == "tf" and per_channel:
            want_w = 0.9 * want_w + 0.1 * want_w      # fp_quantization.py:60 sets it before update_maxval
        np.testing.assert_array_equal(bits(q.fp8_maxval.reshape(-1).cpu().numpy()), bits(want_w.cpu().numpy()))
        assert not w.param_quantizers["bias"].enabled

    # the forward: every quantizer's cast is the oracle's with the same maxvals
    x = batches[1]
    with torch.no_grad():
        got = sim.model(x)
        h = np_cast(x, conv.input_quantizers[0].fp8_maxval)
        for w in (conv, fc):
            q = w.param_quantizers["weight"]
            wq = np_cast(w._module_to_wrap.weight, q.fp8_maxval, 0)
            if w is conv:
                h = torch.nn.functional.conv2d(h, wq, w._module_to_wrap.bias, padding=1)
            else:
                h = torch.nn.functional.linear(h.flatten(1), wq, w._module_to_wrap.bias)
            h = np_cast(h, w.output_quantizers[0].fp8_maxval)
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(h.cpu().numpy()))
    assert not torch.equal(got, model(x))

    # export writes dtype float; loading the file back leaves a sim whose forward is unchanged
    path = sim.export(str(tmp_path), "fp8")
    enc = json.load(open(path))
    assert enc["quantizer_args"]["dtype"] == "float"
    assert enc["param_encodings"]["0.weight"][0] == {"bitwidth": 8, "dtype": "float"}
    assert enc["activation_encodings"]["0"]["output"]["0"] == {"bitwidth": 8, "dtype": "float"}
    assert enc["activation_encodings"]["0"]["input"]["0"] == {"bitwidth": 8, "dtype": "float"}
    sim.load_encodings(path)
    with torch.no_grad():
        assert torch.equal(sim.model(x), got)

    # a forward captured in a HIP graph replays equal (no synchronisation, nothing read back)
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        sim.model(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        static_y = sim.model(static_x)
    static_x.copy_(batches[0])
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(static_y, sim.model(batches[0]))

    # backward: the gradient passes straight through every FP8 quantizer
    q = conv.input_quantizers[0]
    xg = batches[0].clone().requires_grad_(True)
    grad = torch.randn_like(xg)
    q.quantize_dequantize(xg, q.round_mode).backward(grad)
    assert torch.equal(xg.grad, grad)


def test_sharded_calibration_refuses_fp8_statistics():
    from aimet_amd.qc_quantize_op import StatsBatch
    from aimet_amd.quantizers import QuantizationDataType, QuantScheme, StaticGridPerTensorQuantizer
    q = StaticGridPerTensorQuantizer(8, "nearest", QuantScheme.post_training_tf, False, True,
                                     data_type=QuantizationDataType.float)
    t = torch.ones(8, device=DEV)
    assert not StatsBatch.eligible(q, t) and not StatsBatch.eligible_sharded(q, t)


if __name__ == "__main__":
    # python tests/test_fp8_gpu.py <file>: the measurement behind EPS
    with open(sys.argv[1], "w") as f:
        measure_eps(f)
    print(open(sys.argv[1]).read())
