"""The streaming fp32 QDQ / STE kernels under every tile shape (64, 128 and 256 lanes per workgroup,
aimet_qdq_tile_lanes): bit-exact against the CPU oracle at the sizes where a tile ends, ends exactly
or has just ended, on the vector path (16-B aligned) and the scalar path (views offset by one
element), with guard elements around every output. Nearest rounding is checked against the C oracle
(oracle/dlq_oracle.c); stochastic rounding against the restatement below of the library's draw
(common.hpp: uniform01 over the element index, which must not depend on the tile shape).
The fp16 / bf16 I/O forms (a fixed 256 lanes of 8 elements) get the same treatment at their own tile
edges: upcast on the host, the fp32 expectation, torch's CPU downcast.
Needs an MI355X."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import bits, gpu_available
from oracle import oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _native  # noqa: E402
from aimet_amd.libpymo import TfEncoding  # noqa: E402

DEV = "cuda"
SHAPES = (64, 128, 256)
GUARD = 8                  # floats before and after every buffer (keeps the payload 16-B aligned)
SENTINEL = 12345.0
ENC = (-2.5, 4.0, 8)       # min, max, bw as given to the library (it gates them itself)
SEED = 0x5EED1234ABCD
CHANNEL_CASES = ((3, 4), (5, 8), (7, 1028), (64, 3))


def sizes(L):
    return (1, 3, 4, 5, 4 * L - 1, 4 * L, 4 * L + 1, 8 * L + 7, 4 * L * 1000 + 2)


@pytest.fixture(params=SHAPES, ids=["lanes%d" % L for L in SHAPES])
def lanes(request):
    prev = ctypes.c_int()
    _native.call("aimet_qdq_tile_lanes", request.param, ctypes.byref(prev))
    yield request.param
    _native.call("aimet_qdq_tile_lanes", prev.value, None)


def stream():
    return torch.cuda.current_stream().cuda_stream


def enc_c():
    e = TfEncoding()
    e.min, e.max, e.bw = ENC
    return e.to_c()


@functools.lru_cache(maxsize=None)
def filled():
    """(min, max, delta, offset) of ENC as the kernels see them (fillEncodingInfo, then fp32)."""
    e = O.fill_encoding_info(ENC[2], ENC[0], ENC[1])
    return tuple(np.float32(v) for v in e.as_tuple()[:4])


def specials():
    mn, mx, delta, _ = filled()
    return np.array([mn, mx, np.nextafter(mn, np.float32(-9)), np.nextafter(mx, np.float32(9)), -100.0, 100.0,
                     0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, np.nan, mn + delta * np.float32(0.5),
                     delta * np.float32(2.5)], np.float32)


@functools.lru_cache(maxsize=None)
def base(seed=0):
    """One seeded host array that every case slices: N(0, 3) with the special values at its start
    and strewn through it (every 1021st element onwards)."""
    n = 4 * 256 * 1000 + 2 + 1
    x = (np.random.default_rng(seed).standard_normal(n) * 3.0).astype(np.float32)
    s = specials()
    x[:s.size] = s
    k = np.arange(s.size + 7, n, 1021)
    x[k] = s[np.arange(k.size) % s.size]
    x.setflags(write=False)
    return x


def guarded_dev(payload, off, dtype=torch.float32):
    """A device buffer [guard | off | payload | guard] filled with SENTINEL; returns (buffer, view).
    payload: a float32 host array, a host tensor of `dtype`, or an element count."""
    host = None
    if not isinstance(payload, int):
        host = payload if torch.is_tensor(payload) else torch.from_numpy(np.array(payload, np.float32))
        assert host.dtype == dtype
    n = payload if host is None else host.numel()
    buf = torch.full((2 * GUARD + off + n,), SENTINEL, dtype=dtype, device=DEV)
    view = buf[GUARD + off:GUARD + off + n]
    if host is not None:
        view.copy_(host)
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return buf, view


def check_guards(buf, off, n, what):
    h = buf.cpu().float().numpy()
    sentinel = torch.tensor(SENTINEL, dtype=buf.dtype).float().item()   # SENTINEL as the buffer's dtype holds it
    assert np.all(h[:GUARD + off] == sentinel) and np.all(h[GUARD + off + n:] == sentinel), \
        "%s: wrote outside its output" % what


# ---- the library's stochastic rounding restated on the host ------------------------------------
def uniform01(seed, idx):
    idx = np.asarray(idx, np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def stochastic_codes(x, mn, mx, delta, offset, seed, idx):
    """floor((clamp(x) / delta - offset) + U[0, 1)) in fp32, clamp as glibc fminf / fmaxf."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        o = np.where((x < mx) | np.isnan(mx), x, mx).astype(np.float32)
        o = np.where((o > mn) | np.isnan(mn), o, mn).astype(np.float32)
        o = (o / delta).astype(np.float32) - offset
        return np.floor(o.astype(np.float32) + uniform01(seed, idx)).astype(np.float32)


def stochastic_qdq(x, mn, mx, delta, offset, seed, idx):
    q = stochastic_codes(x, mn, mx, delta, offset, seed, idx)
    with np.errstate(all="ignore"):
        return (delta * (q + offset).astype(np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def want_per_tensor(n, off, op, rm):
    x = base()[off:off + n]
    if rm == 0:
        if op == "qdq":
            return O.qdq_per_tensor(x, *ENC)
        return O.quantize_per_tensor(x, *ENC, True)
    mn, mx, delta, offset = filled()
    idx = np.arange(n, dtype=np.uint64)
    if op == "qdq":
        return stochastic_qdq(x, mn, mx, delta, offset, SEED, idx)
    return stochastic_codes(x, mn, mx, delta, offset, SEED, idx) - np.float32(2 ** (ENC[2] - 1))


# ---- per-tensor QDQ and quantize-only --------------------------------------------------------
@pytest.mark.parametrize("rm", [0, 1], ids=["nearest", "stochastic"])
@pytest.mark.parametrize("op", ["qdq", "quantize"])
def test_per_tensor(lanes, op, rm):
    for n in sizes(lanes):
        for off in (0, 1):   # 16-B aligned (vector kernel + scalar tail) / offset by one element (scalar)
            _, x = guarded_dev(base()[off:off + n], off)
            obuf, y = guarded_dev(n, off)
            if op == "qdq":
                _native.call("aimet_qdq_per_tensor", x.data_ptr(), y.data_ptr(), n, enc_c(), rm, SEED, stream())
            else:
                _native.call("aimet_quantize_per_tensor", x.data_ptr(), y.data_ptr(), n, enc_c(), rm, 1, SEED,
                             stream())
            what = "lanes %d n %d offset %d" % (lanes, n, off)
            np.testing.assert_array_equal(bits(y.cpu().numpy()), bits(want_per_tensor(n, off, op, rm)), err_msg=what)
            check_guards(obuf, off, n, what)


# ---- per-channel ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def channel_case(C, K, outer):
    """(x [outer*C*K], table [4][C]) with values at and beyond every channel's clamps."""
    rng = np.random.default_rng(1000 * C + K)
    encs = []
    for c in range(C):
        lo, hi = -0.5 - 0.1 * (c % 5), 0.4 + 0.07 * (c % 7)
        e = O.fill_encoding_info(8, lo, hi)
        encs.append(e.as_tuple())
    table = O.per_channel_table(encs)
    x = rng.standard_normal((outer, C, K)).astype(np.float32)
    s = specials()
    flat = x.reshape(-1)
    k = np.arange(0, flat.size, 3)[:4 * s.size]
    flat[k] = s[np.arange(k.size) % s.size]
    x[:, :, 0] = table[0][None, :]          # each channel's own min and (K > 1) max
    if K > 1:
        x[:, :, K - 1] = table[1][None, :]
    flat.setflags(write=False)
    table.setflags(write=False)
    return flat, table


def want_per_channel(flat, table, C, K, outer, rm, seed=SEED, idx0=0):
    if rm == 0:
        xs = flat.reshape(outer, C * K)
        return np.concatenate([O.qdq_per_channel(xs[o], C, K, table) for o in range(outer)])
    ch = (np.arange(flat.size) // K) % C
    idx = np.arange(flat.size, dtype=np.uint64) + np.uint64(idx0)
    return stochastic_qdq(flat, table[0][ch], table[1][ch], table[2][ch], table[3][ch], seed, idx)


@pytest.mark.parametrize("rm", [0, 1], ids=["nearest", "stochastic"])
@pytest.mark.parametrize("outer", [1, 2])
@pytest.mark.parametrize("C,K", CHANNEL_CASES)
def test_per_channel(lanes, C, K, outer, rm):
    flat, table = channel_case(C, K, outer)
    n = flat.size
    _, x = guarded_dev(flat, 0)
    obuf, y = guarded_dev(n, 0)
    t = torch.from_numpy(np.array(table)).to(DEV)
    _native.call("aimet_qdq_per_channel", x.data_ptr(), y.data_ptr(), outer, C, K, t.data_ptr(), rm, SEED, stream())
    np.testing.assert_array_equal(bits(y.cpu().numpy()), bits(want_per_channel(flat, table, C, K, outer, rm)))
    check_guards(obuf, 0, n, "per-channel %s" % ((C, K, outer),))


# ---- batched plan -----------------------------------------------------------------------------
PLAN_TENSORS = ((1, 4), (1, 256), (2, 130), (3, 172), (5, 3))   # the last takes the scalar path


@pytest.mark.parametrize("rm", [0, 1], ids=["nearest", "stochastic"])
def test_batched_plan(lanes, rm):
    """Tensor boundaries inside, at the end of and just past a workgroup. The plan keeps the shape
    it was created with: it is run after the process-wide shape has been changed."""
    from aimet_amd.tensor_quantizer import ChannelQdqPlan
    entries, cases = [], []
    for C, K in PLAN_TENSORS:
        flat, table = channel_case(C, K, 1)
        _, x = guarded_dev(flat, 0)
        obuf, y = guarded_dev(flat.size, 0)
        t = torch.from_numpy(np.array(table)).to(DEV)
        entries.append((x.view(C, K), y.view(C, K), 0, t))
        cases.append((C, K, flat, table, x, obuf, y, t))
    plan = ChannelQdqPlan(entries)
    _native.call("aimet_qdq_tile_lanes", 64 if lanes != 64 else 256, None)   # the fixture restores it
    _native.call("aimet_qdq_channel_plan_run", plan._handle, rm, SEED, stream())
    for i, (C, K, flat, table, x, obuf, y, t) in enumerate(cases):
        got = bits(y.cpu().numpy())
        if rm == 0:   # equal to the per-tensor launch (and with it to the oracle)
            single = torch.empty(flat.size, dtype=torch.float32, device=DEV)
            _native.call("aimet_qdq_per_channel", x.data_ptr(), single.data_ptr(), 1, C, K, t.data_ptr(), 0, 0,
                         stream())
            np.testing.assert_array_equal(got, bits(single.cpu().numpy()), err_msg="tensor %d" % i)
        # the plan draws over (tensor index << 40) + element index
        want = want_per_channel(flat, table, C, K, 1, rm, idx0=i << 40)
        np.testing.assert_array_equal(got, bits(want), err_msg="tensor %d" % i)
        check_guards(obuf, 0, flat.size, "plan tensor %d" % i)
    del plan


# ---- STE backward -------------------------------------------------------------------------
def ste_want(x, g, mn, mx):
    """grad * (min <= x <= max), as torch computes it on the CPU."""
    x, g = torch.from_numpy(np.array(x)), torch.from_numpy(np.array(g))
    mn, mx = torch.as_tensor(mn), torch.as_tensor(mx)
    inside = (mn <= x) & (x <= mx)
    return torch.where(inside, g * 1.0, g * 0.0).numpy()


def test_ste_per_tensor(lanes):
    mn, mx = np.float32(-2.5), np.float32(4.0)
    for n in sizes(lanes):
        for off in (0, 1):
            xh, gh = base()[off:off + n], base(1)[off:off + n]
            _, x = guarded_dev(xh, off)
            _, g = guarded_dev(gh, off)
            obuf, gi = guarded_dev(n, off)
            _native.call("aimet_ste_backward_per_tensor", x.data_ptr(), g.data_ptr(), gi.data_ptr(), n, float(mn),
                         float(mx), stream())
            what = "lanes %d n %d offset %d" % (lanes, n, off)
            np.testing.assert_array_equal(bits(gi.cpu().numpy()), bits(ste_want(xh, gh, mn, mx)), err_msg=what)
            check_guards(obuf, off, n, what)


@pytest.mark.parametrize("outer", [1, 2])
@pytest.mark.parametrize("C,K", CHANNEL_CASES)
def test_ste_per_channel(lanes, C, K, outer):
    flat, table = channel_case(C, K, outer)
    n = flat.size
    gh = base(1)[:n]
    _, x = guarded_dev(flat, 0)
    _, g = guarded_dev(gh, 0)
    obuf, gi = guarded_dev(n, 0)
    mins = torch.from_numpy(np.array(table[0])).to(DEV)
    maxs = torch.from_numpy(np.array(table[1])).to(DEV)
    _native.call("aimet_ste_backward", x.data_ptr(), g.data_ptr(), gi.data_ptr(), outer, C, K, mins.data_ptr(),
                 maxs.data_ptr(), stream())
    ch = (np.arange(n) // K) % C
    np.testing.assert_array_equal(bits(gi.cpu().numpy()), bits(ste_want(flat, gh, table[0][ch], table[1][ch])))
    check_guards(obuf, 0, n, "STE per-channel %s" % ((C, K, outer),))


# ---- fp16 / bf16 I/O (qdq16.hip: 8 elements per vector, a fixed 256 lanes) ----------------------
# Expected values come from outside the library: the 16-bit input upcast on the host (exact), the
# fp32 expectation of the sections above, and torch's CPU downcast.
DTYPES16 = (torch.float16, torch.bfloat16)
IDS16 = ["fp16", "bf16"]
SIZES16 = (1, 7, 8, 9, 8 * 256 - 1, 8 * 256, 8 * 256 + 1, 16 * 256 + 7)
CHANNEL_CASES16 = ((3, 4, 2), (3, 8, 1), (5, 16, 2), (7, 1032, 1), (64, 3, 1))   # K % 8 != 0: the scalar kernel


def io_code(dtype):
    from aimet_amd.tensor_quantizer import IO_DTYPES
    return IO_DTYPES[dtype]


def bits16(t):
    """Bit patterns of a 16-bit tensor, NaNs compared as NaN-ness (as conftest.bits does)."""
    t = t.detach().cpu().contiguous()
    b = t.view(torch.int16).numpy().view(np.uint16).copy()
    b[torch.isnan(t).numpy()] = 0x7FFF
    return b


def down(a, dtype):
    return torch.from_numpy(np.array(a, np.float32)).to(dtype)


def host16(a, dtype):
    """(the 16-bit host tensor of a float32 array, its exact float32 upcast)."""
    t = down(a, dtype)
    up = t.float().numpy()
    up.setflags(write=False)
    return t, up


@pytest.mark.parametrize("rm", [0, 1], ids=["nearest", "stochastic"])
@pytest.mark.parametrize("dtype", DTYPES16, ids=IDS16)
def test_per_tensor_16(dtype, rm):
    mn, mx, delta, offset = filled()
    for n in SIZES16:
        for off in (0, 1):   # 16-B aligned (vector kernel + scalar tail) / offset by 2 bytes (scalar)
            x16, xf = host16(base()[off:off + n], dtype)
            if rm == 0:
                want = O.qdq_per_tensor(xf, *ENC)
            else:
                want = stochastic_qdq(xf, mn, mx, delta, offset, SEED, np.arange(n, dtype=np.uint64))
            _, x = guarded_dev(x16, off, dtype)
            obuf, y = guarded_dev(n, off, dtype)
            _native.call("aimet_qdq_per_tensor_16", x.data_ptr(), y.data_ptr(), n, io_code(dtype), enc_c(), rm, SEED,
                         stream())
            what = "n %d offset %d" % (n, off)
            np.testing.assert_array_equal(bits16(y), bits16(down(want, dtype)), err_msg=what)
            check_guards(obuf, off, n, what)


@pytest.mark.parametrize("rm", [0, 1], ids=["nearest", "stochastic"])
@pytest.mark.parametrize("C,K,outer", CHANNEL_CASES16)
@pytest.mark.parametrize("dtype", DTYPES16, ids=IDS16)
def test_per_channel_16(dtype, C, K, outer, rm):
    flat, table = channel_case(C, K, outer)
    n = flat.size
    x16, xf = host16(flat, dtype)
    want = bits16(down(want_per_channel(xf, table, C, K, outer, rm), dtype))
    t = torch.from_numpy(np.array(table)).to(DEV)
    for off in (0, 1):
        _, x = guarded_dev(x16, off, dtype)
        obuf, y = guarded_dev(n, off, dtype)
        _native.call("aimet_qdq_per_channel_16", x.data_ptr(), y.data_ptr(), outer, C, K, io_code(dtype),
                     t.data_ptr(), rm, SEED, stream())
        what = "per-channel %s offset %d" % ((C, K, outer), off)
        np.testing.assert_array_equal(bits16(y), want, err_msg=what)
        check_guards(obuf, off, n, what)


def ste_want_16(xf, gf, mn, mx, dtype):
    """grad * (min <= float(x) <= max) on the upcast operands, downcast by torch on the CPU."""
    with np.errstate(invalid="ignore"):
        return down(gf * ((mn <= xf) & (xf <= mx)).astype(np.float32), dtype)


@pytest.mark.parametrize("dtype", DTYPES16, ids=IDS16)
def test_ste_per_tensor_16(dtype):
    mn, mx = np.float32(-2.5), np.float32(4.0)
    for n in SIZES16:
        for off in (0, 1):
            x16, xf = host16(base()[off:off + n], dtype)
            g16, gf = host16(base(1)[off:off + n], dtype)
            _, x = guarded_dev(x16, off, dtype)
            _, g = guarded_dev(g16, off, dtype)
            obuf, gi = guarded_dev(n, off, dtype)
            _native.call("aimet_ste_backward_16", x.data_ptr(), g.data_ptr(), gi.data_ptr(), 1, 1, n, io_code(dtype),
                         None, None, float(mn), float(mx), stream())
            what = "n %d offset %d" % (n, off)
            np.testing.assert_array_equal(bits16(gi), bits16(ste_want_16(xf, gf, mn, mx, dtype)), err_msg=what)
            check_guards(obuf, off, n, what)


@pytest.mark.parametrize("C,K,outer", CHANNEL_CASES16)
@pytest.mark.parametrize("dtype", DTYPES16, ids=IDS16)
def test_ste_per_channel_16(dtype, C, K, outer):
    flat, table = channel_case(C, K, outer)
    n = flat.size
    x16, xf = host16(flat, dtype)
    g16, gf = host16(base(1)[:n], dtype)
    ch = (np.arange(n) // K) % C
    want = bits16(ste_want_16(xf, gf, table[0][ch], table[1][ch], dtype))
    mins = torch.from_numpy(np.array(table[0])).to(DEV)
    maxs = torch.from_numpy(np.array(table[1])).to(DEV)
    for off in (0, 1):
        _, x = guarded_dev(x16, off, dtype)
        _, g = guarded_dev(g16, off, dtype)
        obuf, gi = guarded_dev(n, off, dtype)
        _native.call("aimet_ste_backward_16", x.data_ptr(), g.data_ptr(), gi.data_ptr(), outer, C, K, io_code(dtype),
                     mins.data_ptr(), maxs.data_ptr(), 0.0, 0.0, stream())
        what = "STE per-channel %s offset %d" % ((C, K, outer), off)
        np.testing.assert_array_equal(bits16(gi), want, err_msg=what)
        check_guards(obuf, off, n, what)


# ---- the kernels of the same form in other files -------------------------------------------------
def test_fp16_round_trip(lanes):
    """aimet_qdq_fp16 (the Fp16RoundTrip op: vector kernel + scalar tail): float -> half -> float, as
    the oracle."""
    for n in sizes(lanes):
        for off in (0, 1):
            xh = base()[off:off + n]
            _, x = guarded_dev(xh, off)
            obuf, y = guarded_dev(n, off)
            _native.call("aimet_qdq_fp16", x.data_ptr(), y.data_ptr(), n, stream())
            what = "lanes %d n %d offset %d" % (lanes, n, off)
            np.testing.assert_array_equal(bits(y.cpu().numpy()), bits(O.qdq_fp16(xh)), err_msg=what)
            check_guards(obuf, off, n, what)


@pytest.mark.parametrize("outer", [1, 2])
@pytest.mark.parametrize("C,K", CHANNEL_CASES + ((1, 8 * 256 + 7), (1, 4 * 256 * 3)))
def test_learned_grid_forward_same_under_every_shape(lanes, C, K, outer):
    """aimet_lg_forward (lg_fwd_kernel, two quads per lane LANES apart, and its scalar form) gives
    the bits of its 256-lane form, which tests/test_gpu_parity.py holds against the reference."""
    flat, table = channel_case(C, K, outer)
    n = flat.size
    _, x = guarded_dev(flat, 0)
    delta = torch.from_numpy(np.array(table[2])).to(DEV)
    offset = torch.from_numpy(np.array(table[3])).to(DEV)

    def run():
        obuf, y = guarded_dev(n, 0)
        _native.call("aimet_lg_forward", x.data_ptr(), y.data_ptr(), outer, C, K, delta.data_ptr(),
                     offset.data_ptr(), ctypes.c_float(255.0), stream())
        check_guards(obuf, 0, n, "lg forward %s lanes %d" % ((C, K, outer), lanes))
        return bits(y.cpu().numpy())

    got = run()
    _native.call("aimet_qdq_tile_lanes", 256, None)   # the fixture restores the shape
    np.testing.assert_array_equal(got, run())
