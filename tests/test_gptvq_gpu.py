"""GPTVQ on the GPU (aimet_amd/csrc/gptvq.hip, aimet_amd/gptvq.py).

1. aimet_gptvq_block_update bit for bit against the numpy oracle (tests/gptvq_oracle.py): w, err and
   indices, nothing written outside the block or the buffers, under both lane layouts.
2. aimet_gptvq_kmeans step by step: from the kernel's own state after t - 1 iterations the oracle
   computes the assignments bit-exactly and the means in float64; the state after t iterations agrees
   within the bound of fp32 summation. Bitwise repeatable, guards intact.
3. apply_gptvq end to end on two tiny models: structure of the result, the exported encodings,
   block-level grouping, and agreement with a float64 restatement of the reference algorithm.
Needs an MI355X."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch
from torch import nn

import gptvq_oracle as GO
from conftest import bits, gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _native, gptvq  # noqa: E402
from aimet_amd.gptvq import GPTVQ, GPTVQOptimizer, GPTVQParameters  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

DEV = "cuda"
GUARD = 8                  # elements before and after every buffer (keeps the payload 16-B aligned)
SENTINEL = 12345.0


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded_dev(payload, off=0, dtype=torch.float32):
    """A device buffer [guard | off | payload | guard] filled with SENTINEL; returns (buffer, view).
    `payload` is a host array, or an element count for an output."""
    n = payload if isinstance(payload, int) else payload.size
    buf = torch.full((2 * GUARD + off + n,), SENTINEL, dtype=dtype, device=DEV)
    view = buf[GUARD + off:GUARD + off + n]
    if not isinstance(payload, int):
        view.copy_(torch.from_numpy(np.array(payload).ravel()))
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return buf, view


def check_guards(buf, off, n, what):
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD + off] == SENTINEL) and np.all(h[GUARD + off + n:] == SENTINEL), \
        "%s: wrote outside its buffer" % what


def make_hinv(cols, seed):
    """The upper Cholesky factor of a random SPD matrix: positive diagonal."""
    a = np.random.default_rng(seed).standard_normal((cols, cols))
    return np.ascontiguousarray(np.linalg.cholesky(a @ a.T / cols + np.eye(cols)).T).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# 1. block update
# ------------------------------------------------------------------------------------------------
# name -> (rows, rows_per_block, cols, b0, block length, D, K, duplicate centroids)
UPDATE_CASES = {
    "one-row": (1, 1, 16, 0, 16, 2, 4, False),
    "rows3-rpb3": (3, 3, 24, 0, 24, 2, 8, False),
    "two-groups": (8, 4, 32, 0, 32, 2, 8, False),
    "length-is-D": (5, 5, 8, 2, 4, 4, 4, False),
    "128-D1": (6, 3, 128, 0, 128, 1, 16, False),
    "128-D2": (6, 3, 128, 0, 128, 2, 16, False),
    "128-D4": (6, 3, 128, 0, 128, 4, 16, False),
    "128-D8": (6, 3, 128, 0, 128, 8, 16, False),
    "K1": (4, 2, 64, 0, 64, 2, 1, False),
    "K64": (70, 35, 128, 0, 128, 2, 64, False),
    "K80": (9, 3, 66, 0, 66, 2, 80, False),
    "odd-b0": (7, 7, 200, 37, 128, 2, 16, False),
    "short-odd-b0": (7, 7, 120, 37, 70, 2, 16, False),
    "duplicates": (12, 4, 96, 0, 96, 2, 8, True),
}


@functools.lru_cache(maxsize=None)
def update_inputs(name):
    rows, rpb, cols, b0, length, D, K, dup = UPDATE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    w = rng.standard_normal((rows, cols)).astype(np.float32)
    G = rows // rpb
    # centroids: vectors of the weight itself (exact hits, zero distances) and random ones
    cb = rng.standard_normal((G, K, D)).astype(np.float32)
    for g in range(G):
        cb[g, 0] = w[g * rpb, b0:b0 + D]
    if dup:
        cb[:, 5] = cb[:, 2]
        cb[:, 3] = cb[:, 0]
    hinv = make_hinv(cols, rows * 1000 + cols)
    for a in (w, cb, hinv):
        a.setflags(write=False)
    return w, cb, hinv


@functools.lru_cache(maxsize=None)
def update_want(name):
    rows, rpb, cols, b0, length, D, K, _ = UPDATE_CASES[name]
    w, cb, hinv = update_inputs(name)
    w = w.copy()
    err = np.full((rows, length), SENTINEL, np.float32)
    idx = np.full((rows, length // D), -7, np.int32)
    GO.block_update(w, rpb, b0, 0, length, b0 + length, D, cb, hinv, err, idx)
    for a in (w, err, idx):
        a.setflags(write=False)
    return w, err, idx


def run_update(name, splits=None, off=0):
    """The kernel on guarded buffers, over the step ranges `splits` (default: one call for the block)."""
    rows, rpb, cols, b0, length, D, K, _ = UPDATE_CASES[name]
    w, cb, hinv = update_inputs(name)
    wbuf, dw = guarded_dev(w, off)
    _, dcb = guarded_dev(cb)
    _, dh = guarded_dev(hinv)
    ebuf, derr = guarded_dev(rows * length)
    ibuf, didx = guarded_dev(rows * (length // D), dtype=torch.int32)
    for s0, s1 in splits or ((0, length),):
        _native.call("aimet_gptvq_block_update", dw.data_ptr(), cols, rows, rpb, b0, s0, s1, b0 + length, D, K,
                     dcb.data_ptr(), dh.data_ptr(), cols, derr.data_ptr(), didx.data_ptr(), stream())
    torch.cuda.synchronize()
    check_guards(wbuf, off, rows * cols, name + " w")
    check_guards(ebuf, 0, rows * length, name + " err")
    check_guards(ibuf, 0, rows * (length // D), name + " indices")
    return (dw.cpu().numpy().reshape(rows, cols), derr.cpu().numpy().reshape(rows, length),
            didx.cpu().numpy().reshape(rows, length // D))


def assert_update(name, got):
    rows, rpb, cols, b0, length, D, K, _ = UPDATE_CASES[name]
    w0 = update_inputs(name)[0]
    want_w, want_err, want_idx = update_want(name)
    w, err, idx = got
    assert np.array_equal(idx, want_idx), (name, np.argwhere(idx != want_idx)[:4].tolist())
    assert np.array_equal(bits(err), bits(want_err)), (name, np.argwhere(bits(err) != bits(want_err))[:4].tolist())
    assert np.array_equal(bits(w), bits(want_w)), (name, np.argwhere(bits(w) != bits(want_w))[:4].tolist())
    outside = np.ones(cols, bool)
    outside[b0:b0 + length] = False
    assert np.array_equal(bits(w[:, outside]), bits(w0[:, outside])), "columns outside the block changed"


@pytest.mark.parametrize("layout", [1, 2], ids=["wave-per-row", "lane-per-row"])
@pytest.mark.parametrize("name", list(UPDATE_CASES))
def test_block_update_bit_exact(name, layout):
    prev = ctypes.c_int(0)
    _native.call("aimet_gptvq_update_layout", layout, ctypes.byref(prev))
    try:
        for off in (0, 1):   # the weight 16-B aligned / offset by one float
            assert_update(name, run_update(name, off=off))
    finally:
        _native.call("aimet_gptvq_update_layout", prev.value, None)
    if UPDATE_CASES[name][7]:
        assert not np.any(np.isin(update_want(name)[2], (3, 5))), "a duplicate never wins over its first copy"


def test_block_update_split_calls_equal_one_call():
    name = "128-D2"
    one = run_update(name)
    two = run_update(name, splits=((0, 64), (64, 128)))
    for a, b in zip(one, two):
        assert np.array_equal(bits(a), bits(b))
    assert_update(name, two)
    # a split that is no multiple of 64, and an empty range
    assert_update(name, run_update(name, splits=((0, 22), (22, 22), (22, 128))))
    # steps that were not run leave err and indices alone
    w, err, idx = run_update(name, splits=((0, 64),))
    assert np.all(err[:, 64:] == SENTINEL) and np.all(idx[:, 32:] == int(SENTINEL))
    assert np.array_equal(bits(err[:, :64]), bits(update_want(name)[1][:, :64]))


def test_block_update_rejects_bad_arguments():
    name = "two-groups"
    rows, rpb, cols, b0, length, D, K, _ = UPDATE_CASES[name]
    w, cb, hinv = update_inputs(name)
    wbuf, dw = guarded_dev(w)
    _, dcb = guarded_dev(cb)
    _, dh = guarded_dev(hinv)
    _, derr = guarded_dev(rows * length)
    _, didx = guarded_dev(rows * (length // D), dtype=torch.int32)
    for change in (dict(rpb=3), dict(s1=31), dict(end=34), dict(s0=8, s1=4), dict(K=2000), dict(D=0)):
        a = dict(rpb=rpb, s0=0, s1=length, end=b0 + length, D=D, K=K)
        a.update(change)
        with pytest.raises(ValueError):
            _native.call("aimet_gptvq_block_update", dw.data_ptr(), cols, rows, a["rpb"], b0, a["s0"], a["s1"],
                         a["end"], a["D"], a["K"], dcb.data_ptr(), dh.data_ptr(), cols, derr.data_ptr(),
                         didx.data_ptr(), stream())
    with pytest.raises(ValueError, match="device memory"):
        _native.call("aimet_gptvq_block_update", w.ctypes.data, cols, rows, rpb, b0, 0, length, b0 + length, D, K,
                     dcb.data_ptr(), dh.data_ptr(), cols, derr.data_ptr(), didx.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(bits(dw.cpu().numpy()), bits(w.ravel()))
    check_guards(wbuf, 0, rows * cols, "rejected calls")


# ------------------------------------------------------------------------------------------------
# 2. k-means
# ------------------------------------------------------------------------------------------------
# name -> (G, rows_per_block, ncols, D, K, ld, column offset)
KMEANS_CASES = {
    "one-vector": (1, 1, 2, 2, 4, 2, 0),
    "K-above-N": (2, 2, 4, 2, 16, 4, 0),
    "D1": (2, 4, 24, 1, 8, 24, 0),
    "D2-rpb3-ncols6": (2, 3, 6, 2, 4, 6, 0),
    "D4": (2, 4, 32, 4, 8, 32, 0),
    "D8": (2, 4, 32, 8, 4, 32, 0),
    "G3": (3, 5, 20, 2, 8, 20, 0),
    "odd-offset": (2, 4, 16, 2, 8, 37, 5),
    "K1": (2, 4, 16, 2, 1, 16, 0),
    "K1024": (1, 16, 256, 2, 1024, 256, 0),
    "default-tile": (2, 32, 256, 2, 64, 256, 0),
    "above-64KiB": (1, 32, 512, 2, 64, 512, 0),
    "beyond-LDS": (2, 64, 1024, 2, 64, 1024, 0),
}
KMEANS_STEPS = (1, 2, 3, 100)


@functools.lru_cache(maxsize=None)
def kmeans_inputs(name):
    G, rpb, ncols, D, K, ld, c0 = KMEANS_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    w = rng.standard_normal((G * rpb, ld)).astype(np.float32)
    x = GO.group_vectors(w[:, c0:c0 + ncols], rpb, D)
    start = np.stack([x[g][rng.integers(0, x.shape[1], K)] for g in range(G)]) + \
        (rng.standard_normal((G, K, D)) * 0.01).astype(np.float32)
    start = start.astype(np.float32)
    for a in (w, x, start):
        a.setflags(write=False)
    return w, x, start


def run_kmeans(name, iterations):
    G, rpb, ncols, D, K, ld, c0 = KMEANS_CASES[name]
    w, _, start = kmeans_inputs(name)
    wbuf, dw = guarded_dev(w)
    cbuf, dcb = guarded_dev(start)
    _native.call("aimet_gptvq_kmeans", dw.data_ptr() + 4 * c0, ld, G, rpb, ncols, D, K, iterations, dcb.data_ptr(),
                 stream())
    torch.cuda.synchronize()
    check_guards(cbuf, 0, G * K * D, name + " codebook")
    check_guards(wbuf, 0, w.size, name + " w")
    assert np.array_equal(bits(dw.cpu().numpy()), bits(w.ravel())), "the weight is read only"
    return dcb.cpu().numpy().reshape(G, K, D)


@pytest.mark.parametrize("name", list(KMEANS_CASES))
def test_kmeans_step_by_step(name):
    G, rpb, ncols, D, K, ld, c0 = KMEANS_CASES[name]
    _, x, start = kmeans_inputs(name)
    assert np.array_equal(bits(run_kmeans(name, 0)), bits(start)), "no iteration: the input"
    u = 2.0 ** -24
    for t in KMEANS_STEPS:
        before = run_kmeans(name, t - 1) if t > 1 else start
        after = run_kmeans(name, t)
        want, _, counts, mags = GO.kmeans_step(x, before)
        # a cluster's sum has count terms: count - 1 rounded additions in whatever order (adding an
        # empty slice's zero is exact), then the reciprocal and the product, one rounding each:
        # |got - want| <= gamma(count + 1) * sum |x| / count, gamma(n) = n u / (1 - n u)
        n_round = (counts[..., None] + 1) * u
        bound = n_round / (1 - n_round) * mags / np.maximum(counts, 1)[..., None] + 2.0 ** -149
        diff = np.abs(after.astype(np.float64) - want)
        print("kmeans", name, "t", t, "max |diff| / bound %.3g" % float(np.max(diff / bound)),
              "empty clusters", int(np.sum(counts == 0)))
        assert np.all(diff <= bound), (name, t, np.argwhere(diff > bound)[:4].tolist())
        assert np.all(after[counts == 0] == 0.0), "an empty cluster becomes the zero vector"
        assert np.array_equal(bits(after), bits(run_kmeans(name, t))), "two runs must give the same bits"
    if name == "K1":
        mean = x.astype(np.float64).mean(1, keepdims=True)
        assert np.allclose(run_kmeans(name, 1), mean, rtol=1e-5, atol=1e-7)


def test_kmeans_rejects_bad_arguments():
    name = "D2-rpb3-ncols6"
    G, rpb, ncols, D, K, ld, c0 = KMEANS_CASES[name]
    w, _, start = kmeans_inputs(name)
    _, dw = guarded_dev(w)
    cbuf, dcb = guarded_dev(start)
    for change in (dict(ncols=5), dict(D=4), dict(K=0), dict(K=1025), dict(it=-1), dict(ld=4), dict(G=0)):
        a = dict(G=G, ncols=ncols, D=D, K=K, it=1, ld=ld)
        a.update(change)
        with pytest.raises(ValueError):
            _native.call("aimet_gptvq_kmeans", dw.data_ptr(), a["ld"], a["G"], rpb, a["ncols"], a["D"], a["K"], a["it"],
                         dcb.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(bits(dcb.cpu().numpy()), bits(start.ravel()))
    check_guards(cbuf, 0, start.size, "rejected calls")


def test_generate_codebook_and_codebook_qdq():
    """generate_codebook = hacky_mahalanobis_init + the kernel; quantize_dequantize_codebook puts group g's
    centroids on group g's grid."""
    G, rpb, ncols, D, K, ld, c0 = KMEANS_CASES["G3"]
    w, x, _ = kmeans_inputs("G3")
    dx = torch.from_numpy(np.array(x)).to(DEV)
    got = gptvq.generate_codebook(dx, K, kmeans_iteration=3)
    init = gptvq.hacky_mahalanobis_init(dx, K).contiguous()
    want = init.clone()
    gptvq._kmeans(torch.from_numpy(np.array(w)).to(DEV), c0, ncols, rpb, D, want, 3)
    assert torch.equal(got, want) and not torch.equal(got, init)
    sim = QuantizationSimModel(nn.Sequential(nn.Linear(4, 4)).to(DEV), quant_scheme="tf", default_param_bw=4)
    gq = GPTVQOptimizer._group_quantizer(sim.model[0].param_quantizers["weight"], G)
    gq.update_encoding_stats(dx.reshape(G, -1))
    gq.compute_encoding()
    q = gptvq.quantize_dequantize_codebook(got, gq, G)
    assert q.shape == got.shape
    for g in range(G):
        e = gq.encoding[g]
        codes = q[g].double() / e.delta
        assert torch.all((codes - codes.round()).abs() < 1e-3) and len(torch.unique(q[g])) <= 2 ** 4


# ------------------------------------------------------------------------------------------------
# 3. end to end
# ------------------------------------------------------------------------------------------------
# The yardstick below restates the reference algorithm (Hessian, damping, Cholesky, k-means, sweep,
# the grid of the group table) in float64; run in float32 it is the plain fp32 loop. Every assignment
# decision has a relative gap (runner-up - best) / runner-up between its two smallest distances (the
# best one can be exactly zero, so the runner-up is the scale).
# EPS: the largest deviation, over every decision of the cases below, of the fp32 loop's best and
# runner-up distances from the float64 ones, relative to the float64 runner-up, measured on an MI355X
# with measure_eps() (profiles/r10/gptvq_eps.txt): 1.53e-6 (the 320-column layer; 3.6e-7 .. 7.1e-7 for the
# tiny models), rounded up. The smallest gaps there: 1.57e-2 (three Linears), 5.13e-2 (Conv2d), 1.66e-3
# (320 columns). A decision can only flip when the two deviations
# add up to the gap, i.e. below a relative gap of 2 * EPS; GAP = 4 * EPS is the margin
# test_seq_mse_gpu.py uses. The seeds were chosen on the CPU (yardstick_min_gap()) so that the
# smallest gap of every module is at least 100 times the guard of the seq-mse tests (5.2e-4); no
# module is skipped.
EPS = 1.6e-6
GAP = 4 * EPS
MIN_GAP_WANTED = 100 * 4 * 1.3e-6
E2E = {
    # name -> (seed, symmetric, parameters)
    "linears": (4, True, dict(rows_per_block=4, cols_per_block=8, vector_dim=2, index_bw=2,
                              num_of_kmeans_iterations=10, vector_bw=8)),
    "conv": (1, False, dict(rows_per_block=4, cols_per_block=8, vector_dim=2, index_bw=2,
                            num_of_kmeans_iterations=10, vector_bw=8)),
    # 320 columns: three 128-column blocks (the cross-block update), and cols_per_block = 96 puts codebook
    # boundaries inside the blocks (the sweep is split there); D = 4
    "wide": (7, True, dict(rows_per_block=4, cols_per_block=96, vector_dim=4, index_bw=3,
                           num_of_kmeans_iterations=2, vector_bw=8)),
}


class ThreeLinears(nn.Module):
    def __init__(self):
        super().__init__()
        self.linear1 = nn.Linear(16, 8)
        self.linear2 = nn.Linear(8, 8)
        self.linear3 = nn.Linear(8, 4)
        self.relu = nn.ReLU()

    def forward(self, x):
        return self.linear3(self.relu(self.linear2(self.relu(self.linear1(x)))))


class ConvBnRelu(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(2, 8, 3, stride=1, padding=1)
        self.bn = nn.BatchNorm2d(8)
        self.relu = nn.ReLU()

    def forward(self, x):
        return self.relu(self.bn(self.conv(x)))


def cfg(symmetric):
    return {"defaults": {"ops": {"is_output_quantized": "True"},
                         "params": {"is_quantized": "True", "is_symmetric": str(symmetric)},
                         "strict_symmetric": "False", "per_channel_quantization": "True"}}


def make_case(name, device=DEV, **override):
    seed, symmetric, kwargs = E2E[name]
    kwargs = dict(kwargs, **override)
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    if name == "linears":
        model = ThreeLinears()
        batches = [torch.randn(16, 16, generator=g) for _ in range(2)]
    elif name == "conv":
        model = ConvBnRelu()
        batches = [torch.randn(2, 2, 6, 6, generator=g) for _ in range(2)]
    else:
        model = nn.Sequential(nn.Linear(320, 8))
        batches = [torch.randn(256, 320, generator=g) for _ in range(2)]
    model = model.eval().to(device)
    batches = [b.to(device) for b in batches]
    params = GPTVQParameters(batches, forward_fn=lambda m, d: m(d), **kwargs)
    return model, batches, params, symmetric


def run_gptvq(name, tmp_path, override=None, **kwargs):
    """apply_gptvq with every weight_update recorded, in order: each record has the hook's entries, the
    weight before ("w0"), the float64 Hessian of the same inputs ("h64") and the result ("w")."""
    model, batches, params, symmetric = make_case(name, **(override or {}))
    h64, records = {}, {}
    real_update, real_weight_update = gptvq.update_hessian, GPTVQOptimizer.weight_update.__func__

    def update_hessian(module, inp, n_samples, batch, hessian):
        real_update(module, inp, n_samples, batch, hessian)
        h = h64.setdefault(id(hessian), (hessian, torch.zeros(hessian.shape, dtype=torch.float64, device=DEV)))[1]
        update_hessian64(gptvq._unwrap(module), inp, n_samples, batch, h)

    def weight_update(cls, module, gptvq_params, hessian):
        info = {"w0": module._module_to_wrap.weight.detach().flatten(1).clone(), "h64": h64[id(hessian)][1].clone()}
        GPTVQOptimizer.record_hook = staticmethod(lambda m, rec: info.update(rec))
        try:
            real_weight_update(cls, module, gptvq_params, hessian)
        finally:
            GPTVQOptimizer.record_hook = None
        info["w"] = module._module_to_wrap.weight.detach().flatten(1).clone()
        records[id(module)] = info

    gptvq.update_hessian, GPTVQOptimizer.weight_update = update_hessian, classmethod(weight_update)
    try:
        out = GPTVQ.apply_gptvq(model, batches[0], params, str(tmp_path), config_file_path=cfg(symmetric), **kwargs)
    finally:
        gptvq.update_hessian, GPTVQOptimizer.weight_update = real_update, classmethod(real_weight_update)
    return model, out, params, symmetric, list(records.values())


def update_hessian64(module, inp, n_samples, batch, hessian):
    """gptvq.update_hessian with the scaling and the product in float64 (`hessian` is float64)."""
    inp = inp.double()
    if isinstance(module, nn.Linear):
        inp = inp.reshape(-1, inp.shape[-1]).T
    else:
        inp = torch.nn.functional.unfold(inp, module.kernel_size, dilation=module.dilation, padding=module.padding,
                                         stride=module.stride).permute(1, 0, 2).flatten(1)
    hessian *= n_samples / (n_samples + batch)
    inp = np.sqrt(2 / (n_samples + batch)) * inp
    hessian += inp @ inp.T


def qdq_grid(x, t, dtype):
    """The element arithmetic of the per-channel QDQ (nearest, half away from zero) in `dtype`, with
    the fp32 table row t = {min, max, delta, offset}; also the smallest distance of a code from a tie."""
    mn, mx, delta, offset = (dtype(v) for v in t)
    v = np.minimum(np.maximum(x, mn), mx) / delta - offset
    q = np.sign(v) * np.floor(np.abs(v) + dtype(0.5))
    tie = np.min(np.abs(np.abs(v) - np.floor(np.abs(v)) - 0.5)) if v.size else np.inf
    return (delta * (q + offset)).astype(dtype), float(tie)


def assign_with_gap(x, c):
    """First minimum over the centroids of x [N][D] against c [K][D]; (indices, best, runner-up)."""
    d = ((x[:, None, :] - c[None]) ** 2).sum(-1)
    k = np.argmin(d, axis=1)
    best = d[np.arange(len(k)), k]
    if c.shape[0] == 1:
        return k, best, np.full_like(best, np.inf)
    rest = d.copy()
    rest[np.arange(len(k)), k] = np.inf
    return k, best, rest.min(1)


def yardstick(w0, h, table, params, dtype=np.float64):
    """The reference's weight_update restated in `dtype` on numpy arrays: (weight on the grid, indices
    [rows][cols / D], [(best, runner-up)] of every decision in order, smallest QDQ tie distance)."""
    rpb, cpb, D = params.rows_per_block, params.cols_per_block, params.vector_dim
    K = 2 ** params.index_bw
    w = np.array(w0, dtype)
    h = np.array(h, dtype)
    table = np.array(table, np.float32)
    rows, cols = w.shape
    G = rows // rpb
    dead = np.diag(h) == 0
    h[dead, dead] = 1
    w[:, dead] = 0
    h[np.arange(cols), np.arange(cols)] += dtype(gptvq.DAMPENING_PERCENTAGE) * np.mean(np.diag(h))
    hinv = np.linalg.cholesky(np.linalg.inv(h).astype(dtype)).T.astype(dtype)   # upper factor of the inverse
    decisions, ties = [], [np.inf]
    indices = np.zeros((rows, cols // D), np.int64)
    cb = None
    for b0 in range(0, cols, gptvq.BLOCK_STRIDE):
        end = min(b0 + gptvq.BLOCK_STRIDE, cols)
        err = np.zeros((rows, end - b0), dtype)
        for i in range(0, end - b0, D):
            c = b0 + i
            if c % cpb == 0:
                ncols = min(cpb, cols - c)
                x = w[:, c:c + ncols].reshape(G, -1, D)
                dist = ((x - x.mean(1, keepdims=True)) ** 2).sum(-1)
                pick = np.rint(np.linspace(0, x.shape[1] - 1, K, dtype=np.float32)).astype(np.int64)
                cb = np.stack([x[g][np.argsort(dist[g], kind="stable")[pick]] for g in range(G)])
                for _ in range(params.num_of_kmeans_iterations):
                    new = np.zeros_like(cb)
                    for g in range(G):
                        k, best, second = assign_with_gap(x[g], cb[g])
                        decisions.append((best, second))
                        for j in range(K):
                            if np.any(k == j):
                                new[g, j] = x[g][k == j].sum(0) * (dtype(1) / dtype(np.sum(k == j)))
                    cb = new
                for g in range(G):
                    cb[g], tie = qdq_grid(cb[g], table[:, g], dtype)
                    ties.append(tie)
            x = w[:, c:c + D]
            k = np.zeros(rows, np.int64)
            for g in range(G):
                sel = slice(g * rpb, (g + 1) * rpb)
                k[sel], best, second = assign_with_gap(x[sel], cb[g])
                decisions.append((best, second))
            q = cb[np.arange(rows) // rpb, k]
            e = (x - q) / np.diag(hinv)[c:c + D]
            w[:, c:c + D] = q
            w[:, c + D:end] -= e @ hinv[c:c + D, c + D:end]
            err[:, i:i + D] = e
            indices[:, c // D] = k
        w[:, end:] -= err @ hinv[b0:end, end:]
    for g in range(G):
        w[g * rpb:(g + 1) * rpb], _ = qdq_grid(w[g * rpb:(g + 1) * rpb], table[:, g], dtype)
    return w, indices, decisions, min(ties)


def host_table(w, rpb, bw, symmetric):
    """The [4][G] table of the group quantizer computed on the host (for choosing seeds without a GPU):
    TF encodings of the groups' min / max and the arithmetic of aimet_per_channel_table."""
    G = w.shape[0] // rpb
    flat = np.asarray(w, np.float32).reshape(G, -1)
    encs = []
    for g in range(G):
        e = _native.TfEncodingC()
        _native.call("aimet_encoding_from_minmax", float(flat[g].min()), float(flat[g].max()), bw, int(symmetric), 0, 0,
                     ctypes.byref(e))
        encs.append(e)
    steps = np.float32(2.0 ** encs[0].bw - 1 - (1 if encs[0].min == -encs[0].max else 0))
    table = np.empty((4, G), np.float32)
    for g, e in enumerate(encs):
        mn = np.minimum(np.float32(e.min), np.float32(0))
        mx = np.maximum(np.maximum(np.float32(e.max), np.float32(0)), mn + np.float32(1e-5))
        d = (mx - mn) / steps
        table[:, g] = (mn, mx, d, np.rint(mn / d))
    return table


def yardstick_min_gap(name, seed=None):
    """The whole case in float64 on the CPU: [(smallest gap, smallest QDQ tie distance)] per module. The
    seeds in E2E were chosen with it."""
    if seed is not None:
        E2E[name] = (seed,) + E2E[name][1:]
    model, batches, params, symmetric = make_case(name, "cpu")
    model = model.double()
    out = []
    for n, m in model.named_modules():
        if not isinstance(m, gptvq.GPTVQSupportedModules):
            continue
        h = torch.zeros((m.weight[0].numel(),) * 2, dtype=torch.float64)
        seen = 0
        for b in batches:
            got = []
            handle = m.register_forward_hook(lambda _, inp, __: got.append(inp[0]))
            with torch.no_grad():
                model(b.double())
            handle.remove()
            x = got[0].unsqueeze(0) if got[0].dim() == 2 else got[0]
            update_hessian64(m, x, seen, x.shape[0], h)
            seen += x.shape[0]
        w0 = m.weight.detach().flatten(1).float().numpy()
        zeroed = w0.copy()
        zeroed[:, np.diag(h.numpy()) == 0] = 0
        table = host_table(zeroed, params.rows_per_block, params.vector_bw, symmetric)
        w64, _, decisions, tie = yardstick(w0, h.numpy(), table, params)
        out.append((min_gap(decisions), tie))
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(w64).reshape(m.weight.shape))
    return out


def min_gap(decisions):
    gaps = [np.min((second - best) / second) for best, second in decisions if np.all(np.isfinite(second))]
    return float(min(gaps)) if gaps else float("inf")


def deviation(dec32, dec64):
    """Largest |fp32 - float64| of the best and runner-up distances, relative to the float64 runner-up."""
    worst = 0.0
    for (b32, s32), (b64, s64) in zip(dec32, dec64):
        if np.all(np.isfinite(s64)):
            worst = max(worst, float(np.max(np.maximum(np.abs(b32 - b64), np.abs(s32 - s64)) / s64)))
    return worst


def measure_eps(tmp_path):
    """EPS and the smallest gaps as described above, for every module of every end-to-end case (run
    from a job script on an MI355X)."""
    lines = []
    for name in E2E:
        _, _, params, _, records = run_gptvq(name, tmp_path)
        for j, rec in enumerate(records):
            args = (rec["w0"].cpu().numpy(), rec["h64"].cpu().numpy(), rec["table"].cpu().numpy(), params)
            w64, idx64, dec64, tie = yardstick(*args)
            w32, idx32, dec32, _ = yardstick(*args, dtype=np.float32)
            same = np.array_equal(idx32, idx64)
            lines.append("%s module %d: eps %.3e  smallest gap %.3e  smallest QDQ tie distance %.3e  fp32 loop %s"
                         % (name, j, deviation(dec32, dec64), min_gap(dec64), tie,
                            "agrees" if same else "DIFFERS in %d indices" % int(np.sum(idx32 != idx64))))
    return lines


@pytest.mark.parametrize("name", list(E2E))
def test_apply_gptvq_structure_export_and_yardstick(name, tmp_path):
    model, out, params, symmetric, records = run_gptvq(name, tmp_path)
    D, K, rpb = params.vector_dim, 2 ** params.index_bw, params.rows_per_block
    names = [n for n, m in model.named_modules() if isinstance(m, gptvq.GPTVQSupportedModules)]
    assert len(records) == len(names)
    assert not any(isinstance(m, type(None)) or "Wrapper" in type(m).__name__ for m in out.modules())
    new = dict(out.named_modules())
    # 1. every candidate changed, nothing else did
    for n, m in model.named_modules():
        for pn, p in m.named_parameters(recurse=False):
            q = getattr(new[n], pn)
            if n in names and pn == "weight":
                assert not torch.equal(p, q), n
            else:
                assert torch.equal(p, q), (n, pn)
    for n, rec in zip(names, records):
        w = rec["w"].cpu().numpy()
        assert np.array_equal(bits(w), bits(new[n].weight.detach().flatten(1).cpu().numpy()))
        rows, cols = w.shape
        idx = rec["indices"].cpu().numpy()
        # 2. structure: every D-vector is the QDQ'd codebook row its index names, bit for bit
        assert len(rec["codebooks"]) == -(-cols // params.cols_per_block)
        if name == "wide":
            assert rec["codebook_cols"] == [(0, 96), (96, 96), (192, 96), (288, 32)]
        for cb, (c0, ncols) in zip(rec["codebooks"], rec["codebook_cols"]):
            cb = cb.cpu().numpy()
            assert cb.shape == (rows // rpb, K, D)
            for g in range(rows // rpb):
                block = w[g * rpb:(g + 1) * rpb, c0:c0 + ncols].reshape(rpb, -1, D)
                want = cb[g][idx[g * rpb:(g + 1) * rpb, c0 // D:(c0 + ncols) // D]]
                assert np.array_equal(bits(block), bits(want)), (n, c0, g)
                assert len(np.unique(block.reshape(-1, D), axis=0)) <= K
        # 5. the float64 yardstick: the same indices, the same weights up to fp32 rounding
        w64, idx64, decisions, tie = yardstick(rec["w0"].cpu().numpy(), rec["h64"].cpu().numpy(),
                                               rec["table"].cpu().numpy(), params)
        gap = min_gap(decisions)
        print("e2e", name, n, "smallest gap %.3g" % gap, "smallest QDQ tie distance %.3g" % tie)
        assert gap > GAP and gap >= MIN_GAP_WANTED, "the yardstick's smallest gap is too small: choose another seed"
        assert np.array_equal(idx, idx64), (n, np.argwhere(idx != idx64)[:4].tolist())
        assert np.allclose(w, w64, rtol=8 * EPS, atol=1e-30), (n, float(np.max(np.abs(w - w64))))

    # 3. export: one encoding per output channel, equal inside a row group, and a per-channel sim that
    # loads them reproduces the weights bit for bit (they lie on the grid)
    with open(tmp_path / "gptvq.encodings") as f:
        encodings = json.load(f)["param_encodings"]
    assert sorted(encodings) == sorted(n + ".weight" for n in names)
    sim = QuantizationSimModel(out, quant_scheme="tf", default_param_bw=params.vector_bw, config_file=cfg(symmetric))
    sim.load_and_freeze_encodings(str(tmp_path / "gptvq.encodings"))
    from aimet_amd.libpymo import RoundingMode
    for n in names:
        enc = encodings[n + ".weight"]
        weight = new[n].weight.detach()
        assert len(enc) == weight.shape[0]
        for i in range(0, len(enc), rpb):
            assert all(e == enc[i] for e in enc[i:i + rpb])
        q = dict(sim.model.named_modules())[n].param_quantizers["weight"]
        assert q.enabled and q.is_encoding_frozen
        assert torch.equal(q.quantize_dequantize(weight, RoundingMode.ROUND_NEAREST), weight), n


def test_excluded_modules_and_block_level_grouping(tmp_path):
    model, out, _, _, records = run_gptvq("linears", tmp_path, module_names_to_exclude=["linear2"])
    assert len(records) == 2
    assert torch.equal(out.linear2.weight, model.linear2.weight)
    assert not torch.equal(out.linear1.weight, model.linear1.weight)
    assert not torch.equal(out.linear3.weight, model.linear3.weight)
    with open(tmp_path / "gptvq.encodings") as f:
        assert sorted(json.load(f)["param_encodings"]) == ["linear1.weight", "linear3.weight"]

    # cols_per_block = 4: linear2's second codebook comes from columns that the sweep has already
    # updated through the Hessian, so the Hessian shows in the result (with one codebook per layer and
    # four centroids the assignments of this tiny layer do not move)
    small = dict(cols_per_block=4)
    _, leaf, _, _, _ = run_gptvq("linears", tmp_path, small, block_level_module_names=[["linear1"], ["linear2"]])
    _, block, _, _, _ = run_gptvq("linears", tmp_path, small, block_level_module_names=[["linear1", "linear2"]])
    # the first module sees the same inputs either way; the second one's Hessian sees the optimized
    # first module only at leaf level
    assert torch.equal(leaf.linear1.weight, block.linear1.weight)
    assert not torch.equal(leaf.linear2.weight, block.linear2.weight)
    with pytest.raises(ValueError, match="invalid module names"):
        run_gptvq("linears", tmp_path, module_names_to_exclude=["relu"])
