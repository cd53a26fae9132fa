"""GPTVQ without a GPU (aimet_amd/gptvq.py, aimet_amd/csrc/gptvq.hip): the exported symbols and the
header, the parameter defaults, the module-name helpers against the orderings the reference's own test
asserts, the torch forms of the utilities against numpy restatements on CPU tensors, and the
self-checks of the kernels' numpy oracle (tests/gptvq_oracle.py)."""
import dataclasses
import itertools
import os

import numpy as np
import pytest
import torch
from torch import nn

import aimet_amd
import gptvq_oracle as GO
from aimet_amd import _native, gptvq
from aimet_amd.gptvq import GPTVQ, GPTVQOptimizer, GPTVQParameters

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPTVQ_SYMBOLS = ("aimet_gptvq_kmeans", "aimet_gptvq_block_update", "aimet_gptvq_update_layout")


def test_library_exports_gptvq_symbols_and_header_declares_them():
    lib = aimet_amd.native_library()
    with open(os.path.join(REPO, "include", "aimet_amd.h")) as f:
        header = f.read()
    for s in GPTVQ_SYMBOLS:
        assert hasattr(lib, s), "libaimet_amd.so does not export %s" % s
        assert s in _native.EXPORTED_SYMBOLS
        assert "int %s(" % s in header, "include/aimet_amd.h does not declare %s" % s
    assert sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("aimet_gptvq_")) == sorted(GPTVQ_SYMBOLS)


def test_entries_validate_on_the_host():
    """Bad sizes are refused before anything touches a device."""
    for args in ((0, 8, 1, 4, 8, 2, 4, 1, 0, None),        # null weight
                 (1, 8, 0, 4, 8, 2, 4, 1, 1, None),        # G = 0
                 (1, 8, 1, 4, 7, 2, 4, 1, 1, None),        # ncols % D
                 (1, 8, 1, 4, 8, 9, 4, 1, 1, None),        # D > 8
                 (1, 8, 1, 4, 8, 2, 2000, 1, 1, None),     # K > 1024
                 (1, 4, 1, 4, 8, 2, 4, 1, 1, None),        # ld < ncols
                 (1, 1 << 30, 4, 4, 8, 2, 4, 1, 1, None)):  # >= 2^31 elements
        with pytest.raises(ValueError):
            _native.call("aimet_gptvq_kmeans", *args)
    base = dict(w=1, ld=256, rows=8, rpb=4, b0=0, s0=0, s1=128, end=128, D=2, K=4)
    for change in (dict(rows=7), dict(end=130, s1=130, ld=256), dict(s1=3), dict(s0=4, s1=2), dict(ld=100),
                   dict(D=9), dict(D=4, s1=126, end=126), dict(K=0), dict(b0=-2), dict(rows=1 << 24, rpb=1, ld=1 << 8)):
        a = dict(base, **change)
        with pytest.raises(ValueError):
            _native.call("aimet_gptvq_block_update", a["w"], a["ld"], a["rows"], a["rpb"], a["b0"], a["s0"], a["s1"],
                         a["end"], a["D"], a["K"], 1, 1, a["ld"], 1, 1, None)
    with pytest.raises(ValueError):
        _native.call("aimet_gptvq_update_layout", 3, None)


def test_params_defaults_and_surface():
    p = GPTVQParameters(data_loader=[], forward_fn=None)
    assert dataclasses.asdict(p) == dict(data_loader=[], forward_fn=None, row_axis=0, col_axis=1, rows_per_block=32,
                                         cols_per_block=256, vector_dim=2, vector_bw=8, vector_stride=1, index_bw=6,
                                         num_of_kmeans_iterations=100, assignment_chunk_size=None)
    assert gptvq.GPTVQSupportedModules == (nn.Linear, nn.Conv2d)
    assert gptvq.DAMPENING_PERCENTAGE == 0.01 and gptvq.BLOCK_STRIDE == 128
    assert gptvq.HESSIAN_WEIGHTED_LOOKUP is False and gptvq.DO_CODEBOOK_FINE_TUNING is False
    for name in ("apply_gptvq", "_validate_module_names", "_get_candidate_module_name_set",
                 "_get_block_level_module_names"):
        assert callable(getattr(GPTVQ, name)), name
    for name in ("weight_update", "compute_inverse", "_update_weight_block"):
        assert callable(getattr(GPTVQOptimizer, name)), name
    for name in ("generate_codebook", "hacky_mahalanobis_init", "get_assignments", "do_kmeans_maximization",
                 "quantize_dequantize_codebook", "update_hessian", "get_2d_tensor_shape",
                 "get_module_name_to_hessian_tensor"):
        assert callable(getattr(gptvq, name)), name


class ThreeLinears(nn.Module):
    def __init__(self):
        super().__init__()
        self.linear1 = nn.Linear(16, 8)
        self.linear2 = nn.Linear(8, 8)
        self.linear3 = nn.Linear(8, 4)
        self.relu = nn.ReLU()

    def forward(self, x):
        return self.linear3(self.relu(self.linear2(self.relu(self.linear1(x)))))


def test_module_name_validation():
    model = ThreeLinears()
    with pytest.raises(ValueError, match=r"Parameter `module_names_to_exclude` contains invalid module names \(foo, bar\) "
                                         r"that don't exist in model or aren't GPTVQ supportable"):
        GPTVQ._validate_module_names(model, ["foo", "bar"], "module_names_to_exclude")
    with pytest.raises(ValueError, match=r"`block_level_module_names` contains invalid module names \(foo\)"):
        GPTVQ._validate_module_names(model, itertools.chain.from_iterable([["linear1"], ["linear2", "foo"]]),
                                     "block_level_module_names")
    with pytest.raises(ValueError, match=r"\(relu\)"):
        GPTVQ._validate_module_names(model, ["linear1", "relu"], "module_names_to_exclude")
    GPTVQ._validate_module_names(model, ["linear1", "linear2"], "module_names_to_exclude")
    GPTVQ._validate_module_names(model, itertools.chain.from_iterable([["linear1", "linear2"], ["linear3"]]),
                                 "block_level_module_names")
    assert GPTVQ._get_candidate_module_name_set(model, None) == {"linear1", "linear2", "linear3"}
    assert GPTVQ._get_candidate_module_name_set(model, ["linear2"]) == {"linear1", "linear3"}


@pytest.mark.parametrize("given, exclude, want", [
    ([["linear2"]], {"linear1"}, [["linear2"], ["linear3"]]),
    ([["linear3", "linear2"]], set(), [["linear1"], ["linear2", "linear3"]]),
    ([["linear3"], ["linear1"], ["linear2"]], set(), [["linear1"], ["linear2"], ["linear3"]]),
    ([["linear3", "linear2"], ["linear1"]], set(), [["linear1"], ["linear2", "linear3"]]),
    ([["linear2"], ["linear3", "linear1"]], set(), [["linear1", "linear3"], ["linear2"]]),
    ([["linear3", "linear1", "linear2"]], set(), [["linear1", "linear2", "linear3"]]),
    (None, set(), [["linear1"], ["linear2"], ["linear3"]]),
])
def test_block_level_module_names(given, exclude, want):
    """The seven orderings of the reference's test_gptvq_block_level_module_names."""
    model = ThreeLinears()
    assert GPTVQ._get_block_level_module_names(model, torch.randn(1, 16), given, exclude) == want


def test_apply_gptvq_raises_without_a_device(tmp_path):
    model = ThreeLinears()
    params = GPTVQParameters([torch.randn(2, 16)], forward_fn=lambda m, d: m(d), rows_per_block=4, cols_per_block=8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        GPTVQ.apply_gptvq(model, torch.randn(1, 16), params, str(tmp_path))
    with pytest.raises(RuntimeError, match="HIP"):
        gptvq.generate_codebook(torch.randn(2, 8, 2), 4)


def test_unimplemented_flags_raise(tmp_path, monkeypatch):
    model = ThreeLinears()
    params = GPTVQParameters([torch.randn(2, 16)], forward_fn=lambda m, d: m(d), rows_per_block=4, cols_per_block=8)
    for flag in ("HESSIAN_WEIGHTED_LOOKUP", "DO_CODEBOOK_FINE_TUNING"):
        with monkeypatch.context() as m:
            m.setattr(gptvq, flag, True)
            with pytest.raises(NotImplementedError, match=flag):
                GPTVQ.apply_gptvq(model, torch.randn(1, 16), params, str(tmp_path))
            with pytest.raises(NotImplementedError, match=flag):
                GPTVQOptimizer.weight_update(None, params, torch.eye(16))


# ---------------------------------------------------------------------------------------------------
# the torch forms against numpy
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, K", [((2, 40, 2), 8), ((1, 7, 4), 7), ((3, 16, 1), 5), ((1, 4, 2), 16)])
def test_hacky_mahalanobis_init(shape, K):
    rng = np.random.default_rng(sum(shape) + K)
    x = rng.standard_normal(shape).astype(np.float32)
    x[:, 1] = x[:, 0]   # equal distances: the stable sort keeps the earlier vector first
    got = gptvq.hacky_mahalanobis_init(torch.from_numpy(x), K).numpy()
    t = torch.from_numpy(x)
    dists = (t - t.mean(1).unsqueeze(1)).pow(2).sum(-1).numpy()   # the ranks come from these fp32 distances
    order = np.argsort(dists, axis=1, kind="stable")
    idx = np.rint(np.linspace(0, shape[1] - 1, K, dtype=np.float32)).astype(np.int64)
    want = np.stack([x[g][order[g][idx]] for g in range(shape[0])])
    assert got.shape == (shape[0], K, shape[2]) and np.array_equal(got, want)


def conv_columns(x, kernel, stride, padding, dilation):
    """im2col in numpy: [N][C * kh * kw][L], channel-major then kernel row, kernel column (nn.Unfold)."""
    n, c, h, w = x.shape
    kh, kw = kernel
    xp = np.zeros((n, c, h + 2 * padding[0], w + 2 * padding[1]), x.dtype)
    xp[:, :, padding[0]:padding[0] + h, padding[1]:padding[1] + w] = x
    oh = (h + 2 * padding[0] - dilation[0] * (kh - 1) - 1) // stride[0] + 1
    ow = (w + 2 * padding[1] - dilation[1] * (kw - 1) - 1) // stride[1] + 1
    cols = np.empty((n, c * kh * kw, oh * ow), x.dtype)
    for ci in range(c):
        for i in range(kh):
            for j in range(kw):
                patch = xp[:, ci, i * dilation[0]:i * dilation[0] + stride[0] * oh:stride[0],
                           j * dilation[1]:j * dilation[1] + stride[1] * ow:stride[1]]
                cols[:, (ci * kh + i) * kw + j] = patch.reshape(n, -1)
    return cols


def test_update_hessian_linear_and_conv():
    rng = np.random.default_rng(3)
    lin = nn.Linear(6, 4)
    h = torch.zeros(6, 6)
    want = np.zeros((6, 6))
    seen = 0
    for batch in (3, 2):
        x = rng.standard_normal((batch, 5, 6)).astype(np.float32)
        gptvq.update_hessian(lin, torch.from_numpy(x), seen, batch, h)
        flat = x.reshape(-1, 6).astype(np.float64)
        want = want * (seen / (seen + batch)) + (2 / (seen + batch)) * flat.T @ flat
        seen += batch
    assert np.allclose(h.numpy(), want, rtol=1e-5, atol=1e-6)
    assert tuple(gptvq.get_2d_tensor_shape(lin)) == (4, 6)

    conv = nn.Conv2d(3, 5, (3, 2), stride=(2, 1), padding=(1, 2), dilation=(1, 2))
    assert tuple(gptvq.get_2d_tensor_shape(conv)) == (5, 18)
    h = torch.zeros(18, 18)
    want = np.zeros((18, 18))
    seen = 0
    for batch in (2, 1):
        x = rng.standard_normal((batch, 3, 7, 6)).astype(np.float32)
        gptvq.update_hessian(conv, torch.from_numpy(x), seen, batch, h)
        cols = conv_columns(x.astype(np.float64), (3, 2), (2, 1), (1, 2), (1, 2))
        flat = cols.transpose(1, 0, 2).reshape(18, -1)
        want = want * (seen / (seen + batch)) + (2 / (seen + batch)) * flat @ flat.T
        seen += batch
    assert np.allclose(h.numpy(), want, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        gptvq.update_hessian(nn.ReLU(), torch.zeros(1, 2), 0, 1, torch.zeros(2, 2))


def test_get_assignments_and_maximization():
    rng = np.random.default_rng(11)
    G, N, K, D = 3, 50, 6, 2
    x = rng.standard_normal((G, N, D)).astype(np.float32)
    c = rng.standard_normal((G, K, D)).astype(np.float32)
    c[:, 4] = c[:, 2]   # a duplicate centroid: the first minimum is index 2, never 4
    x[:, 0] = c[:, 2]
    want = np.stack([GO.assign(x[g], c[g]) for g in range(G)])
    for chunk in (None, 7):
        got = gptvq.get_assignments(torch.from_numpy(x), torch.from_numpy(c), None, chunk).numpy()
        assert np.array_equal(got, want)
    assert np.all(want[:, 0] == 2) and not np.any(want == 4)
    new = gptvq.do_kmeans_maximization(torch.from_numpy(x), torch.from_numpy(c), torch.from_numpy(want).long(),
                                       None).numpy()
    want_new = GO.kmeans_step(x, c)[0]
    assert np.allclose(new, want_new, rtol=1e-5, atol=1e-6)
    assert np.all(new[:, 4] == 0.0), "an empty cluster becomes the zero vector"
    # _update_weight_block: the nearest centroid of every row's vector
    w = x[:, :4].reshape(G * 4, D)
    q, idx = GPTVQOptimizer._update_weight_block(torch.from_numpy(w), torch.from_numpy(c), D, G)
    assert np.array_equal(idx.numpy(), want[:, :4])
    assert np.array_equal(q.numpy(), np.stack([c[g][want[g, :4]] for g in range(G)]).reshape(G * 4, D))


def test_compute_inverse_is_the_upper_factor_of_the_inverse():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((12, 12))
    h = a @ a.T / 12 + np.eye(12)
    u = GPTVQOptimizer.compute_inverse(torch.from_numpy(h)).numpy()
    assert np.allclose(np.tril(u, -1), 0) and np.all(np.diag(u) > 0)
    assert np.allclose(u.T @ u, np.linalg.inv(h), rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------------------------------------
# self-checks of the kernels' oracle
# ---------------------------------------------------------------------------------------------------
def test_oracle_kmeans_self_checks():
    rng = np.random.default_rng(7)
    w = rng.standard_normal((6, 8)).astype(np.float32)
    x = GO.group_vectors(w, 3, 2)
    assert x.shape == (2, 12, 2)
    # vector n = r * (ncols / D) + t of group g
    assert np.array_equal(x[1, 1 * 4 + 2], w[3 + 1, 4:6])
    start = rng.standard_normal((2, 1, 2)).astype(np.float32)
    one = GO.kmeans(x, start, 1)
    assert np.array_equal(one, x.astype(np.float64).mean(1, keepdims=True).astype(np.float32)), "K = 1: the mean"
    start = rng.standard_normal((2, 5, 2)).astype(np.float32)
    assert np.array_equal(GO.kmeans(x, start, 0), start), "no iteration: the input"
    # K > N: the clusters without a vector become zero
    many = GO.kmeans(x[:, :3], rng.standard_normal((2, 8, 2)).astype(np.float32), 1)
    assert int(np.sum(np.all(many == 0, axis=-1))) >= 2 * (8 - 3)


def test_oracle_sweep_with_identity_hinv_is_nearest_centroid():
    rng = np.random.default_rng(9)
    rows, cols, D, K, rpb = 6, 16, 2, 5, 3
    w = rng.standard_normal((rows, cols)).astype(np.float32)
    cb = rng.standard_normal((rows // rpb, K, D)).astype(np.float32)
    before = w.copy()
    err = np.zeros((rows, 12), np.float32)
    idx = np.zeros((rows, 6), np.int32)
    GO.block_update(w, rpb, 2, 0, 12, 14, D, cb, np.eye(cols, dtype=np.float32), err, idx)
    assert np.array_equal(w[:, :2], before[:, :2]) and np.array_equal(w[:, 14:], before[:, 14:])
    for r in range(rows):
        for t in range(6):
            x = before[r, 2 + 2 * t:4 + 2 * t]
            k = int(np.argmin(((x[None] - cb[r // rpb]) ** 2).sum(-1)))
            assert idx[r, t] == k
            assert np.array_equal(w[r, 2 + 2 * t:4 + 2 * t], cb[r // rpb, k])
            assert np.array_equal(err[r, 2 * t:2 * t + 2], x - cb[r // rpb, k])
