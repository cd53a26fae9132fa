"""FP8 fake-quantization, the CPU side: the numpy oracle of the kernel's definition (shared with
tests/test_fp8_gpu.py) against the reference chain's outputs in tests/golden/golden_fp8.npz, the
candidate-table form against the golden tables and torch.linspace, the exported symbols, argument
validation and the refusals. No kernel is launched here.

The definition (csrc/fp8.hip, DESIGN.md "FP8"): M mantissa bits, E = 7 - M exponent bits,
F = (2 - 2^-M) * 2^(2^E - 1), alpha = float32(double(maxval) / F); per element
  xc = clamp(x, -maxval, maxval); q = xc / alpha (IEEE float32 divide);
  g = q rounded to M fraction bits at exponent max(floor(log2|q|), 1), ties to even, |g| <= F;
  out = float32(g * alpha);
maxval <= 0 or not finite, or alpha == 0: out = xc.

Agreement with the reference (the bounds are the issue's): every element is within 1e-5 relative
of the reference's output, or is a tie flip -- one grid step away, its exact quotient within 1e-4
(of a grid step) of a rounding tie -- and tie flips are at most 1e-4 of the elements."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, bits

import aimet_amd
from aimet_amd import _native
from aimet_amd import fp_quantization as F8

NUM_CANDIDATES = F8.NUM_CANDIDATES     # 111
REL_TOL = 1e-5           # between the 1.9e-6 the reference's chain was measured at and 2^-7
TIE_DISTANCE = 1e-4      # of a grid step
MAX_TIE_FLIPS = 1e-4     # of the elements


# ------------------------------------------------------------------------------------------------
# the oracle: float32 only where the definition says so (the divide, alpha, the result), float64 /
# integer exponents elsewhere, where every step is exact
# ------------------------------------------------------------------------------------------------
def fp8_largest(M):
    return (2.0 - 2.0 ** -M) * 2.0 ** (2 ** (7 - M) - 1)


def fp8_alpha(maxval, M):
    mv = np.asarray(maxval, np.float32)
    with np.errstate(all="ignore"):
        alpha = (mv.astype(np.float64) / fp8_largest(M)).astype(np.float32)
    return np.where((mv > 0) & np.isfinite(mv), alpha, np.float32(0)).astype(np.float32)


def fp8_clamp(x, maxval):
    x, mv = np.asarray(x, np.float32), np.asarray(maxval, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x > mv, mv, np.where(x < -mv, -mv, x)).astype(np.float32)


def fp8_grid(q, M):
    """|q| (float64 array of float32 values) on the grid: exact in float64."""
    a = np.abs(np.asarray(q, np.float64))
    _, ex = np.frexp(a)                               # a = m * 2^ex, 0.5 <= m < 1
    e = np.maximum(ex - 1, 1)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.ldexp(a, M - e))               # ties to even
        return np.minimum(np.ldexp(r, e - M), fp8_largest(M))


def fp8_cast(x, maxval, M):
    """x: float32 array; maxval: a float32 scalar or an array that broadcasts against x."""
    xc = fp8_clamp(x, maxval)
    alpha = np.broadcast_to(fp8_alpha(maxval, M), xc.shape)
    with np.errstate(all="ignore"):
        q = (xc / alpha).astype(np.float32)
        g = np.copysign(fp8_grid(q, M), q.astype(np.float64))
        out = (g * alpha.astype(np.float64)).astype(np.float32)
    return np.where(alpha == 0, xc, out).astype(np.float32)


def fp8_cast_channels(x, maxvals, M, axis):
    shape = [1] * x.ndim
    shape[axis] = -1
    return fp8_cast(x, np.asarray(maxvals, np.float32).reshape(shape), M)


def candidates(mx):
    """torch.linspace(0.1 * mx, 1.2 * mx, 111) in CPU float32: [111] for a scalar, [111][C] for [C].
    The fused multiply-adds are exact sums in float64 (31-bit product, operands within 2^8 of each
    other), rounded once."""
    mx = np.asarray(mx, np.float32).astype(np.float64)
    start = (0.1 * mx).astype(np.float32)
    end = (1.2 * mx).astype(np.float32)
    with np.errstate(all="ignore"):
        step = ((end - start).astype(np.float32) / np.float32(NUM_CANDIDATES - 1)).astype(np.float32)
    i = np.arange(NUM_CANDIDATES, dtype=np.float64).reshape((-1,) + (1,) * mx.ndim)
    lo = (step.astype(np.float64) * i + start.astype(np.float64)).astype(np.float32)
    hi = (-step.astype(np.float64) * (NUM_CANDIDATES - 1 - i) + end.astype(np.float64)).astype(np.float32)
    return np.where(i < NUM_CANDIDATES // 2, lo, hi).astype(np.float32)


def search_losses(x, M, axis=None):
    """float64 sums of squared errors [111][C] of the oracle's cast at every candidate, the
    candidates [111][C] and max|x| [C]."""
    x = np.asarray(x, np.float32)
    if axis is None:
        x3 = x.reshape(1, 1, -1)
    else:
        outer = int(np.prod(x.shape[:axis], dtype=np.int64))
        x3 = x.reshape(outer, x.shape[axis], -1)
    mx = np.abs(x3).max(axis=(0, 2)).astype(np.float32)
    cands = candidates(mx)
    losses = np.empty((NUM_CANDIDATES, x3.shape[1]), np.float64)
    for i in range(NUM_CANDIDATES):
        out = fp8_cast(x3, cands[i].reshape(1, -1, 1), M)
        losses[i] = ((x3.astype(np.float64) - out.astype(np.float64)) ** 2).sum(axis=(0, 2))
    return losses, cands, mx


def first_min_and_gap(losses):
    """Per channel: the first index of the least loss and (runner-up - best) / best."""
    first = losses.argmin(0)
    best = losses.min(0)
    rest = losses.copy()
    rest[first, np.arange(losses.shape[1])] = np.inf
    with np.errstate(all="ignore"):
        gap = (rest.min(0) - best) / np.maximum(np.abs(best), 1e-300)
    return first, gap


# ------------------------------------------------------------------------------------------------
# golden
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "golden_fp8.npz")))


def agreement(x, maxval, M, ref):
    """(elements, tie flips, worst relative difference of the others, worst tie distance)."""
    x = np.asarray(x, np.float32)
    mv = np.broadcast_to(np.asarray(maxval, np.float32), x.shape)
    got = fp8_cast(x, mv, M).astype(np.float64)
    ref = np.asarray(ref, np.float64)
    assert np.all(np.isfinite(ref))
    diff = np.abs(got - ref)
    close = diff <= REL_TOL * np.abs(ref)
    # the rest must be tie flips, judged with the exact quotient
    alpha = mv.astype(np.float64) / fp8_largest(M)
    qe = np.abs(fp8_clamp(x, mv).astype(np.float64)) / alpha
    _, ex = np.frexp(qe)
    e = np.maximum(ex - 1, 1)
    step = np.ldexp(1.0, e - M) * alpha
    t = np.ldexp(qe, M - e)
    tie_distance = np.abs(t - np.floor(t) - 0.5)
    one_step = np.abs(diff - step) <= REL_TOL * np.abs(ref)
    flip = ~close
    assert np.all(one_step[flip]), "a difference that is neither within tolerance nor one grid step"
    assert np.all(tie_distance[flip] <= TIE_DISTANCE), "a one-step difference away from a rounding tie"
    with np.errstate(all="ignore"):
        rel = np.where(close & (ref != 0), diff / np.abs(ref), 0.0)
    return x.size, int(flip.sum()), float(rel.max()), float(tie_distance[flip].max()) if flip.any() else 0.0


@pytest.mark.parametrize("M", [3, 2])
def test_oracle_against_reference_chain(golden, M):
    n = flips = 0
    worst_rel = worst_tie = 0.0
    cases = [(golden["pt_x"], golden["pt_maxval"][:, None], golden["pt_out_m%d" % M])]
    for ci in (0, 1):
        x = golden["pc%d_x" % ci]
        shape = [1] * x.ndim
        shape[int(golden["pc%d_axis" % ci])] = -1
        cases.append((x, golden["pc%d_maxval" % ci].reshape(shape), golden["pc%d_out_m%d" % (ci, M)]))
    for x, mv, ref in cases:
        a, b, c, d = agreement(x, mv, M, ref)
        n, flips, worst_rel, worst_tie = n + a, flips + b, max(worst_rel, c), max(worst_tie, d)
    print("M=%d: %d elements, %d tie flips, worst relative difference %.3g, worst tie distance %.3g"
          % (M, n, flips, worst_rel, worst_tie))
    assert flips <= MAX_TIE_FLIPS * n


def test_oracle_special_values():
    M = 3
    mv = np.float32(3.0)
    alpha = fp8_alpha(mv, M)
    assert alpha == np.float32(3.0 / 61440.0)
    x = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 3.0, -3.0, 5.0], np.float32)
    out = fp8_cast(x, mv, M)
    np.testing.assert_array_equal(bits(out), bits(np.array([0.0, -0.0, np.nan, 3.0, -3.0, 3.0, -3.0, 3.0],
                                                           np.float32)))
    # ties to even on the integer grid of the quotient: with maxval = F, alpha = 1; 16..32 has step 2
    F = np.float32(fp8_largest(M))
    ties = np.array([17.0, 19.0, 21.0, -17.0, -19.0, 0.125, 0.375, 0.625], np.float32)
    want = np.array([16.0, 20.0, 20.0, -16.0, -20.0, 0.0, 0.5, 0.5], np.float32)   # below 2: step 2^-2
    np.testing.assert_array_equal(bits(fp8_cast(ties, F, M)), bits(want))
    # no grid: the clamped input, never NaN from the cast itself
    for bad in (0.0, -1.0, np.inf, np.nan, 1e-42):
        out = fp8_cast(np.array([0.5, -0.5, 0.0], np.float32), np.float32(bad), M)
        np.testing.assert_array_equal(bits(out), bits(fp8_clamp(np.array([0.5, -0.5, 0.0], np.float32), bad)))
        assert not np.any(np.isnan(out))


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 6])
def test_oracle_values_lie_on_the_format(M):
    """Every output over maxval / F is one of the format's 2^7 magnitudes, and the largest is F."""
    E = 7 - M
    mags = {0.0}
    for e in range(2 ** E):
        for m in range(2 ** M):
            mags.add((m * 2.0 ** -M) * 2.0 if e == 0 else (1 + m * 2.0 ** -M) * 2.0 ** e)
    assert len(mags) == 2 ** 7 and max(mags) == fp8_largest(M)
    F = np.float32(fp8_largest(M))
    x = (np.random.default_rng(M).standard_normal(20000) * float(F) / 3).astype(np.float32)
    x[:2000] *= np.float32(1e-3)
    out = fp8_cast(x, F, M)       # alpha == 1
    assert set(np.abs(out.astype(np.float64)).tolist()) <= mags
    assert np.all(np.abs(out.astype(np.float64) - fp8_clamp(x, F)) <= np.maximum(np.abs(out), 2.0) * 2.0 ** -(M + 1))


def test_candidate_form(golden):
    rng = np.random.default_rng(7)
    mxs = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 300)).astype(np.float32)
    got = candidates(mxs)
    for c, mx in enumerate(mxs):
        want = torch.linspace(0.1 * float(mx), 1.2 * float(mx), NUM_CANDIDATES).numpy()
        np.testing.assert_array_equal(bits(got[:, c]), bits(want), err_msg="mx %r" % mx)
    for si in range(3):
        for M in (3, 2):
            mx = golden["s%d_minmax_m%d" % (si, M)]
            np.testing.assert_array_equal(bits(candidates(mx)), bits(golden["s%d_cands_m%d" % (si, M)]))
            # the reference's choices are rows of its own table
            best = golden["s%d_best_m%d" % (si, M)]
            table = golden["s%d_cands_m%d" % (si, M)]
            assert all(best[c] in table[:, c] for c in range(best.size))


def test_golden_minmax_is_abs_max(golden):
    for si in range(3):
        x, axis = golden["s%d_x" % si], int(golden["s%d_axis" % si])
        if axis < 0:
            want = np.abs(x).max().reshape(1)
        else:
            want = np.abs(np.moveaxis(x, axis, 0).reshape(x.shape[axis], -1)).max(1)
        np.testing.assert_array_equal(golden["s%d_minmax_m3" % si], want)


def test_oracle_search_agrees_with_the_reference_choice(golden):
    """The reference's init_mse (float32 means of its own chain) and the oracle's float64 search
    pick the same candidate wherever the oracle's best and runner-up are at least 1e-3 apart
    (relative): far above the 1e-5 agreement of the two casts and float32 summation."""
    compared = total = 0
    for si in range(3):
        x, axis = golden["s%d_x" % si], int(golden["s%d_axis" % si])
        for M in (3, 2):
            losses, cands, _ = search_losses(x, M, None if axis < 0 else axis)
            first, gap = first_min_and_gap(losses)
            chosen = cands[first, np.arange(first.size)]
            clear = gap >= 1e-3
            np.testing.assert_array_equal(chosen[clear], golden["s%d_best_m%d" % (si, M)][clear])
            compared, total = compared + int(clear.sum()), total + clear.size
    print("compared %d of %d channels" % (compared, total))
    assert compared >= total // 2


# ------------------------------------------------------------------------------------------------
# the library and the Python surface
# ------------------------------------------------------------------------------------------------
FP8_SYMBOLS = ("aimet_fp8_scale_table", "aimet_fp8_qdq", "aimet_fp8_search_workspace", "aimet_fp8_absmax",
               "aimet_fp8_search_elems", "aimet_fp8_mse_search")


def test_exported_symbols():
    lib = aimet_amd.native_library()
    for s in FP8_SYMBOLS:
        assert hasattr(lib, s) and s in _native.EXPORTED_SYMBOLS


def test_native_argument_validation():
    import ctypes
    nbytes = ctypes.c_int64(-1)
    _native.call("aimet_fp8_search_workspace", 2, 3, 1000, ctypes.byref(nbytes))
    assert nbytes.value == 4 * 3 * 2 * NUM_CANDIDATES        # one workgroup per row
    _native.call("aimet_fp8_search_workspace", 1, 1, 70001, ctypes.byref(nbytes))
    assert nbytes.value == 4 * 69 * NUM_CANDIDATES           # 69 tiles of 1024
    with pytest.raises(ValueError, match="shape"):
        _native.call("aimet_fp8_search_workspace", 1, 0, 10, ctypes.byref(nbytes))
    with pytest.raises(ValueError, match="null"):
        _native.call("aimet_fp8_search_workspace", 1, 1, 10, None)
    for M in (0, 7, -1):
        with pytest.raises(ValueError, match="mantissa"):
            _native.call("aimet_fp8_scale_table", None, 1, M, None, None)
        with pytest.raises(ValueError, match="mantissa"):
            _native.call("aimet_fp8_qdq", None, None, 1, 1, 4, None, M, None)
        with pytest.raises(ValueError, match="mantissa"):
            _native.call("aimet_fp8_mse_search", None, 1, 1, 4, None, M, 0, None, None, None, None, None, 0, None)
    with pytest.raises(ValueError, match="at least one"):
        _native.call("aimet_fp8_scale_table", None, 0, 3, None, None)
    with pytest.raises(ValueError, match="shape"):
        _native.call("aimet_fp8_qdq", None, None, 1, 0, 4, None, 3, None)
    with pytest.raises(ValueError, match="shape"):
        _native.call("aimet_fp8_absmax", None, 1, 1, 0, None, None, 0, None)
    with pytest.raises(ValueError, match="workspace"):
        _native.call("aimet_fp8_absmax", None, 1, 1, 10, None, None, 0, None)
    with pytest.raises(ValueError, match="workspace"):
        _native.call("aimet_fp8_mse_search", None, 1, 1, 10, None, 3, 0, None, None, None, None, None, 4 * 110, None)
    _native.call("aimet_fp8_qdq", None, None, 0, 1, 4, None, 3, None)   # empty: nothing to do
    with pytest.raises(ValueError, match="search elements"):
        _native.call("aimet_fp8_search_elems", 5, None)
    prev = ctypes.c_int(-1)
    _native.call("aimet_fp8_search_elems", 8, ctypes.byref(prev))
    assert prev.value == 0
    _native.call("aimet_fp8_search_elems", 0, ctypes.byref(prev))
    assert prev.value == 8


def test_python_surface_and_refusals():
    from aimet_amd import fp_quantization as F
    from aimet_amd.qc_quantize_op import StaticGridQuantWrapper
    from aimet_amd.quantizers import (QuantizationDataType, QuantScheme, StaticGridPerChannelQuantizer,
                                      StaticGridPerTensorQuantizer)
    from aimet_amd.quantsim import QuantizationSimModel
    assert F.NUM_MANTISSA_BITS == 3
    assert F.INIT_MAP == {QuantScheme.post_training_tf: F.init_minmax,
                          QuantScheme.post_training_tf_enhanced: F.init_mse,
                          QuantScheme.post_training_percentile: F.init_percentile}
    for name in ("fp8_quantizer", "quantize_to_fp8"):
        assert callable(getattr(F, name))
    with pytest.raises(NotImplementedError, match="Percentile scheme is not supported for FP8"):
        F.init_percentile(None, None, False)
    for bad in (0, 7, 2.5):
        with pytest.raises(ValueError, match="mantissa"):
            F.quantize_to_fp8(torch.zeros(4), 1.0, bad)

    q = StaticGridPerTensorQuantizer(8, "nearest", QuantScheme.post_training_percentile, False, True,
                                     data_type=QuantizationDataType.float)
    assert q.fp8_maxval is None
    with pytest.raises(NotImplementedError, match="Percentile"):
        q.update_encoding_stats(torch.zeros(4))
    with pytest.raises(ValueError, match="fp8_maxval"):
        q.quantize_dequantize(torch.zeros(4), "nearest")
    q.fp8_maxval = torch.tensor(2.0)
    q.update_maxval(torch.tensor(4.0))
    assert float(q.fp8_maxval) == float(0.9 * torch.tensor(2.0) + 0.1 * torch.tensor(4.0))
    q.compute_encoding()       # v1/tensor_quantizer.py:288-294
    assert q.encoding is not None
    q16 = StaticGridPerTensorQuantizer(16, "nearest", QuantScheme.post_training_tf, False, True,
                                       data_type=QuantizationDataType.float)
    q16.update_encoding_stats(torch.ones(4))          # fp16: skipped
    q16.compute_encoding()
    assert q16.fp8_maxval is None and q16.encoding is None
    x = torch.tensor([1.0002, -3.3e-5])
    assert torch.equal(q16.quantize_dequantize(x, "nearest"), x.half().float())
    qc = StaticGridPerChannelQuantizer(8, "nearest", QuantScheme.post_training_tf, False, 4, True,
                                       data_type=QuantizationDataType.float)
    assert qc.fp8_maxval is None and callable(qc.update_maxval)

    conv = torch.nn.Conv2d(3, 4, 3)
    w = StaticGridQuantWrapper(conv, 8, 8, "nearest", QuantScheme.post_training_tf,
                               data_type=QuantizationDataType.float)
    assert all(p.data_type == QuantizationDataType.float for p in w.param_quantizers.values())
    with pytest.raises(ValueError, match="weight_bw in \\[8, 16, 32\\]"):
        StaticGridQuantWrapper(conv, 4, 8, "nearest", QuantScheme.post_training_tf,
                               data_type=QuantizationDataType.float)
    with pytest.raises(ValueError, match="activation_bw in \\[8, 16, 32\\]"):
        StaticGridQuantWrapper(conv, 8, 4, "nearest", QuantScheme.post_training_tf,
                               data_type=QuantizationDataType.float)
    sim = QuantizationSimModel(torch.nn.Sequential(conv), quant_scheme="tf",
                               default_data_type=QuantizationDataType.float)
    assert all(q.data_type == QuantizationDataType.float for _, m in sim.quant_wrappers()
               for q in sim._quantizers_of(m))
    with pytest.raises(NotImplementedError, match="integer QDQ core"):
        QuantizationSimModel(torch.nn.Sequential(conv), quant_scheme=QuantScheme.training_range_learning_with_tf_init,
                             default_data_type=QuantizationDataType.float)
