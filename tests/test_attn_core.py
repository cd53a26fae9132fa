"""aimet_attn_core without a GPU: the two symbols in the header, the binding and the library, and the
refusal of host tensors (there is no CPU implementation behind attn_core).

Then the float32 restatement of the core's softmax (tests/mha_oracle.py: core_row_sums, core_softmax_rows,
attn_core) and the inputs of tests/test_attn_core_gpu.py (tests/attn_core_cases.py) are sound; everything
there holds on the reference alone:
1. the restatement is a softmax: within a few ulp of the float64 softmax of the same scores;
2. the inputs tell the documented order of the row sum apart from its neighbours;
3. the inputs raise the running maximum late, with mass behind it, and clamp few scores;
4. the probe reads every key, and the case table covers what it says."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO

import attn_core_cases as C
import mha_oracle as O

from aimet_amd import _native
from aimet_amd import transformers as T

F = np.float32


@pytest.mark.parametrize("name", ["aimet_attn_core", "aimet_attn_core_launch_count"])
def test_symbol_is_declared_bound_and_exported(name):
    with open(os.path.join(REPO, "include", "aimet_amd.h")) as f:
        assert "int %s(" % name in f.read()
    assert name in _native.EXPORTED_SYMBOLS and hasattr(_native.load(), name)


def test_host_tensors_are_refused_and_the_route_is_off_by_default():
    q = torch.zeros(2, 3, 32)
    with pytest.raises(ValueError, match="GPU"):
        T.attn_core(q, q, q, 1, 2)
    m = T.QuantizableMultiheadAttention(64, 2)
    assert m.fused_core is False and T.set_fused_attention_core(m) == 1 and m.fused_core is True


MULTI_TILE = [name for name in C.CASES if C.CASES[name][1] > C.TILE]
# The worst distance of section 1 as measured over all families and encodings (it is met on the grid with the
# odd step, where x_j - m is itself rounded before exp_r sees it; 7 without that grid). The kernel's header
# estimates about 26 ulp for exp_r, the sum and the divide together. The bound is twice the measurement.
WORST_MEASURED_ULP = 19


def softmax64(x):
    x = x.astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)


def families():
    return [(name, enc) for name in C.CASES for enc in C.encodings_of(name)]


# ---- 1. the oracle against float64 -------------------------------------------------------------------------
def test_the_restated_softmax_is_within_a_few_ulp_of_float64():
    worst = {}
    for name, enc in families():
        x = C.family(name)["x"][enc]
        got, want = O.core_softmax_rows(x), softmax64(x)
        masked_row = ~np.isfinite(x).any(axis=1)
        assert np.array_equal(np.isnan(got).all(axis=1), masked_row) and not np.isnan(got[~masked_row]).any()
        assert not got[~np.isfinite(x) & ~masked_row[:, None]].any()   # a masked key is exactly +0
        open_ = np.isfinite(x)
        worst[name, enc] = int(O.ulp_distance(got[open_], want[open_].astype(F)).max())
    top = max(worst, key=worst.get)
    print("worst ulp distance to the float64 softmax: %d (%s, %s); by encoding: %s" % (
        worst[top], top[0], top[1], {e: max(v for (_, f), v in worst.items() if f == e) for e in C.SCORE_ENCS}))
    assert worst[top] <= 2 * WORST_MEASURED_ULP


def test_the_row_sum_of_one_tile_is_the_documented_one():
    """One key tile by hand: lane g owns keys 16 st + 4 g + u, adds them in increasing j, then
    (l_0 + l_2) + (l_1 + l_3). Values that make every other grouping round differently."""
    e = (F(1) + np.arange(64, dtype=F) * F(2.0 ** -20)) * F(2.0) ** (np.arange(64) % 7 - 3).astype(F)
    x = np.log(e.astype(np.float64)).astype(F)[None, :]
    m, s = O.core_row_sums(x)
    ex = O.exp_r(x[0] - m[0])
    lanes = []
    for g in range(4):
        acc = None
        for j in sorted(j for j in range(64) if j % 16 // 4 == g):
            acc = ex[j] if acc is None else F(acc + ex[j])
        lanes.append(acc)
    assert O.bits(s)[0] == O.bits(F(F(lanes[0] + lanes[2]) + F(lanes[1] + lanes[3])))
    assert m[0] == x.max()


def test_the_carry_across_tiles_is_the_documented_one():
    """Two tiles by hand on one lane's keys: a leading tile fully masked (m stays -inf, the product is taken
    as 0), a tile that raises the maximum (l * exp_r(m_(t-1) - m_t) + ts), one that does not (l + ts)."""
    inf = F(-np.inf)
    x = np.full((1, 4 * 64), inf, F)
    x[0, 64], x[0, 65] = 1.25, 0.5        # tile 1, lane 0
    x[0, 128] = 3.0                        # tile 2 raises the maximum
    x[0, 192], x[0, 193] = 3.0, -2.0       # tile 3 equals it: no rescale
    m, s = O.core_row_sums(x)
    l = F(O.exp_r(F(0.0)) + O.exp_r(F(0.5) - F(1.25)))
    l = F(F(l * O.exp_r(F(1.25) - F(3.0))) + O.exp_r(F(0.0)))
    l = F(l + F(O.exp_r(F(0.0)) + O.exp_r(F(-2.0) - F(3.0))))
    assert m[0] == F(3.0) and O.bits(s)[0] == O.bits(l)
    assert np.isnan(O.core_softmax_rows(np.full((1, 70), inf, F))).all()   # 0 / 0


# ---- 2. the inputs tell the contract apart from its neighbours --------------------------------------------
def test_the_shortcut_at_an_unchanged_maximum_is_no_variant():
    """`m_t == m_(t-1) ? l : l * exp_r(0)`: exp_r(0) is exactly 1, so taking the product instead of the
    shortcut changes no bit, and no input can tell the two apart. Recorded here instead of a variant."""
    assert O.bits(O.exp_r(F(0.0))) == O.bits(F(1.0))


@pytest.mark.parametrize("name", MULTI_TILE)
def test_the_inputs_tell_the_documented_order_from_its_neighbours(name):
    """Against a plain left-to-right sum, attn_softmax's row_sums and the contract's own lanes and tiles with
    every exponential taken against the final maximum (what a kernel with a maximum pass of its own would
    add): each changes the bits of p in one row at least, under every score encoding the case runs with. The
    last one is told apart on every family too; it differs in the fewest rows (a rescale must round)."""
    fam = C.family(name)
    for enc in C.encodings_of(name):
        x = fam["x"][enc]
        want = O.core_softmax_rows(x)
        rows = {v: C.differing_rows(want, f(x)) for v, f in C.VARIANTS.items()}
        print(name, enc, "rows of %d that differ:" % len(x), rows)
        assert all(rows.values()), (name, enc, rows)


# ---- 3. conditions on the data -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MULTI_TILE)
def test_the_running_maximum_rises_late_with_mass_behind_it(name):
    """A quarter of the rows at least raise their running maximum in a tile after the first one that held an
    open key, while the keys before that tile hold more than 2^-8 of the final sum: a wrong rescale there
    moves the sum by far more than its last bit. Over the rows with an open key; for the two families of
    C.FEW_MULTI_TILE_ROWS over the rows that see two tiles at all. And few scores clamp."""
    fam = C.family(name)
    for enc in C.encodings_of(name):
        x = fam["x"][enc]
        live, multi, ok = C.growth(x)
        print("%s %s: %d of %d rows with an open key (%d of them see two tiles) raise the maximum with mass "
              "behind it: %.2f; clamped scores %.3f" % (name, enc, ok.sum(), live.sum(), multi.sum(),
                                                        C.share(name, x), C.clamped(x, C.SCORE_ENCS[enc])))
        assert C.share(name, x) >= 0.25
        assert C.clamped(x, C.SCORE_ENCS[enc]) <= C.MAX_CLAMPED


def test_the_mask_shapes_are_the_ones_named():
    """A leading tile fully masked, a middle one, trailing ones, a wave split between rows at -inf and rows
    that are not, and one fully masked row in each."""
    def tiles_open(name):
        x = C.family(name)["x"]["none"]
        pad = np.full((len(x), 4 * C.TILE), -np.inf, F)
        pad[:, :x.shape[1]] = x
        return np.isfinite(pad.reshape(len(x), 4, C.TILE)).any(axis=2)
    for name in C.MASKED:
        assert (~tiles_open(name).any(axis=1)).sum() >= 1, name
    t = tiles_open("left_padding_197").reshape(6, 17, 4)
    assert t[:3, :16].all() and not t[3:, :16, 0].any() and t[3:, :16, 1:].all()
    t = tiles_open("middle_197")
    assert not t[:, 1].any() and t[:16, 0].all() and t[:16, 2].all()
    t = tiles_open("window_197")
    assert (t[:, 1:].sum(axis=1) == 0).any() and (~t[:, 0] & ~t[:, 3] & t[:, 1]).any() and (~t[:, 0] & t[:, 3]).any()
    t = tiles_open("causal_197").reshape(6, 197, 4)[0]
    assert t[4].tolist() == [True, False, False, False] and t[196].all()
    t = tiles_open("split_wave_197").reshape(6, 33, 4)
    assert not t[0, :3, 0].any() and t[0, 8:16, 0].all() and t[1, :8, 0].all() and not t[1, 8:16, 0].any()


# ---- 4. the probe and the table -------------------------------------------------------------------------------
def test_the_probe_reads_every_key_and_returns_the_probabilities():
    for D, S in ((32, 197), (128, 257), (32, 1), (64, 64)):
        sels = C.windows(S, D)
        assert len(sels) == -(-S // D) and set(np.concatenate(sels)) == set(range(S))
        assert all(sel.shape == (D,) and sel.max() < S for sel in sels)
    assert len(C.windows(197, 32)) == 7
    fam = C.family("probe_D32_S65")
    p = O.core_softmax_rows(fam["x"]["odd"]).reshape(fam["BH"], fam["L"], 65)
    for sel in C.windows(65, 32):
        v = np.broadcast_to(C.one_hot(sel, 65), (fam["BH"], 65, 32))
        out = O.attn_core(fam["q"], fam["k"], v, fam["B"], fam["H"], score_enc=C.SCORE_ENCS["odd"])
        assert np.array_equal(O.bits(out), O.bits(p[:, :, sel]))


def test_the_case_table_rotates_every_wave_edge_under_both_batch_sizes():
    probe = [C.CASES[n] for n in C.PROBE]
    assert {(c[0], c[1]) for c in probe} == {(D, S) for D in (32, 64, 128) for S in (1, 63, 64, 65, 197, 257)}
    assert {(c[2], c[3]) for c in probe} == {(L, BH) for L in C.LS for BH in C.BHS}
    assert {c[5] for c in probe} == {False, True}
    assert all(c[2] * c[3] > 1 for c in probe if c[1] > C.TILE)   # no multi-tile family of a single row
    assert {C.CASES[n][5] for n in C.MASKED} == {False, True}


def test_the_score_sums_are_exact_in_float32():
    """Every product is a multiple of 2^-6 and the sum of the absolute products stays below 2^8: 14 bits."""
    for name in ("probe_D128_S257", "causal_197", "grid_stride_65"):
        fam = C.family(name)
        q, k = fam["q"].astype(np.float64), fam["k"].astype(np.float64)
        assert np.array_equal(q * 8, np.round(q * 8)) and np.array_equal(k * 8, np.round(k * 8))
        assert float((np.abs(q) @ np.abs(k).transpose(0, 2, 1)).max()) < 2.0 ** 8
