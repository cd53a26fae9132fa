"""Inputs of the bit-for-bit tests of aimet_attn_core (aimet_amd/csrc/attn_core.hip), shared by
tests/test_attn_core.py (CPU: the oracle and these inputs are sound) and tests/test_attn_core_gpu.py (the
kernel against mha_oracle.attn_core). numpy only.

q and k are numerators over 8 in [-1, 1]: every product is a multiple of 2^-6 and every partial sum of a
score stays below 2^8, so the score product is exact in float32 in any order, and the scores are spread
over a few units instead of sitting on the top step of a grid. The last BONUS[D] dimensions are a channel:
q is 1 there, k is 1 for the keys of the last key tile and 0 for the others, which lifts the last tile by
about 2.5 standard deviations of the rest of the score (sqrt((D - c) 0.375^2): 1.95, 2.83, 4.07). Without
it a ragged last tile of one key (S = 65, 257) would hold the row maximum in 1 row of S; with it the
running maximum rises there in a third to a half of the rows, by a few units, so that the mass carried
into the rescale is visible in the final sum.
"""
import functools
import itertools

import numpy as np

import mha_oracle as O

F = np.float32
TILE = O.CORE_TILE
BONUS = {32: 5, 64: 7, 128: 10}
# score encodings of the probe: none, a power-of-two step (1/8) and a step of 29.2 / 255 with offset -99
SCORE_ENCS = {"none": None, "pow2": (-16.0, 127.0 / 8, 8), "odd": (-11.3, 17.9, 8)}
MAX_CLAMPED = 0.05          # of the open scores, asserted on the reference
LS, BHS = (1, 15, 16, 17, 65), (1, 6)

# name -> (D, S, L, BH, mask, transposed). (a): every (D, S) without a mask, L, BH and the layout rotating
# beneath so that all ten (L, BH) occur; the shift of L puts the two cases of a single row (L = BH = 1) on
# single-tile S: one row cannot be asked to tell four summation orders apart. (b): the mask shapes of real
# models.
CASES = {}
for _n, (_D, _S) in enumerate(itertools.product((32, 64, 128), (1, 63, 64, 65, 197, 257))):
    CASES["probe_D%d_S%d" % (_D, _S)] = (_D, _S, LS[(_n + 3) % 5], BHS[_n % 2], "none", bool(_n // 3 % 2))
PROBE = tuple(CASES)
CASES.update({
    "causal_65": (64, 65, 65, 6, "causal", False),
    "causal_197": (128, 197, 197, 6, "causal", True),
    "left_padding_197": (128, 197, 17, 6, "left_padding", False),
    "window_197": (128, 197, 197, 1, "window", True),
    "middle_197": (128, 197, 17, 6, "middle", False),
    "split_wave_197": (128, 197, 33, 6, "split_wave", True),
    "strides_65": (32, 65, 17, 6, "none", False),
    "grid_stride_65": (32, 65, 1, 1, "none", False),   # one row; 65538 per-item masks over it (section d)
})
MASKED = ("causal_65", "causal_197", "left_padding_197", "window_197", "middle_197", "split_wave_197")
# Families whose mask lets only a few rows see two key tiles (causal at S = 65: row 64 of each bh; the window of 8
# keys: the 7 rows around each tile boundary). A quarter of ALL their rows cannot raise the maximum in a later
# tile; the condition is taken over the rows that have open keys in two tiles.
FEW_MULTI_TILE_ROWS = ("causal_65", "window_197")
GRID_ITEMS = (1 << 16) + 2


def draw_qk(D, S, L, BH, rng):
    q = rng.integers(-8, 9, (BH, L, D)).astype(F) / F(8)
    k = rng.integers(-8, 9, (BH, S, D)).astype(F) / F(8)
    c = BONUS[D]
    q[..., D - c:] = 1.0
    k[..., D - c:] = 0.0
    if S > TILE:
        k[:, (S - 1) // TILE * TILE:, D - c:] = 1.0
    return q, k


def masks(kind, L, S, B, BH):
    """-> (attn_mask or None, key_padding_mask or None), True = masked; one fully masked row in each."""
    i, j = np.arange(L)[:, None], np.arange(S)[None, :]
    kpm = None
    if kind == "none":
        return None, None
    if kind == "causal":
        am = np.broadcast_to(j > i, (L, S)).copy()
        am[5] = True
    elif kind == "left_padding":      # batch entry 1: the first 67 keys, a whole key tile and three keys more
        kpm = np.zeros((B, S), bool)
        kpm[1, :67] = True
        am = np.zeros((L, S), bool)
        am[L - 1] = True
    elif kind == "window":            # keys i - 4 .. i + 3: leading and trailing tiles are fully masked
        am = ~((j >= i - 4) & (j <= i + 3))
        am[70] = True
    elif kind == "middle":            # the second key tile
        am = np.zeros((L, S), bool)
        am[:, TILE:2 * TILE] = True
        am[L - 1] = True
    else:
        assert kind == "split_wave"   # half of a wave's 16 rows still at -inf after the first tile
        late = np.broadcast_to((i % 16 < 8) & (j < TILE), (L, S))
        other = np.broadcast_to((i % 16 >= 8) & (j < TILE), (L, S))
        am = np.stack([late if bh % 2 == 0 else other for bh in range(BH)]).copy()
        am[0, 3] = True
    return am, kpm


def growth(x):
    """x [R, S] quantized and masked scores -> (live, multi, ok) [R] bool, in float64 from x alone. live: a
    row with an open key; multi: open keys in two key tiles or more; ok: in some tile after the first one
    that held an open key the running maximum rises while the keys before that tile hold more than 2^-8 of
    the final sum."""
    x = np.asarray(x, np.float64)
    R, S = x.shape
    n = -(-S // TILE)
    pad = np.full((R, n * TILE), -np.inf)
    pad[:, :S] = x
    pad = pad.reshape(R, n, TILE)
    tm = pad.max(axis=2)
    live = np.isfinite(tm.max(axis=1))
    with np.errstate(all="ignore"):
        e = np.where(np.isfinite(pad), np.exp(pad - tm.max(axis=1)[:, None, None]), 0.0)
    mass = e.sum(axis=2)
    before = np.cumsum(mass, axis=1) - mass
    run = np.maximum.accumulate(tm, axis=1)
    run_before = np.concatenate([np.full((R, 1), -np.inf), run[:, :-1]], axis=1)
    rises = np.isfinite(run_before) & (tm > run_before) & (before > 2.0 ** -8 * mass.sum(axis=1, keepdims=True))
    return live, np.isfinite(tm).sum(axis=1) >= 2, rises.any(axis=1) & live


def share(name, x):
    """The share of rows of growth() that the family `name` must keep at a quarter or more."""
    live, multi, ok = growth(x)
    rows = multi if name in FEW_MULTI_TILE_ROWS else live
    return float(ok.sum()) / max(int(rows.sum()), 1)


# ---- the neighbours of the contract: what the probe inputs must tell apart ---------------------------
def _final(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        m = x.max(axis=1, keepdims=True)
        return np.where(x == F(-np.inf), F(0), O.exp_r(x - m)).astype(F)


def left_to_right(x):
    e = _final(x)
    s = e[:, 0].copy()
    for j in range(1, e.shape[1]):
        s = s + e[:, j]
    with np.errstate(all="ignore"):
        return e / s[:, None]


def one_pass_final_maximum(x):
    """The contract's lanes, tiles and butterfly, every e_j against the FINAL maximum and no rescale: the
    arithmetic of a kernel that finds the maximum in a pass of its own."""
    e = _final(x)
    R, S = e.shape
    n = -(-S // TILE)
    pad = np.zeros((R, n * TILE), F)
    pad[:, :S] = e
    pad = pad.reshape(R, n, 4, 4, 4)
    l = np.zeros((R, 4), F)
    for t in range(n):
        ts = pad[:, t, 0, :, 0]
        for st in range(4):
            for u in range(4):
                if st or u:
                    ts = ts + pad[:, t, st, :, u]
        l = l + ts
    with np.errstate(all="ignore"):
        return e / ((l[:, 0] + l[:, 2]) + (l[:, 1] + l[:, 3]))[:, None]


VARIANTS = {"left_to_right": left_to_right, "attn_softmax_row_sums": O.softmax_rows,
            "one_pass_final_maximum": one_pass_final_maximum}


def differing_rows(a, b):
    """Rows in which two probability tables differ in some bit (a NaN row equals a NaN row)."""
    same = (O.bits(a) == O.bits(b)) | (np.isnan(a) & np.isnan(b))
    return int((~same.all(axis=1)).sum())


# ---- a family: the inputs of one case and, per score encoding, its scores ------------------------------
def encodings_of(name):
    """The score encodings a case runs with: all three; the 65538 items of the grid-stride case the odd one."""
    return ("odd",) if name == "grid_stride_65" else tuple(SCORE_ENCS)


def build(name, seed, items=GRID_ITEMS):
    D, S, L, BH, kind, transposed = CASES[name]
    B = 1 if BH == 1 else 2
    q, k = draw_qk(D, S, L, BH, np.random.default_rng(seed))
    if name == "grid_stride_65":   # one q row and one k for every item; the items differ by their masks
        am = np.random.default_rng(seed + 500).random((items, 1, S)) < 0.3
        am[[7, items - 2]] = True   # fully masked items; of 65538, the second is the first of the second trip
        fam = dict(B=items, H=1, per_bh=True, kpm=None, am=am, q=q, k=k)   # q and k: the one shared matrix
    else:
        am, kpm = masks(kind, L, S, B, BH)
        fam = dict(B=B, H=BH // B, per_bh=am is not None and am.ndim == 3, kpm=kpm, am=am, q=q, k=k)
    fam.update(name=name, D=D, S=S, L=L, BH=fam["B"] * fam["H"], transposed=transposed, seed=seed)
    fam["x"] = {}
    for enc_name in encodings_of(name):
        enc = SCORE_ENCS[enc_name]
        if name == "grid_stride_65":   # the product once, not once an item
            x = O.core_scores(q, k, 1, 1, score_enc=enc)
            x = np.where(am, F(-np.inf), np.broadcast_to(x, am.shape))
        else:
            x = O.core_scores(q, k, fam["B"], fam["H"], am, fam["per_bh"], kpm, enc)
        fam["x"][enc_name] = x.reshape(-1, S)
    return fam


def clamped(x, enc):
    """The share of the open scores on either end step of the grid (their own value or clamped to it)."""
    if enc is None:
        return 0.0
    lo, hi = O.qdq(np.array([-1e30, 1e30], F), enc)
    return float(((x == lo) | (x == hi))[np.isfinite(x)].mean())


def sound(fam):
    """The conditions on a multi-tile family, on the reference alone: see tests/test_attn_core.py."""
    if fam["S"] <= TILE:
        return True
    for enc_name, x in fam["x"].items():
        if share(fam["name"], x) < 0.25 or clamped(x, SCORE_ENCS[enc_name]) > MAX_CLAMPED:
            return False
        want = O.core_softmax_rows(x)
        if any(differing_rows(want, f(x)) == 0 for f in VARIANTS.values()):
            return False
    return True


@functools.lru_cache(None)
def family(name):
    """The case's inputs from the first seed on which sound() holds; the tests assert each condition again.
    The grid-stride case chooses its seed on its first 2048 items and is then built whole."""
    small = {"items": 2048} if name == "grid_stride_65" else {}
    for seed in range(32):
        fam = build(name, 1000 * sorted(CASES).index(name) + seed, **small)
        if sound(fam):
            break
    return build(name, fam["seed"]) if small else fam


def windows(S, D):
    """Selections sel [D] of keys such that every key of the row is selected once at least."""
    return [np.minimum(start + np.arange(D), S - 1) for start in range(0, S, D)]


def one_hot(sel, S):
    """v [S, D] with v[j][d] = 1 where j == sel[d]: then out[r][d] is p[r][sel[d]] exactly, whatever order the
    matrix core adds the zeros in."""
    v = np.zeros((S, len(sel)), F)
    v[sel, np.arange(len(sel))] = 1.0
    return v
