"""aimet_attn_core (csrc/attn_core.hip) and the opt-in `fused_core` route of QuantizableMultiheadAttention
against the literal chain restated in float64 on the CPU:

    out = QDQ_out( QDQ_prob( softmax( mask( QDQ_score(q k^T) ) ) ) v )

The kernel's tiles: 64 query rows an item (16 a wave), 64 keys a tile (four subtiles of 16), a grid capped
at 65536 items. The shapes below are the smallest around them.

Sections 5 to 10 hold the kernel to tests/mha_oracle.py's attn_core, the float32 restatement of the order of
the row sum that the kernel's header documents, bit for bit and without exemptions, on the inputs of
tests/attn_core_cases.py (tests/test_attn_core.py shows on the CPU that those inputs tell that order apart
from its neighbours)."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import gpu_available

import attn_core_cases as C
import mha_oracle as O

from aimet_amd import transformers as T
from aimet_amd.elementwise_ops import TRANSFORMER_QUANTIZABLE_TYPES
from aimet_amd.libpymo import RoundingMode, TfEncoding
from aimet_amd.qc_quantize_op import QcQuantizeOpMode
from aimet_amd.quantizers import QuantScheme, StaticGridPerTensorQuantizer
from aimet_amd.quantsim import QuantizationSimModel

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]
DEV, SENTINEL, GUARD = "cuda", -777.25, 64
ROW_TILE, KEY_TILE, MAX_GRID = 64, 64, 1 << 16
INF = float("inf")


def grid(enc):
    """(lo, hi, delta, offset) of an encoding (min, max, bw) as the library fills it in."""
    steps = 2.0 ** enc[2] - 1
    delta = (enc[1] - enc[0]) / steps
    offset = round(enc[0] / delta)
    return offset * delta, delta * steps + offset * delta, delta, offset


def qdq64(x, enc):
    """The oracle's QDQ arithmetic in float64: clamp (a NaN takes the grid's top), divide, round half away."""
    if enc is None:
        return x
    lo, hi, delta, offset = grid(enc)
    t = torch.where(x.isnan(), torch.full_like(x, hi), x).clamp(lo, hi) / delta - offset
    return delta * (torch.sign(t) * torch.floor(t.abs() + 0.5) + offset)


def chain64(q, k, v, B, am, kpm, encs):
    """-> (out, the unquantized probabilities, out before its QDQ), float64."""
    q, k, v = (t.double().cpu() for t in (q, k, v))
    BH, L, S = q.shape[0], q.shape[1], k.shape[1]
    s = qdq64(q @ k.transpose(1, 2), encs[0])
    if am is not None:
        s = s.masked_fill(am.cpu(), -INF)
    if kpm is not None:
        s = s.view(B, BH // B, L, S).masked_fill(kpm.cpu().view(B, 1, 1, S), -INF).view(BH, L, S)
    p = torch.softmax(s, dim=-1)   # NaN in a fully masked row
    raw = qdq64(p, encs[1]) @ v
    return qdq64(raw, encs[2]), p, raw


# ---- 1. exact sums: dyadic inputs and power-of-two grids, so that only the softmax can differ -----------
SCORE, PROB, OUT = (-8.0, 127.0 / 16, 8), (0.0, 255.0 / 256, 8), (-8.0, 127.0 / 16, 8)
ENCS = {"all": (SCORE, PROB, OUT), "no_score": (None, PROB, OUT), "no_prob": (SCORE, None, OUT),
        "none": (None, None, None)}
MASKS = ("none", "2d", "3d", "padding", "2d_padding")
S_ALL = (1, KEY_TILE - 1, KEY_TILE, KEY_TILE + 1, 3 * KEY_TILE + 5)
# every (D, S, mask); L, BH, the encodings and the layout rotate beneath them so that all 32 of their
# combinations occur. The last case has 65538 items: two of them are a second trip of the grid-stride loop.
CASES = [(D, S, mask, (1, ROW_TILE + 1)[n % 2], (1, 6)[n // 2 % 2], tuple(ENCS)[n // 4 % 4], bool(n // 16 % 2))
         for n, (D, S, mask) in enumerate(itertools.product((32, 64, 128), S_ALL, MASKS))]
CASES.append((32, 2, "none", 1, MAX_GRID + 2, "all", False))


def draw(D, S, mask, L, BH, enc, seed):
    B = 1 if BH == 1 else 2
    g = torch.Generator().manual_seed(seed)
    dyadic = lambda rows: torch.randint(-16, 17, (rows, BH, D), generator=g).float() / 8   # noqa: E731
    q, k, v = dyadic(L), dyadic(S), dyadic(S)   # [rows, BH, D]: the module's layout
    am = kpm = None
    if "2d" in mask or "3d" in mask:
        am = torch.rand((BH if "3d" in mask else 1, L, S), generator=g) < 0.3
        am[..., 0] = False
        am[0, L - 1, :] = True   # one fully masked row (of every bh for the 2-D table)
        am = am if "3d" in mask else am[0]
    if "padding" in mask:
        kpm = (torch.arange(S)[None, :] + torch.arange(B)[:, None]) % 5 == 2
    want, p, raw = chain64(*(t.transpose(0, 1) for t in (q, k, v)), B, am, kpm, ENCS[enc])
    exempt = torch.zeros(BH, L, dtype=torch.bool)
    if ENCS[enc][1] is not None:   # a probability within 2^-10 of a rounding tie of the 2^-8 grid
        exempt = ((p * 256 - torch.floor(p * 256) - 0.5).abs() <= 2.0 ** -10).any(-1)
    return (q, k, v, am, kpm, B), (want.float(), raw, exempt)


@functools.lru_cache(None)
def exact_case(D, S, mask, L, BH, enc):
    """The case's inputs and reference, from the first seed whose REFERENCE exempts at most 2 % of the rows
    (a case of 1 or 6 rows: none); the test asserts the condition again."""
    for seed in range(16):
        case = draw(D, S, mask, L, BH, enc, 100 * (D + S) + seed)
        if float(case[1][2].float().mean()) <= 0.02:
            break
    return case


@pytest.mark.parametrize("D,S,mask,L,BH,enc,transposed", CASES)
def test_exact_sums_equal_the_float64_chain_bit_for_bit(D, S, mask, L, BH, enc, transposed):
    (q, k, v, am, kpm, B), (want, raw, exempt) = exact_case(D, S, mask, L, BH, enc)
    assert float(exempt.float().mean()) <= 0.02   # the condition on the seeds; it holds on the reference alone
    dev = lambda t: None if t is None else t.to(DEV)   # noqa: E731
    ops = [dev(t).transpose(0, 1) if transposed else dev(t.transpose(0, 1).contiguous()) for t in (q, k, v)]
    buf = torch.full((GUARD + BH * L * D + GUARD,), SENTINEL, device=DEV)
    n = T.attn_core_launch_count()
    got = T.attn_core(*ops, B, BH // B, dev(am), dev(kpm), *ENCS[enc], out=buf[GUARD:-GUARD].view(BH, L, D))
    assert T.attn_core_launch_count() == n + 1
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    got = got.cpu()
    if ENCS[enc][1] is not None:
        same = ((got == want) | (got.isnan() & want.isnan())).all(-1)
        print("rows exempt: %d of %d; differing rows: %d" % (int(exempt.sum()), exempt.numel(), int((~same).sum())))
        assert bool((same | exempt).all())
        return
    # Without the probability QDQ the second product's sums are not exact. |out - out64| <= (32 + S) 2^-24
    # max|v|: p within about 26 ulp (exp_r within 3, the sum, one divide) and sum_j p_j = 1, plus S roundings
    # of the accumulation. An output within that distance of a rounding tie of its grid may flip: exempt.
    bound = (32 + S) * 2.0 ** -24 * 2.0
    near_tie = torch.zeros_like(raw, dtype=torch.bool)
    if ENCS[enc][2] is not None:
        t = raw / grid(OUT)[2]
        near_tie = (t - torch.floor(t) - 0.5).abs() * grid(OUT)[2] <= bound
    err = (got.double() - want.double()).abs()
    ok = (err <= bound) | near_tie | (got.isnan() & want.isnan())
    print("max |out - out64| = %.3g of the bound %.3g; near a tie: %d" % (float(err[~near_tie].nan_to_num().max()),
                                                                           bound, int(near_tie.sum())))
    assert bool(ok.all()) and float(near_tie.float().mean()) <= 0.02


# ---- 2. general data, one key past the row the fused softmax keeps on chip -------------------------------
def wrong(got, want, enc):
    """Elements further than half an output step from the float64 chain."""
    return int(((got.double().cpu() - want).abs() > grid(enc)[2] / 2).sum())


def tf_encoding(enc):
    e = TfEncoding()
    e.min, e.max, e.delta, e.offset = grid(enc)
    e.bw = enc[2]
    return e


def literal(q, k, v, encs):
    """The module's literal route on q, k, v: torch's products and softmax, the library's QDQ kernels."""
    def qdq(x, enc):
        z = StaticGridPerTensorQuantizer(8, "nearest", QuantScheme.post_training_tf, False, enabled_by_default=True)
        z.encoding = tf_encoding(enc)
        return z.quantize_dequantize(x, RoundingMode.ROUND_NEAREST)
    return qdq(torch.bmm(qdq(torch.softmax(qdq(torch.bmm(q, k.transpose(1, 2)), encs[0]), -1), encs[1]), v), encs[2])


def test_gaussian_data_past_the_resident_row_against_the_literal_route():
    BH, L, S, D = 2, 3, T.attn_softmax_max_s() + 1, 64
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(BH, n, D, generator=g) for n in (L, S, S))
    q = q / 8   # scores of unit variance
    _, p, raw = chain64(q, k, v, 1, None, None, (None, None, None))
    s = q.double() @ k.double().transpose(1, 2)
    encs = [(float(s.min()), float(s.max()), 8), (0.0, float(p.max()), 8)]
    encs.append((float(raw.min()), float(raw.max()), 8))   # realistic 8-bit ranges from the unquantized chain
    want = chain64(q, k, v, 1, None, None, encs)[0]
    q, k, v = (t.to(DEV) for t in (q, k, v))
    core, lit = wrong(T.attn_core(q, k, v, 1, BH, None, None, *encs), want, encs[2]), \
        wrong(literal(q, k, v, encs), want, encs[2])
    line = "attn_core: %d, literal route: %d of %d elements beyond half an output step" % (core, lit, want.numel())
    print(line)
    if os.environ.get("AIMET_ATTN_CORE_PARITY_OUT"):
        with open(os.environ["AIMET_ATTN_CORE_PARITY_OUT"], "a") as f:
            f.write(line + "\n")
    assert core <= 2 * lit + 0.01 * want.numel()


# ---- 3. the module ------------------------------------------------------------------------------------------
def build_sim(E=64, heads=2):
    torch.manual_seed(3)
    m = T.QuantizableMultiheadAttention(E, heads, add_bias_kv=True, add_zero_attn=True, batch_first=True).to(DEV).eval()
    x = torch.randn(2, 5, E, device=DEV)
    kpm = torch.tensor([[False] * 5, [False, False, False, True, True]], device=DEV)
    sim = QuantizationSimModel(m, dummy_input=(x, x, x), quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)
    sim.compute_encodings(lambda model, _: model(x, x, x, key_padding_mask=kpm))
    assert T.set_fused_attention_core(sim.model) == 1 and sim.model.fused_core
    return sim.model, x, kpm


def run(attn, x, kpm, core, grad=False, **kw):
    attn.fused_core = core
    n, c = T.attn_launch_count(), T.attn_core_launch_count()
    with torch.set_grad_enabled(grad):
        out = attn(x, x, x, key_padding_mask=kpm, **kw)
    return out, T.attn_launch_count() - n, T.attn_core_launch_count() - c


def test_module_takes_the_core_route_in_one_launch():
    attn, x, kpm = build_sim()
    (got, _), softmax_launches, core_launches = run(attn, x, kpm, True, need_weights=False)
    assert (softmax_launches, core_launches) == (0, 1)
    (want, _), softmax_launches, core_launches = run(attn, x, kpm, False, need_weights=False)
    assert (softmax_launches, core_launches) == (1, 0)
    e = attn.out_proj.output_quantizers[0].encoding
    off = int(((got - want).abs() > e.delta / 2).sum())   # the other route's own flips are not known here: 0
    print("elements beyond half an output step of fused_core = False: %d of %d" % (off, want.numel()))
    assert off <= 0.01 * want.numel()


@pytest.mark.parametrize("case", ["need_weights", "gradient", "analysis", "head_dim_48"])
def test_module_keeps_the_other_routes(case):
    attn, x, kpm = build_sim(*((96, 2) if case == "head_dim_48" else ()))
    kw = {"need_weights": case == "need_weights", "grad": case == "gradient"}
    if case == "analysis":
        for w in (attn.matmul_1, attn.softmax, attn.matmul_2):
            w.set_mode(QcQuantizeOpMode.ANALYSIS)
    (got, gw), _, core_launches = run(attn, x, kpm, True, **kw)
    (want, ww), _, _ = run(attn, x, kpm, False, **kw)
    assert core_launches == 0 and torch.equal(got, want) and (gw is None or torch.equal(gw, ww))


# ---- 4. refusals ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["head_dim_48", "host_tensor", "out_overlaps_v"])
def test_refusals_leave_the_output_untouched(case):
    D = 48 if case == "head_dim_48" else 32
    q, k, v = (torch.zeros(2, 3, D, device=DEV) for _ in range(3))
    buf = torch.full((GUARD + 2 * 3 * D + GUARD,), SENTINEL, device=DEV)
    out = buf[GUARD:-GUARD].view(2, 3, D)
    if case == "host_tensor":
        k = k.cpu()
    if case == "out_overlaps_v":
        v = buf[GUARD + D:GUARD + D + 2 * 3 * D].view(2, 3, D)
    n = T.attn_core_launch_count()
    with pytest.raises(ValueError):
        T.attn_core(q, k, v, 1, 2, out=out)
    assert T.attn_core_launch_count() == n and bool((buf == SENTINEL).all())


# ---- 5. the probabilities themselves, bit for bit against the restated order of the row sum ---------------
# v[j][d] = 1 where j == sel[d] and 0 elsewhere, no probability and no output QDQ: out[r][d] is p[r][sel[d]]
# exactly, whatever order the matrix core adds the zeros in. The selections slide over all keys.
def to_dev(a, transposed=False):
    """A [BH, rows, D] array on the device: contiguous, or the module's [rows, BH, D] memory transposed."""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a))   # a copy: the cases' arrays may be read-only broadcasts
    return t.transpose(0, 1).contiguous().to(DEV).transpose(0, 1) if transposed else t.to(DEV)


def launch(q, k, v, B, H, am, kpm, encs):
    """One launch on device operands into a guarded buffer -> out as a numpy array."""
    BH, L, D = q.shape
    buf = torch.full((GUARD + BH * L * D + GUARD,), SENTINEL, device=DEV)
    n = T.attn_core_launch_count()
    T.attn_core(q, k, v, B, H, am, kpm, *encs, out=buf[GUARD:-GUARD].view(BH, L, D))
    assert T.attn_core_launch_count() == n + 1
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    return buf[GUARD:-GUARD].view(BH, L, D).cpu().numpy()


def assert_same_bits(got, want, where, sel=None):
    """Equal bits, a NaN where a NaN is expected; the first difference named as (bh, row, column or key)."""
    same = (O.bits(got) == O.bits(want)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        bh, row, d = (int(i) for i in np.argwhere(~same)[0])
        key = "key %d" % sel[d] if sel is not None else "column %d" % d
        raise AssertionError("%s: %d elements differ, the first at bh %d, row %d, %s: got %r (0x%08x), want %r "
                             "(0x%08x)" % (where, int((~same).sum()), bh, row, key, got[bh, row, d],
                                           O.bits(got)[bh, row, d], want[bh, row, d], O.bits(want)[bh, row, d]))


def probe(name, wrap=lambda q, k, v: (q, k, v)):
    """The case `name` of attn_core_cases under each of its score encodings, a launch a selection; `wrap`
    may move the device operands into other memory."""
    fam = C.family(name)
    D, S, L, BH, B, H = (fam[key] for key in ("D", "S", "L", "BH", "B", "H"))
    q, k = to_dev(fam["q"], fam["transposed"]), to_dev(fam["k"], fam["transposed"])
    am = None if fam["am"] is None else torch.from_numpy(fam["am"]).to(DEV)
    kpm = None if fam["kpm"] is None else torch.from_numpy(fam["kpm"]).to(DEV)
    for enc_name in C.encodings_of(name):
        enc = C.SCORE_ENCS[enc_name]
        if S > C.TILE:   # the conditions on the data, again (tests/test_attn_core.py)
            assert C.share(name, fam["x"][enc_name]) >= 0.25 and C.clamped(fam["x"][enc_name], enc) <= C.MAX_CLAMPED
        for sel in C.windows(S, D):
            v = np.broadcast_to(C.one_hot(sel, S), (BH, S, D))
            want = O.attn_core(fam["q"], fam["k"], v, B, H, fam["am"], fam["per_bh"], fam["kpm"], enc)
            got = launch(*wrap(q, k, to_dev(v, fam["transposed"])), B, H, am, kpm, (enc, None, None))
            assert_same_bits(got, want, "%s (D %d, S %d, L %d, BH %d), score encoding %s" % (name, D, S, L, BH, enc_name),
                             sel)


@pytest.mark.parametrize("name", C.PROBE)
def test_probabilities_equal_the_restated_order_bit_for_bit(name):
    probe(name)


# ---- 6. the mask shapes of real models ---------------------------------------------------------------------
@pytest.mark.parametrize("name", C.MASKED)
def test_masked_probabilities_equal_the_restated_order_bit_for_bit(name):
    """Causal; left padding (a leading key tile fully masked: the running maximum still -inf when content
    arrives); a window of 8 keys (leading and trailing tiles fully masked); the middle tile fully masked; a
    wave whose rows 0..7 open only keys >= 64 while rows 8..15 open key 0. One fully masked row in each: NaN."""
    probe(name)
    fam = C.family(name)
    x = fam["x"]["none"]
    assert (~np.isfinite(x).any(axis=1)).sum() >= 1   # the fully masked row, NaN on both sides above


# ---- 7. the whole kernel, bit for bit, no exemptions ---------------------------------------------------------
# Section 1's construction with the q and k of section 5: v numerators over 8 in [-2, 2] and the probabilities
# on the 2^-8 grid make every partial sum of the second product exact (multiples of 2^-11 below 2^9), and the
# oracle predicts the side of every rounding tie of the probability grid.
WHOLE = [(D, S, enc, mask, (15, 17, 65)[n % 3], (1, 6)[n % 2], bool(n // 2 % 2))
         for n, (D, S, enc, mask) in enumerate(itertools.product((32, 64, 128), (KEY_TILE + 1, 3 * KEY_TILE + 5),
                                                                 ("all", "no_score"), ("none", "causal")))]


@pytest.mark.parametrize("D,S,enc,mask,L,BH,transposed", WHOLE)
def test_whole_kernel_equals_the_oracle_bit_for_bit(D, S, enc, mask, L, BH, transposed):
    L, B = S if mask == "causal" else L, 1 if BH == 1 else 2
    rng = np.random.default_rng(7 * D + S + BH)
    q, k = C.draw_qk(D, S, L, BH, rng)
    v = rng.integers(-16, 17, (BH, S, D)).astype(np.float32) / np.float32(8)
    am, _ = C.masks(mask, L, S, B, BH)
    want = O.attn_core(q, k, v, B, BH // B, am, False, None, *ENCS[enc])
    assert np.isfinite(want).all()   # the fully masked causal row: the probability grid's top times v
    got = launch(*(to_dev(t, transposed) for t in (q, k, v)), B, BH // B,
                 None if am is None else torch.from_numpy(am).to(DEV), None, ENCS[enc])
    assert_same_bits(got, want, "D %d, S %d, L %d, BH %d, %s, %s" % (D, S, L, BH, enc, mask))


# ---- 8. the second grid-stride trip over two key tiles --------------------------------------------------------
def test_second_grid_stride_trip_over_two_key_tiles():
    """65538 items of L = 1, S = 65, D = 32: the binding takes expanded views (a bh stride of 0), so q, k and v
    are ONE matrix each expanded over bh, and a per-bh mask [65538, 1, 65] makes the items differ: 4 MB of
    mask and 8 MB of output, no real tensor of 65538 matrices. Every item is compared, items 0, 65535, 65536
    (the first of the second trip, fully masked: NaN) and 65537 first; the output sits between guards."""
    fam = C.family("grid_stride_65")
    BH, S, D = fam["BH"], fam["S"], fam["D"]
    assert BH == MAX_GRID + 2 and S > KEY_TILE
    enc = C.SCORE_ENCS["odd"]
    x = fam["x"]["odd"]
    assert C.share("grid_stride_65", x) >= 0.25
    p = O.core_softmax_rows(x)
    assert np.isnan(p[MAX_GRID]).all() and np.isfinite(p[[0, MAX_GRID - 1, MAX_GRID + 1]]).all()
    q = torch.from_numpy(fam["q"]).to(DEV).expand(BH, 1, D)
    k = torch.from_numpy(fam["k"]).to(DEV).expand(BH, S, D)
    am = torch.from_numpy(fam["am"]).to(DEV)
    assert q.stride(0) == 0 and k.stride(0) == 0
    for sel in C.windows(S, D):
        v = torch.from_numpy(C.one_hot(sel, S)).to(DEV)[None].expand(BH, S, D)
        got = launch(q, k, v, BH, 1, am, None, (enc, None, None))
        want = p[:, None, sel]
        for item in (0, MAX_GRID - 1, MAX_GRID, MAX_GRID + 1):
            assert_same_bits(got[item:item + 1], want[item:item + 1], "item %d" % item, sel)
        assert_same_bits(got, want, "65538 items", sel)


# ---- 9. strides -----------------------------------------------------------------------------------------------
def test_padded_row_and_matrix_strides_are_read_in_place():
    """k and v with rows D + 4 floats apart and q with two rows of padding a matrix, the padding NaN: a read
    outside a row's D floats or a matrix's L rows would reach the probabilities."""
    def wrap(q, k, v):
        out = []
        for t, pad_rows, pad_cols in ((q, 2, 0), (k, 0, 4), (v, 0, 4)):
            buf = torch.full((t.shape[0], t.shape[1] + pad_rows, t.shape[2] + pad_cols), float("nan"), device=DEV)
            view = buf[:, :t.shape[1], :t.shape[2]]
            view.copy_(t)
            out.append(view)
        assert out[0].stride() == ((q.shape[1] + 2) * q.shape[2], q.shape[2], 1)
        assert out[1].stride(1) == k.shape[2] + 4 and out[2].stride(1) == v.shape[2] + 4
        return out
    probe("strides_65", wrap)


# ---- 10. the module, with a named expectation -------------------------------------------------------------------
MODULE_ENCS = {"linear_Q": (-8.0, 127.0 / 16, 8), "linear_K": (-8.0, 127.0 / 16, 8), "linear_V": (-8.0, 127.0 / 16, 8),
               "div": (-2.0, 127.0 / 64, 8), "matmul_1": (-16.0, 127.0 / 8, 8), "softmax": (0.0, 255.0 / 256, 8),
               "matmul_2": (-8.0, 127.0 / 16, 8), "out_proj": (-16.0, 127.0 / 8, 8), "weight": (-2.0, 127.0 / 64, 8)}


def module_case():
    """Weights, biases and inputs are numerators over 64 or 16 and every encoding is a power-of-two grid: every
    sum of every linear layer and of both products is exact in float32, so the module's output is what
    mha_oracle.mha_forward gives with the core's softmax, to the bit. 70 tokens and the two appended keys
    (bias_k, the zero key): S = 72, two key tiles."""
    E, tokens, batch = 64, 70, 2
    rng = np.random.default_rng(11)

    def num(shape, lim, den):
        return rng.integers(-lim, lim + 1, shape).astype(np.float32) / np.float32(den)
    w = {}
    for name, lim in (("linear_Q", 32), ("linear_K", 8), ("linear_V", 32), ("out_proj", 32)):
        w[name + ".weight"], w[name + ".bias"] = num((E, E), lim, 64), num((E,), 16, 16)
    w["bias_k"], w["bias_v"] = num((1, 1, E), 16, 16), num((1, 1, E), 16, 16)
    x = num((batch, tokens, E), 32, 16)
    causal = np.triu(np.ones((tokens, tokens), bool), 1)
    kpm = np.zeros((batch, tokens), bool)
    kpm[1, tokens - 9:] = True
    return w, x, causal, kpm


def test_module_output_equals_the_oracle_bit_for_bit():
    w, x, causal, kpm = module_case()
    want, _ = O.mha_forward(w, x, x, x, 2, MODULE_ENCS, batch_first=True, add_zero_attn=True, attn_mask=causal,
                            key_padding_mask=kpm, need_weights=False, softmax=O.core_softmax_rows)
    # The module divides by sqrt(32) on the device, where a division by a scalar may be a product with its
    # reciprocal; the oracle divides. On this data both land on the same step of div's grid everywhere.
    y = O.qdq(O._gemm(x.reshape(-1, 64), w["linear_Q.weight"].T) + w["linear_Q.bias"], MODULE_ENCS["linear_Q"])
    s = np.float32(32.0 ** 0.5)
    assert np.array_equal(O.qdq(y / s, MODULE_ENCS["div"]), O.qdq(y * (np.float32(1) / s), MODULE_ENCS["div"]))
    assert np.isfinite(want).all() and len(np.unique(want)) > 32

    m = T.QuantizableMultiheadAttention(64, 2, add_bias_kv=True, add_zero_attn=True, batch_first=True)
    with torch.no_grad():
        for name, value in w.items():
            m.get_parameter(name).copy_(torch.from_numpy(value))
    xd = torch.from_numpy(x).to(DEV)
    sim = QuantizationSimModel(m.to(DEV).eval(), dummy_input=(xd, xd, xd), quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)
    attn = sim.model
    for name in MODULE_ENCS:
        if name == "weight":
            continue
        wrapper = getattr(attn, name)
        wrapper.enable_input_quantizers(False)
        wrapper.output_quantizers[0].encoding = tf_encoding(MODULE_ENCS[name])
        if "weight" in wrapper.param_quantizers:
            wrapper.param_quantizers["weight"].encoding = tf_encoding(MODULE_ENCS["weight"])
        wrapper.set_mode(QcQuantizeOpMode.ACTIVE)
    attn.fused_core = True
    was = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        soft, core = T.attn_launch_count(), T.attn_core_launch_count()
        with torch.no_grad():
            got, weights = attn(xd, xd, xd, key_padding_mask=torch.from_numpy(kpm).to(DEV),
                                attn_mask=torch.from_numpy(causal).to(DEV), need_weights=False)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = was
    assert weights is None
    assert (T.attn_launch_count() - soft, T.attn_core_launch_count() - core) == (0, 1)
    assert_same_bits(got.cpu().numpy(), want, "QuantizableMultiheadAttention(64, 2), fused_core")
