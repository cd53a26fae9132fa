"""aimet_attn_softmax_lg(_backward) and QuantizableMultiheadAttention's range-learning fused route, on the
inputs of test_mha_backward_gpu.py. Forward: bit for bit the mha_oracle restatement with both QDQs replaced
by calculate_forward_pass in numpy float32 (correctly rounded x / delta, rint = half to even, clamp).
Backward: the literal chain in float64 (the float32 grid value of the score feeds the softmax, as in
test_mha_backward_gpu.py; asymmetric_gradients / symmetric_gradients restated in numpy float64).
  dx: |dx - dx64| <= 2^-16 max|g|, the bound and derivation of that file (in-grid masks replace its
    range tests; the reference asserts that neither mask is ambiguous: no raw-score quotient within
    2^-18 and no probability quotient at a clip end within 2^-10 of a half-integer).
  range gradients: a sum of terms T_j = ((xq_j + o) - m_j q_j) g_j (and D = the sum of g_j outside the
    grid). In float32 the quotient of a probability inherits the probability's 26 ulp (that file), the
    subtraction and the product add 2 and a sum of depth k adds k: at most (28 + k) 2^-24 M with
    M = sum_j (|xq_j + o| + |m_j q_j|) |g_j|, the operands before they cancel. k: a lane adds at most 17
    elements of one row, then 6 butterfly steps, 3 waves, the fold's lane sum of ceil(partials / 256) and
    its 9 steps: k = 64 covers the small cases, k = 400 the 65536 partials of the second-trip case. The
    score quantizer's gradient t_j = (G_j - d) p_j carries an error itself: d at most 49 ulp of max|g| (p's
    26, depth 22, a product), G_j - d two more, p_j its 26 ulp on |G_j - d| <= 2 max|g|, the product one:
    105 2^-24 max|g| p_j <= 2^-17 max|g| p_j an element (the dx bound, its factor p_j kept), times |T_j / g_j|
    (or 1 in D). A probability whose float64 quotient lies within 2^-10 of a half-integer ("ambiguous") may
    land one level away in float32 and then moves a sum by at most |g_j|; the reference asserts that these are
    at most 1 % of the elements (D moves only where an element changes sides at a clip end: asserted away).
    The bounds go through range_grads_one's factors, plus 8 ulp of the operands of its last subtraction."""
import functools

import numpy as np
import pytest
import torch

import mha_oracle as O
from aimet_amd import transformers as T
from aimet_amd.elementwise_ops import TRANSFORMER_QUANTIZABLE_TYPES
from aimet_amd.learned_grid import get_computed_encodings
from aimet_amd.quantizers import QuantScheme
from aimet_amd.quantsim import QuantizationSimModel
from test_mha_backward_gpu import B, H, L, SENTINEL, data, gpu

DEV, F, D = "cuda", np.float32, np.float64
FLAGS = {False: (False, False, False), True: (True, False, False)}   # sym -> use_symmetric, strict, unsigned
CASES = [(S, sym, masked, "both") for S in (1, 2, 5, 63, 64, 65, 129, 257, 1024, 1025, 1030) for sym in (False, True)
         for masked in (False, True)] + [(65, False, True, "score"), (65, True, True, "prob"),
                                         (1025, True, False, "score"), (1025, False, True, "prob")]


def ranges(S, sym, which="both"):
    """(score range, prob range), None for a missing quantizer. Symmetric scores end at 7.1 too, but for S = 1030,
    where that puts a quotient of these scores within 2^-18 of a half-integer: 7.05 there (reference alone)."""
    top = F(7.05 if sym and S == 1030 else 7.1)
    rngs = (-top, top) if sym else (F(-6.3), top), (F(0.0), F(data(S)[3][1]))
    return tuple(r if which in ("both", w) else None for r, w in zip(rngs, ("score", "prob")))


def effective(S):
    return data(S)[1] | np.repeat(data(S)[4], H, axis=0)[:, None, :]


def encoding32(rng, flags):
    """get_computed_encodings in float32, 8 bits, flags (use_symmetric, strict, unsigned) -> (delta, offset, steps)."""
    (mn, mx), (sym, strict, unsigned) = rng, flags
    steps = F(254 if sym and strict else 255)
    if sym and not unsigned:
        return mx / F(np.floor(steps / 2)), F(-np.ceil(steps / 2)), steps
    d = (mx - mn) / steps
    return d, (mn / d if sym else -np.minimum(steps, np.maximum(F(0), np.rint(-mn / d)))), steps


def qdq32(x, enc):
    """calculate_forward_pass in float32."""
    d, o, steps = enc
    with np.errstate(invalid="ignore"):
        return ((np.clip(np.rint(np.asarray(x, F) / d) - o, F(0), steps) + o) * d).astype(F)


def forward32(S, sym, masked, which="both"):
    srng, prng = ranges(S, sym, which)
    x = qdq32(data(S)[0], encoding32(srng, FLAGS[sym])) if srng else data(S)[0]
    if masked:
        x = np.where(effective(S), F(-np.inf), x)
    p = O.softmax_rows(x.reshape(-1, S)).reshape(x.shape)
    return qdq32(p, encoding32(prng, FLAGS[sym])) if prng else p


def quant64(x, rng, flags):
    """One quantizer in float64 on the float32 encoding: (xq + o, in-grid mask, quotient, the encoding)."""
    d, o, steps = (D(v) for v in encoding32(rng, flags))
    q = x / d
    xq = np.clip(np.rint(q) - o, 0.0, steps)
    return xq + o, xq == np.rint(q) - o, q, (d, o, steps, D(rng[0]), D(rng[1]))


def range_grads64(xqo, m, q, g, enc, sym, amb, dg, depth, times):
    """asymmetric_ / symmetric_gradients in float64, row r counted times[r] times -> [(gradient, bound)] * 2."""
    d, _, steps, mn, mx = enc
    eps = (28 + depth) * 2.0 ** -24
    g, dg = g * times, dg * times
    gss = ((xqo - m * q) * g).sum()
    tol_a = eps * ((np.abs(xqo) + np.abs(m * q)) * np.abs(g)).sum() + np.abs(g * amb).sum() + \
        (dg * np.abs(xqo - m * q)).sum()
    if sym:
        half = np.floor(steps / 2)
        return [(-gss / half, tol_a / half), (gss / half, tol_a / half)]
    out = g * ~m
    tol_d = eps * np.abs(out).sum() + (dg * ~m).sum()   # no ambiguous element changes sides: chain64 asserts it
    term1, term2, f = gss / steps, steps / (mx - mn) ** 2 * (d * out.sum()), steps / (mx - mn) ** 2 * d
    return [(-term1 + mx * term2, tol_a / steps + abs(mx) * f * tol_d + 2.0 ** -21 * (abs(term1) + abs(mx * term2))),
            (term1 - mn * term2, tol_a / steps + abs(mn) * f * tol_d + 2.0 ** -21 * (abs(term1) + abs(mn * term2)))]


def chain64(scores, g, eff, srng, prng, flags, depth, times=1.0):
    """The literal chain on [..., S] rows, row r counted times[r] times in the sums; flags = (the score grid's,
    the prob grid's), a range None where there is no quantizer -> (dx, the positions that must be exactly zero,
    [(gradient, bound) or None] for score min, score max, prob min, prob max)."""
    x, g64 = scores.astype(D), g.astype(D)
    xv, s_m = x.copy(), np.ones(x.shape, bool)
    if srng:
        s_xqo, s_m, s_q, s_enc = quant64(x, srng, flags[0])
        assert np.abs(s_q - np.floor(s_q) - 0.5).min() > 2.0 ** -18   # the score mask and level are unambiguous
        xv = qdq32(scores, encoding32(srng, flags[0])).astype(D)
    xv[eff] = -np.inf
    e = np.exp(xv - xv.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    G, grads = g64, [None, None]
    if prng:
        p_xqo, p_m, p_q, (d, o, steps, mn, mx) = quant64(p, prng, flags[1])
        amb = np.abs(p_q - np.floor(p_q) - 0.5) < 2.0 ** -10
        ends = np.minimum(np.abs(p_q - (steps + o + 0.5)), np.abs(p_q - (o - 0.5)))
        assert amb.mean() <= 0.01 and ends.min() > 2.0 ** -10          # nor is the probability mask
        G, grads = p_m * g64, range_grads64(p_xqo, p_m, p_q, g64, (d, o, steps, mn, mx), flags[1][0], amb, 0.0, depth,
                                            times)
    t = (G - (G * p).sum(axis=-1, keepdims=True)) * p
    t[eff] = 0.0
    if srng:
        grads = range_grads64(s_xqo, s_m, s_q, t, s_enc, flags[0][0], False, 2.0 ** -17 * np.abs(g).max() * p, depth,
                              times) + grads
    return s_m * t, eff | ~s_m, ([None, None] + grads)[-4:]


@functools.lru_cache(None)
def reference(S, sym, masked, which):
    return chain64(data(S)[0], data(S)[2], effective(S) & masked, *ranges(S, sym, which), (FLAGS[sym],) * 2, 64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def grids(S, sym, which="both"):
    return tuple(r and (dev(np.array([r[0]])), dev(np.array([r[1]])), 8) + FLAGS[sym] for r in ranges(S, sym, which))


def check_backward(dx, grads, want, gmax):
    (want_dx, zero, want_grads), dx, grads = want, dx.cpu().numpy(), grads.cpu().numpy().reshape(-1)
    assert np.all(dx[zero] == 0)   # bitwise +0 or -0, never NaN
    err = float(np.abs(dx - want_dx).max())
    print("max |dx - dx64| = %.3g of the bound %.3g" % (err, 2.0 ** -16 * gmax))
    assert err <= 2.0 ** -16 * gmax
    check_grads(("score min", "score max", "prob min", "prob max"), grads, want_grads)


def check_grads(names, got, want, sharp=False):
    """sharp: the bound is also under a third of the value, so a negated, swapped or halved sum fails."""
    for name, value, (ref, bound) in ((n, v, w) for n, v, w in zip(names, got, want) if w):
        print("%s: %.9g, float64 %.9g +- %.3g, |difference| %.3g" % (name, value, ref, bound, abs(value - ref)))
        assert abs(value - ref) <= bound and (not sharp or 3 * bound <= abs(ref)), name


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@gpu
@pytest.mark.parametrize("S,sym,masked,which", CASES)
def test_kernels_against_the_restatement_and_the_float64_chain(S, sym, masked, which):
    scores, mask, g, _, kpm = data(S)
    (sg, pg), masks = grids(S, sym, which), ((dev(mask), dev(kpm)) if masked else (None, None))
    x, n = dev(scores), T.attn_lg_launch_count()
    probs, saved = T.attn_softmax_lg(x, B, H, *masks, sg, pg)
    assert np.array_equal(O.bits(probs.cpu().numpy()), O.bits(forward32(S, sym, masked, which)))
    for row, (lo, hi) in ((row, grid[:2]) for row, grid in zip(saved, (sg, pg)) if grid):
        delta, offset, _ = get_computed_encodings(8, lo, hi, *FLAGS[sym])
        assert torch.equal(row, torch.cat([delta, offset, lo, hi]))
    gd = dev(g)
    dx, grads = T.attn_softmax_lg_backward(x, gd, B, H, *masks, sg, pg, saved)
    check_backward(dx, grads, reference(S, sym, masked, which), float(np.abs(g).max()))
    again, grads2 = T.attn_softmax_lg_backward(x, gd, B, H, *masks, sg, pg, saved, out=gd)   # in place: the same bits
    rows = [i for i, grid in enumerate((sg, pg)) if grid]   # a row without a quantizer is not written
    assert again.data_ptr() == gd.data_ptr() and same_bits(again, dx) and same_bits(grads2[rows], grads[rows])
    assert T.attn_lg_launch_count() == (n[0] + 1, n[1] + 2)


@gpu
def test_out_of_place_and_the_refusal():
    (sg, pg), x, saved = grids(65, False), dev(data(65)[0]), torch.zeros(2, 4, device=DEV)
    with pytest.raises(ValueError, match="out of place"):
        T.attn_softmax_lg(x, B, H, score_grid=sg, out=x)
    S, n = T.attn_softmax_max_s() + 1, T.attn_lg_launch_count()
    out, zeros = torch.full((1, 1, S), SENTINEL, device=DEV), torch.zeros(1, 1, S, device=DEV)
    with pytest.raises(ValueError, match="not resident"):
        T.attn_softmax_lg(zeros, 1, 1, score_grid=sg, prob_grid=pg, out=out)
    with pytest.raises(ValueError, match="not resident"):
        T.attn_softmax_lg_backward(zeros, zeros, 1, 1, score_grid=sg, prob_grid=pg, saved=saved, out=out)
    assert T.attn_lg_launch_count() == n and bool((out == SENTINEL).all())


@gpu
@pytest.mark.parametrize("S,stride", [(2, 4 * 65536), (1025, 65536)], ids=["wave", "lds"])
def test_rows_of_the_second_grid_stride_trip(S, stride):
    """Past the cap of 65536 workgroups of four rows (wave) or one (LDS); a second run gives the same bits."""
    rows, (scores, _, g) = stride + (8 if S == 2 else 2), data(S)[:3]
    tile = np.arange(rows) % (B * H * L)
    assert rows % (B * H) == 0 and stride % (B * H * L) != 0
    flat = lambda a: a.reshape(-1, S)  # noqa: E731
    want_dx, zero, want_grads = chain64(flat(scores), flat(g), flat(effective(S)), *ranges(S, False),
                                        (FLAGS[False],) * 2, 400, np.bincount(tile)[:, None].astype(D))
    sg, pg = grids(S, False)
    x, am, gd = (dev(flat(a)[tile].reshape(B * H, -1, S)) for a in (scores, effective(S), g))
    probs, saved = T.attn_softmax_lg(x, B, H, am, None, sg, pg)
    pick = np.r_[0:5, stride - 3:rows]
    idx = torch.from_numpy(pick).to(DEV)
    assert np.array_equal(O.bits(probs.view(-1, S)[idx].cpu().numpy()),
                          O.bits(flat(forward32(S, False, True))[tile[pick]]))
    dx, grads = T.attn_softmax_lg_backward(x, gd, B, H, am, None, sg, pg, saved)
    check_backward(dx.view(-1, S)[idx], grads, (want_dx[tile[pick]], zero[tile[pick]], want_grads),
                   float(np.abs(g).max()))
    dx2, grads2 = T.attn_softmax_lg_backward(x, gd, B, H, am, None, sg, pg, saved)
    assert same_bits(dx2, dx) and same_bits(grads2, grads)


@gpu
def test_module_trains_through_one_launch_each_way():
    """With the opt-in one forward and one backward launch a block; without it none. Output and input gradient of
    the routes within 1e-3 of the largest value, as test_mha_backward_gpu.py's module test. The four range
    gradients of each block ON EITHER ROUTE against chain64 on the block's own raw scores, masks, ranges and
    gradient at the probabilities, taken from the literal run: the kernel tests' bounds and conditions (8 bits)."""
    torch.manual_seed(5)
    was, torch.backends.cuda.matmul.allow_tf32 = torch.backends.cuda.matmul.allow_tf32, False
    layer = torch.nn.TransformerEncoderLayer(16, 4, 32, dropout=0.0, batch_first=True)
    model = torch.nn.TransformerEncoder(layer, 2).to(DEV).eval()
    T.get_quantizable_pt_transformer_model(model)
    x = torch.randn(3, 5, 16, device=DEV)
    kpm = torch.tensor([[False] * 5, [False, False, False, True, True], [False, True, False, False, False]], device=DEV)
    sim = QuantizationSimModel(model, dummy_input=x, quant_scheme=QuantScheme.training_range_learning_with_tf_init,
                               quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)
    sim.compute_encodings(lambda m, _: m(x, src_key_padding_mask=kpm))
    blocks = [m for m in sim.model.modules() if isinstance(m, T.QuantizableMultiheadAttention)]
    wrappers = [getattr(b, w) for b in blocks for w in ("matmul_1", "softmax")]
    weight = torch.randn(3, 5, 16, device=DEV)
    results, launches, seen = {}, {}, []

    def keep(_module, inputs, output):   # literal run, a block: MatMul's raw scores, then softmax's input and output
        output.retain_grad()
        seen.append((inputs[0], output))
    for route, opt_in in {"literal": False, "fused": True}.items():
        assert T.set_fused_attention_backward(sim.model, opt_in) == 2
        hooks = [m.register_forward_hook(keep) for b in blocks for m in (b.matmul_1._module_to_wrap, b.softmax)
                 if not opt_in]
        xg = x.clone().requires_grad_(True)
        sim.model.zero_grad()
        n = T.attn_lg_launch_count()
        out = sim.model(xg, src_key_padding_mask=kpm)
        (out * weight).sum().backward()
        launches[route] = tuple(a - b for a, b in zip(T.attn_lg_launch_count(), n))
        [h.remove() for h in hooks]
        results[route] = (out.detach(), xg.grad, [float(getattr(w, "output0_encoding_" + e).grad) for w in wrappers
                                                  for e in ("min", "max")])
    torch.backends.cuda.matmul.allow_tf32 = was
    assert launches == {"literal": (0, 0), "fused": (2, 2)} and len(seen) == 4
    for got, want in zip(results["fused"][:2], results["literal"][:2]):
        assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max())
    for i in range(2):
        pair = wrappers[2 * i:2 * i + 2]
        qs = [w.output_quantizers[0] for w in pair]
        assert all(q.bitwidth == 8 for q in qs)
        rngs = [tuple(F(getattr(w, "output0_encoding_" + e).item()) for e in ("min", "max")) for w in pair]
        flags = [(q.use_symmetric_encodings, q.use_strict_symmetric, q.is_unsigned_symmetric) for q in qs]
        (_, raw), (masked, probs) = seen[2 * i:2 * i + 2]
        want = chain64(raw.detach().cpu().numpy(), probs.grad.cpu().numpy(), torch.isinf(masked).cpu().numpy(), *rngs,
                       flags, 64)[2]
        for route in results:
            names = ["%s, block %d, %s" % (route, i, k) for k in ("score min", "score max", "prob min", "prob max")]
            check_grads(names, results[route][2][4 * i:4 * i + 4], want, True)
