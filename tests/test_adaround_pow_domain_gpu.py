"""The AdaRound rounding loss's pow over every exponent the API accepts, in both pow forms and on
every route that hands the kernels an exponent, against a float64 reference (adaround_oracle.py:
the reference's float32 chain around a float64 power rounded once).

The bar: the kernel's dL/dalpha bits equal T(step(p_cr, k)) for a k in {-1, 0, +1}, every element
(the fast pow's error is below 0.5 ulp before its final rounding, Sleef's u10 bound is 1 ulp: both
forms land within 1 ulp of the correctly rounded value). The measured table of this sweep is
profiles/r20/adaround_pow_domain.txt; aimet_amd.adaround.FAST_POW_EXPONENTS is the interval on
which the default pow meets the bar, and outside it every public route takes the exact form
(host-side exponents: the launch picks it; device-resident ones: the optimizer, from beta_range's
two ends) or, below beta = 1 where neither form follows torch at |x| = 0, refuses."""
import ctypes

import numpy as np
import pytest
import torch

import adaround_oracle as AO
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

DEV = "cuda"
f32 = np.float32
REG = 0.01
N = 1 << 18

# e = beta - 1: the stated domain of the fast pow's exp_ln, (0, 64] ...
E_DOMAIN = [2.0 ** -10, 0.01, 0.25, 0.5, 0.999, 1.0, 1.001, 1.5, 2.0, 3.0, 6.25, 13.0, 19.0, 20.0, 24.0, 25.0, 30.0,
            40.5, 63.0, 64.0]
# ... and outside it (beta = 1, beta = 0 and beta < 0 among them)
E_OUTSIDE = [65.0, 100.0, 0.0, -0.5, -1.0, -3.0]
# the routes test: three exponents inside the proven interval, three outside, and e = 1
E_ROUTES = [0.5, 6.25, 19.0, 1.0, 40.5, 100.0, 0.0]

SPECIAL_ALPHAS = f32([np.nan, np.inf, -np.inf, 0.0, -0.0, 100.0, 100.5, 99.99, -100.0, -103.9, -104.0, -104.5, 88.7,
                      87.3, -88.7, 1e30, -1e30, 3e38, -3e38, 1e-30, -1e-30, 2.3, -2.3, 0.125])


def beta_of(e):
    return float(e) + 1.0


def sweep_alpha():
    """n = 2^18: dense over [-2.46, 2.46] (outside +-2.398 the clamp makes |x| exactly 1), 4096
    points in [-1e-3, 1e-3] (|x| down to 2^-24) and the special values, forwards and backwards"""
    a = np.linspace(-2.46, 2.46, N).astype(f32)
    s = SPECIAL_ALPHAS.size
    a[:s] = SPECIAL_ALPHAS
    a[64:64 + s] = SPECIAL_ALPHAS[::-1]
    a[4096:8192] = np.linspace(-1e-3, 1e-3, 4096).astype(f32)
    return a


def dense_alpha(n):
    """every alpha inside h's clamp: dense waves"""
    rng = np.random.default_rng(17)
    a = rng.uniform(-2.39, 2.39, n).astype(f32)
    m = min(n, 4096)
    a[:m] = np.linspace(-1e-3, 1e-3, m).astype(f32)
    return a


def sparse_alpha(n):
    """3 of every 4 quads at alpha = 60 (|x| exactly 1): sparse waves, compacted through LDS"""
    a = dense_alpha(n)
    keep = (np.arange(n) // 4) % 4 == 0
    return np.where(keep, a, f32(60.0)).astype(f32)


_chains = {}


def chain_of(name, alpha, C, K):
    """the float32 chain of one input layout, built once: its reconstruction part is torch CPU
    autograd of oracle/torch_ref.py: adaround_forward with a zero upstream gradient"""
    if name not in _chains:
        from oracle import torch_ref as T
        at = torch.from_numpy(alpha.reshape(C, K).copy()).requires_grad_(True)
        wq = T.adaround_forward(torch.zeros(C, K), at, torch.ones(C, 1), torch.zeros(C, 1), 8)
        (wq * torch.zeros(C, K)).sum().backward()
        _chains[name] = AO.Chain(alpha, at.grad.numpy().reshape(-1))
    return _chains[name]


def launch(alpha, C, K, beta, want_loss, route="host", misalign=False):
    """dL/dalpha (and the loss value) of one launch: w = 0, delta = 1, offset = 0, upstream
    gradient 0, so the result is the rounding loss's own gradient. route: the exponent from the
    host (aimet_adaround_backward), from device memory (aimet_adaround_backward_dev) or from the
    per-iteration table at it_next - 1 (aimet_adaround_backward_adam; returns the updated alpha
    and the Adam state it started from as well)."""
    from aimet_amd import _native
    n = C * K
    pad = 1 if misalign else 0   # a base off by one float: the one-element-per-lane kernel

    def dev(v):
        buf = torch.zeros(n + pad, device=DEV)
        buf[pad:].copy_(torch.as_tensor(v))
        return buf[pad:]
    a, w, g, ga = dev(alpha), dev(np.zeros(n, f32)), dev(np.zeros(n, f32)), dev(np.zeros(n, f32))
    d, o = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    loss = torch.zeros(1, device=DEV)
    lp = loss.data_ptr() if want_loss else None
    s = torch.cuda.current_stream().cuda_stream
    row = [REG, beta, beta - 1.0]
    if route == "host":
        _native.call("aimet_adaround_backward", w.data_ptr(), a.data_ptr(), g.data_ptr(), ga.data_ptr(), 1, C, K,
                     d.data_ptr(), o.data_ptr(), 8, ctypes.c_double(REG), ctypes.c_double(beta), lp, s)
    elif route == "dev":
        rb = torch.tensor(row, dtype=torch.float64).to(torch.float32).to(DEV)
        _native.call("aimet_adaround_backward_dev", w.data_ptr(), a.data_ptr(), g.data_ptr(), ga.data_ptr(), 1, C, K,
                     d.data_ptr(), o.data_ptr(), 8, rb.data_ptr(), lp, s)
    else:
        # rows 0, 1 and 3 hold another schedule's values: only row it_next - 1 = 2 may be read
        other = [0.5, 4.0, 3.0]
        rb = torch.tensor([other, other, row, other], dtype=torch.float64).to(torch.float32).to(DEV)
        ctr = torch.tensor([2, 3], dtype=torch.long, device=DEV)   # {it_cur, it_next}
        rng = np.random.default_rng(3)
        m0, v0 = (rng.standard_normal(n) * 1e-3).astype(f32), (rng.random(n) * 1e-6).astype(f32)
        m, v = dev(m0), dev(v0)
        _native.call("aimet_adaround_backward_adam", w.data_ptr(), a.data_ptr(), g.data_ptr(), m.data_ptr(),
                     v.data_ptr(), 1, C, K, d.data_ptr(), o.data_ptr(), 8, rb.data_ptr(), ctr.data_ptr() + 8,
                     ctr.data_ptr(), ctypes.c_double(1e-3), ctypes.c_double(0.9), ctypes.c_double(0.999),
                     ctypes.c_double(1e-8), lp, None, s)
        torch.cuda.synchronize()
        assert ctr.tolist() == [3, 3]
        return a.cpu().numpy(), float(loss.item()), (m0, v0)
    torch.cuda.synchronize()
    return ga.cpu().numpy(), float(loss.item()), None


def _refused(beta):
    return beta < 1.0   # a negative exponent for the gradient: ValueError on every public route


def _steps(name, alpha, C, K, got, beta):
    k = AO.pow_steps(chain_of(name, alpha, C, K), got, REG, beta)
    return int(k.max()), int((k == 1).sum()), int((k > 1).sum())


@pytest.mark.parametrize("e", E_DOMAIN + E_OUTSIDE, ids=lambda e: "e=%g" % e)
def test_adaround_pow_sweep_vs_float64(e, exact_pow):
    """Every exponent of the list, either pow form selected, through the host-side route: 2^18
    alphas (sweep_alpha) against the float64 reference, the bar above on every element; the loss
    value on the dense layout against the float64 sum, rtol 1e-5 (the project's bar for it). Below
    beta = 1 the launch refuses (ValueError) in either form; outside FAST_POW_EXPONENTS the launch
    takes the exact form whatever is selected, so the bar holds there too."""
    beta = beta_of(e)
    alpha = sweep_alpha()
    if _refused(beta):
        with pytest.raises(ValueError, match="beta_range"):
            launch(alpha, 1, N, beta, False)
        return
    got, _, _ = launch(alpha, 1, N, beta, False)
    worst, ones, beyond = _steps("sweep", alpha, 1, N, got, beta)
    print("e = %g (%s pow): max |k| = %d, %d elements at |k| = 1" % (e, "exact" if exact_pow else "fast", worst, ones))
    assert worst <= 1, (e, worst, beyond)
    da = dense_alpha(N)
    got_l, loss, _ = launch(da, 1, N, beta, True)
    assert _steps("dense", da, 1, N, got_l, beta)[0] <= 1
    want = AO.round_loss_f64(chain_of("dense", da, 1, N), REG, beta)
    print("    loss %.9g, float64 %.9g" % (loss, want))
    assert abs(loss - want) <= 1e-5 * abs(want), (e, loss, want)


def _torch_cpu_adam(alpha, grad, m0, v0):
    """one step of torch.optim.Adam on the CPU from the given state (two steps taken before)"""
    p = torch.nn.Parameter(torch.from_numpy(alpha.copy()))
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    p.grad = torch.from_numpy(grad.copy())
    opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": torch.from_numpy(m0.copy()),
                    "exp_avg_sq": torch.from_numpy(v0.copy())}
    opt.step()
    return p.detach()


LAYOUTS = [   # name, alpha builder, C, K, a base off by one float
    ("dense", dense_alpha, 1, N, False),                # the vector kernel, dense waves
    ("sparse", sparse_alpha, 1, N, False),              # the vector kernel, waves compacted through LDS
    ("tail16", dense_alpha, 1, N + 16, False),          # n = 16 (mod 32): the exact form's scalar tail
    ("ragged", dense_alpha, 3, 1001, False),            # K % 4 != 0 and C > 1: one element per lane
    ("dense", dense_alpha, 1, N, True),                 # the same through a misaligned base
]


@pytest.mark.parametrize("e", E_ROUTES, ids=lambda e: "e=%g" % e)
def test_adaround_pow_routes_vs_float64(e, exact_pow):
    """The same bar on every route that hands the kernels an exponent -- from the host, from device
    memory, from the per-iteration table at it_next - 1 inside the fused Adam step -- on dense and
    sparse waves, a scalar pow tail, the one-element-per-lane kernel, with and without the loss
    value. The device-resident routes cannot pick the pow's form: as their precondition states
    (aimet_amd.h), the exact pow is selected for an exponent outside FAST_POW_EXPONENTS, the way
    AdaroundOptimizer does. The Adam step's updated alpha against torch's CPU Adam on the
    reference gradient, to test_adaround_fused_step_graph_equals_torch_adam_graph's tolerance."""
    from aimet_amd.adaround import fast_pow_covers, set_exact_pow
    beta = beta_of(e)
    for name, build, C, K, misalign in LAYOUTS:
        alpha = build(C * K)
        key = "%s%d" % (name, C * K)
        ch = chain_of(key, alpha, C, K)
        want_loss = AO.round_loss_f64(ch, REG, beta)
        p_cr = AO.pow_cr(ch.ax, f32(beta - 1.0))[0]
        grad_ref = ch.T(p_cr, REG, beta)
        for route in (("host",) if misalign else ("host", "dev", "adam")):
            prev = set_exact_pow(True) if route != "host" and not fast_pow_covers(beta) else None
            try:
                res = {wl: launch(alpha, C, K, beta, wl, route, misalign) for wl in (False, True)}
            finally:
                if prev is not None:
                    set_exact_pow(prev)
            for wl, (got, loss, adam) in res.items():
                what = (e, key, route, wl, misalign)
                if route == "adam":
                    torch.testing.assert_close(torch.from_numpy(got), _torch_cpu_adam(alpha, grad_ref, *adam),
                                               rtol=1e-5, atol=1e-6, msg=lambda m: "%s: %s" % (what, m))
                else:
                    worst, _, beyond = _steps(key, alpha, C, K, got, beta)
                    assert worst <= 1, (what, worst, beyond)
                if wl and name != "sparse":
                    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (what, loss, want_loss)
            if route != "adam":   # the loss value requested or not: the same gradient bits
                assert np.array_equal(res[False][0].view(np.int32), res[True][0].view(np.int32)), (e, key, route)


@pytest.mark.parametrize("route", ["dev", "adam"])
def test_adaround_pow_device_routes_fast_form_on_its_interval(route):
    """The device-resident routes with the default pow at both ends of FAST_POW_EXPONENTS (the
    largest and smallest beta their precondition admits) and at beta = 1."""
    from aimet_amd.adaround import FAST_POW_EXPONENTS, fast_pow_covers, get_exact_pow
    assert not get_exact_pow()
    alpha = dense_alpha(N)
    for beta in (1.0 + FAST_POW_EXPONENTS[0], FAST_POW_EXPONENTS[1], 1.0):
        assert fast_pow_covers(beta)
        got, _, adam = launch(alpha, 1, N, beta, False, route)
        if route == "adam":
            ch = chain_of("dense%d" % N, alpha, 1, N)
            ref = _torch_cpu_adam(alpha, ch.T(AO.pow_cr(ch.ax, f32(beta - 1.0))[0], REG, beta), *adam)
            torch.testing.assert_close(torch.from_numpy(got), ref, rtol=1e-5, atol=1e-6)
        else:
            assert _steps("dense%d" % N, alpha, 1, N, got, beta)[0] <= 1, beta


def test_adaround_beta_predicates():
    """fast_pow_covers / exact_pow_needed: the default schedule is covered, ends outside
    FAST_POW_EXPONENTS need the exact pow, an end below 1 is refused naming beta_range."""
    from aimet_amd.adaround import FAST_POW_EXPONENTS, exact_pow_needed, fast_pow_covers
    lo, hi = FAST_POW_EXPONENTS
    assert all(fast_pow_covers(b) for b in (20, 2, 1, 1 + lo, hi, 3.5))
    assert not any(fast_pow_covers(b) for b in (1 + lo / 2, float(np.nextafter(f32(hi), f32(100))), 65, 101))
    assert not exact_pow_needed((20, 2)) and not exact_pow_needed((2, 20)) and not exact_pow_needed((1, 1))
    assert exact_pow_needed((30, 1)) and exact_pow_needed((66, 2)) and exact_pow_needed((101, 101))
    for bad in ((30, 0.5), (20, 0), (20, -2), (float("nan"), 2), (float("inf"), 2)):
        with pytest.raises(ValueError, match="beta_range"):
            exact_pow_needed(bad)


def _small_conv():
    torch.manual_seed(6)
    conv = torch.nn.Conv2d(8, 12, 3, padding=1).to(DEV)
    inp = torch.randn(64, 8, 8, 8, device=DEV)
    with torch.no_grad():
        out = conv(inp) + 0.01 * torch.randn(64, 12, 8, 8, device=DEV)
    w = conv.weight.detach()
    d = (w.abs().amax(dim=(1, 2, 3)) / 127).contiguous()
    o = torch.full((12,), -128.0, device=DEV)
    return conv, inp, out, d, o


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_adaround_loop_beta_range_guard(use_graph, caplog, monkeypatch):
    """AdaroundOptimizer.optimize_rounding on one small conv layer: the default (20, 2) schedule
    runs with the fast pow (get_exact_pow() False before, inside and after the loop); a beta_range leaving FAST_POW_EXPONENTS -- (30, 1) -- runs the
    loop with the exact pow (bit-equal to the loop with the exact pow selected by hand), says so
    in the log and restores the flag; (30, 0.5), whose end lies below 1, raises ValueError naming
    beta_range before anything is launched."""
    import logging
    from aimet_amd.adaround import get_exact_pow, set_exact_pow
    from aimet_amd.adaround_optimizer import AdaroundHyperParameters, AdaroundOptimizer
    conv, inp, out, d, o = _small_conv()

    def run(beta_range):
        p = AdaroundHyperParameters(num_iterations=40, warm_start=0.25, beta_range=beta_range)
        return AdaroundOptimizer.optimize_rounding(conv, inp, out, d, o, 8, 0, p, torch.nn.ReLU(),
                                                   torch.Generator().manual_seed(2),
                                                   use_graph=use_graph).detach().clone()
    assert not get_exact_pow()
    seen = []
    real = AdaroundOptimizer._optimize_rounding_loop
    monkeypatch.setattr(AdaroundOptimizer, "_optimize_rounding_loop",
                        staticmethod(lambda *a: (seen.append(get_exact_pow()), real(*a))[1]))
    run((20, 2))
    assert seen == [False] and not get_exact_pow()
    AdaroundOptimizer._exact_pow_logged.clear()
    with caplog.at_level(logging.WARNING, logger="aimet_amd.adaround"):
        guarded = run((30, 1))
        run((30, 1))
    assert seen == [False, True, True] and not get_exact_pow()
    assert sum("beta_range" in r.getMessage() for r in caplog.records) == 1   # said once
    prev = set_exact_pow(True)
    try:
        by_hand = run((30, 1))
    finally:
        set_exact_pow(prev)
    if use_graph:   # the captured loop is bit-reproducible
        assert torch.equal(guarded, by_hand)
    else:
        torch.testing.assert_close(guarded, by_hand, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError, match="beta_range"):
        run((30, 0.5))
    assert len(seen) == 4 and not get_exact_pow()


@pytest.mark.parametrize("bw", [2, 3, 16])
def test_adaround_bit_widths_vs_torch_cpu(bw):
    """Forward (soft and hard rounding) and the reconstruction gradient at bit widths the other
    tests do not run, one [4, 256] case, weights at multiples of delta and one ulp beside them,
    across and past the grid's two ends: bit-equal to oracle/torch_ref.py on the CPU."""
    from aimet_amd.adaround import AdaroundFunction
    from oracle import torch_ref as T
    rng = np.random.default_rng(100 + bw)
    C, K = 4, 256
    half = 1 << (bw - 1)
    delta = f32([0.01, 0.0037, 0.25, 1e-3])
    off = f32([-half, -half + 1, 0.0, -(half // 2)])
    span = half + 4 if bw < 16 else 2 * half + 40
    k = rng.integers(-span, span + 1, (C, K)).astype(f32)
    k[:, :8] = f32([-half - 1, -half, -half + 1, -1, 0, half - 2, half - 1, half])
    w = (k * delta[:, None]).astype(f32)
    w[:, 1::3] = np.nextafter(w[:, 1::3], f32(np.inf))
    w[:, 2::3] = np.nextafter(w[:, 2::3], f32(-np.inf))
    a = (rng.standard_normal((C, K)) * 3).astype(f32)
    g = rng.standard_normal((C, K)).astype(f32)
    wt, dt, ot = torch.from_numpy(w), torch.from_numpy(delta).view(C, 1), torch.from_numpy(off).view(C, 1)
    at = torch.from_numpy(a.copy()).requires_grad_(True)
    soft_ref = T.adaround_forward(wt, at, dt, ot, bw)
    (soft_ref * torch.from_numpy(g)).sum().backward()
    hard_ref = (torch.clamp(torch.floor(wt / dt) + (at.detach() >= 0).float() - ot, 0, 2 ** bw - 1) + ot) * dt
    wd, dd, od, gd = (torch.from_numpy(v).to(DEV) for v in (w, delta, off, g))
    ad = torch.from_numpy(a).to(DEV).requires_grad_(True)
    soft = AdaroundFunction.apply(wd, ad, dd, od, bw, 0)
    (soft * gd).sum().backward()
    with torch.no_grad():
        hard = AdaroundFunction.apply(wd, ad, dd, od, bw, 0, False)
    for got, want in ((soft.detach(), soft_ref.detach()), (hard, hard_ref), (ad.grad, at.grad)):
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.numpy().view(np.int32)), bw
    assert int((soft_ref.detach() != hard_ref).sum()) > 0 and float(at.grad.abs().max()) > 0
