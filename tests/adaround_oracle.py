"""TEST INFRASTRUCTURE ONLY: the reference for the AdaRound rounding-loss gradient, element by
element, shared by test_adaround_golden.py and test_adaround_pow_domain_gpu.py.

dL/dalpha with the rounding loss is recon + T(p): p = |2h - 1|^(beta - 1), T the reference's
float32 autograd chain after the pow (pow_backward: grad * (beta * p); abs: * sgn(x); 2 * h: * 2;
clamp; * (zeta - gamma); sigmoid_backward), recon the reconstruction term's gradient. Nothing here
restates a pow implementation: p comes from a float64 power rounded once to float32 (pow_cr), and
a kernel is held to T(p') for a p' within one float32 step of it (pow_steps)."""
import numpy as np
import torch

f32 = np.float32
NO_K = 99   # pow_steps: no k in the searched range reproduces the result


def ulps(a, b):
    a = np.asarray(a, np.float32).ravel().view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).ravel().view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def f32_step(p, k):
    """p (float32 >= 0) moved by k ulps, clamped at +0"""
    b = p.view(np.int32).astype(np.int64) + k
    return np.maximum(b, 0).astype(np.int32).view(np.float32)


def vector_sigmoid(alpha):
    """torch's CPU sigmoid as its vectorized loop computes it, for every element: the scalar loop
    that torch runs on the last elements of a tensor -- and of each thread's share of one -- can
    differ from it by an ulp, so the tensor is padded to whole vectors and run on one thread. This
    is the sigmoid the kernels reproduce bit for bit (test_gpu_parity.py, test_adaround_golden.py)."""
    flat = np.ascontiguousarray(alpha, dtype=f32).reshape(-1)
    padded = np.zeros((flat.size + 127) // 64 * 64, f32)
    padded[:flat.size] = flat
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        sg = torch.sigmoid(torch.from_numpy(padded)).numpy()
    finally:
        torch.set_num_threads(nt)
    return sg[:flat.size].reshape(np.shape(alpha)).copy()


class Chain:
    """The float32 steps around the pow for one alpha tensor: sigmoid (vector_sigmoid, or the
    caller's), pre = sg * 1.2 + -0.1, h = clip(pre, 0, 1), x = 2 h + -1; then
    T(p) = recon + the loss term's gradient for a pow value p, every step one float32 operation."""

    def __init__(self, alpha, recon, sg=None):
        alpha = np.ascontiguousarray(alpha, dtype=f32)
        self.sg = vector_sigmoid(alpha) if sg is None else np.asarray(sg, f32).reshape(alpha.shape)
        pre = self.sg * f32(1.2) + f32(-0.1)
        self.h = np.clip(pre, f32(0), f32(1))
        self.in_h = (pre >= 0) & (pre <= 1)
        self.x = f32(2) * self.h + f32(-1)
        self.ax = np.abs(self.x)
        self.sgn = np.sign(self.x).astype(f32)
        self.recon = np.asarray(recon, f32).reshape(alpha.shape)

    def T(self, p, reg, beta):
        with np.errstate(all="ignore"):
            dpw = f32(-reg) * (f32(beta) * p)
            dh = (dpw * self.sgn) * f32(2)
            return self.recon + ((np.where(self.in_h, dh, f32(0)) * f32(1.2)) * (f32(1) - self.sg)) * self.sg


def pow_cr(ax, e):
    """|x|^e correctly rounded: float64 ax ** float64(float32(e)) rounded once to float32, with the
    exact cases of the power function as IEEE pow and torch define them (e == 0: 1; x == 1: 1;
    x == 0: 0 for e > 0 and inf for e < 0; NaN otherwise for a NaN x). Returns (p, alt, exact): alt is the
    neighbouring float32 where the float64 power lies within 2^-50 (relative) of the rounding
    boundary between the two -- the float64 pow's own error could then decide -- and p elsewhere.
    exact: where the power is one of those exact cases, which no pow may miss by any step."""
    e32 = f32(e)
    x64 = np.asarray(ax, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        p64 = np.power(x64, np.float64(e32))
        p = p64.astype(f32)
        alt = p.copy()
        fin = np.isfinite(p64) & (p64 > 0) & np.isfinite(p)
        for k in (-1, 1):
            q = f32_step(p, k)
            mid = 0.5 * (p.astype(np.float64) + q.astype(np.float64))
            near = fin & np.isfinite(q) & (np.abs(p64 - mid) <= 2.0 ** -50 * p64)
            alt = np.where(near, q, alt)
    exact = (e32 == 0) | (x64 == 0) | (x64 == 1) | np.isnan(x64)
    return p, alt, exact


def _same(a, b):
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def pow_steps(chain, got, reg, beta, e=None, kmax=8):
    """For every element the smallest |k|, k in [-kmax, kmax], for which T(step(p_cr, k)) has the
    bits of `got` (NaN for NaN), p_cr = pow_cr(|x|, e), e = float32(beta - 1) formed in double as
    ATen's pow_backward forms it; NO_K where none does (only k = 0 is tried at the power's exact
    cases). The bar for either pow form is max <= 1."""
    if e is None:
        e = f32(float(beta) - 1.0)
    got = np.asarray(got, f32).reshape(chain.ax.shape)
    p, alt, exact = pow_cr(chain.ax, e)
    best = np.full(got.shape, NO_K, np.int64)
    todo = np.ones(got.shape, bool)
    for k in sorted(range(-kmax, kmax + 1), key=abs):
        if not todo.any():
            break
        hit = np.zeros(got.shape, bool)
        for base in (p, alt):
            hit |= _same(chain.T(f32_step(base, k) if k else base, reg, beta), got)
        hit &= todo if k == 0 else todo & ~exact
        best[hit] = abs(k)
        todo &= ~hit
    return best


def round_loss_f64(chain, reg, beta):
    """reg * sum(1 - |x|^beta) in float64 over the chain's float32 |x| (NaN lanes excluded by the
    caller: a NaN alpha makes the whole loss NaN)"""
    with np.errstate(all="ignore"):
        p = np.power(chain.ax.astype(np.float64), np.float64(f32(beta)))
    return float(reg) * float(np.sum(1.0 - p))


def fast_pow_gradient_ok(c, reg, got):
    """The golden vectors' bar for the default pow (test_adaround_golden.py): for each element, the
    pow values within 3 ulp of the correctly rounded x^(beta - 1) whose T reproduces the golden
    dL/dalpha bit for bit are torch's pow (`pinned`: at least one must); the kernel's result must
    then be T(p') for a p' within 1 ulp of one of them -- the bar the fast pow is proven to
    (profiles/r20/adaround_pow_domain.txt), carried through the reference's own chain. A
    difference of 1 ulp in p can move dL/dalpha by more than 1 ulp of its value: the loss term
    and the reconstruction gradient cancel in part (tests/golden, case 6: up to 64 ulp)."""
    beta = float(c["beta"])
    ch = Chain(c["alpha"], c["ga_recon"], torch.sigmoid(torch.from_numpy(c["alpha"])).numpy())
    p_cr = np.power(ch.ax.astype(np.float64), np.float64(f32(beta - 1.0))).astype(f32)
    want = c["ga_total"].view(np.int32)
    got = got.view(np.int32)
    outs = {k: ch.T(f32_step(p_cr, k), reg, beta).view(np.int32) for k in range(-4, 5)}
    sleef = {k: outs[k] == want for k in range(-3, 4)}
    pinned = np.zeros(want.shape, bool)
    ok = np.zeros(want.shape, bool)
    for k, m in sleef.items():
        pinned |= m
        for d in (-1, 0, 1):
            ok |= m & (outs[k + d] == got)
    return ok, pinned
