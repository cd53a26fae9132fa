"""numpy restatement of what aimet_amd/csrc/dfq.hip computes, on arrays in module layout.

Every fp32 operation of the kernels is its own numpy float32 operation here, in the kernels' order:
np.sqrt and the float32 divide are correctly rounded, the cube root is np.cbrt in float64 rounded to
float32, nothing is contracted. The elementwise results (BN backward fold, CLS scales, weights and
biases, the weight part of the forward fold, HBF's first bias) are therefore the kernels' bits. The
sums (forward-fold bias, HBF's second bias) are order-dependent; they are added in the kernels' order
too (k_sum, block_sum), and `f64=True` evaluates them in float64, the yardstick the float32 sums are
held against.

`transposed` marks a ConvTranspose weight with groups == 1 (output channels on axis 1)."""
import numpy as np

F = np.float32


def _logical(w, transposed):
    """[cout][cin][k] view of a module-layout weight."""
    v = w.reshape(w.shape[0], w.shape[1], -1)
    return v.transpose(1, 0, 2) if transposed else v


def _module(v, shape, transposed):
    return np.ascontiguousarray(v.transpose(1, 0, 2) if transposed else v).reshape(shape)


def ulp_distance(a, b):
    """Largest distance in float32 steps between two arrays (equal NaN-ness required)."""
    a = np.asarray(a, F).ravel()
    b = np.asarray(b, F).ravel()
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    if a.size == 0:
        return 0

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-2 ** 31) - i, i)
    ok = ~np.isnan(a)
    return int(np.max(np.abs(key(a[ok]) - key(b[ok])), initial=0))


def k_sum(v, T):
    """Sum over the kernel taps as one lane does it: from zero, one tap after the other."""
    acc = np.zeros(v.shape[:2], T)
    for q in range(v.shape[2]):
        acc = acc + v[:, :, q].astype(T)
    return acc


def block_sum(terms):
    """Sum over the last axis as a 256-lane workgroup of dfq.hip does it: lane t adds the terms t,
    t + 256, ... in turn (from zero), then a tree halves the 256 partials seven times."""
    n = terms.shape[-1]
    lanes = np.zeros(terms.shape[:-1] + (256,), terms.dtype)
    for start in range(0, n, 256):
        chunk = terms[..., start:start + 256]
        lanes[..., :chunk.shape[-1]] = lanes[..., :chunk.shape[-1]] + chunk
    s = 128
    while s:
        lanes[..., :s] = lanes[..., :s] + lanes[..., s:2 * s]
        s //= 2
    return lanes[..., 0]


def bn_scale(gamma, var, eps):
    sigma = np.sqrt(var.astype(F) + F(eps))
    assert not np.any(sigma == 0)
    return gamma.astype(F) / sigma


def bn_fold_backward(w, b, gamma, beta, mu, var, eps, transposed=False):
    """conv -> bn: w[o] *= scale[o], b = beta - (mu - b) * scale."""
    scale = bn_scale(gamma, var, eps)
    v = _logical(w, transposed) * scale[:, None, None]
    return _module(v, w.shape, transposed), beta - (mu - b) * scale


def bn_fold_forward(w, b, gamma, beta, mu, var, eps, f64=False):
    """bn -> conv (Conv / Linear layout): the bias from the weight before scaling, then w[:, i] *= scale[i]."""
    scale = bn_scale(gamma, var, eps)
    v = _logical(w, False)
    T = np.float64 if f64 else F
    w2d = k_sum(v, T)
    t_beta = w2d * beta.astype(T)[None, :]
    t_mu = w2d * (mu * scale).astype(T)[None, :]
    bias = (block_sum(t_beta) - block_sum(t_mu)) + b.astype(T)
    # sum of |w[o,i,q] * beta[i]| + |w[o,i,q] * (mu * scale)[i]| + |b[o]|: the 2 * cin * k + 1 terms of the sum
    absw = np.abs(v).astype(np.float64).sum(2)
    terms = (absw * (np.abs(beta) + np.abs(mu * scale)).astype(np.float64)[None, :]).sum(1) + np.abs(b)
    return (v * scale[None, :, None]).reshape(w.shape), bias, terms


def sanitize(s):
    with np.errstate(all="ignore"):
        s = np.where(np.isnan(s) | (s == np.inf), F(1), s).astype(F)
        return np.where(s == 0, F(1), s).astype(F)


def _absmax_out(v):
    return np.max(np.abs(v), axis=(1, 2))


def _absmax_in(v):
    return np.max(np.abs(v), axis=(0, 2))


def cls_pair(w0, b0, w1, t0=False, t1=False):
    """-> s, w0', b0' (None stays None), w1'."""
    v0, v1 = _logical(w0, t0), _logical(w1, t1)
    with np.errstate(all="ignore"):
        r0, r1 = _absmax_out(v0), _absmax_in(v1)
        s = sanitize(r0 / np.sqrt(r0 * r1))
        rcp = F(1) / s
        n0 = v0 * rcp[:, None, None]
        n1 = v1 * s[None, :, None]
        nb = None if b0 is None else b0 * rcp
    return s, _module(n0, w0.shape, t0), nb, _module(n1, w1.shape, t1)


def cls_triple(w0, b0, w1, b1, w2, t0=False, t2=False):
    """-> s12, s23, w0', b0', w1', b1', w2'."""
    v0, v1, v2 = _logical(w0, t0), _logical(w1, False), _logical(w2, t2)
    with np.errstate(all="ignore"):
        r0, r1, r2 = _absmax_out(v0), _absmax_out(v1), _absmax_in(v2)
        p = (r0 * r1) * r2
        root = np.cbrt(p.astype(np.float64)).astype(F)
        s12, s23 = sanitize(r0 / root), sanitize(root / r2)
        rcp12, rcp23 = F(1) / s12, F(1) / s23
        n0 = v0 * rcp12[:, None, None]
        n1 = v1 * s12[:, None, None] * rcp23[:, None, None]
        n2 = v2 * s23[None, :, None]
        nb0 = None if b0 is None else b0 * rcp12
        nb1 = None if b1 is None else b1 * rcp23
    return s12, s23, _module(n0, w0.shape, t0), nb0, n1.reshape(w1.shape), nb1, _module(n2, w2.shape, t2)


def absorb(gamma, beta, s, relu):
    bq = beta / s
    if not relu:
        return bq
    return np.maximum(F(0), bq - F(3) * np.abs(gamma / s))


def bias_fold(gamma, beta, s, relu, b1, w2, b2, t2=False, f64=False):
    """-> b1', b2', sum of |terms| per output (for the summation bound)."""
    a = absorb(gamma, beta, s, relu)
    v = _logical(w2, t2)
    T = np.float64 if f64 else F
    w2d = k_sum(v, T)
    absw = np.abs(v).astype(np.float64).sum(2)       # the cin * k + 1 terms: |w2[o,c,q] * absorb[c]|, |b2[o]|
    if v.shape[1] == 1:
        corr, mag = w2d[:, 0] * a.astype(T), absw[:, 0] * np.abs(a)
    else:
        corr, mag = block_sum(w2d * a.astype(T)[None, :]), (absw * np.abs(a).astype(np.float64)[None, :]).sum(1)
    return b1 - a, b2.astype(T) + corr, mag + np.abs(b2)
