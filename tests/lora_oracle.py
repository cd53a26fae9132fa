"""TEST INFRASTRUCTURE ONLY: numpy restatements of the aimet_lora_* kernels (aimet_amd/csrc/lora.hip)
and of the quantized LoRA layer's forward, on the per-tensor QDQ the other oracles use (oracle/).

A tensor of a 16-bit dtype is held as a float32 array of values that dtype represents; rnd() is the
rounding to the dtype the literal route performs wherever it materialises a tensor. Encodings are
(min, max, bitwidth) or None (a disabled quantizer).
"""
import numpy as np

from rnn_oracle import qdq as _qdq

F = np.float32
DTYPES = ("fp32", "fp16", "bf16")
IO_CODE = {"fp32": 0, "fp16": 1, "bf16": 2}
# spacing of the dtype's values relative to their size (for planting a bound's neighbours)
EPS = {"fp32": 2.0 ** -23, "fp16": 2.0 ** -10, "bf16": 2.0 ** -7}


# ---- the roundings, written out ------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> bfloat16 bit patterns: round to nearest even on the upper 16 bits, NaN -> 0x7FC0."""
    x = np.ascontiguousarray(x, F)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def fp16_bits(x):
    """float32 -> float16 bit patterns: IEEE round to nearest even (overflow to inf)."""
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(x, F).astype(np.float16).view(np.uint16)


def store_bits(x, dt):
    """The bit patterns of x stored as dtype dt (uint32 for fp32, uint16 otherwise)."""
    if dt == "fp32":
        return np.ascontiguousarray(x, F).view(np.uint32)
    return bf16_bits(x) if dt == "bf16" else fp16_bits(x)


def load_bits(b, dt):
    """Stored bit patterns -> float32 values (exact)."""
    b = np.ascontiguousarray(b)
    if dt == "fp32":
        return b.view(F)
    if dt == "fp16":
        return b.view(np.float16).astype(F)
    return (b.astype(np.uint32) << np.uint32(16)).view(F)


def rnd(x, dt):
    """x rounded to dt, as float32."""
    return np.ascontiguousarray(x, F) if dt == "fp32" else load_bits(store_bits(x, dt), dt)


def nan_blind(b, dt):
    """Bit patterns with every NaN mapped to one pattern (which NaN an operation yields is the
    hardware's choice; where a NaN stands is not)."""
    v = load_bits(b, dt)
    out = np.array(b, copy=True)
    out[np.isnan(v)] = 0x7FC00000 if dt == "fp32" else (0x7E00 if dt == "fp16" else 0x7FC0)
    return out


def host_scale(scale, dt):
    """The float the scale kernels multiply by: float32(scale), rounded to dt."""
    return F(rnd(np.array([scale], F), dt)[0])


def bound(v, dt):
    """A straight-through bound: the encoding's min or max as float32, then in the tensor's dtype."""
    return F(rnd(np.array([v], F), dt)[0])


# ---- the four kernels ----------------------------------------------------------------------------
def Q(x, enc, dt):
    return np.ascontiguousarray(x, F) if enc is None else rnd(_qdq(x, enc), dt)


def _gate(g, x, enc, dt):
    """g * (min <= x <= max) in dt; a disabled quantizer passes g on."""
    if enc is None:
        return g
    with np.errstate(all="ignore"):
        mask = ((bound(enc[0], dt) <= x) & (x <= bound(enc[1], dt))).astype(F)
        return rnd(g * mask, dt)


def merge_sum(u, v, enc_u, enc_v, dt):
    with np.errstate(all="ignore"):
        return rnd(Q(u, enc_u, dt) + Q(v, enc_v, dt), dt)


def merge(u, v, enc_u, enc_v, enc_out, dt):
    return Q(merge_sum(u, v, enc_u, enc_v, dt), enc_out, dt)


def merge_backward(u, v, g, enc_u, enc_v, enc_out, dt):
    g1 = _gate(np.ascontiguousarray(g, F), merge_sum(u, v, enc_u, enc_v, dt), enc_out, dt)
    return _gate(g1, np.ascontiguousarray(u, F), enc_u, dt), _gate(g1, np.ascontiguousarray(v, F), enc_v, dt)


def scale_product(a, s, enc_a, dt):
    with np.errstate(all="ignore"):
        return rnd(Q(a, enc_a, dt) * F(s), dt)


def scale(a, s, enc_a, enc_out, dt):
    """s: the float the kernel is given (host_scale)."""
    return Q(scale_product(a, s, enc_a, dt), enc_out, dt)


def scale_backward(a, g, s, enc_a, enc_out, dt):
    g1 = _gate(np.ascontiguousarray(g, F), scale_product(a, s, enc_a, dt), enc_out, dt)
    with np.errstate(all="ignore"):
        g2 = rnd(g1 * F(s), dt)
    return _gate(g2, np.ascontiguousarray(a, F), enc_a, dt)


# ---- the layer -----------------------------------------------------------------------------------
def layer_forward(u, a, v_of_m, s, encs, dt):
    """One adapter of a quantized LoRA layer from the raw GEMM outputs: u = base_layer's, a = lora_A's,
    v_of_m(m) = lora_B's for the scaled input m. encs: base, A, mul, B, add. Returns (m, out)."""
    m = scale(a, host_scale(s, dt), encs["A"], encs["mul"], dt)
    return m, merge(u, v_of_m(m), encs["base"], encs["B"], encs["add"], dt)


# ---- planted inputs ------------------------------------------------------------------------------
def _gated(enc):
    from oracle import oracle as O
    e = O.fill_encoding_info(enc[2], enc[0], enc[1])
    return e.min, e.max, e.delta


def planted(encs, dt):
    """Values every kernel test plants: +-0, +-inf, NaN, each encoding's raw and gated min and max with
    their neighbours on both sides (float32's and dt's), rounding ties (x / delta an exact half) and
    values far out of range."""
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e30, -1e30, 3.0e4, -3.0e4, 1e-30, -1e-30]
    for enc in encs:
        if enc is None:
            continue
        gmin, gmax, delta = _gated(enc)
        for b in (enc[0], enc[1], gmin, gmax):
            b32 = F(b)
            bd = bound(b, dt)
            vals += [b32, np.nextafter(b32, F(np.inf)), np.nextafter(b32, F(-np.inf)), bd,
                     F(bd * F(1 + EPS[dt])), F(bd * F(1 - EPS[dt])), F(bd + F(delta)), F(bd - F(delta))]
        d32 = F(delta)
        for k in (-3, -1, 0, 2, 5):
            vals += [F(F(k + 0.5) * d32), F(F(gmin) + F(k + 0.5) * d32)]
    return rnd(np.array(vals, F), dt)


def inputs(n, seed, encs, dt, shift=0):
    """n seeded normals x 3 in dt with planted() written over the front, rotated by `shift` so that a
    short tensor still meets different planted values."""
    rng = np.random.default_rng(seed)
    x = rnd((rng.standard_normal(n) * 3.0).astype(F), dt)
    p = planted(encs, dt)
    k = min(n, len(p))
    x[:k] = np.roll(p, -shift)[:k]
    return x
