"""CPU restatement of the fused attention softmax (aimet_amd/csrc/attn_softmax.hip) and of the
quantizable multi-head attention built on it (aimet_amd/transformers.py), for the tests.

 * attn_softmax(): the kernel operation for operation in numpy float32 -- the QDQ of the project's
   oracle, the masks, exp_r of rnn_math.hpp (tests/rnn_oracle.py), the documented summation order
   (strided lane sums, the xor butterfly, the pair of pairs above 1024 columns) and the IEEE divide.
   Equal inputs give equal bits.
 * mha_forward(): the whole module in ACTIVE mode with every quantizer of the default layout (the
   output quantizer of each child, the weight quantizer of each linear). Its GEMMs run in float64
   and round once: the fixtures (tests/golden/make_golden_mha.py) are built so that every GEMM sum
   is exact, and then any summation order gives these bits.
"""
import numpy as np

from rnn_oracle import F, bits, exp_r, ordered, qdq, ulp_distance   # noqa: F401  (re-exported)

WAVE = 64
WAVE_MAX_S = 1024
MAX_S = 16320


def _butterfly(v):
    """v: [..., 64] lane sums -> the same shape after v_t = v_t + v_(t xor d), d = 32 .. 1."""
    idx = np.arange(WAVE)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ d]
    return v


def row_sums(e):
    """e: [R, S] float32 -> [R] sums in the kernel's order."""
    R, S = e.shape
    lanes = WAVE if S <= WAVE_MAX_S else 4 * WAVE
    n = -(-S // lanes)
    pad = np.zeros((R, n * lanes), F)
    pad[:, :S] = e
    pad = pad.reshape(R, n, lanes)
    acc = pad[:, 0].copy()
    for i in range(1, n):
        acc = acc + pad[:, i]
    w = _butterfly(acc.reshape(R, lanes // WAVE, WAVE))[:, :, 0]
    if lanes == WAVE:
        return w[:, 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def softmax_rows(x):
    """Steps 3 of the kernel on already quantized and masked rows x [R, S]: unquantized probabilities."""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        m = x.max(axis=1, keepdims=True)
        e = np.where(x == F(-np.inf), F(0), exp_r(x - m)).astype(F)
        return e / row_sums(e)[:, None]


def attn_softmax(scores, B, H, L, S, attn_mask=None, per_bh=False, key_padding_mask=None, score_enc=None,
                 prob_enc=None):
    """scores: B*H*L*S float32. attn_mask: [L, S] or (per_bh) [B*H, L, S] bool; key_padding_mask [B, S]
    bool; encodings (min, max, bw) or None. Returns probs [B*H, L, S]."""
    x = np.array(scores, F).reshape(B * H, L, S)
    if score_enc is not None:
        x = qdq(x, score_enc)
    if attn_mask is not None:
        am = np.asarray(attn_mask, bool).reshape((B * H, L, S) if per_bh else (1, L, S))
        x = np.where(am, F(-np.inf), x)
    if key_padding_mask is not None:
        kpm = np.repeat(np.asarray(key_padding_mask, bool).reshape(B, 1, 1, S), H, axis=1).reshape(B * H, 1, S)
        x = np.where(kpm, F(-np.inf), x)
    p = softmax_rows(x.reshape(B * H * L, S)).reshape(B * H, L, S)
    if prob_enc is not None:
        p = qdq(p, prob_enc)
    return p


# ---- the module --------------------------------------------------------------------------------
def _gemm(a, b):
    return (a.astype(np.float64) @ b.astype(np.float64)).astype(F)


def _q(x, enc):
    return qdq(x, enc) if enc is not None else np.asarray(x, F)


def mha_forward(w, query, key, value, num_heads, encs, batch_first=False, add_zero_attn=False, attn_mask=None,
                key_padding_mask=None, need_weights=True, average_attn_weights=True, softmax=None):
    """w: dict of float32 arrays (linear_Q/K/V.weight/.bias, out_proj.weight/.bias, optional bias_k, bias_v).
    encs: dict name -> (min, max, bw) or None for 'linear_Q', 'linear_K', 'linear_V', 'div', 'matmul_1',
    'softmax', 'matmul_2', 'out_proj' (output quantizers) and 'weight' (every linear's weight).
    softmax: a replacement for softmax_rows (the generator plugs in torch's). Returns (out, weights)."""
    softmax = softmax or softmax_rows
    if batch_first:
        query, key, value = (np.ascontiguousarray(np.swapaxes(t, 0, 1)) for t in (query, key, value))
    Lq, B, E = query.shape
    hd = E // num_heads

    def linear(name, x):
        wt = _q(w[name + ".weight"], encs.get("weight"))
        y = _gemm(x.reshape(-1, x.shape[-1]), wt.T)
        if name + ".bias" in w:
            y = y + w[name + ".bias"]
        return _q(y.reshape(x.shape[:-1] + (wt.shape[0],)), encs.get(name))

    k = linear("linear_K", key)
    v = linear("linear_V", value)
    q = _q(linear("linear_Q", query) / F(float(hd) ** 0.5), encs.get("div"))
    am = None if attn_mask is None else np.asarray(attn_mask, bool)
    if am is not None and am.ndim == 2:
        am = am[None]
    kpm = None if key_padding_mask is None else np.asarray(key_padding_mask, bool)

    def pad(mask):
        return None if mask is None else np.concatenate([mask, np.zeros(mask.shape[:-1] + (1,), bool)], axis=-1)

    if "bias_k" in w:
        k = np.concatenate([k, np.broadcast_to(w["bias_k"], (1, B, E))])
        v = np.concatenate([v, np.broadcast_to(w["bias_v"], (1, B, E))])
        am, kpm = pad(am), pad(kpm)
    q = q.reshape(Lq, B * num_heads, hd).transpose(1, 0, 2)
    k = k.reshape(-1, B * num_heads, hd).transpose(1, 0, 2)
    v = v.reshape(-1, B * num_heads, hd).transpose(1, 0, 2)
    if add_zero_attn:
        z = np.zeros((B * num_heads, 1, hd), F)
        k, v = np.concatenate([k, z], axis=1), np.concatenate([v, z], axis=1)
        am, kpm = pad(am), pad(kpm)
    S = k.shape[1]
    scores = np.stack([_gemm(q[i], k[i].T) for i in range(B * num_heads)])
    x = _q(scores, encs.get("matmul_1"))
    if am is not None:
        x = np.where(np.broadcast_to(am, x.shape), F(-np.inf), x)
    if kpm is not None:
        x = np.where(np.repeat(kpm[:, None, None, :], num_heads, axis=1).reshape(B * num_heads, 1, S), F(-np.inf), x)
    p = _q(np.asarray(softmax(x.reshape(-1, S)), F).reshape(x.shape), encs.get("softmax"))
    o = _q(np.stack([_gemm(p[i], v[i]) for i in range(B * num_heads)]), encs.get("matmul_2"))
    o = o.transpose(1, 0, 2).reshape(Lq, B, E)
    if batch_first:
        o = np.ascontiguousarray(np.swapaxes(o, 0, 1))
    out = linear("out_proj", o)
    if not need_weights:
        return out, None
    pw = p.reshape(B, num_heads, Lq, S)
    if average_attn_weights:
        pw = pw.mean(axis=1, dtype=F)
    return out, pw


def run_case(case, a, encs, softmax=None):
    """A golden_mha.npz case (its entry of `cases`, its arrays in float32) through mha_forward."""
    w = {k[2:]: v for k, v in a.items() if k.startswith("w_")}
    return mha_forward(w, a["query"], a["key"], a["value"], case["H"], encs, batch_first=case.get("batch_first", False),
                       add_zero_attn=case.get("add_zero_attn", False), attn_mask=a.get("attn_mask"),
                       key_padding_mask=a.get("key_padding_mask"), need_weights=case["need_weights"],
                       average_attn_weights=case["average"], softmax=softmax)


def case_arrays(golden, name):
    """The arrays of case `name` of golden_mha.npz; parameters (stored as int16 numerators over 64) in float32."""
    out = {}
    for k in golden.files:
        if k.startswith(name + "_"):
            v = golden[k]
            out[k[len(name) + 1:]] = v.astype(F) / F(64) if v.dtype == np.int16 else v
    return out
