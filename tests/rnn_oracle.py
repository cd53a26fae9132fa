"""CPU restatement of the fused recurrent step (aimet_amd/csrc/rnn_cell.hip) for the tests.

 * exp_r / sigmoid_r / tanh_r: aimet_amd/csrc/rnn_math.hpp operation for operation in numpy float32
   (numpy neither contracts a multiply and an add nor reorders them).
 * cell(): one step of the four cell forms in the evaluation order of torch's CPU cells
   (`torch._VF.lstm_cell`, `gru_cell`, `rnn_tanh_cell`, `rnn_relu_cell`); with torch's own CPU sigmoid
   and tanh plugged in (TORCH_FUNCS) it reproduces them bit for bit (tests/test_rnn.py).
 * step(): the cell, the rows at or beyond `valid_rows` kept, then the QDQ of h and c: what one
   aimet_rnn_step launch computes for one job.
 * layer_forward(): a whole multi-layer, bidirectional layer in the indexing the device path uses
   (per-row time index instead of flipped and shifted copies of the input), equal bit for bit to the
   reference's per-step procedure on tests/golden/golden_rnn.npz.
"""
import numpy as np
import torch

F = np.float32
GATES = {"LSTM": 4, "GRU": 3, "RNN_TANH": 1, "RNN_RELU": 1}
MODE_IDS = {"LSTM": 0, "GRU": 1, "RNN_TANH": 2, "RNN_RELU": 3}


# ---- rnn_math.hpp ------------------------------------------------------------------------------
def _pow2i(n):
    return ((n + np.int32(127)).astype(np.uint32) << np.uint32(23)).view(F)


def exp_r(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        x = np.where(x < F(-87.0), F(-87.0), x)
        x = np.where(x > F(88.5), F(88.5), x)
        z = np.floor((F(1.44269504088896341) * x) + F(0.5))
        x = x - (z * F(0.693359375))
        x = x - (z * F(-2.12194440e-4))
        n = np.where(z == z, z, F(0)).astype(np.int32)
        x2 = x * x
        p = (F(1.9875691500e-4) * x) + F(1.3981999507e-3)
        p = (p * x) + F(8.3334519073e-3)
        p = (p * x) + F(4.1665795894e-2)
        p = (p * x) + F(1.6666665459e-1)
        p = (p * x) + F(5.0000001201e-1)
        r = ((p * x2) + x) + F(1.0)
        a = n >> np.int32(1)
        return (r * _pow2i(a)) * _pow2i(n - a)


def sigmoid_r(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return F(1.0) / (F(1.0) + exp_r(-x))


def tanh_r(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        z = x * x
        q = (F(-5.70498872745e-3) * z) + F(2.06390887954e-2)
        q = (q * z) - F(5.37397155531e-2)
        q = (q * z) + F(1.33314422036e-1)
        q = (q * z) - F(3.33332819422e-1)
        small = ((q * z) * x) + x
        b = np.where(a > F(44.0), F(44.0), a)
        t = F(1.0) - (F(2.0) / (exp_r(b + b) + F(1.0)))
        big = np.where(x < F(0.0), -t, t)
        return np.where(a < F(0.625), small, big)


def _torch_fn(fn):
    def f(x):
        # on the view as it is: torch's CPU kernel takes its vector body and its scalar tail (which
        # are not the same function to the last bit) per contiguous run, so a [B, H] column block of
        # the gate matrix must stay one, as it is inside the _VF cells
        return fn(torch.from_numpy(x)).numpy()
    return f


RESTATED_FUNCS = (sigmoid_r, tanh_r)
TORCH_FUNCS = (_torch_fn(torch.sigmoid), _torch_fn(torch.tanh))


# ---- distances ---------------------------------------------------------------------------------
def ordered(a):
    """float32 -> int64 that orders as the floats do (-0 and +0 both 0)."""
    i = np.ascontiguousarray(a, F).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    return np.abs(ordered(a) - ordered(b))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- QDQ ---------------------------------------------------------------------------------------
def qdq(x, enc):
    """enc = (min, max, bitwidth): the project's per-tensor QDQ, nearest rounding (oracle/)."""
    from oracle import oracle as O
    x = np.ascontiguousarray(x, F)
    return O.qdq_per_tensor(x.ravel(), enc[0], enc[1], enc[2]).reshape(x.shape)


# ---- one step ----------------------------------------------------------------------------------
def cell(mode, ig, hg, b_ih, b_hh, h, c=None, funcs=RESTATED_FUNCS):
    """ig = x W_ih^T, hg = h W_hh^T (no bias), [B, G H]; returns (h', c') (c' None but for LSTM)."""
    sig, tanh = funcs
    H = h.shape[1]
    gi = ig + b_ih if b_ih is not None else ig
    gh = hg + b_hh if b_hh is not None else hg
    if mode == "LSTM":
        g = gi + gh
        i, f, gg, o = (g[:, k * H:(k + 1) * H] for k in range(4))
        i, f, gg, o = sig(i), sig(f), tanh(gg), sig(o)
        c2 = (f * c) + (i * gg)
        return o * tanh(c2), c2
    if mode == "GRU":
        s = gh[:, :2 * H] + gi[:, :2 * H]
        r, z = sig(s[:, :H]), sig(s[:, H:])
        n = tanh(gi[:, 2 * H:] + (gh[:, 2 * H:] * r))
        return ((h - n) * z) + n, None
    s = gh + gi
    if mode == "RNN_TANH":
        return tanh(s), None
    assert mode == "RNN_RELU"
    return np.where(s > F(0), s, F(0)), None


def step(mode, ig, hg, b_ih, b_hh, h, c, valid_rows, h_enc=None, c_enc=None, funcs=RESTATED_FUNCS):
    """One job of one aimet_rnn_step launch: (h', c') of all B rows."""
    h2, c2 = cell(mode, ig, hg, b_ih, b_hh, h, c, funcs)
    h2 = np.array(h2, F)
    h2[valid_rows:] = h[valid_rows:]
    if h_enc is not None:
        h2 = qdq(h2, h_enc)
    if c2 is not None:
        c2 = np.array(c2, F)
        c2[valid_rows:] = c[valid_rows:]
        if c_enc is not None:
            c2 = qdq(c2, c_enc)
    return h2, c2


# ---- a whole layer -----------------------------------------------------------------------------
def param_names(layer, direction, bias):
    sfx = "_reverse" if direction else ""
    names = ["weight_ih_l%d%s", "weight_hh_l%d%s"] + (["bias_ih_l%d%s", "bias_hh_l%d%s"] if bias else [])
    return [n % (layer, sfx) for n in names]


def layer_forward(mode, x, params, num_layers, bidirectional, bias, h0=None, c0=None, lens=None,
                  input_encs=None, h_encs=None, c_encs=None, funcs=RESTATED_FUNCS, record=None):
    """x: [T, B, I], rows in descending order of length when `lens` (their lengths) is given. h0 / c0:
    [num_layers * D, B, H] in the same row order; like the reference's procedure, both directions of
    layer l start from h0[l]. Returns (out [T, B, D H] with zeros where a row has ended, h_n, c_n
    [num_layers * D, B, H]). record(layer, direction, it, h, c) sees every step's state."""
    T, B, _ = x.shape
    D = 2 if bidirectional else 1
    H = params["weight_hh_l0"].shape[1]
    lens = np.full(B, T, np.int64) if lens is None else np.asarray(lens, np.int64)
    inp = np.asarray(x, F)
    hn, cn = [], []
    for layer in range(num_layers):
        xq = qdq(inp, input_encs[layer]) if input_encs and input_encs[layer] is not None else inp
        h_enc = h_encs[layer] if h_encs else None
        c_enc = c_encs[layer] if c_encs else None
        out = np.zeros((T, B, D * H), F)
        for d in range(D):
            w_ih, w_hh, *b = (params[n] for n in param_names(layer, d, bias))
            b_ih, b_hh = b if b else (None, None)
            ig_all = (xq.reshape(T * B, -1).astype(np.float64) @ w_ih.T.astype(np.float64)).astype(F).reshape(T, B, -1)
            h = np.zeros((B, H), F) if h0 is None else np.array(h0[layer], F)
            c = None
            if mode == "LSTM":
                c = np.zeros((B, H), F) if c0 is None else np.array(c0[layer], F)
            if h0 is not None and h_enc is not None:
                h = qdq(h, h_enc)
            if c is not None and c0 is not None and c_enc is not None:
                c = qdq(c, c_enc)
            for it in range(T):
                valid = int((lens > it).sum())
                t_of = np.where(lens > it, lens - 1 - it if d else it, 0)
                ig = ig_all[t_of, np.arange(B)]
                hg = (h.astype(np.float64) @ w_hh.T.astype(np.float64)).astype(F)
                h, c = step(mode, ig, hg, b_ih, b_hh, h, c, valid, h_enc, c_enc, funcs)
                rows = np.arange(valid)
                out[t_of[:valid], rows, d * H:(d + 1) * H] = h[:valid]
                if record is not None:
                    record(layer, d, it, h, c)
            hn.append(h)
            cn.append(c)
        inp = out
    return out, np.stack(hn), (np.stack(cn) if mode == "LSTM" else None)


def run_case(case, a, funcs, encs):
    """A golden_rnn.npz case through layer_forward: (out, h_n, c_n) in the fixture's layout (rows in
    the order given, batch first where the case says so). encs: (input, hidden, parameter, cell)."""
    enc_in, enc_h, enc_p, enc_c = (tuple(float(v) for v in e[:2]) + (int(e[2]),) for e in encs)
    mode, lstm = case["mode"], case["mode"] == "LSTM"
    x = a["x"].transpose(1, 0, 2) if case["batch_first"] else a["x"]
    B = x.shape[1]
    params = {k[2:]: (qdq(v, enc_p) if k.startswith("w_weight") else v) for k, v in a.items() if k.startswith("w_")}
    order, lens = np.arange(B), None
    if "lens" in a:
        order = np.argsort(-np.asarray(a["lens"]), kind="stable")
        lens = np.asarray(a["lens"])[order]
    h0 = a["h0"][:, order] if "h0" in a else None
    c0 = a["c0"][:, order] if "c0" in a else None
    out, hn, cn = layer_forward(mode, x[:, order], params, 2, True, case["bias"], h0, c0, lens, [enc_in] * 2,
                                [enc_h] * 2, [enc_c] * 2 if lstm else None, funcs)
    inv = np.argsort(order)
    out, hn = out[:, inv], hn[:, inv]
    cn = cn[:, inv] if cn is not None else None
    if case["batch_first"]:
        out = out.transpose(1, 0, 2)
    return np.ascontiguousarray(out), np.ascontiguousarray(hn), (np.ascontiguousarray(cn) if lstm else None)


def case_arrays(golden, name):
    """The arrays of case `name` of golden_rnn.npz; parameters (stored as int8 numerators over 64) in float32."""
    out = {}
    for k in golden.files:
        if k.startswith(name + "_"):
            v = golden[k]
            out[k[len(name) + 1:]] = v.astype(F) / F(64) if v.dtype == np.int8 else v
    return out
