"""Sequential MSE on the GPU (aimet_amd/csrc/seqmse.hip, aimet_amd/seq_mse.py).

1. aimet_seqmse_candidate_tables / aimet_seqmse_candidate_qdq, bit for bit against the CPU oracle:
   every candidate's {cand_min, cand_max} goes through the oracle's TF analyzer, per_channel_table
   and qdq_per_channel, one candidate at a time.
2. aimet_seqmse_recon_sums against float64 sums of the same fp32 inputs, within the bound of fp32
   summation, bitwise repeatable, nothing written outside its buffers.
3. apply_seq_mse end to end on two tiny models against a yardstick written here: the reference
   algorithm on the project's per-candidate quantizer API with GEMMs and losses in float64.
Needs an MI355X."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import bits, gpu_available
from oracle import oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _native, seq_mse  # noqa: E402
from aimet_amd.libpymo import RoundingMode  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402
from aimet_amd.seq_mse import SeqMseParams, SequentialMse  # noqa: E402

DEV = "cuda"
GUARD = 8                  # floats before and after every buffer (keeps the payload 16-B aligned)
SENTINEL = 12345.0


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded_dev(payload, off=0):
    """A device buffer [guard | off | payload | guard] filled with SENTINEL; returns (buffer, view).
    `payload` is a host array, or an element count for an output."""
    n = payload if isinstance(payload, int) else payload.size
    buf = torch.full((2 * GUARD + off + n,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[GUARD + off:GUARD + off + n]
    if not isinstance(payload, int):
        view.copy_(torch.from_numpy(np.array(payload, np.float32).ravel()))
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return buf, view


def check_guards(buf, off, n, what):
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD + off] == SENTINEL) and np.all(h[GUARD + off + n:] == SENTINEL), \
        "%s: wrote outside its buffer" % what


# ------------------------------------------------------------------------------------------------
# 1. tables and candidate QDQ
# ------------------------------------------------------------------------------------------------
QDQ_SHAPES = ((1, 5), (3, 4), (5, 8), (7, 1028), (64, 3), (130, 96))
# name -> (symmetric, strict, unsigned, explicit per-channel min)
MODES = {"sym": (1, 0, 0, False), "strict": (1, 1, 0, False), "unsigned": (1, 0, 1, True), "asym": (0, 0, 0, True)}


@functools.lru_cache(maxsize=None)
def weights(C, K):
    """N(0, 0.05) weights with one all-zero channel and one all-positive channel (C >= 3); the zero
    channel is channel 0 of the C == 5 shape (the strict-symmetric detection reads channel 0)."""
    w = (np.random.default_rng(C * 10007 + K).standard_normal((C, K)) * 0.05).astype(np.float32)
    if C >= 3:
        w[0 if C == 5 else C // 2] = 0.0
        w[C - 1] = np.abs(w[C - 1]) + np.float32(0.01)
    w.setflags(write=False)
    return w


def minmax(w, mode):
    """The statistics SequentialMse.get_per_channel_min_and_max hands over ('unsigned' also passes
    the rows' min to a symmetric quantizer, so that the all-positive channel reaches the unsigned grid)."""
    if MODES[mode][3]:
        return w.min(1), w.max(1)
    return None, np.abs(w).max(1)


@functools.lru_cache(maxsize=None)
def want_tables(C, K, mode, bw, n):
    """[n][4][C]: candidate by candidate through the oracle's TF analyzer and per_channel_table."""
    sym, strict, unsign, _ = MODES[mode]
    mn, mx = minmax(weights(C, K), mode)
    out = np.empty((n, 4, C), np.float32)
    for j in range(n):
        cmax = (mx / np.float32(n)).astype(np.float32) * np.float32(j + 1)
        cmin = -cmax if mn is None else (mn / np.float32(n)).astype(np.float32) * np.float32(j + 1)
        encs = []
        for c in range(C):
            a = O.Analyzer(O.QUANTIZATION_TF)
            a.update(np.array([cmin[c], cmax[c]], np.float32))
            encs.append(a.compute(bw, sym, strict, unsign).as_tuple())
        out[j] = O.per_channel_table(encs)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_qdq(C, K, mode, bw, n):
    w = weights(C, K).ravel()
    return np.stack([O.qdq_per_channel(w, C, K, t) for t in want_tables(C, K, mode, bw, n)])


def run_tables(C, K, mode, bw, n):
    sym, strict, unsign, _ = MODES[mode]
    mn, mx = minmax(weights(C, K), mode)
    _, dmx = guarded_dev(mx)
    dmn = guarded_dev(mn)[1] if mn is not None else None
    buf, tables = guarded_dev(n * 4 * C)
    _native.call("aimet_seqmse_candidate_tables", dmn.data_ptr() if dmn is not None else None, dmx.data_ptr(), C, n,
                 bw, sym, strict, unsign, tables.data_ptr(), stream())
    torch.cuda.synchronize()
    check_guards(buf, 0, n * 4 * C, "candidate_tables %s" % ((C, K, mode, bw, n),))
    return tables


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", QDQ_SHAPES, ids=lambda s: "%dx%d" % s)
def test_candidate_tables_and_qdq_bit_exact(shape, mode):
    C, K = shape
    for bw in (4, 3):
        for n in (1, 7, 20):
            tables = run_tables(C, K, mode, bw, n)
            want_t = want_tables(C, K, mode, bw, n)
            got_t = tables.cpu().numpy().reshape(n, 4, C)
            assert np.array_equal(bits(got_t), bits(want_t)), \
                "tables differ: %s" % ((C, K, mode, bw, n, np.argwhere(bits(got_t) != bits(want_t))[:4].tolist()),)
            want = want_qdq(C, K, mode, bw, n)
            windows = ((0, 20), (0, 7), (7, 13), (19, 1)) if n == 20 else ((0, n),)
            for off in (0, 1):   # 16-B aligned / views offset by one float (scalar path)
                _, w = guarded_dev(weights(C, K), off)
                for first, count in windows:
                    obuf, out = guarded_dev(count * C * K, off)
                    _native.call("aimet_seqmse_candidate_qdq", w.data_ptr(), out.data_ptr(), C, K, tables.data_ptr(),
                                 n, first, count, stream())
                    torch.cuda.synchronize()
                    what = "candidate_qdq %s" % ((C, K, mode, bw, n, off, first, count),)
                    check_guards(obuf, off, count * C * K, what)
                    got = out.cpu().numpy().reshape(count, C * K)
                    assert np.array_equal(bits(got), bits(want[first:first + count])), what


def test_candidate_qdq_rejects_bad_windows():
    C, K, n = 3, 4, 7
    tables = run_tables(C, K, "sym", 4, n)
    _, w = guarded_dev(weights(C, K))
    obuf, out = guarded_dev(2 * C * K)
    for first, count in ((-1, 2), (6, 2), (0, 8)):
        with pytest.raises(ValueError):
            _native.call("aimet_seqmse_candidate_qdq", w.data_ptr(), out.data_ptr(), C, K, tables.data_ptr(), n, first,
                         count, stream())
    torch.cuda.synchronize()
    check_guards(obuf, 0, 0, "rejected windows")   # nothing was written at all


# ------------------------------------------------------------------------------------------------
# 2. reconstruction sums
# ------------------------------------------------------------------------------------------------
LAYOUTS = ((1, 1, 1), (5, 3, 1), (63, 4, 1), (257, 130, 1), (1024, 48, 1), (2, 16, 64), (3, 12, 49), (1, 5, 1))
LOSS = {"mse": 0, "l1": 1, "sqnr": 2}


@functools.lru_cache(maxsize=None)
def recon_inputs(outer, C, inner, n):
    """fp32 xw [outer][C][inner], xqwq [outer][n * C][inner] = xw + noise per candidate; the last
    candidate equals xw. With the float64 sums of the same fp32 values."""
    rng = np.random.default_rng(outer * 1000003 + C * 1009 + inner * 7 + n)
    xw = rng.standard_normal((outer, 1, C, inner)).astype(np.float32)
    noise = (rng.standard_normal((outer, n, C, inner)) * 0.1).astype(np.float32)
    noise[:, n - 1] = 0.0
    xq = (xw + noise).astype(np.float32)
    d = xq.astype(np.float64) - xw.astype(np.float64)
    want = {"mse": (d * d).sum((0, 3)), "l1": np.abs(d).sum((0, 3)),
            "sig": (xw.astype(np.float64) ** 2).sum((0, 1, 3))}
    return xw.reshape(outer, C, inner), xq.reshape(outer, n * C, inner), want


def run_recon(xw, xq, outer, C, inner, n, loss, off=0):
    _, dxw = guarded_dev(xw, off)
    _, dxq = guarded_dev(xq, off)
    ebuf, err = guarded_dev(n * C)
    sbuf, sig = guarded_dev(C)
    nbytes = ctypes.c_int64(-1)
    _native.call("aimet_seqmse_recon_sums_workspace", outer, C, inner, n, ctypes.byref(nbytes))
    assert nbytes.value >= 0 and nbytes.value % 4 == 0
    wbuf, ws = guarded_dev(nbytes.value // 4)
    _native.call("aimet_seqmse_recon_sums", dxw.data_ptr(), dxq.data_ptr(), outer, C, inner, n, LOSS[loss],
                 err.data_ptr(), sig.data_ptr() if loss == "sqnr" else None, ws.data_ptr(), nbytes.value, stream())
    torch.cuda.synchronize()
    what = "recon_sums %s" % ((outer, C, inner, n, loss, off),)
    check_guards(ebuf, 0, n * C, what + " err")
    check_guards(wbuf, 0, nbytes.value // 4, what + " workspace")
    check_guards(sbuf, 0, C if loss == "sqnr" else 0, what + " sig")
    return err.cpu().numpy().reshape(n, C), sig.cpu().numpy()


@pytest.mark.parametrize("n", [1, 20])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda s: "%dx%dx%d" % s)
def test_recon_sums(layout, n):
    outer, C, inner = layout
    xw, xq, want = recon_inputs(outer, C, inner, n)
    T = outer * inner
    # T non-negative terms per sum, each with at most 3 roundings (subtract, multiply, convert),
    # added in any order with T - 1 roundings: |got - want| <= (T + 3) * 2^-24 * want
    rel = (T + 3) * 2.0 ** -24
    for off in (0, 1):   # 16-B aligned (vector loads) / offset by one float (scalar loads)
        for loss in ("mse", "l1", "sqnr"):
            err, sig = run_recon(xw, xq, outer, C, inner, n, loss, off)
            w = want["l1" if loss == "l1" else "mse"]
            print("recon", layout, n, loss, off, "max rel err %.3g (bound %.3g)" %
                  (float(np.max(np.abs(err - w) / np.maximum(w, 1e-300))), rel))
            assert np.all(np.abs(err.astype(np.float64) - w) <= rel * w), (layout, n, loss, off)
            assert np.all(err[n - 1] == 0.0), "a candidate equal to xw must give exactly 0"
            if loss == "sqnr":
                assert np.all(np.abs(sig.astype(np.float64) - want["sig"]) <= rel * want["sig"]), (layout, n, off)
            err2, sig2 = run_recon(xw, xq, outer, C, inner, n, loss, off)
            assert np.array_equal(bits(err), bits(err2)), "two calls must give the same bits"
            if loss == "sqnr":
                assert np.array_equal(bits(sig), bits(sig2))


def test_recon_sums_rejects_a_small_workspace():
    outer, C, inner, n = 63, 4, 1, 20
    xw, xq, _ = recon_inputs(outer, C, inner, n)
    _, dxw = guarded_dev(xw)
    _, dxq = guarded_dev(xq)
    ebuf, err = guarded_dev(n * C)
    nbytes = ctypes.c_int64(0)
    _native.call("aimet_seqmse_recon_sums_workspace", outer, C, inner, n, ctypes.byref(nbytes))
    wbuf, ws = guarded_dev(nbytes.value // 4)
    with pytest.raises(ValueError, match="workspace"):
        _native.call("aimet_seqmse_recon_sums", dxw.data_ptr(), dxq.data_ptr(), outer, C, inner, n, 0, err.data_ptr(),
                     None, ws.data_ptr(), nbytes.value - 4, stream())
    with pytest.raises(ValueError, match="loss"):
        _native.call("aimet_seqmse_recon_sums", dxw.data_ptr(), dxq.data_ptr(), outer, C, inner, n, 3, err.data_ptr(),
                     None, ws.data_ptr(), nbytes.value, stream())
    torch.cuda.synchronize()
    check_guards(ebuf, 0, 0, "rejected call")


# ------------------------------------------------------------------------------------------------
# 3. end to end
# ------------------------------------------------------------------------------------------------
# EPS: the largest relative difference, over every layer, candidate and channel of the cases below,
# between the plain-torch fp32 loop's losses (F.linear / F.conv2d + mse_loss / l1_loss / neg_sqnr
# + .sum(0): the reference's own arithmetic) and the float64 yardstick, measured on an MI355X with
# measure_eps() below. GAP = 4 * EPS: two losses are compared, and the stacked GEMM may
# sum in another order than the per-candidate one. Channels whose yardstick best and runner-up
# losses are closer than GAP (relative) are not compared; at most MAX_EXCLUDED of a layer's channels.
# Measured: 1.290e-6 (the asymmetric Linear model's first layer under mse; 2.0e-7 .. 1.3e-6 over the
# cases), rounded up. The smallest best-to-runner-up gap of any channel there was 4.0e-5.
EPS = 1.3e-6
GAP = 4 * EPS
MAX_EXCLUDED = 0.05
N_CAND = 20
NUM_BATCHES = 4


def cfg(symmetric):
    return {"defaults": {"ops": {"is_output_quantized": "True"},
                         "params": {"is_quantized": "True", "is_symmetric": str(symmetric)},
                         "strict_symmetric": "False", "per_channel_quantization": "True"}}


def make_model(kind):
    torch.manual_seed(0)
    if kind == "linear":
        m = nn.Sequential(nn.Linear(64, 48), nn.ReLU(), nn.Linear(48, 130))
    else:
        m = nn.Sequential(nn.Conv2d(8, 16, 3, padding=1), nn.ReLU(), nn.Conv2d(16, 12, 1))
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for layer in (m[0], m[2]):
            layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * 0.05)
    return m.eval().to(DEV)


@functools.lru_cache(maxsize=None)
def make_batches(kind):
    g = torch.Generator().manual_seed(0)
    shape = (64, 64) if kind == "linear" else (2, 8, 8, 8)
    return tuple(torch.randn(shape, generator=g).to(DEV) for _ in range(NUM_BATCHES))


def make_sim(model, symmetric, per_channel=True):
    config = cfg(symmetric)
    config["defaults"]["per_channel_quantization"] = str(per_channel)
    return QuantizationSimModel(model, quant_scheme="tf", default_param_bw=4, config_file=config)


def encodings_of(q):
    return [e.to_tuple() for e in (q.encoding if isinstance(q.encoding, list) else [q.encoding])]


def outputs64(module, x, w):
    """x W^T (Linear) or the convolution as unfold + matmul (Conv2d), in float64, channels last."""
    x, w = x.double(), w.double()
    if isinstance(module, nn.Linear):
        return F.linear(x, w).reshape(-1, w.shape[0])
    outs = []
    for xg, wg in zip(x.chunk(module.groups, 1), w.chunk(module.groups, 0)):
        cols = F.unfold(xg, module.kernel_size, dilation=module.dilation, padding=module.padding,
                        stride=module.stride)
        outs.append(wg.reshape(wg.shape[0], -1) @ cols)
    return torch.cat(outs, 1).permute(0, 2, 1).reshape(-1, w.shape[0])


def outputs32(module, x, w):
    """The reference's compute_outputs in fp32 (conv outputs permuted to channels last)."""
    if isinstance(module, nn.Linear):
        return F.linear(x, w).reshape(-1, w.shape[0])
    y = F.conv2d(x, w, stride=module.stride, dilation=module.dilation, padding=module.padding, groups=module.groups)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def recon_loss(xqwq, xw, loss_fn):
    """The reference's compute_recon_loss in the dtype of its inputs."""
    fn = {"mse": F.mse_loss, "l1": F.l1_loss, "sqnr": seq_mse.neg_sqnr}[loss_fn]
    return fn(xqwq, xw, reduction="none").sum(0)


def candidate_loop(quant_module, x, xq, loss_fn, with_fp32=False):
    """The reference's candidate loop of optimize_module on the per-candidate quantizer API
    (reset_encoding_stats / update_encoding_stats / compute_encoding / quantize_dequantize):
    (float64 losses [N_CAND][C], the candidates' encodings, (cand_max, cand_min), fp32 losses)."""
    q = quant_module.param_quantizers["weight"]
    module = quant_module._module_to_wrap
    w = module.weight.detach()
    mn, mx = SequentialMse.get_per_channel_min_and_max(quant_module)
    cands = seq_mse.get_candidates(N_CAND, mx, mn)
    xw64 = [outputs64(module, x[b], w) for b in range(NUM_BATCHES)]
    xw32 = [outputs32(module, x[b], w) for b in range(NUM_BATCHES)] if with_fp32 else None
    loss64, loss32, encs = [], [], []
    with torch.no_grad():
        for cand_max, cand_min in cands:
            q.reset_encoding_stats()
            q.update_encoding_stats(torch.stack([cand_min, cand_max], dim=-1))
            q.compute_encoding()
            encs.append(encodings_of(q))
            wq = q.quantize_dequantize(w, RoundingMode.ROUND_NEAREST)
            loss64.append(sum(recon_loss(outputs64(module, xq[b], wq), xw64[b], loss_fn)
                              for b in range(NUM_BATCHES)))
            if with_fp32:
                loss32.append(sum(recon_loss(outputs32(module, xq[b], wq), xw32[b], loss_fn)
                                  for b in range(NUM_BATCHES)))
    return torch.stack(loss64), encs, cands, (torch.stack(loss32) if with_fp32 else None)


def relative_gap(loss64):
    """Per channel: (runner-up - best) / |best| of the yardstick's losses, and the first minimum."""
    n = loss64.shape[0]
    best = loss64.min(0)
    first = torch.where(loss64 == best.values, torch.arange(n, device=loss64.device).unsqueeze(1), n).min(0).values
    if n == 1:
        return torch.full_like(best.values, float("inf")), first
    rest = loss64.clone()
    rest[first, torch.arange(loss64.shape[1], device=loss64.device)] = float("inf")
    return (rest.min(0).values - best.values) / best.values.abs().clamp_min(1e-300), first


def module_inputs(name, model, sim, params, data):
    """(x, xq) of run_seq_mse for the module called `name`."""
    fp_mod = dict(model.named_modules())[name]
    q_mod = dict(sim.model.named_modules())[name]
    if params.inp_symmetry == "symqt":
        xq = SequentialMse.get_module_inp_acts(q_mod, sim.model, params, params.forward_fn, data)
        return xq, xq
    x = SequentialMse.get_module_inp_acts(fp_mod, model, params, params.forward_fn, data)
    if params.inp_symmetry == "symfp":
        return x, x
    return x, SequentialMse.get_module_inp_acts(q_mod, sim.model, params, params.forward_fn, data)


def walk(kind, symmetric, loss_fn, inp_symmetry, visit, with_fp32=False):
    """Run apply_seq_mse on one sim, then replay it layer by layer on a second sim with the
    yardstick's candidate loop; `visit(name, loss64, loss32, first, gap, chosen)` sees every layer
    (loss32, the plain fp32 loop's losses, only `with_fp32`).
    The second sim then takes the first sim's choice (through compute_param_encodings, checking the
    frozen encodings bit for bit), so both see the same inputs at the next layer."""
    model = make_model(kind)
    data = make_batches(kind)
    params = SeqMseParams(num_batches=NUM_BATCHES, num_candidates=N_CAND, inp_symmetry=inp_symmetry, loss_fn=loss_fn)
    sim = make_sim(model, symmetric)
    flags = [q.enabled for _, w in sim.quant_wrappers() for q in w.input_quantizers + w.output_quantizers]
    seq_mse.apply_seq_mse(model, sim, list(data), params)
    assert flags == [q.enabled for _, w in sim.quant_wrappers() for q in w.input_quantizers + w.output_quantizers]

    yard = make_sim(model, symmetric)
    with SequentialMse.temporarily_disable_quantizers(model, yard, None):
        SequentialMse.compute_all_param_encodings(yard)
        for name in ("0", "2"):
            got_q = dict(sim.model.named_modules())[name].param_quantizers["weight"]
            assert got_q.is_encoding_frozen, name
            got = encodings_of(got_q)
            q_mod = dict(yard.model.named_modules())[name]
            x, xq = module_inputs(name, model, yard, params, data)
            loss64, encs, cands, loss32 = candidate_loop(q_mod, x, xq, loss_fn, with_fp32)
            gap, first = relative_gap(loss64)
            # the candidate the first sim chose, per channel: the one whose encoding it froze
            C = len(got)
            chosen = torch.tensor([next((j for j in range(N_CAND) if encs[j][c] == got[c]), -1) for c in range(C)],
                                  device=DEV)
            assert bool((chosen >= 0).all()), "layer %s: a frozen encoding is no candidate's encoding" % name
            visit(name, loss64, loss32, first, gap, chosen)
            idx = chosen.unsqueeze(0)
            best_max = torch.stack([c[0] for c in cands]).gather(0, idx)[0]
            best_min = torch.stack([c[1] for c in cands]).gather(0, idx)[0]
            yq = q_mod.param_quantizers["weight"]
            SequentialMse.compute_param_encodings(yq, best_min, best_max)
            yq.freeze_encoding()
            assert encodings_of(yq) == got, "layer %s: frozen encodings differ from compute_param_encodings" % name
    return sim


def measure_eps():
    """EPS as described above, over every end-to-end case (run from a job script on an MI355X)."""
    worst = {}

    for case in E2E_CASES:
        def visit(name, loss64, loss32, first, gap, chosen, case=case):
            rel = ((loss32.double() - loss64).abs() / loss64.abs().clamp_min(1e-300)).max().item()
            worst[case + (name,)] = (rel, gap.min().item(), int((first != chosen).sum()))
        walk(*case, visit, with_fp32=True)
    return worst


E2E_CASES = tuple(("linear", s, loss, inp) for s in (True, False) for loss in ("mse", "l1", "sqnr")
                  for inp in ("symqt", "asym")) + \
    tuple(("conv", s, "mse", inp) for s in (True, False) for inp in ("symqt", "asym"))


@pytest.mark.parametrize("case", E2E_CASES, ids=lambda c: "%s-%s-%s-%s" % (c[0], "sym" if c[1] else "asym", c[2], c[3]))
def test_apply_seq_mse_matches_the_float64_yardstick(case):
    def visit(name, loss64, loss32, first, gap, chosen):
        compared = gap >= GAP
        excluded = int((~compared).sum())
        print("e2e", case, "layer", name, "min gap %.3g" % gap.min().item(), "excluded", excluded, "of", gap.numel())
        assert excluded <= MAX_EXCLUDED * gap.numel(), (case, name, excluded)
        assert torch.equal(chosen[compared], first[compared]), \
            (case, name, torch.nonzero(chosen != first).flatten().tolist())

    walk(*case, visit)


def test_excluded_module_stays_unfrozen_and_runs_repeat():
    model = make_model("linear")
    data = list(make_batches("linear"))
    params = SeqMseParams(num_batches=NUM_BATCHES, num_candidates=N_CAND)
    sim = make_sim(model, True)
    seq_mse.apply_seq_mse(model, sim, data, params, modules_to_exclude=[model[2]])
    assert sim.model[0].param_quantizers["weight"].is_encoding_frozen
    q2 = sim.model[2].param_quantizers["weight"]
    assert not q2.is_encoding_frozen and q2.enabled
    # two fresh sims give identical encodings
    a, b = make_sim(model, True), make_sim(model, True)
    seq_mse.apply_seq_mse(model, a, data, params)
    seq_mse.apply_seq_mse(model, b, data, params)
    for name in ("0", "2"):
        qa, qb = (dict(s.model.named_modules())[name].param_quantizers["weight"] for s in (a, b))
        assert qa.is_encoding_frozen and qb.is_encoding_frozen and encodings_of(qa) == encodings_of(qb)
    assert encodings_of(a.model[0].param_quantizers["weight"]) == encodings_of(sim.model[0].param_quantizers["weight"])


@pytest.mark.parametrize("variant", ["per_tensor", "bf16", "grouped", "bw8", "windowed"])
def test_other_paths(variant, monkeypatch):
    """A per-tensor weight quantizer (C = 1 table), 16-bit weights, a grouped convolution (one conv per
    candidate), a module above 4 bits (skipped) and a window smaller than the candidate count."""
    params = SeqMseParams(num_batches=NUM_BATCHES, num_candidates=N_CAND)
    if variant == "grouped":
        torch.manual_seed(0)
        model = nn.Sequential(nn.Conv2d(8, 16, 3, padding=1, groups=2)).eval().to(DEV)
        data = list(make_batches("conv"))
    else:
        model = make_model("linear")
        data = list(make_batches("linear"))
    if variant == "bf16":
        model = model.to(torch.bfloat16)
        data = [d.to(torch.bfloat16) for d in data]
    if variant == "windowed":
        whole = make_sim(model, True)
        seq_mse.apply_seq_mse(model, whole, data, params)
        # from here on: room for three candidates of the larger layer (weights + one batch's output)
        monkeypatch.setattr(seq_mse, "CANDIDATE_WINDOW_BYTES", 3 * 4 * (130 * 48 + 130 * 64))
    sim = make_sim(model, True, per_channel=variant != "per_tensor")
    if variant == "bw8":
        sim.model[2].param_quantizers["weight"].bitwidth = 8
    seq_mse.apply_seq_mse(model, sim, data, params)
    q0 = sim.model[0].param_quantizers["weight"]
    assert q0.is_encoding_frozen and q0.enabled
    if variant == "bw8":
        assert not sim.model[2].param_quantizers["weight"].is_encoding_frozen
    if variant == "windowed":
        for name in ("0", "2"):
            qa, qb = (dict(s.model.named_modules())[name].param_quantizers["weight"] for s in (sim, whole))
            assert encodings_of(qa) == encodings_of(qb)
    if variant in ("per_tensor", "grouped"):
        # the choice against the float64 yardstick on a second sim, as in walk()
        yard = make_sim(model, True, per_channel=variant != "per_tensor")
        with SequentialMse.temporarily_disable_quantizers(model, yard, None):
            SequentialMse.compute_all_param_encodings(yard)
            q_mod = yard.model[0]
            x, xq = module_inputs("0", model, yard, params, data)
            total = SequentialMse._candidate_losses(q_mod, *SequentialMse.get_per_channel_min_and_max(q_mod), x, xq,
                                                    params)
            chosen = seq_mse._first_argmin(total)
            loss64, _, cands, _ = candidate_loop(q_mod, x, xq, "mse")
            gap, first = relative_gap(loss64)
            compared = gap >= GAP
            assert int((~compared).sum()) <= MAX_EXCLUDED * gap.numel()
            assert torch.equal(chosen[compared], first[compared])
            idx = chosen.unsqueeze(0)
            yq = q_mod.param_quantizers["weight"]
            SequentialMse.compute_param_encodings(yq, torch.stack([c[1] for c in cands]).gather(0, idx)[0],
                                                  torch.stack([c[0] for c in cands]).gather(0, idx)[0])
            assert encodings_of(yq) == encodings_of(q0)
