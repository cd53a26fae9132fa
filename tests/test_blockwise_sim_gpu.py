"""Blockwise and LPBQ weight quantization on the device (aimet_bq_encode_qdq, aimet_amd.blockwise).

Every comparison is equality. The reference restates the kernel on the host: float64 min / max per
block, the TF analyzer's gating (zero inside the range, a range of at least 0.01:
TfEncodingAnalyzer.cpp:80-101), the host getComputedEncodings (pinned to golden vectors by
test_capi_host.py), the table as float32 and the oracle's per-channel QDQ over the [1, E, BL] view."""
import copy
import itertools
import json

import numpy as np
import pytest

from conftest import bits, gpu_available
from oracle import oracle as O

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SYMMETRY = {"symmetric": (True, False, False), "strict": (True, True, False), "unsigned": (True, False, True),
            "asymmetric": (False, False, False)}
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def host_encodings(x32, E, BL, bw, sym, strict, unsign):
    from aimet_amd.libpymo import getComputedEncodings
    blocks = x32.reshape(E, BL).astype(np.float64)
    encs = []
    for mn, mx in zip(blocks.min(1).tolist(), blocks.max(1).tolist()):
        lo, hi = min(0.0, mn), max(0.0, mx)
        hi = max(hi, lo + 0.01)
        encs.append(getComputedEncodings(bw, lo, hi, sym, strict, unsign))
    return encs


def table_of(encs):
    return np.array([[e.min, e.max, e.delta, e.offset] for e in encs], np.float64).T.astype(np.float32)


def host_qdq(x32, table, dtype):
    E = table.shape[1]
    y = O.qdq_per_channel(x32, E, x32.size // E, table.ravel())
    return torch.from_numpy(y).to(dtype)   # one rounding to the I/O width


def raw(t):
    """Bit patterns of a float32 / 16-bit tensor."""
    t = t.detach().cpu().contiguous()
    return bits(t.numpy()) if t.dtype == torch.float32 else t.view(torch.int16).numpy()


def device_run(x, R, NB, BL, bw, flags, place, shift, sbw=0):
    """The kernel on x (a CPU tensor) placed `shift` elements into a device buffer; `place`: "in"
    (in place), "out" (an output as far from 16 bytes as the input) or "apart" (one that is not)."""
    from aimet_amd import blockwise as B
    n = x.numel()
    src = torch.empty(n + 1, dtype=x.dtype, device="cuda")[shift:shift + n].copy_(x)
    if place == "in":
        dst = src
    else:
        s = shift if place == "out" else 1 - shift
        dst = torch.zeros(n + 1, dtype=x.dtype, device="cuda")[s:s + n]
    table, q, factor = B.encode_qdq(src, R, NB, BL, bw, *flags, scale_bitwidth=sbw, out=dst)
    return table.cpu().numpy(), dst, q, factor


def data(rng, n, dtype):
    x = torch.from_numpy((rng.standard_normal(n) * 0.7 + 0.1).astype(np.float32)).to(dtype)
    return x, x.float().numpy()


@pytest.mark.parametrize("BL", [16, 64, 96, 288])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_kernel_matches_host_restatement(dtype, BL):
    rng = np.random.default_rng(BL)
    for NB, R in itertools.product((1, 3, 7), (1, 5)):
        x, x32 = data(rng, R * NB * BL, DTYPES[dtype])
        for (name, flags), bw in itertools.product(SYMMETRY.items(), (4, 8)):
            want_t = table_of(host_encodings(x32, R * NB, BL, bw, *flags))
            want_y = raw(host_qdq(x32, want_t, DTYPES[dtype]))
            for place, shift in itertools.product(("in", "out", "apart"), (0, 1)):
                got_t, got_y, _, _ = device_run(x, R, NB, BL, bw, flags, place, shift)
                what = (NB, R, name, bw, place, shift)
                np.testing.assert_array_equal(bits(got_t), bits(want_t), err_msg=str(what))
                np.testing.assert_array_equal(raw(got_y), want_y, err_msg=str(what))


# fp32 blocks of 64 elements take 16 lanes, so a wave holds 4 blocks a round and 8 rounds: 32 blocks;
# 96 (NB + 1) bytes of LDS a 16-element fp32 block: 681 blocks fit 64 KiB, 682 do not
@pytest.mark.parametrize("NB,BL,R,path", [(32, 64, 3, "PATH_WAVE"), (33, 64, 3, "PATH_GROUP"),
                                          (681, 16, 2, "PATH_GROUP"), (682, 16, 2, "PATH_TWO_PASS")])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_kernel_paths(dtype, NB, BL, R, path):
    from aimet_amd import blockwise as B
    if dtype == "fp32":
        assert B.row_path(NB, BL) == getattr(B, path)
    rng = np.random.default_rng(NB)
    x, x32 = data(rng, R * NB * BL, DTYPES[dtype])
    flags = SYMMETRY["asymmetric"]
    want_t = table_of(host_encodings(x32, R * NB, BL, 4, *flags))
    want_y = raw(host_qdq(x32, want_t, DTYPES[dtype]))
    for place, shift in (("in", 0), ("out", 1), ("apart", 0)):
        got_t, got_y, _, _ = device_run(x, R, NB, BL, 4, flags, place, shift)
        np.testing.assert_array_equal(bits(got_t), bits(want_t), err_msg=place)
        np.testing.assert_array_equal(raw(got_y), want_y, err_msg=place)


# blockwise.hip:53 caps the grid at kMaxGrid = 65536 workgroups; bq_wave gives a workgroup four rows
# (kBlk / kWave, blockwise.hip:217), bq_group one. A row past these strides is a second trip of the row
# loop (blockwise.hip:218, :312), over a block table in LDS that the first trip filled.
MAX_GRID = 1 << 16
WAVE_ROWS = 4
TILE = 257   # a prime that divides neither stride: rows one stride apart never hold equal data
SENTINEL = -777.25   # no 4-bit grid of these blocks reaches it; a 16-bit type rounds it, and compares as rounded


# The vector slots a lane of bq_wave holds (plan_of, blockwise.hip:435) choose the instantiation: a block of
# 16 elements takes 4 lanes (fp32) or 8 (16-bit), so a wave covers 16 or 8 blocks a round and NB = 1 is
# <IO, 1>, NB = 9 in bf16 two rounds, <IO, 2>. At BL = 16, the shortest block the suite uses, 64 bf16 blocks
# are the wave path's last row (8 rounds) and 65 the group path's first.
@pytest.mark.parametrize("dtype,NB,path,stride,shift", [("fp32", 1, "PATH_WAVE", MAX_GRID * WAVE_ROWS, 1),
                                                        ("bf16", 1, "PATH_WAVE", MAX_GRID * WAVE_ROWS, 0),
                                                        ("bf16", 9, "PATH_WAVE", MAX_GRID * WAVE_ROWS, 1),
                                                        ("bf16", 65, "PATH_GROUP", MAX_GRID, 1)],
                         ids=["wave1-fp32", "wave1-bf16", "wave2-bf16", "group-bf16"])
def test_rows_past_the_grid_cap(dtype, NB, path, stride, shift):
    """The second trip of the grid-stride row loop of bq_wave<IO, 1>, bq_wave<IO, 2> and bq_group<IO, true>:
    three rows more than the capped grid covers in one trip, out of place into a table and an output that
    hold a sentinel, the base `shift` elements past 16 bytes. The host restatement runs on TILE distinct
    rows, among them an all-zero and a constant block; row r of the tensor is row r mod TILE of them, and
    the two special rows are the first two past the cap.

    bq_group<IO, false> (PATH_TWO_PASS) is not here. Its smallest row is 1023 bf16 blocks of 16 elements,
    32736 bytes (the 64 KiB of LDS less 32 bytes a block, at most 1024 blocks a row), so the 65537 rows
    of a second trip are 2.1 GB, and 1 GB of such rows is 30547 rows: no second trip."""
    from aimet_amd import _native, blockwise as B
    BL, bw, flags = 16, 4, SYMMETRY["asymmetric"]
    td = DTYPES[dtype]
    assert B.row_path(NB, BL, td) == getattr(B, path) and stride % TILE != 0
    if NB == 65:
        assert B.row_path(NB - 1, BL, td) == B.PATH_WAVE
    R = stride + 3
    rng = np.random.default_rng(NB)
    x, x32 = data(rng, TILE * NB * BL, td)
    x, x32 = x.view(TILE, NB, BL), x32.reshape(TILE, NB, BL)
    x[stride % TILE, 0], x32[stride % TILE, 0] = 0.0, 0.0
    x[(stride + 1) % TILE, NB - 1], x32[(stride + 1) % TILE, NB - 1] = 1.25, 1.25
    want_t = table_of(host_encodings(x32.ravel(), TILE * NB, BL, bw, *flags))
    want_y = host_qdq(x32.ravel(), want_t, td).view(TILE, NB * BL)
    tile = torch.arange(R) % TILE
    want_t = torch.from_numpy(want_t).view(4, TILE, NB)[:, tile].reshape(4, R * NB)
    want_y = want_y[tile].ravel()
    n = R * NB * BL
    src = torch.empty(n + 1, dtype=td, device="cuda")[shift:shift + n].copy_(x.view(TILE, NB * BL)[tile].ravel())
    dst = torch.full((n + 1,), SENTINEL, dtype=td, device="cuda")[shift:shift + n]
    table = torch.full((4, R * NB), SENTINEL, dtype=torch.float32, device="cuda")
    _native.call("aimet_bq_encode_qdq", src.data_ptr(), dst.data_ptr(), R, NB, BL, _native.IO_CODES[td], bw,
                 *(int(f) for f in flags), 0, table.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream)
    got_t, got_y = table.cpu(), dst.cpu()
    # the second trip first: rows it leaves unwritten hold the sentinel
    np.testing.assert_array_equal(raw(got_y[stride * NB * BL:]), raw(want_y[stride * NB * BL:]))
    np.testing.assert_array_equal(raw(got_t[:, stride * NB:]), raw(want_t[:, stride * NB:]))
    assert np.array_equal(raw(got_y), raw(want_y))
    assert np.array_equal(raw(got_t), raw(want_t))


@pytest.mark.parametrize("sym", list(SYMMETRY))
def test_kernel_degenerate_blocks(sym):
    """Blocks that are all zero, all positive, all negative and constant, among random ones."""
    rng = np.random.default_rng(3)
    R, NB, BL = 5, 7, 16
    x32 = rng.standard_normal((R * NB, BL)).astype(np.float32)
    x32[0], x32[9], x32[17], x32[25], x32[34] = 0.0, np.abs(x32[9]) + 0.5, -np.abs(x32[17]) - 0.5, 1.25, -0.003
    x32 = x32.ravel()
    want_t = table_of(host_encodings(x32, R * NB, BL, 4, *SYMMETRY[sym]))
    got_t, got_y, _, _ = device_run(torch.from_numpy(x32), R, NB, BL, 4, SYMMETRY[sym], "out", 0)
    np.testing.assert_array_equal(bits(got_t), bits(want_t))
    np.testing.assert_array_equal(raw(got_y), raw(host_qdq(x32, want_t, torch.float32)))


@pytest.mark.parametrize("NB,BL,R", [(7, 16, 5), (33, 64, 2)])
@pytest.mark.parametrize("bw,dbw", [(4, 8), (4, 6)])
def test_lpbq_matches_host_lpbq(bw, dbw, NB, BL, R):
    """q, factor and the table against aimet_amd.lpbq on the uncompressed host encodings. Row 0 has a
    block far more than 2^scale_bitwidth below the row's largest scale (q clips to 1); row 1 has block
    maxima 7 m (7 positive steps at 4 bits, so delta = m exactly) with the row maximum a power of two,
    so delta / factor is exactly k + 0.5 for even and odd k (ties go to even)."""
    from aimet_amd import lpbq
    rng = np.random.default_rng(NB)
    sbw = dbw - bw
    x32 = (rng.standard_normal((R, NB, BL)) * 0.5).astype(np.float32)
    x32[0, 0] *= 1e-4
    x32[0, 1, 0] = 40.0
    x32[1] = np.clip(x32[1], -1, 1)
    unit = 7.0 * 2 ** (5 - sbw)          # factor = 2^(5 - sbw), so delta / factor = absmax / unit
    x32[1, 0, 0] = unit * 2 ** sbw       # the row maximum 7 * 32: q = 2^sbw
    for k in range(4):                   # k + 0.5 stays below 2^sbw, the row maximum's quotient
        x32[1, k + 1, k] = -unit * (k + 0.5)
    x32 = x32.ravel()
    flags = SYMMETRY["symmetric"]
    encs = host_encodings(x32, R * NB, BL, bw, *flags)
    want = lpbq.compress_encoding_scales(encs, [R, NB], [1, -1], sbw)
    scale, _ = lpbq.encodings_to_scale_offset_arrays(encs, (R, NB))
    want_q, want_f = lpbq.grouped_dynamic_quantize(scale, [1, -1], sbw)
    assert want_q[0, 0] == 1 and want_q[1, 1:5].tolist() == [1, 2, 2, 4]
    got_t, got_y, q, factor = device_run(torch.from_numpy(x32), R, NB, BL, bw, flags, "out", 0, sbw)
    np.testing.assert_array_equal(q.cpu().numpy(), want_q.ravel())
    np.testing.assert_array_equal(factor.cpu().numpy(), want_f.ravel())
    np.testing.assert_array_equal(bits(got_t), bits(table_of(want)))
    np.testing.assert_array_equal(raw(got_y), raw(host_qdq(x32, table_of(want), torch.float32)))


# ---- the sim -------------------------------------------------------------------------------------------
class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = torch.nn.Linear(16, 8)
        self.conv = torch.nn.Conv2d(8, 4, 3)
        self.fc2 = torch.nn.Linear(36, 6)
        self.odd = torch.nn.Linear(10, 6)   # block size 4 does not divide its input features

    def forward(self, x):   # [B, 25, 16]
        y = self.fc1(x).transpose(1, 2).reshape(-1, 8, 5, 5)
        return self.fc2(self.conv(y).flatten(1)) + self.odd(x[:, 0, :10])


BLOCKWISE = ("fc1", "conv", "fc2")
PER_CHANNEL = {"defaults": {"per_channel_quantization": "True", "params": {"is_symmetric": "True"}}}


def make_sim(model, grouped, **kw):
    from aimet_amd import blockwise as B
    from aimet_amd.quantsim import QuantizationSimModel
    sim = QuantizationSimModel(model, config_file=PER_CHANNEL, default_param_bw=8, **kw)
    for _, w in sim.quant_wrappers():
        w.enable_activation_quantizers(False)
    types = (torch.nn.Linear, torch.nn.Conv2d)
    if grouped:
        B.set_grouped_blockwise_quantization_for_weights(sim, types, 4, 8, 4)
    else:
        B.set_blockwise_quantization_for_weights(sim, types, 4, True, 4)
    return sim


@pytest.mark.parametrize("grouped", [False, True], ids=["blockwise", "lpbq"])
def test_sim_blockwise(grouped, tmp_path):
    from aimet_amd import blockwise as B, lpbq
    from aimet_amd.quantizers import StaticGridPerChannelQuantizer
    torch.manual_seed(0)
    model = Net().cuda().eval()
    # requires_grad: the wrapper gates a layer's weight gradient when the backward pass reaches its input
    x = torch.randn(3, 25, 16, device="cuda", requires_grad=True)
    sim = make_sim(model, grouped)
    quantizers = {n: getattr(sim.model, n).param_quantizers["weight"] for n in BLOCKWISE + ("odd",)}
    assert all(isinstance(quantizers[n], B.BlockwiseQuantizer) for n in BLOCKWISE)
    assert type(quantizers["odd"]) is StaticGridPerChannelQuantizer
    with pytest.raises(ValueError, match="odd"):
        B.set_blockwise_quantization_for_weights(make_sim(model, grouped), torch.nn.Linear, 4, True, 4, strict=True)

    B.launch_count(reset=True)
    sim.compute_encodings(lambda m, _: m(x))
    assert B.launch_count() == len(BLOCKWISE)

    # the same model with host-QDQ'd weights (the odd layer's from its own per-channel quantizer)
    ref = copy.deepcopy(model)
    tables = {}
    for n in BLOCKWISE:
        w = getattr(model, n).weight.detach().cpu().numpy().ravel()
        q = quantizers[n]
        encs = host_encodings(w, q.num_encodings, q.BL, 4, True, False, False)
        if grouped:
            encs = lpbq.compress_encoding_scales(encs, [q.R, q.NB], [1, -1], 4)
        tables[n] = table_of(encs)
        np.testing.assert_array_equal(bits(q.table.cpu().numpy()), bits(tables[n]), err_msg=n)
        getattr(ref, n).weight.data = host_qdq(w, tables[n], torch.float32).view(q.shape).cuda()
    ref.odd.weight.data = quantizers["odd"].quantize_dequantize(model.odd.weight.detach(), "nearest")
    want = ref(x)
    got = sim.model(x)
    np.testing.assert_array_equal(raw(got), raw(want))

    # weight gradients: grad * (min_b <= w <= max_b), grad being what reaches the weight (a tensor hook
    # sees it before the wrapper gates it)
    reached = {}
    for n in BLOCKWISE:
        getattr(sim.model, n).weight.register_hook(lambda g, n=n: reached.__setitem__(n, g.clone()))
    got.sum().backward()
    for n in BLOCKWISE:
        w = getattr(model, n).weight.detach().cpu().numpy().reshape(-1, quantizers[n].BL)
        mask = (tables[n][0][:, None] <= w) & (w <= tables[n][1][:, None])
        assert not (grouped and mask.all())   # compressed scales leave weights outside their block's range
        g = reached[n].cpu().numpy().reshape(w.shape) * mask
        np.testing.assert_array_equal(bits(getattr(sim.model, n).weight.grad.cpu().numpy().ravel()), bits(g.ravel()),
                                      err_msg=n)

    # export, then load into a fresh sim: no calibration pass, the same table and forward
    path = sim.export(str(tmp_path), "bq")
    entry = json.load(open(path))["param_encodings"]["conv.weight"]
    assert len(entry) == 4 * 2 and entry[0]["block_size"] == 4
    assert ("per_block_int_scale" in entry[0]) == ("compressed_bw" in entry[0]) == grouped
    fresh = make_sim(model, grouped)
    B.launch_count(reset=True)
    fresh.load_encodings(path)
    for n in BLOCKWISE:
        np.testing.assert_array_equal(bits(getattr(fresh.model, n).param_quantizers["weight"].table.cpu().numpy()),
                                      bits(tables[n]), err_msg=n)
    with torch.no_grad():
        np.testing.assert_array_equal(raw(fresh.model(x)), raw(want))
    assert B.launch_count() == 0


@pytest.mark.parametrize("grouped", [False, True], ids=["blockwise", "lpbq"])
def test_sim_range_learning_refused(grouped):
    from aimet_amd.quantizers import QuantScheme
    with pytest.raises(NotImplementedError):
        make_sim(Net().cuda(), grouped, quant_scheme=QuantScheme.training_range_learning_with_tf_init)
