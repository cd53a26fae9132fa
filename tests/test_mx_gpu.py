"""MX fake-quantization on the device (csrc/mx.hip, aimet_amd.mx) against a float64 restatement of the
contract in that file's header. Every step of the contract is exact, so every comparison is value
equality with NaNs in the same places."""
import json

import numpy as np
import pytest

from conftest import gpu_available

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd.mx import (MxFormat, MxQuantizer, mx_dequantize, mx_quantize, mx_quantize_dequantize,  # noqa: E402
                          set_mx_quantization)

SPEC = {MxFormat.MXFP8_E4M3: (3, -6, 8, 448.0), MxFormat.MXFP8_E5M2: (2, -14, 15, 57344.0),
        MxFormat.MXFP6_E3M2: (2, -2, 4, 28.0), MxFormat.MXFP6_E2M3: (3, 0, 2, 7.5),
        MxFormat.MXFP4_E2M1: (1, 0, 2, 6.0)}   # M, emin, emax, max normal
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
FORMATS = pytest.mark.parametrize("fmt", list(MxFormat), ids=lambda f: f.name)
TWO = torch.tensor(2.0, dtype=torch.float64)


def floor_log2(a):
    return torch.frexp(a)[1] - 1   # a = m 2^e with 0.5 <= m < 1


def ref_parts(x, fmt, axis=-1):
    """(p, s, bad) of the contract for a CPU tensor: element values before the scale, the exponent s of
    every block and which blocks hold a NaN or an Inf; blocks on the last two axes [..., K / 32, 32]."""
    M, emin, emax, maxn = SPEC[fmt]
    v = x.to(torch.float64).movedim(axis, -1)
    b = v.reshape(*v.shape[:-1], -1, 32)
    bad = ~torch.isfinite(b).all(-1, keepdim=True)
    a = torch.where(bad, 1.0, b.abs()).amax(-1, keepdim=True)
    s = torch.where(a == 0, -127, (floor_log2(a) - emax).clamp(-127, 127))
    y = torch.where(bad, 0.0, b) / TWO.pow(s)
    step = TWO.pow(floor_log2(y.abs()).clamp(min=emin) - M)
    p = (torch.round(y / step) * step).clamp(-maxn, maxn)   # torch.round: ties to even
    return p, s, bad


def ref_qdq(x, fmt, axis=-1):
    p, s, bad = ref_parts(x, fmt, axis)
    out = torch.where(bad, float("nan"), p * TWO.pow(s))
    moved = x.movedim(axis, -1).shape
    return out.reshape(moved).movedim(-1, axis).to(x.dtype)   # float32-exact, so one rounding to 16 bits


def ref_pack(x, fmt):
    """(scale bytes, code bytes) of a [rows, K] tensor as numpy uint8 arrays."""
    M, emin, _, _ = SPEC[fmt]
    w = fmt.element_bits
    p, s, bad = ref_parts(x, fmt)
    g = p.abs()
    E = floor_log2(g)
    normal = ((E - emin + 1) << M) + ((g / TWO.pow(E) - 1) * 2 ** M).long()
    mag = torch.where(g < 2.0 ** emin, (g * 2.0 ** (M - emin)).long(), normal)
    code = torch.where(bad, 0, (torch.signbit(p).long() << (w - 1)) | mag).reshape(x.shape[0], -1).numpy()
    onebits = ((code[:, :, None] >> np.arange(w)) & 1).astype(np.uint8).reshape(x.shape[0], -1)
    scales = torch.where(bad, 255, s + 127).reshape(x.shape[0], -1).numpy().astype(np.uint8)
    return scales, np.packbits(onebits, axis=1, bitorder="little")


def grid_block(fmt):
    """A block whose scale is 1: values just above the max normal (saturation) and the exact midpoints
    between neighbouring grid values, signs alternating (ties to even)."""
    M, emin, emax, maxn = SPEC[fmt]
    grid = sorted({m * 2.0 ** (emin - M) for m in range(2 ** M)} |
                  {(1 + m / 2 ** M) * 2.0 ** e for e in range(emin, emax + 1) for m in range(2 ** M)})
    grid = [g for g in grid if g <= maxn]
    mid = [(lo + hi) / 2 for lo, hi in zip(grid, grid[1:])]
    picked = [mid[i * len(mid) // 30] * (-1) ** i for i in range(30)]
    return torch.tensor([maxn * 1.0625, -maxn * 1.0625] + picked, dtype=torch.float64)


def variants(shape, fmt, dtype, seed):
    """Inputs [V, outer, K, inner] of `dtype`: normals times a power of two per block, each variant with
    one special block written over block (variant index mod blocks)."""
    outer, K, inner = shape
    g = torch.Generator().manual_seed(seed)
    span = 10 if dtype == torch.float16 else 20
    finfo = torch.finfo(dtype)
    one_max = torch.randn(32, generator=g, dtype=torch.float64)
    one_max[5] = finfo.max
    nan, inf = one_max.clone(), one_max.clone()
    nan[17], inf[30] = float("nan"), float("-inf")
    special = [torch.zeros(32, dtype=torch.float64), one_max, nan, inf, grid_block(fmt)]
    if dtype == torch.float32:
        special.append(torch.randn(32, generator=g, dtype=torch.float64) * 1e-40)   # float32 denormals only
    xs = []
    for i, block in enumerate(special):
        scale = TWO.pow(torch.randint(-span, span + 1, (outer, K // 32, 1, inner), generator=g))
        x = torch.randn(outer, K // 32, 32, inner, generator=g, dtype=torch.float64) * scale
        nb = outer * (K // 32) * inner
        o, rest = divmod(i % nb, (K // 32) * inner)
        x[o, rest // inner, :, rest % inner] = block
        xs.append(x.reshape(outer, K, inner).to(dtype))
    return torch.stack(xs)


def same(got, want):
    got, want = got.cpu(), want.cpu()
    return torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))


SHAPES = [(1, 32, 1), (3, 96, 1), (5, 64, 1), (2, 64, 9), (2, 32, 64), (1, 64, 65), (3, 32, 130)]


@FORMATS
@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("shape", SHAPES + ["view"], ids=str)
def test_qdq(fmt, dtype, shape):
    """Both forms, out of place and in place; "view": a row-form tensor whose base is one element past
    a 16-byte boundary (the element-access path)."""
    view = shape == "view"
    xs = variants((3, 96, 1) if view else shape, fmt, dtype, seed=len(str(shape)) + fmt.value)
    want = ref_qdq(xs, fmt, axis=2)
    for x, w in zip(xs, want):
        n = x.numel()
        dev = torch.empty(n + 8, dtype=dtype, device="cuda")[int(view):int(view) + n].view(x.shape).copy_(x)
        assert dev.data_ptr() % 16 == (dev.element_size() if view else 0)
        got = mx_quantize_dequantize(dev, fmt, axis=1)
        assert got.dtype == dtype and same(got, w)
        assert mx_quantize_dequantize(dev, fmt, axis=1, out=dev) is dev and same(dev, w)


@FORMATS
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,K", [(1, 32), (3, 96)])
def test_pack_unpack(fmt, dtype, rows, K):
    for x in variants((rows, K, 1), fmt, dtype, seed=7 + fmt.value).squeeze(-1):
        dev = x.cuda()
        scales, codes = mx_quantize(dev, fmt)
        want_scales, want_codes = ref_pack(x, fmt)
        assert scales.shape == (rows, K // 32) and codes.shape == (rows, K * fmt.element_bits // 8)
        np.testing.assert_array_equal(scales.cpu().numpy(), want_scales)
        np.testing.assert_array_equal(codes.cpu().numpy(), want_codes)
        back = mx_dequantize(scales, codes, fmt, dtype)
        assert back.dtype == dtype and same(back, mx_quantize_dequantize(dev, fmt)) and same(back, ref_qdq(x, fmt))


# stream_blocks (common.hpp:109) caps these launches at kMaxStreamBlocks = 2048 workgroups (common.hpp:28)
# of kBlock = 256 lanes: lane slots (8 elements of the row kernels, a block of the column kernel) past
# 524288 are a second trip of the loop (MX_ROW_LOOP, mx.hip:225; mx.hip:318).
MAX_SLOTS = 2048 * 256
TILE = 257   # a prime that divides neither stride: blocks one stride apart never hold equal data
SENTINEL = -777.25   # more significant bits than any element format has, also once a 16-bit type rounded it


def tiled_blocks(fmt, dtype, first_past, blocks):
    """`blocks` blocks of 32, block i being block i mod TILE of TILE distinct ones: (the distinct ones
    [TILE, 32], i mod TILE [blocks]). Blocks `first_past` .. `first_past` + 3 are a NaN block, a zero
    block, an Inf block and the grid block."""
    assert first_past % TILE != 0 and first_past < blocks
    base = variants((TILE, 32, 1), fmt, dtype, seed=first_past)[0].squeeze(-1)   # the variant with a zero block
    g = torch.Generator().manual_seed(1)
    nan, inf = (torch.randn(32, generator=g, dtype=torch.float64) for _ in range(2))
    nan[17], inf[30] = float("nan"), float("-inf")
    special = [nan, torch.zeros(32, dtype=torch.float64), inf, grid_block(fmt)]
    for i, block in enumerate(special):
        base[(first_past + i) % TILE] = block.to(dtype)
    return base, torch.arange(blocks) % TILE


def row_kernels_past_the_grid_cap(dtype):
    """The second trip of MX_ROW_LOOP in mx_row_qdq, mx_row_pack and mx_row_unpack: 12 lane slots (three
    blocks) more than the capped grid covers in one trip, every output holding a sentinel before the
    launch. The reference runs on TILE distinct blocks; the first blocks past the cap are the special ones."""
    from aimet_amd import _native
    fmt, K, k = MxFormat.MXFP4_E2M1, 32, 3
    rows = (MAX_SLOTS + 4 * k) // 4
    n = rows * K
    assert n // 8 == MAX_SLOTS + 4 * k and MAX_SLOTS % TILE != 0
    base, tile = tiled_blocks(fmt, dtype, MAX_SLOTS // 4, rows)
    want = ref_qdq(base, fmt)[tile]
    scales, codes = (torch.from_numpy(a)[tile] for a in ref_pack(base, fmt))
    past = MAX_SLOTS // 4   # the first row of the second trip
    assert want[past].isnan().all() and not want[past + 1].any() and want[past + 2].isnan().all()
    dev = base[tile].cuda()
    stream, io = torch.cuda.current_stream().cuda_stream, _native.IO_CODES[dtype]

    out = torch.full_like(dev, SENTINEL)
    assert mx_quantize_dequantize(dev, fmt, out=out) is out
    assert same(out[past:], want[past:]) and same(out, want)

    got_scales, got_codes = torch.full_like(scales, 0xA5).cuda(), torch.full_like(codes, 0xA5).cuda()
    assert not (scales == 0xA5).any() and not (codes.view(torch.int32) == 0xA5A5A5A5 - (1 << 32)).any()
    _native.call("aimet_mx_quantize", dev.data_ptr(), got_scales.data_ptr(), got_codes.data_ptr(), rows, K, io,
                 fmt.value, stream)
    assert torch.equal(got_scales.cpu()[past:], scales[past:]) and torch.equal(got_scales.cpu(), scales)
    assert torch.equal(got_codes.cpu()[past:], codes[past:]) and torch.equal(got_codes.cpu(), codes)

    back = torch.full_like(dev, SENTINEL)
    _native.call("aimet_mx_dequantize", got_scales.data_ptr(), got_codes.data_ptr(), back.data_ptr(), rows, K, io,
                 fmt.value, stream)
    assert same(back[past:], want[past:]) and same(back, want)


def column_kernel_past_the_grid_cap(dtype):
    """The second trip of mx_col_qdq's loop: a [58255, 32, 9] tensor, 7 lane slots (blocks) more
    than the capped grid covers in one trip, into an output that holds a sentinel. Lane slot j is block
    j mod TILE of TILE distinct ones; the first blocks past the cap are the special ones."""
    fmt, outer, K, inner = MxFormat.MXFP8_E4M3, 58255, 32, 9
    slots = outer * inner
    assert slots == outer * K * inner // 32 == MAX_SLOTS + 7 and MAX_SLOTS % TILE != 0
    base, tile = tiled_blocks(fmt, dtype, MAX_SLOTS, slots)

    def spread(blocks):   # [TILE, 32] -> [outer, K, inner], slot j = (outer index, inner index)
        return blocks[tile].view(outer, inner, K).transpose(1, 2).contiguous()
    want = spread(ref_qdq(base, fmt))
    dev = spread(base).cuda()
    assert want[-1, :, 2].isnan().all() and not want[-1, :, 3].any()   # slots MAX_SLOTS and MAX_SLOTS + 1
    out = torch.full_like(dev, SENTINEL)
    assert mx_quantize_dequantize(dev, fmt, axis=1, out=out) is out
    assert same(out[-1, :, 2:], want[-1, :, 2:]) and same(out, want)


@pytest.mark.parametrize("case,dtype", [(row_kernels_past_the_grid_cap, torch.float32),
                                        (row_kernels_past_the_grid_cap, torch.bfloat16),
                                        (column_kernel_past_the_grid_cap, torch.bfloat16)],
                         ids=["row-fp32", "row-bf16", "column-bf16"])
def test_kernels_past_the_grid_cap(case, dtype):
    case(dtype)


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(32, 4, 3)
        self.fc = torch.nn.Linear(64, 8)
        self.odd = torch.nn.Linear(48, 8)

    def forward(self, x):
        h = self.conv(x).flatten(1)
        return self.fc(h) + self.odd(h[:, :48])


def test_sim(tmp_path):
    from aimet_amd.quantsim import QuantizationSimModel
    F = torch.nn.functional
    torch.manual_seed(0)
    model = Net().cuda().eval()
    x = torch.randn(2, 32, 6, 6, device="cuda")
    sim = QuantizationSimModel(model, dummy_input=x)
    for _, w in sim.quant_wrappers():
        w.enable_activation_quantizers(False)
        w.param_quantizers["bias"].enabled = False
    old = sim.model.odd.param_quantizers["weight"]
    with pytest.warns(UserWarning, match="odd") as caught:
        done = set_mx_quantization(sim, (torch.nn.Linear, torch.nn.Conv2d), MxFormat.MXFP4_E2M1, MxFormat.MXFP8_E4M3)
    assert sorted(done) == ["conv", "fc"] and len([w for w in caught if "set_mx_quantization" in str(w.message)]) == 1
    assert sim.model.odd.param_quantizers["weight"] is old and not isinstance(old, MxQuantizer)
    sim.compute_encodings(lambda m, _: m(x))

    seen = {}

    def keep(name):
        def hook(module, inputs, output):
            output.retain_grad()
            seen[name] = (inputs[0], output)
        return hook
    hooks = [getattr(sim.model, n).register_forward_hook(keep(n)) for n in ("conv", "fc")]
    sim.model(x).sum().backward()
    for h in hooks:
        h.remove()
    for n, op, axis in (("conv", F.conv2d, 1), ("fc", F.linear, -1)):
        wrapper, (inp, out) = getattr(sim.model, n), seen[n]
        assert isinstance(wrapper.param_quantizers["weight"], MxQuantizer) and wrapper.input_quantizers[0].enabled
        layer = wrapper._module_to_wrap   # the sim works on a copy of the model
        wq = ref_qdq(layer.weight.detach().cpu(), MxFormat.MXFP4_E2M1, 1).cuda().requires_grad_()
        want = op(ref_qdq(inp.detach().cpu(), MxFormat.MXFP8_E4M3, axis).cuda(), wq, layer.bias.detach())
        assert torch.equal(out, want), n
        want.backward(out.grad)   # identity STE: the gradient with respect to the quantized weight
        assert torch.equal(layer.weight.grad, wq.grad), n

    with open(sim.export(str(tmp_path), "mx")) as f:
        enc = json.load(f)
    entry = {"dtype": "float", "block_size": 32}
    assert enc["param_encodings"]["fc.weight"] == [dict(entry, bitwidth=4, format="MXFP4_E2M1", axis=1)]
    assert enc["param_encodings"]["conv.weight"] == [dict(entry, bitwidth=4, format="MXFP4_E2M1", axis=1)]
    assert enc["activation_encodings"]["fc"]["input"]["0"] == dict(entry, bitwidth=8, format="MXFP8_E4M3", axis=-1)
    assert enc["activation_encodings"]["conv"]["input"]["0"] == dict(entry, bitwidth=8, format="MXFP8_E4M3", axis=1)
