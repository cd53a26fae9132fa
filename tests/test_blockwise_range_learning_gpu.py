"""Learned blockwise ranges (aimet_lg_block_forward / _backward, aimet_amd.learned_grid, aimet_amd.blockwise).

The reference is oracle.torch_ref on the CPU over x.view(E, BL) with ch_axis = 0: y (cast once to the
output dtype) and grad_x are compared bit for bit; the range gradients are sums, held to LGB_BOUND_C
units of 2^-24 x the sum of |terms| around their exact float64 value (lg_encoding_grads_bound).

LGB_BOUND_C. On short blocks the roundings of the final combination dominate, not the sum, so the
bar is not test_gpu_parity's 2: over the inputs of the kernel and grid-loop tests below (computed on
the CPU before any device run) the float32 restatement T.lg_gradients itself reaches 4.12 units (the
grid loop's 524,325 blocks of 16, asymmetric; 2.90 over the small shapes); the bar is twice that,
rounded up to one decimal, since the kernel folds the same float32 terms in another order and either
order can be the unlucky one. The restatement is asserted against the same bar.
Measured on an MI355X: the kernels reach 3.50 there and 2.90 over the small shapes.
"""
import itertools
import json

import numpy as np
import pytest

from conftest import bits, gpu_available
from oracle import torch_ref as T
from test_blockwise_sim_gpu import SYMMETRY

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

LGB_BOUND_C = 8.3
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def raw(t):
    """Bit patterns of a float32 / 16-bit tensor, NaNs as NaN-ness (conftest.bits). A 16-bit tensor is
    compared through its exact float32 upcast, which keeps every other pattern apart: torch's CPU
    cast of a NaN to bfloat16 gives 0x7FC0 or 0xFFFF depending on whether the element fell into the
    vectorised part of the loop."""
    return bits(t.detach().cpu().float().contiguous().numpy())


def blocks(rng, E, BL, dtype):
    """x [E, BL] ~ N(0.1, 0.7), a gradient of `dtype`, and ranges 0.8 x each block's min / max."""
    x = torch.from_numpy((rng.standard_normal((E, BL)) * 0.7 + 0.1).astype(np.float32))
    grad = torch.from_numpy(rng.standard_normal((E, BL)).astype(np.float32)).to(dtype)
    return x, grad, x.amin(1) * 0.8, x.amax(1) * 0.8


def reference(x, grad, emin, emax, bw, flags, dtype):
    """(y in dtype, grad_x, float32 restatement's range gradients, exact ones, their units)."""
    g = grad.float()
    y = T.lg_forward(x, emin, emax, bw, *flags)[0].to(dtype)
    gx, gmin, gmax = T.lg_gradients(x, g, emin, emax, bw, *flags)
    return y, gx, (gmin, gmax), T.lg_encoding_grads_bound(x, g, emin, emax, bw, *flags)


def device(x, grad, emin, emax, bw, flags, dtype, shift=0, want_gx=True):
    """The block op on the device, x and grad placed `shift` elements into their buffers."""
    from aimet_amd.learned_grid import LearnedGridBlockQuantizeDequantize as Op
    n = x.numel()
    xd = torch.empty(n + 1, device="cuda")[shift:shift + n].copy_(x.reshape(-1)).view(x.shape).requires_grad_(want_gx)
    gd = torch.empty(n + 1, dtype=grad.dtype, device="cuda")[shift:shift + n].copy_(grad.reshape(-1)).view(x.shape)
    lo, hi = emin.cuda().requires_grad_(True), emax.cuda().requires_grad_(True)
    y = Op.apply(xd, lo, hi, x.shape[1], bw, *flags, dtype if dtype != torch.float32 else None)
    y.backward(gd)
    return y, xd.grad, lo.grad, hi.grad


def check(got, want, what, bound=True):
    y, gx, restated, (ex_min, ex_max, b_min, b_max) = want
    np.testing.assert_array_equal(raw(got[0]), raw(y), err_msg="y %s" % what)
    np.testing.assert_array_equal(raw(got[1]), raw(gx), err_msg="grad_x %s" % what)
    if bound:
        for ours, ref, ex, b, end in ((got[2], restated[0], ex_min, b_min, "grad_min"),
                                      (got[3], restated[1], ex_max, b_max, "grad_max")):
            T.assert_within_sum_bound(ref, ex, b, LGB_BOUND_C, "block restatement %s %s" % (end, what))
            T.assert_within_sum_bound(ours, ex, b, LGB_BOUND_C, "block kernel %s %s" % (end, what))


# SEG 1, the element path, a sub-wave segment, the Llama block, a vector count that is no power of
# two, two passes of a whole wave, four
@pytest.mark.parametrize("BL", [4, 9, 16, 64, 96, 288, 1024])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_block_kernels_match_reference(dtype, BL):
    rng = np.random.default_rng(BL)
    first = True
    for NB, R in itertools.product((1, 3, 7), (1, 5)):
        x, grad, emin, emax = blocks(rng, R * NB, BL, DTYPES[dtype])
        for (name, flags), bw in itertools.product(SYMMETRY.items(), (4, 8)):
            want = reference(x, grad, emin, emax, bw, flags, DTYPES[dtype])
            for shift in (0, 1):   # 1: off the vector alignment, the element path
                got = device(x, grad, emin, emax, bw, flags, DTYPES[dtype], shift)
                check(got, want, str((BL, dtype, NB, R, name, bw, shift)))
            if first:   # grad_x not requested: the same range gradients
                lean = device(x, grad, emin, emax, bw, flags, DTYPES[dtype], 0, want_gx=False)
                assert lean[1] is None
                np.testing.assert_array_equal(raw(lean[2]), raw(got[2]))
                np.testing.assert_array_equal(raw(lean[3]), raw(got[3]))
                first = False


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_block_kernels_loop_over_the_grid(dtype):
    from aimet_amd.learned_grid import block_round
    BL = 16
    E = block_round(BL, DTYPES[dtype]) + 37
    x, grad, emin, emax = blocks(np.random.default_rng(1), E, BL, DTYPES[dtype])
    flags = SYMMETRY["asymmetric"]
    want = reference(x, grad, emin, emax, 4, flags, DTYPES[dtype])
    check(device(x, grad, emin, emax, 4, flags, DTYPES[dtype]), want, "grid loop " + dtype)


@pytest.mark.parametrize("sym", list(SYMMETRY))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_block_kernels_edge_blocks(dtype, sym):
    """Among random blocks: an all-zero gradient, every element clipped above, a range at the gate's
    floor, a NaN and a +-inf element. y and grad_x bit for bit (the sums of such blocks are NaN)."""
    E, BL = 35, 64
    x, grad, emin, emax = blocks(np.random.default_rng(7), E, BL, DTYPES[dtype])
    grad[3] = 0
    x[9] = x[9].abs() + 100.0
    emin[17], emax[17] = -0.25, -0.25 + 1e-5
    x[25, 5], x[26, 0], x[26, 63] = float("nan"), float("inf"), float("-inf")
    want = reference(x, grad, emin, emax, 4, SYMMETRY[sym], DTYPES[dtype])
    for shift in (0, 1):
        check(device(x, grad, emin, emax, 4, SYMMETRY[sym], DTYPES[dtype], shift), want, "edge %d" % shift, bound=False)


# ---- the sim -------------------------------------------------------------------------------------------
class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(16, 8)
        self.conv = torch.nn.Conv2d(8, 4, 3)

    def forward(self, x):   # [B, 25, 16]
        return self.conv(self.fc(x).transpose(1, 2).reshape(-1, 8, 5, 5))


def test_sim_learns_blockwise_ranges(tmp_path):
    from aimet_amd import blockwise as B
    from aimet_amd.quantizers import QuantScheme
    from aimet_amd.quantsim import QuantizationSimModel
    from test_blockwise_sim_gpu import PER_CHANNEL
    torch.manual_seed(0)
    model = Net().cuda()
    x = torch.randn(3, 25, 16, device="cuda", requires_grad=True)
    types = (torch.nn.Linear, torch.nn.Conv2d)

    def make(scheme):
        sim = QuantizationSimModel(model, config_file=PER_CHANNEL, default_param_bw=8, quant_scheme=scheme)
        for _, w in sim.quant_wrappers():
            w.enable_activation_quantizers(False)
        return sim

    sim = make(QuantScheme.training_range_learning_with_tf_init)
    with pytest.raises(NotImplementedError):
        B.set_grouped_blockwise_quantization_for_weights(sim, types, 4, 8, 4, learn_ranges=True)
    with pytest.raises(ValueError):
        B.set_blockwise_quantization_for_weights(make(QuantScheme.post_training_tf), types, 4, True, 4,
                                                 learn_ranges=True)
    assert B.set_blockwise_quantization_for_weights(sim, types, 4, True, 4, learn_ranges=True) == ["fc", "conv"]
    tables = {}
    for n in ("fc", "conv"):   # the static quantizers are replaced by compute_encodings: keep them
        tables[n] = getattr(sim.model, n).param_quantizers["weight"]
    sim.compute_encodings(lambda m, _: m(x))

    # the trainable ranges: the calibrated table's columns, min = -max for the symmetric grid
    for n, E, BL in (("fc", 8 * 4, 4), ("conv", 4 * 2, 36)):
        w = getattr(sim.model, n)
        q = w.param_quantizers["weight"]
        assert isinstance(q, B.LearnedBlockwiseQuantizer) and (q.num_encodings, q.BL) == (E, BL)
        assert w.weight_encoding_min.shape == w.weight_encoding_max.shape == (E,)
        np.testing.assert_array_equal(raw(w.weight_encoding_max), raw(tables[n].table[1]))
        np.testing.assert_array_equal(raw(w.weight_encoding_min), raw(-tables[n].table[1]))

    # one step under autocast: the gradients against the oracle on what reached the quantized weights (a
    # pre-hook of the wrapped layer sees the quantized weight in the parameter's place)
    reached, handles = {}, []
    for n in ("fc", "conv"):
        handles.append(getattr(sim.model, n)._module_to_wrap.register_forward_pre_hook(
            lambda m, _, n=n: m.weight.register_hook(lambda g: reached.__setitem__(n, g.clone())) and None))
    params = [p for n, p in sim.model.named_parameters() if "encoding" in n]
    opt = torch.optim.SGD(params, lr=1e-2)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        sim.model(x).float().square().sum().backward()
    for h in handles:
        h.remove()
    assert reached["fc"].dtype == torch.bfloat16   # the Linear's cast is fused: its gradient arrives in 16 bits
    before = {}
    for n in ("fc", "conv"):
        w = getattr(sim.model, n)
        W = w.weight.detach().cpu().reshape(w.weight_encoding_min.numel(), -1)
        lo, hi = w.weight_encoding_min.detach().cpu(), w.weight_encoding_max.detach().cpu()
        g = reached[n].float().cpu().reshape(W.shape)
        gx, gmin, gmax = T.lg_gradients(W, g, lo, hi, 4, True)
        ex_min, ex_max, b_min, b_max = T.lg_encoding_grads_bound(W, g, lo, hi, 4, True)
        np.testing.assert_array_equal(raw(w.weight.grad.reshape(W.shape)), raw(gx), err_msg=n)
        for ours, ref, ex, b, end in ((w.weight_encoding_min.grad, gmin, ex_min, b_min, "grad_min"),
                                      (w.weight_encoding_max.grad, gmax, ex_max, b_max, "grad_max")):
            T.assert_within_sum_bound(ref, ex, b, LGB_BOUND_C, "block sim restatement %s %s" % (n, end))
            T.assert_within_sum_bound(ours, ex, b, LGB_BOUND_C, "block sim %s %s" % (n, end))
        before[n] = hi.clone()
    opt.step()

    # the step moved the ranges and the next forward quantizes with them
    fc = sim.model.fc
    assert not torch.equal(fc.weight_encoding_max.detach().cpu(), before["fc"])
    seen = {}
    handle = fc._module_to_wrap.register_forward_pre_hook(lambda m, _: seen.__setitem__("w", m.weight.detach().clone()))
    with torch.no_grad():
        sim.model(x)
    handle.remove()
    lo, hi = fc.weight_encoding_min.detach().cpu(), fc.weight_encoding_max.detach().cpu()
    want = T.lg_forward(fc.weight.detach().cpu().reshape(32, 4), lo, hi, 4, True)[0]
    np.testing.assert_array_equal(raw(seen["w"].reshape(32, 4)), raw(want))

    entries = json.load(open(sim.export(str(tmp_path), "lbq")))["param_encodings"]
    assert len(entries["fc.weight"]) == 32 and len(entries["conv.weight"]) == 8
    assert all(e["block_size"] == 4 and e["bitwidth"] == 4 for e in entries["conv.weight"])
