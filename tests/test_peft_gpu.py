"""aimet_amd.peft on the GPU: the aimet_lora_* kernels against the numpy oracle (tests/lora_oracle.py) bit for
bit on guarded buffers, the quantized LoRA layer's fused route against its literal route and the oracle,
the launch counts of both routes and of every fallback, and PeftQuantUtils on a calibrated sim.

"Bit for bit" leaves one thing open: which NaN an operation yields (its sign and payload) is the
hardware's choice, so every NaN compares equal to every NaN; where a NaN stands is compared.
"""
import itertools

import numpy as np
import pytest
import torch

from conftest import gpu_available

import lora_oracle as L
from test_peft import SCALE, give_encodings, make_net

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import peft as P  # noqa: E402
from aimet_amd.qc_quantize_op import (LearnedGridQuantWrapper, QcQuantizeOpMode,  # noqa: E402
                                      StaticGridQuantWrapper)
from aimet_amd.quantizers import QuantizationDataType, QuantScheme  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

DEV = "cuda"
F = np.float32
GUARD = 8
TORCH_DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
BITS_DT = {"fp32": (np.uint32, np.int32, torch.int32), "fp16": (np.uint16, np.int16, torch.int16),
           "bf16": (np.uint16, np.int16, torch.int16)}
SENTINEL = F(-777.25)   # representable in all three dtypes
# below, at and past one 16-B vector (4 floats / 8 halves) and one 256-lane tile of each width (1024 floats /
# 2048 halves), and a ragged tail
SIZES = [1, 7, 8, 9, 1023, 1024, 1025, 2047, 2048, 2049, 6149]
# (u / a, v, out): 8 and 16 bits, one symmetric with min == -max in each set
ENC_SETS = [((-6.3, 7.1, 8), (-4.0, 4.0, 8), (-9.7, 10.2, 16)),
            ((-5.0, 5.0, 16), (-0.37, 8.9, 8), (-8.0, 8.0, 8))]


class Guarded:
    """A device buffer of n elements of dtype dt between two guards, its base aligned to 256 bytes or off
    by one element (the all-scalar path)."""

    def __init__(self, n, dt, misaligned, fill=None):
        self.n, self.dt, self.lead = n, dt, GUARD + (1 if misaligned else 0)
        self.sentinel = L.store_bits(np.array([SENTINEL]), dt)[0]
        host = np.full(self.lead + n + GUARD, self.sentinel, BITS_DT[dt][0])
        if fill is not None:
            host[self.lead:self.lead + n] = L.store_bits(np.asarray(fill, F).ravel(), dt)
        self.t = torch.from_numpy(host.view(BITS_DT[dt][1])).to(DEV)

    def view(self):
        return self.t[self.lead:self.lead + self.n].view(TORCH_DT[self.dt])

    def bits(self):
        return L.nan_blind(self.t.cpu().numpy().view(BITS_DT[self.dt][0]), self.dt)

    def expect(self, body):
        want = np.full(self.lead + self.n + GUARD, self.sentinel, BITS_DT[self.dt][0])
        want[self.lead:self.lead + self.n] = L.store_bits(np.asarray(body, F).ravel(), self.dt)
        return L.nan_blind(want, self.dt)

    def untouched(self):
        return self.expect(np.full(self.n, SENTINEL, F))


def _operands(n, dt, si, encs):
    u = L.inputs(n, 100 * si + n, encs, dt)
    v = L.inputs(n, 200 * si + n + 1, encs, dt, shift=7)
    g = L.inputs(n, 300 * si + n + 2, encs, dt, shift=13)
    g[::2] = -np.abs(g[::2])   # negative gradients meet masked elements
    return u, v, g


# ---- 1. the kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dt", L.DTYPES)
def test_merge_kernels_equal_the_oracle_bit_for_bit(dt, n):
    negative_zero = False
    for si, encs in enumerate(ENC_SETS):
        u, v, g = _operands(n, dt, si, encs)
        for mis in (False, True):
            su, sv, sg = Guarded(n, dt, mis, u), Guarded(n, dt, mis, v), Guarded(n, dt, mis, g)
            for present in itertools.product((False, True), repeat=3):
                eu, ev, eo = (e if p else None for e, p in zip(encs, present))
                where = (dt, n, si, mis, present)
                out = Guarded(n, dt, mis)
                P.lora_merge(su.view(), sv.view(), eu, ev, eo, out=out.view())
                assert np.array_equal(out.bits(), out.expect(L.merge(u, v, eu, ev, eo, dt))), where
                wu, wv = L.merge_backward(u, v, g, eu, ev, eo, dt)
                negative_zero |= bool((np.signbit(wu) & (wu == 0)).any())
                for need_u, need_v in ((True, True), (True, False), (False, True)):
                    gu, gv = Guarded(n, dt, mis), Guarded(n, dt, mis)
                    P.lora_merge_backward(su.view(), sv.view(), sg.view(), eu, ev, eo, need_u=need_u, need_v=need_v,
                                          grad_u=gu.view(), grad_v=gv.view())
                    assert np.array_equal(gu.bits(), gu.expect(wu) if need_u else gu.untouched()), where
                    assert np.array_equal(gv.bits(), gv.expect(wv) if need_v else gv.untouched()), where
            for src, body in ((su, u), (sv, v), (sg, g)):
                assert np.array_equal(src.bits(), src.expect(body)), (dt, n, si, mis)
    assert negative_zero or n < 1023   # a masked negative gradient (-0) was among the cases


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dt", L.DTYPES)
def test_scale_kernels_equal_the_oracle_bit_for_bit(dt, n):
    s = L.host_scale(SCALE, dt)
    for si, encs in enumerate(ENC_SETS):
        a, _, g = _operands(n, dt, si, (encs[0], encs[2]))
        for mis in (False, True):
            sa, sg = Guarded(n, dt, mis, a), Guarded(n, dt, mis, g)
            for present in itertools.product((False, True), repeat=2):
                ea, eo = (e if p else None for e, p in zip((encs[0], encs[2]), present))
                where = (dt, n, si, mis, present)
                out, ga = Guarded(n, dt, mis), Guarded(n, dt, mis)
                P.lora_scale(sa.view(), float(s), ea, eo, out=out.view())
                assert np.array_equal(out.bits(), out.expect(L.scale(a, s, ea, eo, dt))), where
                P.lora_scale_backward(sa.view(), sg.view(), float(s), ea, eo, grad_a=ga.view())
                assert np.array_equal(ga.bits(), ga.expect(L.scale_backward(a, g, s, ea, eo, dt))), where
            assert np.array_equal(sa.bits(), sa.expect(a)) and np.array_equal(sg.bits(), sg.expect(g))


def test_overlapping_buffers_are_refused_and_nothing_is_launched():
    u, v = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    before = P.lora_launch_count()
    with pytest.raises(ValueError, match="overlaps"):
        P.lora_merge(u, v, out=u)
    with pytest.raises(ValueError, match="overlaps"):
        P.lora_merge(u[:32], v[:32], out=u[16:48])
    with pytest.raises(ValueError, match="overlap"):
        P.lora_merge_backward(u[:16], v[:16], u[16:32], grad_u=v[32:48], grad_v=v[40:56])
    with pytest.raises(ValueError, match="overlaps"):
        P.lora_scale(u, 2.0, out=u)
    with pytest.raises(ValueError, match="overlaps"):
        P.lora_scale_backward(u, v, 2.0, grad_a=v)
    assert P.lora_launch_count() == before
    P.lora_merge(u[:32], v[:32], out=u[32:])
    assert P.lora_launch_count() == before + 1


# ---- 2. the module -------------------------------------------------------------------------------
def _input(kind, dt, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((2, 5, 24) if kind == "linear" else (1, 3, 6, 6), generator=g) * 2.0
    return x.to(DEV, TORCH_DT[dt])


def _sim(kind, dt, scheme="tf", both_adapters=False, **kwargs):
    net = make_net(kind).to(DEV, TORCH_DT[dt]).eval()
    if both_adapters:
        net.layer.active_adapters["spare"] = True
    x = _input(kind, dt)
    sim = QuantizationSimModel(net, x, quant_scheme=scheme, quantizable_types=P.PEFT_QUANTIZABLE_TYPES, **kwargs)
    sim.compute_encodings(lambda m, _: m(x), None)
    return sim, x


def _np(t):
    return t.detach().to(torch.float32).cpu().numpy()


def _run(sim, x, fused, weight):
    """(output, gradients of x, lora_A.weight, lora_B.weight, base weight, launches forward, launches
    backward) of one forward and backward on the chosen route."""
    layer = sim.model.layer
    layer.fused = fused
    params = [layer.lora_A[0].weight, layer.lora_B[0].weight, layer.base_layer.weight]
    for p in params:
        p.grad = None
    x = x.detach().clone().requires_grad_(True)
    P.lora_launch_count(reset=True)
    out = sim.model(x)
    forward = P.lora_launch_count()
    (out * weight).sum().backward()
    backward = P.lora_launch_count() - forward
    return out, [x.grad] + [p.grad for p in params], forward, backward


def _encoding_of(wrapper):
    q = wrapper.output_quantizers[0]
    return (q.encoding.min, q.encoding.max, q.encoding.bw) if q.enabled else None


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["linear", "conv"])
def test_fused_and_literal_routes_and_the_oracle_agree_bit_for_bit(kind, dt):
    sim, x = _sim(kind, dt)
    layer = sim.model.layer
    five = {"base": layer.base_layer, "A": layer.lora_A[0], "mul": layer.mul_scale, "B": layer.lora_B[0],
            "add": layer.add_lora_to_res}
    assert all(type(w) is StaticGridQuantWrapper and w.output_quantizers[0].enabled for w in five.values())
    raw = {}
    hooks = [five[k].get_original_module().register_forward_hook(
        lambda _m, args, out, k=k: raw.__setitem__(k, (_np(args[0]), _np(out)))) for k in ("base", "A", "B")]
    weight = torch.randn(sim.model(x).shape, generator=torch.Generator().manual_seed(5)).to(DEV, TORCH_DT[dt])
    fused = _run(sim, x, True, weight)
    raw_fused = dict(raw)
    literal = _run(sim, x, False, weight)
    for h in hooks:
        h.remove()
    assert (fused[2], fused[3]) == (2, 2)
    assert (literal[2], literal[3]) == (0, 0)
    assert torch.equal(fused[0], literal[0])
    for name, a, b in zip(("x", "lora_A.weight", "lora_B.weight", "base weight"), fused[1], literal[1]):
        assert a is not None and a.abs().sum() > 0, name
        assert torch.equal(a, b), name
    for k in raw:   # both routes ran the same GEMMs on the same operands
        assert np.array_equal(raw[k][0], raw_fused[k][0]) and np.array_equal(raw[k][1], raw_fused[k][1])

    def v_of_m(m):
        assert np.array_equal(L.store_bits(m, dt), L.store_bits(raw["B"][0], dt))   # what lora_B was given
        return raw["B"][1]
    encs = {k: _encoding_of(w) for k, w in five.items()}
    _, want = L.layer_forward(raw["base"][1], raw["A"][1], v_of_m, SCALE, encs, dt)
    assert np.array_equal(L.store_bits(_np(fused[0]), dt), L.store_bits(want, dt))
    if dt == "bf16":
        assert L.host_scale(SCALE, dt) != F(SCALE)   # the scale the 16-bit kernels get is a rounded one


def test_a_write_to_the_scaling_tensor_is_seen_by_the_fused_route():
    sim, x = _sim("linear", "fp32")
    layer = sim.model.layer
    with torch.no_grad():
        layer.scaling[0].fill_(0.75)
        layer.fused = True
        P.lora_launch_count(reset=True)
        fused = sim.model(x)
        assert P.lora_launch_count() == 2
        layer.fused = False
        assert torch.equal(fused, sim.model(x))


# ---- 3. launch counts of the fallbacks -----------------------------------------------------------------
def _literal(sim, x, backward=True):
    """Runs forward (and backward) on the default route and returns the aimet_lora launches."""
    assert sim.model.layer.fused is True
    P.lora_launch_count(reset=True)
    if backward:
        x = x.detach().clone().requires_grad_(True)
        sim.model(x).float().sum().backward()
        assert x.grad is not None
    else:
        with torch.no_grad():
            sim.model(x)
    return P.lora_launch_count()


@pytest.mark.parametrize("mode", [QcQuantizeOpMode.ANALYSIS, QcQuantizeOpMode.PASSTHROUGH])
def test_analysis_and_passthrough_modes_take_the_literal_route(mode):
    sim, x = _sim("linear", "fp32")
    for _, w in sim.quant_wrappers():
        w.set_mode(mode)
    assert _literal(sim, x, backward=False) == 0


def test_a_range_learning_sim_takes_the_literal_route():
    sim, x = _sim("linear", "fp32", scheme=QuantScheme.training_range_learning_with_tf_init)
    assert type(sim.model.layer.mul_scale) is LearnedGridQuantWrapper
    assert _literal(sim, x) == 0


def test_stochastic_rounding_in_training_takes_the_literal_route():
    sim, x = _sim("linear", "fp32", rounding_mode="stochastic")
    assert _literal(sim, x, backward=False) == 2   # eval: rounds to nearest
    sim.model.train()
    assert _literal(sim, x) == 0


def test_float_data_types_take_the_literal_route():
    sim, x = _sim("linear", "fp32", default_data_type=QuantizationDataType.float, default_output_bw=16,
                  default_param_bw=16)
    assert _literal(sim, x) == 0


def test_several_active_adapters_take_the_literal_route():
    sim, x = _sim("linear", "fp32", both_adapters=True)
    assert _literal(sim, x) == 0
    sim.model.layer.active_adapters["spare"] = False
    assert _literal(sim, x) == 4


def test_a_quantized_scale_takes_the_literal_route(tmp_path):
    sim, x = _sim("linear", "fp32")
    utils = P.PeftQuantUtils(P.track_lora_meta_data(sim.model, str(tmp_path), "meta"))
    assert _literal(sim, x, backward=False) == 2
    utils.quantize_lora_scale_with_fixed_range(sim, 16, 0.0, 2.0)
    assert _literal(sim, x) == 0


def test_fp16_takes_the_fused_route_and_equals_the_literal_one():
    sim, x = _sim("linear", "fp16")
    with torch.no_grad():
        P.lora_launch_count(reset=True)
        fused = sim.model(x)
        assert P.lora_launch_count() == 2
        sim.model.layer.fused = False
        assert torch.equal(fused, sim.model(x))
        assert P.lora_launch_count() == 2


def test_cpu_tensors_take_the_literal_route():
    net = make_net("linear").eval()
    sim = QuantizationSimModel(net, quantizable_types=P.PEFT_QUANTIZABLE_TYPES)
    for _, w in sim.quant_wrappers():
        w.enable_param_quantizers(False, None)
        w.set_mode(QcQuantizeOpMode.ACTIVE)
    give_encodings(sim)
    P.lora_launch_count(reset=True)
    with torch.no_grad():
        out = sim.model(_input("linear", "fp32").cpu())
    assert out.device.type == "cpu" and torch.isfinite(out).all()
    assert P.lora_launch_count() == 0


# ---- 4. PeftQuantUtils -------------------------------------------------------------------------------
def _encodings(sim):
    return {"%s/%d" % (name, i): (q.encoding.min, q.encoding.max) if q.enabled and q.encoding else None
            for name, w in sim.quant_wrappers() for i, q in enumerate(sim._quantizers_of(w))}


def test_a_frozen_base_keeps_its_encodings_through_a_second_calibration(tmp_path):
    sim, x = _sim("linear", "fp32")
    utils = P.PeftQuantUtils(P.track_lora_meta_data(sim.model, str(tmp_path), "meta"))
    before = _encodings(sim)
    utils.freeze_base_model(sim)
    with torch.no_grad():
        for _, w in utils.get_quantized_lora_layer(sim):
            w.get_original_module().weight.mul_(3.0)
    sim.compute_encodings(lambda m, _: m(x * 2.0), None)
    after = _encodings(sim)
    adapters = ("layer.lora_A.0/", "layer.lora_B.0/")
    moved = [k for k in before if before[k] != after[k]]
    assert moved and all(k.startswith(adapters) for k in moved)
    for prefix in adapters:   # the weight's and the output's encoding of both adapter layers
        assert sum(k.startswith(prefix) for k in moved) >= 2
    assert _literal(sim, x, backward=False) == 2   # and the calibrated sim is back on the fused route


def test_disabled_adapters_leave_the_base_alone(tmp_path):
    sim, x = _sim("linear", "fp32")
    utils = P.PeftQuantUtils(P.track_lora_meta_data(sim.model, str(tmp_path), "meta"))
    layer = sim.model.layer
    with torch.no_grad():
        adapted = sim.model(x)
        utils.disable_lora_adapters(sim)
        got = sim.model(x)
        # the base alone: its quantized output through the layer's last quantizer, nothing added
        base = layer.base_layer(x)
        want = layer.add_lora_to_res(base, torch.zeros_like(base))
    assert torch.equal(got, want) and not torch.equal(got, adapted)


def test_adapter_bitwidths_reach_only_the_adapter_encodings(tmp_path):
    sim, x = _sim("linear", "fp32")
    utils = P.PeftQuantUtils(P.track_lora_meta_data(sim.model, str(tmp_path), "meta"))
    utils.set_bitwidth_for_lora_adapters(sim, output_bw=16, param_bw=4)
    sim.compute_encodings(lambda m, _: m(x), None)
    for name, w in sim.quant_wrappers():
        if name.endswith(".1"):
            continue   # the inactive adapter's layers never ran: no encodings
        adapter = name in utils.lora_layers
        assert w.output_quantizers[0].encoding.bw == (16 if adapter else 8), name
        if "weight" in w.param_quantizers:
            assert w.param_quantizers["weight"].encoding.bw == (4 if adapter else 8), name
    assert _literal(sim, x, backward=False) == 2
