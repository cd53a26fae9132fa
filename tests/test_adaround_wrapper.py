"""The reference's AdaRound caller surface on the fused kernels:
AdaroundWrapper (v1/adaround/adaround_wrapper.py:93-224) and
AdaroundOptimizer.adaround_module (v1/adaround/adaround_optimizer.py:69-221).

GPU: the wrapper built around a StaticGridQuantWrapper whose per-channel weight quantizer holds
the golden case's delta / offset reproduces golden_adaround.npz (the reference's own
apply_adaround) bit for bit -- Wq soft and hard, and dL/dalpha of the reconstruction term;
adaround_module on a MobileNet-v2-shaped layer gives the alpha that optimize_rounding gives on the
same sampled activations, bit for bit.
CPU: ModuleData / ActivationSampler collection (hooks, early stop, dataset sharding order)."""
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import gpu_available

gpu = pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")
DEV = "cuda"
PER_CHANNEL_CFG = {"defaults": {"ops": {"is_output_quantized": "True"},
                                "params": {"is_quantized": "True", "is_symmetric": "True"},
                                "strict_symmetric": "False", "per_channel_quantization": "True"}}


def _module_for(w):
    if w.ndim == 2:
        m = nn.Linear(w.shape[1], w.shape[0])
    else:
        cin_g = w.shape[1]
        groups = w.shape[0] if cin_g == 1 and w.shape[0] > 1 else 1
        m = nn.Conv2d(cin_g * groups, w.shape[0], w.shape[2], padding=w.shape[2] // 2, groups=groups)
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(w))
    return m


def _encodings(delta, offset, bw):
    from aimet_amd.libpymo import TfEncoding
    out = []
    for d, o in zip(delta.tolist(), offset.tolist()):
        e = TfEncoding()
        e.delta, e.offset, e.bw = d, o, bw
        e.min = o * d
        e.max = e.min + d * (2 ** bw - 1)
        out.append(e)
    return out


def _wrapped(w, delta, offset, bw):
    from aimet_amd.qc_quantize_op import StaticGridQuantWrapper
    from aimet_amd.quantizers import QuantScheme, StaticGridPerChannelQuantizer
    m = _module_for(w).to(DEV)
    qw = StaticGridQuantWrapper(m, bw, 8, "nearest", QuantScheme.post_training_tf_enhanced)
    q = StaticGridPerChannelQuantizer(bw, "nearest", QuantScheme.post_training_tf_enhanced, True, w.shape[0], True)
    q.encoding = _encodings(delta, offset, bw)
    qw.param_quantizers["weight"] = q
    qw.param_quantizers["bias"].enabled = False   # as QuantSim's default config: weights only
    return qw


@pytest.mark.gpu
@gpu
def test_adaround_wrapper_reproduces_reference_apply_adaround(golden_dir):
    from aimet_amd.adaround_wrapper import AdaroundWrapper
    z = dict(np.load(os.path.join(golden_dir, "golden_adaround.npz")))
    for i in range(int(z["count"])):
        k = "c%d_" % i
        w, bw = z[k + "w"], int(z[k + "bw"])
        ada = AdaroundWrapper(_wrapped(w, z[k + "delta"], z[k + "offset"], bw))
        # makeDeltaOffsetTensor -> the fixture's float32 delta / offset, broadcast along axis 0
        assert ada.broadcasted_delta.shape == (w.shape[0],) + (1,) * (w.ndim - 1)
        assert np.array_equal(ada.broadcasted_delta.reshape(-1).cpu().numpy(), z[k + "delta"])
        assert np.array_equal(ada.broadcasted_offset.reshape(-1).cpu().numpy(), z[k + "offset"])
        assert (ada.bitwidth, ada.clip_min, ada.clip_max, ada.use_soft_rounding) == (bw, 0, 2 ** bw - 1, True)
        with torch.no_grad():
            ada.alpha.copy_(torch.from_numpy(z[k + "alpha"]))
        weight = ada.weight
        wq = ada.apply_adaround(weight)
        assert np.array_equal(wq.detach().cpu().numpy().view(np.int32), z[k + "wq"].view(np.int32)), i
        (wq * torch.from_numpy(z[k + "grad"]).to(DEV)).sum().backward()
        assert np.array_equal(ada.alpha.grad.cpu().numpy().view(np.int32), z[k + "ga_recon"].view(np.int32)), i
        ada.use_soft_rounding = False
        with torch.no_grad():
            wh = ada.apply_adaround(weight)
        assert np.array_equal(wh.cpu().numpy().view(np.int32), z[k + "wq_hard"].view(np.int32)), i
        # forward: the wrapped module with the adarounded weight, its weight quantizer off for the
        # call only and the original Parameter back in place afterwards
        x = torch.randn((2, w.shape[1]) if w.ndim == 2 else (2, ada.get_original_module().in_channels, 6, 6),
                        device=DEV)
        ada.module_to_wrap.output_quantizers[0].enabled = False
        with torch.no_grad():
            y = ada(x)
            m = ada.get_original_module()
            want = nn.functional.linear(x, wh, m.bias) if w.ndim == 2 else \
                nn.functional.conv2d(x, wh, m.bias, m.stride, m.padding, m.dilation, m.groups)
        assert torch.equal(y, want), i
        assert ada.module_to_wrap.param_quantizers["weight"].enabled
        assert isinstance(m.weight, nn.Parameter) and "weight" not in m.__dict__


class Block(nn.Module):
    """A MobileNet-v2 inverted-residual slice: pointwise expand -> depthwise -> pointwise project."""
    def __init__(self):
        super().__init__()
        self.expand = nn.Conv2d(16, 96, 1, bias=False)
        self.relu1 = nn.ReLU6()
        self.dw = nn.Conv2d(96, 96, 3, padding=1, groups=96, bias=False)
        self.relu2 = nn.ReLU6()
        self.project = nn.Conv2d(96, 24, 1, bias=False)

    def forward(self, x):
        return self.project(self.relu2(self.dw(self.relu1(self.expand(x)))))


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("layer,act", [("expand", nn.ReLU6()), ("dw", nn.ReLU6()), ("project", None)])
def test_adaround_module_equals_optimize_rounding(layer, act):
    """adaround_module(module, quant_module, orig_model, quant_model, act_func, cached_dataset,
    forward_fn, opt_params) == optimize_rounding on the activations it samples, bit for bit; the
    wrapper ends in hard rounding."""
    from aimet_amd.activation_sampler import ActivationSampler
    from aimet_amd.adaround_optimizer import AdaroundHyperParameters, AdaroundOptimizer
    from aimet_amd.adaround_wrapper import AdaroundWrapper
    from aimet_amd.quantsim import QuantizationSimModel
    torch.manual_seed(0)
    orig = Block().to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    data = [torch.rand(8, 16, 14, 14, generator=g).to(DEV) for _ in range(6)]
    sim = QuantizationSimModel(Block().to(DEV).eval(), config_file=PER_CHANNEL_CFG, default_param_bw=4)
    for (n, p), (_, q) in zip(orig.named_parameters(), sim.model.named_parameters()):
        with torch.no_grad():
            q.copy_(p)
    sim.compute_encodings(lambda m, d: [m(x) for x in d], data[:2])
    ada = AdaroundWrapper(getattr(sim.model, layer))
    setattr(sim.model, layer, ada)
    params = AdaroundHyperParameters(num_iterations=120, warm_start=0.25)
    forward_fn = lambda m, x: m(x)   # noqa: E731
    alpha0 = ada.alpha.detach().clone()
    torch.manual_seed(7)
    AdaroundOptimizer.adaround_module(getattr(orig, layer), ada, orig, sim.model, act, data, forward_fn, params)
    assert not ada.use_soft_rounding
    # the same loop called directly on the same samples and the same randperm stream
    sampler = ActivationSampler(getattr(orig, layer), ada, orig, sim.model, forward_fn)
    ada.use_soft_rounding = True
    inp, out = sampler.sample_all_acts(data, device=torch.device(DEV))
    torch.manual_seed(7)
    want = AdaroundOptimizer.optimize_rounding(ada.get_original_module(), inp, out, ada._delta_vec.to(DEV),
                                               ada._offset_vec.to(DEV), ada.bitwidth, ada._ch_axis, params, act,
                                               alpha=alpha0.clone())
    assert torch.equal(ada.alpha.detach(), want.detach())
    assert not torch.equal(alpha0, want.detach())   # it did optimise


# ------------------------------------------------------------------------------------------
# CPU: activation collection
# ------------------------------------------------------------------------------------------
def test_module_data_collects_and_stops_early():
    from aimet_amd.activation_sampler import ModuleData
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(4, 6), nn.ReLU(), nn.Linear(6, 3))
    ran = []
    net[2].register_forward_hook(lambda m, i, o: ran.append(1))
    x = torch.randn(5, 4)
    inp, out = ModuleData(net, net[0]).collect_inp_out_data(x, collect_input=True, collect_output=True)
    assert torch.equal(inp, x) and torch.equal(out, net[0](x).detach())
    assert not ran                                     # the forward stopped at the layer
    inp, out = ModuleData(net, net[2], lambda m, d: m(d[0])).collect_inp_out_data([x], False, True)
    assert inp is None and torch.equal(out, net(x).detach())
    assert net.training                                # eval mode only for the collection


def test_activation_sampler_concatenates_batches():
    from aimet_amd.activation_sampler import ActivationSampler
    torch.manual_seed(0)
    orig = nn.Sequential(nn.Linear(4, 6), nn.ReLU(), nn.Linear(6, 3))
    quant = nn.Sequential(nn.Linear(4, 6), nn.ReLU(), nn.Linear(6, 3))
    data = [torch.randn(2, 4) for _ in range(3)]
    s = ActivationSampler(orig[2], quant[2], orig, quant, None)
    inp, out = s.sample_and_place_all_acts_on_cpu(data)
    assert inp.shape == (6, 6) and out.shape == (6, 3)
    with torch.no_grad():
        assert torch.equal(inp, torch.cat([quant[1](quant[0](d)) for d in data]))
        assert torch.equal(out, torch.cat([orig(d) for d in data]))


def _plan(m, shape_in, act=None, aligned=True):
    """plan_loop's form for `m` on float32 caches of shape_in and of the output shape it gives."""
    from aimet_amd.adaround_optimizer import plan_loop
    with torch.no_grad():
        shape_out = (shape_in[0],) + tuple(m(torch.zeros((1,) + tuple(shape_in[1:]))).shape[1:])
    return plan_loop(m, tuple(shape_in), torch.float32, shape_out, torch.float32, act, aligned)


def test_adaround_plan_mobilenet_v2_forms(golden_dir):
    """The planner on the 53 conv / linear layers of MobileNet-v2 at 224 x 224 with 1024 cached
    samples gives the forms the 10k-iteration benchmark recorded per layer
    (tests/golden/adaround_loop_forms.json: names and forms of profiles/r05/adaround_mobilenet_10k.json)."""
    import json
    from workloads.mobilenet_v2 import mobilenet_v2
    net = mobilenet_v2(seed=0)
    layers = [(n, m) for n, m in net.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
    follow = {}   # the ReLU6 after a layer, as benchmarks/adaround_mobilenet.py finds it
    for parent in net.modules():
        kids = list(parent.children())
        follow.update({a: b for a, b in zip(kids, kids[1:]) if isinstance(b, nn.ReLU6)})
    shapes = {}
    hooks = [m.register_forward_hook(lambda mod, i, o: shapes.__setitem__(mod, tuple(i[0].shape))) for _, m in layers]
    with torch.no_grad():
        net(torch.zeros(1, 3, 224, 224))
    for h in hooks:
        h.remove()
    got = [[n, _plan(m, (1024,) + shapes[m][1:], follow.get(m)).form] for n, m in layers]
    with open(os.path.join(golden_dir, "adaround_loop_forms.json")) as f:
        assert got == json.load(f)


def _layer(kind, *a):
    """(module, input cache shape with 64 samples) of a test layer, built when the test runs."""
    if kind == "stem":      # 3 -> a[0] channels, k3 s2, from a[1] x a[1] input
        return nn.Conv2d(3, a[0], 3, stride=2, padding=1), (64, 3, a[1], a[1])
    if kind == "pw":        # a[0] -> a[1] channels at a[2] x a[2]
        return nn.Conv2d(a[0], a[1], 1), (64, a[0], a[2], a[2])
    if kind == "dw":        # depthwise, kernel a[0]
        return nn.Conv2d(16, 16, a[0], padding=a[0] // 2, groups=16), (64, 16, 14, 14)
    if kind == "conv3":     # C_in k k = 144 > 64: no im2col form
        return nn.Conv2d(16, 16, 3, padding=1), (64, 16, 14, 14)
    return nn.Linear(96, 40), (64, 96)


@pytest.mark.parametrize("layer,act,aligned,want", [
    (("pw", 16, 48, 14), nn.ReLU6(), True, "pointwise_cm"),
    (("pw", 16, 48, 16), nn.ReLU6(), True, "pointwise"),
    (("pw", 16, 96, 28), nn.ReLU6(), True, "pointwise_fused"),
    (("pw", 192, 32, 28), nn.ReLU6(), True, "mfma"),            # pointwise_fused exactly when on the matrix cores
    (("pw", 200, 32, 28), nn.ReLU6(), True, "pointwise"),       # C_in > 192
    (("pw", 144, 24, 56), nn.ReLU6(), True, "pointwise_fused"),
    (("pw", 16, 96, 27), nn.ReLU6(), True, "pointwise"),        # hw % 4 != 0
    (("stem", 16, 28), nn.ReLU6(), True, "im2col_cm"),
    (("stem", 16, 32), nn.ReLU6(), True, "im2col"),
    (("stem", 32, 64), nn.ReLU6(), True, "im2col_fused"),
    (("conv3",), nn.ReLU6(), True, "autograd"),
    (("dw", 3), nn.ReLU6(), True, "dw"),
    (("dw", 5), nn.ReLU6(), True, "dw"),
    (("dw", 7), nn.ReLU6(), True, "autograd"),
    (("linear",), nn.ReLU6(), True, "linear"),
    (("pw", 16, 48, 14), nn.Hardswish(), True, "autograd"),     # no fused reconstruction gradient
    (("pw", 16, 96, 28), nn.ReLU6(), False, "pointwise"),       # a cache off the 16-byte boundary
])
def test_adaround_plan_boundaries(layer, act, aligned, want):
    """plan_loop at the edges of its rules (the channel-major form up to 14 x 14, the one-pass
    step from 28 x 28 with C_in <= 192 and hw % 4 == 0 on aligned caches, im2col up to
    C_in k k = 64, native depthwise for K in {3, 5}), on a machine without a GPU."""
    from aimet_amd.adaround_optimizer import _pw_step_uses_mfma
    m, shape_in = _layer(*layer)
    if want == "mfma":
        want = "pointwise_fused" if _pw_step_uses_mfma(m.in_channels, m.out_channels) else "pointwise"
    plan = _plan(m, shape_in, act, aligned)
    assert plan.form == want
    assert plan.fallback == ("autograd" if want.startswith("pointwise") or want == "linear" else None)
    assert plan.indexed == (not isinstance(act, nn.Hardswish))


_LOOP_KINDS = {   # kind: (layer, activation, the loop form it runs)
    "stem": (("stem", 16, 32), nn.ReLU6(), "im2col"),
    "stem_cm": (("stem", 16, 28), nn.ReLU6(), "im2col_cm"),
    "dw": (("dw", 3), nn.ReLU6(), "dw"),
    "pointwise": (("pw", 16, 48, 14), nn.ReLU6(), "pointwise_cm"),
    "pointwise_wide": (("pw", 576, 96, 14), nn.ReLU6(), "pointwise_cm"),   # MobileNet-v2's 14x14 projection
    "linear": (("linear",), nn.ReLU6(), "linear"),
    "autograd": (("conv3",), nn.ReLU6(), "autograd"),                     # the indexed reconstruction gradient
    "autograd_hardswish": (("pw", 16, 48, 14), nn.Hardswish(), "autograd"),   # torch ops on a gathered target
}


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("kind", list(_LOOP_KINDS))
def test_adaround_loop_deterministic(kind):
    """Two runs of the fused loop with one seed give bit-identical alpha, for every loop form
    (MIOpen through autograd, native depthwise, GEMM pointwise / linear): the form is a fixed rule
    and the convolutions deterministic. The form that ran is the planner's."""
    from aimet_amd.adaround_optimizer import AdaroundHyperParameters, AdaroundOptimizer
    torch.manual_seed(3)
    layer, act, form = _LOOP_KINDS[kind]
    m, shape_in = _layer(*layer)
    assert _plan(m, shape_in, act).form == form
    m = m.to(DEV)
    inp = torch.rand(shape_in, device=DEV)
    with torch.no_grad():
        out = m(inp) + 0.01 * torch.randn_like(m(inp))
    d = (m.weight.detach().abs().max() / 127).reshape(1)
    o = torch.full((1,), -128.0, device=DEV)
    p = AdaroundHyperParameters(num_iterations=300, warm_start=0.2)
    a = [AdaroundOptimizer.optimize_rounding(m, inp, out, d, o, 8, 0, p, act,
                                             torch.Generator().manual_seed(5)).detach().clone() for _ in range(2)]
    assert torch.equal(a[0], a[1]), AdaroundOptimizer.last_loop_form
    assert AdaroundOptimizer.last_loop_form == form


def _loop_problem(kind, seed=3):
    torch.manual_seed(seed)
    if kind == "stem":
        m, shape_in = nn.Conv2d(3, 16, 3, stride=2, padding=1), (64, 3, 32, 32)
    elif kind == "dw":
        m, shape_in = nn.Conv2d(16, 16, 3, padding=1, groups=16), (64, 16, 14, 14)
    elif kind == "pointwise_wide":
        m, shape_in = nn.Conv2d(576, 96, 1), (64, 576, 14, 14)
    else:
        m, shape_in = nn.Linear(96, 40), (64, 96)
    m = m.to(DEV)
    inp = torch.rand(shape_in, device=DEV)
    with torch.no_grad():
        out = m(inp) + 0.01 * torch.randn_like(m(inp))
    d = (m.weight.detach().abs().max() / 127).reshape(1)
    o = torch.full((1,), -128.0, device=DEV)
    return m, inp, out, d, o


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("kind", ["stem", "dw", "pointwise_wide", "linear"])
def test_adaround_multi_iteration_graph_equals_one_per_graph(monkeypatch, kind):
    """k iterations captured in one HIP graph (adaround_optimizer._GRAPH_ITERS; the counters and the batch
    table live on the device) give the alpha of one iteration per graph, bit for bit, also when k
    does not divide the iteration count (the rest replays the one-iteration graph)."""
    import aimet_amd.adaround_optimizer as ao
    from aimet_amd.adaround_optimizer import AdaroundHyperParameters, AdaroundOptimizer
    m, inp, out, d, o = _loop_problem(kind)
    p = AdaroundHyperParameters(num_iterations=303, warm_start=0.2)
    res = []
    for k in (1, 10, 7):
        monkeypatch.setattr(ao, "_GRAPH_ITERS", k)
        loss = torch.zeros(1, device=DEV)
        a = AdaroundOptimizer.optimize_rounding(m, inp, out, d, o, 8, 0, p, nn.ReLU6(), torch.Generator().manual_seed(5),
                                                loss)
        res.append((a.detach().clone(), loss.clone()))
    for a, loss in res[1:]:
        assert torch.equal(a, res[0][0]), (kind, AdaroundOptimizer.last_loop_form)
        assert torch.equal(loss, res[0][1])


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("kind", ["dw", "linear"])
def test_adaround_round_loss_same_when_capture_pool_used_up(kind):
    """Captured loops keep their round-loss fold slots in a fixed arena (upload.cpp fold_buffers);
    once it is used up, a captured launch folds its partials in a launch of its own, in the same
    order: alpha and the reported round loss equal those of the arena form, bit for bit (ADVICE
    r04: the fallback was one float atomic per workgroup)."""
    import ctypes
    from aimet_amd import _native
    from aimet_amd.adaround_optimizer import AdaroundHyperParameters, AdaroundOptimizer
    m, inp, out, d, o = _loop_problem(kind)
    p = AdaroundHyperParameters(num_iterations=120, warm_start=0.2)
    res = []
    for limit in (None, 0):
        prev = ctypes.c_int64()
        if limit is not None:
            _native.call("aimet_capture_pool_limit", limit, ctypes.byref(prev))
        try:
            loss = torch.zeros(1, device=DEV)
            a = AdaroundOptimizer.optimize_rounding(m, inp, out, d, o, 8, 0, p, nn.ReLU6(),
                                                    torch.Generator().manual_seed(5), loss)
            res.append((a.detach().clone(), loss.clone()))
        finally:
            if limit is not None:
                _native.call("aimet_capture_pool_limit", prev.value, None)
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]) and res[0][1].item() != 0.0


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("cin,cout,k,hw", [(3, 32, 3, 64), (16, 96, 1, 28), (64, 192, 1, 28), (144, 24, 1, 56)])
def test_adaround_one_pass_step_slices_folded_by_adam(monkeypatch, cin, cout, k, hw):
    """The one-pass 1x1 / stem step leaving its weight-gradient slices for the Adam step to add
    (aimet_adaround_pw_step_slices, part_kk = C_in C_out) gives the alpha of the separate fold
    launch (pw_fold_final), bit for bit: VALU (C_in < 32) and matrix-core (C_in >= 32) forms."""
    import aimet_amd.adaround_optimizer as ao
    torch.manual_seed(8)
    m = nn.Conv2d(cin, cout, k, stride=2 if k == 3 else 1, padding=k // 2).to(DEV)
    inp = torch.rand(32, cin, hw, hw, device=DEV)
    with torch.no_grad():
        out = m(inp) + 0.02 * torch.randn_like(m(inp))
    d = (m.weight.detach().abs().amax(dim=(1, 2, 3)) / 127).contiguous()
    o = torch.full((cout,), -128.0, device=DEV)
    p = ao.AdaroundHyperParameters(num_iterations=200, warm_start=0.2)
    res = []
    for fold in (True, False):
        monkeypatch.setattr(ao, "_DW_FOLD_ADAM", fold)
        loss = torch.zeros(1, device=DEV)
        res.append((ao.AdaroundOptimizer.optimize_rounding(m, inp, out, d, o, 8, 0, p, nn.ReLU6(),
                                                           torch.Generator().manual_seed(6), loss).detach().clone(),
                    loss.clone()))
        assert ao.AdaroundOptimizer.last_loop_form in ("pointwise_fused", "im2col_fused")
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("stride,act", [(1, nn.ReLU6()), (2, nn.ReLU()), (1, None)])
def test_adaround_dw_fused_loop_equals_unfused(monkeypatch, stride, act):
    """The depthwise loop with the fused step (aimet_adaround_dw_step: the batch read in place, q and g
    never stored) gives the alpha of the four-launch loop (gather, forward, reconstruction gradient,
    weight gradient), bit for bit."""
    import aimet_amd.adaround_optimizer as ao
    torch.manual_seed(4)
    m = nn.Conv2d(24, 24, 3, stride=stride, padding=1, groups=24).to(DEV)
    inp = torch.rand(48, 24, 28, 28, device=DEV)
    with torch.no_grad():
        out = m(inp) + 0.02 * torch.randn_like(m(inp))
    d = (m.weight.detach().abs().amax(dim=(1, 2, 3)) / 127).contiguous()
    o = torch.full((24,), -128.0, device=DEV)
    p = ao.AdaroundHyperParameters(num_iterations=200, warm_start=0.2)
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ao, "_DW_FUSED", fused)
        res.append(ao.AdaroundOptimizer.optimize_rounding(m, inp, out, d, o, 8, 0, p, act,
                                                          torch.Generator().manual_seed(6)).detach().clone())
        assert ao.AdaroundOptimizer.last_loop_form == "dw"
    assert torch.equal(res[0], res[1])


@pytest.mark.gpu
@gpu
def test_adaround_pw_fused_loop_deterministic_and_close_to_gemm_form(monkeypatch):
    """The one-pass 1x1 loop (aimet_adaround_pw_step) gives one alpha per seed, and the alpha of the
    GEMM form to fp32 summation-order tolerance (the two sum dL/dWq in different orders)."""
    import aimet_amd.adaround_optimizer as ao
    torch.manual_seed(5)
    m = nn.Conv2d(16, 96, 1).to(DEV)
    inp = torch.rand(48, 16, 16, 16, device=DEV)
    with torch.no_grad():
        out = m(inp) + 0.02 * torch.randn_like(m(inp))
    d = (m.weight.detach().abs().amax(dim=(1, 2, 3)) / 127).contiguous()
    o = torch.full((96,), -128.0, device=DEV)
    p = ao.AdaroundHyperParameters(num_iterations=150, warm_start=0.2)

    def run(form):
        monkeypatch.setattr(ao, "_PW_FUSED", form)
        a = ao.AdaroundOptimizer.optimize_rounding(m, inp, out, d, o, 8, 0, p, nn.ReLU6(),
                                                   torch.Generator().manual_seed(8)).detach().clone()
        return a, ao.AdaroundOptimizer.last_loop_form

    (a1, f1), (a2, _), (g, fg) = run("all"), run("all"), run("0")
    assert (f1, fg) == ("pointwise_fused", "pointwise")   # 16 x 16 positions: the per-sample GEMM form
    assert torch.equal(a1, a2)
    torch.testing.assert_close(a1, g, rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
@gpu
@pytest.mark.parametrize("layer", ["stem", "depthwise", "pointwise"])
def test_adaround_loop_decisions_equal_reference_torch_loop(layer):
    """The fused AdaRound loop (one HIP graph per layer, the fused backward + Adam step) against the
    reference's own loop restated with torch ops on the GPU (adaround_optimizer.py:115-221:
    apply_adaround, AdaroundLoss with its beta schedule, torch.optim.Adam), on a MobileNet-v2 layer
    with the same cached activations, weight encoding, initial alpha and batch draws, 2,000
    iterations (the round loss active for 1,600): the hard-rounding decisions (alpha >= 0) agree on
    >= 99.5 % of the weights (the two loops' convolutions sum in different orders, nothing else
    differs; the 10k-iteration study on these layers found 0 of 2,688 decisions differing,
    profiles/r03/adaround_loop_divergence.json), and the fused loop is bit-reproducible."""
    from aimet_amd.adaround import compute_beta, init_alpha
    from aimet_amd.adaround_optimizer import AdaroundHyperParameters, AdaroundOptimizer, layer_forward, recon_loss
    from aimet_amd.libpymo import QuantizationMode
    from aimet_amd.tensor_quantizer import AimetTensorQuantizer
    from oracle import torch_ref as T
    from workloads.mobilenet_v2 import mobilenet_v2

    iters, images = 2000, 64
    fp = mobilenet_v2(seed=0, device=DEV)
    mods = dict(fp.named_modules())
    name = {"stem": "features.0.0" if "features.0.0" in mods else "features.0", "depthwise": "features.2.conv.0",
            "pointwise": "features.3.conv.0"}[layer]
    m = mods[name]
    if not isinstance(m, (nn.Conv2d, nn.Linear)):
        m = next(c for c in m.modules() if isinstance(c, nn.Conv2d))
    x_img = torch.rand(images, 3, 224, 224, generator=torch.Generator().manual_seed(7)).to(DEV)
    ins, outs = [], []
    h = m.register_forward_hook(lambda mod, i, o: (ins.append(i[0].detach()), outs.append(o.detach())) and None)
    with torch.no_grad():
        fp(x_img)
    h.remove()
    inp, out = torch.cat(ins), torch.cat(outs)
    del fp, x_img
    w = m.weight.detach()
    q = AimetTensorQuantizer(QuantizationMode.QUANTIZATION_TF_ENHANCED)
    q.updateStats(w.contiguous().view(-1), True)
    e, _ = q.getEncoding(8, True, False, False)
    d = torch.tensor([e.delta], dtype=torch.float32, device=DEV)
    o = torch.tensor([e.offset], dtype=torch.float32, device=DEV)
    act = nn.ReLU6()
    params = AdaroundHyperParameters(num_iterations=iters)
    ours = AdaroundOptimizer.optimize_rounding(m, inp, out, d, o, 8, 0, params, act,
                                               torch.Generator().manual_seed(11)).detach().clone()
    again = AdaroundOptimizer.optimize_rounding(m, inp, out, d, o, 8, 0, params, act,
                                                torch.Generator().manual_seed(11)).detach().clone()
    assert torch.equal(ours, again)
    a_ref = init_alpha(w, d)
    opt = torch.optim.Adam([a_ref])
    gen = torch.Generator().manual_seed(11)
    for it in range(iters):
        idx = torch.randperm(inp.shape[0], generator=gen)[:32].to(DEV)
        xb, target = inp.index_select(0, idx), out.index_select(0, idx)
        opt.zero_grad()
        loss = recon_loss(act(layer_forward(m, xb, T.adaround_forward(w, a_ref, d, o, 8))), act(target))
        if it >= params.num_iterations * params.warm_start:
            loss = loss + T.adaround_round_loss(a_ref, params.reg_param,
                                                compute_beta(params.num_iterations, it, params.beta_range,
                                                             params.warm_start))
        loss.backward()
        opt.step()
    differ = float(((ours >= 0) != (a_ref.detach() >= 0)).float().mean())
    assert differ <= 0.005, differ
