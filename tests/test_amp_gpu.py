"""Automatic mixed precision on the GPU (csrc/quant_analyzer.hip aimet_amp_sqnr_add, aimet_amd/amp,
aimet_amd/mixed_precision.py) against tests/amp_oracle.py and tests/golden/golden_amp.json:

1. aimet_amp_sqnr_add in fp32 / fp16 / bf16 on every load path (equal and different base misalignment,
   head and tail, one workgroup and several): the float64 bound, repeatability bit for bit, x == ref,
   1e30-scale inputs, accumulation, two launches per call, rejected arguments;
2. the SQNR callback on the fixture's recorded outputs through a pass-through module: the reference's
   recorded float32 dB values, the float64 restatement, launches, read-backs and fp32 forwards;
3. quantizer groups of three small nets against groups written out by hand from the rules (the
   reference's own finder needs its connected graph and the rest of its package, which cannot be
   imported from this snapshot of it, so there is nothing to record it from);
4. candidates: encodings after set_quantizers_to_candidate + compute_encodings equal a fresh sim's;
5. choose_mixed_precision end to end on the residual net.
Needs an MI355X."""
import ctypes
import functools
import json
import math
import operator
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import REPO, gpu_available

import amp_oracle as O
import qa_oracle

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

from aimet_amd import _native  # noqa: E402
from aimet_amd.amp import mixed_precision_algo as A  # noqa: E402
from aimet_amd.amp.quantizer_groups import QuantizerGroup, find_quantizer_group  # noqa: E402
from aimet_amd.amp.utils import AMPSearchAlgo, create_mac_dict  # noqa: E402
from aimet_amd.mixed_precision import choose_mixed_precision  # noqa: E402
from aimet_amd.qc_quantize_op import QcQuantizeOpMode, StaticGridQuantWrapper  # noqa: E402
from aimet_amd.quant_analyzer import CallbackFunc  # noqa: E402
from aimet_amd.quantizers import QuantizationDataType, QuantScheme  # noqa: E402
from aimet_amd.quantsim import QuantizationSimModel  # noqa: E402

DEV = "cuda"
GUARD = 8          # elements: 16 or 32 bytes, so the guard keeps the 16-byte phase
DTYPES = {"fp32": (torch.float32, 0), "fp16": (torch.float16, 1), "bf16": (torch.bfloat16, 2)}
# 1 .. 257: one workgroup, head / tail only, a full block of vectors; 4099, 65541: several workgroups
# on both load paths (a workgroup takes 256 lanes x 2 vectors)
SIZES = [1, 3, 255, 256, 257, 4099, 65541]
OFFSETS = {"fp32": [(0, 0), (1, 1), (1, 0)],
           "fp16": [(0, 0), (1, 1), (1, 0), (3, 3), (5, 2)],
           "bf16": [(0, 0), (1, 1), (1, 0), (3, 3), (5, 2)]}
KERNEL_CASES = [(n, d, o) for n in SIZES for d in DTYPES for o in OFFSETS[d]]
INT, FLOAT = QuantizationDataType.int, QuantizationDataType.float

with open(os.path.join(REPO, "tests", "golden", "golden_amp.json")) as _f:
    GOLDEN = json.load(_f)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def dev_at(values: torch.Tensor, off: int):
    """A device copy of `values` whose first element is `off` elements past a 16-byte boundary, between guards."""
    n = values.numel()
    buf = torch.full((2 * GUARD + off + n,), 777.0, dtype=values.dtype, device=DEV)
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(values)
    assert view.data_ptr() % 16 == (values.element_size() * off) % 16
    return view


@functools.lru_cache(maxsize=4)
def case(n, dtype_name, scale=1.0):
    """(ref, x) host tensors in the dtype and the oracle's ratio of them: computed once per (n, dtype)."""
    dtype = DTYPES[dtype_name][0]
    g = torch.Generator().manual_seed(n % 100003 + len(dtype_name))
    ref = (torch.randn(n, generator=g) * 3.0 + 0.5).mul_(scale).to(dtype)
    x = (ref.float() + torch.randn(n, generator=g) * 0.05 * scale).to(dtype)
    return ref, x, O.sqnr_ratio(ref, x)


def run(ref, x, dtype_name, offs=(0, 0), eps=O.EPS, acc0=0.0):
    """aimet_amp_sqnr_add into an accumulator that starts at acc0 and sits between guards."""
    acc = torch.tensor([555.0, acc0, 555.0], dtype=torch.float64, device=DEV)
    r, v = dev_at(ref, offs[0]), dev_at(x, offs[1])
    _native.call("aimet_amp_sqnr_add", p(r), p(v), ref.numel(), DTYPES[dtype_name][1], eps, p(acc[1:2]), stream())
    torch.cuda.synchronize()
    h = acc.cpu().numpy()
    assert h[0] == 555.0 and h[2] == 555.0, "wrote outside the accumulator"
    return float(h[1])


# ---------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype_name,offs", KERNEL_CASES,
                         ids=["%d-%s-%d_%d" % (n, d, o[0], o[1]) for n, d, o in KERNEL_CASES])
def test_sqnr_add(n, dtype_name, offs):
    ref, x, want = case(n, dtype_name)
    before = A.launch_count()
    first = run(ref, x, dtype_name, offs)
    assert A.launch_count() - before == A.LAUNCHES_PER_BATCH == 2
    second = run(ref, x, dtype_name, offs)
    assert np.float64(first).view(np.uint64) == np.float64(second).view(np.uint64), "two runs differ"
    print("n=%d %s %s: |got - want| / want = %.3e (allowed %.3e)"
          % (n, dtype_name, offs, abs(first - want) / want, O.ratio_bound(n, want) / want))
    assert abs(first - want) <= O.ratio_bound(n, want)
    # x == ref: mean(ref^2) / eps
    same = run(ref, ref.clone(), dtype_name, offs)
    power = qa_oracle.sq_err(ref, ref)[1] / n / O.EPS
    assert O.sqnr_ratio(ref, ref) == power
    assert abs(same - power) <= O.ratio_bound(n, power)


@pytest.mark.parametrize("dtype_name,magnitude", [("fp32", 1e30), ("bf16", 1e30), ("fp16", 4e3)])
@pytest.mark.parametrize("n", [257, 65541])
def test_sqnr_add_large_magnitudes(n, dtype_name, magnitude):
    """1e30-scale outputs (fp16: near its largest values): fp32 squares would overflow."""
    ref, x, want = case(n, dtype_name, magnitude)
    assert dtype_name == "fp16" or qa_oracle.sq_err(ref, x)[1] > 1e59 * n
    got = run(ref, x, dtype_name)
    assert math.isfinite(got) and abs(got - want) <= O.ratio_bound(n, want)
    other_eps = run(ref, x, dtype_name, eps=0.0)
    want0 = O.sqnr_ratio(ref, x, eps=0.0)
    assert abs(other_eps - want0) <= O.ratio_bound(n, want0)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_sqnr_add_accumulates_over_calls(dtype_name):
    acc, want, allowed = 1234.5, 1234.5, 0.0
    for n in (4099, 257, 65541):
        ref, x, ratio = case(n, dtype_name)
        acc = run(ref, x, dtype_name, acc0=acc)
        want += ratio
        allowed += O.ratio_bound(n, ratio, want)
    assert acc > 1234.5 and abs(acc - want) <= allowed


def test_sqnr_add_rejects_bad_arguments():
    lib = _native.load()
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    host = np.zeros(16, np.float32)
    before = A.launch_count()
    ok = (p(buf), p(buf[16:]))
    eps = O.EPS
    assert lib.aimet_amp_sqnr_add(*ok, 0, 0, eps, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(*ok, -1, 0, eps, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(*ok, (1 << 40) + 1, 0, eps, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(*ok, 16, 3, eps, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(*ok, 16, -1, eps, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(*ok, 16, 0, -1.0, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(*ok, 16, 0, math.nan, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(ctypes.c_void_p(buf.data_ptr() + 2), ok[1], 16, 0, eps, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(ok[0], ctypes.c_void_p(buf.data_ptr() + 65), 16, 1, eps, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(*ok, 16, 0, eps, ctypes.c_void_p(acc.data_ptr() + 4), None) != 0
    assert lib.aimet_amp_sqnr_add(ctypes.c_void_p(host.ctypes.data), ok[1], 16, 0, eps, p(acc), None) != 0
    assert lib.aimet_amp_sqnr_add(*ok, 16, 0, eps, ctypes.c_void_p(host.ctypes.data), None) != 0
    torch.cuda.synchronize()
    assert A.launch_count() == before and torch.all(acc == 0)
    assert lib.aimet_amp_sqnr_add(*ok, 16, 0, eps, p(acc), stream()) == 0
    assert A.launch_count() == before + 2
    with pytest.raises(ValueError):
        A.add_sqnr(buf[:4], buf[:5], acc[:1])
    with pytest.raises(ValueError):
        A.add_sqnr(buf[:4].cpu(), buf[:4].cpu(), acc[:1])
    with pytest.raises(ValueError):
        A.add_sqnr(buf[:4], buf[4:8], acc)            # two doubles
    with pytest.raises(ValueError):
        A.add_sqnr(buf[:4].long(), buf[4:8].long(), acc[:1])


# ---------------------------------------------------------------------------------------------------
# 2. the callback
# ---------------------------------------------------------------------------------------------------
class PassThrough(nn.Module):
    """One wrapped Identity in PASSTHROUGH mode: what goes in comes out."""

    def __init__(self):
        super().__init__()
        self.anchor = nn.Parameter(torch.zeros(1, device=DEV))   # where the model lives
        self.layer = StaticGridQuantWrapper(nn.Identity(), 8, 8, "nearest", QuantScheme.post_training_tf_enhanced)
        self.layer.set_mode(QcQuantizeOpMode.PASSTHROUGH)

    def forward(self, x):
        return self.layer(x)


class Loader(list):
    batch_size = None


def recorded(case_):
    """[(ref, x)] float32 host tensors of a fixture case"""
    out = []
    for b in case_["batches"]:
        ref, x = (torch.from_numpy(np.frombuffer(bytes.fromhex(b[k]), dtype=">f4").astype(np.float32).reshape(b["shape"]))
                  for k in ("ref_bits", "x_bits"))
        out.append((ref, x))
    return out


class Recorded:
    """A fixture case behind the callback: the forward_fn hands the pass-through module the recorded
    fp32 output while the quantizers are off, the recorded quantized output otherwise."""

    def __init__(self, case_, cast=None):
        self.batches = recorded(case_)
        if cast is not None:
            self.batches = [(r.to(cast), x.to(cast)) for r, x in self.batches]
        self.loader = Loader(self.batches)
        self.loader.batch_size = case_["batch_size"]
        self.num_samples = case_["num_samples"]
        self.model = PassThrough()
        self.fp32_forwards = self.quantized_forwards = 0
        self.factory = A.EvalCallbackFactory(self.loader, self.forward_fn)
        self.callback = self.factory.sqnr(self.num_samples)

    def forward_fn(self, model, batch):
        ref, x = batch
        assert ref.is_cuda and not model.training and not torch.is_grad_enabled()
        if model.layer.output_quantizers[0].enabled:
            self.quantized_forwards += 1
            return model(x)
        self.fp32_forwards += 1
        return model(ref)

    def evaluate(self):
        return self.callback.func(self.model, self.callback.args)


SQNR_CASES = GOLDEN["sqnr"]["cases"]


def test_the_fixture_has_the_cases_the_callback_is_checked_on():
    by_name = {c["name"]: c for c in SQNR_CASES}
    assert GOLDEN["sqnr"]["eps"] == O.EPS == A.SQNR_EPS
    for c in SQNR_CASES:
        assert all(int(np.prod(b["shape"])) <= 4096 for b in c["batches"])
    seen = {n: sum(b["shape"][0] for b in c["batches"]) for n, c in by_name.items()}
    assert by_name["below"]["num_samples"] < seen["below"] and by_name["above"]["num_samples"] > seen["above"]
    assert all(b["ref_bits"] == b["x_bits"] for b in by_name["equal"]["batches"])


@pytest.mark.parametrize("case_", SQNR_CASES, ids=[c["name"] for c in SQNR_CASES])
def test_callback_against_the_recorded_reference_and_float64(case_):
    r = Recorded(case_)
    took = len(O.taken(r.batches, case_["batch_size"], case_["num_samples"]))
    assert 0 < took <= len(r.batches)
    before = A.launch_count()
    got = r.evaluate()
    assert A.launch_count() - before == 2 * took
    assert (r.fp32_forwards, r.quantized_forwards) == (took, took)
    assert r.factory.stats == {"evaluations": 1, "fp32_forwards": took, "batches": took, "read_backs": 1}
    # the float64 restatement, to the kernel's bound
    want_db, total, allowed = O.evaluate_sqnr_f64(r.batches, case_["batch_size"], case_["num_samples"])
    assert abs(got - want_db) <= O.db_bound(total, allowed, want_db)
    # the reference's recorded float32 value: each of its two means is a float32 sum of n terms
    n = max(ref.numel() for ref, _ in r.batches)
    delta = 2 * (n + 4) * 2.0 ** -24
    print("%s: callback %.12f dB, reference (float32, recorded) %.12f dB, |difference| %.3e dB (allowed %.3e)"
          % (case_["name"], got, case_["db"], abs(got - case_["db"]), 10.0 * math.log10(1.0 + delta)))
    assert abs(got - case_["db"]) <= 10.0 * math.log10(1.0 + delta)
    # the second evaluation reuses the fp32 outputs and gives the same bits
    before = A.launch_count()
    again = r.evaluate()
    assert again == got and A.launch_count() - before == 2 * took
    assert (r.fp32_forwards, r.quantized_forwards) == (took, 2 * took)
    assert r.factory.stats == {"evaluations": 2, "fp32_forwards": took, "batches": 2 * took, "read_backs": 2}
    assert all(q.enabled for q in r.model.layer.output_quantizers)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_callback_takes_16_bit_outputs_as_they_are(dtype):
    case_ = next(c for c in SQNR_CASES if c["name"] == "ragged")
    r = Recorded(case_, cast=dtype)
    got = r.evaluate()
    assert all(t.dtype == dtype for t in r.factory._batchwise_fp32_outputs_list)
    want_db, total, allowed = O.evaluate_sqnr_f64(r.batches, case_["batch_size"], case_["num_samples"])
    assert abs(got - want_db) <= O.db_bound(total, allowed, want_db)


def test_callback_rejects_what_the_kernel_cannot_take():
    case_ = next(c for c in SQNR_CASES if c["name"] == "exact")
    for adapt, match in ((lambda t: t.double(), "float64"), (lambda t: t.long(), "int64"),
                         (lambda t: (t, t), "torch.Tensor"), (lambda t: t.tolist(), "torch.Tensor")):
        r = Recorded(case_)
        plain = r.forward_fn
        r.factory._forward_fn = lambda model, batch: adapt(plain(model, batch))
        with pytest.raises(ValueError, match=match):
            r.evaluate()
        assert all(q.enabled for q in r.model.layer.output_quantizers)
    # the quantized output differs from the fp32 output in shape, then in dtype
    for adapt in (lambda t: t[:, :5], lambda t: t.half()):
        r = Recorded(case_)
        plain, q = r.forward_fn, r.model.layer.output_quantizers[0]
        r.factory._forward_fn = lambda model, batch: adapt(plain(model, batch)) if q.enabled else plain(model, batch)
        with pytest.raises(ValueError, match="fp32 output was"):
            r.evaluate()


def test_default_forward_fn_and_a_real_sim():
    """Without a forward_fn: model(batch); fp32 outputs are those of the sim with every quantizer off."""
    s = Net("chain")
    factory = A.EvalCallbackFactory(s.loader)
    callback = factory.sqnr(num_samples=8)
    got = callback.func(s.sim.model, callback.args)
    pairs = []
    with torch.no_grad():
        for x in s.data[:2]:
            with A._all_quantizers_disabled(s.sim.model):
                fp32 = s.sim.model(x)
            pairs.append((fp32, s.sim.model(x)))
    want_db, total, allowed = O.evaluate_sqnr_f64(pairs, 4, 8)
    assert abs(got - want_db) <= O.db_bound(total, allowed, want_db)
    assert 0.0 < got < 100.0 and factory.stats["fp32_forwards"] == 2


# ---------------------------------------------------------------------------------------------------
# 3. groups
# ---------------------------------------------------------------------------------------------------
class Residual(nn.Module):
    """conv1 - relu1 -+- conv2 -+- add - conv4 - relu2 - flatten - fc
                      +- conv3 -+"""

    def __init__(self):
        super().__init__()
        self.conv1, self.relu1 = nn.Conv2d(3, 8, 3, padding=1), nn.ReLU()
        self.conv2, self.conv3 = nn.Conv2d(8, 8, 3, padding=1), nn.Conv2d(8, 8, 1)
        self.conv4, self.relu2 = nn.Conv2d(8, 4, 1), nn.ReLU()
        self.fc = nn.Linear(4 * 16 * 16, 10)

    def forward(self, x):
        a = self.relu1(self.conv1(x))
        d = operator.add(self.conv2(a), self.conv3(a))
        return self.fc(torch.flatten(self.relu2(self.conv4(d)), 1))


class PoolView(nn.Module):
    """conv1 - maxpool - conv2 - view - fc"""

    def __init__(self):
        super().__init__()
        self.conv1, self.pool = nn.Conv2d(3, 8, 3, padding=1), nn.MaxPool2d(2)
        self.conv2, self.fc = nn.Conv2d(8, 4, 3, padding=1), nn.Linear(4 * 8 * 8, 10)

    def forward(self, x):
        x = self.conv2(self.pool(self.conv1(x)))
        x = x.view(x.size(0), -1)
        return self.fc(x)


def chain():
    """conv - relu - conv - flatten - linear"""
    return nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 8, 3, padding=1), nn.Flatten(),
                         nn.Linear(8 * 16 * 16, 10))


def seeded(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / m.weight[0].numel()) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return net.eval()


def calibrate(model, data):
    for x in data:
        model(x)


class Net:
    """A seeded net, 4 batches of 4 images, and its calibrated sim."""
    MAKERS = {"chain": chain, "residual": Residual, "pool_view": PoolView}

    def __init__(self, kind, device=DEV, output_bw=8, param_bw=8, data_type=INT):
        g = torch.Generator().manual_seed(29)
        self.data = [torch.randn(4, 3, 16, 16, generator=g).to(device) for _ in range(4)]
        self.loader = Loader(self.data)
        self.loader.batch_size = 4
        self.model = seeded(self.MAKERS[kind](), 31).to(device)
        self.dummy = torch.randn(1, 3, 16, 16, generator=g).to(device)
        self.sim = QuantizationSimModel(self.model, self.dummy, quant_scheme=QuantScheme.post_training_tf_enhanced,
                                        default_output_bw=output_bw, default_param_bw=param_bw,
                                        default_data_type=data_type)
        self.forward_pass = CallbackFunc(calibrate, self.data)
        self.sim.compute_encodings(calibrate, self.data)

    def encodings(self):
        """{quantizer name: (bitwidth, data type, encodings as tuples or None)} of the enabled quantizers"""
        out = {}
        for name, w in self.sim.quant_wrappers():
            named = [("in%d" % i, q) for i, q in enumerate(w.input_quantizers)] + \
                [("out%d" % i, q) for i, q in enumerate(w.output_quantizers)] + list(w.param_quantizers.items())
            for kind, q in named:
                if q.enabled:
                    e = q.encoding
                    e = None if e is None else [x.to_tuple() for x in (e if isinstance(e, list) else [e])]
                    out["%s.%s" % (name, kind)] = (q.bitwidth, q.data_type, e)
        return out


def at(group, candidate):
    """What group.get_candidate() gives with the group at `candidate`."""
    return (candidate[0] if group.input_quantizers or group.output_quantizers else (None, None),
            candidate[1] if group.parameter_quantizers else (None, None))


def G(inputs=(), outputs=(), params=(), kernel_ops=()):
    return QuantizerGroup(tuple("%s_input_quantizer_idx_%d" % i for i in inputs), tuple(outputs), tuple(params),
                          tuple(kernel_ops))


# By the rules: a group per model-input op (its enabled input quantizers and its parameters); a group per
# parent (its enabled output quantizers, the enabled input and parameter quantizers of its children);
# a group per enabled model-output quantizer. Only the first wrapper's input quantizer is enabled; bias
# quantizers are off. ReLU and operator.add are ops without quantizers; flatten, view and max-pool are
# looked through; size is not traversed.
BY_HAND = {
    "chain": [G(inputs=[("0", 0)], params=["0"], kernel_ops=["0"]),     # the model input and conv 0
              G(outputs=["0"]),                                         # conv 0 -> relu
              G(params=["2"], kernel_ops=["2"]),                        # relu -> conv 2
              G(outputs=["2"], params=["4"], kernel_ops=["4"]),         # conv 2 -> (flatten) -> linear
              G(outputs=["4"])],                                        # the model output
    "residual": [G(inputs=[("conv1", 0)], params=["conv1"], kernel_ops=["conv1"]),
                 G(outputs=["conv1"]),                                                  # conv1 -> relu1
                 G(params=["conv2", "conv3"], kernel_ops=["conv2", "conv3"]),           # relu1 fans out
                 G(outputs=["conv2"]),                                                  # conv2 -> add
                 G(outputs=["conv3"]),                                                  # conv3 -> add
                 G(params=["conv4"], kernel_ops=["conv4"]),                             # add -> conv4
                 G(outputs=["conv4"]),                                                  # conv4 -> relu2
                 G(params=["fc"], kernel_ops=["fc"]),                                   # relu2 -> (flatten) -> fc
                 G(outputs=["fc"])],
    "pool_view": [G(inputs=[("conv1", 0)], params=["conv1"], kernel_ops=["conv1"]),
                  G(outputs=["conv1"], params=["conv2"], kernel_ops=["conv2"]),         # conv1 -> (maxpool) -> conv2
                  G(outputs=["conv2"], params=["fc"], kernel_ops=["fc"]),               # conv2 -> (view) -> fc
                  G(outputs=["fc"])],
}


@pytest.fixture(scope="module")
def nets():
    return {kind: Net(kind) for kind in Net.MAKERS}


@pytest.mark.parametrize("kind", list(Net.MAKERS))
def test_quantizer_groups_equal_the_groups_by_hand(nets, kind):
    s = nets[kind]
    wrappers, groups = find_quantizer_group(s.sim)
    assert wrappers == dict(s.sim.quant_wrappers())
    assert groups == BY_HAND[kind]
    # every enabled quantizer is in exactly one group
    enabled = [q for _, w in s.sim.quant_wrappers()
               for q in list(w.input_quantizers) + list(w.output_quantizers) + list(w.param_quantizers.values())
               if q.enabled]
    grouped = [q for g in groups for q in g.get_active_quantizers(wrappers)]
    assert sorted(map(id, grouped)) == sorted(map(id, enabled))


def test_untraceable_model_names_amp():
    class Branchy(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(3, 4, 3)

        def forward(self, x):
            y = self.conv(x)
            return y if y.sum() > 0 else -y
    model = seeded(Branchy(), 3).to(DEV)
    sim = QuantizationSimModel(model, torch.randn(1, 3, 16, 16, device=DEV))
    with pytest.raises(RuntimeError, match=r"(?s)automatic mixed precision \(AMP\).*torch.fx cannot trace"):
        find_quantizer_group(sim)


def test_mac_dict(nets):
    assert create_mac_dict(nets["chain"].sim.model, nets["chain"].dummy) == {
        "0": 8 * 3 * 9 * 256, "2": 8 * 8 * 9 * 256, "4": 10 * 8 * 256}
    assert create_mac_dict(nets["pool_view"].sim.model, nets["pool_view"].dummy) == {
        "conv1": 8 * 3 * 9 * 256, "conv2": 4 * 8 * 9 * 64, "fc": 10 * 4 * 64}


# ---------------------------------------------------------------------------------------------------
# 4. candidates
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("candidate", [((4, INT), (4, INT)), ((8, INT), (16, INT)), ((16, INT), (8, INT)),
                                       ((16, FLOAT), (16, FLOAT))],
                         ids=["a4w4", "a8w16", "a16w8", "fp16"])
def test_candidate_encodings_equal_a_fresh_sims(candidate):
    s = Net("chain")
    wrappers, groups = find_quantizer_group(s.sim)
    for g in groups:
        g.set_quantizers_to_candidate(wrappers, candidate)
        assert g.get_candidate(wrappers) == at(g, candidate)
    s.sim.compute_encodings(calibrate, s.data)
    (act_bw, act_type), (param_bw, param_type) = candidate
    fresh = Net("chain", output_bw=act_bw, param_bw=param_bw, data_type=act_type)
    got, want = s.encodings(), fresh.encodings()
    assert list(got) == list(want) and len(got) == 7
    assert got == want
    assert all((bw, dt) == ((param_bw, param_type) if name.endswith(".weight") else (act_bw, act_type))
               for name, (bw, dt, _) in got.items())
    if act_type == INT:
        assert all(e is not None and e[0][4] == bw for bw, _, e in got.values())
    with torch.no_grad():
        assert torch.equal(s.sim.model(s.data[0]), fresh.sim.model(s.data[0]))


# ---------------------------------------------------------------------------------------------------
# 5. end to end
# ---------------------------------------------------------------------------------------------------
CANDIDATES = [((16, INT), (16, INT)), ((16, INT), (8, INT)), ((8, INT), (8, INT))]


class EndToEnd:
    def __init__(self, results_dir, device=DEV, kind="residual", **kwargs):
        self.net = Net(kind, device)
        self.factory = A.EvalCallbackFactory(self.net.loader)
        self.callback = self.factory.sqnr(num_samples=16)
        self.results_dir = str(results_dir)
        self.kwargs = kwargs

    def run(self, drop, algo=AMPSearchAlgo.BruteForce, **kwargs):
        args = dict(self.kwargs)
        args.update(kwargs)
        return choose_mixed_precision(self.net.sim, self.net.dummy, CANDIDATES, self.callback, self.callback, drop,
                                      self.results_dir, True, self.net.forward_pass, amp_search_algo=algo, **args)

    def score(self):
        return self.callback.func(self.net.sim.model, None)

    def state(self):
        wrappers, groups = find_quantizer_group(self.net.sim)
        return [g.get_candidate(wrappers) for g in groups]


@pytest.fixture(scope="module")
def full_curve(tmp_path_factory):
    """choose_mixed_precision with allowed_accuracy_drop=None under brute force: (setup, Pareto list)"""
    e = EndToEnd(tmp_path_factory.mktemp("amp"))
    return e, e.run(None)


def test_full_pareto_curve(full_curve):
    e, pareto = full_curve
    wrappers, groups = find_quantizer_group(e.net.sim)
    assert len(groups) == 9 and len(pareto) == len(groups) * (len(CANDIDATES) - 1)
    bit_ops = [entry[0] for entry in pareto]
    assert all(b1 <= b0 for b0, b1 in zip(bit_ops, bit_ops[1:])) and bit_ops[0] <= 1.0 and bit_ops[-1] > 0.0
    assert {(g, c) for _, _, g, c in pareto} == {(g, c) for g in groups for c in CANDIDATES[1:]}
    assert all(math.isfinite(score) for _, score, _, _ in pareto)
    # target -inf: the whole list is applied
    applied = {}
    for _, _, g, c in pareto:
        applied[g] = c
    assert [g.get_candidate(wrappers) for g in groups] == [at(g, applied[g]) for g in groups]


def test_every_pareto_score_is_the_score_of_its_prefix(full_curve):
    e, pareto = full_curve
    fresh = EndToEnd(e.results_dir)
    wrappers, groups = find_quantizer_group(fresh.net.sim)
    for g in groups:
        g.set_quantizers_to_candidate(wrappers, CANDIDATES[0])
    for i, (_, score, group, candidate) in enumerate(pareto):
        group.set_quantizers_to_candidate(wrappers, candidate)      # cumulative: the prefix 0 .. i
        fresh.net.sim.compute_encodings(calibrate, fresh.net.data)
        assert fresh.score() == score, i


def test_result_files_exist_and_parse(full_curve):
    e, pareto = full_curve
    d = e.results_dir
    rows = json.load(open(os.path.join(d, "pareto_list.json")))
    assert [r[:2] for r in rows] == [list(entry[:2]) for entry in pareto]
    assert len(json.load(open(os.path.join(d, ".cache", "accuracy_list.json")))) == len(pareto)
    info = dict(json.load(open(os.path.join(d, "amp_info_list.json"))))
    assert info["phase2 eval count"] == len(pareto) and info["total_quantizers"] == 11
    assert json.load(open(os.path.join(d, "pareto_curve.json")))["Accuracy"] == [entry[1] for entry in pareto]
    assert len(json.load(open(os.path.join(d, "quantizer_group_sensitivity.json")))["entries"]) == len(pareto)
    for name in ("accuracy_list.pkl", "pareto_list.pkl"):
        assert os.path.getsize(os.path.join(d, ".cache", name)) > 0


@pytest.mark.parametrize("algo", list(AMPSearchAlgo), ids=[a.name for a in AMPSearchAlgo])
def test_finite_drop_leaves_a_configuration_that_meets_it(full_curve, algo, tmp_path):
    _, full = full_curve
    e = EndToEnd(tmp_path)
    scores = [score for _, score, _, _ in full]
    middle = len(scores) // 2
    target = (scores[middle] + scores[middle + 1]) / 2      # between two points of the full curve
    with A._all_quantizers_disabled(e.net.sim.model):
        fp32 = e.score()                                    # x == ref: mean(ref^2) / eps per batch
    drop = fp32 - target
    pareto = e.run(drop, algo)
    assert pareto is not None and 0 < len(pareto) <= len(full)
    final = e.score()
    print("%s: fp32 %.4f dB, allowed drop %.4f dB, final %.4f dB after %d of %d Pareto points"
          % (algo.name, fp32, drop, final, len(pareto), len(full)))
    assert math.isfinite(final)
    if algo == AMPSearchAlgo.BruteForce:
        # the first point below the target ends the search; the one before it is applied. The other two
        # searches bisect and promise this only for a monotone curve.
        assert final >= fp32 - drop
        assert [entry[:2] for entry in pareto] == [entry[:2] for entry in full[:len(pareto)]]
    e.net.sim.compute_encodings(calibrate, e.net.data)
    assert e.score() == final                               # the sim was left calibrated at that point


def test_early_exits_return_none(tmp_path):
    e = EndToEnd(tmp_path)
    with A._all_quantizers_disabled(e.net.sim.model):
        fp32 = e.score()
    # the best candidate already misses the drop: the sim stays at the baseline candidate
    assert e.run(1e-3) is None
    assert e.state() == [at(g, CANDIDATES[0]) for g in find_quantizer_group(e.net.sim)[1]]
    # the lowest candidate meets the drop: every group goes there
    assert e.run(fp32 + 1000.0) is None
    assert e.state() == [at(g, CANDIDATES[2]) for g in find_quantizer_group(e.net.sim)[1]]
    assert not os.path.exists(os.path.join(str(tmp_path), "pareto_list.json"))


def test_phase1_optimize_on_and_off_give_the_same_order(tmp_path):
    lists = []
    for optimize in (True, False):
        e = EndToEnd(tmp_path / str(optimize))
        algo = A.GreedyMixedPrecisionAlgo(e.net.sim, e.net.dummy, CANDIDATES, e.callback, e.callback, e.results_dir,
                                          True, e.net.forward_pass, phase1_optimize=optimize)
        algo.run(None, AMPSearchAlgo.Binary)
        lists.append([(g, c) for g, c, _, _ in algo.accuracy_list])
        for (_, _, s, _), (_, _, s_next, _) in zip(algo.accuracy_list, algo.accuracy_list[1:]):
            assert s >= s_next
    assert lists[0] == lists[1] and len(lists[0]) == 18


def test_set_quantizer_groups_candidates(tmp_path):
    e = EndToEnd(tmp_path)
    algo = A.GreedyMixedPrecisionAlgo(e.net.sim, e.net.dummy, CANDIDATES, e.callback, e.callback, e.results_dir, True,
                                      e.net.forward_pass)
    groups = algo.quantizer_groups
    with_params, without = next(g for g in groups if g.parameter_quantizers), next(
        g for g in groups if not g.parameter_quantizers)
    algo.set_quantizer_groups_candidates([(with_params, CANDIDATES[2]), (without, ((8, INT), (4, INT)))])
    wrappers = algo._module_name_dict
    assert with_params.get_candidate(wrappers) == CANDIDATES[2]
    assert without.get_candidate(wrappers) == ((8, INT), (None, None))
    q = with_params.get_active_quantizers(wrappers)[-1]
    assert q.bitwidth == 8 and q.encoding is not None
    with pytest.raises(AssertionError):
        algo.set_quantizer_groups_candidates([(with_params, ((4, INT), (4, INT)))])
    with pytest.raises(AssertionError):
        algo.set_quantizer_groups_candidates([(without, ((4, INT), (8, INT)))])


def test_raising_callback_restores_the_sim(tmp_path):
    e = EndToEnd(tmp_path)
    calls = []

    def raising(model, args):
        calls.append(1)
        if len(calls) == 9:         # fp32, three baselines, then the fifth score of phase 1
            raise KeyError("phase 1")
        return e.callback.func(model, args)
    algo = A.GreedyMixedPrecisionAlgo(e.net.sim, e.net.dummy, CANDIDATES, CallbackFunc(raising), CallbackFunc(raising),
                                      e.results_dir, True, e.net.forward_pass, phase1_optimize=True)
    algo.set_baseline()
    before = [(q.enabled, q.bitwidth, q.data_type) for _, w in e.net.sim.quant_wrappers()
              for q in list(w.input_quantizers) + list(w.output_quantizers) + list(w.param_quantizers.values())]
    with pytest.raises(KeyError):
        algo.run(None, AMPSearchAlgo.Binary)
    assert [(q.enabled, q.bitwidth, q.data_type) for _, w in e.net.sim.quant_wrappers()
            for q in list(w.input_quantizers) + list(w.output_quantizers) + list(w.param_quantizers.values())] == before


def test_cpu_resident_model(tmp_path):
    """The model's layers run where it lives; the outputs are copied to the device for the reduction."""
    e = EndToEnd(tmp_path, device="cpu", kind="pool_view")
    assert all(not t.is_cuda for t in e.net.model.parameters())
    before = A.launch_count()
    pareto = e.run(None)
    assert len(pareto) == 4 * 2 and A.launch_count() > before
    bit_ops = [entry[0] for entry in pareto]
    assert all(b1 <= b0 for b0, b1 in zip(bit_ops, bit_ops[1:]))
    assert all(t.is_cuda for t in e.factory._batchwise_fp32_outputs_list)
