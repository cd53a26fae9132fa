"""AdaRound per-layer rounding optimisation on the fused soft-quant kernels.

Mirrors aimet_torch/v1/adaround/adaround_optimizer.py:115-222 (AdaroundOptimizer._optimize_rounding)
with the loss of adaround_loss.py:70-133 and the hyper-parameters of AdaroundParameters
(adaround_weight.py: 10000 iterations, reg 0.01, beta 20 -> 2, warm start 0.2): Adam on alpha,
batches of 32 cached (input, fp output) pairs drawn by randperm, reconstruction loss
||q_out - fp_out||_F^2 over dim 1 averaged, rounding loss reg * sum(1 - |2h(alpha) - 1|^beta) after
the warm start with cosine-annealed beta.

MI355X-first: the soft-quantized weight is ONE kernel (aimet_adaround_forward) and its backward ONE
kernel (aimet_adaround_backward) that also adds the rounding-loss gradient -- the reference builds
both from ~16 torch ops per iteration (adaround_wrapper.py:124-149 + compute_round_loss) and runs
the rounding loss as a separate autograd graph. The rounding-loss VALUE is accumulated on the device
(no host sync per iteration) and read back only when asked. The reconstruction loss and its backward
(~12 torch kernels over the layer output) are one pass too (aimet_adaround_recon_grad).

The loop is launch-bound for MobileNet-sized layers, so by default one iteration is captured in a
HIP graph and replayed (batch indices drawn up front in the eager loop's order, the annealed beta
read from device memory, Adam capturable); depthwise convolutions run on PyTorch's native kernels
(3-5x faster than MIOpen's here). MobileNet-v2, 53 layers: 0.0545 ms per iteration
(profiles/r05/adaround_mobilenet_10k.json). plan_loop picks a layer's form from its shapes alone, the
form's builder (_STEP_BUILDERS) the buffers and launches of one iteration around the shared
_LoopState, _run_captured captures and replays them.

Data parallel (adaround_optimizer.py:139-160,214-216), when torch.distributed is initialised (or a
group is given): the cached samples are sharded rank::world, Adam's learning rate is multiplied by
the world size, each rank runs num_iterations // world iterations on batches from its shard, and
alpha.grad is all-reduced (SUM) and divided by the world size before every Adam step. As in the
reference, the rounding-loss schedule keeps num_iterations as its horizon (so with world > 1 the
iterations run are the first 1/world of it). In the HIP-graph form the iteration is two graphs with
the collective between them: [forward + backward] -> all_reduce(alpha.grad) -> [/ world + Adam].
"""
import contextlib
import logging
import math
import warnings
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import ctypes

import torch
import torch.distributed as dist
import torch.nn.functional as F

from aimet_amd import _native
from aimet_amd.adaround import (AdaroundFunction, compute_beta, exact_pow_needed, get_exact_pow, init_alpha,
                                set_exact_pow)
from aimet_amd.tensor_quantizer import per_channel_view

BATCH_SIZE = 32   # adaround_optimizer.py:58
_log = logging.getLogger("aimet_amd.adaround")


@dataclass
class AdaroundHyperParameters:
    """adaround_loss.py:46-63 (defaults of AdaroundParameters, adaround_weight.py)."""
    num_iterations: int = 10000
    reg_param: float = 0.01
    beta_range: Tuple[float, float] = (20, 2)
    warm_start: float = 0.2


def layer_forward(module: torch.nn.Module, inp: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """The wrapped layer's forward with `weight` in place of its parameter
    (adaround_optimizer.py:257-286 _compute_output_with_adarounded_weights). The bias enters
    detached: only alpha is optimised, so its gradient (a reduction over the whole layer output
    per iteration) is never needed."""
    bias = module.bias.detach() if module.bias is not None else None
    if isinstance(module, torch.nn.Conv2d):
        return F.conv2d(inp, weight, bias, module.stride, module.padding, module.dilation, module.groups)
    if isinstance(module, torch.nn.Conv1d):
        return F.conv1d(inp, weight, bias, module.stride, module.padding, module.dilation, module.groups)
    if isinstance(module, torch.nn.Linear):
        return F.linear(inp, weight, bias)
    if isinstance(module, torch.nn.ConvTranspose2d):
        return F.conv_transpose2d(inp, weight, bias, module.stride, module.padding, module.output_padding,
                                  module.groups, module.dilation)
    raise NotImplementedError("AdaRound supports Conv1d / Conv2d / ConvTranspose2d / Linear (got %s)"
                              % type(module).__name__)


@contextlib.contextmanager
def conv_backend(module: torch.nn.Module):
    """Context for a layer's whole iteration (forward AND autograd backward, which picks its
    backend when it runs): depthwise convolutions on PyTorch's native depthwise kernels, 3-5x
    faster than MIOpen's for the forward + weight gradient at MobileNet-v2 shapes on MI355X
    (tools/studies/dw_conv_time.py); MIOpen restricted to deterministic solutions (its weight-gradient
    kernels may add partial sums atomically: the optimised alpha of two runs with one seed then
    differed, tools/studies/adaround_loop_divergence.py)."""
    depthwise = isinstance(module, torch.nn.Conv2d) and 1 < module.groups == module.in_channels
    prev, prev_det = torch.backends.cudnn.enabled, torch.backends.cudnn.deterministic
    torch.backends.cudnn.enabled = prev and not depthwise
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.enabled = prev
        torch.backends.cudnn.deterministic = prev_det


# The loop's forms are fixed rules by layer shape, never timings, so two runs with the same seed give
# the same alpha. The module-level switches below select between forms that the tests compare
# (tests/test_adaround_wrapper.py patches them); none is read from the environment.

# depthwise layers: the whole iteration up to dL/dWq as one pass over the cached rows
# (aimet_adaround_dw_step, bit-identical to gather + forward + reconstruction gradient + weight
# gradient); False runs those four launches instead (the tests' comparison)
_DW_FUSED = True
# the depthwise / 1x1 one-pass steps' weight-gradient slices folded by the Adam step
# (aimet_adaround_backward_adam_parts with part_kk: the folds' sums, one launch fewer per iteration)
_DW_FOLD_ADAM = True
# 1x1 layers / the unfolded stem with few input channels (Cin <= 192, HW % 4 == 0)
# can run the iteration up to dL/dWq as one pass too (aimet_adaround_pw_step: q, g and the gradient
# partials on chip; sums in a fixed order, not a library GEMM's). "auto" (default) takes it for every
# eligible layer with >= 28 x 28 positions except the projecting ones (C_in > C_out) below 56 x 56,
# where the GEMM form measured faster (MobileNet-v2 per iteration: 0.24 -> 0.16 ms at 16 -> 96 x
# 112^2, 0.127 -> 0.088 at 24 -> 144 x 56^2, the stem 0.172 -> 0.133; 192 -> 32 x 28^2: 0.074 vs
# 0.092; 64 -> 384 x 14^2: 0.064 vs 0.076; profiles/r03/adaround_pw_fused_forms.txt). Since the step
# runs on the matrix cores for C_in >= 32 (round 4), the projecting layers at 28 x 28 with C_in >= 32
# take it too (144 -> 32: 0.073 -> 0.056 ms, 192 -> 32: 0.070 -> 0.067; profiles/r04/
# adaround_pw_fused_all.txt) when the step does run them on the matrix cores
# (aimet_adaround_pw_step_uses_mfma; the VALU form is slower than the GEMM form there); below 28 x 28
# the channel-major GEMMs stay faster. "all": every eligible layer, "0": none.
_PW_FUSED = "auto"
# iterations per captured HIP graph in the single-process loop: one hipGraphLaunch per iteration
# left the GPU waiting on the host between replays for small layers (a depthwise layer's ~10 us of
# kernels per iteration in a ~100 us window, profiles/r04/adaround_loop_summary.txt); the counters and
# the batch table live on the device, so k consecutive iterations are one graph. Results are those
# of one iteration per graph, bit for bit.
_GRAPH_ITERS = 10


def _pw_step_uses_mfma(cin: int, cout: int) -> bool:
    """aimet_adaround_pw_step runs (cin, cout) on the matrix cores (else its VALU form)."""
    uses = ctypes.c_int()
    _native.call("aimet_adaround_pw_step_uses_mfma", int(cin), int(cout), ctypes.byref(uses))
    return bool(uses.value)


def _is_pointwise(module: torch.nn.Module) -> bool:
    return isinstance(module, torch.nn.Conv2d) and module.kernel_size == (1, 1) and module.stride == (1, 1) \
        and module.padding in ((0, 0), "valid") and module.dilation == (1, 1) and module.groups == 1


# im2col form of small-Cin convolutions (the stem): C_in * k * k at most this, and the unfolded
# input cache at most this many bytes
_IM2COL_MAX_K = 64
_IM2COL_MAX_BYTES = 8 << 30


def _im2col_ok(module: torch.nn.Module, in_shape, itemsize: int) -> bool:
    """A groups-1 Conv2d (not 1x1 / stride 1, which _is_pointwise runs directly) whose
    C_in * kh * kw <= _IM2COL_MAX_K and whose unfolded input cache (in_shape: the cache's
    [N, C_in, H, W]) fits _IM2COL_MAX_BYTES: its loop runs as the pointwise form on the unfolded
    cache (deterministic GEMMs; MIOpen's deterministic stem solutions were 4x slower than its
    default ones)."""
    if not isinstance(module, torch.nn.Conv2d) or module.groups != 1 or _is_pointwise(module) \
            or module.padding_mode != "zeros" or isinstance(module.padding, str) or len(in_shape) != 4:
        return False
    kdim = module.in_channels * module.kernel_size[0] * module.kernel_size[1]
    if kdim > _IM2COL_MAX_K:
        return False
    h, w = in_shape[2], in_shape[3]
    oh = (h + 2 * module.padding[0] - module.dilation[0] * (module.kernel_size[0] - 1) - 1) // module.stride[0] + 1
    ow = (w + 2 * module.padding[1] - module.dilation[1] * (module.kernel_size[1] - 1) - 1) // module.stride[1] + 1
    return in_shape[0] * kdim * oh * ow * itemsize <= _IM2COL_MAX_BYTES


def depthwise_spec(module: torch.nn.Module):
    """(K, stride, padding, dilation) when `module` is a depthwise Conv2d the native depthwise
    kernels (aimet_dwconv2d_*) run: groups == in == out channels, square K in {3, 5}, square
    stride / padding / dilation, zero padding; else None."""
    if not isinstance(module, torch.nn.Conv2d) or not (module.groups == module.in_channels == module.out_channels) \
            or module.groups == 1 or module.padding_mode != "zeros" or isinstance(module.padding, str):
        return None
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = module.kernel_size, module.stride, module.padding, module.dilation
    if kh != kw or kh not in (3, 5) or sh != sw or ph != pw or dh != dw:
        return None
    return kh, sh, ph, dh


def recon_loss(quant_out: torch.Tensor, orig_out: torch.Tensor) -> torch.Tensor:
    """adaround_loss.py:70-80."""
    return (torch.norm(quant_out - orig_out, p="fro", dim=1) ** 2).mean()


def _act_code(act_func) -> Optional[int]:
    """The fused reconstruction-loss kernel's activation code, None when it has no fused form."""
    if act_func is None:
        return 0
    if isinstance(act_func, torch.nn.ReLU6) or act_func is F.relu6:
        return 2
    if isinstance(act_func, torch.nn.ReLU) or act_func in (F.relu, torch.relu):
        return 1
    return None


def recon_loss_backward(quant_out: torch.Tensor, orig_out: torch.Tensor, act_func=None):
    """recon_loss(act(quant_out), act(orig_out)).backward() as ONE kernel (aimet_adaround_recon_grad:
    the gradient 2 (act(q) - act(t)) act'(q) / count, then autograd from quant_out on); other
    activations take the torch-op form."""
    code = _act_code(act_func)
    if code is None or quant_out.dtype != torch.float32 or quant_out.dim() < 2:
        q, t = (act_func(quant_out), act_func(orig_out)) if act_func is not None else (quant_out, orig_out)
        recon_loss(q, t).backward()
        return
    q = quant_out.detach()
    q = q if q.is_contiguous() else q.contiguous()
    t = orig_out if orig_out.is_contiguous() else orig_out.contiguous()
    g = torch.empty_like(q)
    _native.call("aimet_adaround_recon_grad", q.data_ptr(), t.data_ptr(), g.data_ptr(), q.numel(), q.shape[1], code,
                 torch.cuda.current_stream(q.device).cuda_stream)
    quant_out.backward(g)


class _BoundSoftQuant:
    """The per-iteration soft quantization of ONE layer with every kernel argument bound once
    (weight, alpha, delta, offset and the Wq / grad-alpha buffers keep their addresses for the
    whole optimisation): a forward and a backward are one direct library call each, no per-call
    Python argument marshalling (the loop is launch-bound for MobileNet-sized weights)."""

    def __init__(self, w, alpha, d, o, bitwidth, ch_axis, round_loss_out):
        lib = _native.load()
        self.fwd, self.bwd = lib.aimet_adaround_forward, lib.aimet_adaround_backward
        self.bwd_dev = lib.aimet_adaround_backward_dev
        self.w, self.alpha = w.contiguous(), alpha
        outer, C, K = per_channel_view(self.w.shape, ch_axis) if d.numel() > 1 else (1, 1, self.w.numel())
        self.shape = (outer, C, K)
        self.d, self.o = d.contiguous(), o.contiguous()
        self.bw = int(bitwidth)
        self.loss = round_loss_out
        self.pw, self.pa, self.pd, self.po = _ptr(self.w), _ptr(alpha), _ptr(self.d), _ptr(self.o)
        self.pl = _ptr(round_loss_out) if round_loss_out is not None else None
        self.reg = self.beta = 0.0
        self.reg_beta = None   # graph mode: device tensor [reg, beta, beta - 1] read by the backward kernel

    def forward(self):
        wq = torch.empty_like(self.w)    # fresh outputs: autograd may keep / steal them
        rc = self.fwd(self.pw, self.pa, ctypes.c_void_p(wq.data_ptr()), *self.shape, self.pd, self.po, self.bw, 1,
                      _stream_ptr(self.w.device))
        if rc:
            _native.check(rc)
        return wq

    def backward(self, grad):
        g = grad if grad.is_contiguous() else grad.contiguous()
        ga = torch.empty_like(self.w)
        if self.reg_beta is not None:
            rc = self.bwd_dev(self.pw, self.pa, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(ga.data_ptr()),
                              *self.shape, self.pd, self.po, self.bw, ctypes.c_void_p(self.reg_beta.data_ptr()),
                              self.pl, _stream_ptr(self.w.device))
        else:
            rc = self.bwd(self.pw, self.pa, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(ga.data_ptr()),
                          *self.shape, self.pd, self.po, self.bw, ctypes.c_double(self.reg), ctypes.c_double(self.beta),
                          self.pl if self.reg != 0.0 else None, _stream_ptr(self.w.device))
        if rc:
            _native.check(rc)
        return ga


class _SoftQuantFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, bound):
        ctx.bound = bound
        return bound.forward()

    @staticmethod
    def backward(ctx, grad):
        return ctx.bound.backward(grad), None


def _group_world(group):
    if not (dist.is_available() and dist.is_initialized()):
        return 0, 1
    return dist.get_rank(group), dist.get_world_size(group)


def _reduce_grad(grad, world, group, divide=True):
    """adaround_optimizer.py:214-216: all_reduce(alpha.grad) (SUM), then / world_size."""
    if world > 1:
        if grad.is_cuda and dist.get_backend(group) == "gloo":
            h = grad.cpu()
            dist.all_reduce(h, group=group)
            grad.copy_(h)
        else:
            dist.all_reduce(grad, group=group)
    if divide:
        grad.div_(world)


def _starting_alpha(w, d, shape, alpha_init):
    """The optimised alpha: a float32 copy of the caller's (an AdaroundWrapper's parameter) or
    init_alpha of the weight (_generate_alpha_parameter, adaround_wrapper.py:211-224)."""
    if alpha_init is not None:
        if alpha_init.shape != w.shape:
            raise ValueError("alpha has shape %s, the weight %s" % (tuple(alpha_init.shape), tuple(w.shape)))
        return torch.nn.Parameter(alpha_init.detach().to(w.device, torch.float32).contiguous().clone(),
                                  requires_grad=True)
    return init_alpha(w, d.view(shape) if d.numel() > 1 else d)


def _finish_alpha(alpha, alpha_init):
    """The optimised values written back into the caller's alpha (returned), else alpha."""
    if alpha_init is None:
        return alpha
    with torch.no_grad():
        alpha_init.copy_(alpha.detach())
    return alpha_init


def _loop_setup(module, delta, offset, ch_axis, alpha_init):
    """(weight, device, delta, offset, alpha) of a layer's loop, the encoding as flat float32 vectors."""
    w = module.weight.detach()
    shape = [1] * w.dim()
    shape[ch_axis] = -1
    d = torch.as_tensor(delta, dtype=torch.float32, device=w.device).reshape(-1).contiguous()
    o = torch.as_tensor(offset, dtype=torch.float32, device=w.device).reshape(-1).contiguous()
    return w, w.device, d, o, _starting_alpha(w, d, shape, alpha_init)


def _torch_adam(alpha, world, **kw):
    # one Adam kernel per step (the reference's default multi-tensor Adam: same update rule); the
    # learning rate scaled by the world size (adaround_optimizer.py:155-158)
    try:
        return torch.optim.Adam([alpha], lr=1e-3 * world, fused=True, **kw)
    except (RuntimeError, TypeError):
        return torch.optim.Adam([alpha], lr=1e-3 * world, **kw)


@dataclass(frozen=True)
class LoopPlan:
    """The fused loop's form for one layer (plan_loop)."""
    form: str                       # what last_loop_form reports
    fallback: Optional[str] = None  # the form to run when `form` cannot be captured
    indexed: bool = False           # the reconstruction gradient reads the fp target in place
    C_out: int = 1
    hw: int = 1                     # output positions per channel
    cin: int = 0                    # GEMM forms: the inner dimension (C_in, or C_in k k unfolded)
    dw: Optional[Tuple[int, int, int, int]] = None   # depthwise (K, stride, pad, dil)


def plan_loop(module, in_shape, in_dtype, out_shape, out_dtype, act_func, aligned: bool) -> LoopPlan:
    """The form of the fused loop for `module` on caches of these shapes ([N, ...]) and dtypes.
    aligned: the caches the loop reads start on 16-byte boundaries."""
    # A pure function of its arguments and the switches above: nothing is allocated or launched
    # (aimet_adaround_pw_step_uses_mfma is a host-only query).
    # The fused reconstruction gradient reads the fp target in place (no gathered copy) when it
    # has a fused form: [N, C, ...] float32 outputs, ReLU / ReLU6 / no activation
    indexed = _act_code(act_func) is not None and len(out_shape) >= 2 and out_dtype == torch.float32
    if not indexed:
        return LoopPlan("autograd")
    C_out, hw = out_shape[1], math.prod(out_shape[2:])
    if len(out_shape) == 4 and _im2col_ok(module, in_shape, in_dtype.itemsize):
        # the cached inputs unfolded once ([N, C_in k k, OH OW]): a pointwise problem
        form, cin, hw_in = "im2col", in_shape[1] * module.kernel_size[0] * module.kernel_size[1], hw
    elif depthwise_spec(module) is not None and len(in_shape) == 4:
        return LoopPlan("dw", None, True, C_out, hw, dw=depthwise_spec(module))
    elif _is_pointwise(module) and len(in_shape) == 4:
        form, cin, hw_in = "pointwise", in_shape[1], in_shape[2] * in_shape[3]
    elif isinstance(module, torch.nn.Linear) and len(in_shape) == 2:
        return LoopPlan("linear", "autograd", True, C_out, hw)
    else:
        return LoopPlan("autograd", None, True, C_out, hw)
    wanted = _PW_FUSED == "all" or (_PW_FUSED != "0" and hw >= 28 * 28 and (
        not (cin > C_out and hw < 56 * 56) or (cin >= 32 and _pw_step_uses_mfma(cin, C_out))))
    if wanted and cin <= 192 and hw_in == hw and hw % 4 == 0 and aligned:
        form += "_fused"
    elif hw <= 14 * 14:
        form += "_cm"
    # 1x1 and linear layers have a second form (MIOpen through autograd) that sums the weight
    # gradient in another order: it runs only when the first cannot be captured
    return LoopPlan(form, "autograd" if form.startswith("pointwise") else None, True, C_out, hw, cin)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream_ptr(dev):
    # the current stream at call time: a HIP-graph capture runs on torch's capture stream
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


_ADAM = tuple(ctypes.c_double(v) for v in (1e-3, 0.9, 0.999, 1e-8))   # lr, beta1, beta2, eps
_CHUNK = 500   # iterations per host draw of batch indices (_drawer)


class _LoopState:
    """What every form of the fused loop shares, built once per layer."""
    # alpha and its Adam moments, the device-side iteration counters [it_cur, it_next], the batch
    # table idx_all, the {reg, beta, beta - 1} table rb_all, Adam's bias corrections, the
    # soft-quantized weight wq and the caches. A form's builder (_STEP_BUILDERS) adds its own
    # buffers and returns its step(stream): the launches of one iteration.

    def __init__(self, plan, module, inp_data, out_data, sq, iters, idx_all, rb_all, act_func, round_loss_out):
        self.plan, self.module, self.sq, self.alpha, self.dev = plan, module, sq, sq.alpha, sq.w.device
        self.inp_data, self.out_data, self.iters, self.nb = inp_data, out_data, iters, idx_all.shape[1]
        self.idx_all, self.rb_all, self.act_func, self.loss = idx_all, rb_all, act_func, round_loss_out
        self.lib = _native.load()
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.alpha), torch.zeros_like(self.alpha)
        self.counters = torch.zeros(2, dtype=torch.long, device=self.dev)
        self.it_cur = ctypes.c_void_p(self.counters.data_ptr())
        self.it_next = ctypes.c_void_p(self.counters.data_ptr() + 8)
        self.wq = torch.empty_like(sq.w).requires_grad_(True)
        # Adam's bias corrections for every step of the loop, computed once (the same device
        # arithmetic the step would run per wave: same bits)
        self.bias_corr = torch.empty(iters, 2, dtype=torch.float32, device=self.dev)
        _native.check(self.lib.aimet_adaround_adam_bias_corrections(_ADAM[1], _ADAM[2], iters, _ptr(self.bias_corr),
                                                                    _stream_ptr(self.dev)))
        self.code = _act_code(act_func)
        self.bias = module.bias.detach().contiguous() if module.bias is not None else None
        self.pbias = _ptr(self.bias) if self.bias is not None else None
        self.alpha0 = self.alpha.detach().clone()
        self.loss0 = round_loss_out.clone() if round_loss_out is not None else None

    def adam_step(self, s, grad, nparts=1, part_kk=0):
        # dL/dalpha from dL/dWq (`grad`: nparts ordered slices of it part_kk floats apart, summed
        # here) + the Adam update; it also writes the next iteration's soft-quantized weight into
        # wq (it reads W and the new alpha anyway): no separate forward launch per iteration
        sq = self.sq
        _native.check(self.lib.aimet_adaround_backward_adam_parts(
            sq.pw, sq.pa, _ptr(grad), nparts, part_kk, _ptr(self.exp_avg), _ptr(self.exp_avg_sq), *sq.shape, sq.pd,
            sq.po, sq.bw, _ptr(self.rb_all), self.it_next, self.it_cur, *_ADAM, sq.pl, _ptr(self.wq),
            _ptr(self.bias_corr), s))

    def soft_weight(self):   # wq from the current alpha (before the first iteration)
        sq = self.sq
        _native.check(sq.fwd(sq.pw, sq.pa, _ptr(self.wq), *sq.shape, sq.pd, sq.po, sq.bw, 1, _stream_ptr(self.dev)))

    def restart(self):   # back to iteration 0
        with torch.no_grad():
            self.alpha.copy_(self.alpha0)
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            self.counters.zero_()
            if self.loss is not None:
                self.loss.copy_(self.loss0)
        self.soft_weight()

    def batch_like(self, cache, dtype=None):
        return torch.empty((self.nb,) + tuple(cache.shape[1:]), dtype=dtype or cache.dtype, device=self.dev)

    def batch_buffers(self):   # the gathered input rows, the layer output q and dL/dq
        q = self.batch_like(self.out_data, torch.float32)
        return self.batch_like(self.inp_data), q, torch.empty_like(q)

    def gather(self, s, inp, target=None):   # this iteration's cache rows; it_next moves here
        _native.check(self.lib.aimet_adaround_gather(
            _ptr(self.inp_data), _ptr(self.out_data), _ptr(inp), _ptr(target) if target is not None else None,
            _ptr(self.idx_all), self.it_cur, self.it_next, self.nb, inp[0].numel(), self.out_data[0].numel(), s))

    def recon_grad(self, s, q, g, with_bias):   # g = dL/dq, the target rows read in place
        p = self.plan
        _native.check(self.lib.aimet_adaround_recon_grad_indexed(
            _ptr(q), _ptr(self.out_data), _ptr(self.idx_all), self.it_cur, _ptr(g), self.nb, p.C_out, p.hw,
            self.pbias if with_bias else None, self.code, s))


def _workspace(st, query, *dims):
    n = ctypes.c_int64()
    _native.check(query(*dims, ctypes.byref(n)))
    return torch.empty(n.value, dtype=torch.float32, device=st.dev)


# The iteration up to dL/dWq as one pass (aimet_adaround_dw_step / _pw_step): the batch read in
# place from the caches, q and g never stored; it_next moves in the pass. parts: the weight-gradient
# slices in ws as adam_step's (grad, nparts, part_kk), which then folds them (one launch fewer, the
# same sum); None: the pass folds them itself, in a launch of its own.
def _one_pass_step(st, kernel, dims, ws, parts):
    grad = parts or (torch.empty_like(st.sq.w),)
    gw = None if parts else _ptr(grad[0])

    def step(s):
        _native.check(kernel(_ptr(st.inp_data), _ptr(st.out_data), _ptr(st.idx_all), st.it_cur, st.it_next,
                             _ptr(st.wq), st.pbias, gw, _ptr(ws), *dims, st.code, s))
        st.adam_step(s, *grad)
    return step


# Depthwise layers on the native kernels, no autograd: the one-pass step, or (_DW_FUSED off, its
# comparison) gather + forward + reconstruction gradient + weight gradient.
def _dw_step(st):
    lib, nb, (K, stride, pad, dil) = st.lib, st.nb, st.plan.dw
    (C, H, W), (OH, OW) = st.inp_data.shape[1:], st.out_data.shape[2:]
    dims = (nb, C, H, W, OH, OW, K, stride, pad, dil)
    ws = _workspace(st, lib.aimet_dwconv2d_grad_weight_workspace, nb, C, OH, OW, K)
    if _DW_FUSED:
        slices = ctypes.c_int64()
        if _DW_FOLD_ADAM:
            _native.check(lib.aimet_adaround_dw_step_slices(_ptr(st.out_data), nb, C, OH, OW, K, stride, dil,
                                                            ctypes.byref(slices)))
        return _one_pass_step(st, lib.aimet_adaround_dw_step, dims, ws,
                              (ws, slices.value, K * K) if slices.value else None)
    inp, q, g = st.batch_buffers()
    gw = torch.empty_like(st.sq.w)

    def step(s):
        st.gather(s, inp)
        _native.check(lib.aimet_dwconv2d_forward(_ptr(inp), _ptr(st.wq), st.pbias, _ptr(q), *dims, s))
        st.recon_grad(s, q, g, False)
        _native.check(lib.aimet_dwconv2d_grad_weight(_ptr(inp), _ptr(g), _ptr(gw), _ptr(ws), *dims, s))
        st.adam_step(s, gw)
    return step


# 1x1 layers / the unfolded stem with few input channels (plan_loop's _PW_FUSED rule): one pass.
def _pw_one_pass_step(st):
    dims = (st.nb, st.plan.cin, st.plan.C_out, st.plan.hw)
    ws, parts = _workspace(st, st.lib.aimet_adaround_pw_step_workspace, *dims), None
    if _DW_FOLD_ADAM:
        off, nsl = ctypes.c_int64(), ctypes.c_int64()
        _native.check(st.lib.aimet_adaround_pw_step_slices(*dims, ctypes.byref(off), ctypes.byref(nsl)))
        parts = (ws[off.value:], nsl.value, st.sq.w.numel())
    return _one_pass_step(st, st.lib.aimet_adaround_pw_step, dims, ws, parts)


# 1x1 layers of <= 14 x 14 positions as GEMMs over channel-major batches (aimet_adaround_gather_cm:
# x as [C_in][nb hw], so q = W x and dL/dW = g x^T are ONE GEMM each, no per-sample GEMMs, batch
# sum or transposes). MobileNet-v2: 0.117 -> 0.063 ms per iteration at 576 -> 96 x 14^2; slower at
# 28^2: 0.071 -> 0.09. (The same form on the f32 matrix cores in two kernels of our own, and the
# weight gradient as split-K GEMM slices, measured slower and are not in the library:
# tools/studies/pw_cm_mfma.hip, profiles/r04/pw_cm_*.jsonl.)
def _cm_step(st):
    lib, p, nb = st.lib, st.plan, st.nb
    x = torch.empty((p.cin, nb * p.hw), dtype=torch.float32, device=st.dev)
    q = torch.empty((p.C_out, nb * p.hw), dtype=torch.float32, device=st.dev)
    g = torch.empty_like(q)

    def step(s):
        _native.check(lib.aimet_adaround_gather_cm(_ptr(st.inp_data), _ptr(x), _ptr(st.idx_all), st.it_cur, st.it_next,
                                                   nb, p.cin, p.hw, s))
        torch.mm(st.wq.detach().view(p.C_out, -1), x, out=q)
        _native.check(lib.aimet_adaround_recon_grad_indexed_cm(_ptr(q), _ptr(st.out_data), _ptr(st.idx_all), st.it_cur,
                                                               _ptr(g), nb, p.C_out, p.hw, st.pbias, st.code, s))
        st.adam_step(s, torch.mm(g, x.t()))
    return step


# The other 1x1 layers (or unfolded stems) as one batched GEMM per direction (hipBLASLt, no
# NCHW<->NHWC transposes): q[n] = Wq @ x[n], dL/dWq = sum_n g[n] @ x[n]^T; the bias is added inside
# the reconstruction kernel.
def _gemm_step(st):
    p, nb = st.plan, st.nb
    inp, q, g = st.batch_buffers()
    x3, q3, g3 = inp.view(nb, p.cin, -1), q.view(nb, p.C_out, -1), g.view(nb, p.C_out, -1)

    def step(s):
        st.gather(s, inp)
        torch.matmul(st.wq.detach().view(p.C_out, -1), x3, out=q3)
        st.recon_grad(s, q, g, True)
        st.adam_step(s, torch.matmul(g3, x3.transpose(1, 2)).sum(0))
    return step


# `build` on the input cache unfolded once ([N, C_in k k, OH OW]): each iteration's batch of a
# small-C_in convolution is then a pointwise problem, gathered by rows like any other.
def _unfolded(build):
    def build_im2col(st):
        m = st.module
        st.inp_data = F.unfold(st.inp_data, m.kernel_size, m.dilation, m.padding, m.stride).contiguous()
        return build(st)
    return build_im2col


def _linear_step(st):
    inp, q, g = st.batch_buffers()

    def step(s):
        st.gather(s, inp)
        torch.mm(inp, st.wq.detach().t(), out=q)
        st.recon_grad(s, q, g, True)
        st.adam_step(s, torch.mm(g.t(), inp))
    return step


# Any layer through layer_forward and autograd (MIOpen convolutions): the reconstruction gradient
# from the fused kernel when it has a fused form (indexed), else from torch ops on a gathered target.
def _autograd_step(st):
    inp = st.batch_like(st.inp_data)
    if st.plan.indexed:
        g = st.batch_like(st.out_data, torch.float32)

        def step(s):
            st.gather(s, inp)
            q_out = layer_forward(st.module, inp, st.wq)
            st.recon_grad(s, q_out, g, False)
            (gw,) = torch.autograd.grad(q_out, st.wq, grad_outputs=g)
            st.adam_step(s, gw.contiguous())
        return step
    target, act = st.batch_like(st.out_data), st.act_func

    def step(s):
        st.gather(s, inp, target)
        q_out = layer_forward(st.module, inp, st.wq)
        qa, ta = (act(q_out), act(target)) if act is not None else (q_out, target)
        (gw,) = torch.autograd.grad(recon_loss(qa, ta), st.wq)
        st.adam_step(s, gw.contiguous())
    return step


_STEP_BUILDERS = {
    "autograd": _autograd_step, "linear": _linear_step, "dw": _dw_step,
    "pointwise": _gemm_step, "pointwise_cm": _cm_step, "pointwise_fused": _pw_one_pass_step,
    "im2col": _unfolded(_gemm_step), "im2col_cm": _unfolded(_cm_step), "im2col_fused": _unfolded(_pw_one_pass_step),
}


def _replay_chunks(iters, draw, replay, dev):
    """replay(count) over all iterations, a chunk at a time: the next chunk's batches are drawn on
    the host while the GPU replays this one."""
    for a in range(0, iters, _CHUNK):
        b = min(a + _CHUNK, iters)
        if b < iters:
            draw(b, min(b + _CHUNK, iters))
        replay(b - a)
    torch.cuda.current_stream(dev).synchronize()


def _run_captured(st, draw):
    """Builds the plan's step (its fallback form when the first cannot be captured), captures one
    and _GRAPH_ITERS iterations in HIP graphs and replays them; returns the form that ran."""
    dev, iters = st.dev, st.iters

    def capture(step, k=1):
        # warm-up on a side stream (library handles, allocator, autograd), then capture
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.enable_grad():
            st.soft_weight()
            for _ in range(min(2, iters)):
                step(_stream_ptr(dev))
        torch.cuda.current_stream(dev).wait_stream(side)
        st.restart()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.enable_grad():
            for _ in range(k):   # k consecutive iterations (the counters advance on the device)
                step(_stream_ptr(dev))
        return g

    form, step = st.plan.form, _STEP_BUILDERS[st.plan.form](st)
    try:
        graph = capture(step)
    except RuntimeError:
        if st.plan.fallback is None:
            raise
        form, step = st.plan.fallback, _STEP_BUILDERS[st.plan.fallback](st)
        graph = capture(step)
    k = min(_GRAPH_ITERS, _CHUNK)
    graph_k = None
    if k > 1 and iters >= k:
        # when k iterations cannot be captured (graph-pool memory, an autograd form) the
        # one-iteration graph runs them, the same results
        with contextlib.suppress(RuntimeError):
            graph_k = capture(step, k)
        st.restart()

    def replay(count):
        done = 0
        while graph_k is not None and done + k <= count:
            graph_k.replay()
            done += k
        for _ in range(done, count):
            graph.replay()
    _replay_chunks(iters, draw, replay, dev)
    return form


class AdaroundOptimizer:
    """v1/adaround/adaround_optimizer.py."""

    last_loop_form = None   # the form the last fused loop ran (LoopPlan.form, or its fallback)
    _exact_pow_logged = set()   # the beta ranges whose switch to the exact pow has been logged
    is_activation_caching_enabled = True

    # ---- the reference's caller surface (v1/adaround/adaround_optimizer.py:69-260) -------------
    @classmethod
    def adaround_module(cls, module: torch.nn.Module, quant_module, orig_model: torch.nn.Module,
                        quant_model: torch.nn.Module, act_func, cached_dataset, forward_fn,
                        opt_params: AdaroundHyperParameters, cached_quant_dataset=None):
        """adaround_optimizer.py:69-113: the reconstruction metrics before / after (debug log),
        the rounding optimisation of `quant_module` (an AdaroundWrapper), then hard rounding."""
        from aimet_amd.activation_sampler import ActivationSampler
        from aimet_amd.adaround_wrapper import AdaroundWrapper
        assert isinstance(quant_module, AdaroundWrapper), "%s is not adaround wrapper module." % quant_module
        sampler = ActivationSampler(module, quant_module, orig_model, quant_model, forward_fn)
        if cached_quant_dataset:
            inp_data, _ = sampler.sample_acts(cached_quant_dataset[0], collect_input=True, collect_output=False)
            _, out_data = sampler.sample_acts(cached_dataset[0], collect_input=False, collect_output=True)
        else:
            inp_data, out_data = sampler.sample_acts(cached_dataset[0])
        hard, soft = cls._compute_recons_metrics(quant_module, act_func, inp_data, out_data)
        _log.debug("Before opt, Recons. error metrics using soft rounding=%f and hard rounding=%f", soft, hard)
        cls._optimize_rounding(module, quant_module, orig_model, quant_model, act_func, cached_dataset, forward_fn,
                               opt_params, cached_quant_dataset)
        hard, soft = cls._compute_recons_metrics(quant_module, act_func, inp_data, out_data)
        _log.debug("After opt, Recons. error metrics using soft rounding=%f and hard rounding=%f", soft, hard)
        quant_module.use_soft_rounding = False

    @classmethod
    def _optimize_rounding(cls, module: torch.nn.Module, quant_module, orig_model: torch.nn.Module,
                           quant_model: torch.nn.Module, act_func, cached_dataset, forward_fn,
                           opt_params: AdaroundHyperParameters, cached_quant_dataset=None):
        """adaround_optimizer.py:115-221 over the fused loop (optimize_rounding): the cached
        dataset sharded by batch rank::world as the reference's Subset, every batch's layer input
        (QuantSim model) and output (original model) sampled into HBM, then num_iterations // world
        iterations of Adam (lr 1e-3 x world) on quant_module.alpha with batches of 32 drawn by
        torch.randperm from the global generator, alpha.grad all-reduced / world."""
        from aimet_amd.activation_sampler import ActivationSampler
        from aimet_amd.adaround_wrapper import AdaroundWrapper
        rank, world = _group_world(None)
        indices = range(rank, len(cached_dataset), world)
        shard = [cached_dataset[i] for i in indices]
        shard_q = [cached_quant_dataset[i] for i in indices] if cached_quant_dataset is not None else None
        assert isinstance(quant_module, AdaroundWrapper), "%s is not adaround wrapper module." % quant_module
        assert quant_module.use_soft_rounding, "optimization should use soft rounding only."
        assert quant_module.alpha is not None, "alpha parameter should be initialized."
        original = quant_module.get_original_module()
        device = original.weight.device
        sampler = ActivationSampler(module, quant_module, orig_model, quant_model, forward_fn)
        inp_data, out_data = sampler.sample_all_acts(shard, shard_q, device=device)
        cls.optimize_rounding(original, inp_data, out_data, quant_module._delta_vec.to(device),
                              quant_module._offset_vec.to(device), quant_module.bitwidth, quant_module._ch_axis,
                              opt_params, act_func, generator=None, alpha=quant_module.alpha, presharded=True)

    @classmethod
    def _compute_recons_metrics(cls, quant_module, act_func, inp_data: torch.Tensor,
                                out_data: torch.Tensor) -> Tuple[float, float]:
        """adaround_optimizer.py:223-255: (MSE with hard rounding, MSE with soft rounding)."""
        with torch.no_grad():
            quant_module.use_soft_rounding = False
            out_hard = cls._compute_output_with_adarounded_weights(quant_module, inp_data)
            quant_module.use_soft_rounding = True
            out_soft = cls._compute_output_with_adarounded_weights(quant_module, inp_data)
            if act_func is not None:
                out_data, out_soft, out_hard = act_func(out_data), act_func(out_soft), act_func(out_hard)
            return float(F.mse_loss(out_hard, out_data)), float(F.mse_loss(out_soft, out_data))

    @staticmethod
    def _compute_output_with_adarounded_weights(quant_module, inp_data: torch.Tensor):
        """adaround_optimizer.py:257-286."""
        module = quant_module.get_original_module()
        quant_module.to(inp_data.device)
        if not isinstance(module, (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.Linear)):
            raise ValueError("AdaRound is not supported for the module: ", module)
        weight = quant_module.apply_adaround(quant_module.weight)
        if isinstance(module, torch.nn.Conv2d):
            return F.conv2d(inp_data, weight, bias=module.bias, stride=module.stride, dilation=module.dilation,
                            padding=module.padding, groups=module.groups)
        if isinstance(module, torch.nn.ConvTranspose2d):
            return F.conv_transpose2d(inp_data, weight, bias=module.bias, stride=module.stride,
                                      padding=module.padding, output_padding=module.output_padding,
                                      groups=module.groups, dilation=module.dilation)
        return F.linear(inp_data, weight, bias=module.bias)

    @staticmethod
    def enable_caching_acts_data() -> bool:
        """adaround_optimizer.py:340-349: the samples are always cached here (in HBM)."""
        return AdaroundOptimizer.is_activation_caching_enabled

    @staticmethod
    def optimize_rounding(module: torch.nn.Module, inp_data: torch.Tensor, out_data: torch.Tensor,
                          delta: torch.Tensor, offset: torch.Tensor, bitwidth: int, ch_axis: int = 0,
                          opt_params: AdaroundHyperParameters = AdaroundHyperParameters(),
                          act_func: Optional[Callable] = None, generator: Optional[torch.Generator] = None,
                          round_loss_out: Optional[torch.Tensor] = None, use_graph: bool = True,
                          group=None, alpha: Optional[torch.Tensor] = None,
                          presharded: bool = False) -> torch.nn.Parameter:
        """Optimises alpha for `module` on the cached activations (inp_data / out_data: [N, ...] on
        the device); returns alpha. delta / offset: the weight quantizer's (per-channel) encoding.

        use_graph: the iteration is captured once in a HIP graph and replayed num_iterations times
        (the batch indices of every iteration drawn up front from `generator` in the same order as
        the eager loop, the annealed beta read from device memory by the backward kernel, Adam in
        its capturable form); the loop is launch-bound for MobileNet-sized layers.

        group: the process group to run data parallel over (default: the default group when
        torch.distributed is initialised); see the module docstring.

        alpha: the starting alpha (an AdaroundWrapper's parameter, adaround_wrapper.py:211-224);
        it is updated in place and returned. Default: init_alpha of the weight.
        presharded: inp_data / out_data already hold only this rank's samples (adaround_module
        shards the cached dataset by batch, as the reference does)"""
        rank, world = _group_world(group)
        if world > 1 and not presharded:
            # adaround_optimizer.py:147-150: this rank's shard of the cached samples
            shard = torch.arange(rank, inp_data.shape[0], world, device=inp_data.device)
            inp_data, out_data = inp_data.index_select(0, shard), out_data.index_select(0, shard)
        args = (module, inp_data, out_data, delta, offset, bitwidth, ch_axis, opt_params, act_func, generator,
                round_loss_out, world, group, alpha)
        # the loop's kernels read the annealed beta from device memory, where the pow's form is
        # already chosen: a beta_range that leaves the fast pow's proven exponents runs this
        # layer's whole loop (eager, graph or distributed) with the exact pow; one below 1 raises
        if opt_params.reg_param != 0 and exact_pow_needed(opt_params.beta_range) and not get_exact_pow():
            if tuple(opt_params.beta_range) not in AdaroundOptimizer._exact_pow_logged:
                AdaroundOptimizer._exact_pow_logged.add(tuple(opt_params.beta_range))
                _log.warning("AdaRound: beta_range %r leaves the exponents the fast rounding-loss pow is proven on; "
                             "running with the exact pow", tuple(opt_params.beta_range))
            set_exact_pow(True)
            try:
                return AdaroundOptimizer._optimize_rounding_loop(use_graph, args)
            finally:
                set_exact_pow(False)
        return AdaroundOptimizer._optimize_rounding_loop(use_graph, args)

    @staticmethod
    def _optimize_rounding_loop(use_graph, args):
        (module, opt_params, generator, round_loss_out, world) = (args[0], args[7], args[9], args[10], args[11])
        if opt_params.num_iterations // world == 0:
            # fewer iterations than ranks (or none): the loop runs zero times and alpha keeps its
            # initial value, as the reference's range() loop does -- no batch draw, no capture
            use_graph = False
        with conv_backend(module):
            if use_graph:
                rng = generator.get_state() if generator is not None else torch.get_rng_state()
                loss0 = round_loss_out.clone() if round_loss_out is not None else None
                try:
                    return AdaroundOptimizer._optimize_graphed(*args)
                except RuntimeError as e:   # a layer whose iteration cannot be captured: same loop, eager
                    warnings.warn("AdaRound: HIP-graph capture failed for %s (%s); running the loop eagerly"
                                  % (type(module).__name__, e))
                    torch.cuda.synchronize()
                    if generator is not None:
                        generator.set_state(rng)
                    else:
                        torch.set_rng_state(rng)
                    if round_loss_out is not None:
                        round_loss_out.copy_(loss0)
            return AdaroundOptimizer._optimize_eager(*args)

    @staticmethod
    def _optimize_eager(module, inp_data, out_data, delta, offset, bitwidth, ch_axis, opt_params, act_func,
                        generator, round_loss_out, world=1, group=None, alpha_init=None):
        w, dev, d, o, alpha = _loop_setup(module, delta, offset, ch_axis, alpha_init)
        optimizer = _torch_adam(alpha, world)
        sq = _BoundSoftQuant(w, alpha, d, o, bitwidth, ch_axis, round_loss_out)
        n = inp_data.shape[0]
        warm = opt_params.num_iterations * opt_params.warm_start
        for it in range(opt_params.num_iterations // world):
            idx = torch.randperm(n, generator=generator)[:BATCH_SIZE].to(dev, non_blocking=True)
            inp = inp_data.index_select(0, idx)
            target = out_data.index_select(0, idx)
            optimizer.zero_grad()
            if it < warm:
                sq.reg, sq.beta = 0.0, 0.0
            else:
                sq.reg = opt_params.reg_param
                sq.beta = compute_beta(opt_params.num_iterations, it, opt_params.beta_range, opt_params.warm_start)
            wq = _SoftQuantFn.apply(alpha, sq)
            q_out = layer_forward(module, inp, wq)
            # fused reconstruction-loss gradient; + the rounding-loss gradient, fused in the soft-quant kernel
            recon_loss_backward(q_out, target, act_func)
            if world > 1:
                _reduce_grad(alpha.grad, world, group)
            optimizer.step()
        return _finish_alpha(alpha, alpha_init)

    @staticmethod
    def _drawer(generator, n, iters, dev):
        """The eager loop's batch draws, in its order: idx_all [iters, nb] int64 on the device and
        draw(a, b), which fills rows [a, b) from the host generator through a pinned buffer
        (stream-ordered copy; the host buffers stay alive in `staged` until the caller
        synchronises), so chunk k + 1 is drawn while the GPU replays chunk k."""
        nb = min(n, BATCH_SIZE)
        idx_all = torch.empty((max(iters, 1), nb), dtype=torch.long, device=dev)
        staged = []

        def draw(a, b):
            h = torch.stack([torch.randperm(n, generator=generator)[:BATCH_SIZE] for _ in range(a, b)]).pin_memory()
            idx_all[a:b].copy_(h, non_blocking=True)
            staged.append(h)
        draw(0, min(_CHUNK, iters))
        return idx_all, draw

    @staticmethod
    def _reg_beta_all(opt_params, iters, dev):
        """{reg, beta, beta - 1} of every iteration, formed in double as the reference's python /
        ATen pow_backward do, then stored as float32 (the kernel's arithmetic type)."""
        warm = opt_params.num_iterations * opt_params.warm_start
        return torch.tensor([(0.0, 0.0, 0.0) if it < warm else
                             (lambda b: (opt_params.reg_param, b, b - 1.0))(
                                 compute_beta(opt_params.num_iterations, it, opt_params.beta_range,
                                              opt_params.warm_start))
                             for it in range(max(iters, 1))], dtype=torch.float64).to(torch.float32).to(dev)

    @staticmethod
    def _optimize_fused_graph(module, inp_data, out_data, delta, offset, bitwidth, ch_axis, opt_params, act_func,
                              generator, round_loss_out, alpha_init=None):
        """Single-process HIP-graph loop with the iteration's bookkeeping fused into two kernels:
        the batch draw (aimet_adaround_gather, or inside a one-pass step) and the Adam step
        (_LoopState.adam_step). The iteration counter and Adam moments live in device memory."""
        inp_data, out_data = inp_data.contiguous(), out_data.contiguous()
        # an im2col form reads its own unfolded copy of the input cache (a fresh allocation)
        aligned = out_data.data_ptr() % 16 == 0 and (
            inp_data.data_ptr() % 16 == 0 or _im2col_ok(module, inp_data.shape, inp_data.element_size()))
        plan = plan_loop(module, inp_data.shape, inp_data.dtype, out_data.shape, out_data.dtype, act_func, aligned)
        w, dev, d, o, alpha = _loop_setup(module, delta, offset, ch_axis, alpha_init)
        sq = _BoundSoftQuant(w, alpha, d, o, bitwidth, ch_axis, round_loss_out)
        iters = opt_params.num_iterations
        idx_all, draw = AdaroundOptimizer._drawer(generator, inp_data.shape[0], iters, dev)
        st = _LoopState(plan, module, inp_data, out_data, sq, iters, idx_all,
                        AdaroundOptimizer._reg_beta_all(opt_params, iters, dev), act_func, round_loss_out)
        AdaroundOptimizer.last_loop_form = _run_captured(st, draw)
        return _finish_alpha(alpha, alpha_init)

    @staticmethod
    def _optimize_graphed(module, inp_data, out_data, delta, offset, bitwidth, ch_axis, opt_params, act_func,
                          generator, round_loss_out, world=1, group=None, alpha_init=None, fused_step=True):
        if world == 1 and fused_step:
            return AdaroundOptimizer._optimize_fused_graph(module, inp_data, out_data, delta, offset, bitwidth,
                                                           ch_axis, opt_params, act_func, generator, round_loss_out,
                                                           alpha_init)
        w, dev, d, o, alpha = _loop_setup(module, delta, offset, ch_axis, alpha_init)
        optimizer = _torch_adam(alpha, world, capturable=True)
        sq = _BoundSoftQuant(w, alpha, d, o, bitwidth, ch_axis, round_loss_out)
        iters = opt_params.num_iterations // world
        idx_all, draw = AdaroundOptimizer._drawer(generator, inp_data.shape[0], iters, dev)
        rb_all = AdaroundOptimizer._reg_beta_all(opt_params, iters, dev)
        it_buf = torch.zeros(1, dtype=torch.long, device=dev)
        alpha.grad = torch.zeros_like(alpha)

        def grad_step():
            idx = idx_all.index_select(0, it_buf).view(-1)
            inp = inp_data.index_select(0, idx)
            target = out_data.index_select(0, idx)
            sq.reg_beta = rb_all.index_select(0, it_buf).view(-1)
            optimizer.zero_grad(set_to_none=False)
            wq = _SoftQuantFn.apply(alpha, sq)
            q_out = layer_forward(module, inp, wq)
            recon_loss_backward(q_out, target, act_func)

        def update_step():
            if world > 1:
                alpha.grad.div_(world)
            optimizer.step()
            it_buf.add_(1)

        def step():
            grad_step()
            if world > 1:
                _reduce_grad(alpha.grad, world, group, divide=False)   # the SUM; / world in update_step
            update_step()

        # warm-up on a side stream (library handles, allocator, autograd), then back to iteration 0
        alpha0 = alpha.detach().clone()
        loss0 = round_loss_out.clone() if round_loss_out is not None else None
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(min(3, iters)):
                step()
        torch.cuda.current_stream(dev).wait_stream(side)
        with torch.no_grad():
            alpha.copy_(alpha0)
            it_buf.zero_()
            for st in optimizer.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
            if round_loss_out is not None:
                round_loss_out.copy_(loss0)
        if world == 1:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            replay_one = graph.replay
        else:
            # the collective between two graphs (any backend; gloo stages through the host)
            g_grad, g_upd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_grad):
                grad_step()
            with torch.cuda.graph(g_upd):
                update_step()

            def replay_one():
                g_grad.replay()
                _reduce_grad(alpha.grad, world, group, divide=False)
                g_upd.replay()

        def replay(count):
            for _ in range(count):
                replay_one()
        _replay_chunks(iters, draw, replay, dev)
        sq.reg_beta = None
        return _finish_alpha(alpha, alpha_init)

    @staticmethod
    def hard_rounded_weight(module: torch.nn.Module, alpha: torch.Tensor, delta, offset, bitwidth: int,
                            ch_axis: int = 0) -> torch.Tensor:
        """The adarounded weight: hard rounding h = (alpha >= 0) (adaround_wrapper.py:124-149 with
        use_soft_rounding False)."""
        w = module.weight.detach()
        d = torch.as_tensor(delta, dtype=torch.float32, device=w.device).reshape(-1)
        o = torch.as_tensor(offset, dtype=torch.float32, device=w.device).reshape(-1)
        with torch.no_grad():
            return AdaroundFunction.apply(w, alpha.detach(), d, o, bitwidth, ch_axis, False)
