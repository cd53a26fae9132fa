"""BatchNorm re-estimation (aimet_torch/bn_reestimation.py) on the MI355X core: after range-learning
QAT with the BatchNorms unfolded, their drifting running statistics are replaced by the averages of
the batch statistics over clean batches, before ``fold_all_batch_norms_to_scale``. Names and
semantics follow the reference: everything runs in eval mode except the BatchNorms, under
``no_grad``; ``running_mean`` / ``running_var`` become the mean over ``min(len(dataloader),
num_batches)`` batches of the batch mean and the unbiased batch variance; the returned handle undoes
the call.

What differs is where the arithmetic runs. The reference runs every BatchNorm in training mode at
momentum 1 and, per BatchNorm and batch, adds the two running buffers into float32 sums (a library
BN kernel, a momentum update and two adds), then divides and copies per BatchNorm. Here the forward
of every BatchNorm is replaced, on the instance and for the duration of the call, by one
``aimet_bnre_forward`` (aimet_amd/csrc/bn_reest.hip) on the current stream: it normalises with the
batch statistics and adds them, in double, into that BatchNorm's accumulators; after the last batch
one ``aimet_bnre_finish`` launch writes the running buffers of all BatchNorms. Nothing is read back
and the host never waits for the device.

A BatchNorm call takes that fused route when its input is a float32 HIP tensor, dense in NC...
(contiguous) or channels-last layout, outside an autocast region. Any other call (a 16-bit or strided
input, autocast, a CPU tensor in a model that is otherwise on the device) takes the reference's own
route inside the same call: torch's training-mode forward at momentum 1 and float32 sums of the
running buffers. ``handle.fused`` and ``handle.fallback`` count the BatchNorms on each route.

There is no CPU compute path for a whole model: as ``bias_correction.correct_bias``, a CPU-resident
model is re-estimated through a copy in HBM and its buffers are copied back; with no HIP device the
call raises. ``DataParallel`` is unwrapped to ``.module``. ``SyncBatchNorm`` and runs over several
ranks are out of scope (NotImplementedError for the former).
"""
import copy
import ctypes
import itertools
from typing import Any, Callable, Iterable, List, Optional

import torch
from torch import nn
from torch.nn.modules.batchnorm import _BatchNorm

from aimet_amd import _native
from aimet_amd._native import BnreFinishJobC

DEFAULT_NUM_BATCHES = 100


class Handle:
    """aimet_common/utils.py Handle: remove() runs the clean-up once; usable as a context manager."""

    def __init__(self, cleanup_fn: Optional[Callable[[], None]] = None):
        self._cleanup_fn = cleanup_fn

    def remove(self):
        if self._cleanup_fn is not None:
            fn, self._cleanup_fn = self._cleanup_fn, None
            fn()

    def __enter__(self):
        return self

    def __exit__(self, *_):
        self.remove()


def launch_count(reset: bool = False) -> int:
    """Kernel launches the aimet_bnre_* entry points have issued in this process."""
    n = ctypes.c_int64()
    _native.call("aimet_bnre_launch_count", ctypes.byref(n), 1 if reset else 0)
    return n.value


def _get_active_bn_modules(model: nn.Module) -> Iterable[_BatchNorm]:
    """BatchNorms with running statistics, those inside quantization wrappers included."""
    for module in model.modules():
        if isinstance(module, _BatchNorm) and module.running_mean is not None and module.running_var is not None:
            yield module


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _layout(x: torch.Tensor):
    """(outer, inner) of a dense [N, C, ...] tensor in one of the kernel's two layouts, or None."""
    if x.dim() < 2:
        return None
    if x.is_contiguous():
        inner = 1
        for d in x.shape[2:]:
            inner *= int(d)
        return int(x.shape[0]), inner
    last = {4: torch.channels_last, 5: torch.channels_last_3d}.get(x.dim())
    if last is not None and x.is_contiguous(memory_format=last):
        return x.numel() // int(x.shape[1]), 1
    return None


class _BnState:
    """One BatchNorm for the duration of a call: what to restore, and its sums."""

    def __init__(self, bn: _BatchNorm, acc: Optional[torch.Tensor], total: Optional[torch.Tensor]):
        self.bn = bn
        self.saved = (bn.running_mean.clone(), bn.running_var.clone(),
                      None if bn.num_batches_tracked is None else bn.num_batches_tracked.clone())
        self.momentum, self.training = bn.momentum, bn.training
        self.had_forward = "forward" in bn.__dict__
        self.old_forward = bn.__dict__.get("forward")
        self.acc = acc                  # [2][C] double: this batch's mean and unbiased variance (fused route)
        self.total = total              # [2][C] double: their sums over the batches
        self.sum32 = None               # [2][C] float32 sums of the running buffers (reference route)
        self.fused_now = self.torch_now = False
        self.fused_batches = self.torch_batches = self.calls = 0

    def eligible(self, x) -> bool:
        bn = self.bn
        if self.acc is None or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
            return False
        if torch.is_autocast_enabled("cuda") or x.device != self.acc.device:
            return False
        for p in (bn.weight, bn.bias):
            if p is not None and (p.dtype != torch.float32 or p.device != x.device or not p.is_contiguous()):
                return False
        lay = _layout(x)
        if lay is None or int(x.shape[1]) != bn.num_features:
            return False
        n = lay[0] * lay[1]
        return 2 <= n < 2 ** 31 and x.numel() < 2 ** 46

    def forward(self, x):
        self.calls += 1
        if not self.eligible(x):
            self.torch_now = True
            return type(self.bn).forward(self.bn, x)
        if self.fused_now:              # a second call in one batch: as for the running buffers, the last one counts
            self.acc.zero_()
        self.fused_now = True
        bn = self.bn
        outer, inner = _layout(x)
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _native.call("aimet_bnre_forward", _ptr(x), outer, bn.num_features, inner,
                         _ptr(None if bn.weight is None else bn.weight.detach()),
                         _ptr(None if bn.bias is None else bn.bias.detach()), float(bn.eps), _ptr(y),
                         _ptr(self.acc[0]), _ptr(self.acc[1]),
                         ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
        return y

    def end_batch(self):
        if self.torch_now:              # the reference's two adds; a torch call in the batch overrides a fused one
            if self.fused_now:
                self.acc.zero_()
            if self.sum32 is None:
                self.sum32 = torch.zeros((2,) + tuple(self.bn.running_mean.shape), dtype=self.bn.running_mean.dtype,
                                         device=self.bn.running_mean.device)
            self.sum32[0] += self.bn.running_mean
            self.sum32[1] += self.bn.running_var
            self.torch_batches += 1
        elif self.fused_now:
            self.fused_batches += 1
        self.fused_now = self.torch_now = False

    def restore_flags(self):
        bn = self.bn
        bn.momentum, bn.training = self.momentum, self.training
        if self.had_forward:
            bn.__dict__["forward"] = self.old_forward
        else:
            bn.__dict__.pop("forward", None)

    def restore_stats(self):
        bn = self.bn
        with torch.no_grad():
            bn.running_mean.copy_(self.saved[0])
            bn.running_var.copy_(self.saved[1])
            if self.saved[2] is not None:
                bn.num_batches_tracked.copy_(self.saved[2])


def _to_device_of(model: nn.Module, data):
    device = next((p.device for p in model.parameters()), None)
    if device is not None and isinstance(data, torch.Tensor) and data.device != device:
        return data.to(device)
    return data


def _default_forward(model: nn.Module, data):
    return model(_to_device_of(model, data))


def reestimate_bn_stats(model: nn.Module, dataloader, num_batches: int = DEFAULT_NUM_BATCHES,
                        forward_fn: Callable[[nn.Module, Any], Any] = None) -> Handle:
    """Re-estimates the running mean and variance of every BatchNorm of `model` (a plain model or
    ``sim.model``) over the first ``min(len(dataloader), num_batches)`` batches.

    :param dataloader: yields what forward_fn takes; needs ``len()``
    :param forward_fn: ``forward_fn(model, batch)`` runs one forward; default ``model(batch)`` with a
           tensor batch moved to the model's device
    :returns: a Handle whose remove() restores running_mean, running_var and num_batches_tracked;
              ``handle.fused`` / ``handle.fallback`` are the numbers of BatchNorms that ran on the fused
              kernels / on torch's BatchNorm (module docstring)

    A CPU-resident model is re-estimated through a copy in HBM (forward_fn then gets the copy) and its
    buffers are copied back; without a HIP device the call raises RuntimeError."""
    if isinstance(model, nn.DataParallel):
        return reestimate_bn_stats(model.module, dataloader, num_batches, forward_fn)
    forward_fn = forward_fn or _default_forward
    bns = list(_get_active_bn_modules(model))
    if any(isinstance(bn, nn.SyncBatchNorm) for bn in bns):
        raise NotImplementedError("aimet_amd: reestimate_bn_stats does not cover SyncBatchNorm (multi-rank runs)")
    _native.load()
    if not torch.cuda.is_available():
        raise RuntimeError("aimet_amd: BatchNorm re-estimation needs a HIP device; the MI355X core has no CPU path")
    if bns and not any(bn.running_mean.is_cuda for bn in bns):
        return _reestimate_cpu_resident(model, bns, dataloader, num_batches, forward_fn)

    # per device one buffer of this batch's statistics and one of their sums, a [2][C] slice per BatchNorm
    sizes = {}
    for bn in bns:
        if bn.running_mean.is_cuda:
            sizes[bn.running_mean.device] = sizes.get(bn.running_mean.device, 0) + 2 * bn.num_features
    batch_sums = {d: torch.zeros(n, dtype=torch.float64, device=d) for d, n in sizes.items()}
    totals = {d: torch.zeros(n, dtype=torch.float64, device=d) for d, n in sizes.items()}
    states: List[_BnState] = []
    at = dict.fromkeys(sizes, 0)
    for bn in bns:
        d, n = bn.running_mean.device, 2 * bn.num_features
        if d in sizes:
            lo, at[d] = at[d], at[d] + n
            states.append(_BnState(bn, batch_sums[d][lo:lo + n].view(2, -1), totals[d][lo:lo + n].view(2, -1)))
        else:
            states.append(_BnState(bn, None, None))
    modes = [(m, m.training) for m in model.modules()]
    num_batches = min(len(dataloader), num_batches)

    def restore_stats():
        for st in states:
            st.restore_stats()

    try:
        model.eval()
        for st in states:
            bn = st.bn
            bn.training, bn.momentum = True, 1.0
            bn.reset_running_stats()
            bn.__dict__["forward"] = st.forward
        with torch.no_grad():
            for data in itertools.islice(dataloader, num_batches):
                forward_fn(model, data)
                for st in states:
                    st.end_batch()
                for d in sizes:
                    totals[d] += batch_sums[d]
                    batch_sums[d].zero_()
            _finish(states, num_batches)
    except BaseException:
        restore_stats()
        raise
    finally:
        for st in states:
            st.restore_flags()
        for m, was in modes:
            m.training = was
    handle = Handle(restore_stats)
    handle.fallback = sum(1 for st in states if st.torch_batches)
    handle.fused = sum(1 for st in states if st.fused_batches and not st.torch_batches)
    return handle


def _finish(states: List[_BnState], num_batches: int):
    """The running buffers from the sums: one aimet_bnre_finish launch for the BatchNorms that only
    took the fused route, the reference's float32 divide for those that only took torch's."""
    if num_batches <= 0:
        return
    by_device = {}
    for st in states:
        bn = st.bn
        if st.torch_batches and st.fused_batches:
            mixed = (st.total.to(st.sum32.device) + st.sum32.double()) / num_batches
            bn.running_mean.copy_(mixed[0])
            bn.running_var.copy_(mixed[1])
        elif st.torch_batches:
            bn.running_mean.copy_(st.sum32[0] / num_batches)
            bn.running_var.copy_(st.sum32[1] / num_batches)
        elif st.fused_batches:
            by_device.setdefault(bn.running_mean.device, []).append(st)
        # never called: the reset statistics (zeros and ones), which is what the reference's sums give
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.fill_(st.calls)
    for device, group in by_device.items():
        table = (BnreFinishJobC * len(group))()
        keep = []
        for slot, st in zip(table, group):
            bn = st.bn
            rm, rv = bn.running_mean, bn.running_var
            direct = rm.dtype == torch.float32 and rv.dtype == torch.float32 and rm.is_contiguous() and \
                rv.is_contiguous()
            out = (rm, rv) if direct else (torch.empty(bn.num_features, dtype=torch.float32, device=device),
                                           torch.empty(bn.num_features, dtype=torch.float32, device=device))
            keep.append((st, out, direct))
            slot.sum_mean, slot.sum_var = st.total[0].data_ptr(), st.total[1].data_ptr()
            slot.running_mean, slot.running_var = out[0].data_ptr(), out[1].data_ptr()
            slot.C, slot.count = bn.num_features, float(num_batches)
        with torch.cuda.device(device):
            _native.call("aimet_bnre_finish", table, len(group),
                         ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        for st, out, direct in keep:
            if not direct:
                st.bn.running_mean.copy_(out[0])
                st.bn.running_var.copy_(out[1])


def _reestimate_cpu_resident(model, bns, dataloader, num_batches, forward_fn) -> Handle:
    """There is no CPU compute path: the statistics are re-estimated on a copy of the model in HBM
    and copied back."""
    device = torch.device("cuda", torch.cuda.current_device())
    twin = copy.deepcopy(model).to(device)
    saved = [(bn, bn.running_mean.clone(), bn.running_var.clone(),
              None if bn.num_batches_tracked is None else bn.num_batches_tracked.clone()) for bn in bns]
    inner = reestimate_bn_stats(twin, dataloader, num_batches, forward_fn)
    with torch.no_grad():
        for bn, theirs in zip(bns, _get_active_bn_modules(twin)):
            bn.running_mean.copy_(theirs.running_mean)
            bn.running_var.copy_(theirs.running_var)
            if bn.num_batches_tracked is not None:
                bn.num_batches_tracked.copy_(theirs.num_batches_tracked)

    def restore():
        with torch.no_grad():
            for bn, mean, var, tracked in saved:
                bn.running_mean.copy_(mean)
                bn.running_var.copy_(var)
                if tracked is not None:
                    bn.num_batches_tracked.copy_(tracked)
    handle = Handle(restore)
    handle.fused, handle.fallback = inner.fused, inner.fallback
    return handle
