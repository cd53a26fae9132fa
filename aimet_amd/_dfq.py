"""Shared plumbing of the data-free quantization transforms (batch_norm_fold.py,
cross_layer_equalization.py): the launches of aimet_amd/csrc/dfq.hip on module parameters, and the
graph search on a torch.fx trace. The search is pure Python and needs no device; the transforms have
no CPU compute path (a CPU-resident parameter is staged through HBM and copied back)."""
import ctypes
from typing import Dict, List, Optional

import torch
from torch import nn

from aimet_amd import _native
from aimet_amd._native import BnreFoldScaleJobC, DfqBnFoldJobC, DfqWeightC

_TRANSPOSED = (nn.ConvTranspose1d, nn.ConvTranspose2d, nn.ConvTranspose3d)


def require_fp32(tensors, what: str):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise TypeError("aimet_amd: %s works on float32 parameters (got %s); there is no 16-bit path" %
                            (what, t.dtype))


class Stage:
    """Device tensors for the parameters of one call. A HIP-resident contiguous tensor is used in
    place; anything else is copied to HBM and copied back by finish(). Nothing is computed on the
    host."""

    def __init__(self, tensors):
        _native.load()
        dev = next((t.device for t in tensors if t is not None and t.is_cuda), None)
        if dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError("aimet_amd: the parameters are CPU tensors and no HIP device is visible; the "
                                   "MI355X core has no CPU path")
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self._staged = {}

    def dev(self, t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        if t is None:
            return None
        t = t.detach()
        if t.device == self.device and t.is_contiguous():
            return t
        key = (t.data_ptr(), t.device, tuple(t.shape), tuple(t.stride()))
        if key not in self._staged:
            self._staged[key] = (t, t.to(self.device).contiguous())
        return self._staged[key][1]

    def new(self, n: int, dtype=torch.float32) -> torch.Tensor:
        return torch.zeros(n, dtype=dtype, device=self.device)

    @property
    def stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def finish(self):
        for host, dev in self._staged.values():
            host.copy_(dev)
        self._staged = {}


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def weight_desc(module: nn.Module, w_dev: torch.Tensor) -> DfqWeightC:
    """aimet_dfq_weight of a Linear / ConvNd / ConvTransposeNd weight in module layout. A transposed
    conv with groups == 1 keeps its output channels on axis 1 (the reference permutes a copy); a
    grouped one is read as [axis 0][axis 1][k], as the reference reads it."""
    shape = w_dev.shape
    k = 1
    for d in shape[2:]:
        k *= int(d)
    if isinstance(module, _TRANSPOSED) and module.groups == 1:
        cout, cin = int(shape[1]), int(shape[0])
        return DfqWeightC(w_dev.data_ptr(), cout, cin, k, k, cout * k)
    cout, cin = int(shape[0]), int(shape[1])
    return DfqWeightC(w_dev.data_ptr(), cout, cin, k, cin * k, k)


def launch_count(reset: bool = False) -> int:
    """Kernel launches the DFQ entry points have issued in this process."""
    n = ctypes.c_int64()
    _native.call("aimet_dfq_launch_count", ctypes.byref(n), 1 if reset else 0)
    return n.value


def bn_fold_launch(stage: Stage, jobs: List[dict]):
    """One aimet_dfq_bn_fold launch. Each job: dict(module, weight, bias, bn, forward) with device
    tensors; raises if some sqrt(var + eps) is zero (that channel is left untouched)."""
    if not jobs:
        return
    table = (DfqBnFoldJobC * len(jobs))()
    keep = [_fill_bn_fold_job(stage, slot, j) for slot, j in zip(table, jobs)]
    _run_bn_fold("aimet_dfq_bn_fold", stage, table, jobs)
    del keep


def bn_fold_scale_launch(stage: Stage, jobs: List[dict]):
    """One aimet_bnre_fold_scale launch: backward folds as bn_fold_launch takes them, each with
    enc_min / enc_max (device float32 vectors of cout elements, updated in place)."""
    if not jobs:
        return
    table = (BnreFoldScaleJobC * len(jobs))()
    keep = []
    for slot, j in zip(table, jobs):
        keep.append(_fill_bn_fold_job(stage, slot.fold, j))
        slot.enc_min, slot.enc_max = j["enc_min"].data_ptr(), j["enc_max"].data_ptr()
    _run_bn_fold("aimet_bnre_fold_scale", stage, table, jobs)
    del keep


def _fill_bn_fold_job(stage: Stage, slot, j: dict):
    bn = j["bn"]
    vecs = [stage.dev(bn.weight), stage.dev(bn.bias), stage.dev(bn.running_mean), stage.dev(bn.running_var)]
    slot.w = weight_desc(j["module"], j["weight"])
    slot.bias = j["bias"].data_ptr()
    slot.gamma, slot.beta, slot.mean, slot.var = (v.data_ptr() for v in vecs)
    slot.eps = float(bn.eps)
    slot.forward = 1 if j["forward"] else 0
    return vecs   # alive until the launch


def _run_bn_fold(entry: str, stage: Stage, table, jobs: List[dict]):
    status = stage.new(len(jobs), torch.int32)
    with torch.cuda.device(stage.device):
        _native.call(entry, table, len(jobs), ptr(status), ctypes.c_void_p(stage.stream))
    bad = status.cpu().nonzero().flatten().tolist()
    if bad:
        raise ValueError("batch norm fold: sqrt(running_var + eps) is zero in %s" %
                         ", ".join(repr(jobs[i]["bn"]) for i in bad))


# ---------------------------------------------------------------------------------------------------
# graph search on a torch.fx trace
# ---------------------------------------------------------------------------------------------------
class TracedGraph:
    """The call_module nodes of torch.fx.symbolic_trace(model), with the modules they call."""

    def __init__(self, model: nn.Module, is_leaf=None):
        """is_leaf: modules m with is_leaf(m) are call_module nodes and not traced into (besides the
        torch.nn modules fx always keeps whole); default: fx's own rule."""
        import torch.fx

        class Tracer(torch.fx.Tracer):
            def is_leaf_module(self, m, module_qualified_name):
                return (is_leaf is not None and is_leaf(m)) or super().is_leaf_module(m, module_qualified_name)
        try:
            graph = Tracer().trace(model)
        except Exception as e:  # fx raises several kinds of error for control flow on tensors
            raise RuntimeError(
                "aimet_amd: torch.fx cannot trace %s (%s: %s), so batch norms and cross-layer-scaling sets cannot "
                "be found automatically. Give them explicitly: fold_given_batch_norms(model, layer_pairs) and "
                "CrossLayerScaling.scale_cls_sets(cls_sets) / HighBiasFold.bias_fold(...) need no graph."
                % (type(model).__name__, type(e).__name__, e)) from e
        self.nodes = list(graph.nodes)
        self.module_of: Dict[object, nn.Module] = {}
        self.calls: Dict[nn.Module, int] = {}
        for n in self.nodes:
            if n.op == "call_module":
                m = model.get_submodule(n.target)
                self.module_of[n] = m
                self.calls[m] = self.calls.get(m, 0) + 1

    def module(self, node) -> Optional[nn.Module]:
        return self.module_of.get(node)

    def node_of(self, module: nn.Module):
        for n, m in self.module_of.items():
            if m is module:
                return n
        return None

    def sole_user(self, node, skip_identity: bool = False):
        """The only user of the node's output, or None at a fan-out or a graph output. With
        skip_identity, nn.Identity modules (folded batch norms) are looked through."""
        while True:
            users = list(node.users)
            if len(users) != 1:
                return None
            nxt = users[0]
            if skip_identity and isinstance(self.module(nxt), nn.Identity):
                node = nxt
                continue
            return nxt


def replace_modules(model: nn.Module, predicate, make):
    """Replace every submodule m with predicate(m) by make(m), in its parent."""
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if predicate(child):
                setattr(parent, name, make(child))
