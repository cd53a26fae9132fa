"""Sequential MSE on the MI355X core (aimet_torch/v1/seq_mse.py): for every Linear / Conv2d with
weights of at most 4 bits, try `num_candidates` shrunken per-channel weight ranges, keep per output
channel the one with the smallest output reconstruction loss on calibration data, and freeze it.

Same public surface as the reference (``SeqMseParams``, ``SequentialMse`` and its methods,
``neg_sqnr``, ``apply_seq_mse`` / ``get_candidates`` / ``optimize_module``). What differs is the
candidate loop of ``optimize_module``. The reference runs, per candidate, a quantizer reset + stats
update + host encoding + table upload, a full QDQ of W, two GEMMs (the FP32 one never changes) and a
three-pass loss reduction. Here (aimet_amd/csrc/seqmse.hip):

* ``aimet_seqmse_candidate_tables``: every candidate's [4][C] table in one launch, bit-identical to
  the per-candidate path, no host round trip;
* ``aimet_seqmse_candidate_qdq``: W read once, a window of candidates written;
* per batch: XW once, ONE GEMM / conv of Xq against the window's stacked weights, and
  ``aimet_seqmse_recon_sums``: the per-(candidate, channel) loss sums in one pass over that output
  (Conv2d outputs stay NCHW: no permute copy), without atomics, bitwise reproducible.

Candidates are ``per_channel_max / num_candidates * (cand + 1)`` in fp32 with an IEEE divide (what
torch computes on the CPU); ``get_candidates`` evaluates it on the host so that it holds for device
tensors too, where torch would multiply by a rounded reciprocal instead.

The candidates of one window are held at once: ``CANDIDATE_WINDOW_BYTES`` bounds the window's
stacked weights plus the stacked output of one batch (Llama-3-8B's lm_head at 20 candidates would be
42 GB). ``checkpoints_config`` (block-wise sampling) is not implemented; calibration batches are
cached in device memory.
"""
import contextlib
import ctypes
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple, Union

import torch
import torch.nn.functional as functional

from aimet_amd import _native
from aimet_amd.activation_sampler import StopForwardException, _device_of, _to_device, default_forward_fn
from aimet_amd.libpymo import RoundingMode
from aimet_amd.qc_quantize_op import QcQuantizeOpMode, QcQuantizeWrapper
from aimet_amd.quantizers import (QuantScheme, StaticGridPerChannelQuantizer, StaticGridPerTensorQuantizer,
                                  StaticGridTensorQuantizer)
from aimet_amd.quantsim import QuantizationSimModel, _eval_mode
from aimet_amd.tensor_quantizer import _require_gpu, _stream

# The following modules with weights are supported
SUPPORTED_MODULES = (torch.nn.Linear, torch.nn.Conv2d)

# Skip running Sequential MSE if param BW is higher than supported PARAM_BW.
SUPPORTED_PARAM_BW = 4

# Upper bound, in bytes, of what one candidate window holds at a time: the QDQ'd weights of its
# candidates plus their stacked output for one batch. The window shrinks (down to one candidate)
# until it fits; 8 GiB keeps all 20 candidates of every Llama-3-8B block linear in one window.
CANDIDATE_WINDOW_BYTES = 8 << 30

_INP_SYMMETRY = ("asym", "symfp", "symqt")
_LOSS_KINDS = {"mse": 0, "l1": 1, "sqnr": 2}   # aimet_seqmse_loss
_SQNR_EPS = 1e-10


@dataclass
class SeqMseParams:
    """
    Sequential MSE parameters

    :param num_batches: Number of batches.
    :param num_candidates: Number of candidates to perform grid search. Default 20.
    :param inp_symmetry: Input symmetry. Available options are 'asym', 'symfp' and 'symqt'. Default 'symqt'.
    :param loss_fn: Loss function. Available options are 'mse', 'l1' and 'sqnr'. Default 'mse'.
    :param forward_fn: Optional adapter function that performs forward pass given a model and inputs
     yielded from the data loader. The function expects model as first argument and inputs to model as second argument.
    """
    num_batches: int
    num_candidates: int = 20
    inp_symmetry: str = 'symqt'
    loss_fn: str = 'mse'
    forward_fn: Callable = default_forward_fn


def _check_params(params: SeqMseParams):
    if params.inp_symmetry not in _INP_SYMMETRY:
        raise ValueError(f"Invalid inp_symmetry: {params.inp_symmetry}")
    if params.loss_fn not in _LOSS_KINDS:
        raise ValueError(f"Invalid loss function: {params.loss_fn}")
    if params.num_candidates < 1 or params.num_batches < 1:
        raise ValueError("num_candidates and num_batches must be at least 1")


def get_ordered_list_of_modules(model: torch.nn.Module, dummy_input, fwd_func: Callable = default_forward_fn):
    """[(name, module)] of the leaf modules in the order of their first call in one forward
    (aimet_torch/utils.py get_ordered_list_of_modules)."""
    names = {m: n for n, m in model.named_modules()}
    order, hooks = [], []

    def hook(module, *_):
        if all(module is not m for _, m in order):
            order.append((names[module], module))

    for m in model.modules():
        if not list(m.children()):
            hooks.append(m.register_forward_hook(hook))
    try:
        with _eval_mode(model), torch.no_grad():
            fwd_func(model, dummy_input)
    finally:
        for h in hooks:
            h.remove()
    return order


def _first_argmin(loss: torch.Tensor) -> torch.Tensor:
    """Per column the smallest row index that holds the column's minimum (the first minimum)."""
    n = loss.shape[0]
    rows = torch.arange(n, device=loss.device).unsqueeze(1).expand_as(loss)
    best = torch.where(loss == loss.min(0, keepdim=True)[0], rows, torch.full_like(rows, n)).min(0)[0]
    return best.clamp_(max=n - 1)


class SequentialMse:
    """
    Sequentially minimizing activation MSE loss in layer-wise way to decide optimal param quantization encodings.
    """

    @classmethod
    def apply_seq_mse(cls, model: torch.nn.Module, sim: QuantizationSimModel, data_loader, params: SeqMseParams,
                      modules_to_exclude: Optional[List[torch.nn.Module]] = None,
                      checkpoints_config: Optional[str] = None):
        """
        Sequentially minimizing activation MSE loss in layer-wise way to decide optimal param quantization encodings.

            1 Disable all input/output quantizers, param quantizers of non-supported modules
            2 Find and feeze optimal parameter encodings candidate for remaining supported modules
            3 Re-enable disabled quantizers from step 1

        Run it between ``QuantizationSimModel(...)`` and ``sim.compute_encodings(...)``. Modules in
        `modules_to_exclude` are references into the FP32 `model`.

        :param model: Original fp32 model
        :param sim: Corresponding QuantizationSimModel object
        :param data_loader: Data loader
        :param params: Sequential MSE parameters
        :param modules_to_exclude: List of supported type module(s) to exclude when applying Sequential MSE
        :param checkpoints_config: block-wise sampling config of the reference; not implemented
        """
        # pylint: disable=protected-access
        if checkpoints_config is not None:
            raise NotImplementedError("Sequential MSE with checkpoints_config (block-wise sampling) is not "
                                      "implemented")
        _check_params(params)
        if sim._quant_scheme not in (QuantScheme.post_training_tf, QuantScheme.training_range_learning_with_tf_init):
            raise AssertionError("Use TF quant-scheme with sequential MSE.")

        with cls.temporarily_disable_quantizers(model, sim, modules_to_exclude):
            # Initialize param encodings of modules of supported types.
            cls.compute_all_param_encodings(sim)

            device = _device_of(model)
            cached_dataset = []
            for batch in data_loader:
                if len(cached_dataset) == params.num_batches:
                    break
                cached_dataset.append(_to_device(batch, device))
            if len(cached_dataset) < params.num_batches:
                raise ValueError("data_loader yields %d batches, num_batches is %d" % (len(cached_dataset),
                                                                                      params.num_batches))

            fp32_modules = get_ordered_list_of_modules(model, cached_dataset[0], fwd_func=params.forward_fn)
            fp32_modules = [(name, module) for name, module in fp32_modules if isinstance(module, SUPPORTED_MODULES)]
            if modules_to_exclude:
                fp32_modules = [(name, module) for name, module in fp32_modules
                                if not any(module is m for m in modules_to_exclude)]

            # Find and freeze optimal param encodings candidate
            cls.run_seq_mse(fp32_modules, model, sim.model, params, params.forward_fn, cached_dataset,
                            cached_quant_dataset=None)

    @classmethod
    def run_seq_mse(cls, fp32_modules: List[Tuple[str, torch.nn.Module]], model: torch.nn.Module,
                    quant_model: torch.nn.Module, params: SeqMseParams, forward_fn: Callable, cached_fp_dataset,
                    cached_quant_dataset=None):
        """
        Run Sequential MSE

        :param fp32_modules: List of FP32 candidate modules in order of occurence
        :param model: FP32 model
        :param quant_model: QuantizationSimModel object
        :param params: Sequential MSE parameters
        :param forward_fn: Optional adapter function that performs forward pass given a model and inputs
        :param cached_fp_dataset: Cached batches (a sequence)
        :param cached_quant_dataset: Cached batches for the quantized model (default: the same)
        """
        _check_params(params)
        name_to_quant_module = dict(quant_model.named_modules())
        if not cached_quant_dataset:
            cached_quant_dataset = cached_fp_dataset

        for module_qualified_name, fp32_module in fp32_modules:
            try:
                quant_module = name_to_quant_module[module_qualified_name]
            except KeyError:
                continue
            if not isinstance(quant_module, QcQuantizeWrapper):
                continue
            if quant_module.param_quantizers['weight'].bitwidth > SUPPORTED_PARAM_BW:
                continue

            if params.inp_symmetry == "asym":
                fp32_inp_acts = cls.get_module_inp_acts(fp32_module, model, params, forward_fn, cached_fp_dataset)
                quant_inp_acts = cls.get_module_inp_acts(quant_module, quant_model, params, forward_fn,
                                                         cached_quant_dataset)
                cls.optimize_module(quant_module, fp32_inp_acts, quant_inp_acts, params)
            elif params.inp_symmetry == "symfp":
                fp32_inp_acts = cls.get_module_inp_acts(fp32_module, model, params, forward_fn, cached_fp_dataset)
                cls.optimize_module(quant_module, fp32_inp_acts, fp32_inp_acts, params)
            else:
                quant_inp_acts = cls.get_module_inp_acts(quant_module, quant_model, params, forward_fn,
                                                         cached_quant_dataset)
                cls.optimize_module(quant_module, quant_inp_acts, quant_inp_acts, params)

    @staticmethod
    def get_module_inp_acts(module: torch.nn.Module, model: torch.nn.Module, params: SeqMseParams,
                            forward_fn: Callable, cached_dataset) -> torch.Tensor:
        """
        For given module, get inputs to the module.

        :param module: FP32/quant module
        :param model: FP32/quant model
        :param params: Sequential MSE parameters
        :param forward_fn: Optional adapter function that performs forward pass given a model and inputs
        :param cached_dataset: Cached batches
        :return: Stacked inputs [num_batches, ...]
        """
        inp_acts = []

        def hook_fn(_, inp, __):
            if isinstance(inp, tuple):
                inp_acts.append(inp[0])
            raise StopForwardException

        handle = module.register_forward_hook(hook_fn)
        device = _device_of(model)
        try:
            iterator = iter(cached_dataset)
            for _ in range(params.num_batches):
                batch = _to_device(next(iterator), device)
                try:
                    with _eval_mode(model), torch.no_grad():
                        forward_fn(model, batch)
                except StopForwardException:
                    pass
        finally:
            handle.remove()
        return torch.stack(inp_acts)

    @staticmethod
    def _get_quantizers_to_be_disabled(model: torch.nn.Module, sim: QuantizationSimModel,
                                       modules_to_exclude: Optional[List[torch.nn.Module]]
                                       ) -> List[StaticGridTensorQuantizer]:
        """
        For given quantsim model, get all quantizers to be disabled before applying sequential MSE.
        """
        # pylint: disable=protected-access
        name_to_fp32_module_dict = dict(model.named_modules())
        quantizers_to_be_disabled = []
        for name, quant_wrapper in sim.quant_wrappers():
            for quantizer in list(quant_wrapper.input_quantizers) + list(quant_wrapper.output_quantizers):
                if quantizer.enabled:
                    quantizers_to_be_disabled.append(quantizer)

            for quantizer in quant_wrapper.param_quantizers.values():
                if not isinstance(quant_wrapper._module_to_wrap, SUPPORTED_MODULES) and quantizer.enabled:
                    quantizers_to_be_disabled.append(quantizer)

            # disable param quantizers from exclusion list
            if modules_to_exclude:
                fp32_module = name_to_fp32_module_dict.get(name)
                if fp32_module is not None and any(fp32_module is m for m in modules_to_exclude):
                    for quantizer in quant_wrapper.param_quantizers.values():
                        if quantizer.enabled and not any(quantizer is q for q in quantizers_to_be_disabled):
                            quantizers_to_be_disabled.append(quantizer)
        return quantizers_to_be_disabled

    @classmethod
    @contextlib.contextmanager
    def temporarily_disable_quantizers(cls, model: torch.nn.Module, sim: QuantizationSimModel,
                                       modules_to_exclude: Optional[List[torch.nn.Module]]):
        """
        For given quantsim model, disable quantizers needed to be disabled before applying sequential MSE,
        and enable them again afterwards (also when an exception is raised).

        :param model: Original fp32 model
        :param sim: QuantizationSimModel object
        :param modules_to_exclude: List of supported modules to exclude when applying Sequential MSE
        """
        quantizers_to_be_disabled = cls._get_quantizers_to_be_disabled(model, sim, modules_to_exclude)
        for quantizer in quantizers_to_be_disabled:
            quantizer.enabled = False
        try:
            yield
        finally:
            for quantizer in quantizers_to_be_disabled:
                quantizer.enabled = True

    @staticmethod
    def compute_all_param_encodings(sim: QuantizationSimModel):
        """
        Compute encodings for all parameters, needed for initializing Sequential MSE

        :param sim: Quant sim
        """
        for _, quant_wrapper in sim.quant_wrappers():
            for name, quantizer in quant_wrapper.param_quantizers.items():
                quantizer.reset_encoding_stats()
                quantizer.update_encoding_stats(getattr(quant_wrapper, name).data)
                quantizer.compute_encoding()

            # Wrapper mode must be set to ACTIVE because the wrapper's quantize_dequantize_params() will only call
            # into the param tensor quantizer's quantize_dequantize() if the mode isn't PASSTHROUGH.
            quant_wrapper.set_mode(QcQuantizeOpMode.ACTIVE)

    @classmethod
    def get_per_channel_min_and_max(cls, quant_module: QcQuantizeWrapper
                                    ) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """
        Get per channel min/max values across output channel (float32; 16-bit weights are upcast as
        update_encoding_stats does).

        :param quant_module: Quant module to be optimized
        :return: (per_channel_min or None for a symmetric quantizer, per_channel_max)
        """
        module = cls._get_original_module(quant_module)
        if isinstance(module, torch.nn.Conv2d):
            weight = module.weight.reshape(module.out_channels, -1)
        elif isinstance(module, torch.nn.Linear):
            weight = module.weight
        else:
            raise ValueError('Unsupported module: ', module)
        weight = weight.detach().to(torch.float32)

        if cls._is_symmetric_quantizer(quant_module.param_quantizers["weight"]):
            per_channel_max = torch.max(weight.abs(), dim=1)[0]
            per_channel_min = None
        else:
            per_channel_max = torch.max(weight, dim=1)[0]
            per_channel_min = torch.min(weight, dim=1)[0]
        return per_channel_min, per_channel_max

    @staticmethod
    def get_candidates(num_candidates: int, per_channel_max: torch.Tensor,
                       per_channel_min: Optional[torch.Tensor]) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """
        Perform grid search: candidate `cand` is ``per_channel_max / num_candidates * (cand + 1)`` (and the
        same for min, or ``-cand_max`` without one), an IEEE fp32 divide and then a multiply -- evaluated on
        the host so that device tensors give the same bits -- on the device of `per_channel_max`.

        :param num_candidates: Number of candidates
        :param per_channel_max: Per channel max values
        :param per_channel_min: Per channel min values
        :return: candidates [(cand_max, cand_min)]
        """
        device = per_channel_max.device
        step_max = per_channel_max.detach().cpu() / num_candidates
        step_min = per_channel_min.detach().cpu() / num_candidates if per_channel_min is not None else None
        candidates = []
        for cand in range(num_candidates):
            cand_max = step_max * (cand + 1)
            cand_min = step_min * (cand + 1) if step_min is not None else -cand_max
            candidates.append((cand_max.to(device), cand_min.to(device)))
        return candidates

    @classmethod
    def optimize_module(cls, quant_module: QcQuantizeWrapper, x: torch.Tensor, xq: torch.Tensor,
                        params: SeqMseParams):
        """
        Find and freeze optimal parameter encodings candidate for given module.

        :param quant_module: Quant module to be optimized
        :param x: Inputs to module from FP32 model [num_batches, ...]
        :param xq: Inputs to module from QuantSim model [num_batches, ...]
        :param params: Sequenial MSE parameters
        """
        # pylint: disable=too-many-locals
        _check_params(params)
        quantizer = quant_module.param_quantizers['weight']
        per_channel_min, per_channel_max = cls.get_per_channel_min_and_max(quant_module)
        candidates = cls.get_candidates(params.num_candidates, per_channel_max, per_channel_min)

        with torch.no_grad():
            total_loss = cls._candidate_losses(quant_module, per_channel_min, per_channel_max, x, xq, params)
            best_indices = _first_argmin(total_loss).unsqueeze(0)
            best_max = torch.stack([cand_max for cand_max, _ in candidates]).gather(0, best_indices)[0]
            best_min = torch.stack([cand_min for _, cand_min in candidates]).gather(0, best_indices)[0]

        # Compute and freeze parameter encodings using best candidate
        cls.compute_param_encodings(quantizer, best_min, best_max)
        cls._freeze_quantizer_encoding(quantizer)

    @classmethod
    def _candidate_losses(cls, quant_module, per_channel_min, per_channel_max, x, xq, params) -> torch.Tensor:
        """total_loss [num_candidates, C] of the reference's candidate loop, on the fused kernels."""
        # pylint: disable=too-many-locals
        module = cls._get_original_module(quant_module)
        quantizer = quant_module.param_quantizers['weight']
        w = module.weight.detach()
        _require_gpu(w, what="weight", allow_16bit=True)
        n_cand = int(params.num_candidates)
        C = w.shape[0]
        K = w[0].numel()
        w32 = w.to(torch.float32).contiguous()
        conv = isinstance(module, torch.nn.Conv2d)
        grouped = conv and module.groups > 1

        # (a) tables of every candidate. A per-tensor quantizer sees the whole [C, 2] tensor of a
        # candidate: its range is the candidates' overall min / max (the grid is monotonic in them)
        per_channel = isinstance(quantizer, StaticGridPerChannelQuantizer)
        t_max = per_channel_max if per_channel else per_channel_max.max().reshape(1)
        t_min = per_channel_min
        if t_min is not None and not per_channel:
            t_min = t_min.min().reshape(1)
        tC = t_max.numel()
        t_max = t_max.to(torch.float32).contiguous()
        t_min = t_min.to(torch.float32).contiguous() if t_min is not None else None
        tables = torch.empty((n_cand, 4, tC), dtype=torch.float32, device=w.device)
        with torch.cuda.device(w.device):
            _native.call("aimet_seqmse_candidate_tables", t_min.data_ptr() if t_min is not None else None,
                         t_max.data_ptr(), tC, n_cand, int(quantizer.bitwidth),
                         int(bool(quantizer.use_symmetric_encodings)), int(bool(quantizer.use_strict_symmetric)),
                         int(bool(quantizer.use_unsigned_symmetric)), tables.data_ptr(), _stream(w))

        # window: the candidates held at once
        rows = xq[0].numel() // max(xq[0].shape[1 if conv else -1], 1)   # tokens, or images x input pixels
        per_candidate = 4 * C * K + (w.element_size() * C * K if w.dtype != torch.float32 else 0) + 4 * C * rows
        window = max(1, min(n_cand, CANDIDATE_WINDOW_BYTES // max(per_candidate, 1)))

        total_loss = torch.zeros((n_cand, C), dtype=torch.float32, device=w.device)
        for first in range(0, n_cand, window):
            count = min(window, n_cand - first)
            # (b) QDQ of the window's candidates from one read of W
            wq = torch.empty((count,) + tuple(w.shape), dtype=torch.float32, device=w.device)
            with torch.cuda.device(w.device):
                _native.call("aimet_seqmse_candidate_qdq", w32.data_ptr(), wq.data_ptr(), C if per_channel else 1,
                             K if per_channel else C * K, tables.data_ptr(), n_cand, first, count, _stream(w))
            wq = wq.to(w.dtype)
            stacked = wq.reshape((count * C,) + tuple(w.shape[1:]))
            for batch_idx in range(params.num_batches):
                xb, xqb = x[batch_idx], xq[batch_idx]
                if grouped:
                    # one conv per candidate; still one QDQ launch and the fused loss
                    for j in range(count):
                        xqwq, xw = cls.compute_outputs(quant_module, xb, xqb, w, wq[j])
                        total_loss[first + j] += cls.compute_recon_loss(xqwq, xw, params, channel_dim=1)
                    continue
                xqwq, xw = cls.compute_outputs(quant_module, xb, xqb, w, stacked)
                loss = cls.compute_recon_loss(xqwq, xw, params, channel_dim=1 if conv else -1)
                total_loss[first:first + count] += loss.view(count, C)
            del wq, stacked
        return total_loss

    @staticmethod
    def compute_param_encodings(quantizer: Union[StaticGridPerTensorQuantizer, StaticGridPerChannelQuantizer],
                                x_min: torch.Tensor, x_max: torch.Tensor):
        """
        Compute encodings for parameter quantizer using given x_min and x_max values.

        :param quantizer: Tensor quantizer
        :param x_min: min values
        :param x_max: max values
        """
        tensor = torch.stack([x_min, x_max], dim=-1)
        quantizer.reset_encoding_stats()
        quantizer.update_encoding_stats(tensor)
        quantizer.compute_encoding()

    @classmethod
    def compute_outputs(cls, quant_module: QcQuantizeWrapper, x: torch.Tensor, xq: torch.Tensor, w: torch.Tensor,
                        wq: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        Compute X^W^ and XW output activations. `wq` may hold several candidates stacked along the output
        channels ([count * C, ...], groups == 1): candidate j's channel c is output channel j * C + c.
        A Conv2d's outputs stay [N, C, H, W] (the reference permutes them to channels-last; pass
        ``channel_dim=1`` to compute_recon_loss instead).

        :param quant_module: Wrapper module to be optimized
        :param x: Inputs from FP32 model
        :param xq: Inputs from QuantSim model
        :param w: FP32 weights
        :param wq: Quantized-dequantized weights
        :return: xqwq, xw
        """
        module = cls._get_original_module(quant_module)
        if isinstance(module, torch.nn.Linear):
            xqwq = functional.linear(xq, wq)
            xw = functional.linear(x, w)
        elif isinstance(module, torch.nn.Conv2d):
            xqwq = functional.conv2d(xq, wq, stride=module.stride, dilation=module.dilation,
                                     padding=module.padding, groups=module.groups)
            xw = functional.conv2d(x, w, stride=module.stride, dilation=module.dilation,
                                   padding=module.padding, groups=module.groups)
        else:
            raise ValueError('Unsupported module: ', module)
        return xqwq, xw

    @staticmethod
    def compute_recon_loss(xqwq: torch.Tensor, xw: torch.Tensor, params: SeqMseParams, channel_dim: int = -1):
        """
        Compute reconstruction loss and return the sum by reducing over all the dimensions except the
        channel dimension (the last one, or dimension 1 of an [N, C, ...] tensor), in one fused pass.
        `xqwq` may hold `count` candidates stacked along the channel dimension (count * C channels
        against xw's C); the result then has count * C entries, candidate-major.

        :param xqwq: X^Q^ quantized-dequantized values
        :param xw: XW FP32 values
        :param params: Sequential MSE parameters
        :param channel_dim: -1 (channels last) or 1 ([N, C, ...])
        :return: loss
        """
        if params.loss_fn not in _LOSS_KINDS:
            raise ValueError(f"Invalid loss function: {params.loss_fn}")
        kind = _LOSS_KINDS[params.loss_fn]
        if channel_dim in (-1, xw.dim() - 1):
            C, Cq = xw.shape[-1], xqwq.shape[-1]
            outer, inner = xw.numel() // max(C, 1), 1
        elif channel_dim == 1:
            C, Cq = xw.shape[1], xqwq.shape[1]
            outer, inner = xw.shape[0], xw[0, 0].numel()
        else:
            raise ValueError("channel_dim must be -1 or 1")
        if C == 0 or Cq % C != 0 or xqwq.numel() != outer * Cq * inner:
            raise ValueError("xqwq %s does not stack candidates of xw %s" % (tuple(xqwq.shape), tuple(xw.shape)))
        count = Cq // C
        _require_gpu(xw, what="xw", allow_16bit=True)
        _require_gpu(xqwq, what="xqwq", allow_16bit=True)
        xw = xw.to(torch.float32).contiguous()
        xqwq = xqwq.to(torch.float32).contiguous()
        err = torch.empty((count, C), dtype=torch.float32, device=xw.device)
        sig = torch.empty((C,), dtype=torch.float32, device=xw.device) if params.loss_fn == "sqnr" else None
        nbytes = ctypes.c_int64(0)
        _native.call("aimet_seqmse_recon_sums_workspace", outer, C, inner, count, ctypes.byref(nbytes))
        workspace = torch.empty((max(nbytes.value // 4, 1),), dtype=torch.float32, device=xw.device)
        with torch.cuda.device(xw.device):
            _native.call("aimet_seqmse_recon_sums", xw.data_ptr(), xqwq.data_ptr(), outer, C, inner, count, kind,
                         err.data_ptr(), sig.data_ptr() if sig is not None else None, workspace.data_ptr(),
                         nbytes.value, _stream(xw))
        if sig is None:
            return err.reshape(-1)
        # neg_sqnr from the sums: means over the outer * inner rows of each channel
        n = float(outer * inner)
        sqnr = (sig / n).unsqueeze(0) / (err / n + _SQNR_EPS)
        return (-10 * torch.log10(sqnr)).reshape(-1)

    @staticmethod
    def _is_symmetric_quantizer(quantizer: StaticGridTensorQuantizer):
        return quantizer.use_symmetric_encodings

    @staticmethod
    def _freeze_quantizer_encoding(quantizer: StaticGridTensorQuantizer):
        return quantizer.freeze_encoding()

    @staticmethod
    def _get_quantized_weight(quant_module: QcQuantizeWrapper):
        w = quant_module.weight
        return quant_module.param_quantizers['weight'].quantize_dequantize(w, RoundingMode.ROUND_NEAREST)

    @staticmethod
    def _get_original_module(quant_module: QcQuantizeWrapper):
        # pylint: disable=protected-access
        return quant_module._module_to_wrap


def neg_sqnr(pred: torch.Tensor, target: torch.Tensor, eps=_SQNR_EPS, reduction="none"):
    """
    Loss function to minimize negative SQNR which is equivalent to maximizing SQNR.

    :param pred: X^Q^ quantized-dequantized values
    :param target: XW FP32 values
    :param eps: epsilon
    :param reduction: unused arg
    :return: Negative SQNR
    """
    # pylint: disable=unused-argument
    quant_error = target - pred
    exp_noise = torch.mean(quant_error ** 2, 0, keepdim=True) + eps
    exp_signal = torch.mean(target ** 2, 0, keepdim=True)
    sqnr = exp_signal / exp_noise
    sqnr_db = 10 * torch.log10(sqnr)
    return -sqnr_db


# Global variables for compatibility
apply_seq_mse = SequentialMse.apply_seq_mse
get_candidates = SequentialMse.get_candidates
optimize_module = SequentialMse.optimize_module
