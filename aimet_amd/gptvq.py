"""GPTVQ on the MI355X core (aimet_torch/gptvq/): every Linear / Conv2d weight becomes a small codebook
of `vector_dim`-dimensional vectors per (row group, column block), found by k-means, while a GPTQ-style
sweep over the columns pushes the error of each quantized vector into the columns not yet quantized
through the inverse Hessian of the layer input.

Same public surface as the reference (``GPTVQParameters``, ``GPTVQ`` and its helpers,
``GPTVQOptimizer``, the functions of ``gptvq/utils.py``). What differs is where the two hot loops run
(aimet_amd/csrc/gptvq.hip):

* ``aimet_gptvq_kmeans``: all Lloyd iterations of one column block in one launch, one workgroup per
  row group with the group's vectors in LDS (the reference materialises a [G][N][K][D] distance tensor
  and a [G][N][K] one-hot per iteration);
* ``aimet_gptvq_block_update``: the column sweep inside one block of at most 128 columns in one launch
  (the reference: ~15 launches per `vector_dim` columns).

Codebook initialisation (``hacky_mahalanobis_init``, with a stable argsort), the Hessian accumulation,
the Cholesky factorisations and the cross-block update ``W[:, block_end:] -= err @ hinv[block,
block_end:]`` stay torch operations on the device.

The group quantizer. The reference uses a blockwise quantizer of shape (G, 1) from aimet_torch.v2,
whose source is not part of the reference snapshot. Here it is the project's own per-channel grid on
the weight viewed as [G][rows_per_block * cols]: TF min/max statistics per group, bitwidth
``vector_bw``, the symmetry that the sim's configuration gives the weight quantizer, and the usual
[4][G] table. The codebook QDQ is the per-channel QDQ of the codebook viewed as [G][K * D] with that
table, and the final QDQ of the weight uses the same table. The exported file repeats each group's
encoding ``rows_per_block`` times, so that a per-channel sim can load it.

While GPTVQ runs, every quantizer of the sim is off: a sampling forward sees the FP32 weights of the
modules that are not optimized yet and the GPTVQ weights (already on their grid) of those that are.
``HESSIAN_WEIGHTED_LOOKUP`` and ``DO_CODEBOOK_FINE_TUNING`` are not implemented.
"""
import collections
import contextlib
import itertools
import json
import math
import os
import time
from dataclasses import dataclass
from typing import Any, Callable, Dict, Iterable, List, Optional, Set, Tuple, Union

import torch
from torch import nn

from aimet_amd import _native
from aimet_amd.activation_sampler import StopForwardException, _device_of, _to_device
from aimet_amd.encodings_io import create_encoding_dict
from aimet_amd.qc_quantize_op import QcQuantizeWrapper
from aimet_amd.quantizers import QuantScheme, StaticGridPerChannelQuantizer
from aimet_amd.quantsim import QuantizationSimModel, _eval_mode
from aimet_amd.seq_mse import get_ordered_list_of_modules
from aimet_amd.tensor_quantizer import _require_gpu, _stream, qdq_per_channel_table

GPTVQSupportedModules = (nn.Linear, nn.Conv2d)
DAMPENING_PERCENTAGE = 0.01
BLOCK_STRIDE = 128

HESSIAN_WEIGHTED_LOOKUP = False
DO_CODEBOOK_FINE_TUNING = False


@dataclass
class GPTVQParameters:
    """
    Data carrier containing GPTVQ parameters
    """
    # pylint: disable=too-many-instance-attributes
    data_loader: Iterable
    forward_fn: Callable[[nn.Module, Any], Any]
    row_axis: int = 0
    col_axis: int = 1
    rows_per_block: int = 32
    cols_per_block: int = 256
    vector_dim: int = 2
    vector_bw: int = 8
    vector_stride: int = 1
    index_bw: int = 6
    num_of_kmeans_iterations: int = 100
    assignment_chunk_size: Optional[int] = None


def _check_flags():
    if HESSIAN_WEIGHTED_LOOKUP:
        raise NotImplementedError("GPTVQ with HESSIAN_WEIGHTED_LOOKUP is not implemented")
    if DO_CODEBOOK_FINE_TUNING:
        raise NotImplementedError("GPTVQ with DO_CODEBOOK_FINE_TUNING is not implemented")


def _unwrap(module: nn.Module) -> nn.Module:
    return module.get_original_module() if isinstance(module, QcQuantizeWrapper) else module


# ---------------------------------------------------------------------------------------------------
# gptvq/utils.py
# ---------------------------------------------------------------------------------------------------
def _first_argmin_last(distance: torch.Tensor) -> torch.Tensor:
    """The smallest index along the last dimension that holds the minimum (the first minimum)."""
    k = distance.shape[-1]
    index = torch.arange(k, device=distance.device).expand_as(distance)
    best = distance.min(-1, keepdim=True)[0]
    return torch.where(distance == best, index, torch.full_like(index, k)).min(-1)[0].clamp_(max=k - 1)


def hacky_mahalanobis_init(tensor: torch.Tensor, num_of_centroids: int) -> torch.Tensor:
    """
    Initialize centroids using hacky Mahalanobis: the vectors at evenly spaced ranks of the distance
    to the group's mean (a stable sort, so that equal distances keep their order).

    :param tensor: num_blocks_per_column x N x vector_dim weight tensor
    :param num_of_centroids: Number of centroids
    :return: Initialized codebook
    """
    vector_dim = tensor.shape[-1]
    mu = tensor.mean(1).unsqueeze(1)
    x_centered = tensor - mu

    dists = x_centered.pow(2).sum(-1)
    sorted_dists = torch.argsort(dists, dim=1, stable=True)  # num_blocks_per_column x N
    idx = torch.round(torch.linspace(0, x_centered.shape[1] - 1, num_of_centroids)).long().to(tensor.device)

    idx = sorted_dists[:, idx].unsqueeze(-1).expand(-1, -1, vector_dim)
    return torch.gather(tensor, dim=1, index=idx)


def manipulate_inverse_hessian_diagonal(tensor: torch.Tensor,
                                        inverse_hessian_diagonal: Optional[torch.Tensor]) -> torch.Tensor:
    """Manipulate diagonal of inverse Hessian tensor if needed (gptvq/utils.py:102-122)."""
    if inverse_hessian_diagonal is None:
        return torch.ones(tensor.shape[-1], device=tensor.device, dtype=tensor.dtype)
    if inverse_hessian_diagonal.ndim > 2:  # should then be 1 x N x vector_dim
        assert (inverse_hessian_diagonal.shape[0] == 1 and inverse_hessian_diagonal.shape[1] == tensor.shape[1]
                and inverse_hessian_diagonal.shape[2] == tensor.shape[2]), \
            f"{inverse_hessian_diagonal.shape, tensor.shape}"
        return inverse_hessian_diagonal.unsqueeze(2)  # 1 x N x 1 x vector_dim
    return inverse_hessian_diagonal


def get_assignments(tensor: torch.Tensor, centroids: torch.Tensor,
                    inverse_hessian_diagonal: Optional[torch.Tensor] = None,
                    chunk_size: Optional[int] = None) -> torch.Tensor:
    """
    Calculate nearest centroid index tensor (the torch form; the first minimum on ties)

    :param tensor: num_blocks_per_column x N x vector_dim
    :param centroids: num_blocks_per_column x num_centroids x vector_dim
    :param inverse_hessian_diagonal: Diagonal of inverse Hessian tensor
    :param chunk_size: Chunk size for better memory management
    :return: nearest centroid index tensor
    """
    hessian = manipulate_inverse_hessian_diagonal(tensor, inverse_hessian_diagonal)
    tensor_chunks = [tensor] if chunk_size is None else torch.split(tensor, chunk_size, dim=1)
    if chunk_size is None:
        hessian_chunks = [hessian]
    elif hessian.ndim > 1:
        hessian_chunks = torch.split(hessian, chunk_size, dim=1)
    else:
        hessian_chunks = [hessian] * len(tensor_chunks)

    centroids = centroids.unsqueeze(1)  # num_blocks_per_column x 1 x num_centroids x vector_dim
    assignments = []
    for tensor_chunk, hessian_chunk in zip(tensor_chunks, hessian_chunks):
        tensor_chunk = tensor_chunk.unsqueeze(2)  # num_blocks_per_column x N x 1 x vector_dim
        distance = ((tensor_chunk - centroids).pow(2) * hessian_chunk).sum(-1)
        assignments.append(_first_argmin_last(distance))
    return torch.concat(assignments, dim=1)  # num_blocks_per_column x N


def do_kmeans_maximization(tensor: torch.Tensor, centroids: torch.Tensor, assignments: torch.Tensor,
                           inverse_hessian_diagonal: Optional[torch.Tensor]) -> torch.Tensor:
    """
    Do K-means maximization step (the torch form, gptvq/utils.py:203-241)

    :param tensor: torch.Tensor (num_blocks_per_column x N x vector_dim)
    :param centroids: Codebook including centroids (num_blocks_per_column x num_centroids x vector_dim)
    :param assignments: Assignment result from expectation step (num_blocks_per_column x N)
    :param inverse_hessian_diagonal: Diagonal of inverse Hessian (1 x N x vector_dim)
    :return: Updated codebook after maximization step
    """
    centroid_range = torch.arange(centroids.shape[1], device=centroids.device)
    expanded_assignments = (assignments.unsqueeze(-1) == centroid_range.view(1, 1, -1)).to(tensor.dtype)
    if inverse_hessian_diagonal is None:
        norm = 1.0 / torch.clip(expanded_assignments.sum(1), min=1)
        return torch.einsum("gnd,gnk,gk->gkd", tensor, expanded_assignments, norm)
    norm = 1.0 / torch.clip(torch.einsum("gnk,nd->gkd", expanded_assignments, inverse_hessian_diagonal[0]),
                            min=1e-10)
    return torch.einsum("gnd,nd,gnk,gkd->gkd", tensor, inverse_hessian_diagonal[0], expanded_assignments, norm)


def _kmeans(w2d: torch.Tensor, c0: int, ncols: int, rows_per_block: int, vector_dim: int, codebook: torch.Tensor,
            iterations: int):
    """aimet_gptvq_kmeans on columns [c0, c0 + ncols) of the contiguous fp32 `w2d`; `codebook`
    [G][K][D] (contiguous fp32) is updated in place."""
    rows, cols = w2d.shape
    with torch.cuda.device(w2d.device):
        _native.call("aimet_gptvq_kmeans", w2d.data_ptr() + 4 * c0, cols, rows // rows_per_block, rows_per_block,
                     ncols, vector_dim, codebook.shape[1], int(iterations), codebook.data_ptr(), _stream(w2d))


def generate_codebook(weight_block: torch.Tensor, num_of_centroids: int,
                      inverse_hessian_diagonal: Optional[torch.Tensor] = None,
                      assignment_chunk_size: Optional[int] = None, kmeans_iteration: int = 100):
    """
    Generate and optimize codebook using K-means and return it: the initialisation in torch, every
    Lloyd iteration in one launch of aimet_gptvq_kmeans.

    :param weight_block: Weight block (num_blocks_per_column x N x vector_dim, a HIP tensor)
    :param num_of_centroids: Number of centroids
    :param inverse_hessian_diagonal: Diagonal of inverse Hessian tensor (not implemented)
    :param assignment_chunk_size: unused (the kernel never materialises the distances)
    :param kmeans_iteration: Number of K-means iterations
    :return: Optimized codebook
    """
    # pylint: disable=unused-argument
    if inverse_hessian_diagonal is not None:
        raise NotImplementedError("GPTVQ with HESSIAN_WEIGHTED_LOOKUP is not implemented")
    _require_gpu(weight_block, what="weight_block")
    groups, n, vector_dim = weight_block.shape
    block = weight_block.contiguous()
    codebook = hacky_mahalanobis_init(block, num_of_centroids).contiguous()
    # group g is row g of a [G][N * D] matrix
    _kmeans(block.view(groups, n * vector_dim), 0, n * vector_dim, 1, vector_dim, codebook, kmeans_iteration)
    return codebook


def quantize_dequantize_codebook(codebook: torch.Tensor, quantizer: StaticGridPerChannelQuantizer,
                                 num_blocks_per_column: int) -> torch.Tensor:
    """
    Quantize-Dequantize codebook with the group quantizer's table: group g's centroids on group g's grid

    :param codebook: Codebook
    :param quantizer: Group quantizer (one channel per row group)
    :param num_blocks_per_column: Number of blocks per column
    :return: Quantize-Dequantized codebook
    """
    flat = codebook.reshape(num_blocks_per_column, -1).contiguous()
    table = quantizer.channel_table(flat.device)
    return qdq_per_channel_table(flat, table, 1, num_blocks_per_column, flat.shape[1]).reshape(codebook.shape)


def get_2d_tensor_shape(quant_module: nn.Module) -> torch.Size:
    """
    Compute the 2D shape (rows, columns) of the weight of a (wrapped) module

    :param quant_module: Quantization module
    :return: 2D tensor shape
    """
    module = _unwrap(quant_module)
    if isinstance(module, nn.Linear):
        return module.weight.shape
    if isinstance(module, nn.Conv2d):
        return module.weight.flatten(1).shape
    raise ValueError(f"Unsupported module type {type(module)}")


def update_hessian(quant_module: nn.Module, inp: torch.Tensor, n_samples: int, curr_batch_size: int,
                   hessian: torch.Tensor):
    """
    Updates the hessian matrix using the passed input data to the module and applies scaling

    :param quant_module: Quantization module
    :param inp: activation input passed to the given module
    :param n_samples: samples seen so far for hessian computation
    :param curr_batch_size: batch size of current input
    :param hessian: hessian for the module used to do weight update
    """
    module = _unwrap(quant_module)
    if isinstance(module, nn.Linear):
        if len(inp.shape) >= 3:
            inp = inp.reshape((-1, inp.shape[-1]))
        inp = inp.T
    elif isinstance(module, nn.Conv2d):
        unfold = nn.Unfold(module.kernel_size, dilation=module.dilation, padding=module.padding,
                           stride=module.stride)
        inp = unfold(inp)
        inp = inp.permute([1, 0, 2])
        inp = inp.flatten(1)
    else:
        raise ValueError(f"Unsupported module type {type(module)}")

    hessian *= n_samples / (n_samples + curr_batch_size)
    inp = math.sqrt(2 / (n_samples + curr_batch_size)) * inp.float()
    hessian += inp.matmul(inp.T)


def get_module_name_to_hessian_tensor(gptvq_params: GPTVQParameters, sim: QuantizationSimModel,
                                      module_names: List[str]) -> Dict[str, torch.Tensor]:
    """
    Get module name to Hessian tensor dictionary: one forward per batch for all the modules, stopped
    after the last of them has run (BlockModuleData of the reference).

    :param gptvq_params: Data carrier holding GPTVQ parameters
    :param sim: QuantizationSimModel object
    :param module_names: Topologically ordered module names
    :return: Module name to Hessian tensor dictionary
    """
    name_to_module = dict(sim.model.named_modules())
    module_to_name = {name_to_module[name]: name for name in module_names}
    name_to_hessian = {}
    for name in module_names:
        _, num_cols = get_2d_tensor_shape(name_to_module[name])
        device = _unwrap(name_to_module[name]).weight.device
        name_to_hessian[name] = torch.zeros((num_cols, num_cols), device=device)

    device = _device_of(sim.model)
    n_samples = 0
    for current_data in gptvq_params.data_loader:
        inp_data_dict = {}

        def hook(module, inp, _):
            inp_data_dict[module_to_name[module]] = inp[0].detach()
            if module_to_name[module] == module_names[-1]:
                raise StopForwardException

        handles = [name_to_module[name].register_forward_hook(hook) for name in module_names]
        try:
            with _eval_mode(sim.model), torch.no_grad():
                gptvq_params.forward_fn(sim.model, _to_device(current_data, device))
        except StopForwardException:
            pass
        finally:
            for handle in handles:
                handle.remove()

        curr_batch_size = 0
        for name, inp_data in inp_data_dict.items():
            if len(inp_data.shape) == 2:
                inp_data = inp_data.unsqueeze(0)
            curr_batch_size = inp_data.shape[0]
            update_hessian(name_to_module[name], inp_data, n_samples, curr_batch_size, name_to_hessian[name])
        n_samples += curr_batch_size
    return name_to_hessian


# ---------------------------------------------------------------------------------------------------
# gptvq/gptvq_optimizer.py
# ---------------------------------------------------------------------------------------------------
class GPTVQOptimizer:
    """
    Optimizes the weight rounding of quantized wrapper module
    """
    # record_hook(module, info), when set, sees what weight_update decided: the QDQ'd codebooks, their
    # column ranges, the indices of every step and the group table (the tests read the structure of
    # the result through it)
    record_hook: Optional[Callable] = None
    # a dict here makes weight_update synchronise around its phases and add their seconds to it
    phase_times: Optional[Dict[str, float]] = None
    # True once torch.linalg.cholesky on the device has failed and the host took over
    cholesky_on_host = False

    @classmethod
    @contextlib.contextmanager
    def _phase(cls, name: str, device):
        times = cls.phase_times
        if times is None:
            yield
            return
        torch.cuda.synchronize(device)
        start = time.perf_counter()
        try:
            yield
        finally:
            torch.cuda.synchronize(device)
            times[name] = times.get(name, 0.0) + time.perf_counter() - start

    @staticmethod
    def _group_quantizer(quantizer, num_groups: int) -> StaticGridPerChannelQuantizer:
        """The per-group weight quantizer: the sim's weight quantizer's bitwidth and symmetry, one
        channel per row group, TF statistics."""
        group_quantizer = StaticGridPerChannelQuantizer(quantizer.bitwidth, quantizer.round_mode,
                                                        QuantScheme.post_training_tf, quantizer.use_symmetric_encodings,
                                                        num_groups, True, ch_axis=0)
        group_quantizer.use_strict_symmetric = quantizer.use_strict_symmetric
        group_quantizer.use_unsigned_symmetric = quantizer.use_unsigned_symmetric
        return group_quantizer

    # pylint: disable=too-many-locals, too-many-statements
    @classmethod
    def weight_update(cls, module: QcQuantizeWrapper, gptvq_params: GPTVQParameters, hessian: torch.Tensor):
        """
        Update the weights of module via GPTVQ optimization

        :param module: Quantization wrapper of a Linear / Conv2d
        :param gptvq_params: Data carrier including GPTVQ parameters
        :param hessian: Hessian tensor to be used for computing GPTVQ optimization (changed in place)
        """
        _check_flags()
        inner = _unwrap(module)
        quantizer = module.param_quantizers["weight"]
        weight = inner.weight.detach()
        _require_gpu(weight, what="weight", allow_16bit=True)
        device = weight.device
        num_rows, num_cols = get_2d_tensor_shape(inner)
        rows_per_block, columns_per_block = gptvq_params.rows_per_block, gptvq_params.cols_per_block
        vector_dim = gptvq_params.vector_dim
        assert num_rows % rows_per_block == 0, (f"The number of rows in weight (#: {num_rows}) should be divided by "
                                                f"rows per block (#: {rows_per_block})")
        if BLOCK_STRIDE % vector_dim or columns_per_block % vector_dim or num_cols % vector_dim:
            raise ValueError(f"vector_dim ({vector_dim}) must divide {BLOCK_STRIDE}, cols_per_block "
                             f"({columns_per_block}) and the number of columns ({num_cols})")
        if tuple(hessian.shape) != (num_cols, num_cols):
            raise ValueError(f"Hessian of shape {tuple(hessian.shape)} for a weight with {num_cols} columns")
        num_blocks_per_column = num_rows // rows_per_block
        num_of_centroids = 2 ** gptvq_params.index_bw

        with torch.no_grad():
            # 1-1. if any diagonal elements are zero, mark them as 1, and corresponding weight as 0
            rounded_weight = weight.flatten(1).float().contiguous()
            if rounded_weight.data_ptr() == weight.data_ptr():
                rounded_weight = rounded_weight.clone()
            dead = torch.diag(hessian) == 0
            hessian[dead, dead] = 1
            rounded_weight[:, dead] = 0

            # 1-2. the group encodings, after the dead columns are zeroed
            group_quantizer = cls._group_quantizer(quantizer, num_blocks_per_column)
            group_quantizer.update_encoding_stats(rounded_weight.view(num_blocks_per_column, -1))
            group_quantizer.compute_encoding()
            table = group_quantizer.channel_table(device)

            # 2. apply per channel dampening to have stability in hessian inverse computation
            with cls._phase("cholesky", device):
                damp = DAMPENING_PERCENTAGE * torch.mean(torch.diag(hessian))
                diag = torch.arange(num_cols, device=device)
                hessian[diag, diag] += damp
                hessian_inv = cls.compute_inverse(hessian).contiguous()

            codebook = None
            codebooks, codebook_cols = [], []
            all_indices = torch.empty((num_rows, num_cols // vector_dim), dtype=torch.int32, device=device)
            for block_start_idx in range(0, num_cols, BLOCK_STRIDE):
                block_end_idx = min(block_start_idx + BLOCK_STRIDE, num_cols)
                count = block_end_idx - block_start_idx
                error_block = torch.zeros((num_rows, count), dtype=torch.float32, device=device)
                indices = torch.empty((num_rows, count // vector_dim), dtype=torch.int32, device=device)
                i = 0
                while i < count:
                    col = block_start_idx + i
                    if col % columns_per_block == 0:
                        ncols = min(columns_per_block, num_cols - col)
                        with cls._phase("kmeans_init", device):
                            block = rounded_weight[:, col:col + ncols].reshape(num_blocks_per_column, -1, vector_dim)
                            codebook = hacky_mahalanobis_init(block, num_of_centroids).contiguous()
                            del block
                        with cls._phase("kmeans", device):
                            _kmeans(rounded_weight, col, ncols, rows_per_block, vector_dim, codebook,
                                    gptvq_params.num_of_kmeans_iterations)
                        codebook = quantize_dequantize_codebook(codebook, group_quantizer, num_blocks_per_column)
                        codebooks.append(codebook)
                        codebook_cols.append((col, ncols))
                    # up to the block's end or the next codebook boundary inside it
                    stop = min(count, (col // columns_per_block + 1) * columns_per_block - block_start_idx)
                    with cls._phase("sweep", device):
                        cls._sweep(rounded_weight, rows_per_block, block_start_idx, i, stop, block_end_idx,
                                   vector_dim, codebook, hessian_inv, error_block, indices)
                    i = stop
                all_indices[:, block_start_idx // vector_dim:block_end_idx // vector_dim] = indices
                if block_end_idx < num_cols:
                    with cls._phase("cross_block_gemm", device):
                        rounded_weight[:, block_end_idx:] -= error_block.matmul(
                            hessian_inv[block_start_idx:block_end_idx, block_end_idx:])

            # 3. the whole weight on the groups' grid
            qdq = qdq_per_channel_table(rounded_weight, table, 1, num_blocks_per_column, rows_per_block * num_cols)
            inner.weight.data = qdq.reshape(inner.weight.shape).to(inner.weight.dtype)

        # the weight holds already-quantized values: its quantizer stays off from here on
        quantizer.enabled = False
        module.__dict__["_gptvq_group_quantizer"] = group_quantizer
        hook = cls.record_hook
        if hook is not None:
            hook(module, {"codebooks": codebooks, "codebook_cols": codebook_cols, "indices": all_indices,
                          "table": table, "hessian_inv": hessian_inv, "group_quantizer": group_quantizer})

    @staticmethod
    def _sweep(w2d: torch.Tensor, rows_per_block: int, b0: int, s0: int, s1: int, block_end: int, vector_dim: int,
               codebook: torch.Tensor, hessian_inv: torch.Tensor, err: torch.Tensor, indices: torch.Tensor):
        """aimet_gptvq_block_update: steps [s0, s1) of the block [b0, block_end) of `w2d`, in place."""
        rows, cols = w2d.shape
        with torch.cuda.device(w2d.device):
            _native.call("aimet_gptvq_block_update", w2d.data_ptr(), cols, rows, rows_per_block, b0, s0, s1, block_end,
                         vector_dim, codebook.shape[1], codebook.data_ptr(), hessian_inv.data_ptr(),
                         hessian_inv.shape[1], err.data_ptr(), indices.data_ptr(), _stream(w2d))

    @staticmethod
    def _update_weight_block(weight_block: torch.Tensor, codebook: torch.Tensor, vector_dim: int,
                             num_blocks_per_column: int, inverse_hessian_diagonal: Optional[torch.Tensor] = None,
                             assignment_chunk_size: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        Update weight block using codebook (the torch form of one step of the sweep)

        :param weight_block: Weight block to be updated (num_rows x vector_dim)
        :param codebook: Codebook containing centroids
        :param vector_dim: Vector dimension
        :param num_blocks_per_column: Number of blocks per column
        :return: Updated weight block and corresponding indices
        """
        weight_block_shape = weight_block.shape
        sliced_weight = weight_block.reshape(num_blocks_per_column, -1, vector_dim)
        indices = get_assignments(sliced_weight, codebook, inverse_hessian_diagonal, assignment_chunk_size)
        centroids = torch.gather(codebook, dim=1, index=indices.unsqueeze(-1).expand(-1, -1, vector_dim))
        return centroids.reshape(weight_block_shape), indices

    @classmethod
    def compute_inverse(cls, hessian: torch.Tensor) -> torch.Tensor:
        """
        computes the inverse of the hessian matrix using the Cholesky decomposition: the upper Cholesky
        factor of the inverse, on the device of `hessian` (on the host when this torch build cannot
        factorise there)

        :param hessian: hessian for the module used to do weight update
        :returns the inverse of the passed hessian matrix
        """
        def factorise(h):
            h = torch.linalg.cholesky(h)
            h = torch.cholesky_inverse(h)
            return torch.linalg.cholesky(h, upper=True)

        if hessian.is_cuda and not cls.cholesky_on_host:
            try:
                return factorise(hessian)
            except torch.linalg.LinAlgError:
                raise
            except RuntimeError:
                cls.cholesky_on_host = True
        if hessian.is_cuda:
            return factorise(hessian.cpu()).to(hessian.device)
        return factorise(hessian)


# ---------------------------------------------------------------------------------------------------
# gptvq/gptvq_weight.py
# ---------------------------------------------------------------------------------------------------
# pylint: disable=protected-access, too-many-arguments
class GPTVQ:
    """
    Weight rounding mechanism for GPTVQ
    """
    @classmethod
    def apply_gptvq(cls, model: nn.Module, dummy_input: Union[torch.Tensor, Tuple], gptvq_params: GPTVQParameters,
                    param_encoding_path: str, module_names_to_exclude: Optional[List[str]] = None,
                    block_level_module_names: Optional[List[List[str]]] = None, file_name_prefix: str = "gptvq",
                    config_file_path: Optional[str] = None) -> nn.Module:
        """
        Returns model with optimized weight rounding of GPTVQ supportable modules
        and saves the corresponding parameter quantization encodings to a separate JSON file
        that can be imported by QuantizationSimModel for inference or QAT

        :param model: PyTorch model to GPTVQ
        :param dummy_input: Dummy input to the model. Used to parse model graph. If the model has more than one input,
                            pass a tuple. User is expected to place the tensors on the appropriate device
        :param gptvq_params: Dataclass holding GPTVQ parameters
        :param param_encoding_path: Path where to store parameter encodings
        :param module_names_to_exclude: Module names which are excluded during GPTVQ optimization
        :param block_level_module_names: List of module name lists to optimize block level GPTVQ optimization instead of leaf module level
        :param file_name_prefix: Prefix to use for filename of the encodings file
        :param config_file_path: Configuration file path for model quantizers
        :return: Model with GPTVQ applied weights and saves corresponding parameter encodings JSON file at provided path
        """
        _check_flags()
        if module_names_to_exclude is not None:
            cls._validate_module_names(model, module_names_to_exclude, "module_names_to_exclude")
        if block_level_module_names is not None:
            cls._validate_module_names(model, itertools.chain.from_iterable(block_level_module_names),
                                       "block_level_module_names")
        device = _device_of(model)
        if device.type != "cuda":
            raise RuntimeError("aimet_amd: GPTVQ needs the model on a HIP (cuda) device; the MI355X core has no "
                               "CPU path")

        module_name_set = cls._get_candidate_module_name_set(model, module_names_to_exclude)
        sim = cls._get_quantsim(model, dummy_input, gptvq_params, config_file_path, module_name_set)
        if module_names_to_exclude is None:
            module_names_to_exclude = []

        with cls._disable_quantizers_for_gptvq_optimization(sim, module_name_set):
            cls._apply_gptvq(model, sim, dummy_input, gptvq_params, set(module_names_to_exclude),
                             block_level_module_names)

        cls._export_encodings_to_json(param_encoding_path, file_name_prefix, sim, gptvq_params.rows_per_block)
        if isinstance(sim.model, QcQuantizeWrapper):
            return sim.model.get_original_module()
        QuantizationSimModel._remove_quantization_wrappers(sim.model, list(sim.model.modules()))
        return sim.model

    @staticmethod
    def _validate_module_names(model: nn.Module, module_names: Iterable[str], parameter_name: str):
        """
        Validate user provided parameter containing module names
        Each module should exist in the model and be a GPTVQ supportable module

        :param model: torch Model
        :param module_names: Iterable of module names
        :param parameter_name: Name of parameter to validate
        :raise ValueError: If module names are not valid
        """
        name_to_module = dict(model.named_modules())
        invalid_module_names = []
        for name in module_names:
            if name in name_to_module and isinstance(name_to_module[name], GPTVQSupportedModules):
                continue
            invalid_module_names.append(name)

        if invalid_module_names:
            msg = (f"Parameter `{parameter_name}` contains invalid module names ({', '.join(invalid_module_names)}) "
                   f"that don't exist in model or aren't GPTVQ supportable")
            raise ValueError(msg)

    @staticmethod
    def _get_candidate_module_name_set(model: nn.Module, module_names_to_exclude: Optional[List[str]]) -> Set[str]:
        """
        Return module name set considering module_names_to_exclude

        :param model: Original model
        :param module_names_to_exclude: Module names which are excluded during GPTVQ optimization
        :return: Module name set considering module_names_to_exclude
        """
        possible_module_names = {name for name, module in model.named_modules()
                                 if isinstance(module, GPTVQSupportedModules)}
        module_names_to_exclude = set(module_names_to_exclude) if module_names_to_exclude else set()
        return possible_module_names.difference(module_names_to_exclude)

    @classmethod
    def _get_quantsim(cls, model: nn.Module, dummy_input: Union[torch.Tensor, Tuple], gptvq_params: GPTVQParameters,
                      config_file_path: Optional[str], module_name_set: Set[str]) -> QuantizationSimModel:
        """
        Instantiate QuantizationSimModel object: TF scheme, `vector_bw`-bit parameters. The group
        quantizer of a candidate module is built from its weight quantizer's settings in weight_update.
        """
        sim = QuantizationSimModel(model, dummy_input=dummy_input, quant_scheme=QuantScheme.post_training_tf,
                                   default_param_bw=gptvq_params.vector_bw, config_file=config_file_path)
        name_to_module = dict(sim.model.named_modules())
        for name in module_name_set:
            module = name_to_module[name]
            assert isinstance(module, QcQuantizeWrapper), "%s is not a quantization wrapper" % name
            num_rows = _unwrap(module).weight.shape[0]
            assert num_rows % gptvq_params.rows_per_block == 0, \
                (f"The number of rows in weight (#: {num_rows}) should be divided by rows per block "
                 f"(#: {gptvq_params.rows_per_block})")
        return sim

    @staticmethod
    @contextlib.contextmanager
    def _disable_quantizers_for_gptvq_optimization(sim: QuantizationSimModel, module_name_set: Set[str]):
        """
        Disable temporarily every activation quantizer and every parameter quantizer that GPTVQ does not
        replace; a candidate's weight quantizer is off as well while GPTVQ runs (its settings make the
        group quantizer) and stays off once its weight is optimized.

        :param sim: QuantizationSimModel object
        :param module_name_set: Module name set containing candidates of GPTVQ optimization
        """
        restore = []
        for name, wrapper in sim.quant_wrappers():
            for quantizer in list(wrapper.input_quantizers) + list(wrapper.output_quantizers) + \
                    list(wrapper.param_quantizers.values()):
                if quantizer.enabled:
                    quantizer.enabled = False
                    restore.append((name, wrapper, quantizer))
        try:
            yield
        finally:
            for name, wrapper, quantizer in restore:
                optimized = "_gptvq_group_quantizer" in wrapper.__dict__ and \
                    quantizer is wrapper.param_quantizers.get("weight")
                if not optimized:
                    quantizer.enabled = True

    @classmethod
    def _get_block_level_module_names(cls, original_model: nn.Module, dummy_input: Union[torch.Tensor, Tuple],
                                      block_level_modules_names: Optional[List[List[str]]],
                                      module_names_to_exclude: Set[str]) -> List[List[str]]:
        """
        Return block level module name list

        :param original_model: Original torch model
        :param dummy_input: Dummy input
        :param block_level_modules_names: User provided block level module names
        :param module_names_to_exclude: Module names which are excluded during GPTVQ optimization
        :return: Block level module name list
        """
        ordered_module_names = [name for name, module in get_ordered_list_of_modules(original_model, dummy_input)
                                if isinstance(module, GPTVQSupportedModules) and name not in module_names_to_exclude]
        if block_level_modules_names:
            leaf_level_module_names = set(ordered_module_names).difference(
                set(itertools.chain.from_iterable(block_level_modules_names)))
            leaf_level_module_names = [[name] for name in leaf_level_module_names]

            name_to_index = {name: idx for idx, name in enumerate(ordered_module_names)}
            for module_block in block_level_modules_names:
                module_block.sort(key=lambda x: name_to_index.get(x, float("inf")))

            block_level_modules_names.extend(leaf_level_module_names)
            ordered_block_level_modules = sorted(block_level_modules_names,
                                                 key=lambda x: name_to_index.get(x[0], float("inf")))
        else:
            ordered_block_level_modules = [[name] for name in ordered_module_names]
        return ordered_block_level_modules

    @classmethod
    def _apply_gptvq(cls, original_model: nn.Module, sim: QuantizationSimModel,
                     dummy_input: Union[torch.Tensor, Tuple], gptvq_params: GPTVQParameters,
                     module_names_to_exclude: Set[str], block_level_module_names: Optional[List[List[str]]]):
        """
        Apply GPTVQ algorithm to optimize weights

        :param original_model: Original PyTorch model
        :param sim: QuantizationSimModel object to optimize weight
        :param dummy_input: Dummy input to model to be used to parse model graph
        :param gptvq_params: Dataclass holding GPTVQ parameters
        :param module_names_to_exclude: Module names which are excluded during GPTVQ optimization
        :param block_level_module_names: List of module name lists to optimize block level GPTVQ optimization instead of leaf module level
        """
        block_level_module_names = cls._get_block_level_module_names(original_model, dummy_input,
                                                                     block_level_module_names,
                                                                     module_names_to_exclude)
        for module_names in block_level_module_names:
            name_to_quant_module = cls._get_applicable_name_to_module_dict(module_names, sim, module_names_to_exclude)
            name_to_hessian = get_module_name_to_hessian_tensor(gptvq_params, sim, module_names)
            for name, quant_module in name_to_quant_module.items():
                assert isinstance(quant_module, QcQuantizeWrapper), "%s is not a quantization wrapper" % quant_module
                GPTVQOptimizer.weight_update(module=quant_module, gptvq_params=gptvq_params,
                                             hessian=name_to_hessian[name])

    @staticmethod
    def _get_applicable_name_to_module_dict(module_names: List[str], sim: QuantizationSimModel,
                                            module_names_to_exclude: Set[str]) -> Dict[str, QcQuantizeWrapper]:
        """
        Generate GPTVQ applicable name to module dictionary

        :param module_names: Module name list
        :param sim: QuantizationSimModel object
        :param module_names_to_exclude: Module names to exclude GPTVQ optimization
        :return: Module name to Quantization module dictionary
        """
        name_to_module = dict(sim.model.named_modules())
        name_to_quant_module = collections.OrderedDict()
        for name in module_names:
            if name not in module_names_to_exclude:
                name_to_quant_module[name] = name_to_module[name]
        return name_to_quant_module

    @classmethod
    def _export_encodings_to_json(cls, path: str, filename_prefix: str, sim: QuantizationSimModel,
                                  rows_per_block: int):
        """
        Save GPTVQ applied parameter encodings to JSON file

        :param path: path where to store param encodings
        :param filename_prefix: filename to store exported weight encodings in JSON format
        :param sim: QuantizationSimModel object
        :param rows_per_block: The number of rows per block
        """
        param_encodings = {}
        for name, wrapper in sim.quant_wrappers():
            if "_gptvq_group_quantizer" in wrapper.__dict__:
                cls._update_param_encodings_dict(wrapper, name, param_encodings, rows_per_block)

        encoding = {"param_encodings": param_encodings}
        os.makedirs(os.path.abspath(path), exist_ok=True)
        encoding_file_path = os.path.join(path, f"{filename_prefix}.encodings")
        with open(encoding_file_path, "w") as encoding_fp:
            json.dump(encoding, encoding_fp, sort_keys=True, indent=4)

    @staticmethod
    def _update_param_encodings_dict(quant_module: QcQuantizeWrapper, name: str, param_encodings: Dict,
                                     rows_per_block: int):
        """
        Update block level encodings to per-channel encodings: each group's encoding `rows_per_block` times

        :param quant_module: quant module
        :param name: name of module
        :param param_encodings: Dictionary of param encodings
        :param rows_per_block: The number of rows per block
        """
        group_quantizer = quant_module.__dict__["_gptvq_group_quantizer"]
        per_channel_encodings = []
        for encoding in group_quantizer.encoding:
            entry = create_encoding_dict(encoding, group_quantizer, False)
            per_channel_encodings.extend([dict(entry) for _ in range(rows_per_block)])
        param_encodings[f"{name}.weight"] = per_channel_encodings


apply_gptvq = GPTVQ.apply_gptvq
