"""PyTorch's transformer modules in a form QuantizationSimModel can simulate
(aimet_torch/transformers/activation.py and utils.py, aimet_torch/model_preparer.py:694).

Inside an nn.MultiheadAttention the sim finds one wrappable child (out_proj), and
F.multi_head_attention_forward never calls it; an eval-mode batch_first nn.TransformerEncoderLayer
skips even its feed-forward children on torch's fused fast path. QuantizableMultiheadAttention spells
the block out in children -- linear_Q / linear_K / linear_V / div / matmul_1 / softmax / matmul_2 /
out_proj -- which a sim built with aimet_amd.elementwise_ops.TRANSFORMER_QUANTIZABLE_TYPES wraps like any
other layer (quant_wrappers() lists them, so AdaRound, SeqMSE, bias correction and the analyzer see
them). It sets _qkv_same_embed_dim = False and holds no in_proj_weight / in_proj_bias, so the fast
paths of nn.TransformerEncoderLayer and nn.TransformerEncoder refuse themselves.

    get_quantizable_pt_transformer_model(model)          # in place: MHAs and functional activations
    sim = QuantizationSimModel(model, dummy_input, quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)

Two routes compute the attention probabilities (the same arithmetic but for the last bits of the
exponential: the kernel's is written out in float32 operations, the literal route's is torch's):

  * fused: one raw bmm q k^T, then ONE aimet_attn_softmax launch (csrc/attn_softmax.hip) that applies
    matmul_1's output quantizer, both masks, the softmax and softmax's output quantizer while each row
    of the [B H, L, S] tensor stays on chip. Taken when matmul_1 and softmax are static-grid wrappers
    whose forward is nothing but a per-tensor integer output quantizer rounding to nearest
    (StaticGridQuantWrapper.output_fusable), the tensors are float32 on the GPU, no operand needs a
    gradient, and S <= aimet_attn_softmax_max_s(). In ANALYSIS mode the raw scores and the kernel's
    unquantized probabilities go to the two quantizers' statistics through the wrappers themselves.
  * literal: the children called one by one. Everything else -- range learning without the opt-in
    below, per-channel or disabled learned quantizers, 16-bit or CPU
    tensors, float data types, stochastic rounding, enabled input quantizers, an unwrapped module,
    longer rows -- and `module.fused = False`.
  * fused with a gradient (opt-in, `module.fused_backward = True` or set_fused_attention_backward(model)):
    the fused route also when q or k needs a gradient, through AttnSoftmax. Its forward is the same
    launch, out of place, and keeps the raw scores alone for the way back; its backward is ONE
    aimet_attn_softmax_backward launch that recomputes each row on chip and applies both
    straight-through masks, the softmax backward and the mask fills (the literal route keeps the raw
    scores, the softmax output and the unquantized probabilities, and runs an STE kernel, torch's
    softmax backward, the mask-fill backwards and a second STE kernel). Static-grid wrappers only: the
    gradient of a calibrated sim, STE QAT with the post_training_* schemes. The gradients of the two
    routes differ by float32 rounding and, where exp_r and torch's exponential put a probability on
    neighbouring levels, by one level of softmax's quantizer. Measured against the literal route in
    DESIGN section 5.
  * fused core (opt-in, `module.fused_core = True` or set_fused_attention_core(model)): ONE aimet_attn_core
    launch (csrc/attn_core.hip) computes q k^T, matmul_1's output quantizer, the masks, the softmax,
    softmax's output quantizer, the product with v and matmul_2's output quantizer on the fp32 matrix
    cores, and the [B H, L, S] scores and probabilities never reach memory: rows of any length, where
    the fused route stops at aimet_attn_softmax_max_s() and the literal route needs several tensors of
    that size. Taken when need_weights is false, dropout is inactive, no gradient is wanted, matmul_1,
    softmax and matmul_2 are static-grid wrappers with output_fusable() in ACTIVE or PASSTHROUGH mode
    (ANALYSIS needs the score statistics), the tensors are float32 on one GPU and head_dim is 32, 64 or
    128; otherwise the route is chosen as without it. The score product is computed twice, and below
    aimet_attn_softmax_max_s() this route is not faster than the fused one; nothing
    switches automatically. Its probabilities are those of the fused route but for the order of the
    row sum.
  * fused, range learning (the same opt-in; without it range-learning wrappers take the literal route
    with or without a gradient): matmul_1 and softmax are LearnedGridQuantWrappers whose forward is
    nothing but one enabled per-tensor integer output quantizer (LearnedGridQuantWrapper.output_fusable).
    Each wrapper's gate runs first, then AttnSoftmaxLearned: ONE aimet_attn_softmax_lg launch that reads
    the four trainable range ends on the device (nothing comes back to the host), computes delta and
    offset as the learned-grid kernels do, rounds half to even and keeps the raw scores and eight floats
    of encodings; going back, ONE aimet_attn_softmax_lg_backward row launch recomputes each row, writes
    the score gradient and carries the six sums of the two quantizers' range gradients, which a
    one-workgroup second launch folds in a fixed order into d/d encoding_min and d/d encoding_max of
    both (no atomics: equal inputs give equal bits). The literal route runs a learned-grid forward, the
    mask fills, torch's softmax and a second learned-grid forward, and their four backwards, over four
    saved tensors of the score's size.

Masks: bool (or, deprecated, uint8) attn_mask of [L, S] or [B H, L, S] and key_padding_mask of [B, S],
True = not attended. nn.TransformerEncoderLayer / DecoderLayer hand their masks on as float tensors
of 0 and -inf (F._canonical_mask); such a mask is accepted and used as its bool form, after one check
per mask tensor that costs a read-back (cached while the tensor lives unmodified; not possible during
stream capture).

Differs from the reference:
  * There is no `mask_add` child and a float mask with other values than 0 and -inf raises
    NotImplementedError: the reference computes mask_add(scores, mask) and discards the result
    (activation.py:411), so it offers no behaviour to match.
  * add_zero_attn allocates its zeros on the input's device and in its dtype (the reference allocates
    float32 on the CPU).
  * batch_first: the reference views the [B H, L, head_dim] attention output as [B, L, E] without
    moving the head axis, which mixes heads and positions whenever there is more than one head; here
    the output is what nn.MultiheadAttention(batch_first=True) computes.
  * create_quantizable_multihead_attention on a module with bias_k / bias_v copies them into the new
    module's bias_k / bias_v and takes the linear biases from in_proj_bias; the reference copies bias_k
    ([1, 1, E]) into linear_K.bias ([E]), which torch refuses, and leaves the new bias_k at its random
    initial value.
  * The new module is created on the source's device, in its dtype and training mode.
"""
import copy
import ctypes
import warnings
import weakref
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from aimet_amd import _native
from aimet_amd.elementwise_ops import Add, Divide, MatMul
from aimet_amd.qc_quantize_op import LearnedGridQuantWrapper, QcQuantizeOpMode, StaticGridQuantWrapper

_NEG_INF = float("-inf")


# ---- the fused launch ----------------------------------------------------------------------------
def attn_softmax_max_s() -> int:
    """The longest row aimet_attn_softmax keeps on chip."""
    return int(_native.load().aimet_attn_softmax_max_s())


def attn_launch_count(reset: bool = False) -> int:
    """aimet_attn_softmax launches issued in this process."""
    n = ctypes.c_int64(0)
    _native.call("aimet_attn_launch_count", ctypes.byref(n), int(reset))
    return n.value


def attn_backward_launch_count(reset: bool = False) -> int:
    """aimet_attn_softmax_backward launches issued in this process."""
    n = ctypes.c_int64(0)
    _native.call("aimet_attn_backward_launch_count", ctypes.byref(n), int(reset))
    return n.value


def _encoding_c(enc):
    """A TfEncoding, or (min, max, bitwidth) -> the C struct (delta and offset are recomputed from the
    three, as aimet_qdq_per_tensor does); a C struct is handed on."""
    if enc is None or isinstance(enc, _native.TfEncodingC):
        return enc
    if isinstance(enc, (tuple, list)):
        return _native.TfEncodingC(float(enc[0]), float(enc[1]), 0.0, 0.0, int(enc[2]))
    return _native.TfEncodingC(enc.min, enc.max, enc.delta, enc.offset, enc.bw)


def _mask_bytes(mask, shape, device, what, fn):
    if mask is None:
        return None
    if mask.dtype != torch.bool or tuple(mask.shape) != tuple(shape) or mask.device != device:
        raise ValueError(fn + ": %s must be a bool tensor of shape %s on %s, got %s %s on %s"
                         % (what, tuple(shape), device, mask.dtype, tuple(mask.shape), mask.device))
    return mask.contiguous().view(torch.uint8)


def _launch_args(fn, scores, batch, num_heads, attn_mask, key_padding_mask, score_enc, prob_enc, others):
    """The checks attn_softmax and attn_softmax_backward share -> (the arguments after the float tensors,
    the objects they point into). `fn` names the caller in the errors; `others`: name -> the float
    tensors that must match scores (None: a new one)."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 3 and scores.is_contiguous()):
        raise ValueError(fn + ": scores must be a contiguous float32 [B H, L, S] tensor on the GPU")
    BH, L, S = scores.shape
    if BH != batch * num_heads:
        raise ValueError(fn + ": scores has %d matrices, batch * num_heads is %d" % (BH, batch * num_heads))
    for name, t in others.items():
        if t is None:
            others[name] = torch.empty_like(scores)
        elif not (t.is_cuda and t.dtype == torch.float32 and t.shape == scores.shape and t.is_contiguous() and
                  t.device == scores.device):
            raise ValueError(fn + ": %s must match scores" % name)
    per_bh = attn_mask is not None and attn_mask.dim() == 3
    am = _mask_bytes(attn_mask, (BH, L, S) if per_bh else (L, S), scores.device, "attn_mask", fn)
    kpm = _mask_bytes(key_padding_mask, (batch, S), scores.device, "key_padding_mask", fn)
    s_enc, p_enc = _encoding_c(score_enc), _encoding_c(prob_enc)
    args = (batch, num_heads, L, S, am.data_ptr() if am is not None else None, int(per_bh),
            kpm.data_ptr() if kpm is not None else None, ctypes.byref(s_enc) if s_enc is not None else None,
            ctypes.byref(p_enc) if p_enc is not None else None)
    return args, (am, kpm, s_enc, p_enc)


def attn_softmax(scores: Tensor, batch: int, num_heads: int, attn_mask: Optional[Tensor] = None,
                 key_padding_mask: Optional[Tensor] = None, score_enc=None, prob_enc=None,
                 out: Optional[Tensor] = None) -> Tensor:
    """One aimet_attn_softmax launch on scores [batch * num_heads, L, S] (float32, contiguous, GPU):
    QDQ(score_enc), masks (attn_mask [L, S] or [batch * num_heads, L, S], key_padding_mask
    [batch, S]; bool, True = -inf), softmax, QDQ(prob_enc). Encodings: TfEncoding, (min, max, bw) or
    None. `out` may be `scores`. There is no other implementation behind this function."""
    others = {"out": out}
    args, _alive = _launch_args("attn_softmax", scores, batch, num_heads, attn_mask, key_padding_mask, score_enc,
                                prob_enc, others)
    with torch.cuda.device(scores.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _native.call("aimet_attn_softmax", scores.data_ptr(), others["out"].data_ptr(), *args, stream)
    return others["out"]


def attn_softmax_backward(scores: Tensor, grad_probs: Tensor, batch: int, num_heads: int,
                          attn_mask: Optional[Tensor] = None, key_padding_mask: Optional[Tensor] = None,
                          score_enc=None, prob_enc=None, out: Optional[Tensor] = None) -> Tensor:
    """One aimet_attn_softmax_backward launch: the gradient at the raw `scores` that attn_softmax read,
    from `grad_probs`, the gradient at what it returned (masks and encodings as given to attn_softmax;
    the encodings act as straight-through masks on the raw score and on the unquantized probability,
    a masked position gets exactly 0). `out` may be `grad_probs`. There is no other implementation
    behind this function."""
    if grad_probs is None:
        raise ValueError("attn_softmax_backward: grad_probs must match scores")
    others = {"grad_probs": grad_probs, "out": out}
    args, _alive = _launch_args("attn_softmax_backward", scores, batch, num_heads, attn_mask, key_padding_mask,
                                score_enc, prob_enc, others)
    with torch.cuda.device(scores.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _native.call("aimet_attn_softmax_backward", scores.data_ptr(), grad_probs.data_ptr(),
                     others["out"].data_ptr(), *args, stream)
    return others["out"]


class AttnSoftmax(torch.autograd.Function):
    """attn_softmax with a gradient for `scores`: apply(scores, batch, num_heads, attn_mask,
    key_padding_mask, score_enc, prob_enc). The forward is one out-of-place launch and saves the raw
    scores; the encodings are copied at the forward, so the backward sees the grid the forward used.
    The masks are saved beside the scores (no copy), so autograd refuses the backward if scores or a
    mask was written in place after the forward. Differentiable once: the backward is a launch autograd
    does not see into, and a second derivative raises."""

    @staticmethod
    def forward(ctx, scores, batch, num_heads, attn_mask, key_padding_mask, score_enc, prob_enc):
        ctx.args = (batch, num_heads, _encoding_c(score_enc), _encoding_c(prob_enc))
        ctx.save_for_backward(scores, attn_mask, key_padding_mask)
        return attn_softmax(scores, batch, num_heads, attn_mask, key_padding_mask, *ctx.args[2:])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_probs):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        scores, attn_mask, key_padding_mask = ctx.saved_tensors
        batch, num_heads, score_enc, prob_enc = ctx.args
        return (attn_softmax_backward(scores, grad_probs.contiguous(), batch, num_heads, attn_mask, key_padding_mask,
                                      score_enc, prob_enc),) + (None,) * 6


# ---- the attention core: no score tensor ------------------------------------------------------------
ATTN_CORE_HEAD_DIMS = (32, 64, 128)   # the instantiations of csrc/attn_core.hip


def attn_core_launch_count(reset: bool = False) -> int:
    """aimet_attn_core launches issued in this process."""
    n = ctypes.c_int64(0)
    _native.call("aimet_attn_core_launch_count", ctypes.byref(n), int(reset))
    return n.value


def _extent(t: Tensor) -> Tuple[int, int]:
    """[first byte, one past the last byte) that the view `t` can touch."""
    last = sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()


def attn_core(q: Tensor, k: Tensor, v: Tensor, batch: int, num_heads: int, attn_mask: Optional[Tensor] = None,
              key_padding_mask: Optional[Tensor] = None, score_enc=None, prob_enc=None, out_enc=None,
              out: Optional[Tensor] = None) -> Tensor:
    """One aimet_attn_core launch (csrc/attn_core.hip): for q [batch * num_heads, L, D] and k, v
    [batch * num_heads, S, D] (float32, GPU; transposed views with D contiguous are read in place),
    out = QDQ(out_enc)( QDQ(prob_enc)( softmax( mask( QDQ(score_enc)(q k^T) ) ) ) v ) as a contiguous
    [batch * num_heads, L, D] tensor, without the [.., L, S] scores or probabilities ever reaching memory.
    Masks and encodings as attn_softmax takes them; D must be one of ATTN_CORE_HEAD_DIMS; S is not
    bounded. `out` must not overlap an input. There is no other implementation behind this function.

    The score product is computed twice (3 * 2 * B H L S D matrix FLOPs) and the exponential of every
    element twice; DESIGN section 5 has it measured against the route that keeps the scores in memory:
    where that route can run (S <= attn_softmax_max_s()) this one is not faster (0.91 of its speed at
    L = S = 2048, not told apart at a ViT-L block), and it is the only fused one beyond. Nothing switches
    between the routes automatically."""
    fn = "attn_core"
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not (isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
            raise ValueError(fn + ": %s must be a float32 [B H, rows, D] tensor on the GPU" % name)
    BH, L, D = q.shape
    S = k.shape[1]
    if BH != batch * num_heads:
        raise ValueError(fn + ": q has %d matrices, batch * num_heads is %d" % (BH, batch * num_heads))
    if tuple(k.shape) != (BH, S, D) or tuple(v.shape) != (BH, S, D) or k.device != q.device or v.device != q.device:
        raise ValueError(fn + ": k and v must be [%d, S, %d] tensors on %s" % (BH, D, q.device))
    if D not in ATTN_CORE_HEAD_DIMS:
        raise ValueError(fn + ": head_dim %d is not supported (%s)" % (D, ", ".join(map(str, ATTN_CORE_HEAD_DIMS))))
    if L == 0 or S == 0 or BH == 0:
        raise ValueError(fn + ": empty q, k or v")
    if out is None:
        out = torch.empty((BH, L, D), dtype=torch.float32, device=q.device)
    elif not (isinstance(out, Tensor) and out.is_cuda and out.dtype == torch.float32 and out.device == q.device and
              tuple(out.shape) == (BH, L, D) and out.is_contiguous()):
        raise ValueError(fn + ": out must be a contiguous float32 [%d, %d, %d] tensor on %s" % (BH, L, D, q.device))
    lo, hi = _extent(out)
    for name, t in (("q", q), ("k", k), ("v", v)):
        t_lo, t_hi = _extent(t)
        if t_lo < hi and lo < t_hi:
            raise ValueError(fn + ": out must not overlap %s" % name)

    def operand(t):   # what the kernel's 16-byte loads need; anything else is copied once
        ok = t.stride(2) == 1 and t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0 and t.stride(1) >= D and \
            t.data_ptr() % 16 == 0
        return t if ok else t.clone(memory_format=torch.contiguous_format)

    q, k, v = operand(q), operand(k), operand(v)
    per_bh = attn_mask is not None and attn_mask.dim() == 3
    am = _mask_bytes(attn_mask, (BH, L, S) if per_bh else (L, S), q.device, "attn_mask", fn)
    kpm = _mask_bytes(key_padding_mask, (batch, S), q.device, "key_padding_mask", fn)
    encs = [_encoding_c(e) for e in (score_enc, prob_enc, out_enc)]
    with torch.cuda.device(q.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _native.call("aimet_attn_core", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), batch, num_heads, L,
                     S, D, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                     am.data_ptr() if am is not None else None, int(per_bh),
                     kpm.data_ptr() if kpm is not None else None,
                     *[ctypes.byref(e) if e is not None else None for e in encs], stream)
    return out


# ---- the fused launches on learned grids (range learning) ------------------------------------------
def attn_lg_launch_count(reset: bool = False) -> Tuple[int, int]:
    """(aimet_attn_softmax_lg launches, aimet_attn_softmax_lg_backward row launches) issued in this
    process; the backward's fold launch is not counted."""
    fwd, bwd = ctypes.c_int64(0), ctypes.c_int64(0)
    _native.call("aimet_attn_lg_launch_count", ctypes.byref(fwd), ctypes.byref(bwd), int(reset))
    return fwd.value, bwd.value


def _lg_grid_c(fn, grid, device, with_range):
    """(encoding_min, encoding_max, bitwidth, use_symmetric, use_strict_symmetric, is_unsigned_symmetric)
    -> aimet_attn_lg_grid; None stays None. The range is handed over by address: the kernel reads it."""
    if grid is None:
        return None
    emin, emax, bw, sym, strict, unsigned = grid
    if bw >= 32:
        raise RuntimeError("Invalid bitwidth: %d" % bw)
    ptrs = (None, None)
    if with_range:
        for name, r in (("encoding_min", emin), ("encoding_max", emax)):
            if not (isinstance(r, Tensor) and r.is_cuda and r.device == device and r.dtype == torch.float32 and
                    r.numel() == 1):
                raise ValueError(fn + ": %s must be one float32 element on %s" % (name, device))
        ptrs = (emin.data_ptr(), emax.data_ptr())
    return _native.AttnLgGridC(*ptrs, int(bw), int(bool(sym)), int(bool(strict)), int(bool(unsigned)))


def _ref(struct):
    return ctypes.byref(struct) if struct is not None else None


def attn_softmax_lg(scores: Tensor, batch: int, num_heads: int, attn_mask: Optional[Tensor] = None,
                    key_padding_mask: Optional[Tensor] = None, score_grid=None, prob_grid=None,
                    out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """One aimet_attn_softmax_lg launch: attn_softmax with both quantizers on learned grids
    (calculate_forward_pass). A grid is (encoding_min, encoding_max, bitwidth, use_symmetric,
    use_strict_symmetric, is_unsigned_symmetric) with the range as two one-element float32 GPU tensors,
    which the kernel reads (nothing comes back to the host), or None for no quantizer. Out of place.
    Returns (probs, saved): saved [2, 4] holds {delta, offset, min, max} of the score grid (row 0) and
    of the prob grid (row 1) as the kernel computed and read them, for attn_softmax_lg_backward; a row
    without a quantizer is not written. There is no other implementation behind this function."""
    others = {"out": out}
    args, _alive = _launch_args("attn_softmax_lg", scores, batch, num_heads, attn_mask, key_padding_mask, None, None,
                                others)
    sg = _lg_grid_c("attn_softmax_lg", score_grid, scores.device, True)
    pg = _lg_grid_c("attn_softmax_lg", prob_grid, scores.device, True)
    saved = torch.empty((2, 4), dtype=torch.float32, device=scores.device)
    with torch.cuda.device(scores.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _native.call("aimet_attn_softmax_lg", scores.data_ptr(), others["out"].data_ptr(), *args[:-2], _ref(sg),
                     saved[0].data_ptr(), _ref(pg), saved[1].data_ptr(), stream)
    return others["out"], saved


def attn_softmax_lg_backward(scores: Tensor, grad_probs: Tensor, batch: int, num_heads: int,
                             attn_mask: Optional[Tensor] = None, key_padding_mask: Optional[Tensor] = None,
                             score_grid=None, prob_grid=None, saved: Optional[Tensor] = None,
                             out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """aimet_attn_softmax_lg_backward (the row launch and its fold): from the raw `scores`,
    `grad_probs` and what attn_softmax_lg saved, (grad_scores, range_grads): range_grads [2, 2] holds
    (d/d encoding_min, d/d encoding_max) of the score grid (row 0) and of the prob grid (row 1); a row
    without a quantizer is not written. Of a grid only the bitwidth and the flags are read here.
    `out` may be `grad_probs`. There is no other implementation behind this function."""
    if grad_probs is None:
        raise ValueError("attn_softmax_lg_backward: grad_probs must match scores")
    others = {"grad_probs": grad_probs, "out": out}
    args, _alive = _launch_args("attn_softmax_lg_backward", scores, batch, num_heads, attn_mask, key_padding_mask,
                                None, None, others)
    if not (isinstance(saved, Tensor) and saved.shape == (2, 4) and saved.dtype == torch.float32 and
            saved.device == scores.device and saved.is_contiguous()):
        raise ValueError("attn_softmax_lg_backward: saved must be the [2, 4] float32 tensor attn_softmax_lg returned")
    sg = _lg_grid_c("attn_softmax_lg_backward", score_grid, scores.device, False)
    pg = _lg_grid_c("attn_softmax_lg_backward", prob_grid, scores.device, False)
    grads = torch.empty((2, 2), dtype=torch.float32, device=scores.device)
    with torch.cuda.device(scores.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _native.call("aimet_attn_softmax_lg_backward", scores.data_ptr(), grad_probs.data_ptr(),
                     others["out"].data_ptr(), *args[:-2], _ref(sg), saved[0].data_ptr(), grads[0].data_ptr(),
                     _ref(pg), saved[1].data_ptr(), grads[1].data_ptr(), stream)
    return others["out"], grads


class AttnSoftmaxLearned(torch.autograd.Function):
    """attn_softmax_lg with gradients for `scores` and for the four range ends: apply(scores, batch,
    num_heads, attn_mask, key_padding_mask, score_min, score_max, score_flags, prob_min, prob_max,
    prob_flags), flags = (bitwidth, use_symmetric, use_strict_symmetric, is_unsigned_symmetric), a None
    range = no quantizer. The forward saves the raw scores, the masks and the eight floats of the two
    encodings as the kernel read them (the range parameters may change before the backward: the
    wrapper's gate writes them in place on every call). Differentiable once."""

    @staticmethod
    def forward(ctx, scores, batch, num_heads, attn_mask, key_padding_mask, score_min, score_max, score_flags,
                prob_min, prob_max, prob_flags):
        grids = tuple(None if lo is None else (lo.detach(), hi.detach()) + tuple(flags)
                      for lo, hi, flags in ((score_min, score_max, score_flags), (prob_min, prob_max, prob_flags)))
        probs, saved = attn_softmax_lg(scores, batch, num_heads, attn_mask, key_padding_mask, *grids)
        ctx.args = (batch, num_heads) + tuple(None if g is None else (None, None) + g[2:] for g in grids)
        ctx.shapes = tuple(None if r is None else r.shape for r in (score_min, score_max, prob_min, prob_max))
        ctx.save_for_backward(scores, attn_mask, key_padding_mask, saved)
        return probs

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_probs):
        need = ctx.needs_input_grad
        if not any(need):
            return (None,) * 11
        scores, attn_mask, key_padding_mask, saved = ctx.saved_tensors
        batch, num_heads, score_grid, prob_grid = ctx.args
        dx, grads = attn_softmax_lg_backward(scores, grad_probs.contiguous(), batch, num_heads, attn_mask,
                                             key_padding_mask, score_grid, prob_grid, saved)
        flat = grads.view(-1)
        rg = [flat[i:i + 1].view(ctx.shapes[i]) if need[pos] else None for i, pos in enumerate((5, 6, 8, 9))]
        return (dx if need[0] else None, None, None, None, None, rg[0], rg[1], None, rg[2], rg[3], None)


# ---- masks ---------------------------------------------------------------------------------------
_FLOAT_MASK_CHECKED = {}   # (address, version, shape, dtype) -> weak reference to the checked tensor
float_mask_checks = 0      # read-backs made so far (the tests watch it)


def _bool_mask(mask: Optional[Tensor], what: str) -> Optional[Tensor]:
    """`mask` in its bool form (True = not attended)."""
    global float_mask_checks
    if mask is None or mask.dtype == torch.bool:
        return mask
    if mask.dtype == torch.uint8:
        warnings.warn("Byte tensor for %s is deprecated. Use a bool tensor instead." % what)
        return mask.to(torch.bool)
    if not mask.is_floating_point():
        raise TypeError("Only float, byte and bool types are supported for %s, not %s" % (what, mask.dtype))
    masked = mask == _NEG_INF
    key = (mask.data_ptr(), mask._version, tuple(mask.shape), mask.dtype)
    ref = _FLOAT_MASK_CHECKED.get(key)
    if ref is None or ref() is not mask:
        if mask.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("QuantizableMultiheadAttention: the float %s has not been checked yet (every entry "
                               "must be 0 or -inf), and the check reads a value back from the device, which a "
                               "stream capture does not allow; run one forward with this mask tensor before the "
                               "capture, or pass a bool mask" % what)
        float_mask_checks += 1
        if not bool((masked | (mask == 0)).all()):
            raise NotImplementedError(
                "QuantizableMultiheadAttention: a float %s with entries other than 0 and -inf (an additive mask) is "
                "not supported. The reference computes mask_add(scores, mask) and discards the result "
                "(aimet_torch/transformers/activation.py:411), so it offers no behaviour to match. Pass a bool "
                "mask, or a float mask of 0 and -inf." % what)
        if len(_FLOAT_MASK_CHECKED) >= 256:
            for k in [k for k, r in _FLOAT_MASK_CHECKED.items() if r() is None]:
                del _FLOAT_MASK_CHECKED[k]
            if len(_FLOAT_MASK_CHECKED) >= 256:
                _FLOAT_MASK_CHECKED.clear()
        _FLOAT_MASK_CHECKED[key] = weakref.ref(mask)
    return masked


def _pad_column(mask: Optional[Tensor]) -> Optional[Tensor]:
    """One more key that is never masked (bias_k / bias_v, add_zero_attn)."""
    return None if mask is None else F.pad(mask, (0, 1))


# ---- the module ----------------------------------------------------------------------------------
class QuantizableMultiheadAttention(nn.MultiheadAttention):
    """nn.MultiheadAttention with every operation a child module (see the module docstring)."""
    _FLOAT_MODULE = nn.MultiheadAttention

    def __init__(self, embed_dim: int, num_heads: int, dropout: float = 0.0, bias: bool = True,
                 add_bias_kv: bool = False, add_zero_attn: bool = False, kdim: Optional[int] = None,
                 vdim: Optional[int] = None, batch_first: bool = False, device=None, dtype=None) -> None:
        kw = {"device": device, "dtype": dtype}
        super().__init__(embed_dim, num_heads, dropout, bias, add_bias_kv, add_zero_attn, kdim, vdim, batch_first,
                         **kw)
        # the packed projection is replaced by three linears; without it (and with the flag below)
        # torch's encoder fast paths, which read in_proj_weight directly, do not apply
        for name in ("in_proj_weight", "in_proj_bias", "q_proj_weight", "k_proj_weight", "v_proj_weight"):
            setattr(self, name, None)
        self._qkv_same_embed_dim = False
        self.linear_Q = nn.Linear(self.embed_dim, self.embed_dim, bias=bias, **kw)
        self.linear_K = nn.Linear(self.kdim, self.embed_dim, bias=bias, **kw)
        self.linear_V = nn.Linear(self.vdim, self.embed_dim, bias=bias, **kw)
        self.out_proj = nn.Linear(self.embed_dim, self.embed_dim, bias=bias, **kw)
        self.div = Divide()
        self.matmul_1 = MatMul()
        self.matmul_2 = MatMul()
        self.softmax = nn.Softmax(dim=-1)
        self.fused = True
        # The fused route also where a gradient is wanted (static-grid wrappers; module docstring).
        # Opt-in. DESIGN section 5 has the training step measured against the literal route. While it is
        # on, a forward that wants no gradient (no_grad, evaluation between steps) also goes through
        # AttnSoftmax: out of place, one more score-size tensor than the in-place launch; turn it off
        # for evaluation where that matters.
        self.fused_backward = False
        # The whole attention core in one launch that keeps scores and probabilities on chip (attn_core;
        # module docstring). Opt-in: evaluation only, and not faster than the fused route where that one runs.
        self.fused_core = False

    def _get_name(self):
        return "QuantizableMultiheadAttention"

    # pylint: disable=arguments-differ
    def forward(self, query: Tensor, key: Tensor, value: Tensor, key_padding_mask: Optional[Tensor] = None,
                need_weights: bool = True, attn_mask: Optional[Tensor] = None, average_attn_weights: bool = True,
                is_causal: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
        """As nn.MultiheadAttention.forward for batched input. `is_causal` is a hint torch gives
        alongside the mask itself; the mask is what is applied."""
        if query.dim() != 3:
            raise ValueError("QuantizableMultiheadAttention needs batched (3-D) query, key and value")
        if self.batch_first:
            query, key, value = (t.transpose(0, 1) for t in (query, key, value))
        tgt_len, bsz, embed_dim = query.shape
        if embed_dim != self.embed_dim:
            raise ValueError("query has embedding size %d, the module %d" % (embed_dim, self.embed_dim))
        if key.shape[:2] != value.shape[:2]:
            raise ValueError("key %s and value %s disagree in length or batch" % (tuple(key.shape), tuple(value.shape)))
        heads, head_dim = self.num_heads, self.embed_dim // self.num_heads
        src_len = key.shape[0]

        attn_mask = _bool_mask(attn_mask, "attn_mask")
        if attn_mask is not None:
            if attn_mask.dim() == 2:
                if tuple(attn_mask.shape) != (tgt_len, src_len):
                    raise RuntimeError("The size of the 2D attn_mask is not correct.")
                attn_mask = attn_mask.unsqueeze(0)
            elif attn_mask.dim() == 3:
                if tuple(attn_mask.shape) != (bsz * heads, tgt_len, src_len):
                    raise RuntimeError("The size of the 3D attn_mask is not correct.")
            else:
                raise RuntimeError("attn_mask's dimension %d is not supported" % attn_mask.dim())
        key_padding_mask = _bool_mask(key_padding_mask, "key_padding_mask")
        if key_padding_mask is not None and tuple(key_padding_mask.shape) != (bsz, src_len):
            raise RuntimeError("key_padding_mask must be of shape (%d, %d)" % (bsz, src_len))

        k = self.linear_K(key)
        v = self.linear_V(value)
        q = self.div(self.linear_Q(query), float(head_dim) ** 0.5)
        if self.bias_k is not None and self.bias_v is not None:
            k = torch.cat([k, self.bias_k.repeat(1, bsz, 1)])
            v = torch.cat([v, self.bias_v.repeat(1, bsz, 1)])
            attn_mask, key_padding_mask = _pad_column(attn_mask), _pad_column(key_padding_mask)
        q = q.contiguous().view(tgt_len, bsz * heads, head_dim).transpose(0, 1)
        k = k.contiguous().view(-1, bsz * heads, head_dim).transpose(0, 1)
        v = v.contiguous().view(-1, bsz * heads, head_dim).transpose(0, 1)
        if self.add_zero_attn:
            zeros = k.new_zeros((bsz * heads, 1, head_dim))
            k, v = torch.cat([k, zeros], dim=1), torch.cat([v, zeros.to(v.dtype)], dim=1)
            attn_mask, key_padding_mask = _pad_column(attn_mask), _pad_column(key_padding_mask)
        src_len = k.shape[1]

        if self._core_route(q, k, v, need_weights):
            probs = None
            out = self._core_out(q, k, v, bsz, attn_mask, key_padding_mask)
        else:
            if self._fused_route(q, k, src_len):
                probs = self._fused_probs(q, k, bsz, attn_mask, key_padding_mask)
            else:
                probs = self._literal_probs(q, k, bsz, attn_mask, key_padding_mask)
            probs = F.dropout(probs, p=self.dropout, training=self.training)   # after softmax's quantizer
            out = self.matmul_2(probs, v)                                      # [B H, L, head_dim]
        out = out.transpose(0, 1).contiguous().view(tgt_len, bsz, self.embed_dim)
        out = self.out_proj(out)
        if self.batch_first:
            out = out.transpose(0, 1)
        if not need_weights:
            return out, None
        probs = probs.view(bsz, heads, tgt_len, src_len)
        return out, (probs.mean(dim=1) if average_attn_weights else probs)

    # -- the attention core in one launch ------------------------------------------------------------
    def _core_route(self, q: Tensor, k: Tensor, v: Tensor, need_weights: bool) -> bool:
        if not getattr(self, "fused_core", False) or need_weights:
            return False
        if self.dropout > 0.0 and self.training:
            return False
        if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
            return False
        wrappers = (self.matmul_1, self.softmax, self.matmul_2)
        if not all(isinstance(w, StaticGridQuantWrapper) and w.output_fusable() for w in wrappers):
            return False
        if any(w._mode not in (QcQuantizeOpMode.ACTIVE, QcQuantizeOpMode.PASSTHROUGH) for w in wrappers):
            return False   # ANALYSIS: the statistics need the scores and the probabilities
        if not all(t.is_cuda and t.dtype == torch.float32 and t.device == q.device for t in (q, k, v)):
            return False
        return self.softmax.get_original_module().dim in (-1, 2) and q.shape[2] in ATTN_CORE_HEAD_DIMS

    def _core_out(self, q, k, v, bsz, attn_mask, key_padding_mask):
        if attn_mask is not None and attn_mask.shape[0] == 1:
            attn_mask = attn_mask[0]   # one [L, S] table for every batch entry and head
        score_enc = self.matmul_1.fused_output_encoding()
        prob_enc = self.softmax.fused_output_encoding()
        out_enc = self.matmul_2.fused_output_encoding()
        return attn_core(q, k, v, bsz, self.num_heads, attn_mask, key_padding_mask, score_enc, prob_enc, out_enc)

    # -- the attention probabilities --------------------------------------------------------------
    def _fused_route(self, q: Tensor, k: Tensor, src_len: int) -> bool:
        m1, sm = self.matmul_1, self.softmax
        opt_in = getattr(self, "fused_backward", False)
        if isinstance(m1, LearnedGridQuantWrapper) and isinstance(sm, LearnedGridQuantWrapper):
            allowed = opt_in   # range learning: the fused route is the opt-in one, with or without a gradient
        elif isinstance(m1, StaticGridQuantWrapper) and isinstance(sm, StaticGridQuantWrapper):
            allowed = opt_in or not (torch.is_grad_enabled() and (q.requires_grad or k.requires_grad))
        else:
            return False
        if not (self.fused and allowed):
            return False
        if not (q.is_cuda and q.dtype == torch.float32 and k.dtype == torch.float32 and k.device == q.device):
            return False
        if not (m1.output_fusable() and sm.output_fusable()):
            return False
        return sm.get_original_module().dim in (-1, 2) and src_len <= attn_softmax_max_s()

    def _fused_probs(self, q, k, bsz, attn_mask, key_padding_mask):
        scores = torch.bmm(q, k.transpose(1, 2))
        if attn_mask is not None and attn_mask.shape[0] == 1:
            attn_mask = attn_mask[0]   # one [L, S] table for every batch entry and head
        if isinstance(self.matmul_1, LearnedGridQuantWrapper):
            # range learning: each wrapper's gate first, as its forward() runs it; then one launch that
            # reads the four range parameters on the device
            score_min, score_max, score_flags = self.matmul_1.fused_output_grid()
            prob_min, prob_max, prob_flags = self.softmax.fused_output_grid()
            return AttnSoftmaxLearned.apply(scores, bsz, self.num_heads, attn_mask, key_padding_mask, score_min,
                                            score_max, score_flags, prob_min, prob_max, prob_flags)
        if getattr(self, "fused_backward", False):
            # the statistics (ANALYSIS) see the tensors outside the graph; never in place
            score_enc = self.matmul_1.fused_output_encoding()
            self.matmul_1.observe_output(scores.detach())
            prob_enc = self.softmax.fused_output_encoding()
            probs = AttnSoftmax.apply(scores, bsz, self.num_heads, attn_mask, key_padding_mask, score_enc, prob_enc)
            self.softmax.observe_output(probs.detach())
            return probs
        score_enc = self.matmul_1.fused_output_encoding()
        queued = self.matmul_1.observe_output(scores)   # ANALYSIS: the statistics may read it later
        prob_enc = self.softmax.fused_output_encoding()
        probs = attn_softmax(scores, bsz, self.num_heads, attn_mask, key_padding_mask, score_enc, prob_enc,
                             out=None if queued else scores)
        self.softmax.observe_output(probs)
        return probs

    def _literal_probs(self, q, k, bsz, attn_mask, key_padding_mask):
        scores = self.matmul_1(q, k.transpose(1, 2))
        if attn_mask is not None:
            scores.masked_fill_(attn_mask, _NEG_INF)
        if key_padding_mask is not None:
            shape = scores.shape
            scores = scores.view(bsz, self.num_heads, shape[1], shape[2]).masked_fill(
                key_padding_mask.view(bsz, 1, 1, shape[2]), _NEG_INF).view(shape)
        return self.softmax(scores)


def create_quantizable_multihead_attention(module: nn.MultiheadAttention) -> QuantizableMultiheadAttention:
    """A QuantizableMultiheadAttention computing what `module` computes (activation.py:447)."""
    bias = module.in_proj_bias is not None
    add_bias_kv = module.bias_k is not None and module.bias_v is not None
    ref = module.out_proj.weight
    new = QuantizableMultiheadAttention(module.embed_dim, module.num_heads, dropout=module.dropout, bias=bias,
                                        add_bias_kv=add_bias_kv, add_zero_attn=module.add_zero_attn, kdim=module.kdim,
                                        vdim=module.vdim, batch_first=module.batch_first, device=ref.device,
                                        dtype=ref.dtype)
    with torch.no_grad():
        if module.in_proj_weight is not None:
            w_q, w_k, w_v = torch.chunk(module.in_proj_weight, 3, dim=0)
        else:
            w_q, w_k, w_v = module.q_proj_weight, module.k_proj_weight, module.v_proj_weight
        new.linear_Q.weight.copy_(w_q)
        new.linear_K.weight.copy_(w_k)
        new.linear_V.weight.copy_(w_v)
        new.out_proj.weight.copy_(module.out_proj.weight)
        if bias:
            b_q, b_k, b_v = torch.chunk(module.in_proj_bias, 3, dim=0)
            new.linear_Q.bias.copy_(b_q)
            new.linear_K.bias.copy_(b_k)
            new.linear_V.bias.copy_(b_v)
            new.out_proj.bias.copy_(module.out_proj.bias)
        if add_bias_kv:
            new.bias_k.copy_(module.bias_k)
            new.bias_v.copy_(module.bias_v)
    new.train(module.training)
    return new


# ---- encoder / decoder layers with their residual adds as modules ------------------------------------
class QuantizableTransformerEncoderLayer(nn.TransformerEncoderLayer):
    """nn.TransformerEncoderLayer whose residual additions are the children add1 and add2; always the
    layer-by-layer path (activation.py:491)."""

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.add1 = Add()
        self.add2 = Add()

    # pylint: disable=arguments-differ
    def forward(self, src: Tensor, src_mask: Optional[Tensor] = None, src_key_padding_mask: Optional[Tensor] = None,
                is_causal: bool = False) -> Tensor:
        x = src
        if self.norm_first:
            x = self.add1(x, self._sa_block(self.norm1(x), src_mask, src_key_padding_mask))
            return self.add2(x, self._ff_block(self.norm2(x)))
        x = self.norm1(self.add1(x, self._sa_block(x, src_mask, src_key_padding_mask)))
        return self.norm2(self.add2(x, self._ff_block(x)))


class QuantizableTransformerDecoderLayer(nn.TransformerDecoderLayer):
    """nn.TransformerDecoderLayer whose residual additions are the children add1, add2 and add3
    (activation.py:623)."""

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.add1 = Add()
        self.add2 = Add()
        self.add3 = Add()

    # pylint: disable=arguments-differ
    def forward(self, tgt: Tensor, memory: Tensor, tgt_mask: Optional[Tensor] = None,
                memory_mask: Optional[Tensor] = None, tgt_key_padding_mask: Optional[Tensor] = None,
                memory_key_padding_mask: Optional[Tensor] = None, tgt_is_causal: bool = False,
                memory_is_causal: bool = False) -> Tensor:
        x = tgt
        if self.norm_first:
            x = self.add1(x, self._sa_block(self.norm1(x), tgt_mask, tgt_key_padding_mask))
            x = self.add2(x, self._mha_block(self.norm2(x), memory, memory_mask, memory_key_padding_mask))
            return self.add3(x, self._ff_block(self.norm3(x)))
        x = self.norm1(self.add1(x, self._sa_block(x, tgt_mask, tgt_key_padding_mask)))
        x = self.norm2(self.add2(x, self._mha_block(x, memory, memory_mask, memory_key_padding_mask)))
        return self.norm3(self.add3(x, self._ff_block(x)))


def _quantizable_layer(cls, layer):
    """A `cls` layer with the hyper-parameters of `layer` and copies of its children."""
    ref = layer.linear1.weight
    new = cls(d_model=layer.linear1.in_features, nhead=layer.self_attn.num_heads,
              dim_feedforward=layer.linear1.out_features, dropout=layer.dropout.p, activation=layer.activation,
              layer_norm_eps=layer.norm1.eps, batch_first=layer.self_attn.batch_first, norm_first=layer.norm_first,
              bias=layer.linear1.bias is not None, device=ref.device, dtype=ref.dtype)
    for name, child in layer.named_children():
        setattr(new, name, copy.deepcopy(child))
    new.train(layer.training)
    return new


def create_quantizable_transformer_encoder_layer(layer: nn.TransformerEncoderLayer) \
        -> QuantizableTransformerEncoderLayer:
    """activation.py:715. The children (the attention block whatever its class, the linears, norms,
    dropouts and a module activation) are deep copies of the source's."""
    return _quantizable_layer(QuantizableTransformerEncoderLayer, layer)


def create_quantizable_transformer_decoder_layer(layer: nn.TransformerDecoderLayer) \
        -> QuantizableTransformerDecoderLayer:
    """activation.py:743."""
    return _quantizable_layer(QuantizableTransformerDecoderLayer, layer)


# ---- whole models --------------------------------------------------------------------------------
def set_fused_attention_backward(model: nn.Module, enabled: bool = True) -> int:
    """Sets `fused_backward` on every QuantizableMultiheadAttention of `model` (a QuantizationSimModel's
    .model included); returns how many there are."""
    blocks = [m for m in model.modules() if isinstance(m, QuantizableMultiheadAttention)]
    for m in blocks:
        m.fused_backward = bool(enabled)
    return len(blocks)


def set_fused_attention_core(model: nn.Module, enabled: bool = True) -> int:
    """Sets `fused_core` on every QuantizableMultiheadAttention of `model` (a QuantizationSimModel's
    .model included); returns how many there are."""
    blocks = [m for m in model.modules() if isinstance(m, QuantizableMultiheadAttention)]
    for m in blocks:
        m.fused_core = bool(enabled)
    return len(blocks)


def prepare_pt_transformer_for_quantsim(model: nn.Module) -> None:
    """model_preparer.py:694: the functional activation of every nn.TransformerEncoderLayer /
    DecoderLayer becomes a module (a child the sim can wrap), in place."""
    for m in model.modules():
        if isinstance(m, (nn.TransformerEncoderLayer, nn.TransformerDecoderLayer)) and \
                not isinstance(m.activation, nn.Module):
            if m.activation is F.relu:
                m.activation = nn.ReLU()
            elif m.activation is F.gelu:
                m.activation = nn.GELU()
            else:
                raise NotImplementedError("no module for the activation function %r" % (m.activation,))


def _replace_modules(model: nn.Module, kind, skip, constructor) -> None:
    for name, child in list(model.named_children()):
        if isinstance(child, kind) and not isinstance(child, skip):
            setattr(model, name, constructor(child))
        else:
            _replace_modules(child, kind, skip, constructor)


def get_quantizable_pt_transformer_model(model: nn.Module) -> None:
    """transformers/utils.py:46: every nn.MultiheadAttention of `model` replaced by its quantizable
    form and every functional layer activation by a module, in place."""
    _replace_modules(model, nn.MultiheadAttention, QuantizableMultiheadAttention,
                     create_quantizable_multihead_attention)
    prepare_pt_transformer_for_quantsim(model)
    # nn.TransformerEncoder decides its nested-tensor fast path when it is constructed, from its
    # layer's _qkv_same_embed_dim among others; with the layers' attention replaced the answer is no
    for m in model.modules():
        if isinstance(m, nn.TransformerEncoder) and \
                any(isinstance(l.self_attn, QuantizableMultiheadAttention) for l in m.layers):
            m.use_nested_tensor = False
