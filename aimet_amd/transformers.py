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
  * literal: the children called one by one. Everything else -- range learning / QAT, 16-bit or CPU
    tensors, float data types, stochastic rounding, enabled input quantizers, an unwrapped module,
    longer rows -- and `module.fused = False`.

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

from aimet_amd import _native
from aimet_amd.elementwise_ops import Add, Divide, MatMul
from aimet_amd.qc_quantize_op import StaticGridQuantWrapper

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


def _encoding_c(enc):
    """A TfEncoding, or (min, max, bitwidth) -> the C struct (delta and offset are recomputed from the
    three, as aimet_qdq_per_tensor does)."""
    if enc is None:
        return None
    if isinstance(enc, (tuple, list)):
        return _native.TfEncodingC(float(enc[0]), float(enc[1]), 0.0, 0.0, int(enc[2]))
    return _native.TfEncodingC(enc.min, enc.max, enc.delta, enc.offset, enc.bw)


def _mask_bytes(mask, shape, device, what):
    if mask is None:
        return None
    if mask.dtype != torch.bool or tuple(mask.shape) != tuple(shape) or mask.device != device:
        raise ValueError("attn_softmax: %s must be a bool tensor of shape %s on %s, got %s %s on %s"
                         % (what, tuple(shape), device, mask.dtype, tuple(mask.shape), mask.device))
    return mask.contiguous().view(torch.uint8)


def attn_softmax(scores: Tensor, batch: int, num_heads: int, attn_mask: Optional[Tensor] = None,
                 key_padding_mask: Optional[Tensor] = None, score_enc=None, prob_enc=None,
                 out: Optional[Tensor] = None) -> Tensor:
    """One aimet_attn_softmax launch on scores [batch * num_heads, L, S] (float32, contiguous, GPU):
    QDQ(score_enc), masks (attn_mask [L, S] or [batch * num_heads, L, S], key_padding_mask
    [batch, S]; bool, True = -inf), softmax, QDQ(prob_enc). Encodings: TfEncoding, (min, max, bw) or
    None. `out` may be `scores`. There is no other implementation behind this function."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 3 and scores.is_contiguous()):
        raise ValueError("attn_softmax: scores must be a contiguous float32 [B H, L, S] tensor on the GPU")
    BH, L, S = scores.shape
    if BH != batch * num_heads:
        raise ValueError("attn_softmax: scores has %d matrices, batch * num_heads is %d" % (BH, batch * num_heads))
    if out is None:
        out = torch.empty_like(scores)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.shape == scores.shape and out.is_contiguous() and
              out.device == scores.device):
        raise ValueError("attn_softmax: out must match scores")
    per_bh = attn_mask is not None and attn_mask.dim() == 3
    am = _mask_bytes(attn_mask, (BH, L, S) if per_bh else (L, S), scores.device, "attn_mask")
    kpm = _mask_bytes(key_padding_mask, (batch, S), scores.device, "key_padding_mask")
    s_enc, p_enc = _encoding_c(score_enc), _encoding_c(prob_enc)
    with torch.cuda.device(scores.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _native.call("aimet_attn_softmax", scores.data_ptr(), out.data_ptr(), batch, num_heads, L, S,
                     am.data_ptr() if am is not None else None, int(per_bh),
                     kpm.data_ptr() if kpm is not None else None,
                     ctypes.byref(s_enc) if s_enc is not None else None,
                     ctypes.byref(p_enc) if p_enc is not None else None, stream)
    return out


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

    # -- the attention probabilities --------------------------------------------------------------
    def _fused_route(self, q: Tensor, k: Tensor, src_len: int) -> bool:
        m1, sm = self.matmul_1, self.softmax
        if not (self.fused and isinstance(m1, StaticGridQuantWrapper) and isinstance(sm, StaticGridQuantWrapper)):
            return False
        if not (q.is_cuda and q.dtype == torch.float32 and k.dtype == torch.float32 and k.device == q.device):
            return False
        if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad):
            return False
        if not (m1.output_fusable() and sm.output_fusable()):
            return False
        return sm.get_original_module().dim in (-1, 2) and src_len <= attn_softmax_max_s()

    def _fused_probs(self, q, k, bsz, attn_mask, key_padding_mask):
        scores = torch.bmm(q, k.transpose(1, 2))
        score_enc = self.matmul_1.fused_output_encoding()
        queued = self.matmul_1.observe_output(scores)   # ANALYSIS: the statistics may read it later
        prob_enc = self.softmax.fused_output_encoding()
        if attn_mask is not None and attn_mask.shape[0] == 1:
            attn_mask = attn_mask[0]   # one [L, S] table for every batch entry and head
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
