"""Functional operations as modules, so that QuantizationSimModel can give them quantizers
(aimet_torch.v1.nn.modules.custom: Add, Multiply, Divide, MatMul), and the tuple of module types a transformer
needs wrapped.

    sim = QuantizationSimModel(model, dummy_input, quantizable_types=TRANSFORMER_QUANTIZABLE_TYPES)

The sim's default (DEFAULT_QUANTIZABLE_TYPES) stays as it is.
"""
import torch
from torch import nn

from aimet_amd.quantsim import DEFAULT_QUANTIZABLE_TYPES


class Add(nn.Module):
    """x + y."""

    @staticmethod
    def forward(x, y):
        return x + y


class Multiply(nn.Module):
    """x * y (y a tensor or a number)."""

    @staticmethod
    def forward(x, y):
        return x * y


class Divide(nn.Module):
    """x / y (y a tensor or a number)."""

    @staticmethod
    def forward(x, y):
        return torch.div(x, y)


class MatMul(nn.Module):
    """torch.matmul(x, y)."""

    @staticmethod
    def forward(x, y):
        return torch.matmul(x, y)


TRANSFORMER_QUANTIZABLE_TYPES = DEFAULT_QUANTIZABLE_TYPES + (Add, Divide, MatMul, nn.Softmax, nn.LayerNorm, nn.GELU,
                                                             nn.ReLU)
