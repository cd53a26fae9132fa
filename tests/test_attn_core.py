"""aimet_attn_core without a GPU: the two symbols in the header, the binding and the library, and the
refusal of host tensors (there is no CPU implementation behind attn_core)."""
import os

import pytest
import torch

from conftest import REPO

from aimet_amd import _native
from aimet_amd import transformers as T


@pytest.mark.parametrize("name", ["aimet_attn_core", "aimet_attn_core_launch_count"])
def test_symbol_is_declared_bound_and_exported(name):
    with open(os.path.join(REPO, "include", "aimet_amd.h")) as f:
        assert "int %s(" % name in f.read()
    assert name in _native.EXPORTED_SYMBOLS and hasattr(_native.load(), name)


def test_host_tensors_are_refused_and_the_route_is_off_by_default():
    q = torch.zeros(2, 3, 32)
    with pytest.raises(ValueError, match="GPU"):
        T.attn_core(q, q, q, 1, 2)
    m = T.QuantizableMultiheadAttention(64, 2)
    assert m.fused_core is False and T.set_fused_attention_core(m) == 1 and m.fused_core is True
