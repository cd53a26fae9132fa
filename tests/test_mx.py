"""MX quantization without a GPU (aimet_amd.mx): what the Python surface refuses, the formats' widths,
and what an MxQuantizer keeps through pickling."""
import pickle

import pytest

torch = pytest.importorskip("torch")

from aimet_amd import mx  # noqa: E402
from aimet_amd.mx import MxFormat, MxQuantizer  # noqa: E402
from aimet_amd.quantizers import QuantizationDataType  # noqa: E402


@pytest.mark.parametrize("tensor,error", [(torch.zeros(2, 64), RuntimeError),
                                          (torch.zeros(2, 64, dtype=torch.int32), TypeError),
                                          (torch.zeros(2, 40), ValueError)], ids=["cpu", "int", "axis40"])
def test_refusals(tensor, error):
    with pytest.raises(error):
        mx.mx_quantize_dequantize(tensor, MxFormat.MXFP4_E2M1)
    with pytest.raises(error):
        mx.mx_quantize(tensor, MxFormat.MXFP4_E2M1)
    with pytest.raises(error):
        MxQuantizer(MxFormat.MXFP4_E2M1).quantize_dequantize(tensor, "nearest")


def test_format_widths():
    assert mx.MX_BLOCK_SIZE == 32
    assert {f.name: f.element_bits for f in MxFormat} == {"MXFP8_E4M3": 8, "MXFP8_E5M2": 8, "MXFP6_E3M2": 6,
                                                          "MXFP6_E2M3": 6, "MXFP4_E2M1": 4}


def test_quantizer_pickles():
    q = MxQuantizer(MxFormat.MXFP6_E2M3, axis=1)
    assert q.computes_own_encoding and q.data_type == QuantizationDataType.float and q.bitwidth == 6
    q.compute_encoding()
    q.freeze_encoding()
    back = pickle.loads(pickle.dumps(q))
    assert (back.format, back.axis, back.bitwidth, back.enabled) == (MxFormat.MXFP6_E2M3, 1, 6, True)
    assert back.is_encoding_frozen and back.encoding is not None
    assert back.export_encodings() == [{"dtype": "float", "bitwidth": 6, "block_size": 32, "format": "MXFP6_E2M3",
                                        "axis": 1}]
