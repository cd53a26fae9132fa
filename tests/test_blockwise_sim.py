"""Blockwise / LPBQ weight quantizers in the sim, the parts that need no device: the shape and layout
rules of the two configuration functions, the refusal without a device, the exported fields."""
import pytest

torch = pytest.importorskip("torch")
nn = torch.nn


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(16, 8)
        self.conv = nn.Conv2d(8, 4, 3)
        self.odd = nn.Linear(10, 6)
        self.up = nn.ConvTranspose2d(8, 4, 3)
        self.dw = nn.Conv2d(8, 8, 3, groups=8)
        self.grouped = nn.Conv2d(8, 4, 3, groups=2)


TYPES = (nn.Linear, nn.Conv2d, nn.ConvTranspose2d)


def make_sim():
    from aimet_amd.quantsim import QuantizationSimModel
    return QuantizationSimModel(Net())


def test_block_views():
    from aimet_amd.blockwise import weight_block_view
    net = Net()
    assert weight_block_view(net.fc, 4) == (8, 4, 4)
    assert weight_block_view(net.fc, 16) == (8, 1, 16)
    assert weight_block_view(net.conv, 4) == (4, 2, 36)   # the block along Cin: block_size * kh * kw
    for module, why in ((net.odd, "not divisible"), (net.up, "strided"), (net.dw, "grouped"), (net.grouped, "grouped"),
                        (nn.Embedding(8, 4), "Linear and Conv")):
        with pytest.raises(ValueError, match=why):
            weight_block_view(module, 4)


@pytest.mark.parametrize("grouped", [False, True], ids=["blockwise", "lpbq"])
def test_configuration_functions(grouped):
    from aimet_amd import blockwise as B

    def configure(sim, strict):
        if grouped:
            return B.set_grouped_blockwise_quantization_for_weights(sim, TYPES, 4, 8, 4, strict=strict)
        return B.set_blockwise_quantization_for_weights(sim, TYPES, 4, False, 4, strict=strict)

    sim = make_sim()
    before = {n: w.param_quantizers["weight"] for n, w in sim.quant_wrappers()}
    assert configure(sim, False) == ["fc", "conv"]
    for n, w in sim.quant_wrappers():
        q = w.param_quantizers["weight"]
        if n not in ("fc", "conv"):
            assert q is before[n]   # left untouched
            continue
        assert isinstance(q, B.BlockwiseQuantizer) and q.bitwidth == 4 and q.block_size == 4
        assert (q.R, q.NB, q.BL) == B.weight_block_view(w._module_to_wrap, 4)
        assert q.use_symmetric_encodings == grouped and q.scale_bitwidth == (4 if grouped else 0)
        assert q.decompressed_bw == (8 if grouped else None) and q.encoding is None
    for layer in ("odd", "up", "dw", "grouped"):
        sim = make_sim()
        sim.exclude_layers_from_quantization([getattr(sim.model, n) for n in ("odd", "up", "dw", "grouped")
                                              if n != layer])
        with pytest.raises(ValueError, match=layer):
            configure(sim, True)
    with pytest.raises(ValueError, match="decompressed_bw"):
        B.set_grouped_blockwise_quantization_for_weights(make_sim(), nn.Linear, 4, 4, 4)


def test_no_cpu_path():
    from aimet_amd import blockwise as B
    sim = make_sim()
    B.set_blockwise_quantization_for_weights(sim, nn.Linear, 4, True, 4)
    q = sim.model.fc.param_quantizers["weight"]
    q.update_encoding_stats(sim.model.fc.weight.data)
    with pytest.raises(RuntimeError, match="no CPU path"):
        q.compute_encoding()
    assert q.encoding is None
    with pytest.raises(RuntimeError, match="no encoding"):
        q.quantize_dequantize(sim.model.fc.weight.data, "nearest")


@pytest.mark.parametrize("dbw", [None, 8])
def test_exported_fields_round_trip(dbw):
    from aimet_amd.blockwise import BlockwiseQuantizer
    q = BlockwiseQuantizer((2, 8), 4, "nearest", None, True, 4, decompressed_bw=dbw)
    assert q.export_encodings() is None
    delta = [0.5, 0.25, 1.0, 0.125]
    q.table = torch.tensor([[-8 * d for d in delta], [7 * d for d in delta], delta, [-8.0] * 4])
    if dbw:
        q.int_scale = torch.tensor([16, 8, 16, 2], dtype=torch.int32)
        q.channel_scale = torch.tensor([0.03125, 0.0625], dtype=torch.float64)
    entries = q.export_encodings()
    base = {"min", "max", "scale", "offset", "bitwidth", "is_symmetric", "dtype", "block_size"}
    assert [set(e) for e in entries] == [base | ({"per_block_int_scale", "compressed_bw"} if dbw else set())] * 4
    assert [e["block_size"] for e in entries] == [4] * 4 and entries[1]["offset"] == -8
    if dbw:
        assert [e["scale"] for e in entries] == [0.03125, 0.03125, 0.0625, 0.0625]   # [channel][block] order
        assert [e["per_block_int_scale"] for e in entries] == [16, 8, 16, 2]
        assert entries[0]["compressed_bw"] == 4 and entries[0]["bitwidth"] == 8
    else:
        assert [e["scale"] for e in entries] == delta and entries[0]["bitwidth"] == 4
    fresh = BlockwiseQuantizer((2, 8), 4, "nearest", None, True, 4, decompressed_bw=dbw)
    fresh.import_encodings(entries)
    assert torch.equal(fresh.table, q.table) and fresh.bitwidth == 4 and fresh.decompressed_bw == dbw
    assert [e.delta for e in fresh.encoding] == delta and fresh.encoding[3].bw == 4
    with pytest.raises(AssertionError, match="number of blocks"):
        fresh.import_encodings(entries[:3])
