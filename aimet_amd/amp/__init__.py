"""Automatic mixed precision (aimet_torch/amp, aimet_common/amp): which bitwidth each quantizer group gets."""
