"""Reference arithmetic of BatchNorm re-estimation and BN fold to scale (csrc/bn_reest.hip, the fold
to scale of csrc/dfq.hip, aimet_amd/bn_reestimation.py), in numpy and plain torch; no device needed.

* moments: a channel's exact batch statistics in np.longdouble, with the two magnitudes the error
  bounds of the shifted sums are stated in;
* forward64: the normalisation's coefficients and output in float64;
* fold_scale: the fp32 backward fold with the range rule of aimet_bnre_fold_scale;
* reestimate_torch: the reference's procedure (aimet_torch/bn_reestimation.py) restated in plain
  torch, for any device;
* TinyNet: the network of tests/golden/golden_bnre.npz.
"""
import numpy as np
import torch
from torch import nn
from torch.nn.modules.batchnorm import _BatchNorm

F = np.float32
LD = np.longdouble


def moments(x):
    """x: [outer][C][inner] float32. Per channel, in long double: mean, biased and unbiased variance
    (two-pass around the exact mean), and with the kernel's shift K = x[0][c][0]:
    Q_K = sum (x - K)^2 and A_K = sum |x - K|."""
    x = np.asarray(x, F)
    C = x.shape[1]
    v = np.moveaxis(x, 1, 0).reshape(C, -1).astype(LD)
    n = v.shape[1]
    mean = v.sum(axis=1) / n
    m2 = ((v - mean[:, None]) ** 2).sum(axis=1)
    d = v - v[:, :1]
    return dict(n=n, mean=mean, var_b=m2 / n, var_u=m2 / (n - 1) if n > 1 else m2 * np.nan,
                Q_K=(d * d).sum(axis=1), A_K=np.abs(d).sum(axis=1))


def forward64(x, gamma, beta, eps):
    """(a64, b64, y64) of y = x * a + b in float64 from the exact batch statistics; gamma / beta None:
    ones / zeros."""
    x = np.asarray(x, F)
    C = x.shape[1]
    m = moments(x)
    g = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    bt = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    a = g / np.sqrt(m["var_b"].astype(np.float64) + np.float64(eps))
    b = bt - m["mean"].astype(np.float64) * a
    y = x.astype(np.float64) * a[None, :, None] + b[None, :, None]
    return a, b, y


def fold_scale(w, bias, gamma, beta, mean, var, eps, enc_min, enc_max):
    """The backward fold of aimet_dfq_bn_fold (output channels on axis 0 of w) in float32, every
    product, quotient and root rounded on its own, and the range rule of aimet_bnre_fold_scale.
    A channel with sqrt(var + eps) == 0 is left as it was. Returns (w, bias, enc_min, enc_max, bad)."""
    w, bias = np.array(w, F), np.array(bias, F)
    enc_min, enc_max = np.array(enc_min, F), np.array(enc_max, F)
    gamma, beta, mean, var = (np.asarray(v, F) for v in (gamma, beta, mean, var))
    with np.errstate(all="ignore"):
        sigma = np.sqrt(var + F(eps))
        ok = sigma != 0
        c = np.where(ok, gamma / np.where(ok, sigma, F(1)), F(1)).astype(F)
        shape = (-1,) + (1,) * (w.ndim - 1)
        w_out = np.where(ok.reshape(shape), w * c.reshape(shape), w).astype(F)
        b_out = np.where(ok, beta - (mean - bias) * c, bias).astype(F)
        lo, hi = (enc_min * c).astype(F), (enc_max * c).astype(F)
        new_min = np.where(ok, np.where(c >= 0, lo, hi), enc_min).astype(F)
        new_max = np.where(ok, np.where(c >= 0, hi, lo), enc_max).astype(F)
    return w_out, b_out, new_min, new_max, bool((~ok).any())


def active_bns(model):
    return [m for m in model.modules() if isinstance(m, _BatchNorm) and m.running_mean is not None
            and m.running_var is not None]


def reestimate_torch(model, batches, forward_fn=None):
    """aimet_torch/bn_reestimation.py reestimate_bn_stats over all of `batches`, in plain torch:
    everything in eval mode except the BatchNorms, momentum 1, float32 sums of the running buffers
    after every batch, their mean written back. Flags are restored; nothing is undone."""
    forward_fn = forward_fn or (lambda m, data: m(data))
    bns = active_bns(model)
    modes = [(m, m.training) for m in model.modules()]
    momenta = [bn.momentum for bn in bns]
    try:
        model.eval()
        for bn in bns:
            bn.training, bn.momentum = True, 1.0
            bn.reset_running_stats()
        with torch.no_grad():
            sums = [(torch.zeros_like(bn.running_mean), torch.zeros_like(bn.running_var)) for bn in bns]
            for data in batches:
                forward_fn(model, data)
                for bn, (sm, sv) in zip(bns, sums):
                    sm += bn.running_mean
                    sv += bn.running_var
            for bn, (sm, sv) in zip(bns, sums):
                bn.running_mean.copy_(sm / len(batches))
                bn.running_var.copy_(sv / len(batches))
    finally:
        for bn, momentum in zip(bns, momenta):
            bn.momentum = momentum
        for m, was in modes:
            m.training = was


class TinyNet(nn.Module):
    """conv / BN / ReLU / conv / BN / pool / linear / BN1d on 3x8x8 inputs."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 5, 3, padding=1)
        self.bn1 = nn.BatchNorm2d(5)
        self.relu = nn.ReLU()
        self.conv2 = nn.Conv2d(5, 6, 3, bias=False)
        self.bn2 = nn.BatchNorm2d(6)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.flatten = nn.Flatten()
        self.fc = nn.Linear(6, 4)
        self.bn3 = nn.BatchNorm1d(4)

    def forward(self, x):
        x = self.relu(self.bn1(self.conv1(x)))
        x = self.pool(self.bn2(self.conv2(x)))
        return self.bn3(self.fc(self.flatten(x)))


BN_NAMES = ("bn1", "bn2", "bn3")


def tiny_net(golden, dtype=torch.float32, device="cpu"):
    """TinyNet with the fixture's parameters and starting statistics."""
    net = TinyNet()
    state = {k[len("param_"):]: torch.from_numpy(np.asarray(v)) for k, v in golden.items() if k.startswith("param_")}
    net.load_state_dict(state)
    return net.to(device=device, dtype=dtype)


def tiny_batches(golden, dtype=torch.float32, device="cpu"):
    return [torch.from_numpy(b).to(device=device, dtype=dtype) for b in np.asarray(golden["batches"])]


def reestimate_float64(golden):
    """{bn name: (running_mean, running_var)} of the fixture network re-estimated in float64 on the
    CPU: training-mode BatchNorms, unbiased variance, the mean over the batches."""
    net = tiny_net(golden, torch.float64)
    reestimate_torch(net, tiny_batches(golden, torch.float64))
    return {n: (getattr(net, n).running_mean.numpy().copy(), getattr(net, n).running_var.numpy().copy())
            for n in BN_NAMES}
