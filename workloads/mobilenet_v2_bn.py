"""MobileNet-v2 (1.0, 224x224) as it comes out of training: bias-free convs followed by BatchNorm2d and
ReLU6. The network of workloads/mobilenet_v2.py before batch-norm folding. Random init (seed); the
BatchNorm parameters are seeded so that channel ranges differ as they do in trained networks: gamma
log-uniform over about two decades, beta and running mean normal, running var positive."""
import math

import torch
from torch import nn


def _conv_bn(cin, cout, k, stride=1, pad=0, groups=1, act=True):
    layers = [nn.Conv2d(cin, cout, k, stride, pad, groups=groups, bias=False), nn.BatchNorm2d(cout)]
    if act:
        layers.append(nn.ReLU6())
    return layers


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, stride, expand):
        super().__init__()
        hidden = cin * expand
        self.use_res = stride == 1 and cin == cout
        layers = []
        if expand != 1:
            layers += _conv_bn(cin, hidden, 1)
        layers += _conv_bn(hidden, hidden, 3, stride, 1, groups=hidden)
        layers += _conv_bn(hidden, cout, 1, act=False)
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.use_res else self.conv(x)


class MobileNetV2BN(nn.Module):
    CFG = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]

    def __init__(self, num_classes=1000):
        super().__init__()
        layers = _conv_bn(3, 32, 3, 2, 1)
        cin = 32
        for t, c, n, s in self.CFG:
            for i in range(n):
                layers.append(InvertedResidual(cin, c, s if i == 0 else 1, t))
                cin = c
        layers += _conv_bn(cin, 1280, 1)
        self.features = nn.Sequential(*layers)
        self.classifier = nn.Linear(1280, num_classes)

    def forward(self, x):
        x = self.features(x)
        return self.classifier(x.mean((2, 3)))


def mobilenet_v2_bn(seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    m = MobileNetV2BN()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (nn.Conv2d, nn.Linear)):
                fan_in = mod.weight[0].numel()
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                if mod.bias is not None:
                    mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.01)
            elif isinstance(mod, nn.BatchNorm2d):
                n = mod.num_features
                # gamma log-uniform in 0.03 .. 3 (mean square about 1: activations keep their size)
                mod.weight.copy_(torch.exp(math.log(0.03) + torch.rand(n, generator=g) * math.log(100.0)))
                mod.bias.copy_(torch.randn(n, generator=g) * 0.5)
                mod.running_mean.copy_(torch.randn(n, generator=g) * 0.5)
                mod.running_var.copy_(torch.rand(n, generator=g) * 1.5 + 0.5)
    return m.to(device).eval()
