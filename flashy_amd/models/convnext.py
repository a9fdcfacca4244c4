# Copyright (c) Flashy-AMD authors.
"""ConvNeXt (Liu et al., "A ConvNet for the 2020s"), plain torch: the twin of
:mod:`flashy_amd.models.convnext_native`, as resnet.py is of
resnet_native.py.  No stochastic depth (TODO.md).

ConvNeXt V2 (Woo et al., "ConvNeXt V2: Co-designing and Scaling ConvNets with
Masked Autoencoders") is the same network with :class:`ConvNeXtV2Block`: no
layer scale, and a global response normalization (:class:`GRN`) behind the
GELU.
"""
from __future__ import annotations

import typing as tp

import torch
from torch import nn
import torch.nn.functional as F


class ConvNeXtBlock(nn.Module):
    """NCHW in and out: depthwise k x k -> LayerNorm over channels -> 1x1
    expand (x4) -> GELU (erf) -> 1x1 project -> layer scale -> residual."""

    def __init__(self, dim: int, kernel_size: int = 7,
                 layer_scale_init: float = 1e-6):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size,
                                padding=kernel_size // 2, groups=dim,
                                bias=True)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init * torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.dwconv(x).permute(0, 2, 3, 1)
        y = self.pwconv2(self.act(self.pwconv1(self.norm(y))))
        return x + (self.gamma * y).permute(0, 3, 1, 2)


class GRN(nn.Module):
    """Global response normalization over an NHWC tensor: each (image,
    channel) plane's L2 norm ``Gx``, divided by the mean of the image's norms
    plus ``eps``, rescales the plane; ``weight`` and ``bias`` start at zero,
    which makes the layer the identity."""

    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.zeros(dim))
        self.bias = nn.Parameter(torch.zeros(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        gx = torch.norm(x, p=2, dim=(1, 2), keepdim=True)
        nx = gx / (gx.mean(dim=-1, keepdim=True) + self.eps)
        return self.weight * (x * nx) + self.bias + x


class ConvNeXtV2Block(nn.Module):
    """NCHW in and out: depthwise k x k -> LayerNorm over channels -> 1x1
    expand (x4) -> GELU (erf) -> GRN -> 1x1 project -> residual."""

    def __init__(self, dim: int, kernel_size: int = 7):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size,
                                padding=kernel_size // 2, groups=dim,
                                bias=True)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.grn = GRN(4 * dim)
        self.pwconv2 = nn.Linear(4 * dim, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.dwconv(x).permute(0, 2, 3, 1)
        y = self.pwconv2(self.grn(self.act(self.pwconv1(self.norm(y)))))
        return x + y.permute(0, 3, 1, 2)


class ChannelLayerNorm(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW tensor."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape,
                         self.weight, self.bias, self.eps)
        return y.permute(0, 3, 1, 2)


class ConvNeXt(nn.Module):
    """NCHW in, logits out: patchify stem (conv ``patch`` x ``patch`` stride
    ``patch`` with bias, channel LayerNorm), four stages of
    :class:`ConvNeXtBlock` with LayerNorm + conv 2x2 stride 2 between them,
    global mean, LayerNorm, Linear.  ``block`` is the block class:
    :class:`ConvNeXtV2Block` makes it ConvNeXt V2."""

    def __init__(self, depths: tp.Sequence[int], dims: tp.Sequence[int],
                 num_classes: int, patch: int = 4, in_chans: int = 3,
                 block: tp.Callable[[int], nn.Module] = ConvNeXtBlock):
        super().__init__()
        assert len(depths) == len(dims) == 4, (depths, dims)
        self.stem = nn.Conv2d(in_chans, dims[0], patch, patch)
        self.stem_norm = ChannelLayerNorm(dims[0], eps=1e-6)
        self.stages = nn.ModuleList(
            nn.Sequential(*[block(d) for _ in range(n)])
            for n, d in zip(depths, dims))
        self.down_norms = nn.ModuleList(
            ChannelLayerNorm(d, eps=1e-6) for d in dims[:3])
        self.down_convs = nn.ModuleList(
            nn.Conv2d(d, d2, 2, 2) for d, d2 in zip(dims[:3], dims[1:]))
        self.head_norm = nn.LayerNorm(dims[3], eps=1e-6)
        self.fc = nn.Linear(dims[3], num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.stem_norm(self.stem(x))
        for i, stage in enumerate(self.stages):
            if i:
                x = self.down_convs[i - 1](self.down_norms[i - 1](x))
            x = stage(x)
        return self.fc(self.head_norm(x.mean(dim=(2, 3))))


def convnext_tiny(num_classes: int = 1000) -> ConvNeXt:
    return ConvNeXt((3, 3, 9, 3), (96, 192, 384, 768), num_classes)


def convnext_small(num_classes: int = 1000) -> ConvNeXt:
    return ConvNeXt((3, 3, 27, 3), (96, 192, 384, 768), num_classes)


# ConvNeXt V2: name -> (depths, dims).  Atto (dims 40, 80, 160, 320) is left
# out: the native patch stem needs out_channels % 16 == 0.
CONVNEXTV2 = {
    "femto": ((2, 2, 6, 2), (48, 96, 192, 384)),
    "pico": ((2, 2, 6, 2), (64, 128, 256, 512)),
    "nano": ((2, 2, 8, 2), (80, 160, 320, 640)),
    "tiny": ((3, 3, 9, 3), (96, 192, 384, 768)),
    "base": ((3, 3, 27, 3), (128, 256, 512, 1024)),
}


def convnextv2(name: str, num_classes: int = 1000) -> ConvNeXt:
    depths, dims = CONVNEXTV2[name]
    return ConvNeXt(depths, dims, num_classes, block=ConvNeXtV2Block)
