# Copyright (c) Flashy-AMD authors.
"""ConvNeXt block (Liu et al., "A ConvNet for the 2020s"), plain torch: the
twin of :mod:`flashy_amd.models.convnext_native`, as resnet.py is of
resnet_native.py.  Only the block: see TODO.md for the rest of the network.
"""
from __future__ import annotations

import torch
from torch import nn


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
