# Copyright (c) Flashy-AMD authors.
"""ConvNeXt block on the native NHWC kernels (flashy_amd.nn): depthwise 7x7
(csrc/conv_depthwise.hip), the dense MFMA path for the two 1x1 convs, and the
row kernels of csrc/layernorm.hip for everything between the GEMMs.  Forward
is five launches around the two GEMMs' own: depthwise conv, LayerNorm (which
folds the conv's bias in), bias + GELU, layer scale + bias + residual.
GPU-only.

``from_torch`` copies weights from the torch twin (for numerics tests):
depthwise [C,1,k,k] -> [C,k,k,1], Linear [O,I] -> 1x1 conv [O,1,1,I].
"""
from __future__ import annotations

import torch
from torch import nn

from .. import nn as fnn
from .convnext import ConvNeXtBlock


class NativeConvNeXtBlock(nn.Module):
    """NHWC bf16 in and out.  ``dim % 64 == 0``: the dense 1x1 path needs
    K % 64 forward and C % 64 in backward-data."""

    def __init__(self, dim: int, kernel_size: int = 7,
                 layer_scale_init: float = 1e-6):
        super().__init__()
        if dim < 64 or dim % 64:
            raise ValueError(
                f"NativeConvNeXtBlock needs dim % 64 == 0 (the dense 1x1 conv "
                f"kernels), got {dim}")
        k = kernel_size
        self.dwconv = fnn.Conv2d(dim, dim, k, 1, k // 2, groups=dim)
        self.dwconv_bias = nn.Parameter(torch.zeros(dim))
        self.norm = fnn.LayerNorm2d(dim, eps=1e-6)
        self.pwconv1 = fnn.Conv2d(dim, 4 * dim, 1)
        self.pwconv1_bias = nn.Parameter(torch.zeros(4 * dim))
        self.pwconv2 = fnn.Conv2d(4 * dim, dim, 1)
        self.pwconv2_bias = nn.Parameter(torch.zeros(dim))
        self.gamma = nn.Parameter(layer_scale_init * torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.norm(self.dwconv(x), self.dwconv_bias)
        g = fnn.bias_gelu(self.pwconv1(y), self.pwconv1_bias)
        return fnn.scale_residual(self.pwconv2(g), self.pwconv2_bias,
                                  self.gamma, x)

    @classmethod
    @torch.no_grad()
    def from_torch(cls, twin: ConvNeXtBlock) -> "NativeConvNeXtBlock":
        dim = twin.gamma.numel()
        block = cls(dim, twin.dwconv.kernel_size[0])
        block.dwconv.weight.copy_(twin.dwconv.weight.permute(0, 2, 3, 1))
        block.dwconv_bias.copy_(twin.dwconv.bias)
        block.norm.weight.copy_(twin.norm.weight)
        block.norm.bias.copy_(twin.norm.bias)
        block.pwconv1.weight.copy_(twin.pwconv1.weight.view(4 * dim, 1, 1, dim))
        block.pwconv1_bias.copy_(twin.pwconv1.bias)
        block.pwconv2.weight.copy_(twin.pwconv2.weight.view(dim, 1, 1, 4 * dim))
        block.pwconv2_bias.copy_(twin.pwconv2.bias)
        block.gamma.copy_(twin.gamma)
        return block
