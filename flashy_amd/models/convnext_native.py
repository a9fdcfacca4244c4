# Copyright (c) Flashy-AMD authors.
"""ConvNeXt block on the native NHWC kernels (flashy_amd.nn): depthwise 7x7
(csrc/conv_depthwise.hip), the dense MFMA path for the two 1x1 convs (the
pointwise kernels of csrc/conv_point.hip at widths off the 64 grid), and the
row kernels of csrc/layernorm.hip for everything between the GEMMs.  Forward
is five launches around the two GEMMs' own: depthwise conv, LayerNorm (which
folds the conv's bias in), bias + GELU, layer scale + bias + residual.
GPU-only.

ConvNeXt V2 (:class:`NativeConvNeXtV2Block`) drops the layer scale and puts
a global response normalization (csrc/grn.hip) behind the GELU, whose walk
gathers GRN's sums of squares: :func:`flashy_amd.nn.bias_gelu_grn`.

``from_torch`` copies weights from the torch twin (for numerics tests):
depthwise [C,1,k,k] -> [C,k,k,1], Linear [O,I] -> 1x1 conv [O,1,1,I].
"""
from __future__ import annotations

import typing as tp

import torch
from torch import nn

from .. import nn as fnn
from .convnext import CONVNEXTV2, ConvNeXt, ConvNeXtBlock, ConvNeXtV2Block


class NativeConvNeXtBlock(nn.Module):
    """NHWC bf16 in and out.  By default ``dim % 64 == 0`` and the 1x1 convs
    ride the dense 8-wave kernels; ``dense_only=False`` admits every
    ``dim % 8 == 0`` up to LayerNorm's 1024 and routes the widths off the 64
    grid to the pointwise kernels (:class:`flashy_amd.nn.Conv2d`)."""

    def __init__(self, dim: int, kernel_size: int = 7,
                 layer_scale_init: float = 1e-6, dense_only: bool = True):
        super().__init__()
        if dense_only and (dim < 64 or dim % 64):
            raise ValueError(
                f"NativeConvNeXtBlock needs dim % 64 == 0 (the dense 1x1 conv "
                f"kernels; dense_only=False admits dim % 8 == 0), got {dim}")
        if dim < 8 or dim % 8 or dim > 1024:
            raise ValueError(
                f"NativeConvNeXtBlock needs dim % 8 == 0 and 8 <= dim <= 1024, "
                f"got {dim}")
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
        block = cls(dim, twin.dwconv.kernel_size[0], dense_only=dim % 64 == 0)
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


class NativeConvNeXtV2Block(nn.Module):
    """ConvNeXt V2's block, NHWC bf16 in and out: depthwise conv ->
    LayerNorm2d (the conv's bias folded in) -> pwconv1 -> bias + GELU + GRN
    (:func:`flashy_amd.nn.bias_gelu_grn`) -> pwconv2 -> bias + residual.
    There is no layer scale: :func:`flashy_amd.nn.scale_residual` gets a
    frozen buffer of ones.  ``dense_only`` as in :class:`NativeConvNeXtBlock`.
    """

    def __init__(self, dim: int, kernel_size: int = 7,
                 dense_only: bool = True):
        super().__init__()
        if dense_only and (dim < 64 or dim % 64):
            raise ValueError(
                f"NativeConvNeXtV2Block needs dim % 64 == 0 (the dense 1x1 "
                f"conv kernels; dense_only=False admits dim % 8 == 0), got "
                f"{dim}")
        if dim < 8 or dim % 8 or dim > 1024:
            raise ValueError(
                f"NativeConvNeXtV2Block needs dim % 8 == 0 and 8 <= dim <= "
                f"1024, got {dim}")
        k = kernel_size
        self.dwconv = fnn.Conv2d(dim, dim, k, 1, k // 2, groups=dim)
        self.dwconv_bias = nn.Parameter(torch.zeros(dim))
        self.norm = fnn.LayerNorm2d(dim, eps=1e-6)
        self.pwconv1 = fnn.Conv2d(dim, 4 * dim, 1)
        self.pwconv1_bias = nn.Parameter(torch.zeros(4 * dim))
        self.grn = fnn.GRN(4 * dim, eps=1e-6)
        self.pwconv2 = fnn.Conv2d(4 * dim, dim, 1)
        self.pwconv2_bias = nn.Parameter(torch.zeros(dim))
        self.register_buffer("ones", torch.ones(dim), persistent=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.norm(self.dwconv(x), self.dwconv_bias)
        g = fnn.bias_gelu_grn(self.pwconv1(y), self.pwconv1_bias, self.grn)
        return fnn.scale_residual(self.pwconv2(g), self.pwconv2_bias,
                                  self.ones, x)

    @classmethod
    @torch.no_grad()
    def from_torch(cls, twin: ConvNeXtV2Block) -> "NativeConvNeXtV2Block":
        dim = twin.norm.weight.numel()
        block = cls(dim, twin.dwconv.kernel_size[0], dense_only=dim % 64 == 0)
        block.dwconv.weight.copy_(twin.dwconv.weight.permute(0, 2, 3, 1))
        block.dwconv_bias.copy_(twin.dwconv.bias)
        for mine, theirs in [(block.norm, twin.norm), (block.grn, twin.grn)]:
            mine.weight.copy_(theirs.weight)
            mine.bias.copy_(theirs.bias)
        block.pwconv1.weight.copy_(twin.pwconv1.weight.view(4 * dim, 1, 1, dim))
        block.pwconv1_bias.copy_(twin.pwconv1.bias)
        block.pwconv2.weight.copy_(twin.pwconv2.weight.view(dim, 1, 1, 4 * dim))
        block.pwconv2_bias.copy_(twin.pwconv2.bias)
        return block


class NativeConvNeXt(nn.Module):
    """The whole network, NHWC bf16 ``[N, H, W, in_chans]`` in, fp32 logits
    out.  Stem: the patch conv kernels (csrc/conv_patch.hip), its bias folded
    into the LayerNorm behind it.  Downsample: LayerNorm, the dense 2x2
    stride-2 conv, :func:`flashy_amd.nn.bias_add`.  Head: the pooling
    kernels, LayerNorm on ``[N, 1, 1, C]``, :class:`flashy_amd.nn.Linear`.
    Every ``dims[i] % 64 == 0`` by default; ``dense_only=False`` admits
    ``dims[i] % 8 == 0`` up to 1024 (ConvNeXt-T / -S: 96, 192, 384, 768), as
    the block does, with ``dims[0]`` within the patch stem's rule.  ``block``
    is the block class: :class:`NativeConvNeXtV2Block` makes it ConvNeXt V2.
    """

    def __init__(self, depths: tp.Sequence[int], dims: tp.Sequence[int],
                 num_classes: int, patch: int = 4, in_chans: int = 3,
                 dense_only: bool = True,
                 block: tp.Type[nn.Module] = NativeConvNeXtBlock):
        super().__init__()
        if len(depths) != 4 or len(dims) != 4 or \
                (dense_only and any(d < 64 or d % 64 for d in dims)):
            raise ValueError(
                f"NativeConvNeXt needs four stages with dims % 64 == 0 (the "
                f"dense conv kernels; dense_only=False admits dims % 8 == 0), "
                f"got depths={depths} dims={dims}")
        if any(d < 8 or d % 8 or d > 1024 for d in dims):
            raise ValueError(
                f"NativeConvNeXt needs dims % 8 == 0 and 8 <= dims <= 1024, "
                f"got dims={dims}")
        self.stem = fnn.Conv2d(in_chans, dims[0], patch, patch, 0,
                               input_grad=False)
        if not self.stem.patch:
            raise ValueError(
                f"NativeConvNeXt stem: {fnn.ops.PATCHCONV_RULE}; got "
                f"patch={patch} in_chans={in_chans} dims[0]={dims[0]}")
        self.stem_bias = nn.Parameter(torch.zeros(dims[0]))
        self.stem_norm = fnn.LayerNorm2d(dims[0], eps=1e-6)
        self.stages = nn.ModuleList(
            nn.Sequential(*[block(d, dense_only=dense_only)
                            for _ in range(n)])
            for n, d in zip(depths, dims))
        self.down_norms = nn.ModuleList(
            fnn.LayerNorm2d(d, eps=1e-6) for d in dims[:3])
        self.down_convs = nn.ModuleList(
            fnn.Conv2d(d, d2, 2, 2, 0) for d, d2 in zip(dims[:3], dims[1:]))
        self.down_biases = nn.ParameterList(
            nn.Parameter(torch.zeros(d2)) for d2 in dims[1:])
        self.head_norm = fnn.LayerNorm2d(dims[3], eps=1e-6)
        self.fc = fnn.Linear(dims[3], num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.stem_norm(self.stem(x), self.stem_bias)
        for i, stage in enumerate(self.stages):
            if i:
                x = fnn.bias_add(self.down_convs[i - 1](self.down_norms[i - 1](x)),
                                 self.down_biases[i - 1])
            x = stage(x)
        pooled = fnn.global_avg_pool(x)                     # fp32 [N, C]
        n, c = pooled.shape
        y = self.head_norm(pooled.to(torch.bfloat16).view(n, 1, 1, c))
        return self.fc(y.view(n, c).float())

    @classmethod
    @torch.no_grad()
    def from_torch(cls, twin: ConvNeXt) -> "NativeConvNeXt":
        depths = [len(s) for s in twin.stages]
        dims = [c.out_channels for c in [twin.stem, *twin.down_convs]]
        v2 = any(isinstance(b, ConvNeXtV2Block) for s in twin.stages for b in s)
        block = NativeConvNeXtV2Block if v2 else NativeConvNeXtBlock
        net = cls(depths, dims, twin.fc.out_features,
                  twin.stem.kernel_size[0], twin.stem.in_channels,
                  dense_only=all(d % 64 == 0 for d in dims), block=block)
        net.stem.weight.copy_(twin.stem.weight.permute(0, 2, 3, 1))
        net.stem_bias.copy_(twin.stem.bias)
        for mine, theirs in [(net.stem_norm, twin.stem_norm),
                             (net.head_norm, twin.head_norm),
                             (net.fc, twin.fc),
                             *zip(net.down_norms, twin.down_norms)]:
            mine.weight.copy_(theirs.weight)
            mine.bias.copy_(theirs.bias)
        for conv, bias, theirs in zip(net.down_convs, net.down_biases,
                                      twin.down_convs):
            conv.weight.copy_(theirs.weight.permute(0, 2, 3, 1))
            bias.copy_(theirs.bias)
        net.stages = nn.ModuleList(
            nn.Sequential(*[block.from_torch(b) for b in s])
            for s in twin.stages)
        return net


def native_convnext_tiny(num_classes: int = 10) -> NativeConvNeXt:
    return NativeConvNeXt((3, 3, 9, 3), (96, 192, 384, 768), num_classes,
                          dense_only=False)


def native_convnext_small(num_classes: int = 10) -> NativeConvNeXt:
    return NativeConvNeXt((3, 3, 27, 3), (96, 192, 384, 768), num_classes,
                          dense_only=False)


def _native_convnextv2(name: str, num_classes: int) -> NativeConvNeXt:
    depths, dims = CONVNEXTV2[name]
    return NativeConvNeXt(depths, dims, num_classes, dense_only=False,
                          block=NativeConvNeXtV2Block)


def native_convnextv2_femto(num_classes: int = 10) -> NativeConvNeXt:
    """ConvNeXt V2 Femto.  The family's Atto (dims 40, 80, 160, 320) has no
    constructor: the patch stem needs ``out_channels % 16 == 0``."""
    return _native_convnextv2("femto", num_classes)


def native_convnextv2_pico(num_classes: int = 10) -> NativeConvNeXt:
    return _native_convnextv2("pico", num_classes)


def native_convnextv2_nano(num_classes: int = 10) -> NativeConvNeXt:
    return _native_convnextv2("nano", num_classes)


def native_convnextv2_tiny(num_classes: int = 10) -> NativeConvNeXt:
    return _native_convnextv2("tiny", num_classes)


def native_convnextv2_base(num_classes: int = 10) -> NativeConvNeXt:
    return _native_convnextv2("base", num_classes)
