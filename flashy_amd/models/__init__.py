# Copyright (c) Flashy-AMD authors.
"""Model zoo for the example workloads and benchmarks.

The reference has no model zoo (it borrows torchvision's resnet18,
/root/reference/examples/cifar/train.py:43); torchvision is not a dependency
here, so the architectures the benchmark configs name are implemented
in-house: ResNet-18/50 (CIFAR and ImageNet stems) and the DCGAN-style 64x64
generator/discriminator pair used by the adversarial workload.

ConvNeXt comes as a torch twin and a native network: ``ConvNeXt`` /
``NativeConvNeXt`` with ``convnext_tiny`` / ``convnext_small`` and
``native_convnext_tiny`` / ``native_convnext_small`` (depths (3, 3, 9, 3) /
(3, 3, 27, 3), dims (96, 192, 384, 768)).  The native classes take
``dense_only=False`` for widths off the 64 grid, which the pointwise conv
kernels serve; the native constructors pass it.

ConvNeXt V2 is the same pair of networks built from ``ConvNeXtV2Block`` /
``NativeConvNeXtV2Block`` (no layer scale, a global response normalization
behind the GELU): ``convnextv2(name)`` and ``native_convnextv2_femto`` /
``_pico`` / ``_nano`` / ``_tiny`` / ``_base``.
"""
from .resnet import (ResNet, resnet18, resnet50,  # noqa: F401
                     resnext50_32x4d)
from .resnet_native import (NativeResNet, native_resnet18,  # noqa: F401
                            native_resnet50, native_resnext50_32x4d)
from .convnext import (ConvNeXt, ConvNeXtBlock,  # noqa: F401
                       ConvNeXtV2Block, convnext_small, convnext_tiny,
                       convnextv2)
from .convnext_native import (NativeConvNeXt,  # noqa: F401
                              NativeConvNeXtBlock, NativeConvNeXtV2Block,
                              native_convnext_small, native_convnext_tiny,
                              native_convnextv2_base, native_convnextv2_femto,
                              native_convnextv2_nano, native_convnextv2_pico,
                              native_convnextv2_tiny)
from .dcgan import DCGANGenerator, DCGANDiscriminator  # noqa: F401
from .dcgan_native import (NativeDCGANGenerator,  # noqa: F401
                           NativeDCGANDiscriminator)
