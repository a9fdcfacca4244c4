# Copyright (c) Flashy-AMD authors.
"""What the LayerNorm / bias+GELU / scale+residual wrappers and the native
ConvNeXt block refuse, they refuse before the extension is loaded."""
import pytest
import torch

from flashy_amd import ops


def _act(C, dtype=torch.bfloat16):
    return torch.zeros(4, C, dtype=dtype)


def _calls(x, C):
    """Every wrapper on activations like ``x`` with [C] parameters."""
    p, stats = torch.zeros(C), torch.zeros(4, 2)
    return {
        "ln_fwd": lambda: ops.ln_fwd(x, p, p, x, stats, 1e-6),
        "ln_bwd": lambda: ops.ln_bwd(x, x, stats, p, x, p, p),
        "bias_gelu_fwd": lambda: ops.bias_gelu_fwd(x, p, x),
        "bias_gelu_bwd": lambda: ops.bias_gelu_bwd(x, x, p, x, p),
        "scale_residual_fwd": lambda: ops.scale_residual_fwd(x, p, p, x, x),
        "scale_residual_bwd":
            lambda: ops.scale_residual_bwd(x, x, p, p, x, p, p),
    }


@pytest.mark.parametrize("name", sorted(_calls(_act(8), 8)))
def test_wrappers_refuse_before_touching_the_extension(monkeypatch, name):
    def no_ext():
        raise AssertionError("extension reached")

    monkeypatch.setattr(ops, "require", no_ext)
    widths = (12, 1032) if name.startswith("ln_") else (12,)
    for C in widths:
        with pytest.raises(ValueError, match="channel LayerNorm needs"):
            _calls(_act(C), C)[name]()
    with pytest.raises(AssertionError, match="contiguous"):
        _calls(_act(32)[:, ::2], 16)[name]()
    with pytest.raises(AssertionError, match="bf16"):
        _calls(_act(16, torch.float32), 16)[name]()


def test_block_refuses_widths_the_dense_path_cannot_serve():
    from flashy_amd.models import NativeConvNeXtBlock
    with pytest.raises(ValueError, match="dim % 64"):
        NativeConvNeXtBlock(96)
