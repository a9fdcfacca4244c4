# Copyright (c) Flashy-AMD authors.
"""What the global response normalization wrappers and the ConvNeXt V2
constructors refuse, they refuse before a kernel is reached."""
import pytest
import torch

from flashy_amd import ops


def _calls(x, C, ws_rows=8):
    """Every wrapper on activations like ``x`` ([2, 4, C]) with [C]
    parameters and a workspace of ``ws_rows`` [C] rows."""
    p, coef, rden = torch.zeros(C), torch.zeros(2, C), torch.zeros(2)
    ws = torch.zeros(ws_rows, C)
    return {
        "grn_sqsum": lambda: ops.grn_sqsum(x, ws),
        "bias_gelu_sqsum": lambda: ops.bias_gelu_sqsum(x, p, x, ws),
        "grn_fwd": lambda: ops.grn_fwd(x, p, p, x, coef, coef, rden, 1e-6, ws),
        "grn_bwd": lambda: ops.grn_bwd(x, x, coef, coef, rden, p, x, p, p),
    }


def _act(C, dtype=torch.bfloat16):
    return torch.zeros(2, 4, C, dtype=dtype)


@pytest.mark.parametrize("name", sorted(_calls(_act(8), 8)))
def test_wrappers_refuse_before_touching_the_extension(monkeypatch, name):
    def no_ext():
        raise AssertionError("extension reached")

    monkeypatch.setattr(ops, "require", no_ext)
    for C in (12, 4104):
        with pytest.raises(ValueError, match="global response normalization"):
            _calls(_act(C), C)[name]()
    with pytest.raises(AssertionError, match="contiguous"):
        _calls(_act(32)[:, :, ::2], 16)[name]()
    with pytest.raises(AssertionError, match="bf16"):
        _calls(_act(16, torch.float32), 16)[name]()
    if name != "grn_bwd":       # it sizes its own workspace
        monkeypatch.setattr(ops, "grn_plan", lambda N, HW, C: ops.GrnPlan(
            1, 2, 128, 4, 1, (4, N, 1)))
        with pytest.raises(AssertionError, match="workspace"):
            _calls(_act(16), 16, ws_rows=7)[name]()
        with pytest.raises(AssertionError, match="one GPU"):
            _calls(_act(16), 16, ws_rows=8)[name]()


def test_v2_constructors():
    from flashy_amd import models, nn as fnn
    with pytest.raises(ValueError, match="out_channels % 16"):      # Atto
        models.NativeConvNeXt((2, 2, 6, 2), (40, 80, 160, 320), 10,
                              dense_only=False,
                              block=models.NativeConvNeXtV2Block)
    with pytest.raises(ValueError, match="dim % 64"):
        models.NativeConvNeXtV2Block(96)
    with pytest.raises(ValueError, match="global response normalization"):
        fnn.GRN(4100)
    net = models.native_convnextv2_femto(10)
    assert isinstance(net.stages[2][5], models.NativeConvNeXtV2Block)
    assert net.stages[0][0].grn.weight.abs().sum() == 0
    assert "ones" not in net.state_dict()
    assert isinstance(models.native_convnext_tiny(10).stages[0][0],
                      models.NativeConvNeXtBlock)
