# Copyright (c) Flashy-AMD authors.
"""Pointwise convolution (csrc/conv_point.hip), its fnn.Conv2d route and the
native ConvNeXt at widths off the 64 grid, against float64 CPU references
built from the bf16-rounded inputs (F.conv2d in double).

Forward / backward-data: max |got - ref| / max |ref| < 2^-8, the bound of
tests/test_patchconv_gpu.py.  Weight gradient, elementwise: |got - (pre + ref)|
<= 4 M 2^-24 S + 2^-23 |pre + ref| with S = sum |dy| |x| and M = N Ho Wo.
Outputs are NaN-filled before every launch, so an unwritten element shows.
"""
import copy
import functools
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -8

# (N, H, W, C, p, K): one row, reduction 8 padded to 32, half a column tile;
# the minimum at p = 2; both widths off the 16 / 32 grids, twice; ConvNeXt-T's
# MLP with M = 70, a ragged second tile that crosses an image boundary; the
# same with the widths swapped (two reduction chunks of 256 and 128); the
# downsample with odd H and W and two column panels in both directions; a
# reduction of five LDS chunks whose last one holds 8 live elements; three
# column panels, the last partial (and the five-chunk reduction in
# backward-data); M = 65 536: the grid of 512 blocks wraps and the weight
# gradient sums 512 slices.  The sizes are the issue's own: the chunk of 256
# and the panel limit of 384 columns leave every edge where it was aimed.
SHAPES = [(1, 1, 1, 8, 1, 8), (1, 2, 2, 8, 2, 8), (1, 3, 3, 24, 1, 40),
          (1, 4, 4, 40, 1, 24), (2, 5, 7, 96, 1, 384), (2, 5, 7, 384, 1, 96),
          (2, 7, 9, 96, 2, 192), (1, 4, 4, 1032, 1, 72),
          (1, 4, 4, 72, 1, 1032), (16, 64, 64, 24, 1, 40)]
MODULE = [(2, 5, 7, 96, 1, 384), (2, 5, 7, 384, 1, 96), (2, 7, 9, 96, 2, 192)]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (bf16, on the device) and float64 references of one conv."""
    from flashy_amd import ops
    N, H, W, C, p, K = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(K, p, p, C, generator=g) * 0.2).to(torch.bfloat16)
    d = ops.ConvDims(N, H, W, C, K, p, p, H // p, W // p, p, 0)
    dy = torch.randn(N, d.Ho, d.Wo, K, generator=g).to(torch.bfloat16)
    pre = torch.randn(K, p, p, C, generator=g)

    def conv(xx, ww):
        return F.conv2d(xx.permute(0, 3, 1, 2), ww.permute(0, 3, 1, 2),
                        stride=p)

    xd = x.double().requires_grad_()
    wd = w.double().requires_grad_()
    y = conv(xd, wd)
    gy = dy.double().permute(0, 3, 1, 2)
    dx, dw = torch.autograd.grad(y, (xd, wd), gy)
    wa = w.double().abs().requires_grad_()
    (S,) = torch.autograd.grad(conv(x.double().abs(), wa), wa, gy.abs())
    return dict(d=d, x=x.cuda(), w=w.cuda(), dy=dy.cuda(), pre=pre,
                y=y.detach().permute(0, 2, 3, 1).contiguous(), dx=dx, dw=dw,
                S=S)


def _rel(got, ref):
    assert not torch.isnan(got).any(), "an element was not written"
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _nan(shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fwd_and_dgrad(shape):
    from flashy_amd import ops
    c = _case(shape)
    d = c["d"]
    y = _nan((d.N, d.Ho, d.Wo, d.K))
    ops.pwconv_fwd(c["x"], c["w"], y, d)
    dx = _nan((d.N, d.H, d.W, d.C))
    ops.pwconv_dgrad(c["dy"], c["w"], dx, d)
    ey, ex = _rel(y, c["y"]), _rel(dx, c["dx"])
    print(f"fwd {ey:.3e} dgrad {ex:.3e} bound {BOUND:.3e}")
    assert ey < BOUND and ex < BOUND, (ey, ex)
    # what no patch covers (H % p rows, W % p columns) is exactly zero
    assert (dx[:, d.Ho * d.R:] == 0).all() and (dx[:, :, d.Wo * d.R:] == 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_accumulates(shape):
    from flashy_amd import ops
    c = _case(shape)
    d = c["d"]
    runs = []
    for _ in range(2):
        dw = c["pre"].cuda()
        ops.pwconv_wgrad(c["x"], c["dy"], dw, d)
        runs.append(dw)
    want = c["pre"].double() + c["dw"]
    M = d.N * d.Ho * d.Wo
    tol = 4 * M * 2.0 ** -24 * c["S"] + 2.0 ** -23 * want.abs()
    err = (runs[0].double().cpu() - want).abs()
    print(f"wgrad worst err/tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), (err / tol).max().item()
    assert torch.equal(runs[0], runs[1]), "wgrad is not bitwise repeatable"


@pytest.mark.parametrize("shape", MODULE, ids=lambda s: "x".join(map(str, s)))
def test_module_autograd(shape):
    from flashy_amd import nn as fnn
    c = _case(shape)
    d = c["d"]
    conv = fnn.Conv2d(d.C, d.K, d.R, d.stride, 0).cuda()
    assert conv.pointwise
    with torch.no_grad():
        conv.weight.copy_(c["w"].float())
    x = c["x"].clone().requires_grad_()
    y = conv(x)
    y.backward(c["dy"])
    ey, ex = _rel(y, c["y"]), _rel(x.grad, c["dx"])
    print(f"fwd {ey:.3e} dgrad {ex:.3e} bound {BOUND:.3e}")
    assert ey < BOUND and ex < BOUND, (ey, ex)
    M = d.N * d.Ho * d.Wo
    tol = 4 * M * 2.0 ** -24 * c["S"] + 2.0 ** -23 * c["dw"].abs()
    err = (conv.weight.grad.double().cpu() - c["dw"]).abs()
    print(f"wgrad worst err/tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), (err / tol).max().item()
    frozen = fnn.Conv2d(d.C, d.K, d.R, d.stride, 0).cuda()
    frozen.weight.requires_grad_(False)
    x2 = c["x"].clone().requires_grad_()
    frozen(x2).backward(c["dy"])
    assert frozen.weight.grad is None and x2.grad is not None


def test_grid_widths_keep_their_route():
    from flashy_amd import nn as fnn
    assert not fnn.Conv2d(64, 128, 1).pointwise
    assert not fnn.Conv2d(128, 256, 2, 2).pointwise


@pytest.mark.parametrize("whole", [False, True], ids=["block", "network"])
def test_convnext_off_grid(whole):
    """Native block (dim 96) and network (ConvNeXt-T's widths) against the
    float64 twin; the permitted error of each quantity is twice that of the
    same twin run on the CPU in bf16 (tests/test_patchconv_gpu.py)."""
    from flashy_amd.models import (ConvNeXt, ConvNeXtBlock, NativeConvNeXt,
                                   NativeConvNeXtBlock)
    torch.manual_seed(96 + whole)
    twin = ConvNeXt((1, 1, 1, 1), (96, 192, 384, 768), 10) if whole \
        else ConvNeXtBlock(96)
    with torch.no_grad():
        for name, p in twin.named_parameters():
            if "norm" in name and name.endswith("weight"):
                p.add_(0.5 * torch.randn_like(p))
            elif "norm" in name or name.endswith("gamma"):
                p.copy_(torch.randn_like(p) * (0.5 if "norm" in name else 1))
    x = torch.randn((2, 64, 64, 3) if whole else (2, 8, 8, 96))
    x = x.to(torch.bfloat16).requires_grad_(not whole)
    dy = torch.randn(2, 10) if whole else \
        torch.randn(2, 8, 8, 96).to(torch.bfloat16)

    def run_twin(dtype):
        m = copy.deepcopy(twin).to(dtype)
        xin = x.detach().to(dtype).requires_grad_(not whole)
        out = m(xin.permute(0, 3, 1, 2))
        out = out if whole else out.permute(0, 2, 3, 1)
        out.backward(dy.to(dtype))
        q = {"out": out.detach()}
        if not whole:
            q["x"] = xin.grad
        q.update({k: p.grad for k, p in m.named_parameters()})
        return q

    ref, low = run_twin(torch.float64), run_twin(torch.bfloat16)
    net = (NativeConvNeXt if whole else NativeConvNeXtBlock).from_torch(
        twin).cuda()
    xg = x.detach().cuda().requires_grad_(not whole)
    out = net(xg)
    out.backward(dy.cuda())
    ours = dict(net.named_parameters())
    for k in ref:
        if k in ("out", "x"):
            got = out.detach() if k == "out" else xg.grad
        else:
            name = re.sub(r"down_convs\.(\d)\.bias", r"down_biases.\1", k)
            got = ours[name if name in ours
                       else name.replace(".bias", "_bias")].grad
            if got.dim() == 4 and ref[k].dim() == 4:    # KRSC -> KCRS
                got = got.permute(0, 3, 1, 2)
        e_native = _rel(got.reshape(ref[k].shape), ref[k])
        e_bf16 = _rel(low[k], ref[k])
        print(f"{k}: native {e_native:.3e} bf16 twin {e_bf16:.3e}")
        assert e_native <= 2 * e_bf16, (k, e_native, e_bf16)
